"""Which kernel paths a system REACHES, from the host alone (get_symbolic / get_launch_plan: no device).  A test that names a path -- the 128 x 128
trailing update, the XCD tile tables, the fused pivot-block + panel-solve launch ... -- shows with these facts that its fixture runs it: a later change
of the ordering or of a threshold then fails a CPU test instead of silently emptying a GPU one.

reach(solver) is evaluated under the MI355X_KKT_DISABLE / MI355X_KKT_TUNE settings of the moment (the plan is rebuilt from the environment at every
query), so one analysed handle gives the facts of both legs of an A/B test.  Every fact is a count (0 = not reached)."""
import numpy as np

FC_WAVE, FC_LDS64, FC_LDS128, FC_BIG, FC_COUNT = 0, 1, 2, 3, 4
BIT_TFUSE, BIT_SELFASM, BIT_SOLO, BIT_SPLIT, BIT_TTAB, BIT_TTAB2, BIT_ASMCUT, BIT_ASMFAST, BIT_ALIAS = (1 << i for i in range(9))
INPUTS = ["chain_solve", "fuse_dt", "fastpiv", "asm_pull", "leafchain", "front_df", "tfuse", "fuse_upd", "selfasm", "grouped", "xcd_tiles", "lookahead",
          "pair_solve", "p1_small", "la_wgs", "la_min_nt", "grp_rbw_max", "chain_solve_maxc", "fuse_dt_maxwg", "la_min_tiles"]
PLAN_ARRAYS = ["scalars", "path_scalars", "inputs", "level_list", "path_bits", "asm_fast_ok", "asmcut", "levels", "groups", "tiny16", "tiny_split", "mid_split",
               "big_split", "lc_ptr", "lc_fronts", "df_runs", "chain_segs", "chain_links", "chain_descs", "single.ptr", "single.maxm", "single.maxk",
               "single.last0", "single.last1", "single.allsolo"]


def plan_arrays(s):
    """every exported array of the single-GPU plan under the settings of the moment"""
    return {w: s.launch_plan(w).copy() for w in PLAN_ARRAYS}


def plan_diff(a, b):
    """names of the arrays in which two plans differ"""
    return sorted(w for w in PLAN_ARRAYS if not np.array_equal(a[w], b[w]))


def reach(s):
    I = s.info()
    nl, nsn = I.num_levels, I.num_sn
    order = np.diff(s.symbolic(2, nsn + 1)); cols = np.diff(s.symbolic(1, nsn + 1))
    parent, cls = s.symbolic(4, nsn), s.symbolic(23, nsn)
    grp_rem, alias = s.symbolic(16, nsn), s.symbolic(17, nsn)
    lp = s.symbolic(13, nl * FC_COUNT + 1)
    nchild = np.bincount(parent[parent >= 0], minlength=nsn)
    A = plan_arrays(s)
    L, bits, fast_ok, asmcut = A["level_list"], A["path_bits"], A["asm_fast_ok"], A["asmcut"]
    scal, ps = A["scalars"], A["path_scalars"]
    inp = dict(zip(INPUTS, (int(x) for x in A["inputs"])))
    lev = A["levels"].reshape(-1, 10); grp = A["groups"].reshape(-1, 11)
    la_tiles2, asm_skip, narrow = lev[:, 1], lev[:, 3], lev[:, 4]
    part0, part1, wave_mmax, wave_kmax = lev[:, 5], lev[:, 6], lev[:, 8], lev[:, 9]
    maxm, maxk = A["single.maxm"], A["single.maxk"]
    pair_solve, la_any, ttab_len, grp_cut = int(ps[0]), int(ps[1]), int(ps[2]), int(ps[3])
    lc_levels, grouped = int(scal[2]), int(scal[5])
    big = cls == FC_BIG
    upd = order - cols
    sb = bits[:nsn]                                       # the single-GPU buckets are the leading part of the launch list
    bigq = big[L[:nsn]]
    F = {}
    F["max_order"] = int(order.max())
    F["big_orders"] = sorted(int(x) for x in order[big])
    F["orders_over_1024"] = int(np.sum(order[big] > 1024))
    F["orders_le_1024_big"] = int(np.sum(order[big] <= 1024))
    F["tile_rows_ge_12"] = int(np.sum(big & (grp_rem == 0) & ((upd + 127) // 128 >= 12)))
    F["xcd_tables"] = int(np.sum((sb & BIT_TTAB) != 0)); F["xcd_tables2"] = int(np.sum((sb & BIT_TTAB2) != 0)); F["tile_tab_len"] = ttab_len
    F["tiny_split"] = int(np.sum(A["tiny_split"] > 0)); F["mid_split"] = int(np.sum(A["mid_split"] > 0))
    F["lookahead"] = int(np.sum((sb & BIT_SPLIT) != 0)) if la_any else 0
    F["grouped"] = grouped; F["tfuse"] = int(np.sum((sb & BIT_TFUSE) != 0)); F["selfasm"] = int(np.sum(((sb & BIT_SELFASM) != 0) & bigq))
    F["asmcut"] = int(np.sum(asmcut[:nsn] > 0))
    F["df_run"] = len(A["df_runs"]) // 5; F["leaf_chain"] = lc_levels
    F["kk_over_64"] = int(np.sum(maxk > 64))
    F["pair_solve"] = pair_solve
    in_seg = np.zeros(nl, dtype=bool)
    for lv0, lv1, *_ in A["chain_segs"].reshape(-1, 9):
        in_seg[lv0:lv1 + 1] = True
    # numeric.hip solve_sweep: the leaf-chain prefix is walked by k_fwd_leafchain (pair_solve on, no data-flow segment inside it); solve_level takes the pair
    # kernels on every other level with one-wavefront fronts outside the segments
    lcs = lc_levels if (pair_solve and lc_levels > 0 and not in_seg[:lc_levels].any()) else 0
    F["leafchain_solve"] = lcs
    F["pair_levels"] = sum(1 for lv in range(lcs, nl) if pair_solve and not in_seg[lv] and lp[lv * FC_COUNT + 1] > lp[lv * FC_COUNT])
    F["pair16_levels"] = sum(1 for lv in range(lcs, nl) if pair_solve and not in_seg[lv] and lp[lv * FC_COUNT + 1] > lp[lv * FC_COUNT] and wave_mmax[lv] <= 16)
    fused = asm2 = narrow_fused = aff = grp_launch = schur128 = schur64 = asm_col = la_fork = p1_small = 0
    for lv in range(nl):
        b0, b1 = int(lp[lv * FC_COUNT + FC_BIG]), int(lp[lv * FC_COUNT + FC_BIG + 1])
        nball = b1 - b0
        if nball == 0:
            continue
        mm, kk = int(maxm[lv]), int(maxk[lv])
        if not asm_skip[lv]:
            # restates numeric.hip launch_assemble: `v2 = v2 && maxch * ldi * sizeof(int) <= 158 KiB && (nfronts >= 32 && maxch <= 6)` with v2 = every asm_fast_ok != 0
            ok = fast_ok[b0:b1]
            maxch, ldi = max(1, int(ok.max())), (mm + 15) & ~15
            if np.all(ok != 0) and maxch * ldi * 4 <= 158 * 1024 and nball >= 32 and maxch <= 6:
                asm2 += 1
            else:
                asm_col += 1
        if grouped and lv >= grp_cut:                       # launch_bucket: the chain groups whose first link sits here (launch_groups)
            g0, g1, gsplit = int(grp[lv, 0]), int(grp[lv, 1]), int(grp[lv, 2])
            if g1 > g0:
                grp_launch += 1
                if gsplit > 0 and grp[lv, 4] > 0:
                    schur64 += 1
                    aff += gsplit >= 16
                if g1 - g0 > gsplit:
                    schur128 += 1
                    if grp[lv, 7] > 0:                      # launch_groups `G.la2[lv] > 0`: part 1 on the main stream, part 2 forked to the second one
                        la_fork += 1
                        p1_small += bool(inp["p1_small"] and grp[lv, 6] * (g1 - g0 - gsplit) <= 512)      # (... `knobs.p1_small && G.la1[lv] * nb <= 512`: k_big_schur_p1)
            continue
        nrb = (mm + 63) // 64
        bs = int(A["big_split"][lv])
        # restates numeric.hip launch_big: `knobs.fuse_dt && (single || multi) && kk <= 64 && nball * (1 + nrb) <= knobs.fuse_dt_maxwg`
        if inp["fuse_dt"] and kk <= 64 and nball * (1 + nrb) <= inp["fuse_dt_maxwg"]:
            fused += 1
            if narrow[lv] > 0 and nball * (1 + nrb + int(narrow[lv])) <= 256:      # (... `ntu`: the narrow updates ride in that launch)
                narrow_fused += 1
                continue
        else:
            aff += nball >= 16                               # k_big_trsm over nball fronts (xcd_affine acts on >= 16 fronts)
        if bs > 0 and part0[lv] > 0:
            schur64 += 1
            aff += bs >= 16                                  # k_big_schur64 over bs fronts
        if nball > bs:
            schur128 += 1
            la_fork += bool(la_tiles2[lv] > 0)               # launch_big `single && P.la_tiles2[lv] > 0`
    F["fused_diag_trsm_level"] = fused; F["narrow_fused_level"] = narrow_fused; F["assemble2_level"] = asm2; F["assemble_column_level"] = asm_col
    # (the split bit alone launches nothing: only the 128 x 128 update of fronts above 1024 rows reads it)
    F["lookahead_fork_level"] = int(la_fork); F["p1_small_level"] = int(p1_small)
    F["xcd_affine_launch"] = int(aff); F["group_launch_level"] = grp_launch; F["schur128_level"] = schur128; F["schur64_level"] = schur64
    # k_big_assemble / k_big_assemble2 with V.asm_pull: the fronts that gather children's blocks (not in place on a child, not assembling themselves)
    F["asm_pull_fronts"] = int(np.sum(big & (alias < 0) & (nchild > 0))) if inp["asm_pull"] else 0
    F["asm_gather_fronts"] = int(np.sum(big & (alias < 0) & (nchild > 0)))
    # side stream (numeric.hip enqueue_factor `side`): look-ahead on, a bucket of <= 16 small fronts beside one eight times as large
    side = 0
    skipped = np.zeros(nl, dtype=bool)                     # levels the optimistic schedule hands to k_leaf_chain / k_front_df as a whole
    if inp["fastpiv"]:
        skipped[:lc_levels] = True
        for lv0, lv1, *_ in A["df_runs"].reshape(-1, 5):
            skipped[lv0:lv1 + 1] = True
    for lv in range(nl):
        if skipped[lv]:
            continue
        nbs = [int(lp[lv * FC_COUNT + fc + 1] - lp[lv * FC_COUNT + fc]) for fc in range(FC_COUNT)]
        for fc in range(FC_BIG):
            if la_any and 0 < nbs[fc] <= 16 and max(nbs) >= 8 * nbs[fc] and sum(nbs) > nbs[fc]:
                side += 1
    F["side_small_bucket"] = side
    # the optimistic schedule drops strict launches where the static-order kernels take a whole bucket, and runs the leaf chains / data-flow runs
    # k_front_reg<64, 2> (launch_bucket `nt > 0`): the strict launch over >= 2 048 fronts of order <= 16; the optimistic schedule leaves it out where the
    # static-order kernel has taken the whole bucket (`optimistic && n16 == nb`) and on the levels of the leaf chains and the data-flow runs
    wave_nb = np.array([lp[lv * FC_COUNT + 1] - lp[lv * FC_COUNT] for lv in range(nl)])
    F["reg2_level_strict"] = int(np.sum(A["tiny_split"] > 0))
    F["reg2_level_optimistic"] = int(np.sum((A["tiny_split"] > 0) & ~skipped & ~((A["tiny16"] == wave_nb) & bool(inp["fastpiv"]))))
    F["optimistic_only"] = (lc_levels if inp["fastpiv"] else 0) + F["df_run"]
    # fronts of order exactly 1024 and 1025 in ONE launch (the two sides of the big_split edge)
    level = s.symbolic(5, nsn)
    F["edge_1024_1025_level"] = len(set(level[big & (order == 1024)].tolist()) & set(level[big & (order == 1025)].tolist()))
    # big_diag_body `V.fastpiv && k <= 64`: pivot blocks of big fronts that try the blocked static-order LDL^T first
    F["fastpiv_big_blocks"] = int(np.sum(big & (cols <= 64))) if inp["fastpiv"] else 0
    F["maxsupernode"] = int(I.maxsupernode)
    F["inputs"] = inp
    return F
