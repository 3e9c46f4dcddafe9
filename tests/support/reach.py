"""Which kernel paths a system REACHES, from the host alone (get_symbolic / get_launch_plan: no device).  A test that names a path -- the 128 x 128
trailing update, the XCD tile tables, the fused pivot-block + panel-solve launch ... -- shows with these facts that its fixture runs it: a later change
of the ordering or of a threshold then fails a CPU test instead of silently emptying a GPU one.

What the FACTORISATION launches is counted, not restated: the exported factor schedules ("factor.single.full" / "factor.single.opt", one record per
launch and stream operation, built by launch_plan.cpp build_factor_schedule and walked as they are by numeric.hip) hold every launch decision once.  The
solve-side facts -- pair_levels, pair16_levels, leafchain_solve, and solve_reach(solver) for the fronts above 128 rows and the chain segments -- still
restate numeric.hip solve_sweep / solve_level: the solve walkers are the follow-up of the same shape.

reach(solver) is evaluated under the MI355X_KKT_DISABLE / MI355X_KKT_TUNE settings of the moment (the plan is rebuilt from the environment at every
query), so one analysed handle gives the facts of both legs of an A/B test.  Every fact is a count (0 = not reached)."""
import numpy as np

FC_WAVE, FC_LDS64, FC_LDS128, FC_BIG, FC_COUNT = 0, 1, 2, 3, 4
BIT_TFUSE, BIT_SELFASM, BIT_SOLO, BIT_SPLIT, BIT_TTAB, BIT_TTAB2, BIT_ASMCUT, BIT_ASMFAST, BIT_ALIAS = (1 << i for i in range(9))
INPUTS = ["chain_solve", "fuse_dt", "fastpiv", "asm_pull", "leafchain", "front_df", "tfuse", "fuse_upd", "selfasm", "grouped", "xcd_tiles", "lookahead",
          "pair_solve", "p1_small", "la_wgs", "la_min_nt", "grp_rbw_max", "chain_solve_maxc", "fuse_dt_maxwg", "la_min_tiles", "side_small"]
PLAN_ARRAYS = ["scalars", "path_scalars", "inputs", "level_list", "path_bits", "asm_fast_ok", "asmcut", "levels", "groups", "tiny16", "tiny_split", "mid_split",
               "big_split", "lc_ptr", "lc_fronts", "df_runs", "chain_segs", "chain_links", "chain_descs", "single.ptr", "single.maxm", "single.maxk",
               "single.last0", "single.last1", "single.allsolo", "factor.single.full", "factor.single.opt"]
# the records of a factor schedule (include/mi355x_kkt.h): columns of the exported rows, ops, streams
REC = 13
OP, STREAM, KIND, GX, GY, BLOCK, LV, B0, LDS, A0, A1, A2, A3 = range(REC)
(FO_LEAF_CHAIN, FO_FRONT_DF, FO_FRONT_DPP16, FO_REG_64_2, FO_REG_64_4, FO_REG_64_8, FO_REG_256_6_FAST4, FO_REG_256_8_FAST, FO_REG_256_6, FO_REG_256_8,
 FO_ASSEMBLE, FO_ASSEMBLE2, FO_GRP_FUSED, FO_DIAG_TRSM, FO_DIAG_REG, FO_DIAG_REG_1024, FO_TRSM, FO_TRSM_WIDE, FO_SCHUR64, FO_SCHUR, FO_SCHUR_P1, FO_SCHUR_Q,
 FO_FORK, FO_FORK_DONE, FO_JOIN, FO_SIDE_OPEN, FO_SIDE_CLOSE, FO_COUNT) = range(28)
FS_MAIN, FS_LOOKAHEAD, FS_SIDE = 0, 1, 2


def plan_arrays(s):
    """every exported array of the single-GPU plan under the settings of the moment"""
    return {w: s.launch_plan(w).copy() for w in PLAN_ARRAYS}


def plan_diff(a, b):
    """names of the arrays in which two plans differ"""
    return sorted(w for w in PLAN_ARRAYS if not np.array_equal(a[w], b[w]))


def solve_reach(s):
    """What the solve sweeps launch for the BIG fronts (order > 128) and the chain segments, under the MI355X_KKT_DISABLE / MI355X_KKT_TUNE of the moment:
    numeric.hip solve_sweep / solve_level restated for the single-GPU schedule (the per-class choice of the levels outside the chain segments; the
    segments go to k_fwd_chain / k_bwd_chain whole), with the shapes those kernels branch on.  Sets are returned as sorted lists."""
    I = s.info()
    nl, nsn = I.num_levels, I.num_sn
    order = np.diff(s.symbolic(2, nsn + 1)); cols = np.diff(s.symbolic(1, nsn + 1))
    parent, cls, level = s.symbolic(4, nsn), s.symbolic(23, nsn), s.symbolic(5, nsn)
    grp_pos, grp_rem, alias = s.symbolic(15, nsn), s.symbolic(16, nsn), s.symbolic(17, nsn)
    nchild = np.bincount(parent[parent >= 0], minlength=nsn)
    gathered = nchild - (alias >= 0)                      # children whose rows are added in (the in-place child shares the vector)
    A = {w: s.launch_plan(w).copy() for w in ("chain_segs", "chain_descs", "chain_links", "single.ptr", "single.maxm", "single.maxk", "single.last0",
                                              "single.last1", "single.allsolo", "scalars", "path_scalars")}
    ptr, maxk, allsolo = A["single.ptr"], A["single.maxk"], A["single.allsolo"]
    ng = A["single.last1"] - A["single.last0"]
    pair_solve, solve_group, lc_levels = int(A["path_scalars"][0]), int(A["path_scalars"][4]), int(A["scalars"][2])
    segs, descs, links = A["chain_segs"].reshape(-1, 9), A["chain_descs"].reshape(-1, 6), A["chain_links"].reshape(-1, 4)
    seg_of = np.full(nl, -1)
    for q, (lv0, lv1, *_) in enumerate(segs):
        seg_of[lv0:lv1 + 1] = q
    lcs = lc_levels if (pair_solve and lc_levels > 0 and not (seg_of[:lc_levels] >= 0).any()) else 0
    big = cls == FC_BIG
    F = dict(fwd_solo64_levels=0, fwd_solo_levels=0, fwd_grp_levels=0, bwd_dot64_levels=0, bwd_grp_levels=0)
    on_level = np.zeros(nsn, dtype=bool)                  # big fronts on level launches
    for lv in range(lcs, nl):
        if seg_of[lv] >= 0 or ptr[lv * FC_COUNT + FC_BIG + 1] == ptr[lv * FC_COUNT + FC_BIG] or ng[lv] <= 0:
            continue
        on_level |= big & (level == lv)
        F["fwd_solo64_levels" if allsolo[lv] and maxk[lv] <= 64 else "fwd_solo_levels" if allsolo[lv] else "fwd_grp_levels"] += 1
        F["bwd_dot64_levels" if not solve_group and maxk[lv] <= 64 else "bwd_grp_levels"] += 1
    F["solve_group"] = solve_group
    F["segments"], F["chains"], F["chain_levels"] = len(segs), len(descs), int((seg_of >= 0).sum())
    F["chain_fronts"] = len(links); F["chain_big_fronts"] = int(big[links[:, 0]].sum()) if len(links) else 0
    F["link_widths"] = sorted({int(x) for x in links[:, 1]})
    F["max_nlinks"] = int(descs[:, 1].max()) if len(descs) else 0
    F["chain_shapes"] = sorted({(int(d[1]), int(d[2])) for d in descs if big[d[4]]})      # (links, tail) of the chains that start at a big front
    F["tails"] = sorted({int(x) for x in descs[:, 2]})
    F["inits"] = sorted({int(x) for x in descs[:, 5]})
    F["max_gathered_chain_head"] = int(gathered[descs[:, 4]].max()) if len(descs) else 0
    F["max_gathered_level"] = int(gathered[on_level].max()) if on_level.any() else 0
    F["level_widths"] = sorted({int(x) for x in cols[on_level]})
    F["level_tails"] = sorted({int(x) for x in (order - cols)[on_level]})
    # solve units: per link, or (solve_group) per chain group, handled at the group's last link
    unit = big & ((grp_rem == 0) | (solve_group == 0))
    ulinks = np.where(solve_group != 0, grp_pos + 1, 1)
    ucols = cols.copy()
    if solve_group:
        for f in np.nonzero(unit)[0]:
            cur, tot = f, 0
            for _ in range(int(grp_pos[f]) + 1):
                tot += int(cols[cur]); cur = alias[cur]
            ucols[f] = tot
    F["unit_max_links"] = int(ulinks[unit].max()) if unit.any() else 0
    F["unit_max_cols"] = int(ucols[unit].max()) if unit.any() else 0
    F["unit_shapes"] = sorted({(int(ulinks[f]), int(ucols[f])) for f in np.nonzero(unit)[0]})
    F["upd_mod256"] = sorted({int(x) % 256 for x in (order - cols)[big]})
    F["big_fronts"] = int(big.sum())
    F["big_orders"] = (int(order[big].min()), int(order[big].max())) if big.any() else (0, 0)
    F["maxsupernode"] = int(I.maxsupernode)
    return F


def small_reach(s):
    """What the ONE-WAVEFRONT fronts (class FC_WAVE, order <= 32) of an analysed handle reach, under the MI355X_KKT_DISABLE / MI355X_KKT_TUNE of the moment.
    Solve side (numeric.hip solve_sweep / solve_level restated): the leaf-chain prefix of k_fwd_leafchain / k_bwd_leafchain, and per level outside it and
    outside the chain segments the instantiation taken -- "16x16" (k_*_pair<16, 16>: every front of the level of order <= 16, four per wavefront), "16"
    (k_*_pair<16>: k <= 16), "32" (k_*_pair<32>), "k64" (k_fwd<64> / k_bwd<64>, pair_solve off).  Factor side (counted from the exported plan): the leaf
    chains with their lengths and the input entries of their links, the data-flow runs with the fronts of order 17 .. 32 and the tagged contribution
    squares inside them (launch_plan.cpp: a front of a run whose parent is a front of the same run publishes a 16- or 32-wide square), the launches of
    the two factor schedules.  Sets are returned as sorted lists, histograms as sorted lists of (value, count)."""
    I = s.info()
    nl, nsn = I.num_levels, I.num_sn
    colptr = s.symbolic(1, nsn + 1)
    order = np.diff(s.symbolic(2, nsn + 1)); cols = np.diff(colptr)
    parent, cls, level, alias = s.symbolic(4, nsn), s.symbolic(23, nsn), s.symbolic(5, nsn), s.symbolic(17, nsn)
    acolptr = s.symbolic(7, I.n + 1)
    lp = s.symbolic(13, nl * FC_COUNT + 1)
    nchild = np.bincount(parent[parent >= 0], minlength=nsn)
    gathered = nchild - (alias >= 0)
    upd = order - cols
    entries = acolptr[colptr[1:]] - acolptr[colptr[:-1]]      # input entries of a front's pivot columns (FrontMeta aq0 .. aq1)
    wave = cls == FC_WAVE
    A = {w: s.launch_plan(w).copy() for w in ("scalars", "path_scalars", "levels", "chain_segs", "lc_ptr", "lc_fronts", "df_runs", "tiny16",
                                              "factor.single.full", "factor.single.opt")}
    pair_solve, lc_levels, lc_nchains = int(A["path_scalars"][0]), int(A["scalars"][2]), int(A["scalars"][3])
    lvl = A["levels"].reshape(-1, 10)
    wave_mmax, wave_kmax = lvl[:, 8], lvl[:, 9]
    in_seg = np.zeros(nl, dtype=bool)
    for lv0, lv1, *_ in A["chain_segs"].reshape(-1, 9):
        in_seg[lv0:lv1 + 1] = True
    lcs = lc_levels if (pair_solve and lc_levels > 0 and not in_seg[:lc_levels].any()) else 0
    F = dict(n=int(I.n), num_sn=int(nsn), num_levels=int(nl), pair_solve=pair_solve, lc_levels=lc_levels, lc_nchains=lc_nchains, leafchain_solve=lcs,
             seg_levels=int(in_seg.sum()))
    inst = {"16x16": [], "16": [], "32": [], "k64": []}
    for lv in range(lcs, nl):
        if in_seg[lv] or lp[lv * FC_COUNT + 1] == lp[lv * FC_COUNT]:
            continue
        inst["k64" if not pair_solve else "16x16" if wave_mmax[lv] <= 16 else "16" if wave_kmax[lv] <= 16 else "32"].append(lv)
    F["solve_levels"] = inst
    F["solve_level_counts"] = {k: len(v) for k, v in inst.items()}
    on_pair32 = wave & np.isin(level, inst["32"])
    F["pair32_k_over_16"] = int(np.sum(on_pair32 & (cols > 16)))
    on_level = wave & np.isin(level, sum(inst.values(), []))
    F["max_gathered_on_levels"] = int(gathered[on_level].max()) if on_level.any() else 0
    # the fronts
    F["classes"] = sorted({int(x) for x in cls})
    F["shapes"] = sorted({(int(order[f]), int(cols[f]), int(nchild[f])) for f in np.nonzero(wave)[0]})
    F["wave_fronts"] = int(wave.sum())
    F["wave_k_over_16"] = int(np.sum(wave & (cols > 16)))
    F["max_children"] = int(nchild[wave].max()) if wave.any() else 0
    F["max_gathered"] = int(gathered[wave].max()) if wave.any() else 0
    # leaf chains
    ptr, lcf = A["lc_ptr"], A["lc_fronts"]
    lens = np.diff(ptr) if lc_levels else np.zeros(0, dtype=int)
    F["chain_lengths"] = sorted((int(a), int(b)) for a, b in zip(*np.unique(lens, return_counts=True)))
    F["link_shapes"] = sorted({(int(order[f]), int(cols[f])) for f in lcf})
    F["link_max_entries"] = int(entries[lcf].max()) if len(lcf) else 0
    F["links_over_48_entries"] = int(np.sum(entries[lcf] > 48)) if len(lcf) else 0
    F["root_links_k_eq_order"] = int(np.sum((parent[lcf] < 0) & (order[lcf] == cols[lcf]))) if len(lcf) else 0
    # data-flow runs: (first level, last level, virtual workgroups)
    runs = A["df_runs"].reshape(-1, 5)
    F["df_runs"] = [(int(r[0]), int(r[1]), int(r[4])) for r in runs]
    run_of = np.full(nsn, -1)
    for q, r in enumerate(runs):
        run_of[wave & (level >= r[0]) & (level <= r[1])] = q
    F["df_fronts_17_32"] = int(np.sum((run_of >= 0) & (order > 16)))
    tagged = (run_of >= 0) & (parent >= 0) & (upd > 0)
    tagged[tagged] = run_of[parent[tagged]] == run_of[tagged]
    F["tagged16"] = int(np.sum(tagged & (upd <= 16))); F["tagged32"] = int(np.sum(tagged & (upd > 16)))
    F["tagged_rows"] = sorted({int(x) for x in upd[tagged]})
    F["tagged_parents_17_32_children"] = int(max((np.sum(tagged & (parent == p)) for p in set(parent[tagged].tolist()) if order[p] > 16), default=0))
    F["df_max_gathered"] = int(gathered[run_of >= 0].max()) if (run_of >= 0).any() else 0
    # the two factor schedules: launches per kernel
    for name, key in (("full", "factor.single.full"), ("opt", "factor.single.opt")):
        recs = A[key].reshape(-1, REC)
        F[name] = tuple(int(np.sum(recs[:, OP] == op)) for op in (FO_LEAF_CHAIN, FO_FRONT_DF, FO_FRONT_DPP16, FO_REG_64_4, FO_REG_64_2))
    return F


def reach(s):
    I = s.info()
    nl, nsn = I.num_levels, I.num_sn
    order = np.diff(s.symbolic(2, nsn + 1)); cols = np.diff(s.symbolic(1, nsn + 1))
    parent, cls = s.symbolic(4, nsn), s.symbolic(23, nsn)
    grp_rem, alias = s.symbolic(16, nsn), s.symbolic(17, nsn)
    lp = s.symbolic(13, nl * FC_COUNT + 1)
    nchild = np.bincount(parent[parent >= 0], minlength=nsn)
    A = plan_arrays(s)
    L, bits, asmcut = A["level_list"], A["path_bits"], A["asmcut"]
    scal, ps = A["scalars"], A["path_scalars"]
    inp = dict(zip(INPUTS, (int(x) for x in A["inputs"])))
    wave_mmax = A["levels"].reshape(-1, 10)[:, 8]
    maxk = A["single.maxk"]
    pair_solve, la_any, ttab_len = int(ps[0]), int(ps[1]), int(ps[2])
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
    full, opt = A["factor.single.full"].reshape(-1, REC), A["factor.single.opt"].reshape(-1, REC)
    n_of = lambda recs, *ops: int(np.sum(np.isin(recs[:, OP], ops)))
    F["fused_diag_trsm_level"] = n_of(full, FO_DIAG_TRSM)
    F["narrow_fused_level"] = int(np.sum((full[:, OP] == FO_DIAG_TRSM) & (full[:, GY] > 1 + full[:, A0])))      # (workgroups behind the pivot block and the row blocks: the narrow updates)
    F["assemble2_level"] = n_of(full, FO_ASSEMBLE2); F["assemble_column_level"] = n_of(full, FO_ASSEMBLE)
    # (the split bit alone launches nothing: only the 128 x 128 update of fronts above 1024 rows reads it)
    F["lookahead_fork_level"] = n_of(full, FO_FORK); F["p1_small_level"] = n_of(full, FO_SCHUR_P1)
    # xcd_affine acts in k_big_trsm and k_big_schur64 on launches over >= 16 fronts
    F["xcd_affine_launch"] = int(np.sum(np.isin(full[:, OP], (FO_TRSM, FO_TRSM_WIDE, FO_SCHUR64)) & (full[:, GY] >= 16)))
    F["group_launch_level"] = n_of(full, FO_GRP_FUSED)
    F["schur128_level"] = len(set(full[np.isin(full[:, OP], (FO_SCHUR, FO_SCHUR_P1)), LV].tolist())); F["schur64_level"] = n_of(full, FO_SCHUR64)
    # k_big_assemble / k_big_assemble2 with V.asm_pull: the fronts that gather children's blocks (not in place on a child, not assembling themselves)
    F["asm_pull_fronts"] = int(np.sum(big & (alias < 0) & (nchild > 0))) if inp["asm_pull"] else 0
    F["asm_gather_fronts"] = int(np.sum(big & (alias < 0) & (nchild > 0)))
    # side stream: the (level, class) buckets whose launches the schedule a factorisation first tries puts there
    side = opt[(opt[:, STREAM] == FS_SIDE) & (opt[:, KIND] >= 0)]
    F["side_small_bucket"] = len(set(zip(side[:, LV].tolist(), side[:, KIND].tolist())))      # (the profiling kind of a small-front launch is its class)
    # the optimistic schedule drops strict launches where the static-order kernels take a whole bucket, and runs the leaf chains / data-flow runs:
    # k_front_reg<64, 2> is the strict launch over >= 2 048 fronts of order <= 16
    F["reg2_level_strict"] = n_of(full, FO_REG_64_2)
    F["reg2_level_optimistic"] = n_of(opt, FO_REG_64_2)
    F["optimistic_only"] = int(np.sum(opt[opt[:, OP] == FO_LEAF_CHAIN, A1] + 1)) + n_of(opt, FO_FRONT_DF)      # (levels of the leaf chains + data-flow runs)
    # fronts of order exactly 1024 and 1025 in ONE launch (the two sides of the big_split edge)
    level = s.symbolic(5, nsn)
    F["edge_1024_1025_level"] = len(set(level[big & (order == 1024)].tolist()) & set(level[big & (order == 1025)].tolist()))
    # big_diag_body `V.fastpiv && k <= 64`: pivot blocks of big fronts that try the blocked static-order LDL^T first
    F["fastpiv_big_blocks"] = int(np.sum(big & (cols <= 64))) if inp["fastpiv"] else 0
    F["maxsupernode"] = int(I.maxsupernode)
    F["inputs"] = inp
    return F
