"""The solve-block path (mi355x_kkt_set_solve_block): the rows of its test table -- existing fixtures of smallfix / midfix / bigfix under
the knobs of one of their legs -- and a restatement, in the shape of reach.small_reach / reach.solve_reach, of the rules by which launch_plan.cpp
build_solve_block_schedule lists the launches of one block of right-hand sides ("solve.single.block", include/mi355x_kkt.h):

  lcs  the leaf-chain prefix of solve_sweep; L* = the first level >= lcs that starts a chain segment (num_levels: none)
  bulk (levels below L*): forward the leaf-chain launch, then levels lcs .. L*-1; backward levels L*-1 .. lcs, then the leaf-chain launch.  Per (level,
       class) the kernel solve_level launches; BLOCKED (one launch for all columns) for the leaf chains, the pair kernels and the mid kernels, BY COLUMN
       for everything else
  top  (levels from L* up), per column: k_bump_epoch, the forward walk over [L*, NL), the backward walk over the same levels -- chain segments as one
       k_fwd_chain / k_bwd_chain launch each
  order of the records: bulk forward | top part of one column | bulk backward

tests/test_solve_block_plan.py compares the exported schedule with expected() record by record and pins the counts per row (PINNED), so that a change of
ordering or of a threshold fails on the host and does not silently empty a row of tests/test_gpu_solve_block.py."""
import os

import numpy as np

import ipopt_amd
from tests.support import bigfix, midfix, pathfix, reach as R, smallfix

WIDTH = 4                      # SOLVE_RB (MI355X_KKT_SOLVE_BLOCK)
MID_KMAX = 64
(SO_BUMP_EPOCH, SO_FWD_LEAFCHAIN, SO_BWD_LEAFCHAIN, SO_FWD_PAIR16_16, SO_FWD_PAIR16, SO_FWD_PAIR32, SO_BWD_PAIR16_16, SO_BWD_PAIR16, SO_BWD_PAIR32,
 SO_FWD_MID1, SO_FWD_MID2, SO_BWD_MID1, SO_BWD_MID2, SO_FWD_WAVE, SO_FWD_LDS64, SO_FWD_LDS128, SO_BWD_WAVE, SO_BWD_LDS64, SO_BWD_LDS128,
 SO_FWD_SOLO64, SO_FWD_SOLO, SO_FWD_GRP, SO_FWD_GRP_UPD, SO_BWD_DOT64, SO_BWD_FIN64, SO_BWD_GRP_DOT, SO_BWD_GRP, SO_FWD_CHAIN, SO_BWD_CHAIN, SO_COUNT) = range(30)
SB_BLOCKED, SB_BYCOL, SB_TOP = 0, 1, 2
OP_NAMES = ["bump_epoch", "fwd_leafchain", "bwd_leafchain", "fwd_pair16x16", "fwd_pair16", "fwd_pair32", "bwd_pair16x16", "bwd_pair16", "bwd_pair32",
            "fwd_mid1", "fwd_mid2", "bwd_mid1", "bwd_mid2", "fwd_wave", "fwd_lds64", "fwd_lds128", "bwd_wave", "bwd_lds64", "bwd_lds128",
            "fwd_solo64", "fwd_solo", "fwd_grp", "fwd_grp_upd", "bwd_dot64", "bwd_fin64", "bwd_grp_dot", "bwd_grp", "fwd_chain", "bwd_chain"]
# kernel kinds (MI355X_KKT_KERNEL_*)
KK_SOLVE_PERM, KK_FWD_WAVE, KK_FWD_LDS, KK_FWD_BIG, KK_BWD_WAVE, KK_BWD_LDS, KK_BWD_BIG, KK_FWD_BIG_UPD, KK_BWD_BIG_DOT = 9, 10, 11, 12, 13, 14, 15, 16, 17

# row -> (fixture module, fixture, what selects the knobs)
ROWS = {
    "leaf_edges.levels": ("small", "leaf_edges", "levels"),
    "leaf_edges_w8.levels": ("small", "leaf_edges_w8", "levels"),
    "wave_edges.levels": ("small", "wave_edges", "levels"),
    "leaf_edges.default": ("small", "leaf_edges", "default"),
    "leaf_edges.nopair": ("small", "leaf_edges", "nopair"),
    "mid_edges": ("mid", "mid_edges", False),
    "mid_edges.nomid": ("mid", "mid_edges", True),
    "grid48x44": ("mid", "grid48x44", False),
    "hostile16": ("mid", "hostile16", False),
    "tails.levels": ("big", "tails", "levels"),
    "star6.groups": ("big", "star6", "groups"),
    "chain_delayed.levels": ("big", "chain_delayed", "levels"),
}


def knobs(row):
    """the MI355X_KKT_TUNE / MI355X_KKT_DISABLE of the row, to be held from the set-up of the handle to its last solve"""
    mod, name, sel = ROWS[row]
    if mod == "small":
        return smallfix.leg_knobs(sel)
    if mod == "mid":
        return pathfix.knobs(midfix.disable_list(name, sel), midfix.FIXTURES[name][2])
    return bigfix.leg_knobs(sel)


def system(row):
    mod, name, _ = ROWS[row]
    return {"small": smallfix.system, "mid": midfix.system, "big": bigfix.system}[mod](name)


def handle(row, **more):
    """a handle analysed for the row; call under knobs(row)"""
    mod, name, sel = ROWS[row]
    if mod == "small":
        return smallfix.handle(name, **more)
    if mod == "big":
        return bigfix.handle(name, sel, **more)
    S = system(row)
    s = ipopt_amd.KKTSolver(**{**S["opts"], **more})
    s.initialize_structure(S["n"], S["r"], S["c"], vals=S["v"])
    return s


def schedule(s):
    """the exported records (n x 13)"""
    return s.launch_plan("solve.single.block").reshape(-1, R.REC)


def expected(s):
    """(records as a list of 13-tuples, L*, (blocked launches, launches by column, top launches per column) of one full block) -- the rules of the module
    docstring applied to the exported tables of the plan, under the MI355X_KKT_DISABLE / MI355X_KKT_TUNE of the moment"""
    I = s.info()
    nl = I.num_levels
    A = {w: s.launch_plan(w).copy() for w in ("scalars", "path_scalars", "levels", "chain_segs", "single.ptr", "single.base", "single.maxm", "single.maxk",
                                              "single.last0", "single.last1", "single.allsolo")}
    ptr, base = A["single.ptr"], int(A["single.base"][0])
    maxm, maxk, last0, last1, allsolo = A["single.maxm"], A["single.maxk"], A["single.last0"], A["single.last1"], A["single.allsolo"]
    pair, solve_group = int(A["path_scalars"][0]), int(A["path_scalars"][4])
    lc_levels, lc_nchains = int(A["scalars"][2]), int(A["scalars"][3])
    lvl = A["levels"].reshape(-1, 10)
    wave_mmax, wave_kmax = lvl[:, 8], lvl[:, 9]
    segs = A["chain_segs"].reshape(-1, 9)
    seg0, seg1 = np.full(nl, -1), np.full(nl, -1)
    for q, sg in enumerate(segs):
        seg0[sg[0]] = q; seg1[sg[1]] = q
    mid = "mid_solve" not in (os.environ.get("MI355X_KKT_DISABLE") or "").split(",") and I.maxsupernode <= MID_KMAX
    lds = lambda mmax, kmax: (mmax + 3 * kmax) * 8 + 16
    rec = []

    def put(op, sb, kind, lv, b0, gx, gy, block, ldsb=0, a0=0):
        rec.append((op, sb, kind, gx, gy, block, lv, b0, ldsb, a0, 0, 0, 0))

    def level(lv, fwd, top):
        blk, col = (SB_TOP, SB_TOP) if top else (SB_BLOCKED, SB_BYCOL)
        for fc in range(R.FC_COUNT):
            b0 = base + int(ptr[lv * R.FC_COUNT + fc]); nb = int(ptr[lv * R.FC_COUNT + fc + 1] - ptr[lv * R.FC_COUNT + fc])
            if nb == 0:
                continue
            g0, ng, mm = int(last0[lv]), int(last1[lv] - last0[lv]), int(maxm[lv])
            if fc == R.FC_WAVE:
                if pair and wave_mmax[lv] <= 16:
                    put(SO_FWD_PAIR16_16 if fwd else SO_BWD_PAIR16_16, blk, KK_FWD_WAVE if fwd else KK_BWD_WAVE, lv, b0, (nb + 3) // 4, 1, 64, 0, nb)
                elif pair and wave_kmax[lv] <= 16:
                    put(SO_FWD_PAIR16 if fwd else SO_BWD_PAIR16, blk, KK_FWD_WAVE if fwd else KK_BWD_WAVE, lv, b0, (nb + 1) // 2, 1, 64, 0, nb)
                elif pair:
                    put(SO_FWD_PAIR32 if fwd else SO_BWD_PAIR32, blk, KK_FWD_WAVE if fwd else KK_BWD_WAVE, lv, b0, (nb + 1) // 2, 1, 64, 0, nb)
                else:
                    put(SO_FWD_WAVE if fwd else SO_BWD_WAVE, col, KK_FWD_WAVE if fwd else KK_BWD_WAVE, lv, b0, nb, 1, 64, lds(32, 32))
            elif fc == R.FC_LDS64:
                if mid:
                    put(SO_FWD_MID1 if fwd else SO_BWD_MID1, blk, KK_FWD_LDS if fwd else KK_BWD_LDS, lv, b0, nb, 1, 64)
                else:
                    put(SO_FWD_LDS64 if fwd else SO_BWD_LDS64, col, KK_FWD_LDS if fwd else KK_BWD_LDS, lv, b0, nb, 1, 64, lds(64, 64))
            elif fc == R.FC_LDS128:
                if mid:
                    put(SO_FWD_MID2 if fwd else SO_BWD_MID2, blk, KK_FWD_LDS if fwd else KK_BWD_LDS, lv, b0, nb, 1, 64)
                else:
                    put(SO_FWD_LDS128 if fwd else SO_BWD_LDS128, col, KK_FWD_LDS if fwd else KK_BWD_LDS, lv, b0, nb, 1, 256, lds(128, 128))
            elif ng <= 0:
                continue
            elif fwd:
                if allsolo[lv] and maxk[lv] <= 64:
                    put(SO_FWD_SOLO64, col, KK_FWD_BIG, lv, g0, (mm + 63) // 64 + 1, ng, 256)
                elif allsolo[lv]:
                    put(SO_FWD_SOLO, col, KK_FWD_BIG, lv, g0, (mm + 63) // 64 + 1, ng, 256)
                else:
                    put(SO_FWD_GRP, col, KK_FWD_BIG, lv, g0, ng, 1, 256)
                    put(SO_FWD_GRP_UPD, col, KK_FWD_BIG_UPD, lv, g0, (mm + 63) // 64, ng, 256)
            elif not solve_group and maxk[lv] <= 64:
                put(SO_BWD_DOT64, col, KK_BWD_BIG_DOT, lv, g0, (mm + 255) // 256, ng, 256)
                put(SO_BWD_FIN64, col, KK_BWD_BIG, lv, g0, ng, 1, 256)
            else:
                put(SO_BWD_GRP_DOT, col, KK_BWD_BIG_DOT, lv, g0, (mm + 255) // 256, ng, 256)
                put(SO_BWD_GRP, col, KK_BWD_BIG, lv, g0, ng, 1, 256)

    def walk(lo, hi, fwd, top):
        q = lo
        while q < hi:
            lv = q if fwd else hi - 1 + lo - q
            sgi = seg0[lv] if fwd else seg1[lv]
            if sgi < 0:
                level(lv, fwd, top)
            else:
                sg = segs[sgi]
                if fwd:
                    put(SO_FWD_CHAIN, SB_TOP, KK_FWD_BIG, lv, int(sg[7]), int(sg[4]), 1, 320)
                else:
                    put(SO_BWD_CHAIN, SB_TOP, KK_BWD_BIG, lv, int(sg[8]), int(sg[5]), 1, 320)
                q += int(sg[1] - sg[0])
            q += 1

    lcs = lc_levels if (pair and lc_levels > 0 and not (seg0[:lc_levels] >= 0).any()) else 0
    starts = [lv for lv in range(lcs, nl) if seg0[lv] >= 0]
    ls = starts[0] if starts else nl
    if lcs > 0:
        put(SO_FWD_LEAFCHAIN, SB_BLOCKED, KK_FWD_WAVE, 0, 0, (lc_nchains + 3) // 4, 1, 64, 0, lc_nchains)
    walk(lcs, ls, True, False)
    if ls < nl:
        put(SO_BUMP_EPOCH, SB_TOP, KK_SOLVE_PERM, ls, 0, 1, 1, 64)
        walk(ls, nl, True, True)
        walk(ls, nl, False, True)
    walk(lcs, ls, False, False)
    if lcs > 0:
        put(SO_BWD_LEAFCHAIN, SB_BLOCKED, KK_BWD_WAVE, 0, 0, (lc_nchains + 3) // 4, 1, 64, 0, lc_nchains)
    kinds = [r[1] for r in rec]
    return rec, ls, (kinds.count(SB_BLOCKED), WIDTH * kinds.count(SB_BYCOL), kinds.count(SB_TOP))


def facts(s):
    """what a handle's exported schedule reaches: L*, levels, per issue kind the number of records of every kernel, the three counts of solve_block_info"""
    recs = schedule(s)
    per = {"blocked": {}, "bycol": {}, "top": {}}
    for r in recs:
        d = per[("blocked", "bycol", "top")[r[R.STREAM]]]
        d[OP_NAMES[r[R.OP]]] = d.get(OP_NAMES[r[R.OP]], 0) + 1
    info = s.solve_block_info()
    return dict(first_top_level=info["first_top_level"], num_levels=int(s.info().num_levels), **per,
                counts=(info["blocked_launches"], info["bycol_launches"], info["top_launches_per_column"]))
