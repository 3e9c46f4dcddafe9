"""The factor schedule on the host (launch_plan.cpp build_factor_schedule through mi355x_kkt_get_launch_plan "factor.*", no device): the flat list
of launches and stream operations the device walks record by record, checked against what the STRUCTURE demands -- every front factored by the
launches of its class exactly as often as that class takes, look-ahead forks joined before anything may touch what they write, grids and LDS sizes
the runtime accepts -- for the single-GPU plan in both variants and for every rank of 2- and 4-rank worlds under both mappings."""
import functools

import numpy as np
import pytest

import ipopt_amd
from tests import test_launch_plan as TLP
from tests import test_sr1_abi as HOSTCHECK
from tests.support import mirror, pathfix
from tests.support.reach import (REC, OP, STREAM, KIND, GX, GY, BLOCK, LV, B0, LDS, A0, A1, A2, A3, FS_MAIN, FS_LOOKAHEAD, FS_SIDE,
                                 FO_LEAF_CHAIN, FO_FRONT_DF, FO_FRONT_DPP16, FO_REG_64_2, FO_REG_64_4, FO_REG_64_8, FO_REG_256_6_FAST4, FO_REG_256_8_FAST,
                                 FO_REG_256_6, FO_REG_256_8, FO_ASSEMBLE, FO_ASSEMBLE2, FO_GRP_FUSED, FO_DIAG_TRSM, FO_DIAG_REG, FO_DIAG_REG_1024, FO_TRSM,
                                 FO_TRSM_WIDE, FO_SCHUR64, FO_SCHUR, FO_SCHUR_P1, FO_SCHUR_Q, FO_FORK, FO_FORK_DONE, FO_JOIN, FO_SIDE_OPEN, FO_SIDE_CLOSE, FO_COUNT)

FC_WAVE, FC_LDS64, FC_LDS128, FC_BIG, FC_COUNT = 0, 1, 2, 3, 4
KK_FRONT_WAVE, KK_FRONT_LDS64, KK_FRONT_LDS128, KK_BIG_ASSEMBLE, KK_BIG_DIAG, KK_BIG_TRSM, KK_BIG_SCHUR = 1, 2, 3, 4, 5, 6, 7
PATHFIX = ["grid30", "clique_grid", "lukvl1000"]
STREAM_OPS = (FO_FORK, FO_FORK_DONE, FO_JOIN, FO_SIDE_OPEN, FO_SIDE_CLOSE)
STRICT_WAVE, FAST_MID, STRICT_MID = (FO_REG_64_2, FO_REG_64_4), (FO_REG_256_6_FAST4, FO_REG_256_8_FAST), (FO_REG_256_6, FO_REG_256_8)
PIVOT_BLOCKS, PANELS, UPDATES = (FO_DIAG_REG, FO_DIAG_REG_1024, FO_DIAG_TRSM), (FO_TRSM, FO_TRSM_WIDE, FO_DIAG_TRSM), (FO_SCHUR64, FO_SCHUR, FO_SCHUR_P1)
LDS_MAX = 160 * 1024


@functools.lru_cache(maxsize=None)
def analysed(system, nranks=1, subcube=0):
    """(solver, symbolic arrays, MI355X_KKT_TUNE of the fixture)"""
    if system in PATHFIX:
        S = pathfix.system(system)
        n, r, c, v, tune = S["n"], S["r"], S["c"], S["v"], S["tune"]
    else:
        (n, r, c, v, _), tune = TLP.SYSTEMS[system](), None
    with pathfix.knobs(None, tune):
        s = ipopt_amd.KKTSolver(nranks=nranks, subcube=subcube)
        s.initialize_structure(n, r, c, vals=v)
    sym = mirror.fetch(s)
    nsn = sym["info"].num_sn
    sym.update(order=np.diff(sym["rowptr"]), cols=np.diff(sym["colptr"]), grp_pos=s.symbolic(15, nsn), grp_rem=s.symbolic(16, nsn), alias=s.symbolic(17, nsn))
    return s, sym, tune


def ranges_tile(recs, count, b0, b1):
    """the launch ranges [B0, B0 + count) of the records tile [b0, b1), in order"""
    at = b0
    for r in recs:
        assert r[B0] == at and count(r) > 0, (r.tolist(), at)
        at += count(r)
    return at == b1


def check_list(sym, plan, name, sched, optimistic):
    """every invariant of one exported list `name` over the schedule `sched` (single | local | stage<d>)"""
    recs = plan(name).reshape(-1, REC)
    L = plan("level_list")
    nl = sym["info"].num_levels
    ptr, base = plan(sched + ".ptr"), int(plan(sched + ".base")[0])
    order, cols, cls, level, grp_pos, grp_rem, alias = (sym[k] for k in ("order", "cols", "cls", "level", "grp_pos", "grp_rem", "alias"))
    grouped, grp_cut = int(plan("scalars")[5]), int(plan("path_scalars")[3])
    upd = order - cols
    nchild = np.bincount(sym["parent"][sym["parent"] >= 0], minlength=len(order))
    bucket = lambda lv, fc: (base + int(ptr[lv * FC_COUNT + fc]), base + int(ptr[lv * FC_COUNT + fc + 1]))
    # ---- what the runtime accepts ----
    assert np.all((recs[:, OP] >= 0) & (recs[:, OP] < FO_COUNT))
    assert np.all(recs[:, GX] > 0) and np.all(recs[:, GY] > 0), "a grid of 0 workgroups is refused"
    assert np.all(recs[:, BLOCK] <= 1024) and np.all(recs[:, BLOCK] >= 0)
    assert np.all(recs[np.isin(recs[:, OP], STREAM_OPS) | (recs[:, OP] == FO_SCHUR), BLOCK] == 0) and np.all(recs[~np.isin(recs[:, OP], STREAM_OPS + (FO_SCHUR,)), BLOCK] % 64 == 0)
    assert np.all(recs[~np.isin(recs[:, OP], STREAM_OPS + (FO_SCHUR,)), BLOCK] > 0)
    assert np.all((recs[:, LDS] >= 0) & (recs[:, LDS] <= LDS_MAX))
    assert np.all((recs[:, KIND] == -1) == np.isin(recs[:, OP], STREAM_OPS))
    assert np.all(recs[:, B0] >= 0) and np.all(recs[:, B0] < len(L))
    # ---- streams: levels never decrease along the main stream; the side stream opens and closes inside one level ----
    main = recs[recs[:, STREAM] == FS_MAIN]
    assert np.all(np.diff(main[:, LV]) >= 0)
    side_lv = None
    for r in recs:
        if r[OP] == FO_SIDE_OPEN:
            assert side_lv is None and r[STREAM] == FS_MAIN
            side_lv = r[LV]
        elif r[OP] == FO_SIDE_CLOSE:
            assert side_lv == r[LV] and r[STREAM] == FS_SIDE
            side_lv = None
        elif r[STREAM] == FS_SIDE:
            assert side_lv == r[LV] and r[KIND] in (KK_FRONT_WAVE, KK_FRONT_LDS64, KK_FRONT_LDS128)
        elif side_lv is not None:
            assert r[LV] == side_lv      # (main-stream launches of the same level run beside it)
    assert side_lv is None
    if sched != "single":
        assert np.all(recs[:, STREAM] == FS_MAIN)      # the multi-rank schedules fork nothing
    # ---- look-ahead: fork, part 2, fork-done come together; B is joined before the list ends and before a later full 128 x 128 update ----
    pending = None
    for i, r in enumerate(recs):
        if r[OP] == FO_FORK:
            q, d = recs[i + 1], recs[i + 2]
            assert q[OP] == FO_SCHUR_Q and d[OP] == FO_FORK_DONE and q[STREAM] == d[STREAM] == FS_LOOKAHEAD and r[STREAM] == FS_MAIN
            assert (q[LV], q[B0]) == (r[LV], r[B0]) and (d[LV], d[A0]) == (r[LV], r[A0])
            p1 = recs[i - 1]      # part 1 of the same fronts, or behind it the whole update of those that are not split
            if p1[OP] == FO_SCHUR and p1[A0] == 4:
                p1 = recs[i - 2]
            assert p1[OP] in (FO_SCHUR, FO_SCHUR_P1) and (p1[B0], p1[GY], p1[LV]) == (q[B0], q[GY], q[LV])
        elif r[OP] == FO_SCHUR_Q:
            assert recs[i - 1][OP] == FO_FORK
        elif r[OP] == FO_FORK_DONE:
            pending = (r[A0], r[LV])
        elif r[OP] == FO_JOIN:
            assert pending == (r[A0], r[A1]) and r[STREAM] == FS_MAIN
            pending = None
        elif r[OP] in (FO_SCHUR, FO_SCHUR_P1) and any(grp_rem[L[q]] == 0 for q in range(r[B0], r[B0] + r[GY])):
            assert pending is None, ("a full update behind an unjoined fork", r.tolist())
    assert pending is None
    # ---- variants ----
    if not optimistic:
        assert not np.any(np.isin(recs[:, OP], (FO_LEAF_CHAIN, FO_FRONT_DF))) and not np.any((recs[:, OP] == FO_FRONT_DPP16) & (recs[:, A2] != 0))
    handed = np.zeros(nl, dtype=bool)      # levels the optimistic schedule hands to k_leaf_chain / k_front_df as a whole
    for r in recs[np.isin(recs[:, OP], (FO_LEAF_CHAIN, FO_FRONT_DF))]:
        lv0, lv1 = (0, r[A1]) if r[OP] == FO_LEAF_CHAIN else (r[LV], r[A3])
        assert sched == "single" and not handed[lv0:lv1 + 1].any() and r[B0] == bucket(lv0, FC_WAVE)[0]
        handed[lv0:lv1 + 1] = True
        for lv in range(lv0, lv1 + 1):      # nothing but one-wavefront fronts there (leaf chains: of order <= 16)
            assert bucket(lv, FC_WAVE)[1] == bucket(lv, FC_COUNT - 1)[1] and bucket(lv, FC_WAVE)[1] > bucket(lv, FC_WAVE)[0]
            if r[OP] == FO_LEAF_CHAIN:
                assert np.all(order[L[slice(*bucket(lv, FC_WAVE))]] <= 16)
    assert not np.any(handed[recs[~np.isin(recs[:, OP], (FO_LEAF_CHAIN, FO_FRONT_DF, FO_JOIN)), LV]]), "a level handed over as a whole is launched again"
    # ---- coverage, per (level, class) ----
    grouped_fronts = {}      # front -> times a k_grp_fused launch factors it
    for lv in range(nl):
        if handed[lv]:
            continue
        at = recs[(recs[:, LV] == lv) & (recs[:, KIND] >= 0)]
        of = lambda *ops: at[np.isin(at[:, OP], ops)]
        nfronts = lambda r: int(r[GX])
        # one-wavefront fronts: the static-order launch (order <= 16 only) first, then the strict ones tile the bucket -- or, optimistic, the static-order
        # launch takes a bucket of nothing but such fronts and raises the flag for what it rejects
        b0, b1 = bucket(lv, FC_WAVE)
        dpp = of(FO_FRONT_DPP16)
        assert len(dpp) <= 1
        whole = len(dpp) == 1 and dpp[0][A2] != 0
        for r in dpp:
            assert r[B0] == b0 and 0 < r[A0] <= b1 - b0 and r[GX] == (r[A0] + 3) // 4 and np.all(order[L[b0:b0 + r[A0]]] <= 16)
        if whole:
            assert optimistic and dpp[0][A0] == b1 - b0 and len(of(*STRICT_WAVE)) == 0
        else:
            assert ranges_tile(of(*STRICT_WAVE), nfronts, b0, b1), (name, lv, "wave")
            for r in of(FO_REG_64_2):
                assert np.all(order[L[r[B0]:r[B0] + r[GX]]] <= 16)
            # the strict launches behind a static-order launch skip what it took -- and skip nothing where there was none
            assert np.all((of(*STRICT_WAVE)[:, A0] & 2 != 0) == (len(dpp) == 1))
        b0, b1 = bucket(lv, FC_LDS64)
        assert ranges_tile(of(FO_REG_64_8), nfronts, b0, b1), (name, lv, "lds64")
        b0, b1 = bucket(lv, FC_LDS128)
        assert ranges_tile(of(*STRICT_MID), nfronts, b0, b1), (name, lv, "lds128")
        assert len(of(*FAST_MID)) == 0 or ranges_tile(of(*FAST_MID), nfronts, b0, b1), (name, lv, "lds128 static order")
        assert np.all((of(*STRICT_MID)[:, A0] & 2 != 0) == (len(of(*FAST_MID)) > 0))
        for r in of(FO_REG_256_6, FO_REG_256_6_FAST4):
            assert np.all(order[L[r[B0]:r[B0] + r[GX]]] <= 96)
        # big fronts: pivot blocks and panels once each -- per level, or per chain group at the level of its first link
        b0, b1 = bucket(lv, FC_BIG)
        for r in of(FO_GRP_FUSED):
            for q in range(r[B0], r[B0] + r[GX]):
                sn = int(L[q])
                assert grp_rem[sn] == 0
                for _ in range(grp_pos[sn] + 1):
                    grouped_fronts[sn] = grouped_fronts.get(sn, 0) + 1
                    first, sn = sn, int(alias[sn])
                assert level[first] == lv
        if grouped and lv >= grp_cut:
            assert len(of(*PIVOT_BLOCKS, FO_TRSM, FO_TRSM_WIDE)) == 0
        else:
            assert len(of(FO_GRP_FUSED)) == 0
            assert ranges_tile(of(*PIVOT_BLOCKS), nfronts, b0, b1), (name, lv, "pivot blocks")
            assert ranges_tile(of(*PANELS), lambda r: int(r[GX] if r[OP] == FO_DIAG_TRSM else r[GY]), b0, b1), (name, lv, "panels")
            for r in of(FO_DIAG_REG, FO_TRSM, FO_DIAG_TRSM):
                assert np.all(cols[L[b0:b1]] <= 64)
        assert len(of(FO_ASSEMBLE, FO_ASSEMBLE2)) <= 1
        if any(not (alias[x] >= 0 and nchild[x] == 1) for x in L[b0:b1]) and sched == "single":      # (all pure in-place links: they assemble themselves)
            assert len(of(FO_ASSEMBLE, FO_ASSEMBLE2)) == 1, (name, lv, "assembly")
        for r in of(FO_ASSEMBLE, FO_ASSEMBLE2):
            assert (r[B0], r[B0] + r[GY]) == (b0, b1)
        # trailing updates: every front with update rows gets its update once -- in the fused launch (narrow tiles), from one update launch, or from the
        # pair (part 1 of the split fronts, whole update of the others) of a forked level
        took = {}
        for r in of(*UPDATES):
            for q in range(r[B0], r[B0] + r[GY]):
                took.setdefault(int(L[q]), []).append((int(r[OP]), int(r[A0])))
        narrow_fused = any(r[GY] > 1 + r[A0] for r in of(FO_DIAG_TRSM))
        upd_fronts = [int(L[q]) for r in of(FO_GRP_FUSED) for q in range(r[B0], r[B0] + r[GX])] if (grouped and lv >= grp_cut) else [int(x) for x in L[b0:b1]]
        for sn in upd_fronts:
            if upd[sn] <= 0:
                continue
            got = sorted(took.get(sn, []))
            if narrow_fused:
                assert got == [] and grp_rem[sn] > 0
            else:
                assert len(got) == 1 or got == [(FO_SCHUR, 4), (FO_SCHUR_P1, 0)], (name, lv, sn, got)
        for r in of(FO_SCHUR, FO_SCHUR_P1):
            if sched == "single":
                assert np.all(order[L[r[B0]:r[B0] + r[GY]]] > 1024)
    in_sched = set(int(L[q]) for q in range(bucket(0, 0)[0], bucket(nl - 1, FC_BIG)[1]))
    want = {s for s in in_sched if cls[s] == FC_BIG and level[s] >= grp_cut} if grouped else set()
    assert set(grouped_fronts) == want and all(v == 1 for v in grouped_fronts.values())
    return recs


@pytest.mark.parametrize("system", list(TLP.SYSTEMS) + PATHFIX)
def test_single_gpu_schedules(system):
    s, sym, tune = analysed(system)
    with pathfix.knobs(None, tune):
        plan = functools.lru_cache(maxsize=None)(lambda what: s.launch_plan(what, 1, 0))
        full = check_list(sym, plan, "factor.single.full", "single", False)
        opt = check_list(sym, plan, "factor.single.opt", "single", True)
        # the optimistic schedule only leaves launches out or replaces the launches of whole levels
        assert len(opt) <= len(full)
        with pytest.raises(ipopt_amd.KKTError):
            s.launch_plan("factor.local", 1, 0)


@pytest.mark.parametrize("nranks", [2, 4])
@pytest.mark.parametrize("subcube", [0, 1])
def test_multi_rank_schedules(nranks, subcube):
    s, sym, _ = analysed("grid", nranks, subcube)
    ndepth = int(s.launch_plan("scalars", nranks, 0)[1])
    for rk in range(nranks):
        plan = functools.lru_cache(maxsize=None)(lambda what: s.launch_plan(what, nranks, rk))
        check_list(sym, plan, "factor.local", "local", False)
        for d in range(ndepth):
            recs = check_list(sym, plan, "factor.stage%d" % d, "stage%d" % d, False)
            assert np.all(recs[recs[:, OP] == FO_ASSEMBLE, A0] == 1) and not np.any(recs[:, OP] == FO_ASSEMBLE2)      # top_mode: the arena, never the fast assembly
        with pytest.raises(ipopt_amd.KKTError):
            s.launch_plan("factor.stage%d" % ndepth, nranks, rk)


def test_plan_and_schedules_on_the_cpu_under_sanitizers(tmp_path):
    """tests/support/factor_schedule_check.cpp with the host-only sources of the plan (they link without the HIP runtime) under ASan and UBSan: a grid KKT
    pattern analysed, planned and scheduled for one GPU and for both ranks of two, every record's indices checked against the arrays they index"""
    HOSTCHECK._run_host_program_under_sanitizers(tmp_path, "factor_schedule_check", ("launch_plan.cpp", "symbolic.cpp", "matching_scaling.cpp"))
