"""The launch plan on the host (launch_plan.cpp through mi355x_kkt_get_launch_plan, no device): the schedule the factorisation and the solves
run, checked against the symbolic structure it is built from -- for the single-GPU plan and for every rank of 2 / 4 / 8-rank worlds under both
mappings, on synthetic systems and on recorded ones."""
import os

import numpy as np
import pytest

import ipopt_amd
from tests.support import kktgen, mirror

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FC_WAVE, FC_LDS64, FC_LDS128, FC_BIG, FC_COUNT = 0, 1, 2, 3, 4

SYSTEMS = {
    "lukvl_like": lambda: kktgen.lukvl_like(3000, seed=3),
    "grid": lambda: kktgen.grid_kkt(40, 36, dof=2, ncon=1, seed=7),
    "lukvle1_10000": lambda: kktgen.recorded_kkt(os.path.join(GOLD, "lukvle1_10000.kktrec"), which=0),
    "mbndry1_100": lambda: kktgen.recorded_kkt(os.path.join(GOLD, "mbndry1_100.kktrec"), which=0),
    "mbndry3d_14": lambda: kktgen.recorded_kkt(os.path.join(GOLD, "mbndry3d_14.kktrec"), which=0),
}


def analysed(system, nranks=1, subcube=0):
    n, r, c, v, _ = SYSTEMS[system]()
    s = ipopt_amd.KKTSolver(nranks=nranks, subcube=subcube)
    s.initialize_structure(n, r, c, vals=v)
    sym = mirror.fetch(s)
    I = sym["info"]
    sym["level_ptr"] = s.symbolic(13, I.num_levels * FC_COUNT + 1)
    sym["level_sn"] = s.symbolic(14, I.num_sn)
    sym["grp_rem"] = s.symbolic(16, I.num_sn)
    sym["alias"] = s.symbolic(17, I.num_sn)
    sym["order"] = np.diff(sym["rowptr"])
    sym["cols"] = np.diff(sym["colptr"])
    return s, sym


def plan_of(s, nranks, rank):
    return lambda what: s.launch_plan(what, nranks, rank)


def check_sched(sym, plan, name, L, mine):
    """buckets (level, class) hold exactly the schedule's fronts; the solve units are its group-last BIG fronts (every BIG front with per-link solves)"""
    nl = sym["info"].num_levels
    ptr, base = plan(name + ".ptr"), int(plan(name + ".base")[0])
    last0, last1 = plan(name + ".last0"), plan(name + ".last1")
    level, cls, grp_rem = sym["level"], sym["cls"], sym["grp_rem"]
    for lv in range(nl):
        for fc in range(FC_COUNT):
            b = lv * FC_COUNT + fc
            got = sorted(L[base + ptr[b]: base + ptr[b + 1]].tolist())
            want = [s for s in range(len(level)) if level[s] == lv and cls[s] == fc and mine(s)]
            assert got == want, (name, lv, fc)
        units = L[last0[lv]:last1[lv]].tolist()
        big = [s for s in range(len(level)) if level[s] == lv and cls[s] == FC_BIG and mine(s)]
        assert units in ([s for s in big if grp_rem[s] == 0], big), (name, lv)
        assert 0 <= last0[lv] <= last1[lv] <= len(L)


@pytest.mark.parametrize("system", list(SYSTEMS))
def test_single_gpu_plan(system):
    s, sym = analysed(system)
    plan = plan_of(s, 1, 0)
    L = plan("level_list")
    nl, nsn = sym["info"].num_levels, sym["info"].num_sn
    lp, order, level, cls, parent = sym["level_ptr"], sym["order"], sym["level"], sym["cls"], sym["parent"]
    assert np.array_equal(plan("single.ptr"), lp) and int(plan("single.base")[0]) == 0
    check_sched(sym, plan, "single", L, lambda s_: True)
    # the WAVE, LDS128 and BIG buckets are sorted by front order; the splits count the leading fronts of order <= 16, <= 96, <= 1024
    tiny16, tiny_split, mid_split, big_split = plan("tiny16"), plan("tiny_split"), plan("mid_split"), plan("big_split")
    for lv in range(nl):
        for fc, lim in ((FC_WAVE, 16), (FC_LDS128, 96), (FC_BIG, 1024)):
            o = order[L[lp[lv * FC_COUNT + fc]: lp[lv * FC_COUNT + fc + 1]]]
            assert np.all(np.diff(o) >= 0), (lv, fc)
            lead = int(np.sum(o <= lim))
            if fc == FC_WAVE:
                assert tiny16[lv] == lead and tiny_split[lv] == (lead if lead >= 2048 else 0)
            elif fc == FC_LDS128:
                assert mid_split[lv] == (lead if lead >= 256 else 0)
            else:
                assert big_split[lv] == lead
    scal = plan("scalars")
    lc_levels, lc_nchains = int(scal[2]), int(scal[3])
    # leaf chains: every WAVE front below lc_levels exactly once, each chain a leaf-to-parent walk
    if lc_levels > 0:
        ptr, fr = plan("lc_ptr"), plan("lc_fronts")
        assert len(ptr) == lc_nchains + 1
        assert sorted(fr.tolist()) == [x for x in range(nsn) if level[x] < lc_levels]
        assert all(cls[x] == FC_WAVE for x in fr)
        for c in range(lc_nchains):
            ch = fr[ptr[c]:ptr[c + 1]]
            assert len(ch) >= 1 and level[ch[0]] == 0
            assert all(parent[ch[i]] == ch[i + 1] for i in range(len(ch) - 1))
            assert parent[ch[-1]] < 0 or level[parent[ch[-1]]] >= lc_levels
    # k_front_df runs: disjoint runs of >= 2 levels at or above lc_levels, every level pure WAVE
    runs = plan("df_runs").reshape(-1, 5)
    seen = set()
    for lv0, lv1, tab0, nlev, nq in runs:
        assert lv1 > lv0 >= lc_levels and nlev == lv1 - lv0 + 1 and nq > 0
        for lv in range(lv0, lv1 + 1):
            assert lv not in seen
            seen.add(lv)
            assert lp[lv * FC_COUNT + 1] > lp[lv * FC_COUNT] and lp[lv * FC_COUNT + 1] == lp[lv * FC_COUNT + FC_COUNT]
    check_chain_segments(sym, plan)


def check_chain_segments(sym, plan, maxc=128):
    lp, alias, level = sym["level_ptr"], sym["alias"], sym["level"]
    segs = plan("chain_segs").reshape(-1, 9)
    links = plan("chain_links").reshape(-1, 4)
    descs = plan("chain_descs").reshape(-1, 6)
    for lv0, lv1, desc0, ndesc, *_ in segs:
        fronts = [int(s) for lv in range(lv0, lv1 + 1) for s in sym["level_sn"][lp[lv * FC_COUNT]: lp[lv * FC_COUNT + FC_COUNT]]]
        for lv in range(lv0, lv1 + 1):
            assert 0 < lp[lv * FC_COUNT + FC_COUNT] - lp[lv * FC_COUNT] <= maxc
        in_chains = []
        for d in range(desc0, desc0 + ndesc):
            link0, nlinks = descs[d][0], descs[d][1]
            ch = links[link0:link0 + nlinks]
            assert np.all(ch[:, 3] == np.arange(link0, link0 + nlinks))        # a link's flag slot is its position
            assert ch[0, 0] == descs[d][4] and np.sum(ch[:, 1]) == descs[d][3]
            for i in range(1, nlinks):
                assert alias[ch[i, 0]] == ch[i - 1, 0] and ch[i, 2] == ch[i - 1, 2] + ch[i - 1, 1]
            in_chains += ch[:, 0].tolist()
        assert sorted(in_chains) == sorted(fronts)
        assert all(sym["cols"][s] <= 64 for s in fronts)


@pytest.mark.parametrize("system", ["grid", "mbndry1_100", "mbndry3d_14"])
@pytest.mark.parametrize("nranks", [2, 4, 8])
@pytest.mark.parametrize("subcube", [0, 1])
def test_multi_rank_plans(system, nranks, subcube):
    s, sym = analysed(system, nranks, subcube)
    nsn = sym["info"].num_sn
    own, glo, gsz, gd, parent, order = sym["owner"], sym["glo"], sym["gsz"], sym["gdepth"], sym["parent"], sym["order"]
    ndepth = int(s.launch_plan("scalars", nranks, 0)[1])
    local_cnt = np.zeros(nsn, dtype=int)
    stage_ranks = {}
    join_fronts = set()
    for rk in range(nranks):
        plan = plan_of(s, nranks, rk)
        L = plan("level_list")
        check_sched(sym, plan, "single", L, lambda s_: True)
        check_sched(sym, plan, "local", L, lambda s_: own[s_] == rk)
        b, p = int(plan("local.base")[0]), plan("local.ptr")
        for x in L[b:b + p[-1]]:
            local_cnt[x] += 1
        for d in range(ndepth):
            held = lambda s_: own[s_] < 0 and glo[s_] <= rk < glo[s_] + gsz[s_] and gd[s_] == d
            check_sched(sym, plan, "stage%d" % d, L, held)
            b, p = int(plan("stage%d.base" % d)[0]), plan("stage%d.ptr" % d)
            for x in L[b:b + p[-1]]:
                stage_ranks.setdefault(int(x), []).append(rk)
        # join lists: kind 0 = the parents of this rank's crossing subtree roots, kind 1 + d = of the crossing fronts of its depth-d range it reports
        crosses = lambda c: parent[c] >= 0 and own[parent[c]] < 0 and not (own[c] < 0 and (glo[c], gsz[c]) == (glo[parent[c]], gsz[parent[c]]))
        J = plan("join").reshape(-1, 4)
        assert len(J) == ndepth + 1
        for kind, (base, count, maxm, who) in enumerate(J):
            lst = L[base:base + count].tolist()
            want = sorted({int(parent[c]) for c in range(nsn) if crosses(c) and
                           (own[c] == rk if kind == 0 else (own[c] < 0 and gd[c] == kind - 1 and glo[c] == rk))})
            assert lst == want and who == rk + nranks * kind
            assert maxm == (max(order[lst]) if lst else 0)
            join_fronts.update(lst)
        check_chain_segments(sym, plan)
    # the local schedules partition the owned fronts; every replicated front is in the stage schedule of exactly the ranks of its range
    assert np.all(local_cnt[own >= 0] == 1) and np.all(local_cnt[own < 0] == 0)
    for x in range(nsn):
        if own[x] < 0:
            assert stage_ranks.get(x, []) == list(range(glo[x], glo[x] + gsz[x])), x
        else:
            assert x not in stage_ranks
    # the join fronts are the arena squares of the exchange layout, whose sizes comm_plan's all-reduces carry
    ex = s.launch_plan("exchange", nranks, 0).reshape(-1, 5)
    m = order[sorted(join_fronts)].astype(np.int64)
    assert int(ex[:, 3].sum()) == int((m * (m + 1) // 2).sum())
    for rk in range(nranks):
        mine = [e for e in ex if e[1] <= rk < e[1] + e[2]]
        arena = sorted((int(d), int(cnt)) for what, d, col, g, cnt, dt in s.comm_plan(rk, True) if what == 1)
        assert arena == sorted((int(e[0]), int(e[3])) for e in mine if e[3] > 0)
