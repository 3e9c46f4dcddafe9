"""Host only (no device): what the fixtures of tests/test_gpu_small_fronts.py launch for their one-wavefront fronts (class FC_WAVE, order <= 32), leg by
leg -- the leaf chains and the data-flow runs of the optimistic factor schedule, the launches of both schedules counted from the exported plan, and per
level which instantiation of the pair kernels numeric.hip solve_level takes (tests/support/reach.py small_reach).  The shapes are pinned, so that a later
change of the ordering or of a threshold fails here instead of silently emptying the GPU test.

What each edge is for (kernels_fronts.hip.inc, kernels_solve.hip.inc, launch_plan.cpp):
  leaf chains of 1 .. 16 links, the 16-level cap     k_leaf_chain / k_*_leafchain walk `nlw` links, shorter chains of the wavefront idle      leaf_edges (1, 3, 5 .. 16), w8 (1 .. 6)
  15 / 13 chains: no multiple of four                the last wavefront's `cact`                                                              leaf_edges, leaf_edges_w8, band_hostile (16: a full one)
  links of > 48 input entries                        the remainder loop behind the three prefetched entries per lane of k_leaf_chain          leaf_edges (58), leaf_edges_w8 (up to 100)
  a link with k = 1, a root link with k = order      the masked elimination steps; no update rows, no contribution block                      leaf_edges
  a chain that goes on above level 15                the last link's block goes to memory for k_front_df                                      leaf_edges (two chains, 62 and 29 levels)
  fronts of order 17 .. 32 in a run, k on both       front_lds32_body; k_*_pair<32> with k > 16                                               wave_edges (k = 14 .. 17, 22, 30, 32), leaf_edges (20, 3)
  sides of 16, k = order = 32
  children of 15, 16, 17, 18 update rows under a     `tld = mc <= 16 ? 16 : 32` and the 256 / 1 024 slots of cbt_off                           wave_edges (18 squares of 16, 6 of 32)
  parent of the same run
  5 and 6 gathered children                          the loop over the children beyond the fourth in k_fwd_pair                               wave_edges ((30, 30, 5): five children of 18 rows; (8, 8, 6))
  every pair instantiation                           <16, 16> / <16> / <32>                                                                   leaf_edges [levels] 11 / 6 / 0, wave_edges [levels] 0 / 0 / 3
  rejected fronts at prescribed places               first / middle / last link of a leaf chain; fronts inside k_front_df                      leaf_reject, wave_reject
  2x2 pivots in many small fronts at once            the strict kernel behind k_front_dpp16 at u = 0.01                                        band_hostile (14 in the specification)

Where the fixtures differ from their first drafts, and why (host analysis):
  * a tiny entry of the MATRIX is a tiny pivot only in a leaf front (one child's contribution moves the diagonal by O(1)): the reject fixtures choose the
    diagonal so that the pivot is 1e-6 in its front AS ASSEMBLED (smallfix.with_tiny_pivots); then the specification reorders exactly the prescribed fronts;
  * the default ordering merges every front with k = 2 into its parent: wave_reject makes all THREE pivots of a front (8, 3) tiny instead, and the front
    with k = 2 whose both pivots are tiny sits in the data-flow run of leaf_reject (level 20 of the long chain) -- a 2x2 pivot in either;
  * a second chain of 29 levels in leaf_edges: with one front per level above level 14, MI355X_KKT_TUNE=chain_solve_maxc=1 leaves a chain segment that
    starts inside the leaf-chain prefix, and k_*_leafchain is not launched; its cliques of 20 give the fronts (20, 3) that make k_*_pair<16> levels;
  * leaf_edges_w8 also drops the component whose first front under max_sn_cols=8 is (20, 8) on level 0;
  * wave_edges has a third level (a front (32, 22) with a child and a parent in the run, for wave_reject);
  * band_hostile: hostile_band_kkt(300, seed=2, frac=0.15, tiny=1e-2).  With the generator's defaults (frac 0.3, tiny 1e-6) static pivoting at u = 0.01
    without delays forces zero pivots at every n tried up to 400 (the specification's own error: 1e-6 .. 1e4); n = 300 is the smallest tried at which
    the data-flow run holds a front of order 17 .. 32 beside more than ten 2x2 pivots."""
import functools

import numpy as np
import pytest

from tests.support import reach as R, smallfix as X

STRUCT = {"leaf_reject": "leaf_edges", "wave_reject": "wave_edges"}      # an edit of values: the plan is the unedited fixture's

# fixture -> the pinned facts, as analysed when the fixtures were written.  lc: (levels, chains) of the leaf chains; chain_lengths: (links, chains);
# df_runs: (first level, last level, virtual workgroups); tagged: contribution squares of (16, 32) columns; shapes: (order, k, children)
EXPECT = {
    "leaf_edges": dict(n=530, neg=2, num_sn=186, num_levels=62, lc=(16, 15), chain_lengths=[(1, 3), (3, 2), (5, 1), (7, 1), (8, 1), (9, 1), (11, 1), (12, 1), (15, 2), (16, 2)],
        df_runs=[(16, 61, 52)], df_fronts_17_32=6, tagged=(58, 3), tagged_rows=[2, 4, 5, 7, 8, 10, 11, 13, 14, 17], link_max_entries=58, max_gathered=1, wave_k_over_16=0,
        shapes=[(1, 1, 0), (2, 2, 0), (2, 2, 1), (3, 3, 0), (3, 3, 1), (4, 3, 1), (4, 4, 1), (5, 3, 1), (5, 4, 0), (6, 2, 1), (6, 3, 1), (7, 2, 1), (7, 3, 1), (7, 4, 0), (8, 3, 1), (9, 3, 0), (9, 3, 1), (10, 2, 1), (10, 3, 0), (10, 3, 1), (11, 3, 1), (12, 3, 0), (12, 3, 1), (13, 3, 1), (14, 3, 0), (14, 3, 1), (16, 3, 0), (16, 3, 1), (16, 4, 0), (16, 4, 1), (17, 3, 1), (20, 3, 1)]),
    "leaf_edges_w8": dict(n=476, neg=0, num_sn=75, num_levels=22, lc=(6, 13), chain_lengths=[(1, 3), (2, 2), (3, 1), (4, 1), (5, 1), (6, 5)],
        df_runs=[(6, 21, 19)], df_fronts_17_32=3, tagged=(22, 0), tagged_rows=[2, 6, 8, 9, 13], link_max_entries=100, max_gathered=1, wave_k_over_16=0,
        shapes=[(1, 1, 0), (2, 2, 0), (2, 2, 1), (3, 3, 0), (3, 3, 1), (5, 4, 0), (5, 5, 1), (6, 6, 1), (7, 4, 0), (7, 7, 1), (9, 5, 0), (9, 5, 1), (9, 7, 1), (9, 8, 1), (10, 5, 0), (10, 5, 1), (10, 7, 1), (12, 6, 0), (12, 6, 1), (12, 7, 1), (13, 5, 1), (13, 7, 1), (16, 7, 0), (16, 7, 1), (16, 8, 0), (16, 8, 1), (20, 7, 1)]),
    "wave_edges": dict(n=657, neg=0, num_sn=38, num_levels=3, lc=(0, 0), chain_lengths=[],
        df_runs=[(0, 2, 33)], df_fronts_17_32=30, tagged=(18, 6), tagged_rows=[3, 5, 8, 9, 10, 15, 16, 17, 18], link_max_entries=0, max_gathered=6, wave_k_over_16=14,
        shapes=[(8, 3, 0), (8, 8, 6), (10, 7, 0), (16, 16, 1), (17, 17, 0), (17, 17, 1), (18, 18, 1), (20, 10, 0), (20, 15, 0), (24, 14, 0), (24, 16, 0), (25, 16, 0), (30, 30, 5), (32, 14, 0), (32, 15, 0), (32, 16, 0), (32, 17, 0), (32, 22, 1), (32, 32, 0), (32, 32, 1), (32, 32, 2), (32, 32, 3)]),
    "band_hostile": dict(n=598, neg=298, num_sn=57, num_levels=8, lc=(3, 16), chain_lengths=[(2, 3), (3, 13)],
        df_runs=[(3, 7, 7)], df_fronts_17_32=1, tagged=(11, 0), tagged_rows=[2, 4], link_max_entries=39, max_gathered=5, wave_k_over_16=0,
        shapes=[(4, 2, 2), (6, 2, 2), (6, 4, 1), (8, 4, 3), (8, 8, 5), (9, 7, 0), (10, 8, 1), (14, 10, 1), (15, 13, 2), (16, 12, 0), (16, 12, 1), (16, 14, 2), (18, 16, 3)]),
}
EXPECT["leaf_reject"] = dict(EXPECT["leaf_edges"], neg=6)
EXPECT["wave_reject"] = dict(EXPECT["wave_edges"], neg=4)
# (fixture, leg) -> launches of (FO_LEAF_CHAIN, FO_FRONT_DF, FO_FRONT_DPP16, FO_REG_64_4, FO_REG_64_2) in factor.single.full and factor.single.opt; levels
# solved by (k_*_pair<16, 16>, k_*_pair<16>, k_*_pair<32>, k_fwd<64> / k_bwd<64>); levels of the k_*_leafchain prefix; levels inside chain segments.
# The `full` leg is the `levels` plan: MI355X_KKT_DISABLE=optimistic only makes factor() walk factor.single.full
EXPECT_LEG = {
    ("leaf_edges", "default"): dict(full=(0, 0, 62, 62, 0), opt=(1, 1, 0, 0, 0), solve=(0, 0, 0, 0), leafchain_solve=0, seg_levels=62),
    ("leaf_edges", "levels"): dict(full=(0, 0, 62, 62, 0), opt=(1, 1, 0, 0, 0), solve=(11, 6, 0, 0), leafchain_solve=16, seg_levels=29),
    ("leaf_edges", "nopair"): dict(full=(0, 0, 62, 62, 0), opt=(1, 1, 0, 0, 0), solve=(0, 0, 0, 33), leafchain_solve=0, seg_levels=29),
    ("leaf_edges", "noleaf"): dict(full=(0, 0, 62, 62, 0), opt=(0, 1, 0, 0, 0), solve=(27, 6, 0, 0), leafchain_solve=0, seg_levels=29),
    ("leaf_edges", "nodf"): dict(full=(0, 0, 62, 62, 0), opt=(0, 0, 62, 6, 0), solve=(27, 6, 0, 0), leafchain_solve=0, seg_levels=29),
    ("leaf_edges", "strict"): dict(full=(0, 0, 0, 62, 0), opt=(0, 0, 0, 62, 0), solve=(27, 6, 0, 0), leafchain_solve=0, seg_levels=29),
    ("leaf_edges", "full"): dict(full=(0, 0, 62, 62, 0), opt=(1, 1, 0, 0, 0), solve=(11, 6, 0, 0), leafchain_solve=16, seg_levels=29),
    ("leaf_edges_w8", "default"): dict(full=(0, 0, 22, 22, 0), opt=(1, 1, 0, 0, 0), solve=(0, 0, 0, 0), leafchain_solve=0, seg_levels=22),
    ("leaf_edges_w8", "levels"): dict(full=(0, 0, 22, 22, 0), opt=(1, 1, 0, 0, 0), solve=(4, 3, 0, 0), leafchain_solve=6, seg_levels=9),
    ("leaf_edges_w8", "nopair"): dict(full=(0, 0, 22, 22, 0), opt=(1, 1, 0, 0, 0), solve=(0, 0, 0, 13), leafchain_solve=0, seg_levels=9),
    ("leaf_edges_w8", "noleaf"): dict(full=(0, 0, 22, 22, 0), opt=(0, 1, 0, 0, 0), solve=(10, 3, 0, 0), leafchain_solve=0, seg_levels=9),
    ("leaf_edges_w8", "nodf"): dict(full=(0, 0, 22, 22, 0), opt=(0, 0, 22, 3, 0), solve=(10, 3, 0, 0), leafchain_solve=0, seg_levels=9),
    ("leaf_edges_w8", "strict"): dict(full=(0, 0, 0, 22, 0), opt=(0, 0, 0, 22, 0), solve=(10, 3, 0, 0), leafchain_solve=0, seg_levels=9),
    ("wave_edges", "default"): dict(full=(0, 0, 2, 3, 0), opt=(0, 1, 0, 0, 0), solve=(0, 0, 0, 0), leafchain_solve=0, seg_levels=3),
    ("wave_edges", "levels"): dict(full=(0, 0, 2, 3, 0), opt=(0, 1, 0, 0, 0), solve=(0, 0, 3, 0), leafchain_solve=0, seg_levels=0),
    ("wave_edges", "nopair"): dict(full=(0, 0, 2, 3, 0), opt=(0, 1, 0, 0, 0), solve=(0, 0, 0, 3), leafchain_solve=0, seg_levels=0),
    ("wave_edges", "noleaf"): dict(full=(0, 0, 2, 3, 0), opt=(0, 1, 0, 0, 0), solve=(0, 0, 3, 0), leafchain_solve=0, seg_levels=0),
    ("wave_edges", "nodf"): dict(full=(0, 0, 2, 3, 0), opt=(0, 0, 2, 3, 0), solve=(0, 0, 3, 0), leafchain_solve=0, seg_levels=0),
    ("wave_edges", "strict"): dict(full=(0, 0, 0, 3, 0), opt=(0, 0, 0, 3, 0), solve=(0, 0, 3, 0), leafchain_solve=0, seg_levels=0),
    ("wave_edges", "full"): dict(full=(0, 0, 2, 3, 0), opt=(0, 1, 0, 0, 0), solve=(0, 0, 3, 0), leafchain_solve=0, seg_levels=0),
    ("band_hostile", "default"): dict(full=(0, 0, 8, 8, 0), opt=(1, 1, 0, 0, 0), solve=(0, 0, 0, 0), leafchain_solve=0, seg_levels=8),
    ("band_hostile", "levels"): dict(full=(0, 0, 8, 8, 0), opt=(1, 1, 0, 0, 0), solve=(2, 1, 0, 0), leafchain_solve=3, seg_levels=2),
    ("band_hostile", "nopair"): dict(full=(0, 0, 8, 8, 0), opt=(1, 1, 0, 0, 0), solve=(0, 0, 0, 6), leafchain_solve=0, seg_levels=2),
    ("band_hostile", "noleaf"): dict(full=(0, 0, 8, 8, 0), opt=(0, 1, 0, 0, 0), solve=(5, 1, 0, 0), leafchain_solve=0, seg_levels=2),
    ("band_hostile", "nodf"): dict(full=(0, 0, 8, 8, 0), opt=(0, 0, 8, 1, 0), solve=(5, 1, 0, 0), leafchain_solve=0, seg_levels=2),
    ("band_hostile", "strict"): dict(full=(0, 0, 0, 8, 0), opt=(0, 0, 0, 8, 0), solve=(5, 1, 0, 0), leafchain_solve=0, seg_levels=2),
}
# the specification's statistics (num_neg, num_zero, num_two, num_delay) and the supernodes it reorders, with the static-order paths and (strict) without
SPEC = {
    "leaf_edges": ((2, 0, 0, 0), (), (2, 0, 0, 0)), "leaf_edges_w8": ((0, 0, 0, 0), (), (0, 0, 0, 0)), "wave_edges": ((0, 0, 0, 0), (), (0, 0, 0, 0)),
    "leaf_reject": ((6, 0, 1, 0), (30, 52, 125, 136), (6, 0, 1, 0)), "wave_reject": ((4, 0, 1, 0), (8, 34, 36), (4, 0, 1, 0)),
    "band_hostile": ((298, 0, 14, 0), (3, 5, 9, 15, 20, 28, 36, 39, 54, 56), (298, 0, 23, 0)),
}
ALL_LEGS = [(name, leg) for name in X.FIXTURES for leg in X.FIXTURES[name][3]]


@functools.lru_cache(maxsize=None)
def facts(name, leg):
    with X.leg_knobs(leg):
        s = X.handle(name)
        F = R.small_reach(s)
        s.close()
    return F


def summary(F):
    """the facts that are pinned per fixture"""
    return dict(n=F["n"], num_sn=F["num_sn"], num_levels=F["num_levels"], lc=(F["lc_levels"], F["lc_nchains"]), chain_lengths=F["chain_lengths"], df_runs=F["df_runs"],
                df_fronts_17_32=F["df_fronts_17_32"], tagged=(F["tagged16"], F["tagged32"]), tagged_rows=F["tagged_rows"], link_max_entries=F["link_max_entries"],
                max_gathered=F["max_gathered"], wave_k_over_16=F["wave_k_over_16"], shapes=F["shapes"])


def leg_summary(F):
    c = F["solve_level_counts"]
    return dict(full=F["full"], opt=F["opt"], solve=(c["16x16"], c["16"], c["32"], c["k64"]), leafchain_solve=F["leafchain_solve"], seg_levels=F["seg_levels"])


@pytest.mark.parametrize("fixture", sorted(X.FIXTURES))
def test_pinned_fixture_facts(fixture):
    S = X.system(fixture)
    F = facts(fixture, "default")
    got = dict(summary(F), neg=S["neg"])
    print(f"{fixture}: " + "".join(f"\n    {k} = {v!r}" for k, v in got.items()))
    assert got == EXPECT[fixture]
    assert S["n"] <= 1000 and F["classes"] == [R.FC_WAVE] and F["wave_fronts"] == F["num_sn"]      # every front is a one-wavefront front


@pytest.mark.parametrize("fixture,leg", ALL_LEGS)
def test_pinned_launches_of_a_leg(fixture, leg):
    F = facts(fixture, leg)
    got = leg_summary(F)
    print(f"{fixture} [{leg}]: {got!r} pair32 fronts with k > 16: {F['pair32_k_over_16']}")
    assert got == EXPECT_LEG[STRUCT.get(fixture, fixture), leg]
    assert F["shapes"] == facts(fixture, "default")["shapes"]      # the knobs change what is launched, not the fronts
    lc, df, dpp, reg4, reg2 = F["opt"]
    if leg in ("default", "levels", "nopair", "full"):           # the optimistic schedule is leaf chains + data-flow runs and nothing strict
        assert df == len(F["df_runs"]) >= 1 and lc == (1 if F["lc_levels"] else 0) and (dpp, reg4, reg2) == (0, 0, 0)
    if leg == "noleaf":
        assert lc == 0 and df == 1 and (dpp, reg4) == (0, 0) and F["lc_levels"] == 0 and F["df_runs"][0][:2] == (0, F["num_levels"] - 1)      # the run starts at level 0
    if leg == "nodf":                                            # per level: k_front_dpp16, and the strict kernel where a front of order 17 .. 32 sits
        assert (lc, df) == (0, 0) and dpp == F["full"][2] > 0
    if leg == "strict":
        assert F["full"] == F["opt"] and F["opt"][:3] == (0, 0, 0) and reg4 == F["num_levels"]
    if leg != "default":
        assert sum(got["solve"]) + got["leafchain_solve"] + got["seg_levels"] == F["num_levels"]
    if leg == "default":
        assert got["seg_levels"] == F["num_levels"]              # the chain sweeps take every level
    if leg == "nopair":
        assert got["solve"][:3] == (0, 0, 0) and got["solve"][3] > 0 and not F["pair_solve"]


def test_the_fixtures_together_reach_every_edge():
    L = {(name, leg): facts(name, leg) for name, leg in ALL_LEGS}
    # every instantiation of the pair kernels on some level of some leg, k > 16 in k_*_pair<32>, k_fwd<64> / k_bwd<64> without them
    for inst in ("16x16", "16", "32", "k64"):
        assert any(F["solve_level_counts"][inst] > 0 for F in L.values()), inst
    assert L["wave_edges", "levels"]["pair32_k_over_16"] == 14
    assert L["wave_edges", "levels"]["max_gathered_on_levels"] == 6 > 4
    # leaf chains: the cap, one link and sixteen, a last wavefront that is not full, the remainder loop, the solve kernels of the chains
    D = {name: L[name, "default"] for name in X.FIXTURES}
    assert D["leaf_edges"]["lc_levels"] == 16 and D["leaf_edges"]["num_levels"] > 16
    lengths = dict(D["leaf_edges"]["chain_lengths"])
    assert lengths[1] == 3 and lengths[16] == 2 and len(lengths) == 10
    assert D["leaf_edges"]["lc_nchains"] % 4 == 3 and D["leaf_edges_w8"]["lc_nchains"] % 4 == 1 and D["band_hostile"]["lc_nchains"] % 4 == 0
    assert D["leaf_edges"]["links_over_48_entries"] == 3 and D["leaf_edges"]["link_max_entries"] == 58
    assert D["leaf_edges_w8"]["links_over_48_entries"] == 25 and D["leaf_edges_w8"]["link_max_entries"] == 100 > 96      # (more than one turn of the remainder loop: 48 + 3 x 16 < 100)
    assert (1, 1) in D["leaf_edges"]["link_shapes"] and D["leaf_edges"]["root_links_k_eq_order"] >= 1
    assert any(k == 1 for _, k in D["leaf_edges"]["link_shapes"])
    for name in ("leaf_edges", "leaf_edges_w8", "leaf_reject", "band_hostile"):
        assert L[name, "levels"]["leafchain_solve"] == D[name]["lc_levels"] > 0
    # data-flow runs: both sizes of the tagged square and their edge, a parent of 17 .. 32 rows with five such children, six gathered children
    W = D["wave_edges"]
    assert {15, 16, 17, 18} <= set(W["tagged_rows"]) and W["tagged16"] > 0 and W["tagged32"] > 0
    assert W["tagged_parents_17_32_children"] == 5 and W["df_max_gathered"] == 6 and W["max_children"] == 6
    assert (32, 32, 0) in W["shapes"] and {(32, 15, 0), (32, 16, 0), (32, 17, 0), (17, 17, 0), (30, 30, 5), (8, 8, 6)} <= set(W["shapes"])
    assert W["df_runs"] == [(0, 2, 33)] and W["df_fronts_17_32"] == 30
    assert D["leaf_edges"]["df_runs"][0][0] == 16 and D["leaf_edges"]["df_fronts_17_32"] == 6 and D["leaf_edges"]["tagged32"] == 3      # a chain goes on in the run, with fronts of 20 rows


MIDDLE_NEIGHBOURS = {}      # edited variable of a middle link -> (its position in the chain, the lengths of the four chains of its wavefront, how many others are still walking there)


def kinds(name):
    """the kind of front every edited variable of a reject fixture sits in, from the analysis"""
    S = X.system(name)
    tiny = X.LEAF_TINY if name == "leaf_reject" else X.WAVE_TINY
    with X.leg_knobs("default"):
        s = X.handle(name)
        T = X.fronts(s)
        lcf, ptr, runs = s.launch_plan("lc_fronts").copy(), s.launch_plan("lc_ptr").copy(), s.launch_plan("df_runs").reshape(-1, 5).copy()
        s.close()
    nsn = len(T["cols"])
    nchild = np.bincount(T["parent"][T["parent"] >= 0], minlength=nsn)
    link = {}
    for ci in range(len(ptr) - 1):
        for pos, f in enumerate(lcf[ptr[ci]:ptr[ci + 1]]):
            link[int(f)] = (ci, pos, int(ptr[ci + 1] - ptr[ci]))
    in_run = lambda f: f >= 0 and any(r[0] <= T["level"][f] <= r[1] for r in runs)
    variables = sorted(tiny)
    of = X.front_of(T, variables)
    edited_chains = {link[f][0] for f in of if f in link}
    out = {}
    for x, f in zip(variables, of):
        order, k, pa = int(T["order"][f]), int(T["cols"][f]), int(T["parent"][f])
        mine = [y for y, g in zip(variables, of) if g == f]
        first = int(T["perm"][T["colptr"][f]]) == x              # the first pivot of its front
        if f in link:
            ci, pos, ln = link[f]
            group = range(4 * (ci // 4), 4 * (ci // 4) + 4)      # the four chains of its wavefront: none of the others edited, and some still walking at this link
            alone = 4 * (ci // 4) + 4 <= len(ptr) - 1 and all(c == ci or c not in edited_chains for c in group)
            if alone and 0 < pos < ln - 1:
                walking = [c for c in group if c != ci and ptr[c + 1] - ptr[c] > pos]
                assert len(walking) >= 1, "the rejected middle link has no active chain beside it"
                MIDDLE_NEIGHBOURS[x] = (pos, [int(ptr[c + 1] - ptr[c]) for c in group], len(walking))
            kind = "first" if pos == 0 and ln > 1 else "last" if pos == ln - 1 and ln > 1 else "middle" if alone else "middle, but its wavefront is not otherwise healthy"
            assert first
        elif len(mine) == k == 2 and in_run(f) and in_run(pa) and nchild[f] == 1:
            kind = "df_two"
        elif len(mine) == k == 3 and in_run(f) and in_run(pa):
            kind = "all_three"
        elif order <= 16 and in_run(f) and in_run(pa):
            kind = "small"; assert first
        elif order > 16 and in_run(f) and in_run(pa) and nchild[f] >= 1:
            kind = "wave"; assert first
        else:
            kind = "?"
        out[x] = (kind, f)
    return out, S


@pytest.mark.parametrize("fixture", ["leaf_reject", "wave_reject"])
def test_reject_fixtures_put_tiny_pivots_where_prescribed(fixture):
    tiny = X.LEAF_TINY if fixture == "leaf_reject" else X.WAVE_TINY
    got, S = kinds(fixture)
    print(f"{fixture}: " + ", ".join(f"variable {x}: {k} (supernode {f})" for x, (k, f) in got.items()))
    assert {x: k for x, (k, f) in got.items()} == tiny
    if fixture == "leaf_reject":      # link 3 of a chain of 7 beside chains of 3 (ended), 15 and 12 links (walking): `alive = false` next to active rows of the wavefront
        assert MIDDLE_NEIGHBOURS == {388: (3, [3, 15, 7, 12], 2)}
    # an edit of values: the analysis is the unedited fixture's under the same options, front for front
    with X.leg_knobs("default"):
        a, b = X.handle(fixture), X.handle(S["base"], opts_of=fixture)
        Ta, Tb = X.fronts(a), X.fronts(b)
        a.close(); b.close()
    assert all(np.array_equal(Ta[k], Tb[k]) for k in Ta)
    K, K0 = S["K"].toarray(), X.system(S["base"])["K"].toarray()
    D = K - K0
    assert np.count_nonzero(D) == len(tiny) and all(D[x, x] != 0.0 for x in tiny)
    # the pivots are tiny as assembled, and the specification leaves its natural order in exactly these fronts -- a 2x2 pivot among them
    stats, odd, _ = X.spec(fixture)
    assert set(odd) == {f for _, f in got.values()} and stats[2] == 1 and stats[1] == 0
    touched = X.touched(Ta, sorted(tiny))
    assert touched.sum() < len(touched) // 2                     # most fronts are compared bitwise with the unedited run


@pytest.mark.parametrize("fixture", sorted(X.FIXTURES))
def test_reference_is_not_hidden_by_conditioning(fixture):
    """plain fp64 LAPACK within 1e-9 of the refined reference (measured: 7.8e-16 .. 2.4e-15 on the unedited fixtures and band_hostile, 1.8e-13 on leaf_reject,
    8.3e-13 on wave_reject); the inertia by LAPACK's eigenvalues; the specification's statistics and its own error against the reference (6.7e-16 ..
    1.5e-14): no zero pivot anywhere, 2x2 pivots where they were prescribed"""
    S = X.system(fixture)
    e = X.e_plain(fixture)
    stats, odd, _ = X.spec(fixture)
    strict, odd_strict, _ = X.spec(fixture, False)
    print(f"{fixture}: n {S['n']} inertia {S['neg']} e_plain {e:.2e} tol_f {X.tol_f(fixture):.2e} bound {X.fwd_bound(fixture):.2e} specification: (neg, zero, two, delay) {stats} "
          f"error {X.spec_error(fixture):.2e} reordered {odd}; strict rule {strict}, {len(odd_strict)} reordered")
    assert e <= 1e-9
    assert X.reference(fixture)[2] == S["neg"] == stats[0] == strict[0]
    assert 1e-12 <= X.tol_f(fixture) <= 1e-7 and X.tol_f(fixture) <= X.fwd_bound(fixture) <= 1e-7
    assert (stats, odd, strict) == SPEC[fixture]
    assert stats[1] == strict[1] == 0
    if fixture in ("leaf_reject", "wave_reject", "band_hostile"):
        assert stats[2] > 0 and strict[2] > 0
    assert X.spec_error(fixture) <= 1e-12
