"""Host only (no device): which kernel paths the fixtures of the GPU suite REACH (tests/support/reach.py over get_symbolic / get_launch_plan), and that
every MI355X_KKT_DISABLE switch of tests/test_gpu_fast_paths.py changes the launch plan -- its tables, or the exported factor schedule that the
device walks record by record -- on the fixture it is tested on; where a switch acts inside a kernel, the structural precondition of its path.  A fixture on which a knob changes nothing is no test of it: a later change of the
ordering or of a threshold fails here instead of silently emptying a GPU test."""
import functools

import numpy as np
import pytest

import ipopt_amd
from tests.support import pathfix, reach as R


@functools.lru_cache(maxsize=None)
def analysed(name):
    S = pathfix.system(name)
    with pathfix.knobs(None, S["tune"]):
        s = ipopt_amd.KKTSolver(**S["opts"])
        s.initialize_structure(S["n"], S["r"], S["c"], vals=S["v"])
    return s


def facts(name, disable=None):
    S = pathfix.system(name)
    s = analysed(name)
    with pathfix.knobs(disable, S["tune"]):
        return R.reach(s), R.plan_arrays(s)


# fixture -> the facts it must reach (an int: at least that many; a tuple: exactly that)
REACH = {
    "clique1700": dict(orders_over_1024=10, orders_le_1024_big=10, tile_rows_ge_12=5, xcd_tables=5, grouped=1, tfuse=20, group_launch_level=20, schur128_level=10,
                       schur64_level=10, asm_pull_fronts=20, max_order=1025),
    "clique_edge": dict(edge_1024_1025_level=(1,), orders_over_1024=2, grouped=1, tfuse=20, schur128_level=1, schur64_level=1),
    "clique_grid": dict(lookahead=3, lookahead_fork_level=2, p1_small_level=2, side_small_bucket=1, selfasm=20, xcd_tables=1, xcd_tables2=1, grouped=1,
                        group_launch_level=5, orders_over_1024=5, tfuse=16),
    "grid24": dict(tfuse=16, grouped=1, group_launch_level=4, schur64_level=4, fastpiv_big_blocks=16),
    "grid30": dict(fused_diag_trsm_level=3, selfasm=5, grouped=1, group_launch_level=2),
    "grid48x44": dict(assemble2_level=1, assemble_column_level=1, xcd_affine_launch=1, asm_pull_fronts=64),
    "grid64x56": dict(narrow_fused_level=1, fused_diag_trsm_level=2),
    # what tests/test_gpu_parity.py relies on: test_lookahead_split_updates... (the plan splits an update under its TUNE string -- but see
    # test_the_110x90_grid_forks_no_look_ahead) and test_optional_code_paths_stay_exact[wide_panels] (a panel of more than 96 columns)
    "grid110x90_la": dict(lookahead=1, mid_split=1, selfasm=40, assemble2_level=2, fused_diag_trsm_level=2, side_small_bucket=1),
    "grid110x90_wide": dict(maxsupernode=(128,), kk_over_64=1, narrow_fused_level=1),
    "lukvl1000": dict(df_run=1, leaf_chain=2, optimistic_only=2),
    "lukvl12000": dict(pair_levels=1, pair16_levels=1, leafchain_solve=2),
    "lukvl40000": dict(tiny_split=2, reg2_level_strict=2, pair_levels=2, leaf_chain=2, df_run=1),
}
# every fact a test may name is reached by a fixture of the GPU suite
EVERY_FACT = ["orders_over_1024", "tile_rows_ge_12", "tiny_split", "mid_split", "lookahead", "lookahead_fork_level", "grouped", "tfuse", "selfasm", "df_run",
              "leaf_chain", "fused_diag_trsm_level", "narrow_fused_level", "assemble2_level", "pair_levels", "kk_over_64", "xcd_tables", "xcd_tables2",
              "xcd_affine_launch", "side_small_bucket", "p1_small_level", "reg2_level_strict", "edge_1024_1025_level", "fastpiv_big_blocks"]
# knob -> (plan arrays that must differ between the legs, the fact that must be reached with the knob on and gone with it off)
KNOBS = {
    "tfuse": (["path_bits", "asmcut", "scalars"], "tfuse"),
    "grouped": (["scalars", "groups", "level_list"], "group_launch_level"),
    "selfasm": (["path_bits"], "selfasm"),
    "xcd_tiles": (["path_bits", "path_scalars"], "xcd_tables"),
    "fuse_upd": (["levels"], "narrow_fused_level"),
    "lookahead": (["levels", "path_bits", "path_scalars", "groups"], "lookahead_fork_level"),
    "front_df": (["df_runs"], "df_run"),
    "pair_solve": (["path_scalars"], "pair_levels"),
    "fastpiv": (["df_runs", "lc_ptr", "lc_fronts", "scalars"], "leaf_chain"),
    # these select launches: the factor schedules differ, and the fact counts their records
    "fuse_dt": (["inputs", "factor.single.full", "factor.single.opt"], "fused_diag_trsm_level"),
    "p1_small": (["inputs", "factor.single.full", "factor.single.opt"], "p1_small_level"),
    "side_small": (["inputs", "factor.single.full", "factor.single.opt"], "side_small_bucket"),
    # this one acts in a kernel through a flag: the plan's exported `inputs` carry the switch
    "asm_pull": (["inputs"], "asm_pull_fronts"),
}
# (on a system without small fronts `fastpiv` is the kernel flag DevView::fastpiv alone: the pivot blocks of the big fronts)
OVERRIDE = {("fastpiv", "grid24"): (["inputs"], "fastpiv_big_blocks")}
# knobs numeric.hip reads itself (DevView flags: they select nothing on the host): nothing in the plan can show them; the structural precondition of
# the path they switch (reach is INFERRED)
PRECONDITION = {"xcd_affine": "xcd_affine_launch", "norestore": "group_launch_level"}


@pytest.mark.parametrize("fixture", sorted(REACH))
def test_fixture_reaches_what_its_tests_name(fixture):
    F, _ = facts(fixture)
    for fact, want in REACH[fixture].items():
        if isinstance(want, tuple):
            assert F[fact] == want[0], (fixture, fact, F[fact])
        else:
            assert F[fact] >= want, (fixture, fact, F[fact])


def test_every_fact_and_every_knob_has_a_fixture():
    for fact in EVERY_FACT:
        assert any(fact in REACH[f] for f in REACH), fact
    tested = {t[0] for t in pathfix.TABLE} | {"optimistic"}
    # every MI355X_KKT_DISABLE name that selects a kernel path (env_knobs.h; subcomm, blockcache, thread_pool and purify select none): the twelve of
    # tests/test_gpu_fast_paths.py -- lookahead, p1_small and fuse_dt again on smaller fixtures -- and those tests/test_gpu_parity.py switches
    elsewhere = {"leafchain", "chain_solve", "solve_ctx", "keep_scale"}
    assert tested | elsewhere >= {"lookahead", "chain_solve", "fuse_dt", "fastpiv", "asm_pull", "pair_solve", "selfasm", "xcd_tiles", "xcd_affine", "fuse_upd",
                                  "grouped", "tfuse", "leafchain", "side_small", "front_df", "p1_small", "norestore", "optimistic", "solve_ctx", "keep_scale"}
    assert tested <= set(KNOBS) | set(PRECONDITION) | {"optimistic"}
    for _, fixture, *_ in pathfix.TABLE:
        assert fixture in REACH
    for fixture, *_ in pathfix.OPTIMISTIC:
        assert fixture in REACH


@pytest.mark.parametrize("knob,fixture", [(t[0], t[1]) for t in pathfix.TABLE], ids=[f"{t[0]}-{t[1]}" for t in pathfix.TABLE])
def test_knob_changes_the_plan_on_its_fixture(knob, fixture):
    on, plan_on = facts(fixture)
    off, plan_off = facts(fixture, knob)
    diff = R.plan_diff(plan_on, plan_off)
    if knob in PRECONDITION:      # read by numeric.hip itself: the plan cannot differ; the path's precondition must hold
        assert diff == [] and on[PRECONDITION[knob]] >= 1, (knob, fixture, diff)
        if knob == "norestore":
            assert on["inputs"]["fastpiv"] == 1      # (the optimistic schedule, which alone drops the safety copies, needs the static-order path)
        return
    arrays, fact = OVERRIDE.get((knob, fixture), KNOBS[knob])
    assert set(arrays) <= set(diff), (knob, fixture, diff)
    assert on[fact] >= 1 and off[fact] == 0, (knob, fixture, fact, on[fact], off[fact])
    assert on["inputs"][knob] == 1 and off["inputs"][knob] == 0


@pytest.mark.parametrize("fixture", [t[0] for t in pathfix.OPTIMISTIC])
def test_optimistic_schedule_has_something_to_drop(fixture):
    """`optimistic` is read by numeric.hip at the first factorisation: inferred reach -- leaf chains and data-flow runs (launched by that schedule
    only), and on the larger system the levels whose strict k_front_reg<64, 2> launch it leaves out"""
    F, _ = facts(fixture)
    assert F["optimistic_only"] >= 2 and F["inputs"]["fastpiv"] == 1
    if fixture == "lukvl40000":
        assert F["reg2_level_strict"] >= 2 and F["reg2_level_optimistic"] == 0


def test_the_110x90_grid_forks_no_look_ahead():
    """Under la_min_nt=3,la_min_tiles=0 the plan of grid_kkt(110, 90, dof=3, ncon=2, seed=31) marks an update as split (la_any, the eager multi-stream
    schedule and the side stream follow) -- but its largest front has 730 rows, and only the 128 x 128 update of fronts ABOVE 1024 rows launches part 1 /
    part 2: no level forks.  The split-update kernels are tested on the clique_grid fixture (tests/test_gpu_fast_paths.py), where two levels do."""
    F, _ = facts("grid110x90_la")
    assert F["lookahead"] >= 1 and F["max_order"] <= 1024 and F["orders_over_1024"] == 0 and F["lookahead_fork_level"] == 0
    G, _ = facts("clique_grid")
    assert G["lookahead_fork_level"] >= 2 and G["p1_small_level"] >= 2


@pytest.mark.parametrize("fixture", sorted({t[1] for t in pathfix.TABLE} | {t[0] for t in pathfix.OPTIMISTIC}))
def test_fixture_is_well_enough_conditioned_for_the_forward_error_cap(fixture):
    """plain fp64 LAPACK / SuperLU within 1e-9 of the longdouble-refined reference: the 1e-7 cap of the GPU tests cannot hide a kernel's error behind
    the conditioning; the inertia by construction is LAPACK's where the dense matrix is small enough"""
    S = pathfix.system(fixture)
    ref, plain, eig_neg = pathfix.reference(fixture)
    for k in range(3):
        err = np.abs(plain[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max())
        print(fixture, k, "plain fp64 against the reference: %.2e" % err)
        assert err <= 1e-9
    assert eig_neg is None or eig_neg == S["neg"]
    if S["n"] <= pathfix.EIG_MAX:
        assert eig_neg is not None
