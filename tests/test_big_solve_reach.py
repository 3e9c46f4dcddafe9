"""Host only (no device): what the fixtures of tests/test_gpu_big_solve.py launch for their fronts above 128 rows, leg by leg -- which big-front solve
kernel runs on how many levels, the chains of the data-flow sweeps (links, widths, rows beyond the chain, how a chain starts, gathered children of its
head), the solve units of the `solve_group` option -- restated from numeric.hip solve_sweep / solve_level by tests/support/reach.py solve_reach.  The
shapes are pinned, so that a later change of the ordering or of a threshold fails here instead of silently emptying the GPU test.

What each edge is for (kernels_solve.hip.inc):
  chains of > 64 links         k_fwd_chain / k_bwd_chain keep 64 link records in LDS and reload them at (i & 63) == 0 && i > 0              chain_long2, chain_long7
  narrow links, k < 64         the zero padding of messages, pivot vectors and inverses in every chain / solo / fin kernel                   every fixture; k = 1 in chain_delayed
  rows beyond a chain or unit  64 per forward row workgroup, 256 per backward dot workgroup, `nch` loops unrolled by four                  tails (both sides of 64 and 256), tall (nch = 1 .. 5)
  > 4 gathered children        k_fwd_chain batches four and loops over the rest; k_fwd_grp loops over all                                   star6
  panels wider than 64         k_fwd_solo, k_bwd_grp_dot + k_bwd_grp on per-link units; such a level stays outside the segments            wide
  units of several links       k_fwd_grp + k_fwd_grp_upd, k_bwd_grp_dot + k_bwd_grp; narrow links; exactly 256 columns                      chain_long7, chain_delayed256
Not reachable: a link of ONE column from the options alone (max_sn_cols = 1 falls back to 63, 2 and 3 both give k = 2) -- chain_delayed gets one from a
structural edit instead."""
import functools

import numpy as np
import pytest

from tests.support import bigfix, pathfix, reach as R

CHAIN_ARRAYS = ["chain_descs", "chain_links", "chain_segs", "inputs"]      # what MI355X_KKT_DISABLE=chain_solve changes in the exported plan (the input itself included)

# (fixture, leg) -> the pinned facts of solve_reach, as analysed when the fixtures were written
#   levels: (k_fwd_solo64, k_fwd_solo, k_fwd_grp + k_fwd_grp_upd, k_bwd_dot64 + k_bwd_fin64, k_bwd_grp_dot + k_bwd_grp) level counts
EXPECT = {
    ("chain_long2", "sweeps"): dict(levels=(0, 0, 0, 0, 0), segments=1, chains=65, chain_levels=165, chain_shapes=[(101, 128)], link_widths=[2], inits=[1, 2], gathered=(1, 0), level_widths=[], unit_shapes=[(1, 2)], big=(101, 130, 330), maxsupernode=2),
    ("chain_long2", "levels"): dict(levels=(101, 0, 0, 101, 0), segments=0, chains=0, chain_levels=0, chain_shapes=[], link_widths=[], inits=[], gathered=(0, 0), level_widths=[2], unit_shapes=[(1, 2)], big=(101, 130, 330), maxsupernode=2),
    ("chain_long7", "sweeps"): dict(levels=(0, 0, 0, 0, 0), segments=1, chains=19, chain_levels=86, chain_shapes=[(68, 124)], link_widths=[5, 7], inits=[1, 2], gathered=(1, 0), level_widths=[], unit_shapes=[(1, 7)], big=(68, 131, 600), maxsupernode=7),
    ("chain_long7", "levels"): dict(levels=(68, 0, 0, 68, 0), segments=0, chains=0, chain_levels=0, chain_shapes=[], link_widths=[], inits=[], gathered=(0, 0), level_widths=[7], unit_shapes=[(1, 7)], big=(68, 131, 600), maxsupernode=7),
    ("chain_long7", "groups"): dict(levels=(0, 0, 17, 0, 17), segments=0, chains=0, chain_levels=0, chain_shapes=[], link_widths=[], inits=[], gathered=(0, 0), level_widths=[7], unit_shapes=[(4, 28)], big=(68, 131, 600), maxsupernode=7),
    ("chain_delayed", "sweeps"): dict(levels=(0, 0, 0, 0, 0), segments=1, chains=4, chain_levels=12, chain_shapes=[(9, 99)], link_widths=[1, 34, 60, 61, 62, 63, 64], inits=[1, 2], gathered=(1, 0), level_widths=[], unit_shapes=[(1, 1), (1, 60), (1, 61), (1, 62), (1, 63), (1, 64)], big=(9, 159, 600), maxsupernode=64),
    ("chain_delayed", "levels"): dict(levels=(9, 0, 0, 9, 0), segments=0, chains=0, chain_levels=0, chain_shapes=[], link_widths=[], inits=[], gathered=(0, 0), level_widths=[1, 60, 61, 62, 63, 64], unit_shapes=[(1, 1), (1, 60), (1, 61), (1, 62), (1, 63), (1, 64)], big=(9, 159, 600), maxsupernode=64),
    ("chain_delayed", "groups"): dict(levels=(0, 0, 3, 0, 3), segments=0, chains=0, chain_levels=0, chain_shapes=[], link_widths=[], inits=[], gathered=(0, 0), level_widths=[1, 60, 64], unit_shapes=[(1, 60), (4, 189), (4, 252)], big=(9, 159, 600), maxsupernode=64),
    ("chain_delayed256", "sweeps"): dict(levels=(0, 0, 0, 0, 0), segments=1, chains=3, chain_levels=10, chain_shapes=[(8, 96)], link_widths=[33, 59, 63, 64], inits=[1, 2], gathered=(1, 0), level_widths=[], unit_shapes=[(1, 59), (1, 63), (1, 64)], big=(8, 160, 600), maxsupernode=64),
    ("chain_delayed256", "levels"): dict(levels=(8, 0, 0, 8, 0), segments=0, chains=0, chain_levels=0, chain_shapes=[], link_widths=[], inits=[], gathered=(0, 0), level_widths=[59, 63, 64], unit_shapes=[(1, 59), (1, 63), (1, 64)], big=(8, 160, 600), maxsupernode=64),
    ("chain_delayed256", "groups"): dict(levels=(0, 0, 2, 0, 2), segments=0, chains=0, chain_levels=0, chain_shapes=[], link_widths=[], inits=[], gathered=(0, 0), level_widths=[59, 64], unit_shapes=[(4, 248), (4, 256)], big=(8, 160, 600), maxsupernode=64),
    ("tails", "sweeps"): dict(levels=(0, 0, 0, 0, 0), segments=1, chains=30, chain_levels=8, chain_shapes=[(2, 67), (2, 68), (2, 69), (2, 77), (2, 78), (2, 79), (2, 259), (2, 260), (2, 261), (3, 70), (3, 71), (3, 72), (3, 255), (3, 256), (3, 257)], link_widths=[4, 5, 6, 7, 8, 9, 14, 63], inits=[1, 2], gathered=(2, 0), level_widths=[], unit_shapes=[(1, 63)], big=(36, 130, 446), maxsupernode=63),
    ("tails", "levels"): dict(levels=(5, 0, 1, 6, 0), segments=0, chains=0, chain_levels=0, chain_shapes=[], link_widths=[], inits=[], gathered=(0, 1), level_widths=[63], unit_shapes=[(1, 63)], big=(36, 130, 446), maxsupernode=63),
    ("star6", "sweeps"): dict(levels=(0, 0, 0, 0, 0), segments=1, chains=9, chain_levels=7, chain_shapes=[(2, 74), (3, 150)], link_widths=[11, 14, 63], inits=[1, 2], gathered=(6, 0), level_widths=[], unit_shapes=[(1, 14), (1, 63)], big=(20, 137, 290), maxsupernode=63),
    ("star6", "levels"): dict(levels=(4, 0, 1, 5, 0), segments=0, chains=0, chain_levels=0, chain_shapes=[], link_widths=[], inits=[], gathered=(0, 6), level_widths=[14, 63], unit_shapes=[(1, 14), (1, 63)], big=(20, 137, 290), maxsupernode=63),
    ("star6", "groups"): dict(levels=(0, 0, 2, 0, 2), segments=0, chains=0, chain_levels=0, chain_shapes=[], link_widths=[], inits=[], gathered=(0, 0), level_widths=[14, 63], unit_shapes=[(2, 126), (3, 140)], big=(20, 137, 290), maxsupernode=63),
    ("wide", "sweeps"): dict(levels=(0, 1, 0, 0, 1), segments=1, chains=3, chain_levels=9, chain_shapes=[(7, 70)], link_widths=[7, 63], inits=[0, 2], gathered=(1, 0), level_widths=[89], unit_shapes=[(1, 63), (1, 89)], big=(8, 133, 600), maxsupernode=89),
    ("wide", "levels"): dict(levels=(7, 1, 0, 7, 1), segments=0, chains=0, chain_levels=0, chain_shapes=[], link_widths=[], inits=[], gathered=(0, 0), level_widths=[63, 89], unit_shapes=[(1, 63), (1, 89)], big=(8, 133, 600), maxsupernode=89),
    ("wide", "groups"): dict(levels=(0, 0, 3, 0, 3), segments=0, chains=0, chain_levels=0, chain_shapes=[], link_widths=[], inits=[], gathered=(0, 0), level_widths=[63], unit_shapes=[(1, 63), (3, 215), (4, 252)], big=(8, 133, 600), maxsupernode=89),
    ("indef", "sweeps"): dict(levels=(0, 0, 0, 0, 0), segments=1, chains=13, chain_levels=13, chain_shapes=[(1, 100), (1, 150), (1, 200), (1, 250), (1, 300), (1, 350), (1, 400), (1, 450), (1, 500), (1, 550)], link_widths=[11, 44, 55], inits=[1, 2], gathered=(1, 0), level_widths=[], unit_shapes=[(1, 55)], big=(10, 155, 605), maxsupernode=55),
    ("indef", "levels"): dict(levels=(1, 0, 9, 10, 0), segments=0, chains=0, chain_levels=0, chain_shapes=[], link_widths=[], inits=[], gathered=(0, 1), level_widths=[55], unit_shapes=[(1, 55)], big=(10, 155, 605), maxsupernode=55),
    ("tall", "sweeps"): dict(levels=(0, 0, 0, 0, 0), segments=1, chains=3, chain_levels=18, chain_shapes=[(16, 92)], link_widths=[29, 63], inits=[1, 2], gathered=(1, 0), level_widths=[], unit_shapes=[(1, 63)], big=(16, 155, 1100), maxsupernode=63),
    ("tall", "levels"): dict(levels=(16, 0, 0, 16, 0), segments=0, chains=0, chain_levels=0, chain_shapes=[], link_widths=[], inits=[], gathered=(0, 0), level_widths=[63], unit_shapes=[(1, 63)], big=(16, 155, 1100), maxsupernode=63),
    ("tall", "groups"): dict(levels=(0, 0, 4, 0, 4), segments=0, chains=0, chain_levels=0, chain_shapes=[], link_widths=[], inits=[], gathered=(0, 0), level_widths=[63], unit_shapes=[(4, 252)], big=(16, 155, 1100), maxsupernode=63),
}


@functools.lru_cache(maxsize=None)
def analysed(name, leg):
    with bigfix.leg_knobs(leg):
        return bigfix.handle(name, leg)


def facts(name, leg):
    with bigfix.leg_knobs(leg):
        return R.solve_reach(analysed(name, leg))


def summary(F):
    """the facts that are pinned: small enough to read in a table"""
    return dict(levels=(F["fwd_solo64_levels"], F["fwd_solo_levels"], F["fwd_grp_levels"], F["bwd_dot64_levels"], F["bwd_grp_levels"]),
                segments=F["segments"], chains=F["chains"], chain_levels=F["chain_levels"], chain_shapes=F["chain_shapes"], link_widths=F["link_widths"],
                inits=F["inits"], gathered=(F["max_gathered_chain_head"], F["max_gathered_level"]), level_widths=F["level_widths"],
                unit_shapes=F["unit_shapes"], big=(F["big_fronts"],) + F["big_orders"], maxsupernode=F["maxsupernode"])


@pytest.mark.parametrize("fixture,leg", bigfix.CASES)
def test_pinned_reach_facts(fixture, leg):
    F = facts(fixture, leg)
    S = summary(F)
    print(f"{fixture} [{leg}]: n {bigfix.system(fixture)['n']}")
    for k, v in S.items():
        print(f"    {k} = {v!r}")
    print(f"    tails = {F['tails']!r}\n    level_tails = {F['level_tails']!r}\n    upd_mod256 = {F['upd_mod256']!r}")
    assert S == EXPECT[fixture, leg]
    # the leg is what it says: chain sweeps over every big front, or none at all
    assert F["solve_group"] == (1 if leg == "groups" else 0)
    if leg == "sweeps":
        assert F["segments"] >= 1 and F["chain_big_fronts"] + sum(1 for _ in F["level_widths"]) > 0
    else:
        assert F["segments"] == 0 and sum(S["levels"][:3]) == sum(S["levels"][3:]) > 0
    if leg == "levels":
        assert F["bwd_dot64_levels"] > 0 and F["unit_max_links"] == 1
    if leg == "groups":
        assert S["levels"][:2] == (0, 0) and S["levels"][3] == 0 and F["unit_max_links"] > 1      # k_fwd_grp / k_bwd_grp only


@pytest.mark.parametrize("fixture", sorted(bigfix.FIXTURES))
def test_chain_solve_changes_the_chain_arrays_only(fixture):
    """the sweeps and the levels legs differ by MI355X_KKT_DISABLE=chain_solve: one analysed handle, two plans"""
    s = analysed(fixture, "sweeps")
    with bigfix.leg_knobs("sweeps"):
        a = R.plan_arrays(s)
    with bigfix.leg_knobs("levels"):
        b = R.plan_arrays(s)
    assert R.plan_diff(a, b) == CHAIN_ARRAYS
    assert len(b["chain_segs"]) == 0 and len(a["chain_segs"]) > 0
    with pathfix.knobs(None, "chain_solve_maxc=1"):      # (cannot stand in for it where every level holds one front)
        c = R.plan_arrays(s)
    if fixture in ("chain_long2", "chain_long7", "chain_delayed", "chain_delayed256", "wide", "indef"):
        assert len(c["chain_segs"]) > 0


def test_chain_long2_has_a_chain_of_more_than_64_links():
    F = facts("chain_long2", "sweeps")
    assert F["max_nlinks"] == 101 > 64 and F["link_widths"] == [2] and F["chain_shapes"] == [(101, 128)]
    assert F["chain_levels"] == 165 and F["big_orders"] == (130, 330)
    L = facts("chain_long2", "levels")
    assert L["fwd_solo64_levels"] == L["bwd_dot64_levels"] == 101 and L["level_widths"] == [2]


def test_chain_long7_has_68_links_and_units_of_four_narrow_links():
    F = facts("chain_long7", "sweeps")
    assert F["max_nlinks"] == 68 > 64 and (68, 124) in F["chain_shapes"] and 7 in F["link_widths"]
    G = facts("chain_long7", "groups")
    assert G["unit_max_links"] == 4 and G["unit_shapes"] == [(4, 28)] and G["fwd_grp_levels"] == G["bwd_grp_levels"] == 17


def test_the_delayed_fixtures_solve_on_an_edited_structure():
    for name in ("chain_delayed", "chain_delayed256"):
        assert analysed(name, "sweeps").info().num_delayed == len(bigfix.system(name)["delayed"])
    F = facts("chain_delayed", "sweeps")
    big_widths = sorted({k for _, k in facts("chain_delayed", "levels")["unit_shapes"]})
    assert len(big_widths) >= 3 and big_widths == [1, 60, 61, 62, 63, 64]                 # a ONE-column link of a big front, and both sides of 63
    assert F["chain_shapes"] == [(9, 99)]
    G = facts("chain_delayed256", "groups")
    assert (4, 256) in G["unit_shapes"] and G["unit_max_cols"] == 256                       # k_fwd_grp_upd / k_bwd_grp: the whole 256-entry LDS vector
    assert len({k for _, k in facts("chain_delayed256", "levels")["unit_shapes"]}) == 3


def test_tails_has_both_sides_of_64_and_of_256():
    S = bigfix.system("tails")
    assert S["n"] == 2727
    F = facts("tails", "sweeps")
    assert set(F["tails"]) >= {63, 64, 65, 255, 256, 257, 259, 260, 261}
    assert {n for n, _ in F["chain_shapes"]} == {2, 3}
    assert {0, 1, 255} <= set(F["upd_mod256"])
    L = facts("tails", "levels")
    assert set(L["level_tails"]) >= {255, 256, 257} and {t for t in L["level_tails"] if t > 256} and {t for t in L["level_tails"] if t < 128}


def test_star6_has_a_head_with_more_than_four_gathered_children():
    S = bigfix.system("star6")
    assert S["n"] == 1040
    F = facts("star6", "sweeps")
    assert F["max_gathered_chain_head"] >= 5 and 2 in F["inits"]
    L = facts("star6", "levels")
    assert L["max_gathered_level"] >= 5 and L["fwd_solo64_levels"] > 0 and L["fwd_grp_levels"] > 0      # a solo and a non-solo level


def test_wide_has_one_level_of_the_wide_forward_kernel():
    for leg in ("sweeps", "levels"):
        F = facts("wide", leg)
        assert F["fwd_solo_levels"] == 1 and F["bwd_grp_levels"] == 1 and F["maxsupernode"] == 89
    F = facts("wide", "sweeps")
    assert 0 in F["inits"] and F["level_widths"] == [89]      # the chain above the wide front starts from a vector in place
    assert facts("wide", "groups")["unit_max_cols"] <= 256


def test_indef_gathers_on_every_big_front():
    S = bigfix.system("indef")
    assert S["neg"] == 60
    F = facts("indef", "sweeps")
    assert F["max_nlinks"] == 1 and F["chains"] == 13 and F["tails"][0] == 0 and F["tails"][-1] == 550
    L = facts("indef", "levels")
    assert L["fwd_grp_levels"] == 9 and L["max_gathered_level"] == 1


def test_tall_has_four_and_five_blocks_of_partial_sums():
    """k_bwd_fin64 / k_bwd_grp add nch = ceil(rows beyond the unit / 256) partial sums, four at a time and then one by one"""
    nch = lambda F: sorted({(t + 255) // 256 for t in F["level_tails"]})
    L, G = facts("tall", "levels"), facts("tall", "groups")
    assert nch(L) == [1, 2, 3, 4, 5] and L["level_tails"][-1] == 1037 and L["bwd_dot64_levels"] == 16
    assert nch(G) == [1, 2, 3, 4] and G["bwd_grp_levels"] == 4 and G["unit_shapes"] == [(4, 252)]


@pytest.mark.parametrize("fixture", sorted(bigfix.FIXTURES))
def test_reference_is_not_hidden_by_conditioning(fixture):
    """plain fp64 LAPACK within 1e-9 of the refined reference (measured: 1.4e-15 .. 3.1e-15 on the definite fixtures, 2.4e-13 on indef); the inertia by
    LAPACK's eigenvalues is the one by construction"""
    S = bigfix.system(fixture)
    assert S["n"] <= pathfix.EIG_MAX
    e = bigfix.e_plain(fixture)
    print(f"{fixture}: n {S['n']} inertia {S['neg']} e_plain {e:.2e} tol_f {bigfix.tol_f(fixture):.2e}")
    assert e <= 1e-9
    assert bigfix.reference(fixture)[2] == S["neg"]
    assert 1e-12 <= bigfix.tol_f(fixture) <= 1e-7
