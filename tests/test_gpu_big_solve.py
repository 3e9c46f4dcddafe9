"""-m gpu: the triangular solves of the fronts above 128 rows (kernels_solve.hip.inc: k_fwd_chain / k_bwd_chain, k_fwd_solo64, k_fwd_solo, k_fwd_grp +
k_fwd_grp_upd, k_bwd_dot64 + k_bwd_fin64, k_bwd_grp_dot + k_bwd_grp) on fronts of PRESCRIBED edge shapes (tests/support/bigfix.py), against a reference
refined with longdouble residuals.  tests/test_big_solve_reach.py shows on the host which kernel a leg launches and pins the shapes; every test here
first asserts, from its own handle, the reach facts it stands on.

Legs (bigfix.LEGS), knobs held from the set-up of the handle to its last solve:
  sweeps   default schedule: the chain segments go to k_fwd_chain / k_bwd_chain
  levels   MI355X_KKT_DISABLE=chain_solve: k_fwd_solo64 / k_fwd_solo / k_fwd_grp + k_fwd_grp_upd forward, k_bwd_dot64 + k_bwd_fin64 (k > 64: k_bwd_grp_dot + k_bwd_grp) backward
  groups   option solve_group=1: k_fwd_grp + k_fwd_grp_upd, k_bwd_grp_dot + k_bwd_grp on units of up to four links

Per leg, over three right-hand sides (K 1, a random vector, K random): status SUCCESS with the inertia by construction; scaled residual <= 1e-12;
forward error against the refined reference, relative to max(1, |x_ref|), <= tol_f = min(1e-7, max(1e-12, 1000 e_plain)), where e_plain is the
discrepancy of plain fp64 LAPACK against the same reference (a property of the reference: 1.4e-15 .. 3.1e-15 on the definite fixtures, 2.4e-13 on indef)
and the factor 1 000 stands for what the device does differently (another elimination order, equilibration, a-posteriori pivot acceptance with
multipliers up to 1e4 where partial pivoting admits 1); a repeated solve and a repeated factor-and-solve bitwise the same.  Between the legs of a fixture:
equal pivot statistics, solutions within 2 tol_f.

On the 101-link chain of chain_long2 besides: three right-hand sides in one call (solve contexts forced, and one after the other) bitwise the single
solves; eager launches bitwise the graph replay; factor_device + solve_device2 bitwise multi_solve.

Measured on an MI355X when the tests were written (every leg: all three statuses SUCCESS, the solve repeated and the factor-and-solve repeated bitwise
equal; levels = levels launched per kernel, forward k_fwd_solo64 / k_fwd_solo / k_fwd_grp + k_fwd_grp_upd, backward k_bwd_dot64 + k_bwd_fin64 /
k_bwd_grp_dot + k_bwd_grp; chain = levels inside the segment of k_fwd_chain / k_bwd_chain):
  fixture           leg     forward levels  backward levels  chain  residual  forward error  tol_f
  chain_long2       sweeps    0 / 0 / 0        0 / 0          165   4.28e-16    1.22e-15     1.55e-12   (101 links of k = 2, then 64 one-link chains)
  chain_long2       levels  101 / 0 / 0      101 / 0            0   3.33e-16    4.44e-16     1.55e-12
  chain_long7       sweeps    0 / 0 / 0        0 / 0           86   1.10e-15    1.55e-15     2.66e-12   (68 links of k = 7)
  chain_long7       levels   68 / 0 / 0       68 / 0            0   1.03e-15    8.88e-16     2.66e-12
  chain_long7       groups    0 / 0 / 17       0 / 17           0   1.03e-15    8.88e-16     2.66e-12   (17 units of 4 x 7 columns)
  chain_delayed     sweeps    0 / 0 / 0        0 / 0           12   1.10e-15    8.88e-16     2.66e-12   (9 links, k in {1, 60 .. 64})
  chain_delayed     levels    9 / 0 / 0        9 / 0            0   1.03e-15    8.88e-16     2.66e-12
  chain_delayed     groups    0 / 0 / 3        0 / 3            0   1.03e-15    8.88e-16     2.66e-12
  chain_delayed256  sweeps    0 / 0 / 0        0 / 0           10   7.89e-16    1.11e-15     2.66e-12
  chain_delayed256  levels    8 / 0 / 0        8 / 0            0   8.68e-16    9.99e-16     2.66e-12
  chain_delayed256  groups    0 / 0 / 2        0 / 2            0   8.68e-16    8.88e-16     2.66e-12   (a unit of 4 x 64 = 256 columns)
  tails             sweeps    0 / 0 / 0        0 / 0            8   7.14e-16    1.11e-15     2.44e-12   (rows beyond a chain: 63 .. 65, 255 .. 257, 259 .. 261)
  tails             levels    5 / 0 / 1        6 / 0            0   7.14e-16    1.11e-15     2.44e-12
  star6             sweeps    0 / 0 / 0        0 / 0            7   6.04e-16    6.66e-16     3.22e-12   (a chain head that gathers 6 children)
  star6             levels    4 / 0 / 1        5 / 0            0   5.37e-16    8.88e-16     3.22e-12
  star6             groups    0 / 0 / 2        0 / 2            0   4.70e-16    7.77e-16     3.22e-12
  wide              sweeps    0 / 1 / 0        0 / 1            9   8.68e-16    9.99e-16     2.66e-12   (k = 89 on a level of its own below the segment)
  wide              levels    7 / 1 / 0        7 / 1            0   8.68e-16    9.99e-16     2.66e-12
  wide              groups    0 / 0 / 3        0 / 3            0   7.89e-16    9.99e-16     2.66e-12
  indef             sweeps    0 / 0 / 0        0 / 0           13   1.03e-15    7.13e-14     1.96e-10   (inertia 60)
  indef             levels    1 / 0 / 9       10 / 0            0   1.03e-15    7.24e-14     1.96e-10
  tall              sweeps    0 / 0 / 0        0 / 0           18   1.78e-15    8.88e-16     3.11e-12
  tall              levels   16 / 0 / 0       16 / 0            0   1.78e-15    1.11e-15     3.11e-12   (up to 5 blocks of 256 rows beyond a unit)
  tall              groups    0 / 0 / 4        0 / 4            0   1.91e-15    7.77e-16     3.11e-12
Between the legs of a fixture the solutions differ by 4.4e-16 .. 1.6e-15 (indef: 5.3e-14) and are never bitwise equal: the legs sum in different orders.
No leg came near its bound, and no kernel had to be changed.  That the tests can fail was tried once with a library built with three arithmetic
mutations (the fourth partial sum of the unrolled `nch` loops of k_bwd_fin64 and of k_bwd_grp dropped; the loop of k_fwd_chain over the gathered
children beyond the fourth skipped): tall[levels], tall[groups] and star6[sweeps] failed, with the two between-the-legs tests of those fixtures, and
nothing else did.
"""
import functools

import numpy as np
import pytest
import torch      # noqa: F401  (before the library is loaded: torch brings its own HIP runtime)

from ipopt_amd import kkt
from tests.support import bigfix, pathfix, reach as R

pytestmark = pytest.mark.gpu
RES_TOL = 1e-12            # scaled residual, as in test_gpu_parity.py


def sres(K, x, b):
    return np.abs(K @ x - b).max() / (abs(K).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max() + 1e-300)


def relmax(a, b):
    return max(np.abs(a[k] - b[k]).max() / max(1.0, np.abs(b[k]).max()) for k in range(len(a)))


@functools.lru_cache(maxsize=None)
def run_leg(name, leg):
    """factor + solve the fixture's three right-hand sides; solve again; factor and solve again"""
    S = bigfix.system(name)
    with bigfix.leg_knobs(leg):
        s = bigfix.handle(name, leg)
        facts = R.solve_reach(s)
        s.values()[:] = S["v"]
        x = S["B"].copy()
        st = s.multi_solve(True, x, True, S["neg"])
        I = s.info()
        x2 = S["B"].copy()
        st2 = s.multi_solve(False, x2)
        x3 = S["B"].copy()
        st3 = s.multi_solve(True, x3, True, S["neg"])
    out = dict(st=(int(st), int(st2), int(st3)), neg=int(s.number_of_neg_evals()), x=x, facts=facts, delayed=I.num_delayed,
               stats=(I.num_neg, I.num_two, I.num_small, I.num_zero, I.num_fast_blocks),
               solve_again=bool(np.array_equal(x, x2)), factor_again=bool(np.array_equal(x, x3)))
    x.setflags(write=False)
    s.close()
    return out


def check_reach(name, leg, F):
    """the facts the leg stands on, from the handle that ran it"""
    assert F["solve_group"] == (1 if leg == "groups" else 0)
    if leg == "sweeps":
        assert F["segments"] >= 1 and F["chain_big_fronts"] > 0
    if leg == "levels":
        assert F["segments"] == 0 and F["bwd_dot64_levels"] > 0 and F["fwd_solo64_levels"] > 0 and F["unit_max_links"] == 1
    if leg == "groups":
        assert F["segments"] == 0 and F["fwd_grp_levels"] == F["bwd_grp_levels"] > 0 and F["unit_max_links"] > 1
        assert F["fwd_solo64_levels"] == F["fwd_solo_levels"] == F["bwd_dot64_levels"] == 0
    if name == "chain_long2" and leg == "sweeps":
        assert F["max_nlinks"] == 101 and F["link_widths"] == [2]
    if name == "chain_long7":
        assert (F["max_nlinks"] == 68) if leg == "sweeps" else (F["unit_shapes"] == [(4, 28)]) if leg == "groups" else (F["level_widths"] == [7])
    if name == "chain_delayed":
        assert (1 in F["link_widths"] and F["chain_shapes"] == [(9, 99)]) if leg == "sweeps" else ((1, 1) in F["unit_shapes"]) if leg == "levels" else ((4, 189) in F["unit_shapes"])
    if name == "chain_delayed256":
        assert ((4, 256) in F["unit_shapes"]) if leg == "groups" else ({k for _, k in F["unit_shapes"]} == {59, 63, 64})
    if name == "tails":
        assert ({63, 64, 65, 255, 256, 257} <= set(F["tails"])) if leg == "sweeps" else ({255, 256, 257} <= set(F["level_tails"]))
        assert {0, 1, 255} <= set(F["upd_mod256"])
    if name == "star6":
        assert (F["max_gathered_chain_head"] >= 5) if leg == "sweeps" else (F["max_gathered_level"] >= 5 and F["fwd_grp_levels"] > 0) if leg == "levels" else (F["unit_max_links"] == 3)
    if name == "wide":
        assert F["maxsupernode"] == 89
        if leg != "groups":
            assert F["fwd_solo_levels"] == 1 and F["bwd_grp_levels"] == 1
        if leg == "sweeps":
            assert 0 in F["inits"]
    if name == "indef":
        assert (F["chains"] == 13 and F["max_nlinks"] == 1) if leg == "sweeps" else (F["fwd_grp_levels"] == 9)
    if name == "tall" and leg != "sweeps":
        assert max((t + 255) // 256 for t in F["level_tails"]) == (5 if leg == "levels" else 4)


@pytest.mark.parametrize("fixture,leg", bigfix.CASES)
def test_big_front_solves_against_the_refined_reference(fixture, leg):
    S = bigfix.system(fixture)
    ref, _, eig_neg = bigfix.reference(fixture)
    tol = bigfix.tol_f(fixture)
    out = run_leg(fixture, leg)
    check_reach(fixture, leg, out["facts"])
    res = max(sres(S["K"], out["x"][k], S["B"][k]) for k in range(3))
    fwd = relmax(out["x"], ref)
    F = out["facts"]
    print(f"{fixture} [{leg}]: status {out['st']} neg {out['neg']} stats {out['stats']} residual {res:.2e} forward {fwd:.2e} tol_f {tol:.2e} "
          f"solve again bitwise {out['solve_again']} factor again bitwise {out['factor_again']} | levels fwd solo64/solo/grp {F['fwd_solo64_levels']}/"
          f"{F['fwd_solo_levels']}/{F['fwd_grp_levels']} bwd dot64/grp {F['bwd_dot64_levels']}/{F['bwd_grp_levels']} chain levels {F['chain_levels']}")
    assert out["st"] == (kkt.SUCCESS,) * 3
    assert out["neg"] == S["neg"] == eig_neg and out["stats"][0] == S["neg"]
    assert out["delayed"] == (len(S["delayed"]) if S["delayed"] else 0)
    assert res <= RES_TOL
    assert fwd <= tol
    assert out["solve_again"]
    assert out["factor_again"]


@pytest.mark.parametrize("fixture", sorted(bigfix.FIXTURES))
def test_the_legs_of_a_fixture_agree(fixture):
    """the legs change the solve schedule only: the same factorisation, solutions within twice the forward-error bound of each other"""
    legs = bigfix.system(fixture)["legs"]
    tol = bigfix.tol_f(fixture)
    outs = {leg: run_leg(fixture, leg) for leg in legs}
    for i, a in enumerate(legs):
        for b in legs[i + 1:]:
            d = relmax(outs[a]["x"], outs[b]["x"])
            print(f"{fixture}: {a} against {b}: difference {d:.2e} (2 tol_f {2 * tol:.2e}), bitwise {np.array_equal(outs[a]['x'], outs[b]['x'])}")
            assert outs[a]["stats"] == outs[b]["stats"], (a, b)
            assert d <= 2 * tol, (a, b)


# ---- the 101-link chain: several right-hand sides, eager launches, the device route ----
LONG = "chain_long2"


def long_handle(**more):
    s = bigfix.handle(LONG, "sweeps", **more)
    F = R.solve_reach(s)
    assert F["max_nlinks"] == 101 and F["link_widths"] == [2] and F["segments"] == 1
    s.values()[:] = bigfix.system(LONG)["v"]
    return s


@pytest.mark.parametrize("mode", ["contexts", "one-after-the-other"])
def test_three_right_hand_sides_on_the_long_chain_are_bitwise_the_single_solves(mode):
    """one multi_solve over three right-hand sides, each in a solve context of its own (the gate between the contexts' chain sections on a chain of
    101 links) and one after the other: every column is bitwise the single solve"""
    S = bigfix.system(LONG)
    with pathfix.knobs("solve_ctx" if mode == "one-after-the-other" else None, "solve_ctx_force=1" if mode == "contexts" else None):
        s = long_handle()
        assert s.multi_solve(True, None, True, S["neg"]) == kkt.SUCCESS
        singles = []
        for k in range(3):
            x = S["B"][k].copy(); assert s.multi_solve(False, x) == kkt.SUCCESS; singles.append(x)
        X = S["B"].copy()
        assert s.multi_solve(False, X) == kkt.SUCCESS
        s.close()
    assert max(sres(S["K"], X[k], S["B"][k]) for k in range(3)) <= RES_TOL
    assert all(np.array_equal(X[k], singles[k]) for k in range(3))
    assert np.array_equal(X, run_leg(LONG, "sweeps")["x"])


def test_eager_launches_on_the_long_chain_are_bitwise_the_graph_replay():
    S = bigfix.system(LONG)
    with bigfix.leg_knobs("sweeps"):
        s = long_handle(use_graph=0)
        x = S["B"].copy()
        assert s.multi_solve(True, x, True, S["neg"]) == kkt.SUCCESS
        s.close()
    assert max(sres(S["K"], x[k], S["B"][k]) for k in range(3)) <= RES_TOL
    assert np.array_equal(x, run_leg(LONG, "sweeps")["x"])


def test_device_route_on_the_long_chain_is_bitwise_the_host_route():
    """factor_device + solve_device2 (the benchmark's call path) against multi_solve"""
    S = bigfix.system(LONG)
    with bigfix.leg_knobs("sweeps"):
        s = long_handle()
        dv = torch.tensor(np.array(S["v"]), dtype=torch.float64, device="cuda")
        st, neg, zero = s.factor_device(dv.data_ptr())
        out = []
        for k in range(3):
            db = torch.tensor(np.array(S["B"][k]), dtype=torch.float64, device="cuda")
            dx = torch.zeros_like(db)
            s.solve_device2(db.data_ptr(), dx.data_ptr())
            torch.cuda.synchronize()
            out.append(dx.cpu().numpy())
        s.close()
    assert st == kkt.SUCCESS and neg == S["neg"] and zero == 0
    assert max(sres(S["K"], out[k], S["B"][k]) for k in range(3)) <= RES_TOL
    assert np.array_equal(np.stack(out), run_leg(LONG, "sweeps")["x"])
