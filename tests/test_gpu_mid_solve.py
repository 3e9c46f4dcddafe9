"""-m gpu: the load-batched solve kernels of the fronts of order 33 .. 128 (k_fwd_mid / k_bwd_mid, kernels_solve.hip.inc) against the plain level
kernels underneath them (k_fwd / k_bwd, MI355X_KKT_DISABLE=mid_solve), on fixtures whose mid fronts go through the level launches --
tests/test_mid_solve_reach.py shows that on the host and pins the shapes; each test here asserts the reach facts it stands on first.

Both legs: status SUCCESS, the fixture's inertia (by construction and by LAPACK's eigenvalues where n <= 3 000), scaled residual <= 1e-12, forward error
<= 1e-7 max(1, |x_ref|) against a reference refined with longdouble residuals, a repeated factor-and-solve bitwise the same.  Between the legs: equal
pivot statistics and BITWISE equal solutions over the three right-hand sides -- the new kernels keep, per entry, the operations of the plain ones in
their order (children in list order; y = a0 + a1 over the even / odd columns of the inverse; c = xu - (t0 + t1) over the even / odd panel columns; the
backward dot products row l, row l + 64, butterfly sum; x = a0 + a1 down the column of the inverse)."""
import functools

import numpy as np
import pytest
import torch      # noqa: F401  (before the library is loaded: torch brings its own HIP runtime)

import ipopt_amd
from ipopt_amd import kkt
from tests.support import midfix, mirror, pathfix, reach as R

pytestmark = pytest.mark.gpu
RES_TOL = 1e-12            # scaled residual, as in test_gpu_parity.py
FWD_TOL = 1e-7             # forward error against the refined reference, relative to max(1, |x_ref|)


def sres(K, x, b):
    return np.abs(K @ x - b).max() / (abs(K).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max() + 1e-300)


def leg_knobs(name, mid_off):
    """the leg's MI355X_KKT_DISABLE / MI355X_KKT_TUNE, held from the set-up of the handle to its last solve"""
    return pathfix.knobs(midfix.disable_list(name, mid_off), midfix.system(name)["tune"])


def handle(name):
    """a handle set up under the knobs of the moment, and its mid fronts (level launches, chain sweeps, chain levels)"""
    S = midfix.system(name)
    s = ipopt_amd.KKTSolver(**S["opts"])
    s.initialize_structure(S["n"], S["r"], S["c"], vals=S["v"])
    return s, midfix.mid_fronts(s)


@functools.lru_cache(maxsize=None)
def run_leg(name, mid_off):
    """factor + solve the fixture's three right-hand sides, twice"""
    S = midfix.system(name)
    known = S["neg"] is not None
    with leg_knobs(name, mid_off):
        s, where = handle(name)
        s.values()[:] = S["v"]
        x = S["B"].copy()
        st = s.multi_solve(True, x, known, S["neg"] if known else 0)
        I = s.info()
        x2 = S["B"].copy()
        st2 = s.multi_solve(True, x2, known, S["neg"] if known else 0)
    leg = dict(st=int(st), st2=int(st2), neg=int(s.number_of_neg_evals()), num_two=I.num_two, num_small=I.num_small, num_zero=I.num_zero, x=x,
               repeat_equal=bool(np.array_equal(x, x2)), where=where, maxsn=I.maxsupernode, sym=mirror.fetch(s) if not known else None)
    del s
    return leg


def check_reach(leg):
    level, _, _ = leg["where"]
    assert leg["maxsn"] <= 64                                              # solve_level's condition for the new kernels
    assert sum(1 for f in level if f[0] == R.FC_LDS128) > 0 and sum(1 for f in level if f[0] == R.FC_LDS64) > 0


def check_leg(name, leg, label):
    S = midfix.system(name)
    ref, _, eig_neg = midfix.reference(name)
    res = max(sres(S["K"], leg["x"][k], S["B"][k]) for k in range(3))
    fwd = max(np.abs(leg["x"][k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max()) for k in range(3))
    print(f"{name} [{label}]: status {leg['st']} neg {leg['neg']} two {leg['num_two']} small {leg['num_small']} zero {leg['num_zero']} "
          f"residual {res:.2e} forward {fwd:.2e} repeat bitwise {leg['repeat_equal']}")
    assert leg["st"] == leg["st2"] == kkt.SUCCESS
    assert leg["neg"] == S["neg"] and (eig_neg is None or eig_neg == S["neg"])
    assert res <= RES_TOL
    assert fwd <= FWD_TOL
    assert leg["repeat_equal"]


def check_between(name, on, off):
    d = max(np.abs(on["x"][k] - off["x"][k]).max() / max(1.0, np.abs(on["x"][k]).max()) for k in range(3))
    same = bool(np.array_equal(on["x"], off["x"]))
    print(f"mid_solve on {name}: legs bitwise {same}, difference {d:.2e}")
    assert on["where"] == off["where"]
    assert (on["num_two"], on["num_small"], on["num_zero"]) == (off["num_two"], off["num_small"], off["num_zero"])
    assert same


@pytest.mark.parametrize("fixture", ["mid_edges", "grid24", "grid48x44"])
def test_mid_solve_against_the_plain_level_kernels(fixture):
    on, off = run_leg(fixture, False), run_leg(fixture, True)
    check_reach(on)
    level, chain, nseg = on["where"]
    if fixture == "grid48x44":
        assert nseg > 0 and len(chain) > 0                                 # next to live chain sweeps
    else:
        assert nseg == 0 and chain == []
    if fixture == "mid_edges":
        assert sorted({f[1:4] for f in level}) == sorted(midfix.MID_EDGES_SHAPES)
    check_leg(fixture, on, "default")
    check_leg(fixture, off, "MI355X_KKT_DISABLE=...,mid_solve")
    check_between(fixture, on, off)


def test_mid_solve_with_two_by_two_pivots_in_the_mid_fronts():
    """hostile_grid_kkt(16, 16, seed=3) at u = 0.01 without scaling, delays, chain sweeps and the static-order fast paths: 2x2 pivots fire inside fronts
    of the two classes (pivot types from the pivoting specification, tests/support/mirror.py, whose statistics the device's must equal as in
    test_gpu_pivoting.py).  Bitwise between the legs; no accuracy claim -- the system is ill-conditioned by design, the factorisation is the same."""
    name = "hostile16"
    on, off = run_leg(name, False), run_leg(name, True)
    check_reach(on)
    level, chain, nseg = on["where"]
    assert nseg == 0 and chain == [] and len(level) == 32
    S = midfix.system(name)
    _, spec = mirror.factor_solve_pivoted(on["sym"], S["v"], S["B"][0], u=0.01, u2=0.01, fast_blocks=False, debug=True)
    mid_sn = {f[5] for f in level}
    two_in_mid = sum(int(np.sum(pt == 2)) for s_, _, _, _, _, pt, _ in spec["dbg"] if s_ in mid_sn)
    print(f"{name}: num_two {on['num_two']} (specification {spec['num_two']}), of them {two_in_mid} in fronts of order 33 .. 128")
    assert on["st"] == on["st2"] == off["st"] == off["st2"] == kkt.SUCCESS
    assert on["num_two"] > 0 and on["num_two"] == spec["num_two"] and on["neg"] == off["neg"] == spec["num_neg"]
    assert two_in_mid > 0
    assert on["repeat_equal"] and off["repeat_equal"]
    check_between(name, on, off)


def test_device_route_of_the_benchmark_is_bitwise_too():
    """factor_device + solve_device2 (bench.py's call path: the captured solve graph) on grid48x44, one right-hand side, against the mid_solve leg"""
    name = "grid48x44"
    S = midfix.system(name)
    out = []
    for mid_off in (False, True):
        with leg_knobs(name, mid_off):
            s, (level, chain, nseg) = handle(name)
            assert len(level) == 275 and nseg > 0
            dv = torch.tensor(S["v"], dtype=torch.float64, device="cuda")
            db = torch.tensor(S["B"][1], dtype=torch.float64, device="cuda")
            dx = torch.zeros_like(db)
            st, neg, zero = s.factor_device(dv.data_ptr())
            s.solve_device2(db.data_ptr(), dx.data_ptr())
            torch.cuda.synchronize()
        assert st == kkt.SUCCESS and neg == S["neg"] and zero == 0
        out.append(dx.cpu().numpy())
        del s
    assert sres(S["K"], out[0], S["B"][1]) <= RES_TOL
    assert np.array_equal(out[0], out[1])
