"""-m gpu: the panel solve with its L11 operands in registers (trsm_rows_regs, k_big_trsm<false, true>) against the kernel it replaces
(MI355X_KKT_DISABLE=trsm_regs: trsm_rows_impl with L11 staged in LDS), bit for bit.

Both legs factor ONE system on handles of their own, set up under MI355X_KKT_DISABLE=grouped,fuse_dt (tests/support/trsmfix.py BASE: the per-link
schedule, in which every level of big fronts is an FO_DIAG_REG + FO_TRSM pair -- tests/test_trsm_regs_reach.py shows on the host that each fixture has such
records there, and none in its default plan); the second leg adds `trsm_regs`, held from the set-up of the handle to its last solve.  A leg is
factor + three right-hand sides, twice.

  fixture                                       what it reaches in trsm_rows_regs
  grid24                                        mixed k <= 64 (15 .. 64) and three row blocks per front, up to five fronts per launch
  clique_kkt([331], 0, 0, seed=2), sn_cols 8    kp16 = 16: one column block, no sub-diagonal L11 block; every row remainder mod 64 and mod 2 as the chain shrinks
  the same, sn_cols 40                          kp16 = 48 with k = 39: padded columns
  the same, sn_cols 64                          k = 63, kp16 = 64: all six sub-diagonal blocks
  hostile_grid_kkt(16, 16, seed=3), u = 1e-8    hasis = 0: columns permuted in place, 2x2 pivots, diagonal blocks inverted by the lane substitution
  the same, u = 0.01                            as above, and multipliers above 1/u: colfail / apfail / zpiv marks

Between the legs: solutions bitwise equal; pivot data (mi355x_kkt_debug_pivots: dinv, doff, ptype, lperm), inertia, num_fast_blocks, num_two, num_small
and the failed-pivot list exactly equal.  Each leg: status SUCCESS, the repeat bitwise the same, forward error within the fixture's cap (1e-7 max(1, |x_ref|),
tests/test_gpu_fast_paths.py; the hostile grid 1e-6, tests/test_gpu_pivoting.py) of the longdouble-refined reference -- on which plain fp64 LAPACK is
within 1e-9 (tests/test_trsm_regs_reach.py)."""
import ctypes as C

import numpy as np
import pytest
import torch      # noqa: F401  (before the library is loaded: torch brings its own HIP runtime)

import ipopt_amd
from ipopt_amd import kkt
from tests.support import pathfix, reach as R, trsmfix

pytestmark = pytest.mark.gpu


def pivots(s, n):
    dinv, doff = np.zeros(n), np.zeros(n)
    pt, lp = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    s.lib.mi355x_kkt_debug_pivots.argtypes = [C.c_void_p] * 5
    assert s.lib.mi355x_kkt_debug_pivots(s._h, dinv.ctypes.data, doff.ctypes.data, pt.ctypes.data, lp.ctypes.data) == 0
    return dinv, doff, pt, lp


def run_leg(name, disable):
    S = trsmfix.system(name)
    with pathfix.knobs(disable, None):
        s = ipopt_amd.KKTSolver(**S["opts"])
        s.initialize_structure(S["n"], S["r"], S["c"], vals=S["v"])
        full = s.launch_plan("factor.single.full").reshape(-1, R.REC)
        ntrsm = int(np.sum(full[:, R.OP] == R.FO_TRSM))
        nsn = s.info().num_sn
        nbig = int(np.sum((s.symbolic(23, nsn) == R.FC_BIG) & (np.diff(s.symbolic(1, nsn + 1)) <= 64)))
        out = []
        for _ in range(2):
            s.values()[:] = S["v"]
            x = S["B"].copy()
            st = s.multi_solve(True, x, S["neg"] is not None, S["neg"] or 0)
            I = s.info()
            out.append(dict(st=int(st), x=x, piv=pivots(s, S["n"]), failed=np.sort(s.failed_pivots()),
                            stats=(I.num_neg, I.num_zero, I.num_two, I.num_small, I.num_fast_blocks, int(s.number_of_neg_evals()))))
    del s
    return dict(runs=out, ntrsm=ntrsm, nbig=nbig)


@pytest.mark.parametrize("fixture", sorted(trsmfix.FIXTURES))
def test_register_panel_solve_equals_the_staged_one_bitwise(fixture):
    S = trsmfix.system(fixture)
    ref, _ = trsmfix.reference(fixture)
    regs = run_leg(fixture, trsmfix.BASE)
    staged = run_leg(fixture, trsmfix.BASE + "," + trsmfix.KNOB)
    assert regs["ntrsm"] >= 1 and regs["ntrsm"] == staged["ntrsm"]
    for label, leg in (("trsm_rows_regs", regs), ("MI355X_KKT_DISABLE=trsm_regs", staged)):
        a, b = leg["runs"]
        fwd = max(np.abs(a["x"][k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max()) for k in range(3))
        print(f"{fixture} [{label}]: status {a['st']} (neg, zero, two, small, fast, neg_evals) {a['stats']} failed pivots {len(a['failed'])} "
              f"FO_TRSM records {leg['ntrsm']} forward {fwd:.2e} repeat bitwise {np.array_equal(a['x'], b['x'])}")
        assert a["st"] == b["st"] == kkt.SUCCESS
        assert S["neg"] is None or a["stats"][0] == a["stats"][5] == S["neg"]
        assert np.array_equal(a["x"], b["x"]) and a["stats"] == b["stats"] and np.array_equal(a["failed"], b["failed"])
        assert all(np.array_equal(p, q) for p, q in zip(a["piv"], b["piv"]))
        assert fwd <= S["fwd"]
    a, b = regs["runs"][0], staged["runs"][0]
    print(f"{fixture}: legs bitwise {np.array_equal(a['x'], b['x'])}, largest difference {np.abs(a['x'] - b['x']).max():.2e}")
    assert np.array_equal(a["x"], b["x"])
    assert a["stats"] == b["stats"]
    assert np.array_equal(a["failed"], b["failed"])
    for p, q, what in zip(a["piv"], b["piv"], ("dinv", "doff", "ptype", "lperm")):
        assert np.array_equal(p, q), what
    if S["hostile"] is not None:      # the rejected path is really run: pivot blocks left the fast path, 2x2 pivots; at u = 0.01 columns marked a posteriori
        assert a["stats"][4] < regs["nbig"] and a["stats"][2] >= 20
        if S["hostile"] >= 0.01:
            assert a["stats"][3] >= 50 and len(a["failed"]) >= 1
