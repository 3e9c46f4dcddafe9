"""-m gpu: the limited-memory BFGS history of the C ABI (mi355x_kkt_lbfgs_*; reference IpLimMemQuasiNewtonUpdater.cpp) against its numpy statement
(tests/support/lbfgs_spec.py) in longdouble, and through the whole chain push -> factor K + sigma I_x -> lowrank_update -> lowrank_solve.
Sizes cross the kernels' own boundaries: `rows` 180 (below one 256-row block of k_lb_form), 517 (no multiple of 64 / 256), 1728 (two 1024-row
slabs of k_lb_dots) -- the systems of tests/test_gpu_lowrank.py; max_history 1, 2, 6 (loops unrolled to 8), 12 (to 16), 32 (to 32, the maximum).
Pairs: lbfgs_spec.make_pairs (cond(M) <= 5, lambda_min(sigma I + V V^T - U U^T) >= 0.59).

Bound of the comparisons with the specification: e_dev <= 64 max(e_64, 2^-52), e = max|A - A_ld| / max|A_ld|, e_64 the float64 specification's own
deviation from the longdouble one on the same inputs: 64 allows for a different but fixed summation order over at most 1728 rows and for the
amplification by cond(M) <= 5.  Solves: RES_TOL = 1e-12 and FIX_TOL = 1e-7, the project's tolerances (tests/test_gpu_lowrank.py)."""
import numpy as np
import pytest
import torch      # (before the library is loaded: see tests/test_gpu_parity.py)

import ipopt_amd
from ipopt_amd import kkt
from tests.support import lbfgs_spec as lb
from tests.support import lowrank_spec as lr
from tests.test_gpu_lowrank import SYSTEMS, system, sres, RES_TOL, FIX_TOL

pytestmark = pytest.mark.gpu
ROWS = [180, 517, 1728]
WHAT = ("S", "Y", "V", "U", "D", "L", "STS")


def handle(rows, **define):
    """an analysed handle on the system of `rows` whose x diagonal appears a second time, as duplicate triplets that carry sigma; -> (solver, values(sigma))"""
    S = system(rows)
    ix = np.arange(1, rows + 1).astype(S["r"].dtype)
    r2, c2 = np.concatenate([S["r"], ix]), np.concatenate([S["c"], ix])
    vals = lambda sigma: np.concatenate([S["v"], np.full(rows, sigma)])
    s = ipopt_amd.KKTSolver()
    s.initialize_structure(S["n"], r2, c2, vals=vals(1.0))
    if define:
        s.lbfgs_define(rows, **define)
    return s, vals


def factor(s, vals, sigma, m):
    s.values()[:] = vals(sigma)
    assert s.multi_solve(True, None, True, m) == kkt.SUCCESS


def snapshot(s):
    return {w: s.lbfgs_get(w) for w in WHAT}, s.lbfgs_info(), s.lowrank_info()


def same(a, b):
    (A, ia, la), (B, ib, lb_) = a, b
    ia = dict(ia, push_ms=0.0); ib = dict(ib, push_ms=0.0)
    return all(np.array_equal(A[w], B[w], equal_nan=True) and A[w].shape == B[w].shape for w in WHAT) and ia == ib and la == lb_


def dev(A, Ald):
    return float(np.abs(A - Ald).max() / np.abs(Ald).max())


@pytest.mark.parametrize("k", [1, 2, 6, 12, 32])
@pytest.mark.parametrize("rows", ROWS)
def test_columns_against_the_longdouble_specification(rows, k):
    Sp, Yp = lb.make_pairs(rows, k + 3, seed=1000 + rows + k)
    s, _ = handle(rows, max_history=k)
    H64, Hld = lb.History(rows, k), lb.History(rows, k, dtype=np.longdouble)
    assert s.lbfgs_info() == dict(rows=rows, max_history=k, memory=0, sigma=1.0, skipped_in_a_row=0, push_ms=0.0)
    worst = 0.0
    for j in range(k + 3):
        assert s.lbfgs_push(Sp[:, j], Yp[:, j]) == kkt.LBFGS_STORED
        assert H64.push(Sp[:, j], Yp[:, j]) == lb.STORED and Hld.push(Sp[:, j], Yp[:, j]) == lb.STORED
        if j + 1 not in (1, k, k + 3):
            continue
        m = min(j + 1, k)
        got, info, lri = snapshot(s)
        assert info["memory"] == m and info["skipped_in_a_row"] == 0
        assert lri == dict(rows=rows, nv=m, nu=m, current=False, update_ms=0.0)
        lo = j + 1 - m
        assert np.array_equal(got["S"], Sp[:, lo:j + 1]) and np.array_equal(got["Y"], Yp[:, lo:j + 1])      # bitwise, oldest first
        got["sigma"] = np.array([info["sigma"]])
        cmp = [(w, got[w], np.atleast_1d(getattr(H64, w)), np.atleast_1d(getattr(Hld, w))) for w in ("D", "L", "STS", "sigma", "V", "U")]
        Bld = lb.dense(*lb.recursive_terms(Hld.S, Hld.Y, Hld.sigma), Hld.sigma)                            # the recursive BFGS matrix, longdouble
        cmp.append(("sigma I + V V^T - U U^T", lb.dense(got["V"], got["U"], info["sigma"]), lb.dense(H64.V, H64.U, H64.sigma), Bld))
        for name, A, A64, Ald in cmp:
            assert A.shape == Ald.shape, name
            if not np.abs(Ald).max() > 0:                                                                  # (L of a single pair: the 1 x 1 zero)
                assert name == "L" and m == 1 and not A.any()
                continue
            e_dev, e_64 = dev(A, Ald), dev(A64, Ald)
            ratio = e_dev / max(e_64, 2.0 ** -52)
            worst = max(worst, ratio)
            print(f"rows {rows} k {k} after {j + 1}: {name}: e_dev {e_dev:.2e} e_64 {e_64:.2e} ratio {ratio:.2f}")
            assert e_dev <= 64.0 * max(e_64, 2.0 ** -52), (name, e_dev, e_64)
        assert np.all(np.triu(got["L"]) == 0.0)
    print(f"rows {rows} k {k}: largest e_dev / max(e_64, 2^-52) = {worst:.2f}")


def test_a_skipped_pair_changes_nothing():
    rows, k = 517, 6
    S = system(rows)
    Sp, Yp = lb.make_pairs(rows, 4, seed=5)
    s, vals = handle(rows, max_history=k)
    for j in range(3):
        assert s.lbfgs_push(Sp[:, j], Yp[:, j]) == kkt.LBFGS_STORED
    factor(s, vals, s.lbfgs_info()["sigma"], S["m"])
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    before = snapshot(s)
    assert before[2]["current"]
    ynan = Yp[:, 3].copy(); ynan[300] = np.nan
    for n_skipped, (a, b) in enumerate([(Sp[:, 3], -Yp[:, 3]), (Sp[:, 3], ynan)], 1):
        assert s.lbfgs_push(a, b) == kkt.LBFGS_SKIPPED
        after = snapshot(s)
        assert after[1]["skipped_in_a_row"] == n_skipped
        after[1]["skipped_in_a_row"] = 0                                                                   # (the counter is the one thing a skip moves)
        assert same(before, after) and after[2]["current"]
    assert s.lbfgs_push(Sp[:, 3], Yp[:, 3]) == kkt.LBFGS_STORED
    assert s.lbfgs_info()["skipped_in_a_row"] == 0 and s.lbfgs_info()["memory"] == 4 and not s.lowrank_info()["current"]


def test_a_cholesky_failure_keeps_the_pair_and_the_installed_columns():
    """init constant, init_val 1e8, s = e_1, y = 1e-9 e_1 twice: every dot is exact, M = [[1e8, 1e8], [1e8, 1e8]] in float64, the second pivot is exactly 0"""
    rows = 180
    s, _ = handle(rows, max_history=4, init="constant", init_val=1e8)
    e1 = np.zeros(rows); e1[0] = 1.0
    H = lb.History(rows, 4, init="constant", init_val=1e8)
    assert s.lbfgs_push(e1, 1e-9 * e1) == kkt.LBFGS_STORED and H.push(e1, 1e-9 * e1) == lb.STORED
    V1, U1 = s.lbfgs_get("V"), s.lbfgs_get("U")
    assert V1.shape == U1.shape == (rows, 1)
    assert s.lbfgs_push(e1, 1e-9 * e1) == kkt.LBFGS_NOT_POSDEF and H.push(e1, 1e-9 * e1) == lb.NOT_POSDEF
    I = s.lbfgs_info()
    assert I["memory"] == 2 and I["sigma"] == 1e8 and I["skipped_in_a_row"] == 0
    assert np.array_equal(s.lbfgs_get("V"), V1) and np.array_equal(s.lbfgs_get("U"), U1)
    assert s.lowrank_info() == dict(rows=rows, nv=1, nu=1, current=False, update_ms=0.0)
    assert np.array_equal(s.lbfgs_get("S"), np.column_stack([e1, e1])) and np.array_equal(s.lbfgs_get("Y"), 1e-9 * np.column_stack([e1, e1]))
    assert np.array_equal(s.lbfgs_get("D"), H.D) and np.array_equal(s.lbfgs_get("L"), H.L) and np.array_equal(s.lbfgs_get("STS"), H.STS)
    s.lbfgs_reset()
    I = s.lbfgs_info()
    assert I["memory"] == 0 and I["sigma"] == 1e8
    assert s.lowrank_info() == dict(rows=0, nv=0, nu=0, current=False, update_ms=0.0)
    assert s.lbfgs_get("S").shape == (rows, 0) and s.lbfgs_get("V").shape == (0, 0)
    Sp, Yp = lb.make_pairs(rows, 1, seed=2)
    assert s.lbfgs_push(Sp[:, 0], Yp[:, 0]) == kkt.LBFGS_STORED
    assert s.lbfgs_info()["memory"] == 1 and s.lowrank_info()["nv"] == 1
    s.lbfgs_clear()
    assert s.lbfgs_info() == dict(rows=0, max_history=0, memory=0, sigma=0.0, skipped_in_a_row=0, push_ms=0.0)
    assert s.lowrank_info()["nv"] == 1                                                                     # undefining the history leaves the installed update
    with pytest.raises(ipopt_amd.KKTError, match="lbfgs_define"):
        s.lbfgs_push(Sp[:, 0], Yp[:, 0])


@pytest.mark.parametrize("rows,k", [(517, 32), (1728, 6), (180, 12)])
def test_host_and_device_pushes_and_fresh_handles_give_the_same_bits(rows, k):
    Sp, Yp = lb.make_pairs(rows, k + 3, seed=77)
    dS = torch.tensor(Sp.T.copy(), dtype=torch.float64, device="cuda"); dY = torch.tensor(Yp.T.copy(), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    a, _ = handle(rows, max_history=k); b, _ = handle(rows, max_history=k); c, _ = handle(rows, max_history=k)
    for j in range(k + 3):
        assert a.lbfgs_push(Sp[:, j], Yp[:, j]) == kkt.LBFGS_STORED
        assert b.lbfgs_push_device(dS[j].data_ptr(), dY[j].data_ptr()) == kkt.LBFGS_STORED
        assert c.lbfgs_push(Sp[:, j], Yp[:, j]) == kkt.LBFGS_STORED
        if j + 1 in (1, k, k + 3):
            sa = snapshot(a)
            assert same(sa, snapshot(b)), f"host and device push differ after {j + 1}"
            assert same(sa, snapshot(c)), f"two fresh handles differ after {j + 1}"
    assert np.array_equal(dS.cpu().numpy(), Sp.T) and np.array_equal(dY.cpu().numpy(), Yp.T)              # the caller's vectors are only read


@pytest.mark.parametrize("rows", sorted(SYSTEMS))
def test_whole_chain_push_factor_update_solve(rows):
    S = system(rows)
    n, K = S["n"], S["K"]
    Sp, Yp = lb.make_pairs(rows, 9, seed=300 + rows)
    s, vals = handle(rows, max_history=6)
    for j in range(9):
        assert s.lbfgs_push(Sp[:, j], Yp[:, j]) == kkt.LBFGS_STORED
    sigma = s.lbfgs_info()["sigma"]
    V, U = s.lbfgs_get("V"), s.lbfgs_get("U")
    assert V.shape == U.shape == (rows, 6)
    factor(s, vals, sigma, S["m"])
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    Ks = K.copy(); Ks[np.arange(rows), np.arange(rows)] += sigma
    Kt = lr.dense_updated(Ks, V, U)
    b = Kt @ np.ones(n)
    x = b.copy(); s.lowrank_solve(x)
    xs = lr.solve(Ks, V, U, lr.update(Ks, V, U), b)
    res = sres(Kt, x, b)
    print(f"rows {rows}: sigma {sigma:.3f}, scaled residual {res:.2e}, |x - x_spec| {np.abs(x - xs).max():.2e}")
    assert res <= RES_TOL
    assert np.abs(x - xs).max() <= FIX_TOL * max(1.0, np.abs(xs).max())
    t, _ = handle(rows)                                                                                    # a push IS lowrank_set of these columns
    t.lowrank_set(V, U)
    factor(t, vals, sigma, S["m"])
    assert t.lowrank_update() == (kkt.SUCCESS, 0)
    xt = b.copy(); t.lowrank_solve(xt)
    assert np.array_equal(x, xt)


def test_sigma_modes_and_clips():
    rows = 180
    Sp, Yp = lb.make_pairs(rows, 1, seed=9)
    sv, yv = Sp[:, 0], 3.0 * Yp[:, 0]
    s, _ = handle(rows)
    for init in lb.INIT:
        s.lbfgs_define(rows, 3, init=init, init_val=7.5)
        assert s.lbfgs_info()["sigma"] == 7.5
        H = lb.History(rows, 3, init=init, init_val=7.5)
        assert s.lbfgs_push(sv, yv) == kkt.LBFGS_STORED and H.push(sv, yv) == lb.STORED
        got = s.lbfgs_info()["sigma"]
        print(f"{init}: sigma {got!r}, specification {float(H.sigma)!r}")
        assert abs(got - H.sigma) <= 1e-13 * H.sigma
    s.lbfgs_define(rows, 3)                                                                                # scalar1, the reference's limits
    assert s.lbfgs_push(sv, 1e10 * sv) == kkt.LBFGS_STORED and s.lbfgs_info()["sigma"] == 1e8
    s.lbfgs_reset()
    assert s.lbfgs_push(sv, 1e-10 * sv) == kkt.LBFGS_STORED and s.lbfgs_info()["sigma"] == 1e-8
    s.lbfgs_define(rows, 3, init="scalar2", sigma_min=4.0, sigma_max=5.0)
    assert s.lbfgs_push(sv, sv) == kkt.LBFGS_STORED and s.lbfgs_info()["sigma"] == 4.0


def test_the_history_survives_a_structure_edit():
    rows, k = 1728, 6
    S = system(rows)
    Sp, Yp = lb.make_pairs(rows, k + 2, seed=21)
    s, vals = handle(rows, max_history=k)
    for j in range(k + 1):                                                                                 # (the ring has wrapped once)
        assert s.lbfgs_push(Sp[:, j], Yp[:, j]) == kkt.LBFGS_STORED
    factor(s, vals, s.lbfgs_info()["sigma"], S["m"])
    before = snapshot(s)
    cols = np.random.default_rng(3).choice(S["n"], size=12, replace=False) + 1
    assert s.delay_columns(cols) >= 1
    assert same(before, snapshot(s))
    assert np.array_equal(s.lbfgs_get("S"), Sp[:, 1:k + 1])
    assert s.lbfgs_push(Sp[:, k + 1], Yp[:, k + 1]) == kkt.LBFGS_STORED
    H64, Hld = lb.History(rows, k), lb.History(rows, k, dtype=np.longdouble)
    for j in range(k + 2):
        H64.push(Sp[:, j], Yp[:, j]); Hld.push(Sp[:, j], Yp[:, j])
    assert np.array_equal(s.lbfgs_get("S"), Sp[:, 2:]) and np.array_equal(s.lbfgs_get("Y"), Yp[:, 2:])
    assert dev(s.lbfgs_get("U"), Hld.U) <= 64.0 * max(dev(H64.U, Hld.U), 2.0 ** -52)                       # (the rule of the columns test)
    sigma = s.lbfgs_info()["sigma"]
    factor(s, vals, sigma, S["m"])                                                                         # and the chain still closes on the edited structure
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    V, U = s.lbfgs_get("V"), s.lbfgs_get("U")
    Ks = S["K"].copy(); Ks[np.arange(rows), np.arange(rows)] += sigma
    Kt = lr.dense_updated(Ks, V, U)
    b = Kt @ np.ones(S["n"]); x = b.copy(); s.lowrank_solve(x)
    assert sres(Kt, x, b) <= RES_TOL
