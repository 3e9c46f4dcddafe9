"""-m gpu: the low-rank-updated solve of the C ABI (mi355x_kkt_lowrank_*: K~ = K + V V^T - U U^T; reference IpLowRankAugSystemSolver.cpp) against the
dense K~ and against its numpy statement (tests/support/lowrank_spec.py), plus the two primal-dual hooks.  Sizes cross the kernels' own boundaries:
`rows` 180 (below one 256-row block of the apply kernel), 300, 517 (no multiple of 64 / 256), 1728 (two 1024-row slabs of the Gram kernel); column
counts from 0 / 1 to the maximum 32 (p * q up to 1024: one to four outputs per thread, 1 to 64 row lanes per output); the final reduction sums any
number of slabs in one pass, so there is no slab limit to go beyond.  Recipe of the columns: tests/test_lowrank_spec.py (lambda_min(M1) >= 1,
lambda_min(M2) = 0.25).  Bounds: RES_TOL = 1e-12, the project's solve tolerance; agreement with the specification to the fixture tolerance 1e-7."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch      # (before the library is loaded: see tests/test_gpu_parity.py)

import ipopt_amd
from ipopt_amd import kkt
from tests.support import kktgen
from tests.support import lowrank_spec as lr

pytestmark = pytest.mark.gpu
RES_TOL = 1e-12
FIX_TOL = 1e-7

SYSTEMS = {
    180: lambda: kktgen.grid_kkt(10, 9, dof=2, ncon=1),
    300: lambda: kktgen.lukvl_like(300),
    517: lambda: kktgen.lukvl_like(517, delta_c=1e-8),
    1728: lambda: kktgen.grid_kkt(24, 24, dof=3, ncon=2),
}
PAIRS = [(0, 1), (1, 0), (5, 7), (17, 32), (32, 32)]


def sres(K, x, b):      # (tests/test_gpu_parity.py)
    return np.abs(K @ x - b).max() / (abs(K).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max() + 1e-300)


@functools.lru_cache(maxsize=None)
def system(rows):
    n, r, c, v, m = SYSTEMS[rows]()
    K = kktgen.to_scipy(n, r, c, v).toarray()
    assert n - m == rows
    return dict(n=n, r=r, c=c, v=v, m=m, rows=rows, K=K, ksolve=lr.dense_solver(K))


@functools.lru_cache(maxsize=None)
def reference(rows, nv, nu, u_factor=1.0):
    """V, U, the specification's update, the dense K~ and three right-hand sides with the specification's solutions: computed once, shared, never written"""
    S = system(rows)
    V, U = lr.scaled_columns(S["K"], rows, nv, nu, seed=11, u_factor=u_factor, solve=S["ksolve"])
    upd = lr.update(S["K"], V, U, S["ksolve"])
    Kt = lr.dense_updated(S["K"], V, U)
    rng = np.random.default_rng(5)
    n = S["n"]
    b3 = rng.standard_normal(n); b2 = rng.standard_normal(n); b3[rows:] = 0.0
    B = np.stack([Kt @ np.ones(n), b2, b3])
    X = lr.solve(S["K"], V, U, upd, B.T, S["ksolve"]).T if upd["which"] == 0 else None
    for a in (V, U, Kt, B) + ((X,) if X is not None else ()):
        a.setflags(write=False)
    return dict(V=V, U=U, upd=upd, Kt=Kt, B=B, X=X)


def factored(S, **opts):
    s = ipopt_amd.KKTSolver(**opts)
    s.initialize_structure(S["n"], S["r"], S["c"], vals=S["v"])
    s.values()[:] = S["v"]
    assert s.multi_solve(True, None, True, S["m"]) == kkt.SUCCESS
    return s


def check(Kt, x, b, xs):
    res = sres(Kt, x, b)
    print(f"scaled residual {res:.2e}, |x - x_spec| {np.abs(x - xs).max():.2e}")
    assert res <= RES_TOL
    assert np.abs(x - xs).max() <= FIX_TOL * max(1.0, np.abs(xs).max())


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"nv{p[0]}_nu{p[1]}")
@pytest.mark.parametrize("rows", sorted(SYSTEMS))
def test_lowrank_solve_against_the_dense_updated_system(rows, pair):
    S, R = system(rows), reference(rows, *pair)
    s = factored(S)
    s.lowrank_set(R["V"], R["U"])
    assert s.lowrank_info() == dict(rows=rows, nv=pair[0], nu=pair[1], current=False, update_ms=0.0)
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    assert s.lowrank_info()["current"]
    x = R["B"][0].copy()                                     # nrhs = 1
    s.lowrank_solve(x)
    check(R["Kt"], x, R["B"][0], R["X"][0])
    X = R["B"].copy()                                        # nrhs = 3
    s.lowrank_solve(X)
    for k in range(3):
        check(R["Kt"], X[k], R["B"][k], R["X"][k])
    assert np.array_equal(X[0], x)


def test_device_call_with_a_leading_dimension_beyond_n():
    S, R = system(517), reference(517, 5, 7)
    n, ld = S["n"], S["n"] + 5
    s = factored(S)
    s.lowrank_set(R["V"], R["U"])
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    hb = np.full((3, ld), 7.0); hb[:, :n] = R["B"]
    db = torch.tensor(hb, dtype=torch.float64, device="cuda")
    dx = torch.full((3, ld), -3.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.lowrank_solve_device2(db.data_ptr(), dx.data_ptr(), nrhs=3, ldb=ld, ldx=ld)
    X = dx.cpu().numpy()
    assert np.array_equal(db.cpu().numpy(), hb) and np.all(X[:, n:] == -3.0)          # B untouched, nothing written beyond n
    for k in range(3):
        check(R["Kt"], X[k, :n], R["B"][k], R["X"][k])
    Xh = R["B"].copy(); s.lowrank_solve(Xh)
    assert np.array_equal(Xh, X[:, :n])                                                # the host route is the same computation


def test_rows_equal_to_n_on_a_positive_definite_system_and_the_one_by_one_system():
    n = 40
    r = np.concatenate([np.arange(n), np.arange(1, n)]) + 1; c = np.concatenate([np.arange(n), np.arange(n - 1)]) + 1
    v = np.concatenate([np.full(n, 4.0), np.full(n - 1, -1.0)])
    K = kktgen.to_scipy(n, r, c, v).toarray()
    V, U = lr.scaled_columns(K, n, 5, 7, seed=3)
    upd = lr.update(K, V, U); Kt = lr.dense_updated(K, V, U)
    s = factored(dict(n=n, r=r, c=c, v=v, m=0))
    s.lowrank_set(V, U)
    assert s.lowrank_info()["rows"] == n and s.lowrank_update() == (kkt.SUCCESS, 0)
    b = Kt @ np.ones(n); x = b.copy(); s.lowrank_solve(x)
    check(Kt, x, b, lr.solve(K, V, U, upd, b))
    # K = [-4], V = [1]:  M1 = 1 - 1/4 > 0,  K~ = [-3]
    one = np.array([1], np.int32)
    s = factored(dict(n=1, r=one, c=one, v=np.array([-4.0]), m=1))
    s.lowrank_set(np.array([[1.0]]), None)
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    x = np.array([6.0]); s.lowrank_solve(x)
    assert abs(x[0] + 2.0) <= 4e-16


def test_bitwise_reproducibility():
    S, R = system(517), reference(517, 17, 32)
    s = factored(S)
    s.lowrank_set(R["V"], R["U"])
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    x1 = R["B"].copy(); s.lowrank_solve(x1)
    x2 = R["B"].copy(); s.lowrank_solve(x2)
    assert np.array_equal(x1, x2)                                                      # the same solve twice
    neg, zero = C.c_int(0), C.c_int(0)
    assert s.lib.mi355x_kkt_refactor(s._h, C.byref(neg), C.byref(zero)) == 0           # the same values again
    assert not s.lowrank_info()["current"]
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    x3 = R["B"].copy(); s.lowrank_solve(x3)
    assert np.array_equal(x1, x3)                                                      # update + solve repeated
    rng = np.random.default_rng(9)
    B8 = rng.standard_normal((8, S["n"]))
    X8 = B8.copy(); s.lowrank_solve(X8)
    for k in range(8):
        xk = B8[k].copy(); s.lowrank_solve(xk)
        assert np.array_equal(xk, X8[k]), k                                            # eight columns in one call = eight single calls
    assert max(sres(R["Kt"], X8[k], B8[k]) for k in range(8)) <= RES_TOL
    s.lowrank_set(None, None, rows=0)                                                  # nv = nu = 0: the plain solve, bit for bit
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    xa = B8.copy(); s.lowrank_solve(xa)
    xb = B8.copy(); assert s.multi_solve(False, xb) == 0
    assert np.array_equal(xa, xb)
    s.lowrank_clear()
    assert s.lowrank_info() == dict(rows=0, nv=0, nu=0, current=False, update_ms=0.0)
    with pytest.raises(ipopt_amd.KKTError, match="lowrank_update"):
        s.lowrank_solve(xa)


def test_an_update_that_changes_the_inertia_is_reported_and_not_applied():
    S, R = system(300), reference(300, 5, 7, 2.0)                                      # U doubled: lambda_min(M2) = -2
    assert R["upd"]["which"] == 2
    s = factored(S)
    s.lowrank_set(R["V"], R["U"])
    assert s.lowrank_update() == (kkt.WRONG_INERTIA, 2)
    assert not s.lowrank_info()["current"]
    with pytest.raises(ipopt_amd.KKTError, match="lowrank_update"):
        s.lowrank_solve(R["B"][0].copy())
    G = system(300); Rg = reference(300, 5, 7)                                         # the admissible columns on the same handle
    s.lowrank_set(Rg["V"], Rg["U"])
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    x = Rg["B"][1].copy(); s.lowrank_solve(x)
    check(Rg["Kt"], x, Rg["B"][1], Rg["X"][1])


def test_a_new_factorisation_ends_the_update_until_it_is_renewed():
    S, R = system(180), reference(180, 5, 7)
    s = factored(S)
    s.lowrank_set(R["V"], R["U"])
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    x = R["B"][1].copy(); s.lowrank_solve(x)
    assert s.multi_solve(True, None) == 0                                              # factor
    with pytest.raises(ipopt_amd.KKTError, match="lowrank_update"):
        s.lowrank_solve(R["B"][1].copy())
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    y = R["B"][1].copy(); s.lowrank_solve(y)
    assert np.array_equal(x, y)
    check(R["Kt"], y, R["B"][1], R["X"][1])


def test_columns_set_before_a_delayed_pivot_restructure_survive_it():
    """hostile_band_kkt at the size of tests/test_gpu_pivoting.py: the factorisation moves columns to their parent fronts and rebuilds the structure;
    V and U (caller's numbering) were set before it.  Bound: 10 x the scaled residual the plain solve reaches on this system, measured here -- the
    correction adds two well-conditioned small solves (lambda_min(M) >= 0.25) on top of it."""
    n, r, c, v = kktgen.hostile_band_kkt(2000, frac=0.15, tiny=1e-6, seed=4)
    rows = 2000
    K = kktgen.to_scipy(n, r, c, v).toarray()
    V, U = lr.scaled_columns(K, rows, 5, 7, seed=11)
    Kt = lr.dense_updated(K, V, U)
    s = ipopt_amd.KKTSolver(pivtol=0.01, scaling=0, pivtolmax=0.01, delay_rounds=8)
    s.initialize_structure(n, r, c, vals=v)
    s.lowrank_set(V, U)
    s.values()[:] = v
    b = K @ np.ones(n); x = b.copy()
    assert s.multi_solve(True, x) == kkt.SUCCESS
    I = s.info()
    assert I.num_restructures >= 1 and I.num_small == 0 and I.num_zero == 0
    plain = sres(K, x, b)
    assert s.lowrank_info() == dict(rows=rows, nv=5, nu=7, current=False, update_ms=0.0)
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    bt = Kt @ np.ones(n); xt = bt.copy(); s.lowrank_solve(xt)
    corrected = sres(Kt, xt, bt)
    print(f"plain solve {plain:.2e}, corrected solve {corrected:.2e}")
    assert plain <= RES_TOL and corrected <= 10.0 * plain


def _pd_system(seed):
    """the set-up of tests/test_gpu_pd_system.py, up to the factorisation"""
    from tests.test_gpu_pd_system import build
    P = build(seed)
    nx, ns, nc, nd = P["nx"], P["ns"], P["nc"], P["nd"]
    sig_x = np.zeros(nx); np.add.at(sig_x, P["ixl"], P["zl"] / P["sxl"]); np.add.at(sig_x, P["ixu"], P["zu"] / P["sxu"])
    sig_s = np.zeros(ns); np.add.at(sig_s, P["isl"], P["vl"] / P["ssl"]); np.add.at(sig_s, P["isu"], P["vu"] / P["ssu"])
    deltas = (30.0, 0.5, 1e-3, 2e-3)
    dx, ds, dc, dd = deltas
    wr, wc, wv = P["wt"]; jcr, jcc, jcv = P["jct"]; jdr, jdc, jdv = P["jdt"]
    ar = lambda n, o: np.arange(n) + o
    irn = np.concatenate([wr, ar(nx, 0), ar(ns, nx), jcr + nx + ns, ar(nc, nx + ns), jdr + nx + ns + nc, ar(nd, nx + ns + nc), ar(nd, nx + ns + nc)]) + 1
    jcn = np.concatenate([wc, ar(nx, 0), ar(ns, nx), jcc, ar(nc, nx + ns), jdc, ar(ns, nx), ar(nd, nx + ns + nc)]) + 1
    lens = [len(wv), nx, ns, len(jcv), nc, len(jdv), ns, nd]
    srcs = [wv, sig_x, sig_s, jcv, np.zeros(nc), jdv, np.zeros(ns), np.zeros(nd)]
    scale = np.array([1, 1, 1, 1, 0, 1, 0, 0], dtype=float); shift = np.array([0, dx, ds, 0, -dc, 0, -1, -dd], dtype=float)
    vals0 = np.concatenate([sc * np.asarray(v) + sh for sc, sh, v in zip(scale, shift, srcs)])
    n4 = nx + ns + nc + nd
    s = ipopt_amd.KKTSolver(scaling=0)
    s.initialize_structure(n4, irn, jcn, vals=vals0)
    s.assembly_define(lens)
    for q, v in enumerate(srcs):
        s.assembly_set(q, v)
    st, neg, zero = s.factor_assembled(scale, shift)
    assert st == 0 and neg == nc + nd
    nb = [len(P["ixl"]), len(P["ixu"]), len(P["isl"]), len(P["isu"])]
    s.pd_define([nx, ns, nc, nd] + nb, P["ixl"], P["ixu"], P["isl"], P["isu"], irn, jcn, [0, 3, 5])
    s.pd_put_data([P["zl"], P["zu"], P["vl"], P["vu"], P["sxl"], P["sxu"], P["ssl"], P["ssu"]])
    K4 = kktgen.to_scipy(n4, irn.astype(np.int32), jcn.astype(np.int32), vals0).toarray()
    return P, s, K4, deltas, (scale, shift)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_primal_dual_hooks_match_the_dense_eight_block_system_with_the_update(seed):
    """the four assertions of tests/test_gpu_pd_system.py with their tolerances, the dense K8's x block carrying V V^T - U U^T and the W segment B0 only"""
    from tests.test_gpu_pd_system import dense_k8
    P, s, K4, (dx, ds, dc, dd), _ = _pd_system(seed)
    nx = P["nx"]
    V, U = lr.scaled_columns(K4, nx, 5, 7, seed=11)
    s.lowrank_set(V, U)
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    K, off = dense_k8(P, dx, ds, dc, dd)
    K[:nx, :nx] += V @ V.T - U @ U.T
    rng = np.random.default_rng(100 + seed)
    split = lambda v: [v[off[i]:off[i + 1]] for i in range(8)]
    rhs = rng.standard_normal(off[-1])
    s.pd_put(0, split(rhs))
    s.pd_solve_once(0, 1, 1.0, 0.0)
    res = np.concatenate(s.pd_get(1))
    ref = np.linalg.solve(K, rhs)
    assert np.abs(res - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
    pert = res + 1e-3 * rng.standard_normal(off[-1])
    s.pd_put(1, split(pert))
    nr = s.pd_residual(0, 1, 2, [dx, ds, dc, dd])
    resid = np.concatenate(s.pd_get(2))
    rref = K @ pert - rhs
    assert np.abs(resid - rref).max() <= 1e-12 * max(1.0, np.abs(K).sum(axis=1).max() * np.abs(pert).max())
    assert np.allclose(nr, [np.abs(rhs).max(), np.abs(pert).max(), np.abs(rref).max()], rtol=1e-12, atol=0)
    s.pd_solve_once(2, 1, -1.0, 1.0)
    back = np.concatenate(s.pd_get(1))
    assert np.abs(back - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
    s.pd_put(1, split(pert))
    s.pd_solve_once(0, 1, 0.5, 2.0)
    mix = np.concatenate(s.pd_get(1))
    assert np.abs(mix - (0.5 * ref + 2.0 * pert)).max() <= 1e-9 * max(1.0, np.abs(ref).max())


def test_primal_dual_hooks_refuse_a_stale_update_and_columns_beyond_the_x_block():
    P, s, K4, deltas, (scale, shift) = _pd_system(0)
    nx = P["nx"]
    V, U = lr.scaled_columns(K4, nx, 2, 2, seed=1)
    s.lowrank_set(V, U)
    with pytest.raises(ipopt_amd.KKTError, match="lowrank_update"):
        s.pd_solve_once(0, 1)                                                          # set, never updated
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    s.pd_solve_once(0, 1)
    assert s.factor_assembled(scale, shift)[0] == 0
    with pytest.raises(ipopt_amd.KKTError, match="lowrank_update"):
        s.pd_solve_once(0, 1)                                                          # a new factorisation since
    s.lowrank_set(np.ones((nx + 1, 1)), None)
    with pytest.raises(ipopt_amd.KKTError, match="n_x"):
        s.pd_residual(0, 1, 2, list(deltas))
    with pytest.raises(ipopt_amd.KKTError, match="n_x"):
        s.pd_solve_once(0, 1)
    s.lowrank_clear()
    s.pd_solve_once(0, 1)                                                              # no update: today's sequence
