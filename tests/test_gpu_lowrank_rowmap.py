"""-m gpu: low-rank updates and quasi-Newton histories on an index subset of x (mi355x_kkt_lowrank_rowmap, mi355x_kkt_lbfgs_push_mapped; the reference's
P_LowRank: IpLowRankAugSystemSolver.cpp:274-290, :449-457, IpLimMemQuasiNewtonUpdater.cpp:169-193, :313-325).  Specification: tests/support/rowmap_spec.py,
the permuted statement of tests/support/lowrank_spec.py.  Systems and bounds are those of tests/test_gpu_lowrank.py: RES_TOL = 1e-12 for the scaled
residual against the dense K~, FIX_TOL = 1e-7 against the specification.  Maps (rowmap_spec.make_idx) hold index 0 and index n_x - 1, the rest drawn
with default_rng(3):

  n_x   mapped rows        (nv, nu)   covers
  180   1 (index n_x//2)   (1, 1)     a single mapped row
  180   179                (5, 7)     all but one row
  517   300                (17, 32)   no multiple of 64 or 256
  1728  1100               (32, 32)   crosses the 1024-row slab; every lane layout of the Gram
  1728  1100               (0, 1)     empty V side
  1728  1100               (1, 0)     empty U side

The single-row case is the hard one for the algebra, not for the kernels: V = 101.5 and U = 98.3 on one diagonal entry nearly cancel, and the float64
specification itself reaches 1.1e-12 on its first right-hand side there (tests/test_rowmap_spec.py)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch      # (before the library is loaded: see tests/test_gpu_parity.py)

import ipopt_amd
from ipopt_amd import kkt
from tests.support import kktgen
from tests.support import lbfgs_spec as lb
from tests.support import lowrank_spec as lr
from tests.support import resto_spec as rs
from tests.support import rowmap_spec as rm
from tests.support import sr1_spec as sr
from tests.test_gpu_lbfgs import factor, snapshot, same, dev
from tests.test_gpu_lowrank import system, sres, factored, check, reference as unmapped_reference, _pd_system, RES_TOL, FIX_TOL
from tests.test_gpu_resto import snapshot as resto_snapshot, same as resto_same
from tests.test_gpu_sr1 import snap as sr1_snap, same_sr1

pytestmark = pytest.mark.gpu
IDS = [f"nx{nx}_rows{rows}_nv{p[0]}_nu{p[1]}" for nx, rows, p in rm.CASES]


@functools.lru_cache(maxsize=None)
def reference(nx, rows, nv, nu):
    """the map, V, U, the specification's update, the dense K~ and three right-hand sides with the specification's solutions: computed once, shared, never written"""
    S = system(nx)
    n = S["n"]
    idx = rm.make_idx(nx, rows)
    M = rm.Mapped(S["K"], idx, nv, nu)
    assert M.upd["which"] == 0
    rng = np.random.default_rng(5)
    b2 = rng.standard_normal(n); b3 = rng.standard_normal(n)
    outside = np.ones(n, bool); outside[idx] = False; b3[outside] = 0.0
    B = np.stack([M.Kt @ np.ones(n), b2, b3])
    X = M.solve(B.T).T
    for a in (idx, M.V, M.U, M.Kt, B, X):
        a.setflags(write=False)
    return dict(idx=idx, V=M.V, U=M.U, Kt=M.Kt, B=B, X=X)


def mapped(S, R, **opts):
    """a factored handle with the map and the columns of R set and the update in force"""
    s = factored(S, **opts)
    s.lowrank_rowmap(R["idx"])
    s.lowrank_set(R["V"], R["U"])
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    return s


# ---- 1. the mapped solve against the dense updated system ----
@pytest.mark.parametrize("nx,rows,pair", rm.CASES, ids=IDS)
def test_mapped_solve_against_the_dense_updated_system(nx, rows, pair):
    S, R = system(nx), reference(nx, rows, *pair)
    s = factored(S)
    assert s.lowrank_rowmap_info() is None
    s.lowrank_rowmap(R["idx"])
    s.lowrank_set(R["V"], R["U"])
    assert s.lowrank_info() == dict(rows=rows, nv=pair[0], nu=pair[1], current=False, update_ms=0.0)      # the reduced space
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    got = s.lowrank_rowmap_info()
    assert got.dtype == np.int32 and np.array_equal(got, R["idx"])
    X = R["B"].copy()
    s.lowrank_solve(X)
    for k in range(3):
        check(R["Kt"], X[k], R["B"][k], R["X"][k])


# ---- 2. the identity map is the unmapped path, bit for bit ----
def test_identity_map_solve_is_the_unmapped_solve_bitwise():
    S, R = system(517), unmapped_reference(517, 5, 7)
    a, b = factored(S), factored(S)
    a.lowrank_rowmap(np.arange(517))
    for s in (a, b):
        s.lowrank_set(R["V"], R["U"])
        assert s.lowrank_update() == (kkt.SUCCESS, 0)
    Xa = R["B"].copy(); a.lowrank_solve(Xa)
    Xb = R["B"].copy(); b.lowrank_solve(Xb)
    assert np.array_equal(Xa, Xb)
    assert max(sres(R["Kt"], Xa[k], R["B"][k]) for k in range(3)) <= RES_TOL


def test_identity_map_primal_dual_hooks_are_the_unmapped_hooks_bitwise():
    outs = []
    for use_map in (True, False):
        P, s, K4, deltas, _ = _pd_system(0)
        nx = P["nx"]
        V, U = lr.scaled_columns(K4, nx, 5, 7, seed=11)
        if use_map:
            s.lowrank_rowmap(np.arange(nx))
        s.lowrank_set(V, U)
        assert s.lowrank_update() == (kkt.SUCCESS, 0)
        rng = np.random.default_rng(100)
        lens = [len(b) for b in s.pd_get(0)]
        off = np.concatenate([[0], np.cumsum(lens)])
        split = lambda v: [v[off[i]:off[i + 1]] for i in range(8)]
        rhs = rng.standard_normal(off[-1])
        s.pd_put(0, split(rhs))
        s.pd_solve_once(0, 1, 1.0, 0.0)
        res = np.concatenate(s.pd_get(1))
        s.pd_put(1, split(res + 1e-3 * rng.standard_normal(off[-1])))
        nr = s.pd_residual(0, 1, 2, list(deltas))
        outs.append((res, np.concatenate(s.pd_get(2)), np.asarray(nr)))
    for x, y in zip(*outs):
        assert np.array_equal(x, y)


def test_identity_map_history_columns_are_the_unmapped_columns_bitwise():
    rows = 517
    Sp, Yp = lb.make_pairs(rows, 3, seed=8)
    got = []
    for use_map in (True, False):
        s = factored(system(rows))
        if use_map:
            s.lowrank_rowmap(np.arange(rows))
        s.lbfgs_define(rows, max_history=6)
        for j in range(3):
            assert s.lbfgs_push(Sp[:, j], Yp[:, j]) == kkt.LBFGS_STORED
        got.append((s.lbfgs_get(2), s.lbfgs_get(3)))
    assert got[0][0].shape == (rows, 3) and np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


# ---- 3. against the route users have today: the same update, unmapped, as zero-padded columns of n_x rows ----
@pytest.mark.parametrize("nx,rows,pair", [rm.CASES[2], rm.CASES[3]], ids=[IDS[2], IDS[3]])
def test_mapped_solve_agrees_with_zero_padded_columns(nx, rows, pair):
    S, R = system(nx), reference(nx, rows, *pair)
    a = mapped(S, R)
    b = factored(S)
    b.lowrank_set(rm.expand(R["V"], R["idx"], nx), rm.expand(R["U"], R["idx"], nx))
    assert b.lowrank_info()["rows"] == nx and b.lowrank_update() == (kkt.SUCCESS, 0)
    Xa = R["B"].copy(); a.lowrank_solve(Xa)
    Xb = R["B"].copy(); b.lowrank_solve(Xb)
    for k in range(3):
        ra, rb, d = sres(R["Kt"], Xa[k], R["B"][k]), sres(R["Kt"], Xb[k], R["B"][k]), np.abs(Xa[k] - Xb[k]).max()
        print(f"right-hand side {k}: mapped {ra:.2e}, zero-padded {rb:.2e}, |x_mapped - x_padded| {d:.2e}")
        assert ra <= RES_TOL and rb <= RES_TOL
        assert d <= FIX_TOL * max(1.0, np.abs(Xb[k]).max())


# ---- 4. reproducibility ----
def test_mapped_calls_are_bitwise_reproducible_and_columns_do_not_depend_on_their_company():
    nx, rows, pair = rm.CASES[3]
    S, R = system(nx), reference(nx, rows, *pair)
    a, b = mapped(S, R), mapped(S, R)
    Xa = R["B"].copy(); a.lowrank_solve(Xa)
    Xb = R["B"].copy(); b.lowrank_solve(Xb)
    assert np.array_equal(Xa, Xb)                                                      # a fresh handle: the same bits
    for k in range(3):
        x = R["B"][k].copy(); a.lowrank_solve(x)
        assert np.array_equal(x, Xa[k]), k                                             # 1 against 3 columns


# ---- 5. the primal-dual hooks under a map ----
def _pd_map(P, K4):
    nx = P["nx"]
    idx = rm.make_idx(nx, max(2, (3 * nx) // 5))
    return idx, rm.Mapped(K4, idx, 5, 7)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_primal_dual_hooks_match_the_dense_eight_block_system_with_the_mapped_update(seed):
    """the four assertions of tests/test_gpu_lowrank.py's test with their tolerances, the update embedded in the x block through the map"""
    from tests.test_gpu_pd_system import dense_k8
    P, s, K4, (dx, ds, dc, dd), _ = _pd_system(seed)
    idx, M = _pd_map(P, K4)
    assert M.upd["which"] == 0
    s.lowrank_rowmap(idx)
    s.lowrank_set(M.V, M.U)
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    K, off = dense_k8(P, dx, ds, dc, dd)
    K[np.ix_(idx, idx)] += M.V @ M.V.T - M.U @ M.U.T
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


def test_primal_dual_hooks_refuse_a_stale_update_and_a_map_beyond_the_x_block():
    P, s, K4, deltas, (scale, shift) = _pd_system(0)
    nx = P["nx"]
    idx, M = _pd_map(P, K4)
    s.lowrank_rowmap(idx)
    s.lowrank_set(M.V, M.U)
    with pytest.raises(ipopt_amd.KKTError, match="lowrank_update"):
        s.pd_solve_once(0, 1)                                                          # set, never updated
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    s.pd_solve_once(0, 1)
    assert s.factor_assembled(scale, shift)[0] == 0
    with pytest.raises(ipopt_amd.KKTError, match="lowrank_update"):
        s.pd_solve_once(0, 1)                                                          # a new factorisation since
    s.lowrank_clear()
    s.lowrank_rowmap(np.array([0, nx]))                                                # valid for the system (nx < n), beyond the x block
    s.lowrank_set(np.ones((2, 1)), None)
    with pytest.raises(ipopt_amd.KKTError, match="n_x"):
        s.pd_residual(0, 1, 2, list(deltas))
    with pytest.raises(ipopt_amd.KKTError, match="n_x"):
        s.pd_solve_once(0, 1)
    s.lowrank_clear()
    s.pd_solve_once(0, 1)                                                              # no update: today's sequence, the map alone changes nothing


# ---- 6. histories under a map ----
NX, ROWS, K = 517, 300, 6


def mapped_handle(idx, with_map=True):
    """an analysed handle on the system of NX whose MAPPED x diagonal appears a second time, as duplicate triplets that carry sigma (the caller's side of
    ReducedDiag: sigma on the mapped diagonal entries, 0 elsewhere); -> (solver, values(sigma))"""
    S = system(NX)
    ix = (np.asarray(idx) + 1).astype(S["r"].dtype)
    r2, c2 = np.concatenate([S["r"], ix]), np.concatenate([S["c"], ix])
    vals = lambda sigma: np.concatenate([S["v"], np.full(len(idx), sigma)])
    s = ipopt_amd.KKTSolver()
    s.initialize_structure(S["n"], r2, c2, vals=vals(1.0))
    if with_map:
        s.lowrank_rowmap(idx)
    return s, vals


def test_bfgs_mapped_pushes_are_the_pushes_of_the_gathered_vectors_bitwise():
    idx = rm.make_idx(NX, ROWS)
    Sx, Yx = lb.make_pairs(NX, K + 3, seed=41)                                         # full-space pairs
    dS = torch.tensor(Sx.T.copy(), dtype=torch.float64, device="cuda"); dY = torch.tensor(Yx.T.copy(), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    (a, vals), (b, _), (c, _) = mapped_handle(idx), mapped_handle(idx, with_map=False), mapped_handle(idx)
    for s in (a, b, c):
        s.lbfgs_define(ROWS, max_history=K)
    H64, Hld = lb.History(ROWS, K), lb.History(ROWS, K, dtype=np.longdouble)
    for j in range(K + 3):
        assert a.lbfgs_push_mapped(Sx[:, j], Yx[:, j]) == kkt.LBFGS_STORED
        assert b.lbfgs_push(Sx[idx, j], Yx[idx, j]) == kkt.LBFGS_STORED
        assert c.lbfgs_push_mapped_device(dS[j].data_ptr(), dY[j].data_ptr(), NX) == kkt.LBFGS_STORED
        assert H64.push(Sx[idx, j], Yx[idx, j]) == lb.STORED and Hld.push(Sx[idx, j], Yx[idx, j]) == lb.STORED
        if j + 1 in (1, K, K + 3):
            sa = snapshot(a)                                                           # S, Y, V, U, D, L, S^T S, sigma and both infos
            assert same(sa, snapshot(b)), f"mapped push and push of the gathered vectors differ after {j + 1}"
            assert same(sa, snapshot(c)), f"host and device mapped push differ after {j + 1}"
    assert np.array_equal(dS.cpu().numpy(), Sx.T) and np.array_equal(dY.cpu().numpy(), Yx.T)              # the caller's vectors are only read
    assert np.array_equal(a.lbfgs_get("S"), Sx[idx, 3:]) and a.lowrank_info()["rows"] == ROWS
    with pytest.raises(ipopt_amd.KKTError, match="len"):                               # len <= idx[rows-1]
        a.lbfgs_push_mapped(Sx[:NX - 1, 0], Yx[:NX - 1, 0])
    # dense: K with sigma on the mapped diagonal plus P (V V^T - U U^T) P^T against the recursive BFGS matrix embedded through the map;
    # the bound of tests/test_gpu_lbfgs.py: e_dev <= 64 max(e_64, 2^-52)
    S = system(NX)
    sigma, V, U = a.lbfgs_info()["sigma"], a.lbfgs_get("V"), a.lbfgs_get("U")
    ii = np.ix_(idx, idx)
    def embed(B):
        Kf = S["K"].astype(B.dtype); Kf[ii] += B
        return Kf
    Kld = embed(lb.dense(*lb.recursive_terms(Hld.S, Hld.Y, Hld.sigma), Hld.sigma))
    Kdev, K64 = embed(lb.dense(V, U, sigma)), embed(lb.dense(H64.V, H64.U, H64.sigma))
    e_dev, e_64 = dev(Kdev, Kld), dev(K64, Kld)
    e_dev_r, e_64_r = dev(Kdev[ii], Kld[ii]), dev(K64[ii], Kld[ii])
    print(f"embedded: e_dev {e_dev:.2e} e_64 {e_64:.2e}; mapped block alone: e_dev {e_dev_r:.2e} e_64 {e_64_r:.2e}")
    assert e_dev <= 64.0 * max(e_64, 2.0 ** -52) and e_dev_r <= 64.0 * max(e_64_r, 2.0 ** -52)
    # and the chain closes: factor with sigma on the mapped diagonal, update, solve
    factor(a, vals, sigma, S["m"])
    assert a.lowrank_update() == (kkt.SUCCESS, 0)
    Kt = np.asarray(Kdev, dtype=np.float64)
    bt = Kt @ np.ones(S["n"]); x = bt.copy(); a.lowrank_solve(x)
    res = sres(Kt, x, bt)
    print(f"sigma {sigma:.3f}, scaled residual {res:.2e}")
    assert res <= RES_TOL


def test_sr1_mapped_pushes_and_one_undo_re_form_the_columns_bitwise():
    idx = rm.make_idx(NX, ROWS)
    Sx, Yx = sr.make_pairs(NX, K + 3, seed=2000 + NX + K)
    (a, _), (b, _) = mapped_handle(idx), mapped_handle(idx, with_map=False)
    H = sr.History(ROWS, K)
    for s in (a, b):
        s.lbfgs_define_sr1(ROWS, max_history=K)
    before = None
    for j in range(K + 3):
        want = H.push(Sx[idx, j], Yx[idx, j])
        if j == K + 2:
            assert want == sr.STORED                                                   # (the push that is taken back below is a stored one)
            before = sr1_snap(a)
        assert a.lbfgs_push_mapped(Sx[:, j], Yx[:, j]) == want
        assert b.lbfgs_push(Sx[idx, j], Yx[idx, j]) == want
    assert same_sr1(sr1_snap(a), sr1_snap(b))
    assert a.lbfgs_undo() == 1 and b.lbfgs_undo() == 1
    after = sr1_snap(a)
    assert same_sr1(after, sr1_snap(b))
    assert np.array_equal(after[0]["V"], before[0]["V"]) and np.array_equal(after[0]["U"], before[0]["U"])      # re-formed from the ring, bit for bit
    assert np.array_equal(after[0]["S"], before[0]["S"]) and after[1]["sigma"] == before[1]["sigma"]


@pytest.mark.parametrize("special", [False, True], ids=["special0", "special1"])
def test_resto_mapped_pushes_are_the_pushes_of_the_gathered_vectors_bitwise(special):
    idx = rm.make_idx(NX, ROWS)
    Sx, Yx, DRx = rs.make_resto(NX, K + 3, seed=3000 + NX + K)
    dS = torch.tensor(Sx.T.copy(), dtype=torch.float64, device="cuda"); dY = torch.tensor(Yx.T.copy(), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    (a, _), (b, _), (c, _) = mapped_handle(idx), mapped_handle(idx, with_map=False), mapped_handle(idx)
    for s in (a, b, c):
        s.lbfgs_define_resto(ROWS, DRx[idx], max_history=K, type=rs.BFGS, special=special)      # DR is gathered by the caller, once
    for j in range(K + 3):
        eta = rs.ETAS[j % 4]
        oc = b.lbfgs_push_resto(Sx[idx, j], Yx[idx, j], eta)
        assert oc == kkt.LBFGS_STORED
        assert a.lbfgs_push_resto_mapped(Sx[:, j], Yx[:, j], eta) == oc
        assert c.lbfgs_push_resto_mapped_device(dS[j].data_ptr(), dY[j].data_ptr(), NX, eta) == oc
        if j + 1 in (1, K, K + 3):
            sa = resto_snapshot(a)
            assert resto_same(sa, resto_snapshot(b)), f"mapped push and push of the gathered vectors differ after {j + 1}"
            assert resto_same(sa, resto_snapshot(c)), f"host and device mapped push differ after {j + 1}"


# ---- 7. the state rules ----
def test_the_map_cannot_change_under_an_update_or_a_history_and_fixes_rows():
    nx, rows, pair = rm.CASES[1]
    S, R = system(nx), reference(nx, rows, *pair)
    s = mapped(S, R)
    for new in (R["idx"][:5], None):
        with pytest.raises(ipopt_amd.KKTError, match="low-rank update is set"):
            s.lowrank_rowmap(new)
    s.lowrank_clear()
    s.lbfgs_define(rows, max_history=3)
    for new in (R["idx"][:5], None):
        with pytest.raises(ipopt_amd.KKTError, match="history is defined"):
            s.lowrank_rowmap(new)
    s.lbfgs_reset()
    assert np.array_equal(s.lowrank_rowmap_info(), R["idx"])                           # survives lbfgs_reset
    s.lbfgs_clear()
    assert np.array_equal(s.lowrank_rowmap_info(), R["idx"])                           # survives lowrank_clear and lbfgs_clear
    with pytest.raises(ipopt_amd.KKTError, match="rows"):
        s.lowrank_set(np.ones((rows - 1, 2)), None)
    with pytest.raises(ipopt_amd.KKTError, match="rows"):
        s.lbfgs_define(rows - 1)
    with pytest.raises(ipopt_amd.KKTError, match="rows"):
        s.lbfgs_define_sr1(rows + 1)
    with pytest.raises(ipopt_amd.KKTError, match="rows"):
        s.lbfgs_define_resto(rows - 1, np.ones(rows - 1))
    assert s.lowrank_info()["rows"] == 0 and s.lbfgs_info()["rows"] == 0               # nothing was installed by the refused calls
    s.lowrank_set(R["V"], R["U"])
    neg, zero = C.c_int(0), C.c_int(0)
    assert s.lib.mi355x_kkt_refactor(s._h, C.byref(neg), C.byref(zero)) == 0           # survives a refactorisation
    assert np.array_equal(s.lowrank_rowmap_info(), R["idx"]) and not s.lowrank_info()["current"]
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    x = R["B"][1].copy(); s.lowrank_solve(x)
    check(R["Kt"], x, R["B"][1], R["X"][1])
    s.lowrank_clear()
    s.lowrank_rowmap(None)                                                             # removed: the first `rows` indices again
    assert s.lowrank_rowmap_info() is None
    s.lowrank_set(np.ones((rows - 1, 2)), None)
    assert s.lowrank_info()["rows"] == rows - 1


def test_map_and_columns_set_before_a_delayed_pivot_restructure_survive_it():
    """test_columns_set_before_a_delayed_pivot_restructure_survive_it of tests/test_gpu_lowrank.py with a 1 200-row map: the map is stated in the caller's
    numbering, so the structure edit does not touch it.  The bound is that test's: 10 x the scaled residual of the plain solve on this system."""
    n, r, c, v = kktgen.hostile_band_kkt(2000, frac=0.15, tiny=1e-6, seed=4)
    K = kktgen.to_scipy(n, r, c, v).toarray()
    idx = rm.make_idx(2000, 1200)
    M = rm.Mapped(K, idx, 5, 7)
    s = ipopt_amd.KKTSolver(pivtol=0.01, scaling=0, pivtolmax=0.01, delay_rounds=8)
    s.initialize_structure(n, r, c, vals=v)
    s.lowrank_rowmap(idx)
    s.lowrank_set(M.V, M.U)
    s.values()[:] = v
    b = K @ np.ones(n); x = b.copy()
    assert s.multi_solve(True, x) == kkt.SUCCESS
    I = s.info()
    assert I.num_restructures >= 1 and I.num_small == 0 and I.num_zero == 0
    plain = sres(K, x, b)
    assert np.array_equal(s.lowrank_rowmap_info(), idx)
    assert s.lowrank_info() == dict(rows=1200, nv=5, nu=7, current=False, update_ms=0.0)
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    bt = M.Kt @ np.ones(n); xt = bt.copy(); s.lowrank_solve(xt)
    corrected = sres(M.Kt, xt, bt)
    print(f"plain solve {plain:.2e}, corrected solve {corrected:.2e}")
    assert plain <= RES_TOL and corrected <= 10.0 * plain
