"""-m gpu: the restoration-phase limited-memory history of the C ABI (mi355x_kkt_lbfgs_define_resto, _lbfgs_push_resto; reference
IpLimMemQuasiNewtonUpdater.cpp with update_for_resto_) against its numpy statements (tests/support/resto_spec.py) in longdouble, and through the whole
chain push -> factor K + B0 -> lowrank_update -> lowrank_solve with B0 = sigma I or the vector eta DR.
Sizes are those of tests/test_gpu_lbfgs.py for the same reasons: `rows` 180 (below one 256-row block of the form kernels), 517 (no multiple of 64 /
256), 1728 (two 1024-row slabs of k_lb_dots_resto); max_history 1, 2, 6 (loops unrolled to 8), 12 (to 16), 32 (to 32).  Pairs: resto_spec.make_resto,
seed 3000 + rows + k, eta cycling through 0.3, 0.3, 0.1, 0.03 (tests/test_resto_spec.py states what these inputs are checked for).

Bound of the comparisons: e_dev <= 64 max(e_64, 2^-52), e = max|A - A_ld| / max|A_ld|; A_ld is the longdouble `Literal` (the reference's flow on full
vectors) for D, L, sigma, V V^T, U U^T and B0 + V V^T - U U^T, and the longdouble `History` for G, S^T S and R, which the literal flow does not keep;
e_64 is the float64 `History`'s own deviation from the same A_ld.  Solves: RES_TOL and FIX_TOL of tests/test_gpu_lowrank.py."""
import numpy as np
import pytest
import torch      # (before the library is loaded: see tests/test_gpu_parity.py)

import ipopt_amd
from ipopt_amd import kkt
from tests.support import lowrank_spec as lr
from tests.support import resto_spec as rs
from tests.test_gpu_lbfgs import handle, factor, dev
from tests.test_gpu_lowrank import system, sres, RES_TOL, FIX_TOL

pytestmark = pytest.mark.gpu
ROWS = [180, 517, 1728]
WHAT = ("S", "Ypart", "V", "U", "D", "L", "STS", "G", "R", "eta_col", "dv", "DR")
BOTH = [(rs.BFGS, False), (rs.BFGS, True), (rs.SR1, False), (rs.SR1, True)]


def resto_handle(rows, k, DR, type_, special, **kw):
    s, vals = handle(rows)
    s.lbfgs_define_resto(rows, DR, max_history=k, type=type_, special=special, **kw)
    return s, vals


def snapshot(s):
    return {w: s.lbfgs_get(w) for w in WHAT}, s.lbfgs_info(), s.lowrank_info(), s.lbfgs_resto_info(), s.lbfgs_sr1_info()


def same(a, b, but_counter=False):
    """bitwise; but_counter: skipped_in_a_row and can_undo, the two things a skip or an undo may move, are left out"""
    (A, ia, la, ra, sa), (B, ib, lb_, rb, sb) = a, b
    ia, ib, sa, sb = dict(ia, push_ms=0.0), dict(ib, push_ms=0.0), dict(sa), dict(sb)
    if but_counter:
        ia["skipped_in_a_row"] = ib["skipped_in_a_row"] = 0
        sa["can_undo"] = sb["can_undo"] = False
    Ea, Eb = sa.pop("E"), sb.pop("E")
    return all(np.array_equal(A[w], B[w], equal_nan=True) and A[w].shape == B[w].shape for w in WHAT) and np.array_equal(Ea, Eb) and (ia, la, ra, sa) == (ib, lb_, rb, sb)


def b0(s, DR):
    I, R = s.lbfgs_info(), s.lbfgs_resto_info()
    return R["eta"] * DR if R["special"] else np.full(I["rows"], I["sigma"])


def flow(X):
    return {"D": X.D, "L": X.L, "sigma": np.atleast_1d(X.sigma), "V V^T": X.V @ X.V.T, "U U^T": X.U @ X.U.T, "B0 + V V^T - U U^T": rs.dense(X)}


def grams(X):
    return {"G": np.tril(X.G), "STS": X.STS, "R": X.R}


def dense(V, U, diag):
    B = V @ V.T - U @ U.T
    B[np.diag_indices(B.shape[0])] += diag
    return B


@pytest.mark.parametrize("k", [1, 2, 6, 12, 32])
@pytest.mark.parametrize("type_,special", BOTH)
@pytest.mark.parametrize("rows", ROWS)
def test_columns_against_the_longdouble_specification(rows, type_, special, k):
    Sp, Yp, DR = rs.make_resto(rows, k + 3, seed=3000 + rows + k, sr1=type_ == rs.SR1)
    s, _ = resto_handle(rows, k, DR, type_, special)
    H64, Hld, Lld = (cls(rows, k, DR, type=type_, special=special, dtype=dt) for cls, dt in ((rs.History, np.float64), (rs.History, np.longdouble), (rs.Literal, np.longdouble)))
    assert s.lbfgs_resto_info() == dict(resto=True, special=special, eta=-1.0)
    assert s.lbfgs_info() == dict(rows=rows, max_history=k, memory=0, sigma=-1.0 if special else 1.0, skipped_in_a_row=0, push_ms=0.0)
    assert np.array_equal(s.lbfgs_get("DR"), DR)
    worst = 0.0
    for j in range(k + 3):
        eta = rs.ETAS[j % 4]
        assert s.lbfgs_push_resto(Sp[:, j], Yp[:, j], eta) == kkt.LBFGS_STORED
        assert [X.push(Sp[:, j], Yp[:, j], eta) for X in (H64, Hld, Lld)] == [rs.STORED] * 3
        if j + 1 not in (1, k, k + 3):
            continue
        m = min(j + 1, k)
        got, info, lri, ri, si = snapshot(s)
        assert info["memory"] == m and info["skipped_in_a_row"] == 0 and ri["eta"] == eta
        nneg = Lld.nneg if type_ == rs.SR1 else m
        assert si["type"] == type_ and (type_ == rs.BFGS or si["nneg"] == nneg)
        assert lri == dict(rows=rows, nv=m - nneg if type_ == rs.SR1 else m, nu=nneg, current=False, update_ms=0.0)
        lo = j + 1 - m
        assert np.array_equal(got["S"], Sp[:, lo:j + 1]) and np.array_equal(got["Ypart"], Yp[:, lo:j + 1])      # bitwise, oldest first, through the ring
        assert np.array_equal(got["eta_col"], [rs.ETAS[i % 4] for i in range(lo, j + 1)])
        diag = b0(s, DR)
        mine = {"D": got["D"], "L": got["L"], "sigma": np.array([info["sigma"]]), "V V^T": got["V"] @ got["V"].T, "U U^T": got["U"] @ got["U"].T,
                "B0 + V V^T - U U^T": dense(got["V"], got["U"], diag), "G": got["G"], "STS": got["STS"], "R": got["R"]}
        a64, ald = {**flow(H64), **grams(H64)}, {**flow(Lld), **grams(Hld)}
        for name, A in mine.items():
            assert A.shape == ald[name].shape, name
            if not np.abs(ald[name]).max() > 0:                       # L of a single pair, R of a history that is not special, an empty half of the split
                assert (name == "L" and m == 1) or (name == "R" and not special) or (type_ == rs.SR1 and ((name == "U U^T" and nneg == 0) or (name == "V V^T" and nneg == m))), name
                assert not A.any(), name
                continue
            e_dev, e_64 = dev(A, ald[name]), dev(a64[name], ald[name])
            ratio = e_dev / max(e_64, 2.0 ** -52)
            worst = max(worst, ratio)
            print(f"rows {rows} type {type_} special {int(special)} k {k} after {j + 1}: {name}: e_dev {e_dev:.2e} e_64 {e_64:.2e} ratio {ratio:.2f}")
            assert e_dev <= 64.0 * max(e_64, 2.0 ** -52), (name, e_dev, e_64)
        assert np.all(np.triu(got["L"]) == 0.0) and np.all(np.triu(got["G"], 1) == 0.0)
    print(f"rows {rows} type {type_} special {int(special)} k {k}: largest e_dev / max(e_64, 2^-52) = {worst:.2f}")


@pytest.mark.parametrize("rows,k,type_,special", [(517, 32, rs.BFGS, True), (1728, 12, rs.BFGS, False), (1728, 6, rs.SR1, False), (180, 12, rs.SR1, True)])
def test_host_and_device_pushes_and_fresh_handles_give_the_same_bits(rows, k, type_, special):
    Sp, Yp, DR = rs.make_resto(rows, k + 3, seed=3000 + rows + k, sr1=type_ == rs.SR1)
    dS = torch.tensor(Sp.T.copy(), dtype=torch.float64, device="cuda"); dY = torch.tensor(Yp.T.copy(), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    a, b, c = (resto_handle(rows, k, DR, type_, special)[0] for _ in range(3))
    for j in range(k + 3):
        eta = rs.ETAS[j % 4]
        assert a.lbfgs_push_resto(Sp[:, j], Yp[:, j], eta) == kkt.LBFGS_STORED
        assert b.lbfgs_push_resto_device(dS[j].data_ptr(), dY[j].data_ptr(), eta) == kkt.LBFGS_STORED
        assert c.lbfgs_push_resto(Sp[:, j], Yp[:, j], eta) == kkt.LBFGS_STORED
        if j + 1 in (1, k, k + 3):
            sa = snapshot(a)
            assert same(sa, snapshot(b)), f"host and device push differ after {j + 1}"
            assert same(sa, snapshot(c)), f"two fresh handles differ after {j + 1}"
    assert np.array_equal(dS.cpu().numpy(), Sp.T) and np.array_equal(dY.cpu().numpy(), Yp.T)              # the caller's vectors are only read


@pytest.mark.parametrize("special", [False, True])
def test_an_sr1_undo_re_forms_bitwise_what_the_earlier_push_installed(special):
    rows, k = 517, 6
    Sp, Yp, DR = rs.make_resto(rows, k + 3, seed=3000 + rows + k, sr1=True)
    s, _ = resto_handle(rows, k, DR, rs.SR1, special)
    for j in range(k + 1):                                                                                 # (the last of these evicted a pair)
        assert s.lbfgs_push_resto(Sp[:, j], Yp[:, j], rs.ETAS[j % 4]) == kkt.LBFGS_STORED
    before = snapshot(s)
    assert before[4]["can_undo"]
    assert s.lbfgs_push_resto(Sp[:, k + 1], Yp[:, k + 1], 0.01) == kkt.LBFGS_STORED                        # another eta, another eviction
    assert s.lbfgs_resto_info()["eta"] == 0.01 and not same(before, snapshot(s), but_counter=True)
    assert s.lbfgs_undo() == 1
    after = snapshot(s)
    assert after[1]["skipped_in_a_row"] == 1 and not after[4]["can_undo"]
    assert same(before, after, but_counter=True)
    assert s.lbfgs_undo() == 0
    assert s.lbfgs_push_resto(Sp[:, k + 1], Yp[:, k + 1], 0.01) == kkt.LBFGS_STORED and s.lbfgs_info()["skipped_in_a_row"] == 0


@pytest.mark.parametrize("special", [False, True])
def test_a_skipped_push_changes_nothing_but_the_counter(special):
    """BFGS: a pair failing the curvature test, a NaN entry, and a push whose recomputed min D is not positive (the construction of
    tests/test_resto_spec.py: pair 0 has s^T ypart = -0.05 s^T s, stored at eta 0.3, D_0 < 0 at eta 0.03); SR1: a NaN entry"""
    rows, k = 517, 4
    Sp, Yp, DR = rs.make_resto(rows, 4, seed=12)
    s, _ = resto_handle(rows, k, DR, rs.BFGS, special)
    H = rs.History(rows, k, DR, special=special)
    assert s.lbfgs_push_resto(Sp[:, 0], -0.05 * Sp[:, 0], 0.3) == kkt.LBFGS_STORED and H.push(Sp[:, 0], -0.05 * Sp[:, 0], 0.3) == rs.STORED
    assert s.lbfgs_push_resto(Sp[:, 1], Yp[:, 1], 0.3) == kkt.LBFGS_STORED and H.push(Sp[:, 1], Yp[:, 1], 0.3) == rs.STORED
    before = snapshot(s)
    ynan = Yp[:, 2].copy(); ynan[300] = np.nan
    for n_skipped, (a, b, eta) in enumerate([(Sp[:, 2], -Yp[:, 2] - 2.0 * Sp[:, 2], 0.3), (Sp[:, 2], ynan, 0.3), (Sp[:, 2], Yp[:, 2], 0.03)], 1):
        assert s.lbfgs_push_resto(a, b, eta) == kkt.LBFGS_SKIPPED and H.push(a, b, eta) == rs.SKIPPED
        after = snapshot(s)
        assert after[1]["skipped_in_a_row"] == n_skipped
        assert same(before, after, but_counter=True)
    assert s.lbfgs_push_resto(Sp[:, 2], Yp[:, 2], 0.3) == kkt.LBFGS_STORED and s.lbfgs_info()["memory"] == 3 and s.lbfgs_info()["skipped_in_a_row"] == 0
    s.lbfgs_reset()
    assert s.lbfgs_info()["memory"] == 0 and s.lbfgs_info()["sigma"] == (-1.0 if special else 1.0) and s.lbfgs_resto_info()["eta"] == -1.0
    assert s.lowrank_info()["nv"] == 0
    t, _ = resto_handle(rows, k, DR, rs.SR1, special)
    assert t.lbfgs_push_resto(Sp[:, 0], Yp[:, 0], 0.3) == kkt.LBFGS_STORED
    before = snapshot(t)
    assert t.lbfgs_push_resto(Sp[:, 2], ynan, 0.3) == kkt.LBFGS_SKIPPED
    after = snapshot(t)
    assert after[1]["skipped_in_a_row"] == 1 and same(before, after, but_counter=True)


def test_plain_and_resto_pushes_do_not_mix():
    rows = 180
    Sp, Yp, DR = rs.make_resto(rows, 1, seed=1)
    s, _ = resto_handle(rows, 3, DR, rs.BFGS, False)
    with pytest.raises(ipopt_amd.KKTError, match="restoration-phase history"):
        s.lbfgs_push(Sp[:, 0], Yp[:, 0])
    assert s.lbfgs_info()["memory"] == 0
    s.lbfgs_define(rows, 3)
    with pytest.raises(ipopt_amd.KKTError, match="plain history"):
        s.lbfgs_push_resto(Sp[:, 0], Yp[:, 0], 0.3)
    with pytest.raises(ipopt_amd.KKTError, match="restoration-phase history"):
        s.lbfgs_get("G")
    assert s.lbfgs_resto_info() == dict(resto=False, special=False, eta=0.0)
    assert s.lbfgs_push(Sp[:, 0], Yp[:, 0]) == kkt.LBFGS_STORED


@pytest.mark.parametrize("k", [2, 12])
@pytest.mark.parametrize("type_,special", BOTH)
def test_whole_chain_push_factor_update_solve(type_, special, k):
    """system 517 of tests/test_gpu_lowrank.py; B0 on the x diagonal is sigma, or the vector eta DR.  On these pairs K + B0 + V V^T - U U^T keeps K's
    inertia (the specification's lowrank update answers 0 for all eight cases, SR1 with splits 2 + 0 and 8 + 4 / 7 + 5)"""
    rows = 517
    S = system(rows)
    n, K = S["n"], S["K"]
    Sp, Yp, DR = rs.make_resto(rows, k + 3, seed=300 + rows + k, sr1=type_ == rs.SR1)
    s, vals = resto_handle(rows, k, DR, type_, special)
    for j in range(k + 3):
        assert s.lbfgs_push_resto(Sp[:, j], Yp[:, j], rs.ETAS[j % 4]) == kkt.LBFGS_STORED
    diag = b0(s, DR)
    V, U = s.lbfgs_get("V"), s.lbfgs_get("U")
    assert V.shape[1] + (0 if type_ == rs.BFGS else U.shape[1]) == s.lbfgs_info()["memory"] == k
    factor(s, vals, diag, S["m"])
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    Ks = K.copy(); Ks[np.arange(rows), np.arange(rows)] += diag
    Kt = lr.dense_updated(Ks, V, U)
    b = Kt @ np.ones(n)
    x = b.copy(); s.lowrank_solve(x)
    xs = lr.solve(Ks, V, U, lr.update(Ks, V, U), b)
    res = sres(Kt, x, b)
    print(f"type {type_} special {int(special)} k {k}: nv {V.shape[1]} nu {U.shape[1]}, scaled residual {res:.2e}, |x - x_spec| {np.abs(x - xs).max():.2e}")
    assert res <= RES_TOL
    assert np.abs(x - xs).max() <= FIX_TOL * max(1.0, np.abs(xs).max())
