"""-m gpu: the limited-memory SR1 history of the C ABI (mi355x_kkt_lbfgs_define_sr1, _lbfgs_undo, _lbfgs_sr1_info behind the lbfgs_* calls; reference
IpLimMemQuasiNewtonUpdater.cpp case SR1) against its numpy statement (tests/support/sr1_spec.py) in longdouble, through undo, and through the whole
chain push -> factor K + sigma I_x -> lowrank_update -> lowrank_solve.  Sizes as in tests/test_gpu_lbfgs.py: `rows` 180 (below one 256-row block of
k_lb_form_sr1), 517 (no multiple of 64 / 256), 1728 (two 1024-row slabs of k_lb_dots); max_history 1, 2, 6 (loops unrolled to 8), 12 (to 16), 32 (to
32, the maximum).  Pairs: make_pairs(rows, k + 3, seed=2000 + rows + k): every split with k >= 2 is mixed and emin / emax >= 5.2e-4
(tests/test_sr1_spec.py), so no push is near the skip rule.

Bound of the comparisons with the specification: e_dev <= 64 max(e_64, 2^-52), e = max|A - A_ld| / max|A_ld|, e_64 the float64 specification's own
deviation from the longdouble one on the same inputs (the margin of tests/test_gpu_lbfgs.py: a different but fixed summation order over at most 1728
rows; the amplification by emax / emin is in e_64 already: e_64 of sigma I + V V^T - U U^T is between 3e-16 and 3.4e-12 on these cases).
Solves: RES_TOL = 1e-12 and FIX_TOL = 1e-7, the project's tolerances (tests/test_gpu_lowrank.py)."""
import functools

import numpy as np
import pytest
import torch      # (before the library is loaded: see tests/test_gpu_parity.py)

import ipopt_amd
from ipopt_amd import kkt
from tests.support import lowrank_spec as lr
from tests.support import sr1_spec as sr
from tests.test_gpu_lbfgs import handle, factor, snapshot, same, dev
from tests.test_gpu_lowrank import SYSTEMS, system, sres, RES_TOL, FIX_TOL

pytestmark = pytest.mark.gpu
ROWS = [180, 517, 1728]
KS = [1, 2, 6, 12, 32]


def sr1_handle(rows, k, **define):
    s, vals = handle(rows)
    s.lbfgs_define_sr1(rows, max_history=k, **define)
    return s, vals


def snap(s):
    """snapshot of tests/test_gpu_lbfgs.py plus what only the SR1 calls show"""
    I = s.lbfgs_sr1_info()
    return snapshot(s) + ((I["type"], I["nneg"], I["can_undo"], I["E"].tobytes()),)


def same_sr1(a, b, counter_offset=0, ignore_can_undo=False):
    """bitwise; b's skipped_in_a_row must be a's plus counter_offset"""
    ia = dict(a[1], skipped_in_a_row=a[1]["skipped_in_a_row"] + counter_offset)
    xa, xb = (a[3], b[3]) if not ignore_can_undo else (a[3][:2] + a[3][3:], b[3][:2] + b[3][3:])
    return same((a[0], ia, a[2]), b[:3]) and xa == xb


def pairs(rows, k):
    return sr.make_pairs(rows, k + 3, seed=2000 + rows + k)


@functools.lru_cache(maxsize=None)
def specification(rows, k):
    """the float64 and the longdouble History after pushes 1, k and k + 3 of pairs(rows, k): computed once, shared, never written"""
    Sp, Yp = pairs(rows, k)
    H64, Hld = sr.History(rows, k), sr.History(rows, k, dtype=np.longdouble)
    out = {}
    for j in range(k + 3):
        assert H64.push(Sp[:, j], Yp[:, j]) == sr.STORED and Hld.push(Sp[:, j], Yp[:, j]) == sr.STORED
        if j + 1 in (1, k, k + 3):
            out[j + 1] = tuple({f: getattr(H, f) for f in ("D", "L", "STS", "sigma", "V", "U", "nneg", "E")} for H in (H64, Hld))
    return out


def compare(tag, got, info, A64, Ald):
    """the rule of the module docstring on D, L, S^T S, sigma, V V^T, U U^T and sigma I + V V^T - U U^T; -> the largest e_dev / max(e_64, 2^-52)"""
    m = info["memory"]
    P = lambda A: A @ A.T
    cmp = [(w, got[w], np.atleast_1d(A64[w]), np.atleast_1d(Ald[w])) for w in ("D", "L", "STS")]
    cmp.append(("sigma", np.array([info["sigma"]]), np.atleast_1d(A64["sigma"]), np.atleast_1d(Ald["sigma"])))
    Pv, Pu = P(Ald["V"]), P(Ald["U"])
    cmp.append(("V V^T", P(got["V"]), P(A64["V"]), Pv))
    cmp.append(("U U^T", P(got["U"]), P(A64["U"]), Pu))
    Bld = Pv - Pu; Bld[np.diag_indices(Bld.shape[0])] += Ald["sigma"]
    cmp.append(("sigma I + V V^T - U U^T", sr.dense(got["V"], got["U"], info["sigma"]), sr.dense(A64["V"], A64["U"], A64["sigma"]), Bld))
    worst = 0.0
    for name, A, B64, Bl in cmp:
        assert A.shape == Bl.shape, name
        if not np.abs(Bl).max() > 0:                                                                       # (L of a single pair; an empty half of the split)
            assert (name == "L" and m == 1) or (name == "V V^T" and Ald["nneg"] == m) or (name == "U U^T" and Ald["nneg"] == 0), name
            assert not A.any()
            continue
        e_dev, e_64 = dev(A, Bl), dev(B64, Bl)
        ratio = e_dev / max(e_64, 2.0 ** -52)
        worst = max(worst, ratio)
        print(f"{tag}: {name}: e_dev {e_dev:.2e} e_64 {e_64:.2e} ratio {ratio:.2f}")
        assert e_dev <= 64.0 * max(e_64, 2.0 ** -52), (name, e_dev, e_64)
    return worst


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("rows", ROWS)
def test_columns_against_the_longdouble_specification(rows, k):
    Sp, Yp = pairs(rows, k)
    spec = specification(rows, k)
    s, _ = sr1_handle(rows, k)
    assert s.lbfgs_info() == dict(rows=rows, max_history=k, memory=0, sigma=1.0, skipped_in_a_row=0, push_ms=0.0)
    I = s.lbfgs_sr1_info()
    assert (I["type"], I["nneg"], I["can_undo"], I["E"].shape) == (kkt.LBFGS_SR1, 0, False, (0,))
    worst = 0.0
    for j in range(k + 3):
        assert s.lbfgs_push(Sp[:, j], Yp[:, j]) == kkt.LBFGS_STORED
        if j + 1 not in spec:
            continue
        m = min(j + 1, k)
        A64, Ald = spec[j + 1]
        got, info, lri = snapshot(s)
        I = s.lbfgs_sr1_info()
        nneg = I["nneg"]
        assert info["memory"] == m and info["skipped_in_a_row"] == 0 and I["can_undo"] and I["type"] == kkt.LBFGS_SR1
        assert nneg == A64["nneg"] == Ald["nneg"] and (m < 2 or 1 <= nneg <= m - 1)
        assert lri == dict(rows=rows, nv=m - nneg, nu=nneg, current=False, update_ms=0.0)
        assert I["E"].shape == (m,) and np.all(np.diff(I["E"]) >= 0) and int(np.sum(I["E"] < 0)) == nneg
        lo = j + 1 - m
        assert np.array_equal(got["S"], Sp[:, lo:j + 1]) and np.array_equal(got["Y"], Yp[:, lo:j + 1])      # bitwise, oldest first, through the k + 1 slot ring
        assert got["V"].shape == (rows, m - nneg) and got["U"].shape == (rows, nneg)
        worst = max(worst, compare(f"rows {rows} k {k} after {j + 1}", got, info, A64, Ald))
        assert np.all(np.triu(got["L"]) == 0.0)
    print(f"rows {rows} k {k}: largest e_dev / max(e_64, 2^-52) = {worst:.2f}")


def test_negative_curvature_is_stored_not_skipped():
    rows, k = 517, 6
    Sp, Yp = pairs(rows, k)
    s, _ = sr1_handle(rows, k)
    b, _ = handle(rows, max_history=k)
    H64, Hld = sr.History(rows, k), sr.History(rows, k, dtype=np.longdouble)
    for j in range(3):
        assert b.lbfgs_push(Sp[:, j], -Yp[:, j]) == kkt.LBFGS_SKIPPED                                      # the very pairs a BFGS history skips
        assert s.lbfgs_push(Sp[:, j], -Yp[:, j]) == kkt.LBFGS_STORED
        assert H64.push(Sp[:, j], -Yp[:, j]) == sr.STORED and Hld.push(Sp[:, j], -Yp[:, j]) == sr.STORED
    got, info, lri = snapshot(s)
    I = s.lbfgs_sr1_info()
    assert lri == dict(rows=rows, nv=0, nu=3, current=False, update_ms=0.0)
    assert I["nneg"] == 3 and np.all(I["E"] < 0) and info["sigma"] > 0 and info["memory"] == 3
    f = ("D", "L", "STS", "sigma", "V", "U", "nneg", "E")
    compare("negative curvature", got, info, {w: getattr(H64, w) for w in f}, {w: getattr(Hld, w) for w in f})


def test_a_skipped_push_changes_nothing():
    rows, k = 517, 6
    S = system(rows)
    Sp, Yp = sr.make_pairs(rows, 4, seed=5)
    s, vals = sr1_handle(rows, k, init="constant", init_val=1.0)
    for j in range(3):
        assert s.lbfgs_push(Sp[:, j], Yp[:, j]) == kkt.LBFGS_STORED
    factor(s, vals, s.lbfgs_info()["sigma"], S["m"])
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    before = snap(s)
    assert before[2]["current"] and before[3][2]
    ynan = Yp[:, 3].copy(); ynan[300] = np.nan
    for n_skipped, (a, b) in enumerate([(Sp[:, 2], Yp[:, 2]), (Sp[:, 3], ynan)], 1):                       # the newest pair again: Z is singular
        assert s.lbfgs_push(a, b) == kkt.LBFGS_SKIPPED
        after = snap(s)
        assert after[1]["skipped_in_a_row"] == n_skipped
        assert same_sr1(before, after, counter_offset=n_skipped, ignore_can_undo=True) and after[2]["current"]
        assert not after[3][2]                                                                             # a skipped push leaves nothing to undo
    assert s.lbfgs_undo() == 0
    assert same_sr1(before, snap(s), counter_offset=2, ignore_can_undo=True) and s.lowrank_info()["current"]
    assert s.lbfgs_push(Sp[:, 3], Yp[:, 3]) == kkt.LBFGS_STORED
    assert s.lbfgs_info()["skipped_in_a_row"] == 0 and s.lbfgs_info()["memory"] == 4 and not s.lowrank_info()["current"]


def test_undo_restores_the_state_bitwise():
    rows, k = 1728, 6
    Sp, Yp = pairs(rows, k)
    s, _ = sr1_handle(rows, k)
    f, _ = sr1_handle(rows, k)
    for j in range(7):
        assert s.lbfgs_push(Sp[:, j], Yp[:, j]) == kkt.LBFGS_STORED
    A = snap(s)
    assert np.array_equal(A[0]["S"][:, 0], Sp[:, 1])
    assert s.lbfgs_push(Sp[:, 7], Yp[:, 7]) == kkt.LBFGS_STORED
    B = snap(s)
    assert not same_sr1(A, B, ignore_can_undo=True) and np.array_equal(B[0]["S"][:, 0], Sp[:, 2])
    assert s.lbfgs_undo() == 1
    back = snap(s)
    assert same_sr1(A, back, counter_offset=1, ignore_can_undo=True)                                       # the evicted pair is column 0 again; V, U, nv, nu
    assert np.array_equal(back[0]["S"][:, 0], Sp[:, 1]) and np.array_equal(back[0]["Y"][:, 0], Yp[:, 1])
    assert back[1]["skipped_in_a_row"] == 1 and not back[3][2] and not back[2]["current"]
    assert s.lbfgs_undo() == 0 and same_sr1(back, snap(s))                                                 # one level
    assert s.lbfgs_push(Sp[:, 7], Yp[:, 7]) == kkt.LBFGS_STORED
    for j in range(8):
        assert f.lbfgs_push(Sp[:, j], Yp[:, j]) == kkt.LBFGS_STORED
    assert same_sr1(B, snap(s)) and same_sr1(snap(f), snap(s))
    # a history that is not full yet: the memory goes back by one, nothing was evicted
    rows, k = 180, 6
    Sp, Yp = pairs(rows, k)
    s, _ = sr1_handle(rows, k)
    for j in range(2):
        assert s.lbfgs_push(Sp[:, j], Yp[:, j]) == kkt.LBFGS_STORED
    A = snap(s)
    assert s.lbfgs_push(Sp[:, 2], Yp[:, 2]) == kkt.LBFGS_STORED and s.lbfgs_info()["memory"] == 3
    assert s.lbfgs_undo() == 1 and same_sr1(A, snap(s), counter_offset=1, ignore_can_undo=True)
    # the first push of a history: memory 0 comes back, sigma is init_val, no update is installed
    rows, k = 180, 1
    Sp, Yp = pairs(rows, k)
    s, _ = sr1_handle(rows, k, init_val=2.5)
    assert s.lbfgs_push(Sp[:, 0], Yp[:, 0]) == kkt.LBFGS_STORED and s.lowrank_info()["nv"] + s.lowrank_info()["nu"] == 1
    assert s.lbfgs_undo() == 1
    assert s.lbfgs_info() == dict(rows=rows, max_history=1, memory=0, sigma=2.5, skipped_in_a_row=1, push_ms=s.lbfgs_info()["push_ms"])
    assert s.lowrank_info() == dict(rows=0, nv=0, nu=0, current=False, update_ms=0.0)
    assert s.lbfgs_get("S").shape == (rows, 0) and s.lbfgs_sr1_info()["E"].shape == (0,)
    assert s.lbfgs_undo() == 0
    b, _ = handle(rows, max_history=3)
    with pytest.raises(ipopt_amd.KKTError, match="SR1"):
        b.lbfgs_undo()
    s.lbfgs_reset()
    assert s.lbfgs_push(Sp[:, 0], Yp[:, 0]) == kkt.LBFGS_STORED
    s.lbfgs_reset()
    assert s.lbfgs_undo() == 0 and s.lbfgs_info()["skipped_in_a_row"] == 0                                 # reset leaves nothing to undo


@pytest.mark.parametrize("rows,k", [(517, 32), (1728, 6), (180, 12)])
def test_host_and_device_pushes_and_fresh_handles_give_the_same_bits(rows, k):
    Sp, Yp = pairs(rows, k)
    dS = torch.tensor(Sp.T.copy(), dtype=torch.float64, device="cuda"); dY = torch.tensor(Yp.T.copy(), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    a, _ = sr1_handle(rows, k); b, _ = sr1_handle(rows, k); c, _ = sr1_handle(rows, k)
    for j in range(k + 3):
        assert a.lbfgs_push(Sp[:, j], Yp[:, j]) == kkt.LBFGS_STORED
        assert b.lbfgs_push_device(dS[j].data_ptr(), dY[j].data_ptr()) == kkt.LBFGS_STORED
        assert c.lbfgs_push(Sp[:, j], Yp[:, j]) == kkt.LBFGS_STORED
        if j + 1 in (1, k, k + 3):
            sa = snap(a)
            assert same_sr1(sa, snap(b)), f"host and device push differ after {j + 1}"
            assert same_sr1(sa, snap(c)), f"two fresh handles differ after {j + 1}"
    assert np.array_equal(dS.cpu().numpy(), Sp.T) and np.array_equal(dY.cpu().numpy(), Yp.T)              # the caller's vectors are only read


CHAIN_SPLIT = {180: (3, 3), 300: (2, 4), 517: (3, 3), 1728: (4, 2)}      # (nv, nu) by the numpy specification; both inner matrices are positive definite


@pytest.mark.parametrize("rows", sorted(SYSTEMS))
def test_whole_chain_push_factor_update_solve(rows):
    """the SR1 matrices are indefinite (lambda_min between -4.6 and -25.7) and K~ keeps K's inertia: lambda_min(M2) = 0.51, 0.97, 0.98, 0.50"""
    S = system(rows)
    n, K = S["n"], S["K"]
    Sp, Yp = sr.make_pairs(rows, 9, seed=300 + rows)
    s, vals = sr1_handle(rows, 6)
    for j in range(9):
        assert s.lbfgs_push(Sp[:, j], Yp[:, j]) == kkt.LBFGS_STORED
    sigma = s.lbfgs_info()["sigma"]
    V, U = s.lbfgs_get("V"), s.lbfgs_get("U")
    assert (V.shape, U.shape) == ((rows, CHAIN_SPLIT[rows][0]), (rows, CHAIN_SPLIT[rows][1]))
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


def test_the_history_survives_a_structure_edit():
    rows, k = 1728, 6
    S = system(rows)
    Sp, Yp = sr.make_pairs(rows, k + 2, seed=21)
    s, vals = sr1_handle(rows, k)
    for j in range(k + 1):                                                                                 # (the ring has wrapped once)
        assert s.lbfgs_push(Sp[:, j], Yp[:, j]) == kkt.LBFGS_STORED
    factor(s, vals, s.lbfgs_info()["sigma"], S["m"])
    before = snap(s)
    cols = np.random.default_rng(3).choice(S["n"], size=12, replace=False) + 1
    assert s.delay_columns(cols) >= 1
    assert same_sr1(before, snap(s))
    assert np.array_equal(s.lbfgs_get("S"), Sp[:, 1:k + 1])
    assert s.lbfgs_push(Sp[:, k + 1], Yp[:, k + 1]) == kkt.LBFGS_STORED                                    # one more push on the edited structure
    pushed = snap(s)
    assert np.array_equal(s.lbfgs_get("S"), Sp[:, 2:]) and np.array_equal(s.lbfgs_get("Y"), Yp[:, 2:])
    H64, Hld = sr.History(rows, k), sr.History(rows, k, dtype=np.longdouble)
    for j in range(k + 2):
        H64.push(Sp[:, j], Yp[:, j]); Hld.push(Sp[:, j], Yp[:, j])
    f = ("D", "L", "STS", "sigma", "V", "U", "nneg", "E")
    compare("after the edit", pushed[0], pushed[1], {w: getattr(H64, w) for w in f}, {w: getattr(Hld, w) for w in f})
    sigma = s.lbfgs_info()["sigma"]
    factor(s, vals, sigma, S["m"])                                                                         # and the chain closes on the edited structure
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    V, U = s.lbfgs_get("V"), s.lbfgs_get("U")
    Ks = S["K"].copy(); Ks[np.arange(rows), np.arange(rows)] += sigma
    Kt = lr.dense_updated(Ks, V, U)
    b = Kt @ np.ones(S["n"]); x = b.copy(); s.lowrank_solve(x)
    assert sres(Kt, x, b) <= RES_TOL
    assert s.lbfgs_undo() == 1                                                                             # and an undo
    assert same_sr1(before, snap(s), counter_offset=1, ignore_can_undo=True) and not s.lowrank_info()["current"]
    assert s.lbfgs_push(Sp[:, k + 1], Yp[:, k + 1]) == kkt.LBFGS_STORED
    assert same_sr1(pushed, snap(s))


def test_a_bfgs_history_is_untouched():
    """define_sr1 -> pushes -> clear -> define: bitwise the handle that never saw SR1 (the ring of k slots, the clips, the curvature test)"""
    rows, k = 517, 6
    Sp, Yp = pairs(rows, k)
    a, _ = sr1_handle(rows, k)
    for j in range(k + 2):
        assert a.lbfgs_push(Sp[:, j], Yp[:, j]) == kkt.LBFGS_STORED
    a.lbfgs_clear()
    assert a.lbfgs_sr1_info()["type"] == kkt.LBFGS_BFGS
    a.lbfgs_define(rows, max_history=k)
    b, _ = handle(rows, max_history=k)
    for j in range(k + 3):
        oa, ob = a.lbfgs_push(Sp[:, j], Yp[:, j]), b.lbfgs_push(Sp[:, j], Yp[:, j])
        assert oa == ob == kkt.LBFGS_STORED
        assert same_sr1(snap(a), snap(b)), j
    assert a.lbfgs_push(Sp[:, 0], -Yp[:, 0]) == kkt.LBFGS_SKIPPED                                          # the curvature test is BFGS's again
    I = a.lbfgs_sr1_info()
    assert (I["type"], I["nneg"], I["can_undo"], I["E"].shape) == (kkt.LBFGS_BFGS, 0, False, (0,))
    assert a.lowrank_info()["nv"] == a.lowrank_info()["nu"] == k
