"""-m 'not gpu': the two numpy statements of the restoration-phase limited-memory update (tests/support/resto_spec.py) against each other: `History`,
which keeps what the library keeps (Gram matrices by augment / shift, eta and the scale of V per stored pair), in float64, against `Literal`, the
transcription of the reference's flow that keeps full vectors and recomputes Y, D, L and the Gram matrices at every push, in longdouble.

Rule (the project's): e <= 64 max(e_64, 2^-52), e = max|A - A_ld| / max|A_ld| of History in float64 against Literal in longdouble and e_64 that of
Literal in float64: both float64 runs round the same quantities, in different orders over 180 rows.  Compared after pushes 1, k and k + 3: D, L,
sigma, V V^T, U U^T and B0 + V V^T - U U^T (never column by column for SR1: sign and rotation of eigenvectors are not determined).
Inputs: resto_spec.make_resto, seed 3000 + rows + k; eta cycles through 0.3, 0.3, 0.1, 0.03, so it changes between stored pairs and across an eviction."""
import numpy as np
import pytest

from tests.support import resto_spec as rs

ROWS = 180
KS = [1, 2, 6, 12, 32]


def dev(A, Ald):
    return float(np.abs(A - Ald).max() / np.abs(Ald).max())


def views(H):
    """the compared arrays of a state with installed columns"""
    return {"D": H.D, "L": H.L, "sigma": np.atleast_1d(H.sigma), "V V^T": H.V @ H.V.T, "U U^T": H.U @ H.U.T, "B0 + V V^T - U U^T": rs.dense(H)}


def three(k, type_, special):
    S, Yp, DR = rs.make_resto(ROWS, k + 3, seed=3000 + ROWS + k, sr1=type_ == rs.SR1)
    mk = lambda cls, dt: cls(ROWS, k, DR, type=type_, special=special, dtype=dt)
    return S, Yp, DR, mk(rs.History, np.float64), mk(rs.Literal, np.float64), mk(rs.Literal, np.longdouble)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("special", [False, True])
@pytest.mark.parametrize("type_", [rs.BFGS, rs.SR1])
def test_history_against_the_literal_transcription(type_, special, k):
    S, Yp, DR, H, L64, Lld = three(k, type_, special)
    mixed, worst = False, 0.0
    for j in range(k + 3):
        eta = rs.ETAS[j % 4]
        got = [X.push(S[:, j], Yp[:, j], eta) for X in (H, L64, Lld)]
        assert got == [rs.STORED] * 3, (j, got)
        m = min(j + 1, k)
        assert H.memory == L64.memory == Lld.memory == m and H.skipped_in_a_row == 0
        if type_ == rs.SR1:
            assert H.nneg == L64.nneg == Lld.nneg
            assert Lld.last_ratio >= 1e-6, f"push {j + 1}: emin / emax = {Lld.last_ratio:.2e} is within 1e6 of the split rule's 1e-12: change the seed"
            mixed = mixed or 0 < Lld.nneg < m
        if j + 1 not in (1, k, k + 3):
            continue
        assert np.array_equal(H.S, Lld.S.astype(np.float64)) and np.array_equal(H.Ypart, Lld.Ypart.astype(np.float64))
        a, a64, ald = views(H), views(L64), views(Lld)
        for name in a:
            assert a[name].shape == ald[name].shape, name
            if not np.abs(ald[name]).max() > 0:                       # L of a single pair; an empty half of the SR1 split
                assert (name == "L" and m == 1) or (type_ == rs.SR1 and ((name == "U U^T" and Lld.nneg == 0) or (name == "V V^T" and Lld.nneg == m))), name
                assert not a[name].any()
                continue
            e, e_64 = dev(a[name], ald[name]), dev(a64[name], ald[name])
            ratio = e / max(e_64, 2.0 ** -52)
            worst = max(worst, ratio)
            print(f"type {type_} special {int(special)} k {k} after {j + 1}: {name}: e {e:.2e} e_64 {e_64:.2e} ratio {ratio:.2f}")
            assert e <= 64.0 * max(e_64, 2.0 ** -52), (name, e, e_64)
        if type_ == rs.BFGS:
            lam = float(np.linalg.eigvalsh(rs.dense(Lld).astype(np.float64)).min())
            print(f"  smallest eigenvalue of B0 + V V^T - U U^T: {lam:.3e}")
            assert lam > 0
    if type_ == rs.SR1 and k >= 6:
        assert mixed, "no push of this case had a mixed split: change the seed"
    print(f"type {type_} special {int(special)} k {k}: largest e / max(e_64, 2^-52) = {worst:.2f}")


@pytest.mark.parametrize("type_", [rs.BFGS, rs.SR1])
def test_the_stored_y_has_no_dr(type_):
    """quirk: D and L are those of Y = Ypart + eta S, not of Ypart + eta DR o S, although DR is far from 1 (in [0.25, 1])"""
    k = 6
    S, Yp, DR, H, _, Lld = three(k, type_, False)
    for j in range(k + 2):
        eta = rs.ETAS[j % 4]
        assert H.push(S[:, j], Yp[:, j], eta) == rs.STORED and Lld.push(S[:, j], Yp[:, j], eta) == rs.STORED
    Sk, Yk = S[:, 2:k + 2].astype(np.longdouble), Yp[:, 2:k + 2].astype(np.longdouble)
    eta = np.longdouble(rs.ETAS[(k + 1) % 4])
    plain = Sk.T @ (Yk + eta * Sk)
    weighted = Sk.T @ (Yk + eta * DR.astype(np.longdouble)[:, None] * Sk)
    for X in (H, Lld):
        stored = np.diag(X.D) + X.L
        assert dev(stored, np.tril(plain)) <= 64.0 * 2.0 ** -52
        assert dev(stored, np.tril(weighted)) >= 1e-3


def test_older_columns_of_v_stay_what_they_were_when_eta_changes():
    """quirk (BFGS): a push appends one column to V; the others keep the eta and the scale of their own push"""
    k = 6
    S, Yp, DR, H, _, Lld = three(k, rs.BFGS, False)
    for j in range(k + 3):
        eta = rs.ETAS[j % 4]
        V0 = {id(X): X.V for X in (H, Lld)}
        assert H.push(S[:, j], Yp[:, j], eta) == rs.STORED and Lld.push(S[:, j], Yp[:, j], eta) == rs.STORED
        if j == 0:
            continue
        lo = 1 if j >= k else 0
        for X in (H, Lld):
            assert np.array_equal(X.V[:, :-1], V0[id(X)][:, lo:]), j
        y_new = Yp[:, j] + eta * DR * S[:, j]
        assert dev(H.V[:, -1], y_new / np.sqrt(S[:, j] @ y_new)) <= 64.0 * 2.0 ** -52
    assert len(set(H.eta_col.tolist())) == 3                         # the live columns were pushed at three different eta


def same_but_counter(a, b, fields):
    for f in fields:
        if f == "skipped_in_a_row":
            continue
        x, y = a[f], b[f]
        if x is None or y is None:
            assert x is None and y is None, f
        else:
            assert np.array_equal(np.asarray(x), np.asarray(y)), f


@pytest.mark.parametrize("special", [False, True])
@pytest.mark.parametrize("cls", [rs.History, rs.Literal])
def test_a_pair_that_fails_the_curvature_test_moves_only_the_counter(cls, special):
    S, Yp, DR = rs.make_resto(ROWS, 4, seed=11)
    H = cls(ROWS, 3, DR, special=special)
    for j in range(3):
        assert H.push(S[:, j], Yp[:, j], 0.3) == rs.STORED
    before = H.snapshot()
    assert H.push(S[:, 3], -Yp[:, 3] - 2.0 * S[:, 3], 0.3) == rs.SKIPPED      # s^T y_new < 0
    same_but_counter(before, H.snapshot(), cls.FIELDS)
    assert H.skipped_in_a_row == 1
    assert H.push(S[:, 3], Yp[:, 3], 0.3) == rs.STORED and H.skipped_in_a_row == 0


@pytest.mark.parametrize("special", [False, True])
@pytest.mark.parametrize("cls", [rs.History, rs.Literal])
def test_a_push_whose_recomputed_d_is_not_positive_moves_only_the_counter(cls, special):
    """pair 0 has s^T ypart = -0.05 s^T s: at eta 0.3 its D = 0.25 s^T s and s^T y_new = s^T ypart + 0.3 s^T (DR o s) > 0 (the mean of DR is 0.54), so it is
    stored; a good pair pushed at eta 0.03 recomputes D_0 = -0.02 s^T s: that push is skipped and nothing but the counter changes"""
    S, Yp, DR = rs.make_resto(ROWS, 3, seed=12)
    H = cls(ROWS, 4, DR, special=special)
    assert H.push(S[:, 0], -0.05 * S[:, 0], 0.3) == rs.STORED
    assert H.push(S[:, 1], Yp[:, 1], 0.3) == rs.STORED and np.all(H.D > 0)
    before = H.snapshot()
    assert H.push(S[:, 2], Yp[:, 2], 0.03) == rs.SKIPPED
    same_but_counter(before, H.snapshot(), cls.FIELDS)
    assert H.skipped_in_a_row == 1 and H.memory == 2 and float(H.eta) == 0.3
    assert H.push(S[:, 2], Yp[:, 2], 0.3) == rs.STORED and H.memory == 3 and H.skipped_in_a_row == 0


def test_an_sr1_undo_brings_eta_and_the_gram_matrices_back():
    k = 3
    S, Yp, DR, H, _, _ = three(k, rs.SR1, True)
    for j in range(k + 1):
        assert H.push(S[:, j], Yp[:, j], rs.ETAS[j % 4]) == rs.STORED
    before = H.snapshot()
    assert H.push(S[:, k + 1], Yp[:, k + 1], 0.01) == rs.STORED and float(H.eta) == 0.01
    assert H.undo() == 1 and H.undo() == 0
    same_but_counter(before, H.snapshot(), rs.History.FIELDS)
    assert H.skipped_in_a_row == before["skipped_in_a_row"] + 1
