"""-m 'not gpu': the numpy statement of the limited-memory BFGS updater (tests/support/lbfgs_spec.py) against itself -- the compact form
sigma I + V V^T - U U^T against the recursive dense BFGS matrix, the incremental D / L / S^T S against a recomputation, the skip rule, the
five sigma modes and both clips.  Pairs: the tests' recipe (lbfgs_spec.make_pairs).  Bounds: the compact and the recursive form are two
backward-stable evaluations of one matrix whose small system has cond(M) <= 5 on these pairs: 1e-13 relative in float64 (observed: at most
2e-15), 1e-17 in longdouble (64-bit significand; observed below 1e-18)."""
import numpy as np
import pytest

from tests.support import lbfgs_spec as lb

LD_IS_WIDER = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble], ids=["float64", "longdouble"])
@pytest.mark.parametrize("k", [1, 2, 6, 32])
@pytest.mark.parametrize("rows", [180, 517])
def test_compact_form_is_the_recursive_bfgs_matrix(rows, k, dtype):
    S, Y = lb.make_pairs(rows, k + 3, seed=rows + k)
    H = lb.History(rows, k, dtype=dtype)
    for j in range(k + 3):
        assert H.push(S[:, j], Y[:, j]) == lb.STORED
        if j + 1 in (1, k, k + 3):
            assert H.memory == min(j + 1, k)
            B = lb.recursive_bfgs(H.S, H.Y, H.sigma)
            dev = np.abs(lb.dense(H.V, H.U, H.sigma) - B).max() / np.abs(B).max()
            terms = np.abs(lb.dense(*lb.recursive_terms(H.S, H.Y, H.sigma), H.sigma) - B).max() / np.abs(B).max()
            tol = 1e-17 if dtype is np.longdouble and LD_IS_WIDER else 1e-13
            assert dev <= tol and terms <= tol, (dev, terms)
            assert np.linalg.eigvalsh(B.astype(np.float64)).min() > 0.5


@pytest.mark.parametrize("k", [1, 2, 6, 32])
def test_incremental_small_matrices_equal_a_recomputation(k):
    rows = 300
    S, Y = lb.make_pairs(rows, k + 3, seed=k)
    H = lb.History(rows, k)
    for j in range(k + 3):
        H.push(S[:, j], Y[:, j])
    assert np.array_equal(H.S, S[:, 3:]) and np.array_equal(H.Y, Y[:, 3:])          # the last k pairs, oldest first
    D, L, T = lb.recomputed(S[:, 3:], Y[:, 3:])
    scale = np.abs(T).max()
    for inc, rec in ((H.D, D), (H.L, L), (H.STS, T)):
        assert inc.shape == rec.shape and np.abs(inc - rec).max() <= 1e-13 * scale
    assert np.all(np.triu(H.L) == 0.0)


def test_skip_rule():
    rows = 50
    rng = np.random.default_rng(0)
    s = rng.standard_normal(rows)
    H = lb.History(rows, 4)
    assert H.push(s, 2.0 * s) == lb.STORED
    before = (H.S.copy(), H.Y.copy(), H.D.copy(), H.sigma, H.V.copy(), H.U.copy())
    e = np.zeros(rows); e[0] = 1.0; f = np.zeros(rows); f[1] = 1.0
    tol = np.sqrt(np.finfo(np.float64).eps)
    ynan = s.copy(); ynan[3] = np.nan
    skipped = [(s, -s), (e, f), (e, 0.5 * tol * e + f), (s, ynan), (s, np.full(rows, np.inf)), (np.zeros(rows), s)]
    for k, (a, b) in enumerate(skipped):
        assert H.push(a, b) == lb.SKIPPED and H.skipped_in_a_row == k + 1
    after = (H.S, H.Y, H.D, H.sigma, H.V, H.U)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert H.push(e, 2.0 * tol * e + f) == lb.STORED and H.skipped_in_a_row == 0     # s^T y = 2 tol > tol |s| |y| = tol sqrt(1 + 4 tol^2)
    assert lb.skip(1.0, tol, 1.0) and not lb.skip(1.0, np.nextafter(tol, 1.0), 1.0)  # the boundary itself is a skip


def test_sigma_modes_and_clips():
    rows = 40
    rng = np.random.default_rng(1)
    s = rng.standard_normal(rows); y = 3.0 * s + 0.1 * rng.standard_normal(rows)
    ss, sy, yy = s @ s, s @ y, y @ y
    want = {"scalar1": sy / ss, "scalar2": yy / sy, "scalar3": (sy / ss + yy / sy) / 2, "scalar4": np.sqrt((sy / ss) * (yy / sy)), "constant": 7.5}
    for init in lb.INIT:
        H = lb.History(rows, 3, init=init, init_val=7.5)
        assert H.sigma == 7.5                                                        # before the first stored pair
        assert H.push(s, y) == lb.STORED
        assert abs(H.sigma - want[init]) <= 1e-15 * want[init]
        H.push(s, -y)
        assert abs(H.sigma - want[init]) <= 1e-15 * want[init]                       # a skip leaves it
        H.reset()
        assert H.sigma == 7.5 and H.memory == 0 and H.V is None
    assert want["scalar1"] < want["scalar4"] < want["scalar3"] < want["scalar2"]
    H = lb.History(rows, 3); H.push(s, 1e10 * s); assert H.sigma == 1e8              # the reference's default limits
    H = lb.History(rows, 3); H.push(s, 1e-10 * s); assert H.sigma == 1e-8
    H = lb.History(rows, 3, init="constant", init_val=50.0, sigma_max=20.0); H.push(s, y); assert H.sigma == 20.0
    H = lb.History(rows, 3, init="scalar2", sigma_min=4.0, sigma_max=5.0); H.push(s, y); assert H.sigma == 4.0


def test_cholesky_failure_keeps_the_pair_and_the_installed_columns():
    """init constant, init_val 1e8, s = e_1, y = 1e-9 e_1 twice: every dot is exact, M = [[1e8, 1e8], [1e8, 1e8]] in float64, the second pivot is 0"""
    rows = 8
    s = np.zeros(rows); s[0] = 1.0
    y = 1e-9 * s
    H = lb.History(rows, 4, init="constant", init_val=1e8)
    assert H.push(s, y) == lb.STORED
    V1, U1 = H.V.copy(), H.U.copy()
    assert H.push(s, y) == lb.NOT_POSDEF
    assert H.memory == 2 and H.sigma == 1e8 and np.array_equal(H.V, V1) and np.array_equal(H.U, U1)
    if LD_IS_WIDER:
        G = lb.History(rows, 4, init="constant", init_val=1e8, dtype=np.longdouble)
        assert G.push(s, y) == lb.STORED and G.push(s, y) == lb.STORED               # the failure is float64's rounding of M
