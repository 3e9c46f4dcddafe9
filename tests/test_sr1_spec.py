"""-m 'not gpu': the numpy statement of the limited-memory SR1 updater (tests/support/sr1_spec.py) against itself: the compact matrix
sigma I + V V^T - U U^T of the longdouble History equals the recursive SR1 matrix of the stored pairs, B <- B + r r^T / (r^T s), to 1e-14 relative to
the largest entry (measured: at most 4.6e-16 on these ten cases; the smallest |r^T s| / (|r| |s|) is 1.7e-3, so the recursion is well defined), and
the inputs of the GPU tests give a MIXED split for every k >= 2: 1 <= nneg <= m - 1, with emin / emax >= 5.2e-4, far from the 1e-12 skip rule.
The counts (from an independent numpy eigh) are properties of the inputs: k = 1, 2, 6, 12, 32 -> nneg 0, 1, 3, 6, 18 at rows 180; 0, 1, 3, 5, 17 at
517; 0, 1, 5, 4, 17 at 1728."""
import numpy as np
import pytest

from tests.support import sr1_spec as sr

KS = [1, 2, 6, 12, 32]
NNEG = {180: [0, 1, 3, 6, 18], 517: [0, 1, 3, 5, 17], 1728: [0, 1, 5, 4, 17]}


def history(rows, k, dtype):
    Sp, Yp = sr.make_pairs(rows, k + 3, seed=2000 + rows + k)
    H = sr.History(rows, k, init="scalar1", init_val=1.0, dtype=dtype)
    for j in range(k + 3):
        assert H.push(Sp[:, j], Yp[:, j]) == sr.STORED
    return H


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("rows", [180, 517])
def test_compact_matrix_is_the_recursive_sr1_matrix(rows, k):
    H = history(rows, k, np.longdouble)
    assert H.memory == k and H.V.shape == (rows, k - H.nneg) and H.U.shape == (rows, H.nneg)
    B, angle = sr.recursive_sr1(H.S, H.Y, H.sigma)
    e = float(np.abs(sr.dense(H.V, H.U, H.sigma) - B).max() / np.abs(B).max())
    print(f"rows {rows} k {k}: deviation {e:.2e}, smallest |r^T s| / (|r| |s|) {angle:.2e}, nneg {H.nneg}")
    assert e <= 1e-14
    assert angle >= 1e-3                                 # (1.7e-3 measured: no step of the recursion divides by a vanishing r^T s)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("rows", [180, 517, 1728])
def test_the_split_of_the_gpu_tests_inputs_is_mixed(rows, k):
    H = history(rows, k, np.float64)
    nneg, emin, emax = sr.split(H.E)
    print(f"rows {rows} k {k}: nneg {nneg} of {k}, emin / emax {emin / emax:.2e}")
    assert nneg == H.nneg == NNEG[rows][KS.index(k)]
    if k >= 2:
        assert 1 <= nneg <= k - 1
    assert emin / emax >= 5.2e-4
    assert np.all(np.diff(H.E) >= 0)                     # ascending


def test_undo_restores_the_state_and_is_one_level():
    rows, k = 180, 3
    Sp, Yp = sr.make_pairs(rows, 5, seed=11)
    H = sr.History(rows, k)
    assert H.undo() == 0
    for j in range(4):
        assert H.push(Sp[:, j], Yp[:, j]) == sr.STORED
    before = {f: np.array(getattr(H, f), copy=True) for f in H.FIELDS}
    assert H.push(Sp[:, 4], Yp[:, 4]) == sr.STORED
    assert H.undo() == 1 and H.undo() == 0
    for f in H.FIELDS:
        want = before[f] + 1 if f == "skipped_in_a_row" else before[f]
        assert np.array_equal(np.asarray(getattr(H, f)), want), f
    ynan = Yp[:, 4].copy(); ynan[3] = np.nan
    assert H.push(Sp[:, 4], ynan) == sr.SKIPPED and H.skipped_in_a_row == 2 and H.undo() == 0
