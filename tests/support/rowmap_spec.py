"""numpy statement of the low-rank-updated solve under a ROW MAP (include/mi355x_kkt.h, mi355x_kkt_lowrank_rowmap; the reference's P_LowRank,
IpLowRankAugSystemSolver.cpp:274-290, :449-457): K~ = K + P (V V^T - U U^T) P^T, row i of V and U being the caller's index idx[i] (strictly ascending).

No new algebra: with perm = idx followed by the remaining indices and Kp = K[perm][:, perm], the mapped update on K IS the update of
tests/support/lowrank_spec.py on Kp with the first `rows` indices, permuted back.  The columns come from lowrank_spec.scaled_columns on Kp: (Kp^-1)
restricted to the first `rows` indices is a principal submatrix of (K^-1)_xx, so the recipe's guarantee (lambda_min(M1) >= 1, lambda_min(M2) = 0.25)
carries over."""
from __future__ import annotations

import numpy as np

from tests.support import lowrank_spec as lr

# (n_x, mapped rows, (nv, nu)): what each covers is said in tests/test_gpu_lowrank_rowmap.py
CASES = [(180, 1, (1, 1)), (180, 179, (5, 7)), (517, 300, (17, 32)), (1728, 1100, (32, 32)), (1728, 1100, (0, 1)), (1728, 1100, (1, 0))]


def make_idx(nx, rows, seed=3):
    """the tests' maps: index 0, index nx - 1 and rows - 2 more drawn with default_rng(seed); a single row is index nx // 2.  int32, strictly ascending"""
    if rows == 1:
        return np.array([nx // 2], dtype=np.int32)
    rng = np.random.default_rng(seed)
    mid = rng.choice(np.arange(1, nx - 1), size=rows - 2, replace=False)
    idx = np.sort(np.concatenate([[0, nx - 1], mid])).astype(np.int32)
    assert idx.size == rows and np.all(np.diff(idx) > 0)
    return idx


def perm_of(idx, n):
    """idx, then the remaining indices ascending"""
    rest = np.setdiff1d(np.arange(n), idx)
    return np.concatenate([np.asarray(idx, dtype=np.int64), rest])


def expand(A, idx, n):
    """P A: the n-row form of the columns of A"""
    out = np.zeros((n,) + A.shape[1:], dtype=A.dtype)
    out[np.asarray(idx)] = A
    return out


def dense_updated(K, idx, V, U):
    """the dense K~ = K + P (V V^T - U U^T) P^T"""
    Kt = np.array(K, dtype=np.float64, copy=True)
    Kt[np.ix_(idx, idx)] += V @ V.T - U @ U.T
    return Kt


class Mapped:
    """the permuted system of a map: Kp, one LU of it, the columns of the recipe and the specification's update"""

    def __init__(self, K, idx, nv, nu, seed=11):
        self.n, self.idx, self.rows = K.shape[0], np.asarray(idx), len(idx)
        self.perm = perm_of(idx, self.n)
        self.Kp = K[np.ix_(self.perm, self.perm)]
        self.ksolve = lr.dense_solver(self.Kp)
        self.V, self.U = lr.scaled_columns(self.Kp, self.rows, nv, nu, seed=seed, solve=self.ksolve)
        self.upd = lr.update(self.Kp, self.V, self.U, self.ksolve)
        self.Kt = dense_updated(K, self.idx, self.V, self.U)

    def solve(self, b):
        """b: (n,) or (n, nrhs) in the caller's numbering -> the specification's solution of K~ x = b, same numbering"""
        x = np.empty_like(b, dtype=np.float64)
        x[self.perm] = lr.solve(self.Kp, self.V, self.U, self.upd, b[self.perm], self.ksolve)
        return x
