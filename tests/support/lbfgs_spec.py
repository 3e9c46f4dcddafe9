"""numpy statement of the limited-memory BFGS updater of include/mi355x_kkt.h (mi355x_kkt_lbfgs_*; reference IpLimMemQuasiNewtonUpdater.cpp, BFGS
"with skipping"), in the arithmetic `dtype` (float64: what the library computes in; longdouble: what it is held to).

  skip     s^T y <= sqrt(eps_double) |s|_2 |y|_2, or a non-finite s^T s, s^T y, y^T y                                   (CheckSkippingBFGS :985-1019)
  store    append the pair / drop the oldest when full; D = diag(s_i^T y_i), L_ij = s_i^T y_j (i > j), S^T S by "augment" or "shift": only the
           new row and column are computed                                                                             (UpdateInternalData :769-818)
  sigma    scalar1 s^T y / s^T s, scalar2 y^T y / s^T y, scalar3 / scalar4 their arithmetic / geometric mean, constant init_val; from the new
           pair; clipped to [sigma_min, sigma_max]; init_val before the first stored pair                              (:405-432)
  columns  V = Y D^(-1/2), Lt = L D^(-1/2), M = Lt Lt^T + sigma S^T S, J = chol(M), C = J^(-T), Lbar = Lt^T C, U = sigma S C + V Lbar   (:440-520)
           M not positive definite: the pair and sigma stay, V and U stay what they were                               (:484-495)

`recursive_bfgs` is the independent check: the dense BFGS matrix of the stored pairs started from sigma I, one rank-two update per pair.
"""
from __future__ import annotations

import numpy as np

STORED, SKIPPED, NOT_POSDEF = 0, 1, 2
INIT = ("scalar1", "scalar2", "scalar3", "scalar4", "constant")
SQRT_EPS = np.sqrt(np.finfo(np.float64).eps)


def skip(ss, sy, yy):
    if not (np.isfinite(ss) and np.isfinite(sy) and np.isfinite(yy)):
        return True
    return bool(sy <= type(ss)(SQRT_EPS) * np.sqrt(ss) * np.sqrt(yy))


def sigma_of(init, init_val, sigma_min, sigma_max, ss, sy, yy):
    dt = type(ss)
    s1, s2 = sy / ss, yy / sy
    sg = {"scalar1": s1, "scalar2": s2, "scalar3": (s1 + s2) / dt(2), "scalar4": np.sqrt(s1 * s2), "constant": dt(init_val)}[init]
    return max(min(dt(sigma_max), sg), dt(sigma_min))


def cholesky(M):
    """lower factor in M's dtype, or None when a pivot is <= 0 or not finite"""
    m = M.shape[0]
    J = np.array(M, copy=True)
    for j in range(m):
        d = J[j, j] - np.dot(J[j, :j], J[j, :j])
        if not (d > 0) or not np.isfinite(d):
            return None
        J[j, j] = np.sqrt(d)
        for i in range(j + 1, m):
            J[i, j] = (J[i, j] - np.dot(J[i, :j], J[j, :j])) / J[j, j]
        J[:j, j] = 0
    return J


def coefficients(sts, L, D, sigma):
    """-> (d, C, Lbar), or None when some D_j or a Cholesky pivot of M is <= 0 or not finite; everything in D's dtype"""
    dt = D.dtype
    m = D.shape[0]
    if not np.all(D > 0) or not np.all(np.isfinite(D)):
        return None
    d = 1 / np.sqrt(D)
    Lt = np.tril(L, -1) * d[None, :]
    M = Lt @ Lt.T + dt.type(sigma) * (sts + sts.T) / 2
    J = cholesky(M)
    if J is None:
        return None
    X = np.zeros((m, m), dtype=dt)                       # X = J^-1 by forward substitution, row by row
    I = np.eye(m, dtype=dt)
    for r in range(m):
        X[r] = (I[r] - J[r, :r] @ X[:r]) / J[r, r]
    C = X.T.copy()
    return d, C, Lt.T @ C


def columns(S, Y, sts, L, D, sigma):
    """-> (V, U) or None"""
    co = coefficients(sts, L, D, sigma)
    if co is None:
        return None
    d, C, Lbar = co
    V = Y * d[None, :]
    return V, D.dtype.type(sigma) * (S @ C) + V @ Lbar


def recursive_bfgs(S, Y, sigma):
    """the dense BFGS matrix of the pairs (columns of S, Y, oldest first) started from sigma I, in S's dtype"""
    rows, k = S.shape
    B = np.zeros((rows, rows), dtype=S.dtype)
    B[np.diag_indices(rows)] = S.dtype.type(sigma)
    for j in range(k):
        s, y = S[:, j], Y[:, j]
        Bs = B @ s
        B -= np.outer(Bs / np.dot(s, Bs), Bs)
        B += np.outer(y / np.dot(y, s), y)
    return B


def recursive_terms(S, Y, sigma):
    """the same recursion with B_j kept as sigma I + P P^T - Q Q^T (P_j = y_j / sqrt(y_j^T s_j), Q_j = B_(j-1) s_j / sqrt(s_j^T B_(j-1) s_j)) instead of
    as a dense matrix: B_(j-1) s_j costs O(rows j), not O(rows^2).  dense(P, Q, sigma) is recursive_bfgs(S, Y, sigma); no Cholesky, no D, L, S^T S."""
    rows, k = S.shape
    sg = S.dtype.type(sigma)
    P = np.zeros((rows, k), dtype=S.dtype); Q = np.zeros((rows, k), dtype=S.dtype)
    for j in range(k):
        s, y = S[:, j], Y[:, j]
        b = sg * s + P[:, :j] @ (P[:, :j].T @ s) - Q[:, :j] @ (Q[:, :j].T @ s)
        Q[:, j] = b / np.sqrt(np.dot(s, b))
        P[:, j] = y / np.sqrt(np.dot(y, s))
    return P, Q


def dense(V, U, sigma):
    """sigma I + V V^T - U U^T"""
    B = V @ V.T - U @ U.T
    B[np.diag_indices(B.shape[0])] += V.dtype.type(sigma)
    return B


class History:
    """the state behind a handle's lbfgs_* calls; S, Y, V, U, D, L, STS as lbfgs_get returns them (oldest first)"""

    def __init__(self, rows, max_history, init="scalar1", init_val=1.0, sigma_min=1e-8, sigma_max=1e8, dtype=np.float64):
        self.dt = np.dtype(dtype)
        self.rows, self.max_history, self.init = rows, max_history, init
        self.init_val, self.sigma_min, self.sigma_max = init_val, sigma_min, sigma_max
        self.reset()

    def reset(self):
        dt = self.dt
        self.S = np.zeros((self.rows, 0), dtype=dt); self.Y = np.zeros((self.rows, 0), dtype=dt)
        self.D = np.zeros(0, dtype=dt); self.L = np.zeros((0, 0), dtype=dt); self.STS = np.zeros((0, 0), dtype=dt)
        self.sigma = dt.type(self.init_val)
        self.V = self.U = None                           # the installed columns
        self.skipped_in_a_row = 0

    @property
    def memory(self):
        return self.S.shape[1]

    def push(self, s, y):
        dt = self.dt
        s = np.asarray(s).astype(dt); y = np.asarray(y).astype(dt)
        with np.errstate(all="ignore"):
            ss, sy, yy = np.dot(s, s), np.dot(s, y), np.dot(y, y)
            if skip(ss, sy, yy):
                self.skipped_in_a_row += 1
                return SKIPPED
        self.skipped_in_a_row = 0
        self.sigma = sigma_of(self.init, self.init_val, self.sigma_min, self.sigma_max, ss, sy, yy)
        sS, sY = s @ self.S, s @ self.Y                  # the new column of S^T S, the new row of L: over the pairs stored before
        if self.memory == self.max_history:              # shift
            self.S, self.Y = self.S[:, 1:], self.Y[:, 1:]
            self.D, self.L, self.STS = self.D[1:], self.L[1:, 1:], self.STS[1:, 1:]
            sS, sY = sS[1:], sY[1:]
        m = self.memory
        self.S = np.column_stack([self.S, s]); self.Y = np.column_stack([self.Y, y])
        D = np.zeros(m + 1, dtype=dt); D[:m] = self.D; D[m] = sy
        L = np.zeros((m + 1, m + 1), dtype=dt); L[:m, :m] = self.L; L[m, :m] = sY
        T = np.zeros((m + 1, m + 1), dtype=dt); T[:m, :m] = self.STS; T[m, :m] = sS; T[:m, m] = sS; T[m, m] = ss
        self.D, self.L, self.STS = D, L, T
        vu = columns(self.S, self.Y, self.STS, self.L, self.D, self.sigma)
        if vu is None:
            return NOT_POSDEF
        self.V, self.U = vu
        return STORED


def recomputed(S, Y):
    """D, L, S^T S straight from the stored pairs"""
    G = S.T @ Y
    return np.diag(G).copy(), np.tril(G, -1), S.T @ S


def make_pairs(rows, count, seed):
    """the tests' recipe: a = exp(U(ln 0.5, ln 2)) per row, S standard normal, Y = a S + 0.05 (standard normal)"""
    rng = np.random.default_rng(seed)
    a = np.exp(rng.uniform(np.log(0.5), np.log(2.0), rows))
    S = rng.standard_normal((rows, count))
    Y = a[:, None] * S + 0.05 * rng.standard_normal((rows, count))
    return S, Y
