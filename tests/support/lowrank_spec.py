"""numpy statement of the low-rank-updated solve of include/mi355x_kkt.h (mi355x_kkt_lowrank_*): K~ = K + Vb Vb^T - Ub Ub^T with Vb, Ub the
rows x nv, rows x nu matrices V, U padded with zero rows to n.  Dense inner solves; what the device route is held to.

  update (reference IpLowRankAugSystemSolver.cpp:299-396):
      Z1 = K^-1 Vb,  M1 = I + sym(V^T Z1[:rows]),  W1 = K^-1 Ub,  C = M1^-1 (Z1[:rows]^T U),  Z2 = W1 - Z1 C,  M2 = I - sym(U^T Z2[:rows])
  solve, in place, both corrections taken from the running solution:
      x0 = K^-1 b,  x1 = x0 - Z1 M1^-1 (V^T x0[:rows]),  x = x1 + Z2 M2^-1 (U^T x1[:rows])
  solve_rhs_form: the reference's own form (:195-228), both corrections taken from the right-hand side: Z1^T b and Z2^T b.
"""
from __future__ import annotations

import numpy as np


def sym(G):
    return 0.5 * (G + G.T)


def pad(A, n):
    out = np.zeros((n, A.shape[1]))
    out[: A.shape[0]] = A
    return out


def dense_updated(K, V, U):
    """the dense K~"""
    Kt = np.array(K, dtype=np.float64, copy=True)
    r = V.shape[0]
    Kt[:r, :r] += V @ V.T - U @ U.T
    return Kt


def cholesky(M):
    """lower factor, or None when a pivot is <= 0 or not finite (what the library calls wrong inertia); the loop order of lowrank_host.h"""
    p = M.shape[0]
    L = np.array(M, dtype=np.float64, copy=True)
    for j in range(p):
        d = L[j, j] - np.dot(L[j, :j], L[j, :j])
        if not (d > 0.0) or not np.isfinite(d):
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, p):
            L[i, j] = (L[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
        L[:j, j] = 0.0
    return L


def chol_solve(L, B):
    import scipy.linalg as sl
    if L.shape[0] == 0:
        return np.array(B, copy=True)
    return sl.solve_triangular(L.T, sl.solve_triangular(L, B, lower=True), lower=False)


def update(K, V, U, solve=None):
    """-> dict(Z1, L1, M1, Z2, L2, M2, which): which = 0, or 1 / 2 when M1 / M2 is not positive definite (the later pieces are then None)"""
    n = K.shape[0]
    rows, nv, nu = V.shape[0], V.shape[1], U.shape[1]
    solve = solve or dense_solver(K)
    Z1 = solve(pad(V, n))
    M1 = np.eye(nv) + sym(V.T @ Z1[:rows])
    L1 = cholesky(M1)
    out = dict(Z1=Z1, M1=M1, L1=L1, Z2=None, M2=None, L2=None, which=0, rows=rows)
    if L1 is None:
        out["which"] = 1
        return out
    W1 = solve(pad(U, n))
    Cm = chol_solve(L1, Z1[:rows].T @ U)
    Z2 = W1 - Z1 @ Cm
    M2 = np.eye(nu) - sym(U.T @ Z2[:rows])
    L2 = cholesky(M2)
    out.update(Z2=Z2, M2=M2, L2=L2)
    if L2 is None:
        out["which"] = 2
    return out


def solve(K, V, U, upd, b, solve0=None):
    """the in-place form; b is (n,) or (n, nrhs)"""
    rows = V.shape[0]
    x = np.linalg.solve(K, b) if solve0 is None else solve0(b)
    x = x - upd["Z1"] @ chol_solve(upd["L1"], V.T @ x[:rows])
    x = x + upd["Z2"] @ chol_solve(upd["L2"], U.T @ x[:rows])
    return x


def solve_rhs_form(K, V, U, upd, b, solve0=None):
    """the reference's form: x = K^-1 b - Z1 M1^-1 (Z1^T b) + Z2 M2^-1 (Z2^T b)"""
    x = np.linalg.solve(K, b) if solve0 is None else solve0(b)
    x = x - upd["Z1"] @ chol_solve(upd["L1"], upd["Z1"].T @ b)
    x = x + upd["Z2"] @ chol_solve(upd["L2"], upd["Z2"].T @ b)
    return x


def num_neg(K):
    """negative eigenvalues of a dense symmetric matrix through a Bunch-Kaufman LDL^T (Sylvester), cheaper than the spectrum"""
    import scipy.linalg as sl
    _, d, _ = sl.ldl(K)
    n, i, neg = d.shape[0], 0, 0
    while i < n:
        if i + 1 < n and d[i + 1, i] != 0.0:
            neg += int((np.linalg.eigvalsh(d[i:i + 2, i:i + 2]) < 0).sum()); i += 2
        else:
            neg += int(d[i, i] < 0); i += 1
    return neg


def dense_solver(K):
    """B -> K^-1 B through ONE LU factorisation (what the tests share among the inner solves of a system)"""
    import scipy.linalg as sl
    lu = sl.lu_factor(K)
    return lambda B: sl.lu_solve(lu, B) if B.size else np.zeros_like(B)


def scaled_columns(K, rows, nv, nu, seed, lam_v=4.0, lam_u=0.75, u_factor=1.0, solve=None):
    """random V, U scaled by the tests' recipe: lambda_max(V^T (K^-1)_xx V) = lam_v, lambda_max(U^T ((K + Vb Vb^T)^-1)_xx U) = lam_u
    (x = the first `rows` indices).  Then lambda_min(M1) >= 1 -- when (K^-1)_xx is positive semidefinite, as it is for a KKT matrix with a
    positive definite reduced Hessian -- and lambda_min(M2) = 1 - lam_u.  u_factor multiplies U afterwards (2: M2 indefinite).
    `solve`: B -> K^-1 B (dense_solver); (K + Vb Vb^T)^-1 Ub is formed by Woodbury from it."""
    rng = np.random.default_rng(seed)
    n = K.shape[0]
    solve = solve or dense_solver(K)
    V = rng.standard_normal((rows, nv)); U = rng.standard_normal((rows, nu))
    if nv:
        lam = np.linalg.eigvalsh(sym(V.T @ solve(pad(V, n))[:rows])).max()
        V *= np.sqrt(lam_v / lam)
    if nu:
        Z1 = solve(pad(V, n))
        Y = solve(pad(U, n))
        Y = Y - Z1 @ np.linalg.solve(np.eye(nv) + sym(V.T @ Z1[:rows]), Z1[:rows].T @ U)
        lam = np.linalg.eigvalsh(sym(U.T @ Y[:rows])).max()
        U *= np.sqrt(lam_u / lam)
    return V, U * u_factor
