"""numpy statement of the limited-memory SR1 updater of include/mi355x_kkt.h (mi355x_kkt_lbfgs_define_sr1, _lbfgs_undo; reference
IpLimMemQuasiNewtonUpdater.cpp case SR1 :523-671, SplitEigenvalues :873-983), in the arithmetic `dtype` (float64: what the library computes in;
longdouble: what it is held to).  D, L, S^T S are those of tests/support/lbfgs_spec.py (same augment / shift).

  skip     only a non-finite s^T s, s^T y, y^T y, or the eigenvalue rule below; a skipped push changes nothing but skipped_in_a_row
  sigma    the new pair is the only stored one: init_val; otherwise t = max(1e-8, |s^T y|): scalar1 t / s^T s, scalar2 y^T y / t, scalar3 / scalar4
           their arithmetic / geometric mean, constant init_val; not clipped                                                  (:551-578)
  split    Z = D + L + L^T - sigma S^T S = Q diag(E) Q^T, E ascending, nneg of them < 0; emax = max(|E_0|, |E_(m-1)|), emin the |E_j| next to the
           sign change; skipped when emax = 0 or emin / emax < 1e-12                                                          (:890-928)
  columns  W = Y - sigma S, Qs[:, j] = Q[:, j] / sqrt(|E_j|), U = W Qs[:, :nneg], V = W Qs[:, nneg:]                           (:630-669)
  undo     one level: the state before the last stored push comes back, skipped_in_a_row is its earlier value plus one     (:523-532)

The eigen-solver is the library's own rule (ipopt_amd/csrc/lbfgs_host.h lb_jacobi) in `dtype`: numpy has no longdouble eigh, and the float64 run is
then a fair sample of what the library's arithmetic does.  `recursive_sr1` is the independent check: B <- B + r r^T / (r^T s), r = y - B s, from sigma I.
"""
from __future__ import annotations

import numpy as np

from tests.support.lbfgs_spec import make_pairs, dense      # noqa: F401  (re-exported: the tests take them from here)

STORED, SKIPPED = 0, 1
BFGS, SR1 = 0, 1
INIT = ("scalar1", "scalar2", "scalar3", "scalar4", "constant")
SWEEPS = 30
RATIO_TOL = 1e-12


class NoConvergence(Exception):
    pass


def sigma_of(init, init_val, m_after, ss, sy, yy):
    dt = type(ss)
    if m_after <= 1:
        return dt(init_val)
    t = max(dt(1e-8), abs(sy))
    s1, s2 = t / ss, yy / t
    return {"scalar1": s1, "scalar2": s2, "scalar3": (s1 + s2) / dt(2), "scalar4": np.sqrt(s1 * s2), "constant": dt(init_val)}[init]


def jacobi(Z):
    """cyclic Jacobi by rows in Z's dtype -> (E ascending, ties by index; Q in E's order).  u = half the spacing of the dtype at 1.
    skip (p, q) when |a_pq| <= u min(|a_pp|, |a_qq|) or |a_pq| <= u^2 |Z|_F; stop after the first sweep without a rotation; at most SWEEPS sweeps"""
    dt = Z.dtype
    m = Z.shape[0]
    A = np.array(Z, copy=True)
    Q = np.eye(m, dtype=dt)
    u = dt.type(np.finfo(dt).eps) / dt.type(2)
    floor = u * u * np.sqrt(np.sum(A * A))
    one = dt.type(1)
    for _ in range(SWEEPS):
        rotated = 0
        for p in range(m - 1):
            for q in range(p + 1, m):
                apq, app, aqq = A[p, q], A[p, p], A[q, q]
                g = abs(apq)
                if g <= u * min(abs(app), abs(aqq)) or g <= floor:
                    continue
                rotated += 1
                theta = (aqq - app) / (dt.type(2) * apq)
                t = (one if theta >= 0 else -one) / (abs(theta) + np.sqrt(theta * theta + one))
                c = one / np.sqrt(t * t + one)
                s = t * c
                akp, akq = A[:, p].copy(), A[:, q].copy()
                A[:, p] = c * akp - s * akq; A[:, q] = s * akp + c * akq
                A[p, :] = A[:, p]; A[q, :] = A[:, q]
                A[p, p] = app - t * apq; A[q, q] = aqq + t * apq; A[p, q] = A[q, p] = 0
                qp, qq = Q[:, p].copy(), Q[:, q].copy()
                Q[:, p] = c * qp - s * qq; Q[:, q] = s * qp + c * qq
        if rotated == 0:
            order = np.argsort(np.diag(A), kind="stable")
            return np.diag(A)[order].copy(), Q[:, order].copy()
    raise NoConvergence(f"{SWEEPS} sweeps")


def z_of(sts, L, D, sigma):
    Lt = np.tril(L, -1)
    return np.diag(D) + Lt + Lt.T - D.dtype.type(sigma) * (sts + sts.T) / 2


def split(E):
    """-> (nneg, emin, emax) by the reference's rule"""
    m = E.shape[0]
    nneg = int(np.sum(E < 0))
    emax = max(abs(E[0]), abs(E[-1]))
    emin = E[0] if nneg == 0 else -E[-1] if nneg == m else min(-E[nneg - 1], E[nneg])
    return nneg, emin, emax


def coefficients(sts, L, D, sigma):
    """-> (E, Qs, nneg), or (E, None, nneg) when the split rule says skip; everything in D's dtype"""
    E, Q = jacobi(z_of(sts, L, D, sigma))
    nneg, emin, emax = split(E)
    if emax == 0 or emin / emax < D.dtype.type(RATIO_TOL):
        return E, None, nneg
    return E, Q / np.sqrt(np.abs(E))[None, :], nneg


def recursive_sr1(S, Y, sigma):
    """the dense SR1 matrix of the pairs (columns of S, Y, oldest first) started from sigma I, in S's dtype; also the smallest |r^T s| / (|r| |s|) met"""
    rows, k = S.shape
    B = np.zeros((rows, rows), dtype=S.dtype)
    B[np.diag_indices(rows)] = S.dtype.type(sigma)
    worst = np.inf
    for j in range(k):
        s, y = S[:, j], Y[:, j]
        r = y - B @ s
        rs = np.dot(r, s)
        worst = min(worst, float(abs(rs) / (np.sqrt(np.dot(r, r)) * np.sqrt(np.dot(s, s)))))
        B += np.outer(r / rs, r)
    return B, worst


class History:
    """the state behind a handle's lbfgs_* calls on an SR1 history; S, Y, V, U, D, L, STS as lbfgs_get returns them (oldest first)"""
    FIELDS = ("S", "Y", "D", "L", "STS", "sigma", "E", "Qs", "nneg", "V", "U", "skipped_in_a_row")

    def __init__(self, rows, max_history, init="scalar1", init_val=1.0, dtype=np.float64):
        self.dt = np.dtype(dtype)
        self.rows, self.max_history, self.init, self.init_val = rows, max_history, init, init_val
        self.reset()

    def reset(self):
        dt = self.dt
        self.S = np.zeros((self.rows, 0), dtype=dt); self.Y = np.zeros((self.rows, 0), dtype=dt)
        self.D = np.zeros(0, dtype=dt); self.L = np.zeros((0, 0), dtype=dt); self.STS = np.zeros((0, 0), dtype=dt)
        self.sigma = dt.type(self.init_val)
        self.E = np.zeros(0, dtype=dt); self.Qs = np.zeros((0, 0), dtype=dt); self.nneg = 0
        self.V = self.U = None                           # the installed columns
        self.skipped_in_a_row = 0
        self.backup = None

    @property
    def memory(self):
        return self.S.shape[1]

    def push(self, s, y):
        dt = self.dt
        s = np.asarray(s).astype(dt); y = np.asarray(y).astype(dt)
        with np.errstate(all="ignore"):
            ss, sy, yy = np.dot(s, s), np.dot(s, y), np.dot(y, y)
        if not (np.isfinite(ss) and np.isfinite(sy) and np.isfinite(yy)):
            self.skipped_in_a_row += 1; self.backup = None
            return SKIPPED
        sS, sY = s @ self.S, s @ self.Y
        S0, Y0, D0, L0, T0 = self.S, self.Y, self.D, self.L, self.STS
        if self.memory == self.max_history:              # shift
            S0, Y0, D0, L0, T0, sS, sY = S0[:, 1:], Y0[:, 1:], D0[1:], L0[1:, 1:], T0[1:, 1:], sS[1:], sY[1:]
        m = S0.shape[1]
        S1 = np.column_stack([S0, s]); Y1 = np.column_stack([Y0, y])
        D = np.zeros(m + 1, dtype=dt); D[:m] = D0; D[m] = sy
        L = np.zeros((m + 1, m + 1), dtype=dt); L[:m, :m] = L0; L[m, :m] = sY
        T = np.zeros((m + 1, m + 1), dtype=dt); T[:m, :m] = T0; T[m, :m] = sS; T[:m, m] = sS; T[m, m] = ss
        sigma = sigma_of(self.init, self.init_val, m + 1, ss, sy, yy)
        E, Qs, nneg = coefficients(T, L, D, sigma)
        if Qs is None:
            self.skipped_in_a_row += 1; self.backup = None
            return SKIPPED
        self.backup = {f: getattr(self, f) for f in self.FIELDS}
        W = Y1 - sigma * S1
        self.S, self.Y, self.D, self.L, self.STS, self.sigma = S1, Y1, D, L, T, sigma
        self.E, self.Qs, self.nneg = E, Qs, nneg
        self.U, self.V = W @ Qs[:, :nneg], W @ Qs[:, nneg:]
        self.skipped_in_a_row = 0
        return STORED

    def undo(self):
        if self.backup is None:
            return 0
        for f, v in self.backup.items():
            setattr(self, f, v)
        self.skipped_in_a_row += 1
        self.backup = None
        return 1
