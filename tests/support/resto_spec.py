"""numpy statement of the restoration-phase half of the limited-memory updater of include/mi355x_kkt.h (mi355x_kkt_lbfgs_define_resto,
_lbfgs_push_resto; reference IpLimMemQuasiNewtonUpdater.cpp with update_for_resto_: UpdateHessian :141-343 and :359-700, UpdateInternalData
:820-868, SetW :1338-1380, RecalcY/D/L :1382-1433), in the arithmetic `dtype` (float64: what the library computes in; longdouble: what it is held
to).  Per history: DR (rows positive entries), type (BFGS / SR1), special.  Per push: s, ypart, eta.  o is the element-wise product.

  y_new    ypart + eta DR o s: the BFGS skip test, sigma, s^T y_new, y_new^T y_new                                             (:337-341)
  stored Y Ypart + eta S -- WITHOUT DR (RecalcY gets S in the place of DR o S) -- with the current eta in every column; D, L from it   (:864, :1382-1433)
  BFGS     skip test; store; D, L at eta; min D <= 0: skipped, nothing but the counter changes (:387-399); sigma unless special (then -1);
           V takes only a new last column y_new / sqrt(s^T y_new) (:440-451); d = D^(-1/2), Lt = L diag(d), M = Lt Lt^T + sigma S^T S (or
           + eta S^T (DR o S)); C, Lbar; U = sigma S C + V Lbar (or eta (DR o S) C + V Lbar); M not positive definite: pair and V column stay  (:453-520)
  SR1      store; D, L; sigma by the SR1 rule unless special; Z = D + L + L^T - sigma S^T S (or - eta S^T (DR o S)); the split rule; W = Y - sigma S
           (or Y - eta DR o S), Y the stored one; U, V = W Qs split                                                            (:523-671)
  B0       sigma I, or eta DR when special                                                                                       (:1343-1355)

Two statements.  `Literal` transcribes the reference's flow: it keeps the full vectors (S, Ypart, DR o S, V) and at every push recomputes Y, D, L and
the Gram matrices from them.  `History` mirrors the library (ipopt_amd/csrc/lbfgs_host.h, "the restoration phase"): G = S^T Ypart, S^T S and
R = S^T (DR o S) grow by augment / shift, D = diag(G) + eta diag(S^T S), L = G + eta S^T S below the diagonal, and V's older columns come from the
ring with the eta and the scale 1 / sqrt(s^T y_new) of THEIR push.  tests/test_resto_spec.py holds the two against each other.
"""
from __future__ import annotations

import numpy as np

from tests.support import lbfgs_spec as lb
from tests.support import sr1_spec as sr

STORED, SKIPPED, NOT_POSDEF = 0, 1, 2
BFGS, SR1 = 0, 1
ETAS = (0.3, 0.3, 0.1, 0.03)                             # the tests' cycle: eta changes between stored pairs and across an eviction


def b0_of(H):
    """the diagonal of B0 as a vector of rows"""
    dt = H.dt
    return dt.type(H.eta) * H.DR if H.special else np.full(H.rows, dt.type(H.sigma), dtype=dt)


def dense(H):
    """diag(B0) + V V^T - U U^T of the installed columns"""
    B = H.V @ H.V.T - H.U @ H.U.T
    B[np.diag_indices(H.rows)] += b0_of(H)
    return B


class _Base:
    FIELDS = ()

    def __init__(self, rows, max_history, DR, type=BFGS, special=False, init="scalar1", init_val=1.0, sigma_min=1e-8, sigma_max=1e8, dtype=np.float64):
        self.dt = np.dtype(dtype)
        self.rows, self.max_history, self.type, self.special, self.init = rows, max_history, type, bool(special), init
        self.init_val, self.sigma_min, self.sigma_max = init_val, sigma_min, sigma_max
        self.DR = np.asarray(DR).astype(self.dt)
        self.reset()

    @property
    def memory(self):
        return self.S.shape[1]

    def snapshot(self):
        return {f: getattr(self, f) for f in self.FIELDS}

    def restore(self, snap):
        for f, v in snap.items():
            setattr(self, f, v)

    def undo(self):
        if self.backup is None:
            return 0
        self.restore(self.backup)
        self.skipped_in_a_row += 1
        self.backup = None
        return 1

    def _sigma(self, m_after, ss, sy, yy):
        if self.special:
            return self.dt.type(-1)
        if self.type == SR1:
            return sr.sigma_of(self.init, self.init_val, m_after, ss, sy, yy)
        return lb.sigma_of(self.init, self.init_val, self.sigma_min, self.sigma_max, ss, sy, yy)


def _append(A, col, full):
    return np.column_stack([A[:, 1:] if full else A, col])


class Literal(_Base):
    """the reference's flow on full vectors; every array is replaced, never written in place, so a snapshot is a backup"""
    FIELDS = ("S", "Ypart", "DRS", "Vhist", "Y", "D", "L", "STS", "R", "sigma", "eta", "E", "Qs", "nneg", "V", "U", "skipped_in_a_row")

    def reset(self):
        dt = self.dt
        z = lambda: np.zeros((self.rows, 0), dtype=dt)
        self.S, self.Ypart, self.DRS, self.Vhist, self.Y = z(), z(), z(), z(), z()
        self.D = np.zeros(0, dtype=dt); self.L = np.zeros((0, 0), dtype=dt); self.STS = np.zeros((0, 0), dtype=dt); self.R = np.zeros((0, 0), dtype=dt)
        self.sigma = dt.type(-1 if self.special else self.init_val); self.eta = dt.type(-1)
        self.E = np.zeros(0, dtype=dt); self.Qs = np.zeros((0, 0), dtype=dt); self.nneg = 0
        self.V = self.U = None
        self.skipped_in_a_row = 0
        self.backup = None

    def _update_internal_data(self, s, ypart, eta):
        """UpdateInternalData :820-868: store, then RecalcY with S in the place of DR o S, RecalcD, RecalcL"""
        full = self.memory == self.max_history
        self.S = _append(self.S, s, full); self.Ypart = _append(self.Ypart, ypart, full); self.DRS = _append(self.DRS, s * self.DR, full)
        self.STS = self.S.T @ self.S; self.R = self.S.T @ self.DRS
        self.Y = eta * self.S + self.Ypart
        G = self.S.T @ self.Y
        self.D, self.L = np.diag(G).copy(), np.tril(G, -1)
        self.eta = eta
        return full

    def push(self, s, ypart, eta):
        dt = self.dt
        s = np.asarray(s).astype(dt); ypart = np.asarray(ypart).astype(dt); eta = dt.type(eta)
        with np.errstate(all="ignore"):
            y = (eta * s) * self.DR + ypart                          # :337-341
            ss, sy, yy = np.dot(s, s), np.dot(s, y), np.dot(y, y)
        before = self.snapshot()
        if self.type == BFGS:
            if lb.skip(ss, sy, yy):
                self.skipped_in_a_row += 1
                return SKIPPED
            full = self._update_internal_data(s, ypart, eta)
            if self.D.min() <= 0:                                    # :387-399
                self.restore(before); self.skipped_in_a_row += 1
                return SKIPPED
            self.skipped_in_a_row = 0
            self.sigma = self._sigma(self.memory, ss, sy, yy)
            self.Vhist = _append(self.Vhist, y * (1 / np.sqrt(sy)), full)      # only the last column is new
            d = 1 / np.sqrt(self.D)
            Lt = self.L * d[None, :]
            M = Lt @ Lt.T + (eta * (self.R + self.R.T) / 2 if self.special else self.sigma * (self.STS + self.STS.T) / 2)
            J = lb.cholesky(M)
            if J is None:
                return NOT_POSDEF
            C = _inv_lower(J).T
            U = (eta * self.DRS if self.special else self.sigma * self.S) @ C
            self.V, self.U = self.Vhist, U + self.Vhist @ (Lt.T @ C)
            return STORED
        if not (np.isfinite(ss) and np.isfinite(sy) and np.isfinite(yy)):
            self.skipped_in_a_row += 1; self.backup = None
            return SKIPPED
        self._update_internal_data(s, ypart, eta)
        self.sigma = self._sigma(self.memory, ss, sy, yy)
        Z = np.diag(self.D) + self.L + self.L.T - (eta * (self.R + self.R.T) / 2 if self.special else self.sigma * (self.STS + self.STS.T) / 2)
        E, Q = sr.jacobi(Z)
        nneg, emin, emax = sr.split(E)
        self.last_ratio = float(emin / emax) if emax > 0 else 0.0
        if emax == 0 or emin / emax < dt.type(sr.RATIO_TOL):
            self.restore(before); self.skipped_in_a_row += 1; self.backup = None
            return SKIPPED
        Qs = Q / np.sqrt(np.abs(E))[None, :]
        W = self.Y - (eta * self.DRS if self.special else self.sigma * self.S)
        self.E, self.Qs, self.nneg = E, Qs, nneg
        self.U, self.V = W @ Qs[:, :nneg], W @ Qs[:, nneg:]
        self.skipped_in_a_row = 0
        self.backup = before
        return STORED


def _inv_lower(J):
    """J^-1 of a lower triangular J by forward substitution, row by row, in J's dtype"""
    m = J.shape[0]
    X = np.zeros((m, m), dtype=J.dtype); I = np.eye(m, dtype=J.dtype)
    for r in range(m):
        X[r] = (I[r] - J[r, :r] @ X[:r]) / J[r, r]
    return X


class History(_Base):
    """the state behind a handle's lbfgs_* calls on a restoration-phase history, kept as the library keeps it; S, Ypart, V, U, D, L, STS, G, R, eta_col,
    dv as lbfgs_get returns them (oldest first)"""
    FIELDS = ("S", "Ypart", "G", "STS", "R", "eta_col", "dv", "D", "L", "sigma", "eta", "E", "Qs", "nneg", "V", "U", "skipped_in_a_row")

    def reset(self):
        dt = self.dt
        self.S = np.zeros((self.rows, 0), dtype=dt); self.Ypart = np.zeros((self.rows, 0), dtype=dt)
        sq = lambda: np.zeros((0, 0), dtype=dt)
        self.G, self.STS, self.R, self.L, self.Qs = sq(), sq(), sq(), sq(), sq()
        self.eta_col = np.zeros(0, dtype=dt); self.dv = np.zeros(0, dtype=dt); self.D = np.zeros(0, dtype=dt); self.E = np.zeros(0, dtype=dt)
        self.sigma = dt.type(-1 if self.special else self.init_val); self.eta = dt.type(-1)
        self.nneg = 0
        self.V = self.U = None
        self.skipped_in_a_row = 0
        self.backup = None

    def _candidate(self, s, ypart, eta, dots, dv_new):
        """-> the fields of the state with the pair stored: Gram matrices by augment / shift, D and L at eta"""
        dt = self.dt
        sS, sYp, sR, ss, syp, sDs = dots
        lo = 1 if self.memory == self.max_history else 0
        m = self.memory - lo

        def grown(A, row, col, corner):
            B = np.zeros((m + 1, m + 1), dtype=dt)
            B[:m, :m] = A[lo:, lo:]; B[m, :m] = row[lo:]; B[m, m] = corner
            if col is not None:
                B[:m, m] = col[lo:]
            return B
        c = dict(S=np.column_stack([self.S[:, lo:], s]), Ypart=np.column_stack([self.Ypart[:, lo:], ypart]),
                 G=grown(self.G, sYp, None, syp), STS=grown(self.STS, sS, sS, ss),
                 R=grown(self.R, sR, sR, sDs) if self.special else np.zeros((m + 1, m + 1), dtype=dt),
                 eta_col=np.append(self.eta_col[lo:], eta), dv=np.append(self.dv[lo:], dv_new), eta=eta)
        c["D"] = np.diag(c["G"]) + eta * np.diag(c["STS"])
        c["L"] = np.tril(c["G"] + eta * c["STS"], -1)
        return c

    def push(self, s, ypart, eta):
        dt = self.dt
        s = np.asarray(s).astype(dt); ypart = np.asarray(ypart).astype(dt); eta = dt.type(eta)
        with np.errstate(all="ignore"):
            ds = self.DR * s
            ss, syp, ypyp, sDs, ypDs, DsDs = np.dot(s, s), np.dot(s, ypart), np.dot(ypart, ypart), np.dot(s, ds), np.dot(ypart, ds), np.dot(ds, ds)
            sy, yy = syp + eta * sDs, ypyp + eta * (2 * ypDs + eta * DsDs)
            dots = (s @ self.S, s @ self.Ypart, ds @ self.S, ss, syp, sDs)
        if self.type == BFGS:
            if lb.skip(ss, sy, yy):
                self.skipped_in_a_row += 1
                return SKIPPED
            c = self._candidate(s, ypart, eta, dots, 1 / np.sqrt(sy))
            if not np.all(c["D"] > 0):
                self.skipped_in_a_row += 1
                return SKIPPED
            self.restore(c)
            self.skipped_in_a_row = 0
            self.sigma = self._sigma(self.memory, ss, sy, yy)
            co = lb.coefficients(self.R if self.special else self.STS, self.L, self.D, eta if self.special else self.sigma)
            if co is None:
                return NOT_POSDEF
            _, C, Lbar = co
            V = (self.Ypart + (self.eta_col[None, :] * self.DR[:, None]) * self.S) * self.dv[None, :]
            f = eta * self.DR if self.special else np.full(self.rows, self.sigma, dtype=dt)
            self.V, self.U = V, f[:, None] * (self.S @ C) + V @ Lbar
            return STORED
        if not (np.isfinite(ss) and np.isfinite(sy) and np.isfinite(yy)):
            self.skipped_in_a_row += 1; self.backup = None
            return SKIPPED
        c = self._candidate(s, ypart, eta, dots, dt.type(0))
        m = c["S"].shape[1]
        sigma = self._sigma(m, ss, sy, yy)
        E, Qs, nneg = sr.coefficients(c["R"] if self.special else c["STS"], c["L"], c["D"], eta if self.special else sigma)
        if Qs is None:
            self.skipped_in_a_row += 1; self.backup = None
            return SKIPPED
        before = self.snapshot()
        self.restore(c)
        f = eta * self.DR if self.special else np.full(self.rows, sigma, dtype=dt)
        W = (self.Ypart + eta * self.S) - f[:, None] * self.S
        self.sigma, self.E, self.Qs, self.nneg = sigma, E, Qs, nneg
        self.U, self.V = W @ Qs[:, :nneg], W @ Qs[:, nneg:]
        self.skipped_in_a_row = 0
        self.backup = before
        return STORED


def make_resto(rows, count, seed, sr1=False):
    """the tests' recipe -> (S, Ypart, DR): lbfgs_spec.make_pairs (a = exp(U(ln 0.5, ln 2)) per row, S standard normal, Ypart = a S + 0.05 standard
    normal), for SR1 with `a` negated on every SECOND row; then DR = exp(U(ln 0.25, 0)) from the same stream.
    Every second row, not every third: with B0 = eta DR, Z is about S^T diag(a + eta (1 - DR)) S, which for rows >> k concentrates on
    rows mean(a) I; negating a third of the rows leaves the mean positive, and at rows >= 517 no seed of five tried (3000 .. 7000 + rows + k) gave one
    negative eigenvalue at k 6 or 12.  With every second row the mean is near zero and every (rows, k >= 6) case has a mixed split, special or not."""
    rng = np.random.default_rng(seed)
    a = np.exp(rng.uniform(np.log(0.5), np.log(2.0), rows))
    if sr1:
        a[::2] = -a[::2]
    S = rng.standard_normal((rows, count))
    Y = a[:, None] * S + 0.05 * rng.standard_normal((rows, count))
    DR = np.exp(rng.uniform(np.log(0.25), 0.0, rows))
    return S, Y, DR
