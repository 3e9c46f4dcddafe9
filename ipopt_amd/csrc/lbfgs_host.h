// lbfgs_host.h -- the small dense algebra of the limited-memory BFGS updater (numeric.hip lbfgs_push and the stand-alone
// mi355x_kkt_lbfgs_coefficients share it; reference IpLimMemQuasiNewtonUpdater.cpp: CheckSkippingBFGS :985-1019, sigma :405-432,
// UpdateInternalData :769-818, the columns :440-520): plain host loops with a fixed order, column-major with an explicit leading
// dimension, at most 32 pairs.  No HIP in here: a stand-alone host program can include it.
#pragma once
#include <cmath>
#include <limits>
#include "lowrank_host.h"      // lr_cholesky

namespace mi355x {

static constexpr int LBH_MAX = 32;      // pairs (MI355X_KKT_LBFGS_MAX)

// the pair (s, y) is not stored: s^T y <= sqrt(eps) |s| |y|, or one of the three dots is not finite (the reference never sees such a pair)
inline bool lb_skip(double ss, double sy, double yy)
{
    if (!std::isfinite(ss) || !std::isfinite(sy) || !std::isfinite(yy)) return true;
    return sy <= std::sqrt(std::numeric_limits<double>::epsilon()) * std::sqrt(ss) * std::sqrt(yy);
}

// sigma of B0 = sigma I from the new pair: init 0..3 = scalar1..4, 4 = constant; then clipped to [smin, smax]
inline double lb_sigma(int init, double init_val, double smin, double smax, double ss, double sy, double yy)
{
    double sg = init_val;
    switch (init) {
    case 0: sg = sy / ss; break;
    case 1: sg = yy / sy; break;
    case 2: sg = (sy / ss + yy / sy) / 2.0; break;
    case 3: sg = std::sqrt((sy / ss) * (yy / sy)); break;
    default: break;
    }
    return std::fmax(std::fmin(smax, sg), smin);
}

// D (m), L (strictly lower; L_ij = s_i^T y_j, i > j) and S^T S of m stored pairs, leading dimension LBH_MAX, take the new pair: "augment"
// while m < max_history, "shift" (the oldest pair leaves) when the history is full.  sS[j] = s^T S_j and sY[j] = s^T Y_j over the m pairs stored
// BEFORE the call (oldest first), ss = s^T s, sy = s^T y.  Only the new row and column are computed.  Returns the new m.
inline int lb_store(int m, int max_history, double* D, double* L, double* STS, const double* sS, const double* sY, double ss, double sy)
{
    const int ld = LBH_MAX;
    int off = 0;
    if (m == max_history) {                                          // shift: entry (i, j) <- (i + 1, j + 1)
        for (int j = 0; j + 1 < m; ++j) {
            D[j] = D[j + 1];
            for (int i = 0; i + 1 < m; ++i) { L[i + j * ld] = L[i + 1 + (j + 1) * ld]; STS[i + j * ld] = STS[i + 1 + (j + 1) * ld]; }
        }
        off = 1; --m;
    }
    for (int j = 0; j < m; ++j) {
        L[m + j * ld] = sY[j + off]; L[j + m * ld] = 0.0;
        STS[m + j * ld] = STS[j + m * ld] = sS[j + off];
    }
    L[m + m * ld] = 0.0; STS[m + m * ld] = ss; D[m] = sy;
    return m + 1;
}

// d = D^(-1/2);  Lt = L diag(d);  M = Lt Lt^T + sigma S^T S;  J = chol(M);  C = J^(-T) (upper);  Lbar = Lt^T C (strictly upper): then with
// V = Y diag(d) and U = sigma S C + V Lbar,  sigma I + V V^T - U U^T  is the BFGS matrix of the pairs started from sigma I.
// sts, L have leading dimension ldi; C, Lbar leading dimension ldo; d (m) may be null.  false: a D_j or a Cholesky pivot is <= 0 or not finite.
inline bool lb_coefficients(int m, const double* sts, const double* L, int ldi, const double* D, double sigma, double* d, double* C, double* Lbar, int ldo)
{
    double dd[LBH_MAX], Lt[LBH_MAX * LBH_MAX], J[LBH_MAX * LBH_MAX];
    for (int j = 0; j < m; ++j) {
        if (!(D[j] > 0.0) || !std::isfinite(D[j])) return false;
        dd[j] = 1.0 / std::sqrt(D[j]);
        if (d) d[j] = dd[j];
    }
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) Lt[i + j * m] = i > j ? L[i + j * ldi] * dd[j] : 0.0;
    for (int j = 0; j < m; ++j)
        for (int i = j; i < m; ++i) {
            double s = 0.0;
            for (int k = 0; k < j; ++k) s += Lt[i + k * m] * Lt[j + k * m];      // (Lt is strictly lower: k < min(i, j) = j)
            s += sigma * (0.5 * (sts[i + j * ldi] + sts[j + i * ldi]));
            J[i + j * m] = J[j + i * m] = s;
        }
    if (!lr_cholesky(J, m)) return false;
    // C = J^-T: column i of J^-1 by forward substitution on e_i, stored as row i of C
    for (int i = 0; i < m; ++i) {
        for (int r = 0; r < m; ++r) {
            if (r < i) { C[i + r * ldo] = 0.0; continue; }
            double s = r == i ? 1.0 : 0.0;
            for (int k = i; k < r; ++k) s -= J[r + k * m] * C[i + k * ldo];
            C[i + r * ldo] = s / J[r + r * m];
        }
    }
    // after the loop above C[i + r ldo] = (J^-1)[r, i] = (J^-T)[i, r]: upper triangular
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) {
            double s = 0.0;
            for (int k = i + 1; k <= j; ++k) s += Lt[k + i * m] * C[k + j * ldo];
            Lbar[i + j * ldo] = s;
        }
    return true;
}

} // namespace mi355x
