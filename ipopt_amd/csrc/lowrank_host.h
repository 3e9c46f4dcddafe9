// lowrank_host.h -- the two small dense factorisations of a low-rank update (numeric.hip lowrank_update; reference
// IpLowRankAugSystemSolver.cpp:319-323 and :383-387, DenseSymMatrix::HighRankUpdateTranspose + DenseGenMatrix::ComputeCholeskyFactor): plain host loops with a
// fixed order, column-major p x p with leading dimension p, p <= 32.  No HIP in here: a stand-alone host program can include it.
#pragma once
#include <cmath>

namespace mi355x {

// M <- sign * sym(G) + I,  sym(G) = (G + G^T) / 2
inline void lr_shifted_sym(const double* G, int p, double sign, double* M)
{
    for (int j = 0; j < p; ++j)
        for (int i = 0; i < p; ++i) M[i + j * p] = sign * (0.5 * (G[i + j * p] + G[j + i * p])) + (i == j ? 1.0 : 0.0);
}

// lower Cholesky factor in place (the strict upper triangle is zeroed); false when a pivot is <= 0 or not finite: M is not positive definite
inline bool lr_cholesky(double* M, int p)
{
    for (int j = 0; j < p; ++j) {
        double d = M[j + j * p];
        for (int k = 0; k < j; ++k) d -= M[j + k * p] * M[j + k * p];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        d = std::sqrt(d);
        M[j + j * p] = d;
        for (int i = j + 1; i < p; ++i) {
            double s = M[i + j * p];
            for (int k = 0; k < j; ++k) s -= M[i + k * p] * M[j + k * p];
            M[i + j * p] = s / d;
        }
        for (int i = 0; i < j; ++i) M[i + j * p] = 0.0;
    }
    return true;
}

// b <- (L L^T)^{-1} b for q columns of length p
inline void lr_cholesky_solve(const double* L, int p, double* b, int q)
{
    for (int c = 0; c < q; ++c) {
        double* y = b + c * p;
        for (int i = 0; i < p; ++i) { double s = y[i]; for (int k = 0; k < i; ++k) s -= L[i + k * p] * y[k]; y[i] = s / L[i + i * p]; }
        for (int i = p - 1; i >= 0; --i) { double s = y[i]; for (int k = i + 1; k < p; ++k) s -= L[k + i * p] * y[k]; y[i] = s / L[i + i * p]; }
    }
}

} // namespace mi355x
