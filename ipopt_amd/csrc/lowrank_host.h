// lowrank_host.h -- the two small dense factorisations of a low-rank update (numeric.hip lowrank_update; reference
// IpLowRankAugSystemSolver.cpp:319-323 and :383-387, DenseSymMatrix::HighRankUpdateTranspose + DenseGenMatrix::ComputeCholeskyFactor): plain host loops with a
// fixed order, column-major p x p with leading dimension p, p <= 32; and the validation of a row map.  No HIP in here: a stand-alone host program can include it.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

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

// The row map of a low-rank update (lowrank_rowmap; the reference's P_LowRank, ExpansionMatrix::ExpandedPosIndices, IpLowRankAugSystemSolver.cpp:274-290): row i
// of V, U, S, Y, DR is the caller's index idx[i], 0-based, STRICTLY ascending, 0 <= idx[i] < n.  This check is the reason no kernel reading or writing
// through the map can index out of range: nothing reaches the device before it has passed.  rows == 0 or idx == nullptr removes the map (valid).
// false: `why` names the offending argument -- `rows`, `idx`, the first position that is not ascending, or the first value out of range.
inline bool lr_rowmap_check(long long n, int rows, const int32_t* idx, std::string& why)
{
    if (rows < 0 || rows > n) { why = "rows must be in [0, n] (rows = " + std::to_string(rows) + ", n = " + std::to_string(n) + ")"; return false; }
    if (rows > 0 && !idx) return true;      // (removes the map)
    for (int i = 0; i < rows; ++i) {
        if (idx[i] < 0 || idx[i] >= n) { why = "idx[" + std::to_string(i) + "] = " + std::to_string(idx[i]) + " is out of range: every index must be in [0, n)"; return false; }
        if (i > 0 && idx[i] <= idx[i - 1]) { why = "idx is not strictly ascending at position " + std::to_string(i) + " (idx[" + std::to_string(i - 1) + "] = " + std::to_string(idx[i - 1]) + ", idx[" + std::to_string(i) + "] = " + std::to_string(idx[i]) + ")"; return false; }
    }
    return true;
}
// a full-space vector of `len` entries read through a map whose largest index is `last` (idx[rows - 1]; -1: no map set)
inline bool lr_rowmap_len_check(long long len, long long last, std::string& why)
{
    if (last < 0) { why = "no row map is set (lowrank_rowmap first)"; return false; }
    if (len <= last) { why = "len = " + std::to_string(len) + " must be > idx[rows-1] = " + std::to_string(last); return false; }
    return true;
}

} // namespace mi355x
