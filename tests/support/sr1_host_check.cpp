// Stand-alone host program for tests/test_sr1_abi.py: lb_sr1_coefficients (ipopt_amd/csrc/lbfgs_host.h) on m = 1, 2, 31, 32 with an all-positive, an
// all-negative and a mixed Z = D + L + L^T - sigma S^T S; built with -fsanitize=address,undefined and run on the CPU.  Z is strictly diagonally
// dominant, so its negative eigenvalues are counted by its negative diagonal entries; the answer is checked through
//   Z (Qs+ Qs+^T - Qs- Qs-^T) = I   to 1e-12 (cond(Z) <= 4: |Z_jj| in [m + 1, 2 m], off-diagonal row sums below 0.4 m).
// Exit status 0: every case passed.
#include <cmath>
#include <cstdio>
#include "lbfgs_host.h"

using namespace mi355x;

static int run(int m, int kind)      // kind 0: all positive, 1: all negative, 2: mixed
{
    double sts[LBH_MAX * LBH_MAX], L[LBH_MAX * LBH_MAX], D[LBH_MAX], E[LBH_MAX], Qs[LBH_MAX * LBH_MAX], Z[LBH_MAX * LBH_MAX];
    const double sigma = 0.5;
    int expect = 0;
    for (int j = 0; j < m; ++j) {
        const bool neg = kind == 1 || (kind == 2 && j % 3 == 1);
        expect += neg ? 1 : 0;
        D[j] = (neg ? -1.0 : 1.0) * (m + j + 1);
        for (int i = 0; i < m; ++i) {
            sts[i + j * m] = 0.02 / (1 + (i > j ? i - j : j - i));
            L[i + j * m] = i > j ? 0.3 * std::cos(1.0 + i + 2.0 * j) : 0.0;
        }
    }
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i)
            Z[i + j * m] = (i == j ? D[j] : i > j ? L[i + j * m] : L[j + i * m]) - sigma * sts[i + j * m];
    int nneg = -1;
    const int r = lb_sr1_coefficients(m, sts, L, m, D, sigma, E, Qs, m, &nneg);
    if (r != LB_SR1_OK || nneg != expect) { std::printf("m %d kind %d: status %d, nneg %d (expected %d)\n", m, kind, r, nneg, expect); return 1; }
    for (int j = 0; j + 1 < m; ++j) if (!(E[j] <= E[j + 1])) { std::printf("m %d kind %d: E is not ascending at %d\n", m, kind, j); return 1; }
    double worst = 0.0;
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) {
            double a = 0.0;                                            // (Z Zinv)_ij, Zinv_kj = sum_c sign_c Qs_kc Qs_jc
            for (int k = 0; k < m; ++k) {
                double zi = 0.0;
                for (int c = 0; c < m; ++c) zi += (c < nneg ? -1.0 : 1.0) * Qs[k + c * m] * Qs[j + c * m];
                a += Z[i + k * m] * zi;
            }
            worst = std::fmax(worst, std::fabs(a - (i == j ? 1.0 : 0.0)));
        }
    std::printf("m %d kind %d: nneg %d, |Z Zinv - I| %.2e\n", m, kind, nneg, worst);
    return worst <= 1e-12 ? 0 : 1;
}

int main()
{
    int bad = 0;
    const int ms[4] = {1, 2, 31, 32};
    for (int q = 0; q < 4; ++q)
        for (int kind = 0; kind < 3; ++kind) {
            if (kind == 2 && ms[q] == 1) continue;                     // (one eigenvalue cannot be mixed)
            bad += run(ms[q], kind);
        }
    // the split rule: the zero matrix and a singular Z are skips, and E is still set
    {
        double z[4] = {0, 0, 0, 0}, d[2] = {0, 0}, E[2], Qs[4]; int nneg = -1;
        if (lb_sr1_coefficients(2, z, z, 2, d, 1.0, E, Qs, 2, &nneg) != LB_SR1_SKIP) { std::printf("zero Z: not skipped\n"); ++bad; }
        double one[4] = {1, 1, 1, 1}, d2[2] = {2, 2};                  // Z = [[1, -1], [-1, 1]]: eigenvalues 0, 2
        double L2[4] = {0, 0, 0, 0};
        if (lb_sr1_coefficients(2, one, L2, 2, d2, 1.0, E, Qs, 2, &nneg) != LB_SR1_SKIP) { std::printf("singular Z: not skipped\n"); ++bad; }
    }
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
