// kernels_lbfgs.hip.inc -- part of numeric.hip (one translation unit; included there, inside namespace mi355x, behind kernels_lowrank.hip.inc): the
// tall-skinny algebra of the limited-memory BFGS updater (reference IpLimMemQuasiNewtonUpdater.cpp: the dots of UpdateInternalData :769-818 and
// CheckSkippingBFGS :985-1019, the columns V and U :440-520; restated in DESIGN.md).  The history S, Y (rows x max_history each, leading dimension
// `ld`) is a RING of column slots: the kernels get the logical -> physical slot map by value, so dropping the oldest pair copies nothing.
// ================================================================================================
// Three kernels, all streaming (1/4 flop per byte in the dots, m / 16 -- 2 at m = 32 -- in the form: HBM is the ruler, fp64 MFMA buys nothing), each
// written once for the plain history and for the restoration phase (lbfgs_host.h, "the restoration phase": the ring's Y holds Ypart, DR (rows entries)
// is one more streamed vector, eta a scalar; B0 = sigma I, or eta DR when special).  `if constexpr` picks the expressions; a plain instantiation
// reads neither DR nor eta nor special, which every launch passes.
//   k_lb_dots<KP, MODE>  per slab of LR_SLAB rows the partials of  s^T S_j, s^T Y_j (j over the m live pairs, oldest first),  s^T s, s^T y, y^T y:
//               2 m + 3 numbers per slab (LB_PLAIN).  LB_RESTO, LB_RESTO_SPECIAL: one more group  s^T (DR o S_j)  (formed only when special, zeros
//               otherwise) and the scalars  s^T (DR o s), ypart^T (DR o s), (DR o s)^T (DR o s)  behind the three: 3 m + 6 numbers per slab.  Summed
//               over the slabs by k_lr_reduce (kernels_lowrank.hip.inc) in its fixed order
//   k_lb_form<KP, RESTO>  writes the new pair into its slot and forms  V = Y diag(d),  U = sigma S C + V Lbar  in one pass, one thread per row, the
//               small matrices (d, C, Lbar: lbfgs_host.h) in LDS.  RESTO, with dr = DR[i] a per-row scalar:  V[i, j] = fma(eta_col[j] dr, S[i, j],
//               Ypart[i, j]) dv[j],  and the factor of S C is  f = sigma, or eta dr when special
//   k_lb_form_sr1<KP, RESTO>  the SR1 sibling (reference :630-669):  W = Y - sigma S,  U = W Qs[:, :nneg],  V = W Qs[:, nneg:]  with the scaled
//               eigenvectors Qs of Z = D + L + L^T - sigma S^T S (lb_sr1_coefficients, lbfgs_host.h) in LDS; 2 m^2 flop per row over 8 (3 m + 2)
//               bytes: streaming as well.  RESTO:  W = (Ypart + eta S) - f S  (the reference's stored Y: no DR),  f as above
// No atomics; every sum has an order fixed by (rows, m) -- dots: a thread's four rows of the slab in ascending order, the 64 lanes of a wavefront by
// the xor butterfly 32, 16, 8, 4, 2, 1, the four wavefronts in ascending order, then k_lr_reduce's order over the slabs; form: k ascending in each sum.
// KP = the compile-time bound on m the loops are unrolled to (8 / 16 / 32: arrays indexed at compile time stay in registers).
// ================================================================================================
#define LB_MAX 32         // pairs (MI355X_KKT_LBFGS_MAX = LR_MAX: V and U have one column per stored pair)
enum { LB_PLAIN = 0, LB_RESTO = 1, LB_RESTO_SPECIAL = 2 };                                   // MODE of k_lb_dots; the form kernels know RESTO = (MODE != LB_PLAIN)
constexpr int lb_ngroup(int mode) { return mode == LB_PLAIN ? 2 : 3; }                       // groups of m dots against the history
constexpr int lb_nscal(int mode) { return mode == LB_PLAIN ? 3 : 6; }                        // scalars behind them
constexpr int lb_nout(int mode, int m = LB_MAX) { return lb_ngroup(mode) * m + lb_nscal(mode); }

struct LbRing { int m; unsigned char slot[LB_MAX]; };      // logical column j (oldest first), j < m, lives in physical slot slot[j]

// part[slab * nout + o], nout = lb_nout(MODE, m):  o < m: s^T S_o;  m <= o < 2 m: s^T Y_(o - m);  a resto history, 2 m <= o < 3 m: s^T (DR o S_(o - 2 m))
// (0 unless special);  then s^T s, s^T y, y^T y  and, a resto history, s^T (DR o s), y^T (DR o s), (DR o s)^T (DR o s)  -- over the slab's rows
template <int KP, int MODE>
__global__ __launch_bounds__(256) void k_lb_dots(const double* __restrict__ S, const double* __restrict__ Y, long long ld, const double* __restrict__ DR, const double* __restrict__ s,
                                                 const double* __restrict__ y, int rows, LbRing ring, double* __restrict__ part)
{
    constexpr int NG = lb_ngroup(MODE), NS = lb_nscal(MODE);
    __shared__ double wsum[4][lb_nout(MODE)];
    const int t = threadIdx.x, m = ring.m, nout = NG * m + NS;
    const long long r0 = (long long)blockIdx.x * LR_SLAB;
    double aS[KP], aY[KP], aR[MODE == LB_RESTO_SPECIAL ? KP : 1], sc[NS];
#pragma unroll
    for (int j = 0; j < KP; ++j) { aS[j] = 0.0; aY[j] = 0.0; if constexpr (MODE == LB_RESTO_SPECIAL) aR[j] = 0.0; }
#pragma unroll
    for (int e = 0; e < NS; ++e) sc[e] = 0.0;
    for (int q = 0; q < LR_SLAB / 256; ++q) {
        const long long r = r0 + q * 256 + t;
        if (r < rows) {
            const double sv = s[r], yv = y[r];
            double ds = 0.0;
            sc[0] = fma(sv, sv, sc[0]); sc[1] = fma(sv, yv, sc[1]); sc[2] = fma(yv, yv, sc[2]);
            if constexpr (MODE != LB_PLAIN) { ds = DR[r] * sv; sc[3] = fma(sv, ds, sc[3]); sc[4] = fma(yv, ds, sc[4]); sc[5] = fma(ds, ds, sc[5]); }
#pragma unroll
            for (int j = 0; j < KP; ++j)
                if (j < m) {                                           // (uniform)
                    const long long c = (long long)ring.slot[j] * ld + r;
                    const double Sv = S[c];
                    aS[j] = fma(sv, Sv, aS[j]); aY[j] = fma(sv, Y[c], aY[j]);
                    if constexpr (MODE == LB_RESTO_SPECIAL) aR[j] = fma(ds, Sv, aR[j]);
                }
        }
    }
    const int w = t >> 6, lane = t & 63;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int e = 0; e < NS; ++e) sc[e] += __shfl_xor(sc[e], d);
#pragma unroll
        for (int j = 0; j < KP; ++j)
            if (j < m) { aS[j] += __shfl_xor(aS[j], d); aY[j] += __shfl_xor(aY[j], d); if constexpr (MODE == LB_RESTO_SPECIAL) aR[j] += __shfl_xor(aR[j], d); }
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < KP; ++j)
            if (j < m) {
                wsum[w][j] = aS[j]; wsum[w][m + j] = aY[j];
                if constexpr (MODE == LB_RESTO) wsum[w][2 * m + j] = 0.0;
                if constexpr (MODE == LB_RESTO_SPECIAL) wsum[w][2 * m + j] = aR[j];
            }
#pragma unroll
        for (int e = 0; e < NS; ++e) wsum[w][NG * m + e] = sc[e];
    }
    __syncthreads();
    if (t < nout) part[(long long)blockIdx.x * nout + t] = ((wsum[0][t] + wsum[1][t]) + wsum[2][t]) + wsum[3][t];
}

// coef (device): d[LB_MAX], then C and Lbar, LB_MAX x LB_MAX column-major each (C upper, Lbar strictly upper triangular; zero elsewhere); RESTO
// (LBH_NCOEF_RESTO doubles): d is dv, and eta_col[LB_MAX] stands behind Lbar.
// ring.m counts the NEW pair, which is logical column m - 1: it is read from s, y and written to its slot of S, Y.  Per row i
//   V[i, j] = Y[i, j] d_j,   U[i, j] = fma(sigma, sum_{k <= j} S[i, k] C[k, j], sum_{k < j} V[i, k] Lbar[k, j])      (k ascending, fma chains from 0)
// RESTO:  V[i, j] = fma(eta_col[j] dr, S[i, j], Ypart[i, j]) dv[j],  and special != 0 (B0 = eta DR) puts eta dr in the place of sigma, which is not read then.
template <int KP, bool RESTO>
__global__ __launch_bounds__(256) void k_lb_form(double* S, double* Y, long long ld, const double* __restrict__ s, const double* __restrict__ y, int rows,
                                                 LbRing ring, const double* __restrict__ coef, double sigma, double* __restrict__ V, double* __restrict__ U, long long ldv,
                                                 const double* __restrict__ DR, double eta, int special)
{
    __shared__ double sd[KP], se[RESTO ? KP : 1], sC[KP * KP], sL[KP * KP];
    const int m = ring.m;
    for (int e = threadIdx.x; e < KP * KP; e += 256) {
        const int k = e % KP, j = e / KP;
        sC[e] = coef[LB_MAX + k + j * LB_MAX]; sL[e] = coef[LB_MAX + LB_MAX * LB_MAX + k + j * LB_MAX];
    }
    if (threadIdx.x < KP) { sd[threadIdx.x] = coef[threadIdx.x]; if constexpr (RESTO) se[threadIdx.x] = coef[LB_MAX + 2 * LB_MAX * LB_MAX + threadIdx.x]; }
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    double dr = 0.0, f = sigma;
    if constexpr (RESTO) { dr = DR[i]; f = special ? eta * dr : sigma; }
    double sv[KP], vv[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        sv[j] = 0.0; vv[j] = 0.0;
        if (j < m) {                                                   // (uniform)
            const long long c = (long long)ring.slot[j] * ld + i;
            double yv;
            if (j == m - 1) { sv[j] = s[i]; yv = y[i]; S[c] = sv[j]; Y[c] = yv; }
            else { sv[j] = S[c]; yv = Y[c]; }
            if constexpr (RESTO) vv[j] = fma(se[j] * dr, sv[j], yv) * sd[j]; else vv[j] = yv * sd[j];
            V[i + j * ldv] = vv[j];
        }
    }
#pragma unroll
    for (int j = 0; j < KP; ++j)
        if (j < m) {
            double a = 0.0, b = 0.0;
#pragma unroll
            for (int k = 0; k <= j; ++k) a = fma(sv[k], sC[k + j * KP], a);
#pragma unroll
            for (int k = 0; k < j; ++k) b = fma(vv[k], sL[k + j * KP], b);
            U[i + j * ldv] = fma(f, a, b);
        }
}

// coef (device): Qs, LB_MAX x LB_MAX column-major (rows and columns >= m are zero).  ring.m = m live columns.  s != nullptr: the NEW pair is logical
// column m - 1, read from s, y and written to its slot of S, Y;  s == nullptr: every column is read from its slot and S, Y are only read (the
// re-form of an undo).  Per row i, w_k = fma(-sigma, S[i, k], Y[i, k]) and for every column c < m
//   out = sum_{k < m} w_k Qs[k, c]   (k ascending, an fma chain from 0)   ->   U[i, c] when c < nneg,  V[i, c - nneg] otherwise
// so V has m - nneg and U has nneg columns of leading dimension ldv: the caller sizes them so BEFORE the launch.
// RESTO:  w_k = fma(-f, S[i, k], fma(eta, S[i, k], Ypart[i, k])),  f = sigma, or eta DR[i] when special.
template <int KP, bool RESTO>
__global__ __launch_bounds__(256) void k_lb_form_sr1(double* S, double* Y, long long ld, const double* __restrict__ s, const double* __restrict__ y, int rows,
                                                     LbRing ring, const double* __restrict__ coef, double sigma, int nneg, double* __restrict__ V, double* __restrict__ U, long long ldv,
                                                     const double* __restrict__ DR, double eta, int special)
{
    __shared__ double sQ[KP * KP];
    const int m = ring.m;
    for (int e = threadIdx.x; e < KP * KP; e += 256) sQ[e] = coef[e % KP + (e / KP) * LB_MAX];
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    double f = sigma;
    if constexpr (RESTO) f = special ? eta * DR[i] : sigma;
    double w[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        w[k] = 0.0;
        if (k < m) {                                                   // (uniform)
            const long long c = (long long)ring.slot[k] * ld + i;
            double sv, yv;
            if (s != nullptr && k == m - 1) { sv = s[i]; yv = y[i]; S[c] = sv; Y[c] = yv; }
            else { sv = S[c]; yv = Y[c]; }
            if constexpr (RESTO) w[k] = fma(-f, sv, fma(eta, sv, yv)); else w[k] = fma(-sigma, sv, yv);
        }
    }
#pragma unroll
    for (int c = 0; c < KP; ++c)
        if (c < m) {
            double a = 0.0;
#pragma unroll
            for (int k = 0; k < KP; ++k)
                if (k < m) a = fma(w[k], sQ[k + c * KP], a);
            if (c < nneg) U[i + c * ldv] = a; else V[i + (c - nneg) * ldv] = a;
        }
}
