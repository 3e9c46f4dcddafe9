// kernels_lowrank.hip.inc -- part of numeric.hip (one translation unit; included there, inside namespace mi355x): the tall-skinny algebra of a
// low-rank-updated solve,  K~ = K + V V^T - U U^T  with V (rows x nv), U (rows x nu) on `rows` indices of the caller's numbering (the first `rows`, or those of the row map)
// (reference IpLowRankAugSystemSolver.cpp:299-396 UpdateFactorization, :195-228 Solve; the in-place form is restated in DESIGN.md).
// ================================================================================================
// Under a row map (lowrank_rowmap; P_LowRank, :274-290, :449-457) row i of V and U is the caller's index idx[i]: the n-row operands are then gathered
// through the map (k_lr_gram<GA, GB>, k_lr_apply<true>), the columns scattered into their n-row form (k_lr_scatter), a full-space pair gathered (k_lr_gather2).
// Three kernels, all of them streaming: at p = q = 32 a Gram does 4 flop per byte, so HBM is the ruler and fp64 MFMA buys nothing.
//   k_lr_gram     partial p x q blocks of A^T B, one per SLAB of LR_SLAB rows (the split depends on `rows` alone)
//   k_lr_reduce   ONE workgroup: sums the partials of all slabs in a fixed order; in solve mode applies an uploaded Cholesky factor to every column
//   k_lr_apply    X (n x q) += sigma Z (n x p) T (p x q), T in device memory
// No atomics on floating-point data; every sum has an order fixed by (rows, p, q) -- per output element: the rows of a chunk in `L` interleaved
// lanes, the chunks of a slab in ascending order, the lanes in ascending order, the slabs in LR_RLANES contiguous runs (each ascending, then the runs
// ascending).  Right-hand sides of a solve are separate grid rows with q = 1 each, so a column's sums do not depend on how many columns travel with it.
// ================================================================================================
#define LR_MAX   32       // columns of V, and of U (MI355X_KKT_LOWRANK_MAX)
#define LR_SLAB  1024     // rows of one workgroup's slab
#define LR_CHUNK 64       // rows staged in LDS at a time
#define LR_RLANES 8       // lanes per output element of the final reduction (a fixed number: the order depends on the number of slabs alone)
#define LR_LDC   (LR_CHUNK + 1)      // (odd leading dimension: the p columns of one row fall on distinct LDS banks)

// row lanes per output element: the largest power of two with nout * L <= 256, at most LR_CHUNK (nout > 128: one lane, several outputs per thread)
__host__ __device__ __forceinline__ int lr_lanes(int nout) { int L = 1; while (2 * L * nout <= 256 && 2 * L <= LR_CHUNK) L *= 2; return L; }

// part[(blockIdx.y * gridDim.x + slab) * p * q + i + j * p] = sum over the slab's rows r of A[ra(r) + i lda] * B[rb(r) + (blockIdx.y q + j) ldb]
// GA / GB: that side has n rows and is read through the row map, ra(r) = idx[r] (ExpansionMatrix::ExpandedPosIndices: strictly ascending, validated on the
// host by lr_rowmap_check, so a gathered chunk touches no more cache lines than its span); the other side has `rows` rows, ra(r) = r.  The chunk's 64
// indices are staged in LDS once, not once per column.  Every summation order is that of the unmapped kernel; <false, false> IS the unmapped kernel.
template <bool GA, bool GB>
__global__ __launch_bounds__(256) void k_lr_gram(const double* __restrict__ A, long long lda, const double* __restrict__ B, long long ldb, int rows, int p, int q, double* __restrict__ part, const int* __restrict__ idx)
{
    __shared__ double sa[LR_MAX * LR_LDC], sb[LR_MAX * LR_LDC], red[256];
    __shared__ int si[(GA || GB) ? LR_CHUNK : 1];
    const int t = threadIdx.x, nout = p * q;
    const int L = lr_lanes(nout), l = t % L, og = t / L, ostep = 256 / L;
    const long long r0 = (long long)blockIdx.x * LR_SLAB;
    B += (long long)blockIdx.y * q * ldb;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int ch = 0; ch < LR_SLAB / LR_CHUNK; ++ch) {
        const long long rc = r0 + (long long)ch * LR_CHUNK;
        if (rc >= rows) break;                                        // (uniform: the whole workgroup leaves together)
        if constexpr (GA || GB) {
            if (t < LR_CHUNK) si[t] = (rc + t < rows) ? idx[rc + t] : 0;
            __syncthreads();
        }
        for (int e = t; e < LR_CHUNK * p; e += 256) { const int r = e % LR_CHUNK, c = e / LR_CHUNK; sa[c * LR_LDC + r] = (rc + r < rows) ? A[(GA ? (long long)si[r] : rc + r) + c * lda] : 0.0; }
        for (int e = t; e < LR_CHUNK * q; e += 256) { const int r = e % LR_CHUNK, c = e / LR_CHUNK; sb[c * LR_LDC + r] = (rc + r < rows) ? B[(GB ? (long long)si[r] : rc + r) + c * ldb] : 0.0; }
        __syncthreads();
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
            const int o = og + ps * ostep;
            if (o < nout) {
                const double* a = sa + (o % p) * LR_LDC; const double* b = sb + (o / p) * LR_LDC;
                double s = acc[ps];
                for (int r = l; r < LR_CHUNK; r += L) s = fma(a[r], b[r], s);
                acc[ps] = s;
            }
        }
        __syncthreads();
    }
    double* out = part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * nout;
    if (L == 1) {
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) { const int o = og + ps * ostep; if (o < nout) out[o] = acc[ps]; }
    } else {                                                          // (nout * L <= 256: one output per thread group, the lanes summed in ascending order)
        red[t] = acc[0];
        __syncthreads();
        if (l == 0 && og < nout) { double s = red[t]; for (int k = 1; k < L; ++k) s += red[t + k]; out[og] = s; }
    }
}

// out[i + c p] (p x ncol, device memory) = sum over the slabs s of part[c cstride + s sstride + i] (in LR_RLANES contiguous runs, see below); with Lf != nullptr each column is then
// solved with the Cholesky factor Lf (p x p, lower, column-major): forward and back substitution, one thread per column, serial, in LDS.  ncol <= LR_MAX.
__global__ __launch_bounds__(256) void k_lr_reduce(const double* __restrict__ part, int nslab, long long cstride, long long sstride, int p, int ncol, const double* __restrict__ Lf, double* __restrict__ out)
{
    __shared__ double g[LR_MAX * LR_MAX], lf[LR_MAX * LR_MAX], red[256];
    const int t = threadIdx.x;
    // 32 outputs at a time, LR_RLANES lanes each: a lane sums a contiguous run of slabs in ascending order, lane 0 then the lanes in ascending order
    const int lane = t % LR_RLANES, per = (nslab + LR_RLANES - 1) / LR_RLANES, s0 = lane * per, s1 = min(nslab, s0 + per);
    for (int e0 = 0; e0 < p * ncol; e0 += 256 / LR_RLANES) {
        const int e = e0 + t / LR_RLANES;
        double s = 0.0;
        if (e < p * ncol) {
            const double* src = part + (long long)(e / p) * cstride + e % p;
            for (int sl = s0; sl < s1; ++sl) s += src[(long long)sl * sstride];
        }
        red[t] = s;
        __syncthreads();
        if (lane == 0 && e < p * ncol) { double a = red[t]; for (int k = 1; k < LR_RLANES; ++k) a += red[t + k]; g[e] = a; }
        __syncthreads();
    }
    if (Lf) for (int e = t; e < p * p; e += 256) lf[e] = Lf[e];
    __syncthreads();
    if (Lf && t < ncol) {
        double* y = g + t * p;
        for (int i = 0; i < p; ++i) { double s = y[i]; for (int k = 0; k < i; ++k) s -= lf[i + k * p] * y[k]; y[i] = s / lf[i + i * p]; }
        for (int i = p - 1; i >= 0; --i) { double s = y[i]; for (int k = i + 1; k < p; ++k) s -= lf[k + i * p] * y[k]; y[i] = s / lf[i + i * p]; }
    }
    __syncthreads();
    for (int e = t; e < p * ncol; e += 256) out[e] = g[e];
}

// X[x(i) + j ldx] += sigma * sum_k Z[i + k ldz] T[k + j p], k ascending (one thread per row: Z is read once, coalesced along the rows)
// MX (lr_residual under a row map only): Z has n = `rows` rows and X is an x-block vector, x(i) = idx[i]; otherwise x(i) = i
template <bool MX>
__global__ __launch_bounds__(256) void k_lr_apply(double* __restrict__ X, long long ldx, const double* __restrict__ Z, long long ldz, const double* __restrict__ T, long long n, int p, int q, double sigma, const int* __restrict__ idx)
{
    __shared__ double ts[LR_MAX * LR_MAX];
    for (int e = threadIdx.x; e < LR_MAX * q; e += 256) { const int k = e % LR_MAX, j = e / LR_MAX; ts[e] = k < p ? T[k + j * p] : 0.0; }
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long xi = MX ? (long long)idx[i] : i;
    double z[LR_MAX];
#pragma unroll
    for (int k = 0; k < LR_MAX; ++k) z[k] = k < p ? Z[i + k * ldz] : 0.0;
    for (int j = 0; j < q; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < LR_MAX; ++k) s = fma(z[k], ts[k + LR_MAX * j], s);
        X[xi + j * ldx] += sigma * s;
    }
}

// Z[idx[i] + k n] = A[i + k rows] for the `rows` mapped rows of column k = blockIdx.y (lr_pad under a row map, behind the zero fill of Z: P V, P U)
__global__ __launch_bounds__(256) void k_lr_scatter(double* __restrict__ Z, long long n, const double* __restrict__ A, int rows, const int* __restrict__ idx)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    Z[idx[i] + (long long)blockIdx.y * n] = A[i + (long long)blockIdx.y * rows];
}

// s[i] = sx[idx[i]], y[i] = yx[idx[i]]: the reduced pair of a mapped push, P^T s_full and P^T y_full (IpLimMemQuasiNewtonUpdater.cpp:323-324), one launch
__global__ __launch_bounds__(256) void k_lr_gather2(const double* __restrict__ sx, const double* __restrict__ yx, int rows, const int* __restrict__ idx, double* __restrict__ s, double* __restrict__ y)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const long long x = idx[i];
    s[i] = sx[x]; y[i] = yx[x];
}
