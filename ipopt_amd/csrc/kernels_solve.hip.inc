// kernels_solve.hip.inc -- part of numeric.hip (one translation unit; included there, inside namespace mi355x): triangular solves: level kernels, two / four fronts per wavefront, chain groups, data-flow chain sweeps.
// ------------------------------------------------------------------------------------------------
// solves
// ------------------------------------------------------------------------------------------------
__global__ void k_load_rhs(DevView V, const double* b)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < V.n; i += gridDim.x * blockDim.x) V.xw[i] = V.scale[i] * b[V.perm[i]];
}
__global__ void k_store_sol(DevView V, double* b)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < V.n; i += gridDim.x * blockDim.x) b[V.perm[i]] = V.scale[i] * V.xw[i];
}

// iterative refinement in the scaled, permuted space:  xacc += xw;  xw <- bw - K xacc   (K = scaled matrix, symmetric row
// view => gather, no atomics).  first != 0: xacc = xw (no accumulation yet).  The residual is then solved for again.
__global__ void k_refine_residual(DevView V, int first)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < V.n; i += gridDim.x * blockDim.x)
        V.xacc[i] = first ? V.xw[i] : V.xacc[i] + V.xw[i];
}
__global__ void k_refine_spmv(DevView V)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < V.n; i += gridDim.x * blockDim.x) {
        double acc = 0.0;
        for (int p = V.rslot_ptr[i]; p < V.rslot_ptr[i + 1]; ++p) {
            const int q = V.rslot_idx[p];
            const int r = V.arow[q], c = V.acol[q];
            acc += V.aval[q] * V.xacc[r == i ? c : r];
        }
        V.xw[i] = V.bw[i] - acc;
    }
}
__global__ void k_save_rhs(DevView V) { for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < V.n; i += gridDim.x * blockDim.x) V.bw[i] = V.xw[i]; }
__global__ void k_refine_finish(DevView V) { for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < V.n; i += gridDim.x * blockDim.x) V.xw[i] += V.xacc[i]; }

// ------------------------------------------------------------------------------------------------
// Steps of a front that several sweep kernels take: ONE definition each.  The kernels that share a step agree bit for bit because they call the same
// expression -- same operand order inside each product and sum, same number and pairing of partial accumulators, same guards.
// ------------------------------------------------------------------------------------------------
// z = D^{-1} y over 1x1 and 2x2 pivots is NOT among them: every kernel spells it out.  Moved into a shared function, with the same expressions, the step
// gave other bits on tests/support/midfix.py hostile16, the one fixture with 2x2 pivots (which product of a * b + c * d goes into the fma is the compiler's
// choice, and it chose differently there).  It chose differently again when the pair, leaf-chain and mid kernels got their column loop (RB_ON below), so
// THOSE kernels name the fma: the form the compiler had chosen for each of them -- pair / leaf chain  fma(d, y_j, o y_j+-1)  for both rows of a 2x2 pivot,
// mid  fma(d, y_j, o y_j+1)  for its first and  fma(o, y_j-1, d y_j)  for its second row --, so one column and a block of columns agree.  Shared is the load of what the step needs, for the kernels that request everything
// the front record gives before they wait for anything: pivot type, the row's diagonal entry of D^{-1}, the off-diagonal entries towards the next and
// the previous row.
struct PivD { int pt; double dq, oq, oq1; };
__device__ __forceinline__ PivD ld_pivd(const DevView& V, const int c0, const int j, const bool on)
{
    PivD D = {1, 0.0, 0.0, 0.0};
    if (on) { D.pt = V.ptype[c0 + j]; D.dq = V.dinv[c0 + j]; D.oq = V.doff[c0 + j]; D.oq1 = j > 0 ? V.doff[c0 + j - 1] : 0.0; }
    return D;
}
// ys = L11^{-1} bp with the stored k x k inverse (column-major, lower triangle), a workgroup of 256: 4 threads per row (columns part, part + 4, ...),
// combined by two quad shuffles
__device__ __forceinline__ void minv_rows_quad(const double* Mg, const int k, const double* bp, double* ys, const int tid)
{
    const int part = tid & 3;
    for (int q = tid >> 2; q < k; q += 64) {
        double a = 0.0;
        int p = part;
        for (; p + 12 <= q; p += 16) {
            const double m0 = Mg[q + (size_t)p * k], m1 = Mg[q + (size_t)(p + 4) * k], m2 = Mg[q + (size_t)(p + 8) * k], m3 = Mg[q + (size_t)(p + 12) * k];
            a += m0 * bp[p] + m1 * bp[p + 4] + m2 * bp[p + 8] + m3 * bp[p + 12];
        }
        for (; p <= q; p += 4) a += Mg[q + (size_t)p * k] * bp[p];
        a += __shfl_xor(a, 1); a += __shfl_xor(a, 2);
        if (part == 0) ys[q] = a;
    }
}
// x = P^T L11^{-T} ws, written un-permuted to xw: x_p = sum_{q >= p} Minv(q,p) w_q, 4 threads per column (contiguous quarter-interleaved walk), combined by shuffles
__device__ __forceinline__ void minv_cols_quad(const DevView& V, const double* Mg, const int c0, const int k, const double* ws, const int tid)
{
    const int part = tid & 3;
    for (int p = tid >> 2; p < k; p += 64) {
        double a = 0.0;
        int q = p + part;
        for (; q + 12 < k; q += 16) {
            const double m0 = Mg[q + (size_t)p * k], m1 = Mg[q + 4 + (size_t)p * k], m2 = Mg[q + 8 + (size_t)p * k], m3 = Mg[q + 12 + (size_t)p * k];
            a += m0 * ws[q] + m1 * ws[q + 4] + m2 * ws[q + 8] + m3 * ws[q + 12];
        }
        for (; q < k; q += 4) a += Mg[q + (size_t)p * k] * ws[q];
        a += __shfl_xor(a, 1); a += __shfl_xor(a, 2);
        if (part == 0) V.xw[c0 + V.lperm[c0 + p]] = a;
    }
}
// The 16-entry register forms of the two (k <= 64): thread (row, part) holds entries part, part + 4, ... of row `row` of the inverse (columns <= row),
// thread (col, part) the entries col + part, col + part + 4, ... of column `col` (rows < k); zeros elsewhere.
__device__ __forceinline__ void ld_minv_row16(double (&mreg)[16], const double* Mg, const int k, const int tid)
{
    const int row = (tid >> 2) & 63, part = tid & 3;
#pragma unroll
    for (int u = 0; u < 16; ++u) { const int p = part + 4 * u; mreg[u] = (row < k && p <= row) ? Mg[row + (size_t)p * k] : 0.0; }      // Minv(row, p)
}
__device__ __forceinline__ void ld_minv_col16(double (&mreg)[16], const double* Mg, const int k, const int col, const int part)
{
#pragma unroll
    for (int u = 0; u < 16; ++u) { const int q = col + part + 4 * u; mreg[u] = (col < k && q < k) ? Mg[q + (size_t)col * k] : 0.0; }      // Minv(q, col), q >= col
}
// Their product with the 64-entry LDS vector x, entry u against x[(o + 4 u) mod 64] (every entry of x must be a number: zeros of v meet it).  TWO shapes,
// different bits, and each kernel keeps its own: the level kernels (k_fwd_solo64, k_bwd_fin64) sum in one accumulator and combine the quad by shuffles;
// the chain sweeps (k_fwd_chain, k_bwd_chain: the steps along the chain and the final solve) sum the even and the odd entries apart, and combine by DPP
// where they use the sum (quad_sum_dpp).
__device__ __forceinline__ double quad_dot16(const double (&v)[16], const double* x, const int o)
{
    double a = 0.0;
#pragma unroll
    for (int u = 0; u < 16; ++u) a += v[u] * x[(o + 4 * u) & 63];
    a += __shfl_xor(a, 1); a += __shfl_xor(a, 2);
    return a;
}
__device__ __forceinline__ void quad_dot16_eo(const double (&v)[16], const double* x, const int o, double& a0, double& a1)
{
    a0 = 0.0; a1 = 0.0;
#pragma unroll
    for (int u = 0; u < 16; u += 2) { a0 += v[u] * x[(o + 4 * u) & 63]; a1 += v[u + 1] * x[(o + 4 * u + 4) & 63]; }
}
__device__ __forceinline__ double quad_sum_dpp(double t) { t += dpp_f64<0xB1>(t); t += dpp_f64<0x4E>(t); return t; }      // the 4 lanes of a row / column are a DPP quad
// the sum over the nch row blocks of the partial sums of column col (rows of gcols entries), in four accumulators
__device__ __forceinline__ double part_sum4(const double* part, const int nch, const int gcols, const int col)
{
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
    int c = 0;
    for (; c + 3 < nch; c += 4) { t0 += part[(size_t)c * gcols + col]; t1 += part[(size_t)(c + 1) * gcols + col];
                                  t2 += part[(size_t)(c + 2) * gcols + col]; t3 += part[(size_t)(c + 3) * gcols + col]; }
    for (; c < nch; ++c) t0 += part[(size_t)c * gcols + col];
    return (t0 + t1) + (t2 + t3);
}
// 64 update rows per workgroup of 256 (one per lane, Lg: the lane's row of the panel), the k columns dealt to the 4 wavefronts in blocks of 8 (8 coalesced
// loads in flight per lane): t0 += over the even, t1 += over the odd columns of this wavefront's blocks.  The 4 wavefronts' t0 + t1 go to red[wave][lane]
// and are combined in fixed order (red4).
__device__ __forceinline__ void upd_row_acc(const double* Lg, const int ldp, const int k, const double* y, const int wave, double& t0, double& t1)
{
    for (int p = wave * 8; p < k; p += 32) {
        double l[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) l[u] = (p + u < k) ? Lg[(size_t)(p + u) * ldp] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; u += 2) { t0 += l[u] * ((p + u < k) ? y[p + u] : 0.0); t1 += l[u + 1] * ((p + u + 1 < k) ? y[p + u + 1] : 0.0); }
    }
}
__device__ __forceinline__ double red4(const double (&red)[4][64], const int lane) { return (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]); }

// forward: y = L11^{-1} P b for the pivot rows (a k x k mat-vec with the stored inverse: no substitution chain),
// z = D^{-1} y, and the contribution  c = (children) - L21 y  for the ancestors is left in cvec (the parent
// gathers it: no atomics, deterministic).  One workgroup per front of order <= 128 (BIG fronts: k_fwd_grp).
template <int NT>
__global__ __launch_bounds__(NT) void k_fwd(DevView V, int list_off, int top_mode)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x;
    const FrontMeta M = V.fmeta[list_off + blockIdx.x];
    const int c0 = M.c0, k = M.k, m = M.m;
    double* xp = reinterpret_cast<double*>(smem_raw);   // k   pivot rows (original local order)
    double* ys = xp + k;                                // k
    double* bp = ys + k;                                // k   pivot rows in pivot order
    double* xu = bp + k;                                // m-k update-row accumulators (LDS classes only)
    for (int i = tid; i < k; i += NT) xp[i] = V.xw[c0 + i];
    for (int i = k + tid; i < m; i += NT) xu[i - k] = 0.0;
    if (top_mode && V.top_rhs) {
        const double* tr = V.top_rhs + V.top_rhs_off[M.s];
        __syncthreads();
        for (int i = tid; i < m; i += NT) { if (i < k) xp[i] += tr[i]; else xu[i - k] += tr[i]; }
    }
    __syncthreads();
    for (int cp = M.ch0; cp < M.ch1; ++cp) {
        const ChildMeta Cm = V.cmeta[cp];
        if (top_mode && V.top_rhs && Cm.owner >= 0) continue;
        const int base = Cm.relbase, mc = Cm.mc;
        for (int t = tid; t < mc; t += NT) {
            const int tg = V.rel[base + t]; const double v = V.cvec[Cm.cvbase + t];
            if (tg < k) xp[tg] += v; else xu[tg - k] += v;
        }
        __syncthreads();
    }
    // y = Minv * (P b): thread j, independent (pipelined) loads down row j of the column-major inverse
    const double* Mg = V.minv + M.minv_off;
    for (int j = tid; j < k; j += NT) bp[j] = xp[V.lperm[c0 + j]];
    __syncthreads();
    for (int j = tid; j < k; j += NT) {
        double a0 = 0.0, a1 = 0.0;
        int p = 0;
        for (; p + 1 <= j; p += 2) { a0 += Mg[j + (size_t)p * k] * bp[p]; a1 += Mg[j + (size_t)(p + 1) * k] * bp[p + 1]; }
        if (p <= j) a0 += Mg[j + (size_t)p * k] * bp[p];
        ys[j] = a0 + a1;
    }
    __syncthreads();
    {
        const double* Lg = V.L + M.panel_off;
        for (int i = k + tid; i < m; i += NT) {
            double t0 = 0.0, t1 = 0.0;
            int j = 0;
            for (; j + 1 < k; j += 2) { t0 += Lg[i + (size_t)j * M.ldp] * ys[j]; t1 += Lg[i + (size_t)(j + 1) * M.ldp] * ys[j + 1]; }
            if (j < k) t0 += Lg[i + (size_t)j * M.ldp] * ys[j];
            V.cvec[M.cv + i] = xu[i - k] - (t0 + t1);
        }
    }
    for (int j = tid; j < k; j += NT) {
        const int pt = V.ptype[c0 + j];
        double z;
        if (pt == 1) z = ys[j] * V.dinv[c0 + j];
        else if (pt == 2) z = V.dinv[c0 + j] * ys[j] + V.doff[c0 + j] * ys[j + 1];
        else z = V.doff[c0 + j - 1] * ys[j - 1] + V.dinv[c0 + j] * ys[j];
        V.zb[c0 + j] = z;
    }
}

// backward: x_piv = P^T L11^{-T} ( z - L21^T x_upd ), written un-permuted
template <int NT>
__global__ __launch_bounds__(NT) void k_bwd(DevView V, int list_off)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NW = NT / 64;
    const FrontMeta M = V.fmeta[list_off + blockIdx.x];
    const int c0 = M.c0, k = M.k, r0 = M.r0, m = M.m;
    double* ws = reinterpret_cast<double*>(smem_raw);   // k
    double* xu = ws + k;                                // m-k gathered ancestor values (LDS classes)
    for (int i = k + tid; i < m; i += NT) xu[i - k] = V.xw[V.sn_rows[r0 + i]];
    for (int j = tid; j < k; j += NT) ws[j] = V.zb[c0 + j];
    __syncthreads();
    {
        const double* Lg = V.L + M.panel_off;
        for (int j = wave; j < k; j += NW) {
            double t = 0.0;
            for (int i = lane; i < m - k; i += 64) t += Lg[k + i + (size_t)j * M.ldp] * xu[i];
            t = wave_sum(t);
            if (lane == 0) ws[j] -= t;
        }
    }
    __syncthreads();
    // x_p = sum_{j >= p} Minv(j,p) w_j : thread p walks its own (contiguous) column of the inverse
    const double* Mg = V.minv + M.minv_off;
    for (int p = tid; p < k; p += NT) {
        double a0 = 0.0, a1 = 0.0;
        int j = p;
        for (; j + 1 < k; j += 2) { a0 += Mg[j + (size_t)p * k] * ws[j]; a1 += Mg[j + 1 + (size_t)p * k] * ws[j + 1]; }
        if (j < k) a0 += Mg[j + (size_t)p * k] * ws[j];
        V.xw[c0 + V.lperm[c0 + p]] = a0 + a1;
    }
}

// ------------------------------------------------------------------------------------------------
// Fronts of order 33..128 on the level launches of the single-GPU schedule (MI355X_KKT_DISABLE=mid_solve: k_fwd / k_bwd above): the arithmetic of
// k_fwd / k_bwd, entry by entry in the same order (same bits), with the loads batched.  Everything whose address the front record gives -- pivot order,
// D, the first MID_KB columns of the row of L11^{-1} and of the panel rows a thread owns, the child records -- is requested before anything is waited
// for, then the children's vectors (forward) / the ancestors' entries (backward), then arithmetic: three dependent memory phases for a front of
// k <= MID_KB pivots (98 % of them on the tree levels below the chains), one more per further MID_KB columns, instead of one per two to four entries.
// A guarded entry of a batch is loaded from a clamped address inside the same array and dropped by a select on the RESULT of its fma: no branch and no
// wait per element, and the accumulator keeps its bits (the sign of a zero included).  ONE WAVEFRONT PER FRONT -- a workgroup of 256 threads per front
// of order 65..128, as k_fwd<256> has it, was measured slower (1.99 against 1.85 ms per solve of synth_1e6; k_fwd / k_bwd: 2.05) --, MR = rows of the
// front per lane (1: order <= 64, 2: order <= 128); k <= MID_KMAX (solve_level asks for it: the 128-column panels of the wide_panels option stay with
// k_fwd / k_bwd).
// ------------------------------------------------------------------------------------------------
constexpr int MID_KB = 16, MID_KMAX = 64;      // columns per batch; the pivot count these kernels take (max_sn_cols: a thread owns ONE pivot row / column)
// batch pb of row j of the inverse (forward: columns p <= j) / of column j (backward: rows j + q), batch jb of panel row i
__device__ __forceinline__ void mid_ld_mrow(double (&mv)[MID_KB], const double* Mg, const int k, const int j, const int pb)
{
#pragma unroll
    for (int p = 0; p < MID_KB; ++p) { const bool ok = j < k && pb + p <= j; mv[p] = Mg[ok ? j + (size_t)(pb + p) * k : 0]; }
}
__device__ __forceinline__ void mid_ld_mcol(double (&mv)[MID_KB], const double* Mg, const int k, const int p, const int qb)
{
#pragma unroll
    for (int q = 0; q < MID_KB; ++q) { const bool ok = p + qb + q < k; mv[q] = Mg[ok ? p + qb + q + (size_t)p * k : 0]; }
}
__device__ __forceinline__ void mid_ld_lrow(double (&lv)[MID_KB], const double* Lg, const int k, const int m, const int ldp, const int i, const int jb)
{
#pragma unroll
    for (int p = 0; p < MID_KB; ++p) { const bool ok = i < m && jb + p < k; lv[p] = Lg[ok ? i + (size_t)(jb + p) * ldp : 0]; }
}
// a0 += over the even, a1 += over the odd entries q < n of a batch (ascending); x: the LDS vector from the batch's first entry on (readable MID_KB entries past its end)
__device__ __forceinline__ void mid_acc(const double (&v)[MID_KB], const double* x, const int n, double& a0, double& a1)
{
#pragma unroll
    for (int q = 0; q < MID_KB; q += 2) {
        const double f0 = fma(v[q], x[q], a0), f1 = fma(v[q + 1], x[q + 1], a1);
        a0 = q < n ? f0 : a0; a1 = q + 1 < n ? f1 : a1;
    }
}

// BLOCKS OF RIGHT-HAND SIDES (the solve-block path of numeric.hip): the bodies below take NC columns through a front together.  What the front record
// gives -- pivot order, D, the rows and columns of L11^{-1} and of the panel, the child records, the targets rel[...] -- is loaded once; per column there
// are its entries of xw / zb / cvec (column c at c * sx / c * sx / c * scv doubles behind column 0), its slice of the LDS vectors and its accumulators.
// Per column the operations and their order are those of one column (the kernels of one column ARE the NC = 1 instantiation); nc <= NC columns are
// active (uniform over the launch), the others are neither read, written nor multiplied in.
#define RB_ON(c) (NC == 1 || (c) < nc)
template <int MR, int NC>
__device__ __forceinline__ void fwd_mid_front(const DevView& V, const int list_off, const int nc, const size_t sx, const size_t scv)
{
    __shared__ double xp[NC][MID_KMAX], ys[NC][MID_KMAX + MID_KB], bp[NC][MID_KMAX + MID_KB], xu[NC][128];
    const int tid = threadIdx.x;
    const FrontMeta M = V.fmeta[list_off + blockIdx.x];
    const int c0 = M.c0, k = M.k, m = M.m, ldp = M.ldp, ch0 = M.ch0, ch1 = M.ch1;
    const double* Mg = V.minv + M.minv_off;
    const double* Lg = V.L + M.panel_off;
    // ---- phase 1: the front record gives every address.  The child records first (what phase 2 waits for): lane c of every wavefront loads child c's ----
    const int nch = ch1 - ch0 < 4 ? ch1 - ch0 : 4;
    int mcl = 0, rbl = 0; long long cbl = 0;
    if (nch > 0) { const ChildMeta* Cl = V.cmeta + ch0 + ((tid & 3) < nch ? (tid & 3) : nch - 1); mcl = Cl->mc; rbl = Cl->relbase; cbl = Cl->cvbase; }
    const bool piv = tid < k;
    const int jc = piv ? tid : 0;
    double xwv[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) if (RB_ON(c)) xwv[c] = V.xw[c * sx + (c0 + jc)];
    const int lpv = V.lperm[c0 + jc];
    double mrow[MID_KB], lrow[MR][MID_KB];
    mid_ld_mrow(mrow, Mg, k, tid, 0);
#pragma unroll
    for (int r = 0; r < MR; ++r) mid_ld_lrow(lrow[r], Lg, k, m, ldp, k + tid + 64 * r, 0);
    const int pt = V.ptype[c0 + jc];
    const double dq = V.dinv[c0 + jc], oq = V.doff[c0 + jc], oq1 = V.doff[c0 + (jc > 0 ? jc - 1 : 0)];
    // ---- phase 2: the children's contribution vectors (the first four children's in one batch) ----
    int tg[4][MR]; double cv[NC][4][MR];
    if (nch > 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {      // (lanes c >= nch hold the last child's record again: valid addresses, no entry taken)
            const int mc = c < nch ? __builtin_amdgcn_readlane(mcl, c) : 0, rb = __builtin_amdgcn_readlane(rbl, c);
            const long long cb = ((long long)__builtin_amdgcn_readlane((int)(cbl >> 32), c) << 32) | (unsigned)__builtin_amdgcn_readlane((int)cbl, c);
#pragma unroll
            for (int r = 0; r < MR; ++r) {
                const int t = tid + 64 * r; const bool on = t < mc;
                const int g = V.rel[rb + (on ? t : 0)];
#pragma unroll
                for (int col = 0; col < NC; ++col) if (RB_ON(col)) cv[col][c][r] = V.cvec[col * scv + (cb + (on ? t : 0))];
                tg[c][r] = on ? g : -1;
            }
        }
    }
    // ---- phase 3: arithmetic ----
#pragma unroll
    for (int col = 0; col < NC; ++col) if (RB_ON(col)) {
        if (piv) xp[col][tid] = xwv[col];
        for (int i = k + tid; i < m; i += 64) xu[col][i - k] = 0.0;
    }
    __syncthreads();
    if (nch > 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int r = 0; r < MR; ++r) {
                const int g = tg[c][r];
                if (g >= 0) {
#pragma unroll
                    for (int col = 0; col < NC; ++col) if (RB_ON(col)) { if (g < k) xp[col][g] += cv[col][c][r]; else xu[col][g - k] += cv[col][c][r]; }
                }
            }
            __syncthreads();
        }
        for (int cp = ch0 + 4; cp < ch1; ++cp) {                 // (more than four children: rare)
            const ChildMeta Cm = V.cmeta[cp];
            for (int t = tid; t < Cm.mc; t += 64) {
                const int g = V.rel[Cm.relbase + t];
#pragma unroll
                for (int col = 0; col < NC; ++col) if (RB_ON(col)) {
                    const double v = V.cvec[col * scv + (Cm.cvbase + t)];
                    if (g < k) xp[col][g] += v; else xu[col][g - k] += v;
                }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int col = 0; col < NC; ++col) if (RB_ON(col)) { if (piv) bp[col][tid] = xp[col][lpv]; }
    __syncthreads();
    {   // y = Minv * (P b): thread j walks row j of the column-major inverse, even and odd columns p <= j apart
        double a0[NC], a1[NC];
#pragma unroll
        for (int col = 0; col < NC; ++col) if (RB_ON(col)) { a0[col] = 0.0; a1[col] = 0.0; mid_acc(mrow, bp[col], tid + 1, a0[col], a1[col]); }
        for (int pb = MID_KB; pb < k; pb += MID_KB) {
            double mv[MID_KB]; mid_ld_mrow(mv, Mg, k, tid, pb);
#pragma unroll
            for (int col = 0; col < NC; ++col) if (RB_ON(col)) mid_acc(mv, bp[col] + pb, tid + 1 - pb, a0[col], a1[col]);
        }
#pragma unroll
        for (int col = 0; col < NC; ++col) if (RB_ON(col)) { if (piv) ys[col][tid] = a0[col] + a1[col]; }
    }
    __syncthreads();
    {   // c = (children) - L21 y: a thread's rows, even and odd columns apart
        double t0[NC][MR], t1[NC][MR];
#pragma unroll
        for (int col = 0; col < NC; ++col) if (RB_ON(col)) {
#pragma unroll
            for (int r = 0; r < MR; ++r) { t0[col][r] = 0.0; t1[col][r] = 0.0; mid_acc(lrow[r], ys[col], k, t0[col][r], t1[col][r]); }
        }
        for (int jb = MID_KB; jb < k; jb += MID_KB) {
            double lv[MR][MID_KB];
#pragma unroll
            for (int r = 0; r < MR; ++r) mid_ld_lrow(lv[r], Lg, k, m, ldp, k + tid + 64 * r, jb);
#pragma unroll
            for (int col = 0; col < NC; ++col) if (RB_ON(col)) {
#pragma unroll
                for (int r = 0; r < MR; ++r) mid_acc(lv[r], ys[col] + jb, k - jb, t0[col][r], t1[col][r]);
            }
        }
#pragma unroll
        for (int col = 0; col < NC; ++col) if (RB_ON(col)) {
#pragma unroll
            for (int r = 0; r < MR; ++r) { const int i = k + tid + 64 * r; if (i < m) V.cvec[col * scv + (M.cv + i)] = xu[col][i - k] - (t0[col][r] + t1[col][r]); }
        }
    }
    if (piv) {
        const int j = tid;
#pragma unroll
        for (int col = 0; col < NC; ++col) if (RB_ON(col)) {
            double z;
            if (pt == 1) z = ys[col][j] * dq;
            else if (pt == 2) z = fma(dq, ys[col][j], oq * ys[col][j + 1]);      // (the fma is spelled out: see PivD)
            else z = fma(oq1, ys[col][j - 1], dq * ys[col][j]);
            V.zb[col * sx + (c0 + j)] = z;
        }
    }
}
// The forward kernel of ONE column stays as it was written, beside fwd_mid_front: as fwd_mid_front<MR, 1> the same statements took 114 instead of 99 VGPRs
// for MR = 1 (the allocator spills fewer SGPRs and keeps more vector registers; every other one-column kernel of this file IS the NC = 1 instantiation of
// its body, within two VGPRs of what it took before).  What holds the two together: tests/test_gpu_solve_block.py asks every column of a block for the
// bits of a solve of its own.
template <int MR>
__global__ __launch_bounds__(64) void k_fwd_mid(DevView V, int list_off)
{
    __shared__ double xp[MID_KMAX], ys[MID_KMAX + MID_KB], bp[MID_KMAX + MID_KB], xu[128];
    const int tid = threadIdx.x;
    const FrontMeta M = V.fmeta[list_off + blockIdx.x];
    const int c0 = M.c0, k = M.k, m = M.m, ldp = M.ldp, ch0 = M.ch0, ch1 = M.ch1;
    const double* Mg = V.minv + M.minv_off;
    const double* Lg = V.L + M.panel_off;
    // ---- phase 1: the front record gives every address.  The child records first (what phase 2 waits for): lane c of every wavefront loads child c's ----
    const int nch = ch1 - ch0 < 4 ? ch1 - ch0 : 4;
    int mcl = 0, rbl = 0; long long cbl = 0;
    if (nch > 0) { const ChildMeta* Cl = V.cmeta + ch0 + ((tid & 3) < nch ? (tid & 3) : nch - 1); mcl = Cl->mc; rbl = Cl->relbase; cbl = Cl->cvbase; }
    const bool piv = tid < k;
    const int jc = piv ? tid : 0;
    const double xwv = V.xw[c0 + jc];
    const int lpv = V.lperm[c0 + jc];
    double mrow[MID_KB], lrow[MR][MID_KB];
    mid_ld_mrow(mrow, Mg, k, tid, 0);
#pragma unroll
    for (int r = 0; r < MR; ++r) mid_ld_lrow(lrow[r], Lg, k, m, ldp, k + tid + 64 * r, 0);
    const int pt = V.ptype[c0 + jc];
    const double dq = V.dinv[c0 + jc], oq = V.doff[c0 + jc], oq1 = V.doff[c0 + (jc > 0 ? jc - 1 : 0)];
    // ---- phase 2: the children's contribution vectors (the first four children's in one batch) ----
    int tg[4][MR]; double cv[4][MR];
    if (nch > 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {      // (lanes c >= nch hold the last child's record again: valid addresses, no entry taken)
            const int mc = c < nch ? __builtin_amdgcn_readlane(mcl, c) : 0, rb = __builtin_amdgcn_readlane(rbl, c);
            const long long cb = ((long long)__builtin_amdgcn_readlane((int)(cbl >> 32), c) << 32) | (unsigned)__builtin_amdgcn_readlane((int)cbl, c);
#pragma unroll
            for (int r = 0; r < MR; ++r) {
                const int t = tid + 64 * r; const bool on = t < mc;
                const int g = V.rel[rb + (on ? t : 0)]; cv[c][r] = V.cvec[cb + (on ? t : 0)];
                tg[c][r] = on ? g : -1;
            }
        }
    }
    // ---- phase 3: arithmetic ----
    if (piv) xp[tid] = xwv;
    for (int i = k + tid; i < m; i += 64) xu[i - k] = 0.0;
    __syncthreads();
    if (nch > 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int r = 0; r < MR; ++r) { const int g = tg[c][r]; if (g >= 0) { if (g < k) xp[g] += cv[c][r]; else xu[g - k] += cv[c][r]; } }
            __syncthreads();
        }
        for (int cp = ch0 + 4; cp < ch1; ++cp) {                 // (more than four children: rare)
            const ChildMeta Cm = V.cmeta[cp];
            for (int t = tid; t < Cm.mc; t += 64) {
                const int g = V.rel[Cm.relbase + t]; const double v = V.cvec[Cm.cvbase + t];
                if (g < k) xp[g] += v; else xu[g - k] += v;
            }
            __syncthreads();
        }
    }
    if (piv) bp[tid] = xp[lpv];
    __syncthreads();
    {   // y = Minv * (P b): thread j walks row j of the column-major inverse, even and odd columns p <= j apart
        double a0 = 0.0, a1 = 0.0;
        mid_acc(mrow, bp, tid + 1, a0, a1);
        for (int pb = MID_KB; pb < k; pb += MID_KB) { double mv[MID_KB]; mid_ld_mrow(mv, Mg, k, tid, pb); mid_acc(mv, bp + pb, tid + 1 - pb, a0, a1); }
        if (piv) ys[tid] = a0 + a1;
    }
    __syncthreads();
    {   // c = (children) - L21 y: a thread's rows, even and odd columns apart
        double t0[MR], t1[MR];
#pragma unroll
        for (int r = 0; r < MR; ++r) { t0[r] = 0.0; t1[r] = 0.0; mid_acc(lrow[r], ys, k, t0[r], t1[r]); }
        for (int jb = MID_KB; jb < k; jb += MID_KB) {
            double lv[MR][MID_KB];
#pragma unroll
            for (int r = 0; r < MR; ++r) mid_ld_lrow(lv[r], Lg, k, m, ldp, k + tid + 64 * r, jb);
#pragma unroll
            for (int r = 0; r < MR; ++r) mid_acc(lv[r], ys + jb, k - jb, t0[r], t1[r]);
        }
#pragma unroll
        for (int r = 0; r < MR; ++r) { const int i = k + tid + 64 * r; if (i < m) V.cvec[M.cv + i] = xu[i - k] - (t0[r] + t1[r]); }
    }
    if (piv) {
        const int j = tid;
        double z;
        if (pt == 1) z = ys[j] * dq;
        else if (pt == 2) z = fma(dq, ys[j], oq * ys[j + 1]);      // (the fma is spelled out: see PivD)
        else z = fma(oq1, ys[j - 1], dq * ys[j]);
        V.zb[c0 + j] = z;
    }
}
template <int MR> __global__ __launch_bounds__(64) void k_fwd_mid_rb(DevView V, int list_off, int nc, size_t sx, size_t scv) { fwd_mid_front<MR, SOLVE_RB>(V, list_off, nc, sx, scv); }

// backward: MID_KB columns per batch, rows lane and lane + 64 (MR = 2) of each per lane
template <int MR, int NC>
__device__ __forceinline__ void bwd_mid_front(const DevView& V, const int list_off, const int nc, const size_t sx)
{
    __shared__ double ws[NC][MID_KMAX + MID_KB], xu[NC][128];
    const int tid = threadIdx.x, lane = tid;
    const FrontMeta M = V.fmeta[list_off + blockIdx.x];
    const int c0 = M.c0, k = M.k, r0 = M.r0, m = M.m, ldp = M.ldp, nu = m - k;
    const double* Mg = V.minv + M.minv_off;
    const double* Lg = V.L + M.panel_off;
    // ---- phase 1 ----
    int ridx[MR];
#pragma unroll
    for (int r = 0; r < MR; ++r) { const int i = lane + 64 * r; ridx[r] = V.sn_rows[r0 + (i < nu ? k + i : 0)]; }
    const bool piv = tid < k;
    const int jc = piv ? tid : 0;
    double zbv[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) if (RB_ON(c)) zbv[c] = V.zb[c * sx + (c0 + jc)];
    double lcol[MID_KB][MR];
#pragma unroll
    for (int q = 0; q < MID_KB; ++q)
#pragma unroll
        for (int r = 0; r < MR; ++r) { const int j = q, i = lane + 64 * r; const bool ok = j < k && i < nu; lcol[q][r] = Lg[ok ? k + i + (size_t)j * ldp : 0]; }
    double mcol[MID_KB];
    mid_ld_mcol(mcol, Mg, k, tid, 0);
    const int lpv = V.lperm[c0 + jc];
    // ---- phase 2: the ancestors' solution entries (the fence keeps the scheduler from drawing the gather, and its wait, in front of the batch) ----
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < NC; ++c) if (RB_ON(c)) {
#pragma unroll
        for (int r = 0; r < MR; ++r) xu[c][lane + 64 * r] = V.xw[c * sx + ridx[r]];      // (unconditional: rows >= nu hold the front's first row again and are never read)
    }
    // ---- phase 3 ----
#pragma unroll
    for (int c = 0; c < NC; ++c) if (RB_ON(c)) ws[c][piv ? tid : MID_KMAX + MID_KB - 1] = zbv[c];      // (unconditional: a store under `piv` draws the load into the branch, behind the gather)
    __syncthreads();
#pragma unroll
    for (int q = 0; q < MID_KB; ++q) {
        const int j = q;
#pragma unroll
        for (int c = 0; c < NC; ++c) if (RB_ON(c)) {
            double t = 0.0;
#pragma unroll
            for (int r = 0; r < MR; ++r) { const int i = lane + 64 * r; const double f = fma(lcol[q][r], xu[c][i], t); t = i < nu ? f : t; }
            t = wave_sum(t);
            if (lane == 0 && j < k) ws[c][j] -= t;
        }
    }
    for (int jb = MID_KB; jb < k; jb += MID_KB) {
        double lv[MID_KB][MR];
#pragma unroll
        for (int q = 0; q < MID_KB; ++q)
#pragma unroll
            for (int r = 0; r < MR; ++r) { const int j = jb + q, i = lane + 64 * r; const bool ok = j < k && i < nu; lv[q][r] = Lg[ok ? k + i + (size_t)j * ldp : 0]; }
#pragma unroll
        for (int q = 0; q < MID_KB; ++q) {
            const int j = jb + q;
#pragma unroll
            for (int c = 0; c < NC; ++c) if (RB_ON(c)) {
                double t = 0.0;
#pragma unroll
                for (int r = 0; r < MR; ++r) { const int i = lane + 64 * r; const double f = fma(lv[q][r], xu[c][i], t); t = i < nu ? f : t; }
                t = wave_sum(t);
                if (lane == 0 && j < k) ws[c][j] -= t;
            }
        }
    }
    __syncthreads();
    {   // x_p = sum_{j >= p} Minv(j,p) w_j: thread p walks its own column of the inverse, rows p, p + 2, ... and p + 1, p + 3, ... apart
        double a0[NC], a1[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) if (RB_ON(c)) { a0[c] = 0.0; a1[c] = 0.0; mid_acc(mcol, ws[c] + jc, k - tid, a0[c], a1[c]); }
        for (int qb = MID_KB; qb < k; qb += MID_KB) {
            double mv[MID_KB]; mid_ld_mcol(mv, Mg, k, tid, qb);
#pragma unroll
            for (int c = 0; c < NC; ++c) if (RB_ON(c)) mid_acc(mv, ws[c] + (piv ? tid + qb < k ? tid + qb : 0 : 0), k - tid - qb, a0[c], a1[c]);
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) if (RB_ON(c)) { if (piv) V.xw[c * sx + (c0 + lpv)] = a0[c] + a1[c]; }
    }
}
template <int MR> __global__ __launch_bounds__(64) void k_bwd_mid(DevView V, int list_off) { bwd_mid_front<MR, 1>(V, list_off, 1, 0); }
template <int MR> __global__ __launch_bounds__(64) void k_bwd_mid_rb(DevView V, int list_off, int nc, size_t sx) { bwd_mid_front<MR, SOLVE_RB>(V, list_off, nc, sx); }


// ------------------------------------------------------------------------------------------------
// Fronts of order <= 32 (the LukVl regime: 10^5..10^6 of them per sweep): TWO fronts per wavefront (one per half: a front of
// order <= 32 leaves half a wavefront idle) and three dependent memory phases instead of seven -- everything that only depends on
// the front record (pivot order, D, the row of L11^{-1} and the panel row / column a lane owns) is loaded up front into registers,
// then the children's contributions (forward) or the ancestors' solution entries (backward), then arithmetic.  The sweeps are
// bound by (dependent round trips) x (fronts / resident wavefronts), not by bytes.  KP = compile-time bound on the pivot count.
// ------------------------------------------------------------------------------------------------
// The body of ONE front on its LPF lanes (lane li; xs, bp, ys, xus, w: the front's rows of the LDS arrays), called once per front by the pair kernels and
// once per link by the leaf chains (k_fwd_leafchain / k_bwd_leafchain): one definition, so the two agree bit for bit.  The gather of the children between
// the forward phases stays with each kernel: four children from memory there, one from LDS here.  So do the three guarded loads that open phase 1 (the
// lane's right-hand side entry, pivot position and D): written out in the kernel they stay three branches, out of a shared function the compiler merges
// them into one, which costs k_fwd_pair two registers.
// forward, phase 1: the lane's row of L11^{-1} (a pivot lane) or of the panel (an update lane)
template <int KP>
__device__ __forceinline__ void small_ld_rows(double (&mrow)[KP], double (&lrow)[KP], const double* Mg, const double* Lg, const int k, const int m, const int ldp, const int li)
{
    const bool piv = li < k, upd = li >= k && li < m;
#pragma unroll
    for (int p = 0; p < KP; ++p) {
        mrow[p] = (piv && p <= li) ? Mg[li + (size_t)p * k] : 0.0;
        lrow[p] = (upd && p < k) ? Lg[li + (size_t)p * ldp] : 0.0;
    }
}
// forward, phase 3, behind the gather into xs: y (returned, and left in ys), the update row's  xs - L21 y  handed to put(value) on the update lanes.
// z = D^{-1} y stays with each kernel, as every kernel's does (see PivD).
// NC columns (see RB_ON): column c's rows of the LDS arrays lie CS (xs, bp) / CSY (ys) doubles behind column 0's; y[c] is returned per column, put(c, value)
template <int KP, int LPF, int NC, int CS, int CSY, class Put>
__device__ __forceinline__ void small_fwd_solve(const int k, const int m, const int li, const int lpv, const double (&mrow)[KP], const double (&lrow)[KP], const double* xs, double* bp, double* ys, const int nc, double (&y)[NC], Put put)
{
    const bool piv = li < k, upd = li >= k && li < m;
#pragma unroll
    for (int c = 0; c < NC; ++c) if (RB_ON(c)) bp[c * CS + li] = piv ? xs[c * CS + lpv] : 0.0;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NC; ++c) if (RB_ON(c)) {
        double yc = 0.0;
#pragma unroll
        for (int p = 0; p < KP; ++p) yc += mrow[p] * bp[c * CS + p];
        ys[c * CSY + li] = piv ? yc : 0.0;
        if (li == 0) ys[c * CSY + LPF] = 0.0;
        y[c] = yc;
    }
    __syncthreads();
    if (upd) {
#pragma unroll
        for (int c = 0; c < NC; ++c) if (RB_ON(c)) {
            double t = 0.0;
#pragma unroll
            for (int p = 0; p < KP; ++p) t += lrow[p] * ys[c * CSY + p];
            put(c, xs[c * CS + li] - t);
        }
    }
}
// backward, all three phases: the front record's loads, the ancestors' solution entries, arithmetic
template <int KP, int LPF, int NC, int CS, class Rec>      // NC columns (see RB_ON): column c's rows of xus and w lie CS doubles behind column 0's
__device__ __forceinline__ void small_bwd(const DevView& V, const Rec& R, const int k, const int m, const int li, double* xus, double* w, const int nc, const size_t sx)
{
    const int c0 = R.c0, r0 = R.r0, ldp = R.ldp;
    const bool piv = li < k, upd = li >= k && li < m;
    // ---- phase 1 ----
    double zbv[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) if (RB_ON(c)) zbv[c] = piv ? V.zb[c * sx + (c0 + li)] : 0.0;
    const int lpv = piv ? V.lperm[c0 + li] : 0;
    const int ridx = upd ? V.sn_rows[r0 + li] : 0;
    const double* Mg = V.minv + R.minv_off;
    const double* Lg = V.L + R.panel_off;
    double mcol[KP], lcol[LPF];
#pragma unroll
    for (int q = 0; q < KP; ++q) mcol[q] = (piv && li + q < k) ? Mg[li + q + (size_t)li * k] : 0.0;      // Minv(li + q, li)
#pragma unroll
    for (int i = 0; i < LPF; ++i) lcol[i] = (piv && k + i < m) ? Lg[k + i + (size_t)li * ldp] : 0.0;        // L(k + i, li)
    // ---- phase 2: the ancestors' solution entries ----
#pragma unroll
    for (int c = 0; c < NC; ++c) if (RB_ON(c)) xus[c * CS + li] = upd ? V.xw[c * sx + ridx] : 0.0;
    __syncthreads();
    // ---- phase 3 ----
#pragma unroll
    for (int c = 0; c < NC; ++c) if (RB_ON(c)) {
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < LPF; ++i) t += lcol[i] * xus[c * CS + ((k + i) & (LPF - 1))];
        w[c * CS + li] = piv ? zbv[c] - t : 0.0;
    }
    __syncthreads();
    if (piv) {
#pragma unroll
        for (int c = 0; c < NC; ++c) if (RB_ON(c)) {
            double a = 0.0;
#pragma unroll
            for (int q = 0; q < KP; ++q) a += mcol[q] * w[c * CS + ((li + q) & (LPF - 1))];
            V.xw[c * sx + (c0 + lpv)] = a;
        }
    }
}

template <int KP, int LPF, int NC>      // LPF lanes per front: 32 (order <= 32, two fronts per wavefront) or 16 (levels whose fronts all have order <= 16: four)
__device__ __forceinline__ void fwd_pair_front(const DevView& V, const int list_off, const int nfronts, const int nc, const size_t sx, const size_t scv)
{
    constexpr int FPW = 64 / LPF;
    __shared__ double xs[NC][FPW][LPF], bp[NC][FPW][LPF], ys[NC][FPW][LPF + 1];
    const int lane = threadIdx.x, h = lane / LPF, li = lane % LPF;
    const int f = FPW * (int)blockIdx.x + h;
    const bool act = f < nfronts;
    const FrontMeta* Mp = V.fmeta + list_off + (act ? f : 0);
    const int c0 = Mp->c0, k = act ? Mp->k : 0, m = act ? Mp->m : 0, ch0 = Mp->ch0, ch1 = act ? Mp->ch1 : Mp->ch0, ldp = Mp->ldp;
    const long long cvo = Mp->cv;
    // ---- phase 1: depends on the front record only ----
    const bool piv = li < k;
    double xwv[NC];
#pragma unroll
    for (int col = 0; col < NC; ++col) if (RB_ON(col)) xwv[col] = piv ? V.xw[col * sx + (c0 + li)] : 0.0;
    const int lpv = piv ? V.lperm[c0 + li] : 0;
    const PivD D = ld_pivd(V, c0, li, piv);
    double mrow[KP], lrow[KP];
    small_ld_rows(mrow, lrow, V.minv + Mp->minv_off, V.L + Mp->panel_off, k, m, ldp, li);
    int cmc[4], crel[4]; long long ccv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const bool has = ch0 + c < ch1;
        const ChildMeta* Cp = V.cmeta + ch0 + (has ? c : 0);
        cmc[c] = has ? Cp->mc : 0; crel[c] = Cp->relbase; ccv[c] = Cp->cvbase;
    }
    // ---- phase 2: the children's contribution vectors ----
    int tg[4]; double cv[NC][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const bool on = li < cmc[c]; tg[c] = on ? V.rel[crel[c] + li] : -1;
#pragma unroll
        for (int col = 0; col < NC; ++col) if (RB_ON(col)) cv[col][c] = on ? V.cvec[col * scv + (ccv[c] + li)] : 0.0;
    }
    // ---- phase 3: arithmetic ----
#pragma unroll
    for (int col = 0; col < NC; ++col) if (RB_ON(col)) xs[col][h][li] = xwv[col];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (tg[c] >= 0) {
#pragma unroll
            for (int col = 0; col < NC; ++col) if (RB_ON(col)) xs[col][h][tg[c]] += cv[col][c];
        }
        __syncthreads();
    }
    for (int cp = ch0 + 4; cp < ch1; ++cp) {                 // (more than four children: rare)
        const int mc = V.cmeta[cp].mc;
        if (li < mc) {
#pragma unroll
            for (int col = 0; col < NC; ++col) if (RB_ON(col)) xs[col][h][V.rel[V.cmeta[cp].relbase + li]] += V.cvec[col * scv + (V.cmeta[cp].cvbase + li)];
        }
        __syncthreads();
    }
    double y[NC];
    small_fwd_solve<KP, LPF, NC, FPW * LPF, FPW * (LPF + 1)>(k, m, li, lpv, mrow, lrow, xs[0][h], bp[0][h], ys[0][h], nc, y, [&](const int col, const double r) { V.cvec[col * scv + (cvo + li)] = r; });
    if (piv) {
#pragma unroll
        for (int col = 0; col < NC; ++col) if (RB_ON(col)) {
            double z;
            if (D.pt == 1) z = y[col] * D.dq;
            else if (D.pt == 2) z = fma(D.dq, y[col], D.oq * ys[col][h][li + 1]);      // (the fma is spelled out: see PivD)
            else z = fma(D.dq, y[col], D.oq1 * ys[col][h][li - 1]);
            V.zb[col * sx + (c0 + li)] = z;
        }
    }
}
template <int KP, int LPF = 32> __global__ __launch_bounds__(64) void k_fwd_pair(DevView V, int list_off, int nfronts) { fwd_pair_front<KP, LPF, 1>(V, list_off, nfronts, 1, 0, 0); }
template <int KP, int LPF = 32> __global__ __launch_bounds__(64) void k_fwd_pair_rb(DevView V, int list_off, int nfronts, int nc, size_t sx, size_t scv) { fwd_pair_front<KP, LPF, SOLVE_RB>(V, list_off, nfronts, nc, sx, scv); }
template <int KP, int LPF, int NC>
__device__ __forceinline__ void bwd_pair_front(const DevView& V, const int list_off, const int nfronts, const int nc, const size_t sx)
{
    constexpr int FPW = 64 / LPF;
    __shared__ double xus[NC][FPW][LPF], w[NC][FPW][LPF];
    const int lane = threadIdx.x, h = lane / LPF, li = lane % LPF;
    const int f = FPW * (int)blockIdx.x + h;
    const bool act = f < nfronts;
    const FrontMeta* Mp = V.fmeta + list_off + (act ? f : 0);
    small_bwd<KP, LPF, NC, FPW * LPF>(V, *Mp, act ? Mp->k : 0, act ? Mp->m : 0, li, xus[0][h], w[0][h], nc, sx);
}
template <int KP, int LPF = 32> __global__ __launch_bounds__(64) void k_bwd_pair(DevView V, int list_off, int nfronts) { bwd_pair_front<KP, LPF, 1>(V, list_off, nfronts, 1, 0); }
template <int KP, int LPF = 32> __global__ __launch_bounds__(64) void k_bwd_pair_rb(DevView V, int list_off, int nfronts, int nc, size_t sx) { bwd_pair_front<KP, LPF, SOLVE_RB>(V, list_off, nfronts, nc, sx); }

// ------------------------------------------------------------------------------------------------
// LEAF CHAINS in the sweeps (see k_leaf_chain): a 16-lane row walks its chain -- forward from the leaf up, the contribution vector of a link handed to
// the next one through LDS (only the last link's goes to memory), backward from the top link down (a link reads the entries its ancestors INSIDE the chain
// have just stored: same CU, a barrier in between) -- one launch per sweep for all the levels of the chains.  A link's body is that of a front of
// k_fwd_pair / k_bwd_pair<16, 16>: small_ld_rows, small_fwd_solve, small_bwd.
// ------------------------------------------------------------------------------------------------
template <int NC>
__device__ __forceinline__ void fwd_leafchain_row(const DevView& V, const int nchains, const int nc, const size_t sx, const size_t scv)
{
    constexpr int KP = 16, LPF = 16, FPW = 4;
    __shared__ double xs[NC][FPW][LPF], bp[NC][FPW][LPF], ys[NC][FPW][LPF + 1], cvs[NC][FPW][LPF];
    const int lane = threadIdx.x, h = lane / LPF, li = lane % LPF;
    const int ch = FPW * (int)blockIdx.x + h;
    const bool cact = ch < nchains;
    const int l0 = V.lc_ptr[min(ch, nchains - 1)];
    const int nl = cact ? V.lc_ptr[min(ch, nchains - 1) + 1] - l0 : 0;
    const int nlw = max(max(__builtin_amdgcn_readlane(nl, 0), __builtin_amdgcn_readlane(nl, 16)), max(__builtin_amdgcn_readlane(nl, 32), __builtin_amdgcn_readlane(nl, 48)));
    int kprev = 0, mprev = 0, relprev = 0;
    const LeafLink* Lc = V.lc_link + l0;
    const int nlc = max(nl, 1);
    LeafLink K0 = Lc[0];
#pragma unroll 1
    for (int t = 0; t < nlw; ++t) {
        const bool act = t < nl;
        const LeafLink K1 = Lc[min(t + 1, nlc - 1)];          // (the next link's record: on its way while this link is solved)
        const int c0 = K0.c0, k = act ? K0.k : 0, m = act ? K0.m : 0, ldp = K0.ldp;
        const long long cvo = K0.cv;
        const bool piv = li < k;
        double xwv[NC];
#pragma unroll
        for (int col = 0; col < NC; ++col) if (RB_ON(col)) xwv[col] = piv ? V.xw[col * sx + (c0 + li)] : 0.0;
        const int lpv = piv ? V.lperm[c0 + li] : 0;
        const PivD D = ld_pivd(V, c0, li, piv);
        double mrow[KP], lrow[KP];
        small_ld_rows(mrow, lrow, V.minv + K0.minv_off, V.L + K0.panel_off, k, m, ldp, li);
        // the child (the previous link): its contribution vector is in cvs
        const int mc = (act && t > 0) ? mprev - kprev : 0;
        const int tg = li < mc ? V.rel[relprev + li] : -1;
        double cv[NC];
#pragma unroll
        for (int col = 0; col < NC; ++col) if (RB_ON(col)) { cv[col] = li < mc ? cvs[col][h][li] : 0.0; xs[col][h][li] = xwv[col]; }
        __syncthreads();
        if (tg >= 0) {
#pragma unroll
            for (int col = 0; col < NC; ++col) if (RB_ON(col)) xs[col][h][tg] += cv[col];
        }
        __syncthreads();
        double y[NC];
        small_fwd_solve<KP, LPF, NC, FPW * LPF, FPW * (LPF + 1)>(k, m, li, lpv, mrow, lrow, xs[0][h], bp[0][h], ys[0][h], nc, y,
            [&](const int col, const double r) { cvs[col][h][li - k] = r; if (t == nl - 1) V.cvec[col * scv + (cvo + li)] = r; });
        if (piv) {
#pragma unroll
            for (int col = 0; col < NC; ++col) if (RB_ON(col)) {
                double z;
                if (D.pt == 1) z = y[col] * D.dq;
                else if (D.pt == 2) z = fma(D.dq, y[col], D.oq * ys[col][h][li + 1]);      // (the fma is spelled out: see PivD)
                else z = fma(D.dq, y[col], D.oq1 * ys[col][h][li - 1]);
                V.zb[col * sx + (c0 + li)] = z;
            }
        }
        __syncthreads();
        kprev = k; mprev = m; relprev = K0.relbase;
        K0 = K1;
    }
}
__global__ __launch_bounds__(64) void k_fwd_leafchain(DevView V, int nchains) { fwd_leafchain_row<1>(V, nchains, 1, 0, 0); }
__global__ __launch_bounds__(64) void k_fwd_leafchain_rb(DevView V, int nchains, int nc, size_t sx, size_t scv) { fwd_leafchain_row<SOLVE_RB>(V, nchains, nc, sx, scv); }
template <int NC>
__device__ __forceinline__ void bwd_leafchain_row(const DevView& V, const int nchains, const int nc, const size_t sx)
{
    constexpr int KP = 16, LPF = 16, FPW = 4;
    __shared__ double xus[NC][FPW][LPF], w[NC][FPW][LPF];
    const int lane = threadIdx.x, h = lane / LPF, li = lane % LPF;
    const int ch = FPW * (int)blockIdx.x + h;
    const bool cact = ch < nchains;
    const int l0 = V.lc_ptr[min(ch, nchains - 1)];
    const int nl = cact ? V.lc_ptr[min(ch, nchains - 1) + 1] - l0 : 0;
    const int nlw = max(max(__builtin_amdgcn_readlane(nl, 0), __builtin_amdgcn_readlane(nl, 16)), max(__builtin_amdgcn_readlane(nl, 32), __builtin_amdgcn_readlane(nl, 48)));
    const LeafLink* Lc = V.lc_link + l0;
    LeafLink K0 = Lc[max(nl - 1, 0)];
#pragma unroll 1
    for (int u = 0; u < nlw; ++u) {
        const int t = nl - 1 - u;                         // the top link first
        const bool act = t >= 0;
        const LeafLink K1 = Lc[max(t - 1, 0)];            // (the next link's record: on its way while this link is solved)
        // (ancestors inside the chain: their entries of xw were stored by this row one iteration ago, barrier below)
        small_bwd<KP, LPF, NC, FPW * LPF>(V, K0, act ? K0.k : 0, act ? K0.m : 0, li, xus[0][h], w[0][h], nc, sx);
        __syncthreads();
        K0 = K1;
    }
}
__global__ __launch_bounds__(64) void k_bwd_leafchain(DevView V, int nchains) { bwd_leafchain_row<1>(V, nchains, 1, 0); }
__global__ __launch_bounds__(64) void k_bwd_leafchain_rb(DevView V, int nchains, int nc, size_t sx) { bwd_leafchain_row<SOLVE_RB>(V, nchains, nc, sx); }

// ================================================================================================
// BIG fronts in the triangular solves: a CHAIN GROUP (<= 4 links of an in-place separator chain, <= 256 columns) is one
// unit, handled at its LAST link (FrontMeta::grem == 0; the other links return at once).  All links of a chain share one
// forward vector (cvec + cv): the update entries of a link ARE the entries of the next link, nothing is copied.
//   k_fwd_grp      one workgroup: children gathered into the chain vector; per link  y = L11^{-1} P b, z = D^{-1} y, and
//                  the entries of the group's later pivots updated (<= 192 rows)
//   k_fwd_grp_upd  256 rows per workgroup: entries beyond the group  -=  sum over links  L21 y   (<= 256 columns in one pass)
//   k_bwd_grp_dot  256 rows per workgroup: partial  L21^T x  of the rows beyond the group, for all the group's columns
//   k_bwd_grp      one workgroup: per link (last to first)  x = P^T L11^{-T} ( z - partials - L(group rows)^T x )
// ================================================================================================
__global__ __launch_bounds__(256) void k_fwd_grp(DevView V, int list_off, int top_mode)
{
    __shared__ double bp[128], ys[128];
    const FrontMeta M = V.fmeta[list_off + blockIdx.x];
    if (M.grem != 0) return;
    const int tid = threadIdx.x;
    const int nl = M.gpos + 1;
    for (int j = 0; j < nl; ++j) {
        const GroupLink G = V.gtab[M.gbase + j];
        double* cv = V.cvec + G.cv;
        if (!G.alias) { for (int i = tid; i < G.m; i += 256) cv[i] = 0.0; __syncthreads(); }
        if (top_mode && V.top_rhs && G.tr >= 0) {
            const double* tr = V.top_rhs + G.tr;
            for (int i = tid; i < G.m; i += 256) cv[i] += tr[i];
            __syncthreads();
        }
        for (int cp = G.ch0; cp < G.ch1; ++cp) {
            const ChildMeta Cm = V.cmeta[cp];
            if (Cm.aliased) continue;
            if (top_mode && V.top_rhs && Cm.owner >= 0) continue;
            const int base = Cm.relbase, mc = Cm.mc;
            for (int t = tid; t < mc; t += 256) cv[V.rel[base + t]] += V.cvec[Cm.cvbase + t];
            __syncthreads();
        }
    }
    int done = 0;
    for (int j = 0; j < nl; ++j) {
        const GroupLink G = V.gtab[M.gbase + j];
        double* cv = V.cvec + G.cv;
        const int k = G.k, c0 = G.c0;
        done += k;
        const int rem = M.gcols - done;
        for (int p = tid; p < k; p += 256) { const int lp = V.lperm[c0 + p]; bp[p] = V.xw[c0 + lp] + cv[lp]; }
        __syncthreads();
        minv_rows_quad(V.minv + G.minv_off, k, bp, ys, tid);
        __syncthreads();
        for (int q = tid; q < k; q += 256) {
            const int pt = V.ptype[c0 + q];
            double z;
            if (pt == 1) z = ys[q] * V.dinv[c0 + q];
            else if (pt == 2) z = V.dinv[c0 + q] * ys[q] + V.doff[c0 + q] * ys[q + 1];
            else z = V.doff[c0 + q - 1] * ys[q - 1] + V.dinv[c0 + q] * ys[q];
            V.zb[c0 + q] = z;
            V.ybuf[c0 + q] = ys[q];
        }
        const double* Lg = V.L + G.panel_off;
        for (int i = k + tid; i < k + rem; i += 256) {
            double t0 = 0.0, t1 = 0.0;
            int p = 0;
            for (; p + 7 < k; p += 8) {                      // 8 independent loads in flight per thread
                double l[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) l[u] = Lg[i + (size_t)(p + u) * G.ldp];
#pragma unroll
                for (int u = 0; u < 8; u += 2) { t0 += l[u] * ys[p + u]; t1 += l[u + 1] * ys[p + u + 1]; }
            }
            for (; p < k; ++p) t0 += Lg[i + (size_t)p * G.ldp] * ys[p];
            cv[i] -= t0 + t1;
        }
        __syncthreads();
    }
}

// Fused forward step of a one-link solve unit that has nothing to gather (FrontMeta::solo): block 0 does the pivot part,
// blocks 1.. each take 64 update rows and recompute y = L11^{-1} P b themselves (64 x 64 mat-vec from L2) instead of
// waiting for another launch.  b is read from xw, z goes to zb: nothing a sibling block reads is overwritten.
__global__ __launch_bounds__(256) void k_fwd_solo(DevView V, int list_off)
{
    __shared__ double bp[128], ys[128];
    __shared__ double red[4][64];
    const FrontMeta M = V.fmeta[list_off + blockIdx.y];
    const int k = M.k, m = M.m, c0 = M.c0;
    const int rb = (int)blockIdx.x - 1;                       // -1: pivot part
    if (rb >= 0 && k + rb * 64 >= m) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* cv = V.cvec + M.cv;
    for (int p = tid; p < k; p += 256) { const int lp = V.lperm[c0 + p]; bp[p] = V.xw[c0 + lp] + (M.solo == 1 ? cv[lp] : 0.0); }
    __syncthreads();
    minv_rows_quad(V.minv + M.minv_off, k, bp, ys, tid);
    __syncthreads();
    if (rb < 0) {
        for (int q = tid; q < k; q += 256) {
            const int pt = V.ptype[c0 + q];
            double z;
            if (pt == 1) z = ys[q] * V.dinv[c0 + q];
            else if (pt == 2) z = V.dinv[c0 + q] * ys[q] + V.doff[c0 + q] * ys[q + 1];
            else z = V.doff[c0 + q - 1] * ys[q - 1] + V.dinv[c0 + q] * ys[q];
            V.zb[c0 + q] = z;
        }
        return;
    }
    const int i = k + rb * 64 + lane;
    const bool ok = i < m;
    double t0 = 0.0, t1 = 0.0;
    upd_row_acc(V.L + M.panel_off + (ok ? i : k), M.ldp, k, ys, wave, t0, t1);
    red[wave][lane] = t0 + t1;
    __syncthreads();
    if (wave == 0 && ok) {
        const double t = red4(red, lane);
        cv[i] = (M.solo == 1 ? cv[i] : 0.0) - t;
    }
}

// k <= 64 variant of k_fwd_solo with every load that only depends on the front record issued up front (the pivot order, the
// inverse and the panel entries do not depend on the right-hand side): one dependent round trip instead of four.  On this part a
// dependent global access costs 1.5-2 us, which is what a launch of these latency-bound kernels is made of.
__global__ __launch_bounds__(256) void k_fwd_solo64(DevView V, int list_off)
{
    __shared__ double bp[64], ys[64];
    __shared__ double red[4][64];
    const FrontMeta M = V.fmeta[list_off + blockIdx.y];
    const int k = M.k, m = M.m, c0 = M.c0;
    const int rb = (int)blockIdx.x - 1;                       // -1: pivot part
    if (rb >= 0 && k + rb * 64 >= m) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* cv = V.cvec + M.cv;
    // ---- everything that depends on M only ----
    const int lpv = (tid < k) ? V.lperm[c0 + tid] : 0;
    const double* Mg = V.minv + M.minv_off;
    const int q = tid >> 2, part = tid & 3;
    double mreg[16];
    ld_minv_row16(mreg, Mg, k, tid);
    const int i = k + rb * 64 + lane;
    const bool ok = rb >= 0 && i < m;
    const double* Lg = V.L + M.panel_off + (ok ? i : k);
    double lreg[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) { const int p = wave * 8 + (u & 7) + 32 * (u >> 3); lreg[u] = (ok && p < k) ? Lg[(size_t)p * M.ldp] : 0.0; }
    const double cvi = (ok && wave == 0 && M.solo == 1) ? cv[i] : 0.0;
    const PivD D = ld_pivd(V, c0, tid, rb < 0 && tid < k);
    // ---- dependent on the pivot order ----
    if (tid < 64) bp[tid] = tid < k ? V.xw[c0 + lpv] + (M.solo == 1 ? cv[lpv] : 0.0) : 0.0;      // (ALL 64 entries: the product below runs over them with zeros of mreg, and 0 x a NaN left in LDS by an earlier kernel is NaN)
    __syncthreads();
    {
        const double a = quad_dot16(mreg, bp, part);
        if (part == 0 && q < k) ys[q] = a;
    }
    __syncthreads();
    if (rb < 0) {
        if (tid < k) {
            double z;
            if (D.pt == 1) z = ys[tid] * D.dq;
            else if (D.pt == 2) z = D.dq * ys[tid] + D.oq * ys[tid + 1];
            else z = D.oq1 * ys[tid - 1] + D.dq * ys[tid];
            V.zb[c0 + tid] = z;
        }
        return;
    }
    double t0 = 0.0, t1 = 0.0;
#pragma unroll
    for (int u = 0; u < 16; u += 2) {
        const int p = wave * 8 + (u & 7) + 32 * (u >> 3);
        t0 += lreg[u] * ((p < k) ? ys[p] : 0.0); t1 += lreg[u + 1] * ((p + 1 < k) ? ys[p + 1] : 0.0);
    }
    red[wave][lane] = t0 + t1;
    __syncthreads();
    if (wave == 0 && ok) cv[i] = cvi - red4(red, lane);
}

__global__ __launch_bounds__(256) void k_fwd_grp_upd(DevView V, int list_off)
{
    // 64 rows per workgroup (one per lane), the columns of the group's links one link after the other (upd_row_acc, red4)
    __shared__ double ys[256];
    __shared__ double red[4][64];
    const FrontMeta M = V.fmeta[list_off + blockIdx.y];
    if (M.grem != 0) return;
    if (M.k + blockIdx.x * 64 >= M.m) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nl = M.gpos + 1;
    int cb = 0;
    for (int j = 0; j < nl; ++j) {
        const GroupLink G = V.gtab[M.gbase + j];
        for (int p = tid; p < G.k; p += 256) ys[cb + p] = V.ybuf[G.c0 + p];
        cb += G.k;
    }
    __syncthreads();
    const int i = M.k + blockIdx.x * 64 + lane;
    const bool ok = i < M.m;
    double t0 = 0.0, t1 = 0.0;
    cb = 0;
    for (int j = 0; j < nl; ++j) {
        const GroupLink G = V.gtab[M.gbase + j];
        upd_row_acc(V.L + G.panel_off + (G.m - M.m) + (ok ? i : M.k), G.ldp, G.k, ys + cb, wave, t0, t1);
        cb += G.k;
    }
    red[wave][lane] = t0 + t1;
    __syncthreads();
    if (wave == 0 && ok) V.cvec[M.cv + i] -= red4(red, lane);
}

__global__ __launch_bounds__(256) void k_bwd_grp_dot(DevView V, int list_off)
{
    // 256 rows per workgroup (4 per lane); column blocks of 4 are dealt to the wavefronts: 16 loads in flight per lane
    __shared__ double xs[256];
    const FrontMeta M = V.fmeta[list_off + blockIdx.y];
    if (M.grem != 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ibase = M.k + blockIdx.x * 256;
    if (ibase >= M.m) return;
    const int nrow = min(256, M.m - ibase);
    xs[tid] = (tid < nrow) ? V.xw[V.sn_rows[M.r0 + ibase + tid]] : 0.0;
    __syncthreads();
    double* part = V.gpart + M.gpart + (size_t)blockIdx.x * M.gcols;
    const int nl = M.gpos + 1;
    const double x0 = xs[lane], x1 = xs[lane + 64], x2 = xs[lane + 128], x3 = xs[lane + 192];
    const bool v0 = lane < nrow, v1 = lane + 64 < nrow, v2 = lane + 128 < nrow, v3 = lane + 192 < nrow;
    int cb = 0;
    for (int j = 0; j < nl; ++j) {
        const GroupLink G = V.gtab[M.gbase + j];
        const double* Lg = V.L + G.panel_off + (G.m - M.m) + ibase + lane;
        const int k = G.k;
        for (int pb = wave * 4; pb < k; pb += 16) {
            double t[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool cv = pb + u < k;
                const double* c = Lg + (size_t)(pb + u) * G.ldp;
                const double a0 = (cv && v0) ? c[0] : 0.0, a1 = (cv && v1) ? c[64] : 0.0, a2 = (cv && v2) ? c[128] : 0.0, a3 = (cv && v3) ? c[192] : 0.0;
                t[u] = (a0 * x0 + a1 * x1) + (a2 * x2 + a3 * x3);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) { t[u] = wave_sum(t[u]); if (lane == 0 && pb + u < k) part[cb + pb + u] = t[u]; }
        }
        cb += k;
    }
}

// A 256-row x 64-column block of a panel in the registers of a workgroup of 4 wavefronts, lv[pass][column of the pass][row strip]: wavefront `wave` holds
// the columns wave * 4 + 16 ps + u < k, lane `lane` their rows lane + 64 s < nrow (Lg: the lane's first row of the panel's first column); zeros elsewhere.
// CLAMP: the address of a column >= k is that of column 0 (the chain sweep's dot workgroups).
template <bool CLAMP>
__device__ __forceinline__ void ld_panel_block(double (&lv)[4][4][4], const double* Lg, const int ldp, const int k, const int wave, const int lane, const int nrow)
{
    const bool v0 = lane < nrow, v1 = lane + 64 < nrow, v2 = lane + 128 < nrow, v3 = lane + 192 < nrow;
#pragma unroll
    for (int ps = 0; ps < 4; ++ps)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int col = wave * 4 + 16 * ps + u;
            const bool cv = col < k;
            const double* c = Lg + (size_t)(CLAMP && !cv ? 0 : col) * ldp;
            lv[ps][u][0] = (cv && v0) ? c[0] : 0.0; lv[ps][u][1] = (cv && v1) ? c[64] : 0.0;
            lv[ps][u][2] = (cv && v2) ? c[128] : 0.0; lv[ps][u][3] = (cv && v3) ? c[192] : 0.0;
        }
}
// a column of the block against the lane's four solution entries; the wavefront's sum over the lanes is the caller's (wave_sum here, wave_sum_dpp in the chain sweep)
__device__ __forceinline__ double strip_dot(const double (&l)[4], const double x0, const double x1, const double x2, const double x3) { return (l[0] * x0 + l[1] * x1) + (l[2] * x2 + l[3] * x3); }

// per-link (one link per solve unit), k <= 64 variants of k_bwd_grp_dot / k_bwd_grp with the loads that only depend on the front
// record hoisted to the top (same order of summation: part_sum4 is k_bwd_grp's, the dot products sum as k_bwd_grp_dot's)
__global__ __launch_bounds__(256) void k_bwd_dot64(DevView V, int list_off)
{
    const FrontMeta M = V.fmeta[list_off + blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ibase = M.k + blockIdx.x * 256;
    if (ibase >= M.m) return;
    const int nrow = min(256, M.m - ibase), k = M.k;
    const bool v0 = lane < nrow, v1 = lane + 64 < nrow, v2 = lane + 128 < nrow, v3 = lane + 192 < nrow;
    // the panel entries first (they depend on the front record only) ...
    double lv[4][4][4];
    ld_panel_block<false>(lv, V.L + M.panel_off + ibase + lane, M.ldp, k, wave, lane, nrow);
    // ... then the two dependent hops to the solution entries of the rows
    const int r0i = M.r0 + ibase;
    const double x0 = v0 ? V.xw[V.sn_rows[r0i + lane]] : 0.0, x1 = v1 ? V.xw[V.sn_rows[r0i + lane + 64]] : 0.0;
    const double x2 = v2 ? V.xw[V.sn_rows[r0i + lane + 128]] : 0.0, x3 = v3 ? V.xw[V.sn_rows[r0i + lane + 192]] : 0.0;
    double* part = V.gpart + M.gpart + (size_t)blockIdx.x * M.gcols;
#pragma unroll
    for (int ps = 0; ps < 4; ++ps)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int col = wave * 4 + 16 * ps + u;
            const double t = wave_sum(strip_dot(lv[ps][u], x0, x1, x2, x3));
            if (lane == 0 && col < k) part[col] = t;
        }
}
__global__ __launch_bounds__(256) void k_bwd_fin64(DevView V, int list_off)
{
    __shared__ double ws[64];
    const FrontMeta M = V.fmeta[list_off + blockIdx.x];
    const int tid = threadIdx.x;
    const int k = M.k, c0 = M.c0;
    const int nch = (M.m - M.k + 255) / 256;
    const double* part = V.gpart + M.gpart;
    const double* Mg = V.minv + M.minv_off;
    const int pcol = tid >> 2, part4 = tid & 3;
    double mreg[16];
    ld_minv_col16(mreg, Mg, k, pcol, part4);
    const int lpv = (part4 == 0 && pcol < k) ? V.lperm[c0 + pcol] : 0;
    if (tid < 64) ws[tid] = 0.0;
    __syncthreads();
    if (tid < k) { const double t = part_sum4(part, nch, M.gcols, tid); ws[tid] = V.zb[c0 + tid] - t; }
    __syncthreads();
    const double a = quad_dot16(mreg, ws, pcol + part4);       // (entries beyond k are zero in mreg)
    if (part4 == 0 && pcol < k) V.xw[c0 + lpv] = a;
}

__global__ __launch_bounds__(256) void k_bwd_grp(DevView V, int list_off)
{
    __shared__ double ws[128], xs[256];
    const FrontMeta M = V.fmeta[list_off + blockIdx.x];
    if (M.grem != 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nch = (M.m - M.k + 255) / 256;
    const double* part = V.gpart + M.gpart;
    int cb = M.gcols;
    for (int j = M.gpos; j >= 0; --j) {
        const GroupLink G = V.gtab[M.gbase + j];
        const int k = G.k, c0 = G.c0;
        cb -= k;                                           // first group column of this link
        const int rem = M.gcols - cb - k;                  // pivots of the later links = this link's first update rows
        for (int p = tid; p < k; p += 256) { const double t = part_sum4(part, nch, M.gcols, cb + p); ws[p] = V.zb[c0 + p] - t; }
        for (int i = tid; i < rem; i += 256) xs[i] = V.xw[V.sn_rows[G.r0 + k + i]];
        __syncthreads();
        if (rem > 0) {
            const double* Lg = V.L + G.panel_off + k;
            for (int pb = wave * 4; pb < k; pb += 16) {           // 4 columns per pass: their loads are all in flight together
                double t[4] = {0.0, 0.0, 0.0, 0.0};
                for (int i = lane; i < rem; i += 64) {
                    const double x = xs[i];
#pragma unroll
                    for (int u = 0; u < 4; ++u) if (pb + u < k) t[u] += Lg[i + (size_t)(pb + u) * G.ldp] * x;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) { t[u] = wave_sum(t[u]); if (lane == 0 && pb + u < k) ws[pb + u] -= t[u]; }
            }
            __syncthreads();
        }
        minv_cols_quad(V, V.minv + G.minv_off, c0, k, ws, tid);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// sync-free chain sweeps (see ChainLink / ChainDesc)
// ------------------------------------------------------------------------------------------------
__global__ void k_merge_err(int* dst, const int* src) { if (threadIdx.x == 0 && blockIdx.x == 0 && *src != 0) *dst = 1; }      // time-out flag of a solve context into the solver's own
__global__ void k_bump_epoch(int* e) { if (threadIdx.x == 0 && blockIdx.x == 0) *e += 1; }
template <int NAP>
__device__ __forceinline__ void chain_wait(const int* flag, const int epoch, int* err)
{
    if (threadIdx.x == 0) {
        // bounded: a producer that never shows up (it cannot: it has a lower workgroup index, so it was dispatched before) must not hang the GPU
        // NAP: 64-cycle units between two polls -- long where the flag is not the last one the workgroup waits for (fewer requests in the
        // L2 queues the critical hop goes through)
        int spins = 0;
        while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch) {
            __builtin_amdgcn_s_sleep(NAP);
            if (++spins > (1 << 24)) { *err = 1; break; }
        }
    }
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}
__device__ __forceinline__ void chain_signal(int* flag, const int epoch)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");       // every wavefront publishes its own stores
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The same hand-over without the fence.  A release fence at agent scope writes back EVERY dirty line of the XCD's L2 (buffer_wbl2) -- whoever dirtied it: on a
// chain-group launch that is the trailing-matrix traffic of a few dozen workgroups -- 1.1-1.75 us per signal on the critical chain of every link
// (profiles/r04b_synth_1e6_pivot_block_phases.txt: "F flag raised", "S flag raised").  When everything the consumers read behind this flag was stored
// agent-coherently (st_coh / st16_coh: sc1 stores go through the L2 to the fabric), the stores' acknowledgements are all the ordering needed -- the
// pattern of the solve sweeps below.  The consumer side (chain_wait: poll, acquire = buffer_inv) is unchanged.
__device__ __forceinline__ void chain_signal_coh(int* flag, const int epoch)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // every wavefront: its own coherent stores have been acknowledged
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_coh(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st16_coh(double* p, double v0, double v1)      // two consecutive doubles, one 16-byte agent-coherent store (8-byte alignment is enough, as for the compiler's own)
{
    typedef double v2d_ __attribute__((ext_vector_type(2)));
    const v2d_ v = (v2d_){v0, v1};
    asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(p), "v"(v) : "memory");
}
// ---- the messages of the sweeps ----
// The 8 XCDs of the part have an L2 each; what one workgroup stores becomes visible to another XCD only through the fabric.  A release
// fence at agent scope writes the WHOLE L2 back (buffer_wbl2) and an acquire invalidates it: measured 1.6-2.1 us per one-way message of
// 64 doubles with "data, fence, flag / poll, fence, load" (tools/micro/pingpong.hip).  So nothing here uses fences:
//   * a link's solution travels as 64 {value, tag} pairs, each ONE 16-byte agent-coherent store (sc1: through the L2 to the fabric) that the
//     consumers poll with 16-byte agent-coherent loads -- value and tag arrive together, no flag, no fence: 0.4-0.5 us per message;
//   * everything else a workgroup hands to another one inside a launch (rows of a chain vector, solution entries) is stored and loaded
//     agent-coherently too, and the flag that announces it goes out after the stores have been acknowledged (s_waitcnt vmcnt(0)).
__device__ __forceinline__ v2d ld_tag(const v2d* p) { v2d r; asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(r) : "v"(p) : "memory"); return r; }
__device__ __forceinline__ void st_tag(v2d* p, v2d v) { asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ double ld_coh(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_coh(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// a value every lane holds identically, moved to scalar registers (the compiler cannot see that what a vector load of a per-workgroup record returns is uniform)
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ long long uni(long long x) { return ((long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(x >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ ChainLink uni(const ChainLink& a)
{
    ChainLink r; r.panel_off = uni(a.panel_off); r.minv_off = uni(a.minv_off); r.c0 = uni(a.c0); r.k = uni(a.k); r.ldp = uni(a.ldp); r.s = uni(a.s); r.r0 = uni(a.r0); r.koff = uni(a.koff); r.fi = uni(a.fi); r.pad1 = 0;
    return r;
}
__device__ __forceinline__ ChainDesc uni(const ChainDesc& a)
{
    ChainDesc r; r.cvb = uni(a.cvb); r.link0 = uni(a.link0); r.nlinks = uni(a.nlinks); r.tail = uni(a.tail); r.ktot = uni(a.ktot); r.wg0f = uni(a.wg0f); r.wg0b = uni(a.wg0b);
    r.ch0 = uni(a.ch0); r.ch1 = uni(a.ch1); r.alias0 = uni(a.alias0); r.s0 = uni(a.s0); r.init = uni(a.init); r.gw0 = uni(a.gw0); r.gw1 = uni(a.gw1); r.tf0 = uni(a.tf0);
    r.pw0 = uni(a.pw0); r.pw1 = uni(a.pw1); r.dot0 = uni(a.dot0); r.pad0 = 0;
    return r;
}
// the whole wavefront waits until the (first k of the) 64 tagged entries at p carry this solve's tag; returns lane's value (0 beyond k).
// Dozens of workgroups wait for the same message, and every poll is a request to the ONE memory channel that holds it: polls of all 64
// entries from every waiter queue up there and the message the next link is waiting for arrives 1.7 us late instead of 0.45 (measured).  So a
// waiter polls the first entry only (one request per wavefront), and the further it is from needing the message -- dist: hops between this
// message and the last one it waits for -- the longer it sleeps between polls; then one load of all entries (repeated if the producer's other
// wavefronts have not landed yet).  There is ALWAYS an s_sleep between two polls: re-issued back to back (~100 ns apart) by the same wavefront,
// the agent-coherent load of the same line kept returning the value of the first poll -- for seconds -- on this part.
__device__ __forceinline__ double tag_await(const v2d* p, const int lane, const int k, const double ep, const int dist, int* err)
{
    int spins = 0;
    const int ehi = __double2hiint(ep), elo = __double2loint(ep);
    while (dist > 0) {          // (the message the workgroup needs next is polled in full straight away: one round trip less)
        const v2d h = ld_tag(p);
        if (__builtin_amdgcn_readfirstlane(__double2hiint(h.y)) == ehi && __builtin_amdgcn_readfirstlane(__double2loint(h.y)) == elo) break;      // (scalar branch)
        __builtin_amdgcn_s_sleep(1);
        for (int d = 0; d < min(dist, 6); ++d) __builtin_amdgcn_s_sleep(10);
        if (++spins > (1 << 22)) { *err = 1; break; }       // (cannot happen: the producer has a lower workgroup index, it was dispatched first)
    }
    const v2d* q = p + (lane < k ? lane : 0);
    v2d v;
    while (true) {
        v = ld_tag(q);
        if (__all(v.y == ep)) break;
        __builtin_amdgcn_s_sleep(1);
        if (++spins > (1 << 22)) { *err = 1; break; }
    }
    return lane < k ? v.x : 0.0;
}
// flags of the sweeps (FLAG_STRIDE ints apart): raised after this workgroup's coherent stores are acknowledged; awaited side by side, one per lane
__device__ __forceinline__ void flag_raise(int* flag, const int epoch)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void flags_await(const int* flags, const int* list, const int f0, const int f1, const int epoch, int* err)
{
    if (threadIdx.x < 64)
        for (int f = f0 + (int)threadIdx.x; f < f1; f += 64) {
            const int* flag = flags + (size_t)(list ? list[f] : f) * FLAG_STRIDE;
            int spins = 0;
            while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch) {
                __builtin_amdgcn_s_sleep(4);
                if (++spins > (1 << 22)) { *err = 1; break; }
            }
        }
    __syncthreads();
}

// Forward sweep of a segment.  Workgroup = one link of a chain (64 pivot rows of the chain vector) or 64 rows beyond the chain; it OWNS its rows:
// their running value sits in registers (4 lanes per row, each with 16 of the 64 columns of a panel block) until every earlier link of the
// chain has been applied.  Five wavefronts:
//   * wavefront 4 is the POLLER: it waits for the tagged y of one earlier link after the other and puts it into LDS -- it has no other memory
//     operation in flight, ever: loads return to a wavefront in order, so a poll issued behind the prefetch of a panel block (HBM, ~2 us) would
//     see the message that much late (measured: 2.4 us per hop that way, 0.9 us for the bare message, tools/micro/chain_hop.hip);
//   * wavefronts 0-3 apply a message as soon as the barrier says it is there: 16 FMAs per lane, two DPP adds.  The panel blocks of the NEXT TWO
//     links are in registers or on their way (a block is requested two hops before it is needed).
// A link then permutes (LDS, one barrier), applies its stored inverse from registers and publishes y.  Everything that does not depend on the
// incoming vectors -- inverse, pivot data, panel blocks, the children's inverse row maps -- is requested before the first wait.
__global__ __launch_bounds__(320) void k_fwd_chain(DevView V, int wg0)
{
    __shared__ double ymsg[2][64], bps[64], yss[64];
    __shared__ int ipos[64], lc0[64], lkk[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = (tid >> 2) & 63, part = tid & 3;
    const bool poller = wave == 4;
    const int di = V.chwg_f[wg0 + (int)blockIdx.x];
    const ChainDesc C = uni(V.chdesc[di]);
    unsigned long long* tr = V.strace ? V.strace + 4 * (size_t)(wg0 + (int)blockIdx.x) : nullptr;
    if (tr && tid == 0) tr[0] = wall_clock64();
    const int w = (int)blockIdx.x - C.wg0f;
    const int epoch = uni(*V.sepoch);
    const double ep = (double)epoch;
    int* err = V.sepoch + 1;
    const bool is_link = w < C.nlinks;
    const ChainLink Me = uni(V.chlink[C.link0 + (is_link ? w : C.nlinks - 1)]);
    const int roff = is_link ? Me.koff : C.ktot + 64 * (w - C.nlinks);       // my rows inside the chain vector
    const int rows = is_link ? Me.k : min(64, C.tail - 64 * (w - C.nlinks));
    const bool rok = !poller && row < rows;
    double* cvp = V.cvec + C.cvb;
    const int k = Me.k, c0 = Me.c0;
    const int nprev = is_link ? w : C.nlinks;
    double mreg[16], lrA[16], lrB[16];
    PivD D = {1, 0.0, 0.0, 0.0};
    auto fetch_block = [&](double (&lr)[16], const int i) {      // my rows of link i's panel
        const ChainLink L = V.chlink[C.link0 + i];
        const double* Lb = V.L + uni(L.panel_off) + (roff - uni(L.koff));      // (uniform base + 32-bit lane offsets: one address register pair, not 16)
        const int ldl = uni(L.ldp), kl = uni(L.k);
        const int off = (rok ? row : 0) + part * ldl;
#pragma unroll
        for (int u = 0; u < 16; ++u) lr[u] = (rok && part + 4 * u < kl) ? Lb[off + 4 * u * ldl] : 0.0;
    };
    double xb = 0.0;
    if (!poller) {
        if (is_link) {
            ld_minv_row16(mreg, V.minv + Me.minv_off, k, tid);
            if (tid < 64) bps[tid] = 0.0;          // (entries beyond k meet zeros of mreg below: they must not be whatever an earlier kernel left in LDS -- 0 x NaN)
            if (tid < k) ipos[V.lperm[c0 + tid]] = tid;
            D = ld_pivd(V, c0, row, part == 0 && row < k);
            if (rok) xb = V.xw[c0 + row];
        }
        if (nprev > 0) fetch_block(lrA, 0);
        if (nprev > 1) fetch_block(lrB, 1);
    } else {
        for (int i = lane; i < min(nprev, 64); i += 64) { const ChainLink L = V.chlink[C.link0 + i]; lc0[i] = L.c0; lkk[i] = L.k; }
    }
    // ---- the value my rows start from ----
    double acc = 0.0;
    if (C.init == 2) {
        // rows of the children's fronts that land on mine (inverse row maps: static), then the children's chains must be complete
        int inv[4]; long long cvb[4]; int nc = 0, cp = C.ch0;
        if (!poller)
            for (; cp < C.ch1 && nc < 4; ++cp) {
                const ChildMeta Cm = V.cmeta[cp];
                if (Cm.aliased) continue;
                inv[nc] = rok ? V.relinv[Cm.inv + roff + row] : -1; cvb[nc] = Cm.cvbase; ++nc;
            }
        flags_await(V.sflag_t, V.chwait, C.gw0, C.gw1, epoch, err);
        if (!poller) {
            double t = (C.alias0 && rok) ? ld_coh(&cvp[roff + row]) : 0.0;
            for (int c = 0; c < nc; ++c) if (inv[c] >= 0) t += ld_coh(V.cvec + cvb[c] + inv[c]);
            for (; cp < C.ch1; ++cp) {          // (more than 4 gathered children: not a nested-dissection tree)
                const ChildMeta Cm = V.cmeta[cp];
                if (Cm.aliased) continue;
                const int iv = rok ? V.relinv[Cm.inv + roff + row] : -1;
                if (iv >= 0) t += ld_coh(V.cvec + Cm.cvbase + iv);
            }
            acc = xb + t;
        }
    } else {
        __syncthreads();                    // (ipos)
        if (!poller) acc = (C.init == 0 && rok) ? xb + cvp[roff + row] : xb;
    }
    const int myipos = (!poller && is_link && row < k) ? ipos[row] : 0;
    if (tr && tid == 0) tr[1] = wall_clock64();
    auto poll = [&](const int i, double* dst) {
        if ((i & 63) == 0 && i > 0) { for (int q = lane; q < min(nprev - i, 64); q += 64) { const ChainLink L = V.chlink[C.link0 + i + q]; lc0[q] = L.c0; lkk[q] = L.k; } __builtin_amdgcn_wave_barrier(); }
        dst[lane] = tag_await(V.ytag + lc0[i & 63], lane, lkk[i & 63], ep, nprev - 1 - i, err);
    };
    auto step = [&](double (&lr)[16], const double* ym, const int i) {
        double a0, a1;
        quad_dot16_eo(lr, ym, part, a0, a1);
        if (i + 2 < nprev) fetch_block(lr, i + 2);          // two hops ahead
        acc -= quad_sum_dpp(a0 + a1);
    };
    for (int i = 0; i < nprev; i += 2) {
        if (poller) poll(i, ymsg[0]);
        __syncthreads();
        if (!poller) step(lrA, ymsg[0], i);
        if (i + 1 < nprev) {
            if (poller) poll(i + 1, ymsg[1]);
            __syncthreads();
            if (!poller) step(lrB, ymsg[1], i + 1);
        }
    }
    if (poller) return;
    if (tr && tid == 0) tr[2] = wall_clock64();
    if (!is_link) {          // rows beyond the chain: complete, the parent's chain may take them
        if (rok && part == 0) st_coh(&cvp[roff + row], acc);
        flag_raise(&V.sflag_t[(size_t)(C.tf0 + (w - C.nlinks)) * FLAG_STRIDE], epoch);
        if (tr && tid == 0) tr[3] = wall_clock64();
        return;
    }
    if (part == 0 && row < k) bps[myipos] = acc;              // P b
    __syncthreads();
    double a0, a1;
    quad_dot16_eo(mreg, bps, part, a0, a1);      // (mreg is zero beyond the row)
    const double y = quad_sum_dpp(a0 + a1);
    if (part == 0 && row < k) { v2d m; m.x = y; m.y = ep; st_tag(V.ytag + c0 + row, m); }
    if (tr && tid == 0) tr[3] = wall_clock64();
    // off the chain's critical path: z = D^{-1} y for the backward sweep
    if (part == 0) yss[row] = y;
    __syncthreads();
    if (part == 0 && row < k) {
        double z;
        if (D.pt == 1) z = y * D.dq;
        else if (D.pt == 2) z = D.dq * y + D.oq * yss[row + 1];
        else z = D.oq1 * yss[row - 1] + D.dq * y;
        V.ybuf[c0 + row] = y;
        V.zb[c0 + row] = z;
    }
}
// Backward sweep of a segment, the parents' chains first.  Per chain, two kinds of workgroups:
//   * DOT workgroups, one per (link, 256 rows beyond the chain): the 256 x 64 block of the link's panel goes into registers BEFORE anything is awaited
//     (it does not depend on the solution), then -- once every link of the parent's chain has raised its flag -- the rows' solution entries, 64 FMAs per
//     lane, a DPP sum per column, 64 partial sums stored coherently, flag.  The streaming of a chain's panels is spread over the whole machine and is
//     over when the parent finishes; up to round 2 one workgroup per link streamed its own rows after the wait (18-30 us per tree level);
//   * LINK workgroups, top link first, walk the chain as in the forward sweep: wavefront 4 polls the tagged x of the later links, wavefronts 0-3 apply the
//     64 x 64 block of MY panel that meets a later link's rows (16 FMAs per lane, two DPP adds; blocks requested two hops ahead); finally L11^{-T} from
//     registers, x published tagged (for the chain) and plain (for everything below), flag for the children's chains.
__global__ __launch_bounds__(320) void k_bwd_chain(DevView V, int wg0)
{
    __shared__ double ws[64], xmsg[2][64];
    __shared__ int lc0[64], lkk[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = (tid >> 2) & 63, part = tid & 3;
    const bool poller = wave == 4;
    const ChainDesc C = uni(V.chdesc[V.chwg_b[wg0 + (int)blockIdx.x]]);
    unsigned long long* tr = V.strace ? V.strace + 4 * (size_t)(V.strace_b + wg0 + (int)blockIdx.x) : nullptr;
    if (tr && tid == 0) tr[0] = wall_clock64();
    const int r = (int)blockIdx.x - C.wg0b;
    const int nbk = (C.tail + 255) >> 8, ndots = C.nlinks * nbk;
    const int epoch = uni(*V.sepoch);
    const double ep = (double)epoch;
    int* err = V.sepoch + 1;
    if (r < ndots) {
        // ---------------- dot workgroup ----------------
        if (poller) return;
        const int jj = r / nbk, b = r - jj * nbk;                // (jj = 0: the top link)
        const ChainLink Me = uni(V.chlink[C.link0 + C.nlinks - 1 - jj]);
        const int k = Me.k, toff = C.ktot - Me.koff, ibase = b * 256, nrow = min(256, C.tail - ibase);
        const bool v0 = lane < nrow, v1 = lane + 64 < nrow, v2 = lane + 128 < nrow, v3 = lane + 192 < nrow;
        double lv[4][4][4];
        ld_panel_block<true>(lv, V.L + Me.panel_off + toff + ibase + lane, Me.ldp, k, wave, lane, nrow);
        const int r0i = Me.r0 + toff + ibase + lane;
        const int i0 = v0 ? V.sn_rows[r0i] : 0, i1 = v1 ? V.sn_rows[r0i + 64] : 0, i2 = v2 ? V.sn_rows[r0i + 128] : 0, i3 = v3 ? V.sn_rows[r0i + 192] : 0;
        flags_await(V.sflag_b, V.chwait, C.pw0, C.pw1, epoch, err);
        if (tr && tid == 0) tr[1] = wall_clock64();
        const double x0 = v0 ? ld_coh(&V.xw[i0]) : 0.0, x1 = v1 ? ld_coh(&V.xw[i1]) : 0.0, x2 = v2 ? ld_coh(&V.xw[i2]) : 0.0, x3 = v3 ? ld_coh(&V.xw[i3]) : 0.0;
        double* dp = V.dpart + (size_t)(C.dot0 + r) * 64;
#pragma unroll
        for (int ps = 0; ps < 4; ++ps)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int cc = wave * 4 + 16 * ps + u;
                const double t = wave_sum_dpp(strip_dot(lv[ps][u], x0, x1, x2, x3));
                if (lane == 0 && cc < k) st_coh(&dp[cc], t);
            }
        if (tr && tid == 0) tr[2] = wall_clock64();
        flag_raise(&V.sflag_dot[(size_t)(C.dot0 + r) * FLAG_STRIDE], epoch);
        if (tr && tid == 0) tr[3] = wall_clock64();
        return;
    }
    // ---------------- link workgroup ----------------
    const int jt = r - ndots;                                  // 0: the top link, the head of the dependency chain
    const int j = C.nlinks - 1 - jt;
    const int nlater = jt;                                     // links whose x I wait for, top first: link nlinks - 1 - i is message i
    const ChainLink Me = uni(V.chlink[C.link0 + j]);
    const int k = Me.k, c0 = Me.c0;
    double mreg[16], lrA[16], lrB[16];
    int lpv = 0;
    auto fetch_block = [&](double (&lr)[16], const int i) {      // rows of the pivots of link nlinks - 1 - i in my panel, my column; lane part has rows part, part + 4, ...
        const ChainLink L = V.chlink[C.link0 + C.nlinks - 1 - i];
        const double* Lb = V.L + uni(Me.panel_off) + (uni(L.koff) - uni(Me.koff));
        const int kl = uni(L.k);
        const int off = (col < k ? col : 0) * uni(Me.ldp) + part;
#pragma unroll
        for (int u = 0; u < 16; ++u) lr[u] = (col < k && part + 4 * u < kl) ? Lb[off + 4 * u] : 0.0;
    };
    if (!poller) {
        ld_minv_col16(mreg, V.minv + Me.minv_off, k, col, part);
        if (col < k) lpv = V.lperm[c0 + col];
        if (nlater > 0) fetch_block(lrA, 0);
        if (nlater > 1) fetch_block(lrB, 1);
    } else {
        for (int i = lane; i < min(nlater, 64); i += 64) { const ChainLink L = V.chlink[C.link0 + C.nlinks - 1 - i]; lc0[i] = L.c0; lkk[i] = L.k; }
    }
    const double zv = (tid < k) ? V.zb[c0 + tid] : 0.0;
    if (C.tail > 0) {
        // the partial sums of my dot workgroups, added in block order
        flags_await(V.sflag_dot, nullptr, C.dot0 + jt * nbk, C.dot0 + (jt + 1) * nbk, epoch, err);
        if (tr && tid == 0) tr[1] = wall_clock64();
        if (tid < 64) {
            double t = 0.0;
            const double* dp = V.dpart + (size_t)(C.dot0 + jt * nbk) * 64 + tid;
            for (int b = 0; b < nbk; ++b) t += (tid < k) ? ld_coh(dp + (size_t)b * 64) : 0.0;
            ws[tid] = zv - t;
        }
    } else if (tid < 64) ws[tid] = zv;
    __syncthreads();
    double wv = poller ? 0.0 : ws[col];
    __syncthreads();                                           // (everybody has read ws)
    if (tr && tid == 0) tr[2] = wall_clock64();
    auto poll = [&](const int i, double* dst) {
        if ((i & 63) == 0 && i > 0) { for (int q = lane; q < min(nlater - i, 64); q += 64) { const ChainLink L = V.chlink[C.link0 + C.nlinks - 1 - i - q]; lc0[q] = L.c0; lkk[q] = L.k; } __builtin_amdgcn_wave_barrier(); }
        dst[lane] = tag_await(V.xtag + lc0[i & 63], lane, lkk[i & 63], ep, nlater - 1 - i, err);
    };
    auto step = [&](double (&lr)[16], const double* xm, const int i) {
        double a0, a1;
        quad_dot16_eo(lr, xm, part, a0, a1);
        if (i + 2 < nlater) fetch_block(lr, i + 2);
        wv -= quad_sum_dpp(a0 + a1);
    };
    for (int i = 0; i < nlater; i += 2) {
        if (poller) poll(i, xmsg[0]);
        __syncthreads();
        if (!poller) step(lrA, xmsg[0], i);
        if (i + 1 < nlater) {
            if (poller) poll(i + 1, xmsg[1]);
            __syncthreads();
            if (!poller) step(lrB, xmsg[1], i + 1);
        }
    }
    if (poller) return;
    if (part == 0) ws[col] = wv;
    __syncthreads();
    double a0, a1;
    quad_dot16_eo(mreg, ws, col + part, a0, a1);     // (mreg is zero beyond k)
    const double x = quad_sum_dpp(a0 + a1);
    if (part == 0 && col < k) {
        v2d m; m.x = x; m.y = ep;
        st_tag(V.xtag + c0 + lpv, m);
        st_coh(&V.xw[c0 + lpv], x);
    }
    flag_raise(&V.sflag_b[(size_t)Me.fi * FLAG_STRIDE], epoch);
    if (tr && tid == 0) tr[3] = wall_clock64();
}

