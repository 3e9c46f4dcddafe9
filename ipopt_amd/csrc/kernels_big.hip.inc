// kernels_big.hip.inc -- part of numeric.hip (one translation unit; included there, inside namespace mi355x): fronts of order > 128: assembly, pivot blocks, panel solves, MFMA trailing updates, chain groups factored in one launch.
// ================================================================================================
// BIG fronts (order > 128): the front stays in HBM/L2 -- panel (m x k, k <= 66) in the L storage, the
// (m-k)^2 contribution block in the cb arena -- and is processed by four launches per tree level:
//   k_big_assemble  one wavefront per front column: zero, scatter A, extend-add children (deterministic)
//   k_big_diag      one workgroup per front: k x k pivot block to LDS, Bunch-Kaufman LDL^T (ldlt_lds)
//   k_big_trsm      64 rows per wavefront: L21 = A21 P L11^{-T} D^{-1}, W21 = L21 D kept for the update
//   k_big_schur     T -= L21 W21^T on 64x64 tiles, v_mfma_f64_16x16x4_f64 (the frontal GEMM)
// ================================================================================================
typedef double v4f64 __attribute__((ext_vector_type(4)));
typedef double double2a __attribute__((ext_vector_type(2), aligned(8)));      // two consecutive doubles, 8-byte aligned: one 16-byte access

// one front column by one wavefront (the whole of the first version of the kernel; the column-chunk version below falls back to it)
__device__ __forceinline__ void big_assemble_column(const DevView& V, const FrontMeta& M, const int fc, const int top_mode)
{
    const int s = M.s, c0 = M.c0, k = M.k, r0 = M.r0, m = M.m; (void)s; (void)c0; (void)r0; (void)k;
    const int lane = threadIdx.x & 63;
    const bool active = fc < m && !(M.asmcut && fc >= M.asmcut);      // (asmcut: the columns from there on are formed by the trailing update itself)
    double* col = nullptr;                                 // col[i] = front(i, fc) for i in [0,m) (panel) or [k,m) (T)
    const bool from_arena = top_mode && V.arena && V.arena_off[s] >= 0;   // replicated front at a subtree join
    const bool skip_owned = top_mode && V.arena;                           // rank-owned children are inside the arena
    if (active) {
        const double* Ar = from_arena ? V.arena + V.arena_off[s] + (size_t)fc * (m - 1) - ((size_t)fc * (fc - 1)) / 2 : nullptr;   // summed square, lower triangle packed by columns: Ar[i] = (i, fc), i >= fc
        if (fc < k) col = V.L + M.panel_off + (size_t)fc * M.ldp;
        else        col = V.cb + M.cb_off + (size_t)(fc - k) * M.ldt - k;
        if (M.alias) {          // the front already sits in its chain child's contribution block: nothing to clear or copy
            if (from_arena) for (int i = fc + lane; i < m; i += 64) col[i] += Ar[i];
        } else if (V.asm_pull) {
            // PULL: every entry of the column is the sum of what the children hold for it -- looked up through the inverse row maps -- and is
            // written ONCE: no zero fill, no read-modify-write chain per child (the scatter form costs three stores and two dependent loads per
            // entry).  Children are added in their fixed order; up to 4 of them here, the others (rare) by the scatter loop below.
            const double* Cc[4]; const int* Iv[4]; int nc = 0;
            for (int cp = M.ch0; cp < M.ch1 && nc < 4; ++cp) {
                const ChildMeta Cm = V.cmeta[cp];
                if (Cm.aliased || (skip_owned && Cm.owner >= 0) || fc < Cm.rlo || fc > Cm.rhi) continue;      // (rlo / rhi: the child has no row at this column -- no look-up)
                const int lo = V.relinv[Cm.inv + fc];
                if (lo < 0) continue;
                Cc[nc] = V.cb + Cm.cb_off + (size_t)lo * Cm.ldt; Iv[nc] = V.relinv + Cm.inv; ++nc;
            }
            if (fc < k) for (int i = lane; i < fc; i += 64) col[i] = 0.0;
            for (int i0 = fc + lane; i0 < m; i0 += 256) {
                int av[4][4]; double t[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = i0 + 64 * u;
#pragma unroll
                    for (int c = 0; c < 4; ++c) av[c][u] = (c < nc && i < m) ? Iv[c][i] : -1;
                    t[u] = (from_arena && i < m) ? Ar[i] : 0.0;
                }
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int u = 0; u < 4; ++u) if (av[c][u] >= 0) t[u] += Cc[c][av[c][u]];
#pragma unroll
                for (int u = 0; u < 4; ++u) { const int i = i0 + 64 * u; if (i < m) col[i] = t[u]; }
            }
        } else if (fc < k) {
            for (int i = lane; i < m; i += 64) col[i] = (from_arena && i >= fc) ? Ar[i] : 0.0;
        } else {
            for (int i = fc + lane; i < m; i += 64) col[i] = from_arena ? Ar[i] : 0.0;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");      // each wavefront owns its column: ordering of its own stores/loads is all that is needed
    if (active && fc < k) {
        const int q0 = V.acolptr[c0 + fc], q1 = V.acolptr[c0 + fc + 1];
        for (int q = q0 + lane; q < q1; q += 64) col[V.apos[q] - fc * m] += V.aval[q];
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");      // each wavefront owns its column: ordering of its own stores/loads is all that is needed
    int npulled = 0;                                           // contributing children the pull loop has dealt with
    for (int cp = M.ch0; cp < M.ch1; ++cp) {
        const ChildMeta Cm = V.cmeta[cp];
        const int ch = Cm.ch; (void)ch;
        if (fc < Cm.rlo || fc > Cm.rhi) continue;      // (the child has no row at this column: nothing to add, nothing to order)
        if (active && !Cm.aliased && !(skip_owned && Cm.owner >= 0)) {
            const int mc = Cm.mc;
            const int* relc = V.rel + Cm.relbase;
            const int lo = V.relinv[Cm.inv + fc];          // index of parent column fc among the child's update rows (one load, no search)
            if (lo >= 0 && V.asm_pull && !M.alias && npulled < 4) { ++npulled; continue; }
            if (lo >= 0) {
                const double* C = V.cb + Cm.cb_off + (size_t)lo * Cm.ldt;
                int a = lo + lane;
                for (; a + 192 < mc; a += 256) {             // 4 independent gather-add chains in flight per lane
                    const int r0_ = relc[a], r1_ = relc[a + 64], r2_ = relc[a + 128], r3_ = relc[a + 192];
                    const double c0_ = C[a], c1_ = C[a + 64], c2_ = C[a + 128], c3_ = C[a + 192];
                    const double t0 = col[r0_], t1 = col[r1_], t2 = col[r2_], t3 = col[r3_];
                    col[r0_] = t0 + c0_; col[r1_] = t1 + c1_; col[r2_] = t2 + c2_; col[r3_] = t3 + c3_;
                }
                for (; a < mc; a += 64) col[relc[a]] += C[a];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");      // each wavefront owns its column: ordering of its own stores/loads is all that is needed
    }
}
__global__ __launch_bounds__(256) void k_big_assemble(DevView V, int list_off, int top_mode)
{
    const FrontMeta M = V.fmeta[list_off + blockIdx.y];
    if (M.selfasm) return;                    // pure in-place chain link: its A entries are added by its own pivot-block / TRSM kernels
    big_assemble_column(V, M, blockIdx.x * 4 + (threadIdx.x >> 6), top_mode);
}

// Column-chunk version (round 4).  The kernel above gives every front COLUMN a wavefront: ~94 entries behind a chain of five dependent global
// loads (front record -> child records -> inverse row maps -> child values), 592 000 such wavefronts on the widest level of synth_1e6 -- the
// launch ran at the latency of that chain times the number of wavefront rounds (685 us for 438 MB: 1.5 TB/s).  Here a workgroup takes
// ASM_CH consecutive columns of one front and its threads own ROWS: the children's inverse row maps go to LDS once per workgroup; a thread
// looks its row up once per child and then has ASM_CH independent loads in flight -- the same row of the child in ASM_CH of its columns --
// before the first add; lanes = consecutive rows, so loads and stores of one column are contiguous.  Children are added in list order, the A
// entries behind them (as the column kernel does for the columns at most 4 children contribute to: bitwise the same there).  Fronts it does
// not cover (in-place links with other children, arena fronts of the multi-GPU top, more children than the LDS holds) go through
// big_assemble_column.
constexpr int ASM_CH = 16, ASM_MAXCH = 16;      // (ASM_MAXCH: bound of the static tables; a launch passes the largest number of children of its fronts, which sizes the row maps in LDS)
// XCD-affine order on levels of many fronts: workgroups go to the 8 XCDs round-robin by their linear index, so with the plain (tile, front) grid the ~100
// tiles of one front are spread over all eight L2s and each of them fetches that front's panels (every 64-row panel block is an operand of ~2 nt tiles);
// here XCD x takes the fronts f = x (mod 8) whole, one tile after the other -- a front's panels are fetched into ONE L2.  Same tiles, same sums.
__device__ __forceinline__ void xcd_affine(int& tx, int& fy)
{
    const int T = (int)gridDim.x, F = (int)gridDim.y, F8 = F & ~7;
    if (F8 < 16) return;
    const long long lin = (long long)blockIdx.x + (long long)T * blockIdx.y;
    if (lin >= (long long)T * F8) return;                    // (the last F mod 8 fronts: as launched)
    const long long slot = lin >> 3;
    fy = 8 * (int)(slot / T) + (int)(lin & 7); tx = (int)(slot % T);
}
__global__ __launch_bounds__(256) void k_big_assemble2(DevView V, int list_off, int top_mode, int ldi, int maxch)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    int* sidx = reinterpret_cast<int*>(smem_raw);                  // [c * ldi + i]: index of front row i among child c's update rows, or -1
    __shared__ const double* Cb[ASM_MAXCH]; __shared__ int Ld[ASM_MAXCH];      // (indexed at run time: LDS, not registers)
    __shared__ int slo[ASM_MAXCH][ASM_CH];                          // the same index for the chunk's columns
    const FrontMeta M = V.fmeta[list_off + blockIdx.y];      // (the XCD-affine order of k_big_schur64 / k_big_trsm measured equal here)
    if (M.selfasm) return;
    const int m = M.m, k = M.k, c0 = M.c0;
    const int fc0 = blockIdx.x * ASM_CH;
    if (fc0 >= m || (M.asmcut && fc0 >= M.asmcut)) return;      // (asmcut: the columns from there on are formed by the trailing update itself)
    const int tid = threadIdx.x, wave = tid >> 6;
    const bool from_arena = top_mode && V.arena && V.arena_off[M.s] >= 0;
    int nch = 0;                                                    // children that reach the front through their contribution blocks
    bool plain = !M.alias && V.asm_pull && !from_arena && m <= ldi;
    if (plain) {
        const bool skip_owned = top_mode && V.arena;
        for (int cp = M.ch0; cp < M.ch1; ++cp) {
            const ChildMeta Cm = V.cmeta[cp];
            if (Cm.aliased || (skip_owned && Cm.owner >= 0)) continue;
            if (nch == maxch) { plain = false; break; }
            const int* inv = V.relinv + Cm.inv;
            for (int i = fc0 + tid; i < m; i += 256) sidx[nch * ldi + i] = inv[i];       // (rows above the chunk's first column are never looked up)
            if (tid == 0) { Cb[nch] = V.cb + Cm.cb_off; Ld[nch] = Cm.ldt; }
            ++nch;
        }
    }
    if (!plain) {      // (workgroup-uniform)
        for (int fc = fc0 + wave; fc < min(fc0 + ASM_CH, m); fc += 4) big_assemble_column(V, M, fc, top_mode);
        return;
    }
    __syncthreads();
    for (int e = tid; e < ASM_MAXCH * ASM_CH; e += 256) { const int c = e / ASM_CH, j = e % ASM_CH; slo[c][j] = (c < nch && fc0 + j < m) ? sidx[c * ldi + fc0 + j] : -1; }
    __syncthreads();
    double* const Lp = V.L + M.panel_off; double* const Tp = V.cb + M.cb_off - k;
    const size_t ldp = (size_t)M.ldp, ldt = (size_t)M.ldt;
    for (int i = fc0 + tid; i < m; i += 256) {
        double t[ASM_CH];
#pragma unroll
        for (int j = 0; j < ASM_CH; ++j) t[j] = 0.0;
#pragma unroll 1
        for (int c = 0; c < nch; ++c) {      // (not unrolled: 16 loads in flight per child are plenty, 96 cost the occupancy)
            const int a = sidx[c * ldi + i];
            if (a < 0) continue;
            const double* Cc = Cb[c] + a; const size_t ld = (size_t)Ld[c];
            double v[ASM_CH];
#pragma unroll
            for (int j = 0; j < ASM_CH; ++j) { const int lo = slo[c][j]; v[j] = (lo >= 0 && lo <= a) ? Cc[(size_t)lo * ld] : 0.0; }      // (lo <= a <=> the entry lies in the lower triangle: i >= column)
#pragma unroll
            for (int j = 0; j < ASM_CH; ++j) t[j] += v[j];
        }
#pragma unroll
        for (int j = 0; j < ASM_CH; ++j) {
            const int fc = fc0 + j;
            if (fc < m && i >= fc) { if (fc < k) Lp[i + (size_t)fc * ldp] = t[j]; else if (!M.asmcut || fc < M.asmcut) Tp[i + (size_t)(fc - k) * ldt] = t[j]; }
        }
    }
    if (fc0 < k) {
        // panel columns: the part above the diagonal is cleared, the A entries of the chunk's columns are added behind the children
        const int ncp = min(ASM_CH, k - fc0);
        for (int idx = tid; idx < ncp * (fc0 + ncp); idx += 256) { const int j = idx / (fc0 + ncp), i = idx - j * (fc0 + ncp); if (i < fc0 + j) Lp[i + (size_t)(fc0 + j) * ldp] = 0.0; }
        __syncthreads();                                            // (a barrier orders the workgroup's global stores before the read-modify-writes below)
        const int q0 = V.acolptr[c0 + fc0], q1 = V.acolptr[c0 + fc0 + ncp];
        for (int q = q0 + tid; q < q1; q += 256) { const int pos = V.apos[q]; const int i = pos % m, c = pos / m; Lp[i + (size_t)c * ldp] += V.aval[q]; }
    }
}

// rows below the pivot block:  W21 = (A21 P) L11^{-T},  then L21 = W21 D^{-1}.  64 rows per workgroup, 16 rows per wavefront,
// BLOCKED SUBSTITUTION with L11 itself, 16 columns at a time: the columns already solved are applied by fp64 MFMA, the 16 x 16
// diagonal block through its inverse (each wavefront inverts one diagonal block first, a 16-lane register substitution), again by
// MFMA -- NOT a product with the whole L11^{-1}: that inverse (needed by the triangular solves only) then leaves the critical
// path of the factorisation, the pivot-block workgroup builds it while the panel is being solved.  In the column loop every
// wavefront works on its own 16 rows: no workgroup barrier between the column blocks.  k <= 128.
struct TrsmLds { double* As; double* Ls; double* Is; double* Ds; int* Ts; int* Lp; double* Au; int kp16, ldl; };
// au_fixed: the staging copy sits where it would for k = 64 whatever k is.  k_grp_fused keeps the L21 rows of the link BEFORE a pivot-row block's own
// link there (T.Au) while big_diag_body factors the block in the LDS in front of it; its scratch (sized by the block's OWN k, up to 64) reaches
// 2 640 doubles into this layout, and behind a NARROW link (k = 1, 2: a delayed-pivot edit makes such links in the middle of a group) the
// k-dependent offset of Au would lie inside that scratch: L21 of those rows came out overwritten (D correct, solves wrong).
__device__ __forceinline__ TrsmLds trsm_layout(char* smem_raw, const int k, const bool staged, const bool no_ls = false, const bool au_fixed = false)
{
    TrsmLds T;
    T.kp16 = (k + 15) & ~15; T.ldl = T.kp16 | 1;
    T.As = reinterpret_cast<double*>(smem_raw);               // 64 x kp16: As[r + p*65] = (A21 P)(ibase+r, p), overwritten by W in place
    T.Ls = T.As + (size_t)65 * T.kp16;                        // L11 (strictly lower part, pivot order), zero padded to kp16 x kp16 -- staged only for
    const size_t lsz = no_ls ? 0 : (size_t)T.ldl * T.kp16;            // k <= 64; the 128-column panels of the wide_panels option read it from L2 (LDS budget)
    T.Is = T.Ls + lsz;                     // inverses of the 16 x 16 diagonal blocks of L11: Is[b*272 + i + p*17]
    T.Ds = T.Is + (size_t)17 * T.kp16;                        // dinv[k], doff[k]
    T.Ts = reinterpret_cast<int*>(T.Ds + 2 * k);              // ptype[k]
    T.Lp = T.Ts + k;                                          // lperm[k]
    T.Au = staged ? reinterpret_cast<double*>(T.Lp + k + (k & 1)) : nullptr;   // 64 x k: my rows as they lie in the panel (unpermuted), staged before the pivot block is known
    if (staged && au_fixed) T.Au = reinterpret_cast<double*>(smem_raw) + (65 * 64 + 65 * 64 + 17 * 64 + 2 * 64 + 64);      // (= the k = 64 offset: As, Ls, Is, Ds, Ts + Lp)
    return T;
}
// (host side: bytes of the layout above)
static size_t trsm_lds_bytes(int k, bool staged)       // (levels with k > 64 launch the variant without the LDS copy of L11)
{
    const size_t kp16 = (size_t)((k + 15) & ~15), ldl = kp16 | 1;
    return (65 * kp16 + (kp16 <= 64 ? ldl * kp16 : 0) + 17 * kp16 + 2 * (size_t)k) * sizeof(double) + (size_t)(2 * k + 2) * sizeof(int) + (staged ? (size_t)65 * kp16 * sizeof(double) : 0) + 16;
}
template <bool STAGED_L, bool COH = false>       // L11 staged in LDS (k <= 64) or read from L2 (the 128-column panels of the wide_panels option); COH: W21 is stored agent-coherently (k_grp_fused: the flag behind it needs no release fence)
__device__ __forceinline__ void trsm_rows_impl(const DevView& V, const FrontMeta& M, const TrsmLds& T, const int ibase, const int rlim = 64, unsigned long long* ts = nullptr, const bool in_as = false, const int store_mode = 3)
// rlim: rows of the block that are this workgroup's; ts: phase clocks (development); in_as: the caller has staged the rows in As (panel column order);
// store_mode: bit 0 = W21 -> wbuf, bit 1 = L21 -> panel (a caller on the critical chain stores L21 later, out of T.Au: trsm_store_l)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = M.s, c0 = M.c0, k = M.k, m = M.m;
    double* P = V.L + M.panel_off;
    const size_t ldp = (size_t)M.ldp;
    double* W = V.wbuf + M.wb;
    double* As = T.As; const double* Ls = T.Ls; const double* Ds = T.Ds; const int* Ts = T.Ts;
    const int kp16 = T.kp16, ldl = T.ldl;
    auto Lat = [&](int i, int c) -> double {          // L11(i, c), strictly lower part, zero elsewhere
        if (STAGED_L) return Ls[i + c * ldl];
        return (i < k && c < k && i > c) ? P[i + (size_t)c * ldp] : 0.0;
    };
    // pivot data + L11 (written by the pivot-block workgroup / kernel)
    for (int j = tid; j < k; j += 256) { T.Ds[j] = V.dinv[c0 + j]; T.Ds[k + j] = V.doff[c0 + j]; T.Ts[j] = V.ptype[c0 + j]; T.Lp[j] = V.lperm[c0 + j]; }
    // the diagonal-block inverses the blocked pivot-block factorisation left behind (fetched in the same batch; used when valid)
    const int his = V.hasis[s];
    double isv[5];
    {
        const double* Ig = V.isg + (size_t)M.bigidx * ISG_STRIDE;
        const int nis = (kp16 >> 4) * 272;
#pragma unroll
        for (int u = 0; u < 5; ++u) { const int idx = tid + 256 * u; isv[u] = (idx < nis) ? Ig[idx] : 0.0; }
    }
    if (STAGED_L) {          // one batch of independent loads (a dependent global access behind the flag costs ~2 us)
        const int i = tid & 63, cq = tid >> 6;
        double lv[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) { const int c = cq + 4 * u; lv[u] = (i < k && c < k && i > c) ? P[i + (size_t)c * ldp] : 0.0; }
#pragma unroll
        for (int u = 0; u < 16; ++u) { const int c = cq + 4 * u; if (i < kp16 && c < kp16) T.Ls[i + c * ldl] = lv[u]; }
    }      // (k > 64: read through Lat() from L2)
    if (his) {
        const int nis = (kp16 >> 4) * 272;
#pragma unroll
        for (int u = 0; u < 5; ++u) { const int idx = tid + 256 * u; if (idx < nis) T.Is[idx] = isv[u]; }
    }
    __syncthreads();
    if (ts) ts[0] = clock64();
#ifdef MI355X_PIVSTAT
    const bool bprobe = gridDim.x == 1 && blockIdx.y == 1 && tid == 0 && T.Au;
    if (bprobe) g_dt[10] = wall_clock64();
#endif
    if (in_as) {
        // the rows sit in As already, in PANEL column order: nothing to do behind the blocked factorisation (natural pivot order), a
        // column permutation in place behind the strict loop
        if (!his) {
            const int r = tid & 63, pq = tid >> 6;
            double av[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) { const int p = pq + 4 * u; av[u] = (p < k) ? As[r + T.Lp[p] * 65] : 0.0; }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 16; ++u) { const int p = pq + 4 * u; if (p < kp16) As[r + p * 65] = av[u]; }
        }
    }
    else if (T.Au && kp16 <= 64) {      // (batched: the three LDS accesses of an element are a dependent chain)
        const int r = tid & 63, pq = tid >> 6;
        int lpv[16]; double av[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) { const int p = pq + 4 * u; lpv[u] = (p < k) ? T.Lp[p] : -1; }
#pragma unroll
        for (int u = 0; u < 16; ++u) av[u] = (lpv[u] >= 0) ? T.Au[r + lpv[u] * 65] : 0.0;
#pragma unroll
        for (int u = 0; u < 16; ++u) { const int p = pq + 4 * u; if (p < kp16) As[r + p * 65] = av[u]; }
    }
    else if (T.Au) { for (int idx = tid; idx < 64 * kp16; idx += 256) { const int r = idx & 63, p = idx >> 6; As[r + p * 65] = (p < k) ? T.Au[r + T.Lp[p] * 65] : 0.0; } }
    else      { for (int idx = tid; idx < 64 * kp16; idx += 256) { const int r = idx & 63, p = idx >> 6; As[r + p * 65] = (p < k && ibase + r < m) ? P[ibase + r + (size_t)T.Lp[p] * ldp] : 0.0; } }
    // inverses of the unit-lower 16 x 16 diagonal blocks: block b by wavefront b & 3, column c of the inverse by lane c
    // (only after the strict pivot loop: the blocked factorisation hands them over)
    for (int b = wave; 16 * b < kp16 && !his; b += 4) {
        if (lane < 16) {
            const int o = 16 * b;
            double x[16];                    // x = column `lane` of the inverse; column-oriented substitution: independent updates per step
#pragma unroll
            for (int i = 0; i < 16; ++i) x[i] = (i == lane) ? 1.0 : 0.0;
#pragma unroll
            for (int pp = 0; pp < 15; ++pp) {
                const double xp = (pp >= lane) ? x[pp] : 0.0;
#pragma unroll
                for (int i = pp + 1; i < 16; ++i) x[i] = fma(-Lat(o + i, o + pp), xp, x[i]);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) T.Is[b * 272 + i + lane * 17] = x[i];
        }
    }
    __syncthreads();
    if (ts) ts[1] = clock64();
#ifdef MI355X_PIVSTAT
    if (bprobe) g_dt[11] = wall_clock64();
#endif
    const int l15 = lane & 15, l4 = lane >> 4;
    const int r16 = wave * 16;
    for (int c16 = 0; c16 < kp16; c16 += 16) {
        // columns [c16, c16+16) minus what the solved columns contribute: (16 x c16) . (c16 x 16), transposed product as in the updates
        v4f64 acc = (v4f64){0.0, 0.0, 0.0, 0.0};
        if (c16 <= 48) {     // operands of the whole product in flight at once
            double oa[12], ob[12];
#pragma unroll
            for (int u = 0; u < 12; ++u) { const bool v = 4 * u < c16; oa[u] = v ? Lat(c16 + l15, 4 * u + l4) : 0.0; ob[u] = v ? As[r16 + l15 + (4 * u + l4) * 65] : 0.0; }
#pragma unroll
            for (int u = 0; u < 12; ++u) if (4 * u < c16) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(oa[u], ob[u], acc, 0, 0, 0);
        } else {
            for (int p = 0; p < c16; p += 4)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Lat(c16 + l15, p + l4), As[r16 + l15 + (p + l4) * 65], acc, 0, 0, 0);
        }
        // the block A' = A - acc goes from accumulator layout to operand layout through LDS (rows of this wavefront only)
#pragma unroll
        for (int g = 0; g < 4; ++g) As[r16 + l15 + (c16 + l4 + 4 * g) * 65] -= acc[g];
        double bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) bv[u] = As[r16 + l15 + (c16 + 4 * u + l4) * 65];
        const double* Ib = T.Is + (c16 >> 4) * 272;
        v4f64 w = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int u = 0; u < 4; ++u) w = __builtin_amdgcn_mfma_f64_16x16x4f64(Ib[l15 + (4 * u + l4) * 17], bv[u], w, 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 4; ++g) As[r16 + l15 + (c16 + l4 + 4 * g) * 65] = w[g];
    }
    __syncthreads();
    if (ts) ts[2] = clock64();
#ifdef MI355X_PIVSTAT
    if (bprobe) g_dt[12] = wall_clock64();
#endif
    // a posteriori threshold test on the rows below the pivot block (the in-block test of ldlt_reg cannot see them): a column
    // with a multiplier above 1/u is a FAILED pivot -- a delayed pivot in MA97/SSIDS, counted once per column here (num_delay)
    // (two consecutive rows per lane: 16-byte stores -- a CU issues stores at ~10 bytes per cycle whatever their width.  The loop-invariant
    //  pieces of the view are pinned in VGPRs: with ~100 SGPRs of kernel arguments spilled, the compiler otherwise RELOADS them from the
    //  kernarg segment inside the loop, a scalar-cache round trip per iteration)
    {
        const int r = 2 * (tid & 31), jq = tid >> 5;
        const int i = ibase + r;
        const bool ok0 = i < m && r < rlim, ok1 = i + 1 < m && r + 1 < rlim;
        double* Wv = W + i; double* Pv = P + i; double uv = V.pivtol; double* Auv = T.Au ? T.Au + r : nullptr; const double* Asv = As + r;
        // (Asv is NOT pinned: behind the asm its address space is unknown, the loads become FLAT ones, and the loop's base pointer is biased by the
        //  Asv[(j - 1) * 65] of a 2x2 pivot's second column to Asv - 520 with an instruction offset of 520 -- the hardware picks the aperture of a flat
        //  access from the base alone, and As starts the workgroup's LDS: for j < 8 the base lies BELOW the LDS aperture and the load of a rejected block's
        //  panel faults, HSA_STATUS_ERROR_MEMORY_APERTURE_VIOLATION.  Left to the compiler the accesses are ds_read: no aperture, no flat path)
        asm volatile("" : "+v"(Wv), "+v"(Pv), "+v"(uv), "+v"(Auv));
        if (Auv) for (int j = k + jq; j < kp16; j += 8) { Auv[j * 65] = 0.0; Auv[1 + j * 65] = 0.0; }
        bool big = false;
        if (his) {        // behind the blocked factorisation every pivot is 1x1: straight-line body
#pragma unroll 4
            for (int j = jq; j < k; j += 8) {
                const double d = Ds[j];
                const double w0 = Asv[j * 65], w1 = Asv[1 + j * 65];
                const double l0 = w0 * d, l1 = w1 * d;
                if (Auv) { Auv[j * 65] = l0; Auv[1 + j * 65] = l1; }
                if (ok1) {
                    if (store_mode & 1) { if (COH) st16_coh(&Wv[(size_t)j * m], w0, w1); else *reinterpret_cast<double2a*>(&Wv[(size_t)j * m]) = (double2a){w0, w1}; }
                    if (store_mode & 2) *reinterpret_cast<double2a*>(&Pv[(size_t)j * ldp]) = (double2a){l0, l1};
                } else if (ok0) {
                    if (store_mode & 1) { if (COH) st_coh(&Wv[(size_t)j * m], w0); else Wv[(size_t)j * m] = w0; }
                    if (store_mode & 2) Pv[(size_t)j * ldp] = l0;
                }
                big |= (ok0 && fabs(l0) * uv > 1.0) || (ok1 && fabs(l1) * uv > 1.0);
            }
        } else {
            for (int j = jq; j < k; j += 8) {
                const int pt = Ts[j];
                const double w0 = Asv[j * 65], w1 = Asv[1 + j * 65];
                double l0, l1;
                if (pt == 1) { l0 = w0 * Ds[j]; l1 = w1 * Ds[j]; }
                else if (pt == 2) { l0 = Ds[j] * w0 + Ds[k + j] * Asv[(j + 1) * 65]; l1 = Ds[j] * w1 + Ds[k + j] * Asv[1 + (j + 1) * 65]; }
                else { l0 = Ds[k + j - 1] * Asv[(j - 1) * 65] + Ds[j] * w0; l1 = Ds[k + j - 1] * Asv[1 + (j - 1) * 65] + Ds[j] * w1; }
                if (Auv) { Auv[j * 65] = l0; Auv[1 + j * 65] = l1; }      // (the staging copy is dead: L21 of my rows stays in LDS for the updates that follow)
                if (ok1) {
                    if (store_mode & 1) { if (COH) st16_coh(&Wv[(size_t)j * m], w0, w1); else *reinterpret_cast<double2a*>(&Wv[(size_t)j * m]) = (double2a){w0, w1}; }
                    if (store_mode & 2) *reinterpret_cast<double2a*>(&Pv[(size_t)j * ldp]) = (double2a){l0, l1};
                } else if (ok0) {
                    if (store_mode & 1) { if (COH) st_coh(&Wv[(size_t)j * m], w0); else Wv[(size_t)j * m] = w0; }
                    if (store_mode & 2) Pv[(size_t)j * ldp] = l0;
                }
                big |= (ok0 && fabs(l0) * uv > 1.0) || (ok1 && fabs(l1) * uv > 1.0);
            }
        }
        // a multiplier above 1/u somewhere in my rows (rare): find the columns and count each once
        if (__ballot(big) != 0ull) {
            for (int j = jq; j < k; j += 8) {
                const int pt = Ts[j];
                double l0, l1;
                const double w0 = Asv[j * 65], w1 = Asv[1 + j * 65];
                if (pt == 1) { l0 = w0 * Ds[j]; l1 = w1 * Ds[j]; }
                else if (pt == 2) { l0 = Ds[j] * w0 + Ds[k + j] * Asv[(j + 1) * 65]; l1 = Ds[j] * w1 + Ds[k + j] * Asv[1 + (j + 1) * 65]; }
                else { l0 = Ds[k + j - 1] * Asv[(j - 1) * 65] + Ds[j] * w0; l1 = Ds[k + j - 1] * Asv[1 + (j - 1) * 65] + Ds[j] * w1; }
                if (((ok0 && fabs(l0) * uv > 1.0) || (ok1 && fabs(l1) * uv > 1.0)) && atomicExch(&V.colfail[c0 + j], 1) == 0) {
                    atomicAdd(&V.apfail[s], 1);
                    atomicOr(&V.zpiv[c0 + T.Lp[j]], 2);                    // a delayed pivot: the column (and its 2x2 partner) should have waited for the parent front
                    if (pt != 1) atomicOr(&V.zpiv[c0 + T.Lp[pt == 2 ? j + 1 : j - 1]], 2);
                }
            }
        }
    }
    if (ts) ts[3] = clock64();
}
// The same panel solve IN STEP with the blocked factorisation of the pivot block (k_grp_fused, optimistic schedule; the producer side is PubHook in
// kernels_fronts.hip.inc).  The blocked substitution above consumes L11 16 columns at a time: step b needs row block b of L11 left of its diagonal
// block, that block's inverse and its pivots -- all final once phase A of sub-block b of the factorisation is through.  So the workgroup waits for the
// link's sub-block counter (sflag_p >= ftarget + b + 1), fetches exactly those pieces (agent-coherent loads: no acquire fence), does step b for its 64
// rows, scales and stores the 16 finished columns of W21 / L21, and -- a pivot-row block -- adds the step's 16 columns to the running update of its own
// pivot block (accumulators kept in registers over the four steps: the same MFMA chain as the one-pass update, so that the block comes out bitwise
// the same).  When the LAST sub-block of the pivot block is published, 48 of the 64 columns are already solved, scaled, stored and applied: what is
// left on the critical chain between two pivot blocks is one 16-column step instead of the whole panel solve, the whole own-block update and the
// hand-over of a 64 x 64 block (~43 000 of the ~106 000 cycles of a chain link, profiles/r04b_synth_1e6_pivot_block_phases.txt).
// Pivot order = natural order, all pivots 1 x 1 (the blocked factorisation; a block it REJECTS makes the whole factorisation repeat: qstat[5]).
// own: the rows are the pivot rows of a later link of the group -- Db (ldb) its pivot block in LDS, myrows its order.
__device__ __forceinline__ void trsm_rows_pipe(const DevView& V, const FrontMeta& M, const TrsmLds& T, const int ibase, const int rlim, const int store_mode,
                                               const int ftarget, const bool own, double* Db, const int ldb, const int myrows, unsigned long long* ts = nullptr)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int s = M.s, c0 = M.c0, k = M.k, m = M.m;
    double* P = V.L + M.panel_off;
    const size_t ldp = (size_t)M.ldp;
    double* W = V.wbuf + M.wb;
    double* As = T.As; double* Ls = T.Ls; double* Is = T.Is; double* Ds = T.Ds; double* Au = T.Au;
    const int kp16 = T.kp16, ldl = T.ldl, nb = kp16 >> 4;
    const double* Ig = V.isg + (size_t)M.bigidx * ISG_STRIDE;
    const int* pflag = V.sflag_p + s;
    const int r16 = wave * 16, rloc = r16 + l15, row = ibase + rloc;
    const bool rok = rloc < rlim && row < m;
    const double uv = V.pivtol;
    for (int j = tid; j < k; j += 256) { T.Ts[j] = 1; T.Lp[j] = j; Ds[k + j] = 0.0; }      // (what the slow re-check below and lval() expect of a link factored in natural order)
    // my tiles of the own pivot block (lower 16 x 16 tiles, dealt to the wavefronts as the one-pass update deals them: q & 3 == wave)
    int oti[3] = {0, 0, 0}, otc[3] = {0, 0, 0}; bool ook[3] = {false, false, false};
    v4f64 oacc[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) oacc[e] = (v4f64){0.0, 0.0, 0.0, 0.0};
    if (own) {
        const int nt = (myrows + 15) >> 4;
        int q = 0;
        for (int tc = 0; tc < nt; ++tc)
            for (int ti = tc; ti < nt; ++ti, ++q) {
                if ((q & 3) != wave) continue;
#pragma unroll
                for (int e = 0; e < 3; ++e) if ((q >> 2) == e) { oti[e] = ti; otc[e] = tc; ook[e] = true; }
            }
    }
    bool big = false;
#pragma unroll 1
    for (int b = 0; b < nb; ++b) {
        const int c16 = 16 * b;
        if (tid == 0) {
            int spins = 0;
            while (__hip_atomic_load(pflag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < ftarget + b + 1) { __builtin_amdgcn_s_sleep(2); if (++spins > (1 << 24)) { V.qstat[1] = 1; break; } }
        }
        __syncthreads();
        if (ts && b == nb - 1) ts[4] = clock64();      // (development: the LAST sub-block of the pivot block before mine is published)
        // the pieces of sub-block b (stored agent-coherently by the pivot block's workgroup)
        for (int idx = tid; idx < 16 * c16; idx += 256) { const int i = c16 + (idx & 15), c = idx >> 4; Ls[i + c * ldl] = (i < k) ? __hip_atomic_load(&P[i + (size_t)c * ldp], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0; }
        for (int idx = tid; idx < 272; idx += 256) Is[b * 272 + idx] = __hip_atomic_load(&Ig[b * 272 + idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid < 16 && c16 + tid < k) Ds[c16 + tid] = __hip_atomic_load(&V.dinv[c0 + c16 + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        // step b of the blocked substitution (trsm_rows_impl's column loop, one pass): my wavefront's 16 rows, columns [c16, c16 + 16)
        v4f64 acc = (v4f64){0.0, 0.0, 0.0, 0.0};
        if (c16 <= 48) {
            double oa[12], ob[12];
#pragma unroll
            for (int u = 0; u < 12; ++u) { const bool v = 4 * u < c16; oa[u] = v ? Ls[(c16 + l15) + (4 * u + l4) * ldl] : 0.0; ob[u] = v ? As[r16 + l15 + (4 * u + l4) * 65] : 0.0; }
#pragma unroll
            for (int u = 0; u < 12; ++u) if (4 * u < c16) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(oa[u], ob[u], acc, 0, 0, 0);
        } else {
            for (int p = 0; p < c16; p += 4)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ls[(c16 + l15) + (p + l4) * ldl], As[r16 + l15 + (p + l4) * 65], acc, 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) As[r16 + l15 + (c16 + l4 + 4 * g) * 65] -= acc[g];
        double bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) bv[u] = As[r16 + l15 + (c16 + 4 * u + l4) * 65];
        const double* Ib = Is + b * 272;
        v4f64 w = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int u = 0; u < 4; ++u) w = __builtin_amdgcn_mfma_f64_16x16x4f64(Ib[l15 + (4 * u + l4) * 17], bv[u], w, 0, 0, 0);
        // the 16 finished columns: W21 stays in As, L21 = W21 D^{-1} goes to Au; both to memory (W agent-coherently: other workgroups read it behind my S flag)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = c16 + l4 + 4 * g;
            const double wv = w[g], lv = (c < k) ? wv * Ds[c] : 0.0;
            As[rloc + c * 65] = wv;
            if (Au) Au[rloc + c * 65] = lv;
            if (rok && c < k) {
                if (store_mode & 1) __hip_atomic_store(&W[row + (size_t)c * m], wv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (store_mode & 2) P[row + (size_t)c * ldp] = lv;
                big |= fabs(lv) * uv > 1.0;
            }
        }
        if (own) {
            __syncthreads();                      // the other wavefronts' rows of these 16 columns (As / Au)
#pragma unroll
            for (int e = 0; e < 3; ++e)
                if (ook[e]) {
#pragma unroll
                    for (int u4 = 0; u4 < 4; ++u4) {
                        const int u = 4 * b + u4;
                        oacc[e] = __builtin_amdgcn_mfma_f64_16x16x4f64(Au[(16 * oti[e] + l15) + (4 * u + l4) * 65], As[(16 * otc[e] + l15) + (4 * u + l4) * 65], oacc[e], 0, 0, 0);
                    }
                }
        }
    }
    __syncthreads();
    if (ts) ts[2] = clock64();
    if (own) {
#pragma unroll
        for (int e = 0; e < 3; ++e)
            if (ook[e]) {
                const int cc = 16 * otc[e] + l15;
#pragma unroll
                for (int gg = 0; gg < 4; ++gg) { const int rr = 16 * oti[e] + l4 + 4 * gg; if (rr < myrows && cc < myrows && rr >= cc) Db[rr + cc * ldb] -= oacc[e][gg]; }
            }
    }
    // a multiplier above 1/u somewhere in my rows (rare): find the columns and count each once (as trsm_rows_impl does).  The test above ran with a wavefront
    // per 16 rows, the search below runs with a wavefront per set of columns: the verdict has to be the workgroup's, not the wavefront's
    // (through four words of the dynamic LDS -- T.Lp is not read on this path: __syncthreads_or would add static LDS to a kernel that asks for the full 160 KiB of dynamic)
    const unsigned long long bigm = __ballot(big);
    if (lane == 0) T.Lp[wave] = bigm != 0ull ? 1 : 0;
    __syncthreads();
    if ((T.Lp[0] | T.Lp[1] | T.Lp[2] | T.Lp[3]) != 0) {
        const int r = 2 * (tid & 31), jq = tid >> 5, i = ibase + r;
        const bool ok0 = i < m && r < rlim, ok1 = i + 1 < m && r + 1 < rlim;
        for (int j = jq; j < k; j += 8) {
            const double l0 = As[r + j * 65] * Ds[j], l1 = As[r + 1 + j * 65] * Ds[j];
            if (((ok0 && fabs(l0) * uv > 1.0) || (ok1 && fabs(l1) * uv > 1.0)) && atomicExch(&V.colfail[c0 + j], 1) == 0) {
                atomicAdd(&V.apfail[s], 1);
                atomicOr(&V.zpiv[c0 + j], 2);
            }
        }
    }
}
// L21 of a row block out of its LDS copy (T.Au) into the panel -- for a caller that kept it back (store_mode 1)
__device__ __forceinline__ void trsm_store_l(const DevView& V, const FrontMeta& M, const double* Lr, const int ibase, const int rlim)
{
    const int tid = threadIdx.x, k = M.k, m = M.m;
    double* P = V.L + M.panel_off;
    const size_t ldp = (size_t)M.ldp;
    const int r = 2 * (tid & 31), jq = tid >> 5, i = ibase + r;
    const bool ok0 = i < m && r < rlim, ok1 = i + 1 < m && r + 1 < rlim;
    for (int j = jq; j < k; j += 8) {
        if (ok1) *reinterpret_cast<double2a*>(&P[i + (size_t)j * ldp]) = (double2a){Lr[r + j * 65], Lr[r + 1 + j * 65]};
        else if (ok0) P[i + (size_t)j * ldp] = Lr[r + j * 65];
    }
}
// The panel solve of k_big_trsm for k <= 64 with the L11 operands in REGISTERS (MI355X_KKT_DISABLE=trsm_regs: trsm_rows_impl<true> as before).
// trsm_rows_impl stages L11 in LDS (Ls, 33 KB at k = 64, half of it zeros): 76.8 KB per workgroup, two workgroups per CU, and the launches ran at the
// latency of a workgroup's load chain (record -> pivot data, L11 -> barrier -> panel rows through lperm) times the rounds of resident workgroups.
// The column loop reads L11 only as the strictly sub-diagonal 16 x 16 blocks, each as the MFMA operand L11(c16 + l15, 4u + l4), 4u < c16: 24 doubles per
// lane, the same set in every wavefront -- loaded here straight from the panel in that layout.  The layout is trsm_layout(.., no_ls = true): As, Is, pivot
// data, 43.5 KB at k = 64, three workgroups per CU.  The panel rows are requested in NATURAL column order in the same batch as everything else -- behind
// the blocked factorisation (hasis: natural pivot order, 1x1 pivots) that is the order wanted and nothing waits for hasis or lperm; behind the strict loop
// the rows are permuted in place (the in_as branch of trsm_rows_impl) and the diagonal blocks inverted from the panel (Lat() of STAGED_L = false).
// Operand values and MFMA sequence are those of trsm_rows_impl: W21, L21 and the failed-pivot marks come out bit for bit the same.
// (host side: bytes of trsm_layout(.., k, false, true))
static size_t trsm_regs_lds_bytes(int k)
{
    const size_t kp16 = (size_t)((k + 15) & ~15);
    return (65 * kp16 + 17 * kp16 + 2 * (size_t)k) * sizeof(double) + (size_t)(2 * k + 2) * sizeof(int) + 16;
}
__device__ __forceinline__ void trsm_rows_regs(const DevView& V, const FrontMeta& M, const TrsmLds& T, const int ibase)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int s = M.s, c0 = M.c0, k = M.k, m = M.m;
    double* P = V.L + M.panel_off;
    const size_t ldp = (size_t)M.ldp;
    double* W = V.wbuf + M.wb;
    double* As = T.As; const double* Ds = T.Ds; const int* Ts = T.Ts;
    const int kp16 = T.kp16;      // (<= 64)
    // ONE batch of independent loads: pivot data, hasis, the diagonal-block inverses, the L11 operands, my rows of the panel
    const bool pj = tid < k;
    const double dv = pj ? V.dinv[c0 + tid] : 0.0, fv = pj ? V.doff[c0 + tid] : 0.0;
    const int tv = pj ? V.ptype[c0 + tid] : 0, pv = pj ? V.lperm[c0 + tid] : 0;
    const int his = V.hasis[s];
    const int nis = (kp16 >> 4) * 272;
    double isv[5];
    {
        const double* Ig = V.isg + (size_t)M.bigidx * ISG_STRIDE;
#pragma unroll
        for (int u = 0; u < 5; ++u) { const int idx = tid + 256 * u; isv[u] = (idx < nis) ? Ig[idx] : 0.0; }
    }
    double l11[24];               // block row b = 1, 2, 3 (columns [0, 16 b)): l11[2 b (b - 1) + u] = L11(16 b + l15, 4 u + l4), u < 4 b
#pragma unroll
    for (int b = 1; b < 4; ++b)
#pragma unroll
        for (int u = 0; u < 4 * b; ++u) { const int i = 16 * b + l15; l11[2 * b * (b - 1) + u] = (i < k) ? P[i + (size_t)(4 * u + l4) * ldp] : 0.0; }      // (column < 16 b <= i: strictly lower)
    {
        const int r = tid & 63, pq = tid >> 6;
        double av[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) { const int p = pq + 4 * u; av[u] = (p < k && ibase + r < m) ? P[ibase + r + (size_t)p * ldp] : 0.0; }
        if (pj) { T.Ds[tid] = dv; T.Ds[k + tid] = fv; T.Ts[tid] = tv; T.Lp[tid] = pv; }
        if (his) {
#pragma unroll
            for (int u = 0; u < 5; ++u) { const int idx = tid + 256 * u; if (idx < nis) T.Is[idx] = isv[u]; }
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) { const int p = pq + 4 * u; if (p < kp16) As[r + p * 65] = av[u]; }
    }
    __syncthreads();
    if (!his) {      // (workgroup-uniform; rare) behind the strict loop: the columns in pivot order, the diagonal blocks inverted by a 16-lane register substitution
        const int r = tid & 63, pq = tid >> 6;
        double av[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) { const int p = pq + 4 * u; av[u] = (p < k) ? As[r + T.Lp[p] * 65] : 0.0; }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 16; ++u) { const int p = pq + 4 * u; if (p < kp16) As[r + p * 65] = av[u]; }
        auto Lat = [&](int i, int c) -> double { return (i < k && c < k && i > c) ? P[i + (size_t)c * ldp] : 0.0; };      // L11(i, c), strictly lower part, zero elsewhere
        if (16 * wave < kp16) {      // block `wave` (kp16 <= 64: at most one per wavefront)
            // the diagonal block goes through the place of its inverse, fetched in one round trip by the whole wavefront (unrolled over Lat() the
            // substitution keeps its 120 loads in 240 registers); a wavefront's LDS accesses stay in program order: every read below precedes the stores
            const int o = 16 * wave;
            double* Ib = T.Is + wave * 272;
            double lv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) lv[u] = Lat(o + l15, o + 4 * u + l4);
#pragma unroll
            for (int u = 0; u < 4; ++u) Ib[l15 + (4 * u + l4) * 17] = lv[u];
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier();
            double x[16];                    // x = column `lane` of the inverse; column-oriented substitution: independent updates per step
#pragma unroll
            for (int i = 0; i < 16; ++i) x[i] = (i == lane) ? 1.0 : 0.0;
            if (lane < 16) {
#pragma unroll
                for (int pp = 0; pp < 15; ++pp) {
                    const double xp = (pp >= lane) ? x[pp] : 0.0;
#pragma unroll
                    for (int i = pp + 1; i < 16; ++i) x[i] = fma(-Ib[i + pp * 17], xp, x[i]);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier();
            if (lane < 16) {
#pragma unroll
                for (int i = 0; i < 16; ++i) Ib[i + lane * 17] = x[i];
            }
        }
        __syncthreads();
    }
    // the blocked substitution: trsm_rows_impl's column loop with the sub-diagonal operands out of l11[] (unrolled: registers are indexed statically)
    const int r16 = wave * 16;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int c16 = 16 * b;
        if (c16 < kp16) {
            v4f64 acc = (v4f64){0.0, 0.0, 0.0, 0.0};
            double ob[12];
#pragma unroll
            for (int u = 0; u < 4 * b; ++u) ob[u] = As[r16 + l15 + (4 * u + l4) * 65];
#pragma unroll
            for (int u = 0; u < 4 * b; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(l11[2 * b * (b - 1) + u], ob[u], acc, 0, 0, 0);
#pragma unroll
            for (int g = 0; g < 4; ++g) As[r16 + l15 + (c16 + l4 + 4 * g) * 65] -= acc[g];
            double bv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) bv[u] = As[r16 + l15 + (c16 + 4 * u + l4) * 65];
            const double* Ib = T.Is + b * 272;
            v4f64 w = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int u = 0; u < 4; ++u) w = __builtin_amdgcn_mfma_f64_16x16x4f64(Ib[l15 + (4 * u + l4) * 17], bv[u], w, 0, 0, 0);
#pragma unroll
            for (int g = 0; g < 4; ++g) As[r16 + l15 + (c16 + l4 + 4 * g) * 65] = w[g];
        }
    }
    __syncthreads();
    // L21 = W21 D^{-1}, the stores and the a posteriori threshold test: trsm_rows_impl's (two consecutive rows per lane, 16-byte stores, the loop-invariant
    // pieces of the view pinned in VGPRs), without the staging copy
    {
        const int r = 2 * (tid & 31), jq = tid >> 5;
        const int i = ibase + r;
        const bool ok0 = i < m, ok1 = i + 1 < m;
        double* Wv = W + i; double* Pv = P + i; double uv = V.pivtol; const double* Asv = As + r;
        asm volatile("" : "+v"(Wv), "+v"(Pv), "+v"(uv));      // (not Asv: see trsm_rows_impl)
        auto lval = [&](int j, double& l0, double& l1) {
            const int pt = Ts[j];
            const double w0 = Asv[j * 65], w1 = Asv[1 + j * 65];
            if (pt == 1) { l0 = w0 * Ds[j]; l1 = w1 * Ds[j]; }
            else if (pt == 2) { l0 = Ds[j] * w0 + Ds[k + j] * Asv[(j + 1) * 65]; l1 = Ds[j] * w1 + Ds[k + j] * Asv[1 + (j + 1) * 65]; }
            else { l0 = Ds[k + j - 1] * Asv[(j - 1) * 65] + Ds[j] * w0; l1 = Ds[k + j - 1] * Asv[1 + (j - 1) * 65] + Ds[j] * w1; }
        };
        bool big = false;
        if (his) {        // behind the blocked factorisation every pivot is 1x1: straight-line body
#pragma unroll 4
            for (int j = jq; j < k; j += 8) {
                const double d = Ds[j];
                const double w0 = Asv[j * 65], w1 = Asv[1 + j * 65];
                const double l0 = w0 * d, l1 = w1 * d;
                if (ok1) {
                    *reinterpret_cast<double2a*>(&Wv[(size_t)j * m]) = (double2a){w0, w1};
                    *reinterpret_cast<double2a*>(&Pv[(size_t)j * ldp]) = (double2a){l0, l1};
                } else if (ok0) { Wv[(size_t)j * m] = w0; Pv[(size_t)j * ldp] = l0; }
                big |= (ok0 && fabs(l0) * uv > 1.0) || (ok1 && fabs(l1) * uv > 1.0);
            }
        } else {
            for (int j = jq; j < k; j += 8) {
                const double w0 = Asv[j * 65], w1 = Asv[1 + j * 65];
                double l0, l1;
                lval(j, l0, l1);
                if (ok1) {
                    *reinterpret_cast<double2a*>(&Wv[(size_t)j * m]) = (double2a){w0, w1};
                    *reinterpret_cast<double2a*>(&Pv[(size_t)j * ldp]) = (double2a){l0, l1};
                } else if (ok0) { Wv[(size_t)j * m] = w0; Pv[(size_t)j * ldp] = l0; }
                big |= (ok0 && fabs(l0) * uv > 1.0) || (ok1 && fabs(l1) * uv > 1.0);
            }
        }
        // a multiplier above 1/u somewhere in my rows (rare): find the columns and count each once
        if (__ballot(big) != 0ull) {
            for (int j = jq; j < k; j += 8) {
                const int pt = Ts[j];
                double l0, l1;
                lval(j, l0, l1);
                if (((ok0 && fabs(l0) * uv > 1.0) || (ok1 && fabs(l1) * uv > 1.0)) && atomicExch(&V.colfail[c0 + j], 1) == 0) {
                    atomicAdd(&V.apfail[s], 1);
                    atomicOr(&V.zpiv[c0 + T.Lp[j]], 2);                    // a delayed pivot: the column (and its 2x2 partner) should have waited for the parent front
                    if (pt != 1) atomicOr(&V.zpiv[c0 + T.Lp[pt == 2 ? j + 1 : j - 1]], 2);
                }
            }
        }
    }
}
template <bool WIDEK, bool REGS = false>          // WIDEK: the level has panels of more than 64 columns (wide_panels option): L11 is not staged in LDS; REGS: trsm_rows_regs (k <= 64)
__global__ __launch_bounds__(256) void k_big_trsm(DevView V, int list_off, int rb0)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x;
    int tx = blockIdx.x, fy = blockIdx.y;
    if (V.xcd_affine) xcd_affine(tx, fy);
    const FrontMeta M = V.fmeta[list_off + fy];
    const int k = M.k, m = M.m;
    const int ibase = k + (tx + rb0) * 64;       // rb0: first row block of this launch (chain look-ahead: block 0 alone, then the rest)
    if (ibase >= m) return;
    double* P = V.L + M.panel_off;
    const size_t ldp = (size_t)M.ldp;
    if (M.selfasm) {            // pure in-place chain link: the A entries of the rows below are added by the workgroup that owns the rows
        for (int q = M.aq0 + tid; q < M.aq1; q += 256) { const int pos = V.apos[q]; const int i = pos % m, c = pos / m; if (i >= ibase && i < ibase + 64) P[i + (size_t)c * ldp] += V.aval[q]; }
        __syncthreads();
    }
    const TrsmLds T = trsm_layout(smem_raw, k, false, WIDEK || REGS);
    if (REGS) trsm_rows_regs(V, M, T, ibase);
    else      trsm_rows_impl<!WIDEK>(V, M, T, ibase);
}

// 32 x 32 block (rows i0.., columns cc0.. of the trailing matrix T of order mu) of  T -= sum over the links j0..jlast of a chain group  W L^T  on ONE wavefront,
// operands straight from L2.  The panel columns are fetched 16 at a time, the next 16 (of this or the next link) are in flight while the 16 MFMAs of the
// current ones issue: a launch of a few dozen tiles at the top of the tree runs at the L2 latency of its operand loads otherwise (measured: 39 us for
// K = 256 with one load round trip per 4 columns -- 64 dependent round trips).  A tile element accumulates its products in the same order as before
// (link by link, 4 columns per MFMA): bit-identical, also to the 128 x 128 kernel.  Rows >= ilimit and columns >= climit are not touched.
// FUSE (FrontMeta::tfuse): T is not read -- it was never assembled -- but FORMED here: the sum of the children's contributions, looked up through the inverse row
// maps and added in the children's list order exactly as the assembly kernels add them, minus the product; written once.  The contribution block of such a
// front crosses HBM twice (this store, the parent's load) instead of four times (assembly store, update load + store, parent's load).
// FUSE (FrontMeta::tfuse): the sum of the children's contributions to a wavefront's R x R block of 16 x 16 accumulator tiles -- element (r, q, g): front row fk + ib +
// 16 q + l15, front column fk + cb + 16 r + l4 + 4 g -- looked up through the inverse row maps and added in the children's list order exactly as the assembly kernels
// add them.  A child costs three dependent round trips -- its record, its row maps, its values -- and a front has 2 .. 6 of them (dozens on the first link of a 3-D
// separator chain, most of them a handful of rows: ChildMeta::rlo / rhi skip the row maps of a child that has no row in this block): on the levels of many fronts that
// chain, not the product, set the pace.  Software pipeline: while the values of child c are in flight the row maps of child c + 1 and the record of child c + 2 are
// requested (same additions in the same order).
template <int R, bool LEAN = false>
__device__ __forceinline__ void fused_children(const DevView& V, const int ch0, const int ch1, const int fk, const int ib, const int cb, const int ilimit, const int climit,
                                               double (&tv)[R][R][4])
{
    const int lane = threadIdx.x & 63, l15 = lane & 15, l4 = lane >> 4;
    auto rowmaps = [&](const ChildMeta& Cm, int (&ar)[R], int (&lc)[R][4]) {
        const int* inv = V.relinv + Cm.inv + fk;              // front row fk + i  ->  index among the child's update rows, or -1
        const bool on = !Cm.aliased && Cm.rhi >= fk + cb && Cm.rlo < fk + ib + 16 * R;      // (no row of the child in this block's rows or columns: every map entry would be -1)
#pragma unroll
        for (int q = 0; q < R; ++q) { const int i = ib + q * 16 + l15; ar[q] = (on && i < ilimit) ? inv[i] : -1; }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int g = 0; g < 4; ++g) { const int c = cb + r * 16 + l4 + 4 * g; lc[r][g] = (on && c < climit) ? inv[c] : -1; }
    };
    if (ch0 >= ch1) return;
    ChildMeta Cm = V.cmeta[ch0], Cn = V.cmeta[min(ch0 + 1, ch1 - 1)];
    int ar[R], lc[R][4], nar[R], nlc[R][4];
    rowmaps(Cm, ar, lc);
    for (int cp = ch0; cp < ch1; ++cp) {
        const double* C = V.cb + Cm.cb_off; const size_t ldc = (size_t)Cm.ldt;
        const bool skip = Cm.aliased != 0;
        double cv[R][R][4];
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int q = 0; q < R; ++q)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int c = cb + r * 16 + l4 + 4 * g, i = ib + q * 16 + l15;
                    cv[r][q][g] = (ar[q] >= 0 && lc[r][g] >= 0 && i >= c) ? C[ar[q] + (size_t)lc[r][g] * ldc] : 0.0;
                }
            if (r == 0 && cp + 1 < ch1) rowmaps(Cn, nar, nlc);                        // (behind the first part of this child's values, in front of the rest)
            if (LEAN && !skip) {      // (the 16-wavefront kernels: a quarter of the block at a time, 8 value registers instead of 32)
#pragma unroll
                for (int q = 0; q < R; ++q)
#pragma unroll
                    for (int g = 0; g < 4; ++g) tv[r][q][g] += cv[r][q][g];
            }
        }
        const ChildMeta Cnn = V.cmeta[min(cp + 2, ch1 - 1)];
        if (!LEAN && !skip) {
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int q = 0; q < R; ++q)
#pragma unroll
                    for (int g = 0; g < 4; ++g) tv[r][q][g] += cv[r][q][g];
        }
        Cm = Cn; Cn = Cnn;
#pragma unroll
        for (int q = 0; q < R; ++q) ar[q] = nar[q];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int g = 0; g < 4; ++g) lc[r][g] = nlc[r][g];
    }
}
template <bool FUSE = false>
__device__ __forceinline__ void group_update32(const DevView& V, const int gbase, const int j0, const int jlast, const int mu, const int i0, const int cc0,
                                               const int ilimit, const int climit, double* T, const size_t ldt, const int fk = 0, const int ch0 = 0, const int ch1 = 0)
{
    const int lane = threadIdx.x & 63;
    const int l15 = lane & 15, l4 = lane >> 4;
    v4f64 acc[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[r][q] = (v4f64){0.0, 0.0, 0.0, 0.0};
    const int ca = cc0 + l15, cb_ = cc0 + 16 + l15, ia = i0 + l15, ib = i0 + 16 + l15;
    const bool vca = ca < mu, vcb = cb_ < mu, via = ia < mu, vib = ib < mu;
    GroupLink G = V.gtab[gbase + j0];
    int jf = j0, pf = 0;                                   // the next chunk to fetch: link, first column
    double xa0[4], xa1[4], xb0[4], xb1[4], ya0[4], ya1[4], yb0[4], yb1[4];      // two register stages (statically named)
    int xk = 0, xp = 0, yk = 0, yp = 0;                    // the link's k and the first column of the chunk a stage holds
    auto fetch = [&](double (&a0)[4], double (&a1)[4], double (&b0)[4], double (&b1)[4], int& ck, int& cp) -> bool {
        if (jf > jlast) return false;
        const double* Lp = V.L + G.panel_off + (G.m - mu);
        const double* Wp = V.wbuf + G.wb + (G.m - mu);
        ck = G.k; cp = pf;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int pk = pf + 4 * u + l4;
            const bool v = pk < G.k;
            const size_t off = (size_t)pk * G.m, offp = (size_t)pk * G.ldp;
            a0[u] = (v && vca) ? Wp[ca + off] : 0.0;
            a1[u] = (v && vcb) ? Wp[cb_ + off] : 0.0;
            b0[u] = (v && via) ? Lp[ia + offp] : 0.0;
            b1[u] = (v && vib) ? Lp[ib + offp] : 0.0;
        }
        pf += 16;
        if (pf >= G.k) { ++jf; pf = 0; if (jf <= jlast) G = V.gtab[gbase + jf]; }
        return true;
    };
    auto mma = [&](const double (&a0)[4], const double (&a1)[4], const double (&b0)[4], const double (&b1)[4], const int ck, const int cp) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (cp + 4 * u < ck) {
                acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[u], b0[u], acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[u], b1[u], acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[u], b0[u], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[u], b1[u], acc[1][1], 0, 0, 0);
            }
    };
    bool hx = fetch(xa0, xa1, xb0, xb1, xk, xp);
    while (hx) {
        const bool hy = fetch(ya0, ya1, yb0, yb1, yk, yp);
        mma(xa0, xa1, xb0, xb1, xk, xp);
        if (!hy) break;
        hx = fetch(xa0, xa1, xb0, xb1, xk, xp);
        mma(ya0, ya1, yb0, yb1, yk, yp);
    }
    double tv[2][2][4];
    if (FUSE) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int g = 0; g < 4; ++g) tv[r][q][g] = 0.0;
        fused_children<2>(V, ch0, ch1, fk, i0, cc0, ilimit, climit, tv);
    } else {
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = cc0 + r * 16 + l4 + 4 * g, i = i0 + q * 16 + l15;
                tv[r][q][g] = (i < ilimit && c < climit && i >= c) ? T[i + (size_t)c * ldt] : 0.0;
            }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = cc0 + r * 16 + l4 + 4 * g, i = i0 + q * 16 + l15;
                if (i < ilimit && c < climit && i >= c) T[i + (size_t)c * ldt] = tv[r][q][g] - acc[r][q][g];
            }
}

// 64 x 64 tile of the trailing update on one 256-thread workgroup (k_big_schur64; also the narrow updates fused into k_big_diag_trsm)
__device__ __forceinline__ void schur64_tile(const DevView& V, const FrontMeta& M, const int t, const int mode)      // mode 0: every tile, 1: tile (0,0) only (look-ahead), 2: all but it
{
    const int k = M.k, m = M.m;
    const int mu = m - k;
    const int nt = (mu + 63) >> 6;
    if ((mode == 2 && t == 0) || (mode == 1 && t != 0)) return;
    int ti, tc, climit, j0;
    if (M.grem > 0) {
        const int ntc = (M.grem + 63) >> 6;
        if (t >= nt * ntc) return;
        ti = t / ntc; tc = t - ti * ntc; climit = M.grem; j0 = M.gpos;
    } else {
        if (t >= nt * (nt + 1) / 2) return;
        ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
        while (ti * (ti + 1) / 2 > t) --ti;
        while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
        tc = t - ti * (ti + 1) / 2; climit = mu; j0 = 0;
    }
    const int wave = threadIdx.x >> 6;
    const int i0 = ti * 64 + (wave >> 1) * 32, cc0 = tc * 64 + (wave & 1) * 32;
    if (i0 + 31 < cc0 || cc0 >= climit || i0 >= mu) return;
    if (M.tfuse) {      // (host: such a front only ever sees mode 0; the children are those of the group's FIRST link -- the front itself unless it ends a chain group)
        const GroupLink G0 = V.gtab[M.gbase];
        group_update32<true>(V, M.gbase, j0, M.gpos, mu, i0, cc0, mu, climit, V.cb + M.cb_off, (size_t)M.ldt, G0.m - mu, G0.ch0, G0.ch1);
    }
    else group_update32(V, M.gbase, j0, M.gpos, mu, i0, cc0, mu, climit, V.cb + M.cb_off, (size_t)M.ldt);
}


// the same tile for a NARROW update on the serial chain (this link's k <= 64 columns only): every operand of the product is
// requested before the first MFMA -- behind the panel workgroups' flag each dependent access is a ~2 us trip to another XCD's data
__device__ __forceinline__ void narrow_tile64(const DevView& V, const FrontMeta& M, const int t)
{
    const int k = M.k, m = M.m;
    const int mu = m - k;
    const int nt = (mu + 63) >> 6, ntc = (M.grem + 63) >> 6;
    if (t >= nt * ntc) return;
    const int ti = t / ntc, tc = t - ti * ntc, climit = M.grem;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = ti * 64 + (wave >> 1) * 32, cc0 = tc * 64 + (wave & 1) * 32;
    if (i0 + 31 < cc0 || cc0 >= climit || i0 >= mu) return;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int ca = cc0 + l15, cb_ = cc0 + 16 + l15, ia = i0 + l15, ib = i0 + 16 + l15;
    const GroupLink G = V.gtab[M.gbase + M.gpos];
    const int kj = G.k;
    const double* Lp = V.L + G.panel_off + (G.m - mu);
    const double* Wp = V.wbuf + G.wb + (G.m - mu);
    double a0[16], a1[16], b0[16], b1[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int pk = 4 * u + l4;
        const bool v = pk < kj;
        const size_t off = (size_t)pk * G.m, offp = (size_t)pk * G.ldp;
        a0[u] = (v && ca < mu) ? Wp[ca + off] : 0.0;
        a1[u] = (v && cb_ < mu) ? Wp[cb_ + off] : 0.0;
        b0[u] = (v && ia < mu) ? Lp[ia + offp] : 0.0;
        b1[u] = (v && ib < mu) ? Lp[ib + offp] : 0.0;
    }
    double* T = V.cb + M.cb_off;
    double tv[2][2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = cc0 + r * 16 + l4 + 4 * g, i = i0 + q * 16 + l15;
                tv[r][q][g] = (i < mu && c < climit && i >= c) ? T[i + (size_t)c * M.ldt] : 0.0;
            }
    v4f64 acc[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[r][q] = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < 16; ++u)
        if (4 * u < kj) {
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[u], b0[u], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[u], b1[u], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[u], b0[u], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[u], b1[u], acc[1][1], 0, 0, 0);
        }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = cc0 + r * 16 + l4 + 4 * g, i = i0 + q * 16 + l15;
                if (i < mu && c < climit && i >= c) T[i + (size_t)c * M.ldt] = tv[r][q][g] - acc[r][q][g];
            }
}

// Pivot block AND panel solve of a front in ONE launch (the top of the tree, where a level has a handful of fronts and both
// kernels are a chain of dependent round trips rather than work): workgroup 0 of a front is the pivot-block kernel and raises the
// front's flag as soon as L11 and D are stored (its inverse follows, off the critical path); workgroups 1.. each own 64 panel
// rows, add their A entries and stage their rows in LDS BEFORE they wait, then permute / solve / scale.  Same arithmetic as
// k_big_diag_reg + k_big_trsm, bit for bit.
__global__ __launch_bounds__(256) void k_big_diag_trsm(DevView V, int list_off, int nrb)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const FrontMeta M = V.fmeta[list_off + blockIdx.x];      // x = front, y = role: every pivot block is dispatched before the first waiting workgroup
    const int role = blockIdx.y;
    const int epoch = V.sepoch[2];
#ifdef MI355X_PIVSTAT
    const bool tprobe = gridDim.x == 1 && threadIdx.x == 0;
    if (tprobe && role == 0) g_dt[0] = wall_clock64();
    if (tprobe && role == 1) g_dt[6] = wall_clock64();
#endif
    if (role == 0) { big_diag_body<4, 256>(V, M, smem_raw, &V.sflag_d[M.s], epoch, nullptr, nullptr, FrontMeta(), 0, 0, V.norestore ? &V.sflag_p[M.s] : nullptr); return; }
    const int tid = threadIdx.x;
    const int s = M.s, k = M.k, m = M.m;
    if (role > nrb) {
        // workgroups behind the panel blocks: the NARROW trailing update of a chain link that is not the last of its group (64 x 64
        // tiles over the group's remaining panel columns: a fraction of a GFlop, not worth a launch of its own on the serial chain)
        const int t = role - 1 - nrb;
        const int mu = m - k, nt = (mu + 63) >> 6;
        if (M.grem <= 0 || t >= nt * ((M.grem + 63) >> 6)) return;
        if (tid == 0) {
            int spins = 0;
            while (__hip_atomic_load(&V.tcnt[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < nt) { __builtin_amdgcn_s_sleep(16);      // (~0.4 us: a hundred pollers of one address must not saturate its memory channel)
                if (++spins > (1 << 24)) { V.qstat[1] = 1; break; } }
        }
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        narrow_tile64(V, M, t);
        return;
    }
    const int ibase = k + (role - 1) * 64;
    if (ibase >= m) return;
    double* P = V.L + M.panel_off;
    const size_t ldp = (size_t)M.ldp;
    if (M.selfasm) {
        for (int q = M.aq0 + tid; q < M.aq1; q += 256) { const int pos = V.apos[q]; const int i = pos % m, c = pos / m; if (i >= ibase && i < ibase + 64) P[i + (size_t)c * ldp] += V.aval[q]; }
        __syncthreads();
    }
    const TrsmLds T = trsm_layout(smem_raw, k, true);
    if (V.norestore) {
        // optimistic schedule: the panel rows are solved in step with the blocked factorisation of the pivot block, 16 columns at a time (trsm_rows_pipe:
        // natural pivot order, so the rows go straight into the working block); a pivot block the a-posteriori test rejects makes factor() repeat everything
        for (int idx = tid; idx < 64 * T.kp16; idx += 256) { const int r = idx & 63, c = idx >> 6; T.As[r + c * 65] = (c < k && ibase + r < m) ? P[ibase + r + (size_t)c * ldp] : 0.0; }
        __syncthreads();
        trsm_rows_pipe(V, M, T, ibase, 64, 3, 8 * epoch, false, nullptr, 0, 0);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __syncthreads();
        if (tid == 0) __hip_atomic_fetch_add(&V.tcnt[s], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    for (int idx = tid; idx < 64 * k; idx += 256) { const int r = idx & 63, c = idx >> 6; T.Au[r + c * 65] = (ibase + r < m) ? P[ibase + r + (size_t)c * ldp] : 0.0; }
#ifdef MI355X_PIVSTAT
    if (tprobe && role == 1) g_dt[7] = wall_clock64();
#endif
    chain_wait(&V.sflag_d[s], epoch, V.qstat + 1);            // L11 and D of this front are stored
#ifdef MI355X_PIVSTAT
    if (tprobe && role == 1) g_dt[8] = wall_clock64();
#endif
    trsm_rows_impl<true>(V, M, T, ibase);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");       // my rows of L21 / W21 are stored: one more panel block done
    __syncthreads();
    if (tid == 0) __hip_atomic_fetch_add(&V.tcnt[s], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#ifdef MI355X_PIVSTAT
    if (tprobe && role == 1) {
        const unsigned long long te = wall_clock64(), t0 = g_dt[0];
        for (int q = 1; q <= 8; ++q) if (q != 3 && q != 4) g_dtacc[q] += g_dt[q] - t0;
        g_dtacc[9] += te - t0; g_dtacc[0] += 1;
        for (int q = 10; q <= 12; ++q) g_dtacc[q] += g_dt[q] - t0;
    }
#endif
}

// T(i,c) -= sum_p L21(i,p) W21(c,p),  i >= c, on 64x64 tiles; each of the 4 waves owns a 32x32 sub-tile made of
// 2x2 v_mfma_f64_16x16x4_f64 accumulators.  The product is formed TRANSPOSED (A operand = W rows, B operand = L rows)
// so that the 16 lanes sharing an accumulator register hold 16 consecutive ROWS of the column-major T => 128-byte
// coalesced read-modify-write segments.
// Chain groups: a link that is not the last of its group only updates the group's remaining `grem` columns (the panels
// of the later links); the LAST link applies the update of ALL the group's panels to its contribution block in one
// pass (K = sum of the links' columns, <= 256), so the block is read and written once per group instead of once per link.
// Look-ahead: the update of a group-last front whose chain continues may be SPLIT (FrontMeta::split): part 1 = the first two
// tile columns (all that the next group's panels, pivot blocks and narrow updates touch) stays on the main stream, part 2 =
// the rest runs on a second stream, overlapped with the latency-bound pivot chains of the next group.  part 0 = everything.
constexpr int SCHUR_KC = 16, SCHUR_LD = 132;
// the tile itself: TS x TS on 16 wavefronts, TS = 128 (32 x 32 = 2 x 2 accumulators per wavefront) or 64 (16 x 16: a launch of a few dozen 128-tiles -- the
// part-1 launches at the top of the tree -- is spread over four times the CUs, 6.8 instead of 27 us of MFMA time per workgroup)
template <int TS, int TCW = TS, int NT = 1024, int LD = SCHUR_LD>
__device__ __forceinline__ void schur_tile_body(const DevView& V, const FrontMeta& M, const int i0, const int cc0, const int climit, const int j0, const int skip00,
                                                double (&As)[2][SCHUR_KC][LD], double (&Bs)[2][SCHUR_KC][LD])
{
    // TS rows x TCW columns of the trailing matrix on NT threads (TCW < TS: the 128 x 64 tile of 512 threads -- two workgroups per CU, one in its
    // read-modify-write epilogue while the other multiplies)
    constexpr int KC = SCHUR_KC;
    const int mu = M.m - M.k;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    constexpr int WT = (TS == TCW && NT == 1024) ? TS / 4 : 32, R = WT / 16, WC = TCW / WT;      // a wavefront's block of the tile: WT x WT = R x R accumulators; WC wavefronts side by side (64 x 64 on 256 threads: 32 x 32 each, as in the 128 x 128 tile)
    static_assert((TS / WT) * WC * 64 == NT, "wavefront grid does not cover the tile");
    const int wr = (wave / WC) * WT, wc = (wave % WC) * WT;
    // skip00: the leading 64 x 64 block of the trailing matrix (the NEXT link's pivot block) was already updated by the look-ahead launch
    const bool work = (i0 + wr + WT - 1 >= cc0 + wc) && (cc0 + wc < climit) && (i0 + wr < mu) && !(skip00 && i0 + wr < 64 && cc0 + wc < 64);
    v4f64 acc[R][R];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < R; ++q) acc[r][q] = (v4f64){0.0, 0.0, 0.0, 0.0};
    // staging role of this thread: L row (tid % TS) of the tile, panel columns (tid / TS) + SCB u of the chunk, u < UB; W row (tid % TCW), columns (tid / TCW) + SCA u, u < UA
    constexpr int SCB = NT / TS, UB = KC / SCB, SCA = NT / TCW, UA = KC / SCA;
    const int srowb = tid % TS, scolb = tid / TS, srowa = tid % TCW, scola = tid / TCW;
    const bool arow_ok = cc0 + srowa < mu, brow_ok = i0 + srowb < mu;
    // software pipeline of depth 2 over the 16-column chunks: while chunk i is multiplied out of LDS, chunk i+1 sits in registers on its
    // way to LDS and chunk i+2 is in flight from L2 / HBM -- on the chain levels a launch is a handful of workgroups and the per-chunk
    // cost is the load latency, not the 16 MFMAs; the link record (gtab) is re-read only when the link changes, not once per chunk.
    // (The order in which a tile element accumulates its products is unchanged: results are bit-identical.)
    GroupLink Gc = V.gtab[M.gbase + j0];
    int gj = j0;
    double ga0[UA], gb0[UB], ga1[UA], gb1[UB];             // two register stages (statically named: no indexed register arrays)
    auto fetch = [&](int j, int p0, double (&ga)[UA], double (&gb)[UB]) {
        if (j != gj) { Gc = V.gtab[M.gbase + j]; gj = j; }
        const double* Lp = V.L + Gc.panel_off + (Gc.m - mu) + i0 + srowb;
        const double* Wp = V.wbuf + Gc.wb + (Gc.m - mu) + cc0 + srowa;
#pragma unroll
        for (int u = 0; u < UA; ++u) { const int pk = p0 + scola + SCA * u; ga[u] = (pk < Gc.k && arow_ok) ? Wp[(size_t)pk * Gc.m] : 0.0; }
#pragma unroll
        for (int u = 0; u < UB; ++u) { const int pk = p0 + scolb + SCB * u; gb[u] = (pk < Gc.k && brow_ok) ? Lp[(size_t)pk * Gc.ldp] : 0.0; }
    };
    // chunk sequence: (link j, first column p), j = j0 .. M.gpos, p = 0, KC, ... < k_j.  advance() is called right after the fetch of
    // chunk (j, p), so the cached link record is that of j.
    auto advance = [&](int& j, int& p) -> bool { p += KC; if (p >= Gc.k) { ++j; p = 0; } return j <= M.gpos; };
    auto to_lds = [&](int b, const double (&ga)[UA], const double (&gb)[UB]) {
#pragma unroll
        for (int u = 0; u < UA; ++u) As[b][scola + SCA * u][srowa] = ga[u];
#pragma unroll
        for (int u = 0; u < UB; ++u) Bs[b][scolb + SCB * u][srowb] = gb[u];
    };
    auto multiply = [&](int b) {
        if (!work) return;
#pragma unroll
        for (int st = 0; st < KC / 4; ++st) {
            const int kk = 4 * st + l4;
            double av[R], bv[R];
#pragma unroll
            for (int r = 0; r < R; ++r) { av[r] = As[b][kk][wc + 16 * r + l15]; bv[r] = Bs[b][kk][wr + 16 * r + l15]; }
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int q = 0; q < R; ++q) acc[r][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[r], bv[q], acc[r][q], 0, 0, 0);
        }
    };
    int jn = j0, pn = 0;                   // the chunk most recently fetched
    fetch(jn, pn, ga0, gb0);
    to_lds(0, ga0, gb0);                   // chunk 0 -> LDS
    bool have1 = advance(jn, pn);          // chunk 1 exists -> stage 0
    if (have1) fetch(jn, pn, ga0, gb0);
    bool have2 = have1 && advance(jn, pn); // chunk 2 exists -> stage 1
    if (have2) fetch(jn, pn, ga1, gb1);
    __syncthreads();
    while (true) {
        multiply(0);
        if (!have1) break;
        to_lds(1, ga0, gb0);
        have1 = have2;
        if (have2) { have2 = advance(jn, pn); if (have2) fetch(jn, pn, ga0, gb0); }
        __syncthreads();
        multiply(1);
        if (!have1) break;
        to_lds(0, ga1, gb1);
        have1 = have2;
        if (have2) { have2 = advance(jn, pn); if (have2) fetch(jn, pn, ga1, gb1); }
        __syncthreads();
    }
    if (!work) return;
    double* T = V.cb + M.cb_off;
    double tv[R][R][4];
    if (M.tfuse) {      // (workgroup-uniform) T was never assembled: it is FORMED here, the sum of the children's contributions minus the product -- see fused_children
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int q = 0; q < R; ++q)
#pragma unroll
                for (int g = 0; g < 4; ++g) tv[r][q][g] = 0.0;
        const GroupLink G0 = V.gtab[M.gbase];
        fused_children<R, true>(V, G0.ch0, G0.ch1, G0.m - mu, i0 + wr, cc0 + wc, mu, climit, tv);
    } else {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < R; ++q)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = cc0 + wc + r * 16 + l4 + 4 * g;      // D row index  -> T column
                const int i = i0 + wr + q * 16 + l15;              // D column index -> T row
                tv[r][q][g] = (i < mu && c < climit && i >= c) ? T[i + (size_t)c * M.ldt] : 0.0;
            }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < R; ++q)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = cc0 + wc + r * 16 + l4 + 4 * g;
                const int i = i0 + wr + q * 16 + l15;
                if (i < mu && c < climit && i >= c) T[i + (size_t)c * M.ldt] = tv[r][q][g] - acc[r][q][g];
            }
}
// SCHUR_HALVES = 2: a 128 x 128 tile is worked as two 128 x 64 halves by two 512-thread workgroups (k_big_schur's launches then carry twice the
// workgroups; the halves of a tile get the same workgroup id modulo 8, i.e. the same XCD and its L2 copy of the tile's L rows)
#ifdef MI355X_SCHUR_HALVES
constexpr int SCHUR_GM = 2, SCHUR_NT = 512;
#else
constexpr int SCHUR_GM = 1, SCHUR_NT = 1024;
#endif
__device__ __forceinline__ void schur_tile(const DevView& V, const FrontMeta& M, const int t, const int half, const int part, const int skip00,
                                           double (&As)[2][SCHUR_KC][SCHUR_LD], double (&Bs)[2][SCHUR_KC][SCHUR_LD])
{
    // 128 x 128 tile per workgroup of 16 wavefronts (32 x 32 each = 2 x 2 accumulators of v_mfma_f64_16x16x4_f64).  The
    // operands are staged through LDS in chunks of 16 panel columns (double buffered, one barrier per chunk): every panel
    // entry is fetched from L2 once per tile instead of once per wavefront, and 4 wavefronts per SIMD hide the LDS latency.
    const int k = M.k, m = M.m;
    const int mu = m - k;
    const int nt = (mu + 127) >> 7;
    int ti, tc, climit, j0;
    const bool sp = part != 0 && M.split != 0;
    if (part == 2 && !sp) return;
    if (M.grem > 0) {
        const int ntc = (M.grem + 127) >> 7;
        if (t >= nt * ntc) return;
        ti = t / ntc; tc = t - ti * ntc; climit = M.grem; j0 = M.gpos;
        if (ti < tc) return;
    } else if (sp && part == 1) {
        if (t >= 2 * nt - 1) return;
        if (t < nt) { ti = t; tc = 0; } else { ti = t - nt + 1; tc = 1; }
        climit = mu; j0 = 0;
    } else {
        const int n2 = sp ? nt - 2 : nt, sh = sp ? 2 : 0;
        const int ntri = n2 * (n2 + 1) / 2;
        const int tab = sp ? M.ttab2 : M.ttab;
        if (tab >= 0) {
            // large update: workgroups are dealt to the 8 XCDs round-robin (linear id mod 8), so XCD x walks the x-th
            // contiguous eighth of a super-tile ordered list (8 x 8 tile blocks): the ~64 tiles in flight on one XCD share
            // 16 panel row blocks, which its 4 MB L2 holds, instead of streaming the whole panel from the fabric per tile
            const int chunk = (ntri + 7) >> 3;
            const int pos = (t & 7) * chunk + (t >> 3);
            if ((t >> 3) >= chunk || pos >= ntri) return;
            const int e = V.tile_tab[tab + pos];
            ti = e >> 16; tc = e & 0xffff;
        } else {
            if (t >= ntri) return;
            ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
            while (ti * (ti + 1) / 2 > t) --ti;
            while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
            tc = t - ti * (ti + 1) / 2;
        }
        climit = mu; j0 = 0;
        ti += sh; tc += sh;
    }
    if constexpr (SCHUR_GM == 2) schur_tile_body<128, 64, 512>(V, M, ti * 128, tc * 128 + half * 64, climit, j0, skip00, As, Bs);
    else schur_tile_body<128>(V, M, ti * 128, tc * 128, climit, j0, skip00, As, Bs);
}
// part 0 / 1: one tile per workgroup.  part 2 (look-ahead, second stream) strides over the tiles, normally also one per
// workgroup (a persistent grid smaller than the chip was measured: one 16-wave workgroup per CU reaches half the MFMA rate).
__global__ __launch_bounds__(SCHUR_NT, 4) void k_big_schur(DevView V, int list_off, int part, int ntiles, int skip00)
{
    __shared__ double As[2][SCHUR_KC][SCHUR_LD];      // W rows (-> T columns) of the tile
    __shared__ double Bs[2][SCHUR_KC][SCHUR_LD];      // L rows (-> T rows)
    const FrontMeta M = V.fmeta[list_off + blockIdx.y];
    if (part == 4) { if (M.split) return; part = 0; }      // (part 4: the fronts that are NOT split -- the split ones' part 1 is k_big_schur_p1's)
    // virtual workgroup id -> (tile, half): id = 16 a + 8 h + x  ->  tile 8 a + x, half h
    auto split_id = [](int id, int& t, int& h) { if (SCHUR_GM == 2) { t = ((id >> 4) << 3) + (id & 7); h = (id >> 3) & 1; } else { t = id; h = 0; } };
    int t, h;
    if (part != 2) { split_id(blockIdx.x, t, h); schur_tile(V, M, t, h, part, skip00, As, Bs); return; }
    if (!M.split) return;
    const int nvirt = SCHUR_GM == 2 ? ((ntiles + 7) >> 3) << 4 : ntiles;
    for (int id = blockIdx.x; id < nvirt; id += gridDim.x) { split_id(id, t, h); if (t < ntiles) schur_tile(V, M, t, h, part, 0, As, Bs); __syncthreads(); }
}

// Part 1 of the split updates (the first 256 columns of the trailing matrix: what the next chain group reads) in 64 x 64 tiles.  At the top of the tree a
// part-1 launch is a few dozen 128 x 128 tiles with K = 256 -- 27 us of MFMA time each on ONE CU while most of the chip idles, on the critical path
// between two groups (measured 43-51 us per launch); four times the workgroups of a quarter of the work each.  Same sums in the same order.
__global__ __launch_bounds__(1024) void k_big_schur_p1(DevView V, int list_off)
{
    __shared__ double As[2][SCHUR_KC][SCHUR_LD];
    __shared__ double Bs[2][SCHUR_KC][SCHUR_LD];
    const FrontMeta M = V.fmeta[list_off + blockIdx.y];
    if (!M.split || M.grem > 0) return;
    const int mu = M.m - M.k, nt = (mu + 63) >> 6;
    int t = blockIdx.x, tc = 0;
    while (tc < 4 && tc < nt && t >= nt - tc) { t -= nt - tc; ++tc; }      // tile column tc < 4 holds the tile rows tc .. nt - 1
    if (tc >= 4 || tc >= nt) return;
    schur_tile_body<64>(V, M, (tc + t) * 64, tc * 64, mu, 0, 0, As, Bs);
}

// Part 2 of the split updates in QUARTER tiles on small workgroups (round 5).  Part 2 runs on the second stream next to the NEXT group's k_grp_fused, and that
// launch pins one CU per workgroup: 386 VGPRs and up to 143 KB of LDS each (188 of the 256 CUs with four fronts on a level).  A 16-wavefront workgroup of
// k_big_schur needs 4 x 96 VGPRs per SIMD and 66 KB of LDS: it cannot share a CU with them and gets the CUs that are left -- the part-2 launches of the
// levels with 4-8 chains ran at ~26 TFLOP/s where the same kernel alone reaches 42, and they ARE the critical path there (the next part 1 reads what they
// write).  Here a workgroup is 4 wavefronts (one per SIMD) on a 64 x 64 quarter of a 128 x 128 tile:
//   k_big_schur_q   the LDS-staged tile body on 256 threads (35 KB of LDS).  (A variant with the operands straight from L2, no LDS at all, measured slower: removed.)
// Tile order = the 128-tile order of k_big_schur (the XCD-aware table; the four quarters of a tile on the same XCD).  Same sums in the same order.
__device__ __forceinline__ bool part2_tile(const DevView& V, const FrontMeta& M, const int t, int& ti, int& tc)
{
    const int mu = M.m - M.k, nt = (mu + 127) >> 7, n2 = nt - 2;
    if (n2 <= 0) return false;
    const int ntri = n2 * (n2 + 1) / 2;
    if (M.ttab2 >= 0) {
        const int chunk = (ntri + 7) >> 3;
        const int pos = (t & 7) * chunk + (t >> 3);
        if ((t >> 3) >= chunk || pos >= ntri) return false;
        const int e = V.tile_tab[M.ttab2 + pos];
        ti = e >> 16; tc = e & 0xffff;
    } else {
        if (t >= ntri) return false;
        ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
        while (ti * (ti + 1) / 2 > t) --ti;
        while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
        tc = t - ti * (ti + 1) / 2;
    }
    ti += 2; tc += 2;
    return true;
}
constexpr int SCHURQ_LD = 68;
// virtual workgroup id -> (tile, quarter): id = 32 a + 8 q + x  ->  tile 8 a + x (XCD x, as in k_big_schur), quarter q
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(120))) void k_big_schur_q(DevView V, int list_off, int ntiles)
{
    __shared__ double As[2][SCHUR_KC][SCHURQ_LD];
    __shared__ double Bs[2][SCHUR_KC][SCHURQ_LD];
    const FrontMeta M = V.fmeta[list_off + blockIdx.y];
    if (!M.split || M.grem > 0) return;
    const int mu = M.m - M.k;
    const int nvirt = ((ntiles + 7) >> 3) << 5;
    for (int id = blockIdx.x; id < nvirt; id += gridDim.x) {
        const int t = ((id >> 5) << 3) + (id & 7), q = (id >> 3) & 3;
        int ti, tc;
        if (t >= ntiles || !part2_tile(V, M, t, ti, tc)) continue;
        const int i0 = ti * 128 + (q & 1) * 64, cc0 = tc * 128 + (q >> 1) * 64;
        if (i0 + 63 < cc0 || i0 >= mu || cc0 >= mu) continue;
        schur_tile_body<64, 64, 256, SCHURQ_LD>(V, M, i0, cc0, mu, 0, 0, As, Bs);
        __syncthreads();
    }
}

// Small-front variant of the trailing update (levels whose largest front has <= 640 rows: thousands of fronts, a handful
// of tiles each): 64 x 64 tile per 256-thread workgroup, 32 x 32 per wavefront, operands straight from L2.  The 128 x 128
// LDS-staged kernel above leaves most of its 16 wavefronts idle on such fronts (PMC: 7.6 % MFMA utilisation).
__global__ __launch_bounds__(256, 4) void k_big_schur64(DevView V, int list_off, int mode)
{
    int tx = blockIdx.x, fy = blockIdx.y;
    if (V.xcd_affine) xcd_affine(tx, fy);
    const FrontMeta M = V.fmeta[list_off + fy];
    schur64_tile(V, M, tx, mode);
}


// ================================================================================================
// CHAIN GROUPS FACTORED AS ONE UNIT.  A chain group = up to 4 consecutive links of an in-place separator chain (<= 256 columns); every
// link after the first has the chain child as its ONLY child, so the whole group can be factored at the tree level of its first link:
// one launch for the group's leading block and all its panel rows (k_grp_fused), then the rank-(<= 256) update of the contribution block
// by all the group's panels (k_big_schur, unchanged).  (A two-launch variant -- one 512-thread workgroup walking the leading block link by
// link, row blocks behind it -- was built first and measured slower: 210 us per group, a lone wavefront issues one fp64 MFMA per ~150
// cycles; removed.)
// ================================================================================================
// A chain group as ONE launch of row-block workgroups (the default of the grouped schedule): grid = (groups, 4 + row blocks below the
// group).  Role q < 4 owns the pivot rows of the group's link q, role 4 + b the b-th block of 64 rows below the group's columns.  A
// row block walks the links p before its own (all of them for the rows below): rows staged in LDS, wait for link p's pivot block
// (flag), solve against it (k_big_trsm's arithmetic), publish W / L of its rows (flag), then update its own rows' entries in the
// columns of the later links r, waiting per r for the rows that hold W(r, p).  A pivot-row block then factors its own pivot block
// (big_diag_body: blocked a-posteriori LDL^T or the strict loop) and raises the flag the blocks after it wait for.  Every wait is on
// a workgroup with a SMALLER role of the same group: with workgroups dispatched in linear order (roles are the slow grid dimension)
// a waiting workgroup never holds up the one it waits for; the spins are bounded all the same (qstat[1]).
// Critical path per link: pivot block -> flag -> one 64 x 64 panel solve -> one 64 x 64 x 64 update -> next pivot block.
constexpr size_t GRP_DB_BYTES = (size_t)64 * 65 * sizeof(double);      // a pivot-row block's own pivot block, LDS-resident from the start of the launch
// rbw: 64-row blocks per row-block workgroup.  A workgroup of this kernel has a CU to itself (385 VGPRs, 110-143 KB of LDS), and one that arrives when
// the chip is full starts only when another one has walked ALL its links: a level with 8 groups of ~47 row blocks (408 workgroups) took 374 us
// against 190 us for 4 groups.  The host picks rbw so that a launch fits the chip; a workgroup then takes its rbw blocks one after the other
// against every link (the blocks below the group are not on the critical chain of the pivot rows).
// role0: first role of the launch (0: the fused form, grid.y = 4 + row-block workgroups -- the only form in use; cutting the launch in two next to a running part-2
// update, pivot-row blocks first, was measured and is gone).
__device__ __forceinline__ void grp_fused_body(const DevView& V, const int list_off, const int staged_arg, const int rbw, const int role0)
{
    const int staged = staged_arg;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const FrontMeta M = V.fmeta[list_off + blockIdx.x];              // the LAST link of the group
    const int g = M.gpos + 1, role = (int)blockIdx.y + role0;
    const int tail = M.m - M.k;                                      // rows below the group's columns
    int myq = -1, eb0 = 0, nsub = 1;
    if (role < 4) { if (role >= g) return; myq = role; }
    else { eb0 = 64 * rbw * (role - 4); if (eb0 >= tail) return; nsub = min(rbw, (tail - eb0 + 63) >> 6); }
    const int epoch = V.sepoch[2];
#define GSTAMP(i) do { if (V.dbg && blockIdx.x == 0 && role < 4 && tid == 0) V.dbg[32 + 8 * role + (i)] = wall_clock64(); } while (0)
    GSTAMP(0);
    unsigned long long tsv[28];
#pragma unroll
    for (int q = 0; q < 28; ++q) tsv[q] = 0ull;
    unsigned long long* const tsp = (V.dbg && blockIdx.x == 0 && role == 1) ? tsv : nullptr;
    int kk[4], koff[5];
    koff[0] = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { kk[j] = (j < g) ? V.gtab[M.gbase + j].k : 0; koff[j + 1] = koff[j] + kk[j]; }
    const int last_p = (myq >= 0) ? myq - 1 : g - 1;
    int myrows = min(64, tail - eb0), mystart = M.gcols + eb0;        // my rows, counted from the first column of the group (a row-block workgroup: its first block)
#pragma unroll
    for (int j = 0; j < 4; ++j) if (j == myq) { myrows = kk[j]; mystart = koff[j]; }
    // ---- a pivot-row block keeps its own pivot block in LDS (lower triangle) from the start: the updates of the links before it
    //      are applied there, the factorisation at the end reads it there -- the block never makes a round trip through L2 ----
    double* Db = reinterpret_cast<double*>(smem_raw);
    const int ldb = myrows | 1;
    GroupLink Gq = V.gtab[M.gbase];
    if (myq >= 0) {
#pragma unroll
        for (int j = 1; j < 4; ++j) if (j == myq) Gq = V.gtab[M.gbase + j];
        const double* Pq = V.L + Gq.panel_off;
        const size_t ldq = (size_t)Gq.ldp;
        const int i = tid & 63, cq = tid >> 6, kq = Gq.k;
        double pv[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) { const int c = cq + 4 * e; pv[e] = (i < kq && c < kq && i >= c) ? Pq[i + (size_t)c * ldq] : 0.0; }
#pragma unroll
        for (int e = 0; e < 16; ++e) { const int c = cq + 4 * e; if (i < kq && c < kq && i >= c) Db[i + c * ldb] = pv[e]; }
        __syncthreads();
        if (Gq.selfasm) {
            for (int q = Gq.aq0 + tid; q < Gq.aq1; q += 256) { const int pos = V.apos[q]; const int ii = pos % Gq.m, cc = pos / Gq.m; if (ii < kq) Db[ii + cc * ldb] += V.aval[q]; }
            __syncthreads();
        }
    }
    char* tsm = smem_raw + GRP_DB_BYTES;
    const double* crit_Lr = nullptr; FrontMeta crit_Mp = M; int crit_ibase = 0;      // the kept-back L21 of the last link before my pivot block
#pragma unroll 1
    for (int sub = 0; sub < nsub; ++sub) {      // (a row-block workgroup: its rbw blocks one after the other, each against every link; the first one keeps pace with the chain)
    if (myq < 0) { myrows = min(64, tail - (eb0 + 64 * sub)); mystart = M.gcols + eb0 + 64 * sub; }
    for (int p = 0; p <= last_p; ++p) {
        const GroupLink G = V.gtab[M.gbase + p];
        const int k = G.k, m = G.m;
        int kend = 0;                                                 // columns of the group up to and including link p
#pragma unroll
        for (int j = 0; j < 4; ++j) if (j == p) kend = koff[j + 1];
        const int ibase = k + (mystart - kend);                       // my first row in this link's front
        double* P = V.L + G.panel_off;
        const size_t ldp = (size_t)G.ldp;
        FrontMeta Mp = M;
        Mp.s = G.s; Mp.c0 = G.c0; Mp.k = k; Mp.m = m; Mp.panel_off = G.panel_off; Mp.ldp = G.ldp; Mp.wb = G.wb;
        const TrsmLds T = trsm_layout(tsm, k, staged != 0, false, true);      // (levels with hundreds of groups: no staging copy, more workgroups per CU)
        Mp.bigidx = G.bigidx;
        if (staged) {
            // my rows as they lie in the panel (and the link's own A entries for them) go to LDS before the pivot block is known --
            // straight into the working block: behind the blocked factorisation the pivot order is the panel's column order
            for (int idx = tid; idx < 64 * T.kp16; idx += 256) { const int r = idx & 63, c = idx >> 6; T.As[r + c * 65] = (c < k && r < myrows && ibase + r < m) ? P[ibase + r + (size_t)c * ldp] : 0.0; }
            if (G.selfasm) {
                __syncthreads();
                for (int q = G.aq0 + tid; q < G.aq1; q += 256) { const int pos = V.apos[q]; const int i = pos % m, c = pos / m; if (i >= ibase && i < ibase + myrows) T.As[(i - ibase) + c * 65] += V.aval[q]; }
            }
        } else if (G.selfasm) {
            for (int q = G.aq0 + tid; q < G.aq1; q += 256) { const int pos = V.apos[q]; const int i = pos % m, c = pos / m; if (i >= ibase && i < ibase + myrows) P[i + (size_t)c * ldp] += V.aval[q]; }
            __syncthreads();
        }
        const bool crit = staged && myq >= 0 && p == last_p;          // the link before my own pivot block: L21 of my rows goes to the panel AFTER my pivot block
        if (crit) { crit_Lr = T.Au; crit_Mp = Mp; crit_ibase = ibase; }
        const bool pipe = V.norestore != 0 && staged != 0;            // (workgroup-uniform) the panel solve in step with the pivot block's factorisation: trsm_rows_pipe
        if (pipe) {
            __syncthreads();                                          // (the staging of my rows above)
            trsm_rows_pipe(V, Mp, T, ibase, myrows, crit ? 1 : 3, 8 * epoch, myq >= 0, Db, ldb, myrows, crit ? tsp : nullptr);
        } else {
        chain_wait(&V.sflag_d[G.s], epoch, V.qstat + 1);              // L11, D, the pivot order (and the diagonal-block inverses) of link p are stored
        if (p == last_p) GSTAMP(1);
        if (tsp) tsp[4] = clock64();
        trsm_rows_impl<true, true>(V, Mp, T, ibase, myrows, tsp, staged != 0, crit ? 1 : 3);
        }
        if (p == last_p) GSTAMP(2);
        // W(my rows, p) and L(my rows, p) are stored: the blocks after me may use them.  On the critical iteration (the link before my own pivot block) the
        // signal -- wait for the stores' acknowledgements, release fence, flag: 4 300 cycles measured -- is raised BEHIND the update of my own block: the stores
        // complete while that update runs, and whoever waits for these rows needs them for a panel solve that cannot start before MY pivot block is factored.
        if (myq >= 0 && !crit) chain_signal_coh(&V.sflag_s[4 * G.s + myq], epoch);
        else __syncthreads();
        if (p == last_p) GSTAMP(3);
        if (tsp) tsp[5] = clock64();
        // my rows' entries in the columns of the later links:  T(i, c) -= sum_q L21(i, q) W21(c, q)
        {
            const double* Ds = T.Ds; const int* Ts = T.Ts; const double* As = T.As; const double* Lr = T.Au;
            auto lval = [&](const int r, const int q) -> double {
                if (Lr) return Lr[r + q * 65];                        // (kept by the panel solve)
                const int pt = Ts[q];
                const double wq = As[r + q * 65];
                if (pt == 1) return wq * Ds[q];
                if (pt == 2) return Ds[q] * wq + Ds[k + q] * As[r + (q + 1) * 65];
                return Ds[k + q - 1] * As[r + (q - 1) * 65] + Ds[q] * wq;
            };
            const int kp16 = T.kp16;
            const int rmax = (myq >= 0) ? myq : g - 1;
            // (a) the columns of OTHER links: W21 of their pivot rows comes from their row blocks (global), the target lives in L2
            if ((myq >= 0) ? (myq > p + 1) : (g - 1 > p)) {
                double bv[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) { const int qq = 4 * u + l4; bv[u] = (qq < k) ? lval(16 * wave + l15, qq) : 0.0; }
                double* Tt = V.cb + G.t_off;
                const size_t ldt = (size_t)G.ldt;
                const int irow = (mystart - kend) + 16 * wave + l15;  // my row in T
                const bool rowok = 16 * wave + l15 < myrows;
                for (int r = p + 1; r <= rmax; ++r) {
                    if (r == myq) continue;
                    int cs = 0, cn = 0;                               // columns of link r, counted from the first column after link p
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (j == r) { cs = koff[j] - kend; cn = kk[j]; }
                    chain_wait(&V.sflag_s[4 * G.s + r], epoch, V.qstat + 1);
                    const double* Wg = V.wbuf + G.wb + k + cs;        // W21 rows of link r's pivots
                    const int nct = (cn + 15) >> 4;
                    for (int tc = 0; tc < nct; tc += 2) {
                        double a0[16], a1[16];
                        const int ra = 16 * tc + l15, rb = ra + 16;
#pragma unroll
                        for (int u = 0; u < 16; ++u) {
                            const int qq = 4 * u + l4;
                            a0[u] = (ra < cn && qq < k) ? Wg[ra + (size_t)qq * m] : 0.0;
                            a1[u] = (rb < cn && qq < k) ? Wg[rb + (size_t)qq * m] : 0.0;
                        }
                        double t0[4], t1[4];
#pragma unroll
                        for (int gg = 0; gg < 4; ++gg) {
                            const int c = 16 * tc + l4 + 4 * gg;
                            t0[gg] = (rowok && c < cn) ? Tt[irow + (size_t)(cs + c) * ldt] : 0.0;
                            t1[gg] = (rowok && c + 16 < cn) ? Tt[irow + (size_t)(cs + c + 16) * ldt] : 0.0;
                        }
                        v4f64 c0v = (v4f64){0.0, 0.0, 0.0, 0.0}, c1v = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll
                        for (int u = 0; u < 16; ++u)
                            if (4 * u < kp16) {
                                c0v = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[u], bv[u], c0v, 0, 0, 0);
                                c1v = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[u], bv[u], c1v, 0, 0, 0);
                            }
#pragma unroll
                        for (int gg = 0; gg < 4; ++gg) {
                            const int c = 16 * tc + l4 + 4 * gg;
                            if (rowok && c < cn) Tt[irow + (size_t)(cs + c) * ldt] = t0[gg] - c0v[gg];
                            if (rowok && c + 16 < cn) Tt[irow + (size_t)(cs + c + 16) * ldt] = t1[gg] - c1v[gg];
                        }
                    }
                }
            }
            if (tsp) tsp[6] = clock64();
            // (b) my OWN pivot block: both operands and the target are in LDS (lower 16 x 16 tiles, v_mfma_f64_16x16x4_f64; a lone
            //     wavefront issues one per ~150 cycles -- the same 1024 FMAs as 16 v_fmac_f64 take ~105, but those would want 8 LDS
            //     operands per step instead of 2: measured slower, tools/micro/fma_lds_latency.hip).  All 16 operand pairs of a tile
            //     are requested before its first MFMA.
            if (myq >= 0 && !pipe) {
                const int nt = (myrows + 15) >> 4;
                if (tsp) tsp[13] = clock64();
                int q = 0;
                for (int tc = 0; tc < nt; ++tc)
                    for (int ti = tc; ti < nt; ++ti, ++q) {
                        if ((q & 3) != wave) continue;
                        double av[16], bw[16];
                        v4f64 acc = (v4f64){0.0, 0.0, 0.0, 0.0};
                        if (Lr && kp16 == 64) {      // (straight-line: both LDS blocks are zero beyond column k)
#pragma unroll
                            for (int u = 0; u < 16; ++u) { av[u] = Lr[(16 * ti + l15) + (4 * u + l4) * 65]; bw[u] = As[(16 * tc + l15) + (4 * u + l4) * 65]; }
#pragma unroll
                            for (int u = 0; u < 16; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bw[u], acc, 0, 0, 0);
                        } else {
                            for (int u = 0; 4 * u < kp16; ++u) {
                                const int qq = 4 * u + l4;
                                acc = __builtin_amdgcn_mfma_f64_16x16x4f64((qq < k) ? lval(16 * ti + l15, qq) : 0.0, (qq < k) ? As[(16 * tc + l15) + qq * 65] : 0.0, acc, 0, 0, 0);
                            }
                        }
                        const int cc = 16 * tc + l15;
#pragma unroll
                        for (int gg = 0; gg < 4; ++gg) { const int rr = 16 * ti + l4 + 4 * gg; if (rr < myrows && cc < myrows && rr >= cc) Db[rr + cc * ldb] -= acc[gg]; }
                    }
                if (tsp) tsp[14] = clock64();
            }
        }
        __syncthreads();
        if (crit) chain_signal_coh(&V.sflag_s[4 * G.s + myq], epoch);
        if (tsp) tsp[7] = clock64();
        if (p == last_p) GSTAMP(4);
    }
    }
    if (myq < 0) return;
    {   // my own pivot block: a copy goes to the panel storage (the strict fall-back reads it there), then the factorisation in place.  Not in the optimistic
        // schedule (V.norestore): 32 KB of stores and their acknowledgement sat on the critical chain of every link (6 400 cycles of ~106 000,
        // profiles/r04b_synth_1e6_pivot_block_phases.txt) for a fall-back that 0 of the 9 800 pivot blocks of synth_1e6 takes; a block that IS rejected
        // there raises qstat[5] (big_diag_body) and the factorisation is repeated with the copy.
        double* Pq = V.L + Gq.panel_off;
        const size_t ldq = (size_t)Gq.ldp;
        const int i = tid & 63, cq = tid >> 6, kq = Gq.k;
        if (!V.norestore) {
#pragma unroll
        for (int e = 0; e < 16; ++e) { const int c = cq + 4 * e; if (i < kq && c < kq && i >= c) Pq[i + (size_t)c * ldq] = Db[i + c * ldb]; }
        }
        FrontMeta Mq = M;
        Mq.s = Gq.s; Mq.c0 = Gq.c0; Mq.k = Gq.k; Mq.m = Gq.m; Mq.panel_off = Gq.panel_off; Mq.ldp = Gq.ldp; Mq.wb = Gq.wb; Mq.minv_off = Gq.minv_off;
        Mq.selfasm = 0; Mq.aq0 = Gq.aq0; Mq.aq1 = Gq.aq1; Mq.bigidx = Gq.bigidx;      // (the A entries are in already)
        __syncthreads();
        big_diag_body<4, 256, true>(V, Mq, smem_raw, &V.sflag_d[Gq.s], epoch, tsp, crit_Lr, crit_Mp, crit_ibase, myrows, (V.norestore && staged) ? &V.sflag_p[Gq.s] : nullptr);
        if (tsp && tid == 0) { for (int q = 0; q < 28; ++q) V.dbg[64 + q] = tsp[q]; }
        GSTAMP(7);
    }
#undef GSTAMP
}
__global__ __launch_bounds__(256) void k_grp_fused(DevView V, int list_off, int staged, int rbw, int role0) { grp_fused_body(V, list_off, staged, rbw, role0); }



