// kernels_fronts.hip.inc -- part of numeric.hip (one translation unit; included there, inside namespace mi355x): fronts of order <= 128: register-tiled Bunch-Kaufman LDL^T core, blocked a-posteriori pivot blocks, static-order fast paths, inertia reduction.
// ================================================================================================
// Register-tiled LDL^T core (the production path).  The assembled front is pulled from LDS into VGPRs as a
// G x G grid of TS x TS tiles (full symmetric storage, thread (ti,tj) owns rows ti*TS.., columns tj*TS..);
// LDS only carries the pivot column(s) of the current step (published by the G owner threads, read by everybody:
// by symmetry the same vector serves as row and column multipliers) and the finished L columns.
//   * no interchanges: Bunch-Kaufman picks the pivot among the still-alive fully-summed rows and the chosen
//     PHYSICAL row is eliminated in place; the pivot order `ord` is applied once at write-back;
//   * one barrier per 1x1 pivot (two when the BK test needs the partner column), none of them inside a wavefront's
//     own dependency chain when the workgroup is a single wave (fronts of order <= 64);
//   * pivot search: DPP wave reduction, done redundantly by every wave on the published column.
// (NT,TS) = (64,4): order <= 32, (64,8): <= 64, (256,8): <= 128, (256,4): the 64-column pivot block of a big front.
// ================================================================================================
template <int TS>
__device__ __forceinline__ void publish_col(double* buf, const double (&t)[TS][TS], const int row0, const int jl)
{
    // jl is wave-uniform: a scalar branch selects the STATICALLY indexed register column.  The empty asm keeps the
    // cases apart -- merged, they become a dynamically indexed t[a][jl] and the whole tile array moves to scratch.
#pragma unroll
    for (int b = 0; b < TS; ++b)
        if (jl == b) {
#pragma unroll
            for (int a = 0; a < TS; ++a) { double v = t[a][b]; asm volatile("" : "+v"(v)); buf[row0 + a] = v; }
        }
}

#ifdef MI355X_PIVSTAT
__device__ unsigned long long g_fstat[32];
__device__ unsigned long long g_dt[16], g_dtacc[16];     // fused pivot block + panel solve, single front: wall-clock stamps of one launch / sums over launches
__device__ unsigned long long g_pivstat[16];      // development build only: [0] pivots steps, [1] slow-path entries, [2] quick accepts, [3] exact path, [4] pass-overs, [5] 2x2, [6] no-partner
#ifdef MI355X_PIVSTAT_COUNT
#define PIVSTAT(i) do { if (threadIdx.x == 0) atomicAdd(&g_pivstat[i], 1ull); } while (0)
#else
#define PIVSTAT(i) do { } while (0)
#endif
#else
#define PIVSTAT(i) do { } while (0)
#endif

__device__ __forceinline__ double fast_rcp(double d)
{
    double r = __builtin_amdgcn_rcp(d);          // v_rcp_f64 + two Newton steps: full fp64 accuracy without the division macro
    double e = fma(-d, r, 1.0); r = fma(r, e, r);
    e = fma(-d, r, 1.0); r = fma(r, e, r);
    return r;
}

// Threshold pivoting (what u = pivtol means here; DESIGN.md "pivoting"):
//   * candidate order: the still-alive fully-summed rows in physical order; a candidate j whose diagonal is within
//     alpha0 = 0.1 of its whole remaining column (|a_jj| >= alpha0 max_{i != j} |a_ij|: the threshold test of UMFPACK / MA48
//     at their default u, seven orders of magnitude tighter than Ipopt's 1e-8) is eliminated as a 1x1 without looking
//     further; otherwise the Bunch-Kaufman rule (alpha = 0.64, on the alive fully-summed part) PREFERS one of
//     {1x1 at j, 1x1 at r, 2x2 (j,r)}, r = the fully-summed row with the largest |a_rj|;
//   * a pivot is ACCEPTED only if it passes the MA27/MA57 threshold tests against the WHOLE remaining front column --
//     alive fully-summed rows AND update rows:   1x1: |a_pp| >= u max_{i != p} |a_ip|;
//     2x2: |E^{-1}| (g_p, g_q)^T <= 1/u componentwise, g = column maxima outside the block (Duff & Reid 1983; MA57);
//     if the preferred pivot fails, the other two are tried;
//   * a candidate with no acceptable pivot is PASSED OVER (retried after the next elimination has updated it: the
//     in-front part of MA27's delayed pivoting).  When every alive candidate has failed, the structure being static
//     (no delay to the parent front), the first one is eliminated anyway by the plain Bunch-Kaufman choice and counted in
//     `ndelay` (reported as num_delay; the reference adapters read the same counter from MA97/SPRAL);
//   * zero test relative to what was assembled into the candidate's own column: a candidate whose whole remaining column is
//     <= max(small, 1e-14 max_i |F(i,j)| at assembly) is a zero pivot => SYMSOLVER_SINGULAR;
//   * `chg` is set when some decision would come out differently at u2 (= pivtolmax): IncreaseQuality uses it to
//     answer "can a larger u change the factorisation at all".
// Big fronts: the pivot block only sees its k x k block here (ext rows are checked a posteriori in k_big_trsm).
template <int NT, int TS, bool WIDE>
__device__ __forceinline__ void ldlt_reg(double (&t)[TS][TS], const int m, const int k, double* Lbuf, const int ldL, double* colbuf,
                                         double* dinv_s, double* doff_s, int* pt_s, int* ord, const double u, const double u2, const double small, const double* cm0, const double cmx, int* zp,
                                         int& nneg, int& nzero, int& ntwo, int& ndelay, int& chg)
{
    // The per-pivot instruction stream IS the critical path (measured: ~5 cycles per wave instruction), so the common
    // case -- 1x1 pivot on the first alive row -- is kept to ~100 instructions: unconditional wide LDS reads + bit-mask
    // selects, ballots instead of max-reductions for the Bunch-Kaufman and threshold acceptance tests, reciprocal by
    // v_rcp_f64 + Newton, L column written by the 16 (8) threads that already hold it.
    constexpr int G = (NT == 64) ? 8 : (NT == 1024 ? 32 : 16);
    constexpr int MAXM = G * TS;
    constexpr bool TWO = MAXM > 64;              // each lane looks at rows `lane` and `lane + 64` of a published column
    const int tid = threadIdx.x, lane = tid & 63;
    const int ti = tid % G, tj = tid / G;
    const int row0 = ti * TS, col0 = tj * TS;
    unsigned rowvalid = 0;
#pragma unroll
    for (int x = 0; x < TS; ++x) if (row0 + x < m) rowvalid |= 1u << x;
    const unsigned long long lanebit = 1ull << lane;
    const int lane1 = TWO ? min(lane + 64, MAXM - 1) : 0;
    const bool up0 = lane >= k && lane < m;                   // update rows seen by this lane
    const bool up1 = TWO && lane + 64 >= k && lane + 64 < m;
    // fully-summed rows not yet eliminated: rows 0..63 in alive, rows 64..127 in alive1 (WIDE: pivot blocks of <= 128 columns)
    unsigned long long alive = (k >= 64) ? ~0ull : ((1ull << k) - 1ull);
    unsigned long long alive1 = (WIDE && k > 64) ? ((k >= 128) ? ~0ull : ((1ull << (k - 64)) - 1ull)) : 0ull;
    unsigned long long tryb = alive, tryb1 = alive1;          // candidates not yet passed over since the last elimination
    bool force = false;
    double u2e = u2;                                          // 0 while forced: a forced pivot stays forced at any larger u
    unsigned long long chgm = 0ull;
    const double zmax = fmax(small, ZERO_REL * cmx);
    auto clear_row = [&](int r) { if (!WIDE || r < 64) alive &= ~(1ull << r); else alive1 &= ~(1ull << (r - 64)); };
    int step = 0, bufsel = 0;
#ifdef MI355X_PIVSTAT
    long long tprev = clock64(); bool was_slow = false; int first = 1; unsigned long long acc_f = 0, acc_s = 0, n_f = 0, n_s = 0;
#endif
    while ((alive | alive1) != 0ull) {
#ifdef MI355X_PIVSTAT
        if (NT == 256 && TS == 4 && tid == 0 && gridDim.x == 1 && blockIdx.y == 0) { const long long tn = clock64(); if (!first) { if (was_slow) { acc_s += tn - tprev; n_s++; } else { acc_f += tn - tprev; n_f++; } } tprev = tn; first = 0; was_slow = false; }
#endif
        double* colA = colbuf + bufsel * 2 * MAXM; bufsel ^= 1;
        double* colB = colA + MAXM;
        const int j = __builtin_amdgcn_readfirstlane(tryb != 0ull ? __ffsll((long long)tryb) - 1 : 64 + __ffsll((long long)tryb1) - 1);
        if (tj == j / TS) publish_col<TS>(colA, t, row0, j % TS);
        __syncthreads();
        // every LDS read of the common case (1x1 pivot on row j) is issued here, in ONE round trip
        const double djj = colA[j];
        const double avr = colA[lane];
        const double avr1 = TWO ? colA[lane1] : 0.0;
        double rv[TS], cv[TS];
#pragma unroll
        for (int x = 0; x < TS; ++x) { rv[x] = colA[row0 + x]; cv[x] = colA[col0 + x]; }
        const double ajj = fabs(djj);
        const double f0 = fabs(avr), f1 = fabs(avr1);
        const bool cand = (alive & lanebit) != 0ull && lane != j;
        const bool cand1 = WIDE && (alive1 & lanebit) != 0ull && lane + 64 != j;
        const double av0 = cand ? f0 : -1.0, av1 = cand1 ? f1 : -1.0;
        const double av = fmax(av0, av1);                      // alive fully-summed rows (the Bunch-Kaufman candidates)
        const double ga = fmax(fmax(av, up0 ? f0 : 0.0), up1 ? f1 : 0.0);      // whole remaining column, diagonal excluded
        // the common case must stay ONE straight instruction stream (every taken branch costs an instruction refetch on the
        // serial pivot chain): three ballots OR-ed into one scalar test, statistics accumulated branch-free
        const unsigned long long slowm = __ballot(ga * BK_ALPHA0 > ajj)       // some |a_ij| > |a_jj| / alpha0: full Bunch-Kaufman test
                                       | __ballot(ga * u > ajj)               // 1x1 at j fails the threshold test
                                       | __ballot(!(ajj > zmax));             // possibly a (numerically) zero diagonal: exact test below
        chgm |= __ballot(ga * u2e > ajj);
        double d = djj;                    // 1x1 pivot value on physical row p (pivot column in rv / cv)
        int p = j;
        PIVSTAT(0);
        if (__builtin_expect(slowm != 0ull, 0)) {
            PIVSTAT(1);
#ifdef MI355X_PIVSTAT
            was_slow = true;
#endif
            const int bi = (av1 > av0) ? lane + 64 : lane;       // this lane's best candidate row
            const double ztol = fmax(small, ZERO_REL * cm0[j]);     // zero threshold of candidate j
            const double uu = force ? 0.0 : u;
            const double lam = wave_max_all(av);               // -1: no alive fully-summed partner
            int sel = -1;                                      // 0: 1x1 at j, 1: 1x1 at r, 2: 2x2 (j, r)
            int r = -1;
            bool zero = false;
            if (lam > 0.0) {
#ifdef MI355X_PIVSTAT_COUNT
                { const double rho = ajj / lam; if (threadIdx.x == 0) atomicAdd(&g_pivstat[rho >= 0.5 ? 12 : (rho >= 0.25 ? 13 : (rho >= 0.1 ? 14 : 15))], 1ull); if (threadIdx.x == 0 && rho < 0.01) atomicAdd(&g_pivstat[7], 1ull); }
#endif
                const unsigned long long hit = __ballot(av == lam);
                const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)hit) - 1);
                r = __builtin_amdgcn_readlane(bi, src);
                if (tj == r / TS) publish_col<TS>(colB, t, row0, r % TS);
                __syncthreads();
                const double h0 = fabs(colB[lane]), h1 = TWO ? fabs(colB[lane1]) : 0.0;
                const bool cs = (alive & lanebit) != 0ull && lane != r;
                const bool cs1 = WIDE && (alive1 & lanebit) != 0ull && lane + 64 != r;
                const double sfs = fmax(cs ? h0 : 0.0, cs1 ? h1 : 0.0);
                const double sig = wave_max_all(sfs);                                            // Bunch-Kaufman sigma
                const double hall = fmax(fmax(sfs, up0 ? h0 : 0.0), up1 ? h1 : 0.0);             // whole column r, diagonal excluded
                const double a = djj, b = colA[r], c = colB[r];
                const double arr = fabs(c), ab = fabs(b);
                const double det = a * c - b * b, adet = fabs(det);
                const double ztr = fmax(small, ZERO_REL * cm0[r]);
                const bool nz2 = adet > fmax(small, ZERO_REL * fmax(ajj * arr, ab * ab));     // the block itself is not (numerically) singular
                const int pref = (ajj >= BK_ALPHA * lam || ajj * sig >= BK_ALPHA * lam * lam) ? 0 : ((arr >= BK_ALPHA * sig) ? 1 : 2);
                // ONE reduction bounds every column maximum the threshold tests need (G >= gj, gr, gj2, gr2): when the
                // preferred pivot passes them with G -- at u and at u2, the usual case -- it passes the exact tests too
                const double G = wave_max_all(fmax(ga, hall));
                const double um = fmax(uu, u2e);
                const bool quick = !force && ((pref == 0) ? (ajj > ztol && ajj >= um * G)
                                            : (pref == 1) ? (arr > ztr && arr >= um * G)
                                                          : (nz2 && (arr + ab) * G * um <= adet && (ab + ajj) * G * um <= adet));   // (forced pivots are counted exactly)
                if (quick) { sel = pref; PIVSTAT(2); }
                else {
                    PIVSTAT(3);
                    const double gj = wave_max_all(ga);
                    const double gr = wave_max_all(hall);
                    const bool nj0 = lane != j, nj1 = lane + 64 != j;
                    const double gj2 = wave_max_all(fmax(fmax((cand && lane != r) ? f0 : 0.0, (cand1 && lane + 64 != r) ? f1 : 0.0), fmax(up0 ? f0 : 0.0, up1 ? f1 : 0.0)));
                    const double gr2 = wave_max_all(fmax(fmax((cs && nj0) ? h0 : 0.0, (cs1 && nj1) ? h1 : 0.0), fmax(up0 ? h0 : 0.0, up1 ? h1 : 0.0)));
                    const double t1 = arr * gj2 + ab * gr2, t2 = ab * gj2 + ajj * gr2;                // |E^{-1}| (gj2, gr2)^T |det|
                    const bool ok0 = ajj > ztol && ajj >= uu * gj;
                    const bool ok1 = arr > ztr && arr >= uu * gr;
                    const bool ok2 = nz2 && t1 * uu <= adet && t2 * uu <= adet;
                    if ((pref == 0 && ok0) || (pref == 1 && ok1) || (pref == 2 && ok2)) sel = pref;
                    else if (ok0) sel = 0; else if (ok2) sel = 2; else if (ok1) sel = 1;
                    if (sel >= 0) {
                        const bool f_u  = (sel == 0) ? (ajj < u * gj)  : ((sel == 1) ? (arr < u * gr)  : (t1 * u > adet  || t2 * u > adet));
                        const bool f_u2 = (sel == 0) ? (ajj < u2 * gj) : ((sel == 1) ? (arr < u2 * gr) : (t1 * u2 > adet || t2 * u2 > adet));
                        if (f_u) ndelay += (sel == 2) ? 2 : 1;     // only possible when forced
                        if (f_u2 && !force) chgm |= 1ull;          // (a forced pivot stays forced at any larger u)
                    }
                }
            } else {
                PIVSTAT(6);
                const double gj = wave_max_all(ga);
                if (ajj > ztol && ajj >= uu * gj) { sel = 0; if (ajj < u * gj) ndelay += 1; }
                else if (!(ajj > ztol) && !(gj > ztol)) { sel = 0; zero = true; }          // the whole remaining column is zero
            }
            if (sel < 0) {
                if (!force) {          // pass over: retried once another elimination has updated the column
                    PIVSTAT(4);
                    if (!WIDE || j < 64) tryb &= ~(1ull << j); else tryb1 &= ~(1ull << (j - 64));
                    if ((tryb | tryb1) == 0ull) {      // every candidate failed: all of them are DELAYED pivots (bit 1 of zpiv; the host moves them to the parent front and
                        force = true; u2e = 0.0; tryb = alive; tryb1 = alive1;      // refactors, symbolic.cpp restructure_delays); this factorisation goes on with static pivoting
                        if (tid == 0) { for (unsigned long long bm = alive; bm != 0ull; bm &= bm - 1ull) zp[__ffsll((long long)bm) - 1] |= 2;
                                        if (WIDE) for (unsigned long long bm = alive1; bm != 0ull; bm &= bm - 1ull) zp[64 + __ffsll((long long)bm) - 1] |= 2; }
                    }
                    continue;
                }
                sel = 0; zero = true;  // forced and nothing usable: a (perturbed) zero pivot => singular
            }
            force = false; u2e = u2;
            if (sel == 2) {
                PIVSTAT(5);
                const int q = r;
                const double a = colA[p], b = colA[q], c = colB[q];
                const double det = a * c - b * b;
                const double idet = fast_rcp(det);
                double l0[TS], l1[TS], w0[TS], w1[TS];
#pragma unroll
                for (int x = 0; x < TS; ++x) {
                    const double r0 = colA[row0 + x], r1 = colB[row0 + x];
                    l0[x] = (c * r0 - b * r1) * idet; l1[x] = (a * r1 - b * r0) * idet;
                    w0[x] = colA[col0 + x]; w1[x] = colB[col0 + x];
                }
#pragma unroll
                for (int x = 0; x < TS; ++x)
#pragma unroll
                    for (int y = 0; y < TS; ++y) t[x][y] -= l0[x] * w0[y] + l1[x] * w1[y];
                if (tj == 0) {
#pragma unroll
                    for (int x = 0; x < TS; ++x) if ((rowvalid >> x) & 1u) { Lbuf[row0 + x + step * ldL] = l0[x]; Lbuf[row0 + x + (step + 1) * ldL] = l1[x]; }
                }
                if (tid == 0) {
                    ord[step] = p; ord[step + 1] = q; pt_s[step] = 2; pt_s[step + 1] = 3;
                    dinv_s[step] = c * idet; dinv_s[step + 1] = a * idet; doff_s[step] = -b * idet; doff_s[step + 1] = 0.0;
                }
                if (det < 0.0) nneg += 1; else if (a + c < 0.0) nneg += 2;
                ntwo++; clear_row(p); clear_row(q); step += 2;
                tryb = alive; tryb1 = alive1;
                continue;
            }
            if (sel == 1) {
                p = r; d = colB[r];
#pragma unroll
                for (int x = 0; x < TS; ++x) { rv[x] = colB[row0 + x]; cv[x] = colB[col0 + x]; }
            }
            if (zero) { nzero++; d = (d < 0.0) ? -PIV_PERT : PIV_PERT; if (tid == 0) zp[p] |= 1; }
        }
        {   // 1x1 pivot on physical row p
            const double di = fast_rcp(d);
            // No masking of dead rows / columns: the rank-1 update itself annihilates row and column p (l_p = 1 up to
            // rounding), padding rows are exact zeros, and whatever residue is left in dead positions is never read
            // (alive mask in the search, (i > c) filter at write-back).  That removes ~50 instructions per pivot.
            double l0[TS];
#pragma unroll
            for (int x = 0; x < TS; ++x) l0[x] = rv[x] * di;
            const double (&w0)[TS] = cv;
#pragma unroll
            for (int x = 0; x < TS; ++x)
#pragma unroll
                for (int y = 0; y < TS; ++y) t[x][y] -= l0[x] * w0[y];
            if (tj == 0) {
#pragma unroll
                for (int x = 0; x < TS; ++x) if ((rowvalid >> x) & 1u) Lbuf[row0 + x + step * ldL] = l0[x];
            }
            if (tid == 0) { ord[step] = p; pt_s[step] = 1; dinv_s[step] = di; doff_s[step] = 0.0; }
            nneg += (d < 0.0) ? 1 : 0;
            clear_row(p); step += 1;
            tryb = alive; tryb1 = alive1;
        }
    }
#ifdef MI355X_PIVSTAT
    if (n_f + n_s) { atomicAdd(&g_pivstat[8], acc_f); atomicAdd(&g_pivstat[9], acc_s); atomicAdd(&g_pivstat[10], n_f); atomicAdd(&g_pivstat[11], n_s); }
#endif
    if (chgm != 0ull) chg = 1;
    __syncthreads();
}

// zero-pivot scale of every fully-summed COLUMN -> cm0[0..k): the larger of the column's inf-norm in the (scaled) input matrix
// and of what was assembled into it in this front.  A pivot is numerically zero relative to ITS column -- a huge Sigma entry
// elsewhere in the front (late barrier iterations, no equilibration) must not make healthy small pivots look like zeros, and a
// column whose entries already cancelled in the children (dependent constraint rows) must still be measured against what it was.
template <int NT, int TS>
__device__ __forceinline__ double front_colmax(const double (&t)[TS][TS], double* cm0, const int k, const double* cnorm)
{
    constexpr int G = (NT == 64) ? 8 : (NT == 1024 ? 32 : 16);
    const int tid = threadIdx.x, ti = tid % G, tj = tid / G;
#pragma unroll
    for (int y = 0; y < TS; ++y) {
        double mx = 0.0;
#pragma unroll
        for (int x = 0; x < TS; ++x) mx = fmax(mx, fabs(t[x][y]));
        // the G threads that share tile column tj are G consecutive lanes (tid = ti + G tj): butterfly inside the group
        mx = fmax(mx, dpp_f64<0xB1>(mx));
        mx = fmax(mx, dpp_f64<0x4E>(mx));
        mx = fmax(mx, dpp_f64<0x141>(mx));           // 8 lanes
        if (G >= 16) mx = fmax(mx, dpp_f64<0x140>(mx));   // 16 lanes
        if (G == 32) mx = fmax(mx, __shfl_xor(mx, 16));
        if (ti == 0 && tj * TS + y < k) cm0[tj * TS + y] = fmax(mx, cnorm[tj * TS + y]);
    }
    __syncthreads();
    // the largest of them: lets the per-pivot fast path test |a_jj| against ONE register value (a pivot that clears the largest
    // threshold clears its own); only candidates below it look their own threshold up (slow path)
    const int lane = tid & 63;
    return wave_max_all(fmax(lane < k ? cm0[lane] : 0.0, lane + 64 < k ? cm0[lane + 64] : 0.0));
}

// fronts of order 65 .. 128 with <= 16 pivots: static-order blocked elimination accepted a posteriori (defined behind the DPP helpers below)
__device__ __forceinline__ bool front_fast16(double* F, const int m, const int k, double* scratch, double* dinv_s, const double* cnorm, const double small, const double gmax, int& nneg);

// front kernel on the register-tiled core: LDS assembly (A scatter + children extend-add), tiles -> VGPRs, LDL^T,
// write-back of the pivot-ordered panel, the contribution block (straight from registers), pivot data and L11^{-1}.
// FAST (256 threads only): the fronts of the bucket with <= 16 pivots are assembled and eliminated on the static-order path (front_fast16) and
// marked done (hasis[s] = 2) when it accepts them; the ordinary instantiation is launched behind it with flags & 2 and leaves those alone.  Two
// kernels, not one with a branch: inlined into the strict kernel the fast path's 100 registers pushed <256, 6> from 134 to 459 spilled VGPRs.
template <int NT, int TS, bool FAST = false, int OCC = 0>      // OCC > 0: wavefronts per SIMD the register budget is cut for (development: MI355X_KKT_FAST_OCC)
__global__ __launch_bounds__(NT, OCC > 0 ? OCC : ((NT == 64 && TS == 4) ? 4 : ((NT == 64 && TS == 2) ? 6 : ((NT == 256 && TS == 6) ? 3 : 1)))) void k_front_reg(DevView V, int list_off, int flags)
{
    const int top_mode = flags & 1;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int G = (NT == 64) ? 8 : 16;
    constexpr int MAXM = G * TS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NW = NT / 64;
    const FrontMeta M = V.fmeta[list_off + blockIdx.x];
    const int s = M.s, c0 = M.c0, k = M.k, r0 = M.r0, m = M.m; (void)s; (void)c0; (void)r0; (void)k;
    if (FAST) { if (k > 16) { if (tid == 0) V.hasis[s] = 0; return; } }
    else if ((flags & 2) && V.hasis[s] == 2) return;
    const int ld = m | 1, ldi = k | 1;
    DBGSTAMP(4);
#ifdef MI355X_PIVSTAT
    long long ph0 = clock64(), ph1 = 0, ph2 = 0, ph3 = 0, ph4 = 0;
#endif
    // F: the front's LOWER triangle, packed by columns (column c starts at c m - c (c - 1) / 2) -- half the LDS of a square, so
    // twice as many fronts per CU on levels made of thousands of them (the pivot loop is a latency chain: co-resident fronts are
    // what fills the SIMDs); later overlaid by Lbuf (k columns of stride ld) + the k x k inverse
    const int npk = m * (m + 1) / 2;
    const int fdoubles = max(npk, k * ld + k * ldi);
    double* F      = reinterpret_cast<double*>(smem_raw);
    double* colbuf = F + fdoubles;               // 4 * MAXM
    double* dinv_s = colbuf + 4 * MAXM;          // k
    double* doff_s = dinv_s + k;                 // k
    double* cm0    = doff_s + k;                 // k   max |entry| of each fully-summed column of the assembled front
    int*    ord    = reinterpret_cast<int*>(cm0 + k);      // k
    int*    pt_s   = ord + k;                    // k
    auto pk = [m](int i, int c) { return c * m - ((c * (c - 1)) >> 1) + (i - c); };      // i >= c

    // ---- (a)-(c) assembly in LDS (lower storage) ----
    const bool from_arena = top_mode && V.arena && V.arena_off[s] >= 0;   // replicated front at a subtree join
    const bool skip_owned = top_mode && V.arena;
    if (from_arena) {
        const double* Ar = V.arena + V.arena_off[s];
        for (int idx = tid; idx < npk; idx += NT) F[idx] = Ar[idx];          // (the arena square is packed exactly like F)
    } else {
        for (int idx = tid; idx < npk; idx += NT) F[idx] = 0.0;
    }
    __syncthreads();
    {
        const int q0 = M.aq0, q1 = M.aq1;
        for (int q = q0 + tid; q < q1; q += NT) { const int pos = V.apos[q]; const int i = pos % m, c = pos / m; F[pk(i, c)] += V.aval[q]; }
    }
    __syncthreads();
    // children: extend-add of each contribution block (lower triangle of an mc x mc square).  A dependent global access costs
    // 1.5-2 us on this part, so a child is NOT walked column by column: its lower triangle is enumerated flat -- column b paired
    // with column mc-1-b, mc+1 entries per pair -- and fetched in batches of 16 independent loads per thread, issued together
    // with the load of its relative indices; the scatter into F then runs out of registers.
    {
        int* relS = reinterpret_cast<int*>(colbuf);              // the child's relative indices (colbuf is free until the LDL^T)
        for (int cp = M.ch0; cp < M.ch1; ++cp) {
            const ChildMeta* Cp = V.cmeta + cp;
            if (skip_owned && Cp->owner >= 0) continue;
            const int mc = Cp->mc, ldt = Cp->ldt;
            const double* C = V.cb + Cp->cb_off;
            const int* relg = V.rel + Cp->relbase;
            const unsigned d = (unsigned)(mc + 1), inv = 0xFFFFFFFFu / d + 1u;      // floor(e / d) = umulhi(e, inv) for e < 2^16
            const int npr = (mc + 1) >> 1, total = npr * (mc + 1);
            int r0v = (tid < mc) ? relg[tid] : 0, r1v = 0;
            if (NT == 64 && tid + 64 < mc) r1v = relg[tid + 64];
            auto decode = [&](int e, int& a, int& b) -> bool {      // flat index -> (row a >= column b) of the child's lower triangle
                const int pr = (int)__umulhi((unsigned)e, inv), q = e - pr * (mc + 1);
                const bool second = q >= mc - pr;
                b = second ? mc - 1 - pr : pr;
                a = second ? b + (q - (mc - pr)) : pr + q;
                return e < total && !(second && 2 * pr == mc - 1);        // (mc odd: the middle column pairs with itself)
            };
            constexpr int U = (TS <= 6) ? 8 : 16;                     // loads in flight per thread (the small-tile instantiations are register-capped)
            for (int base = 0; base < total; base += NT * U) {
                double cvv[U];
#pragma unroll
                for (int u = 0; u < U; ++u) { int a, b; cvv[u] = decode(base + tid + NT * u, a, b) ? C[a + (size_t)b * ldt] : 0.0; }
                if (base == 0) {
                    if (tid < mc) relS[tid] = r0v;
                    if (NT == 64 && tid + 64 < mc) relS[tid + 64] = r1v;
                    __syncthreads();
                }
#pragma unroll
                for (int u = 0; u < U; ++u) { int a, b; if (decode(base + tid + NT * u, a, b)) F[pk(relS[a], relS[b])] += cvv[u]; }
            }
            __syncthreads();
        }
    }
#ifdef MI355X_PIVSTAT
    ph1 = clock64();
#endif
    // ---- fast path: <= 16 pivots eliminated in natural order by ONE wavefront (DPP), the rest of the front by MFMA; accepted a posteriori ----
    if constexpr (FAST) {
        int fneg = 0;
        const double gmax = 1.0 / fmax(fmax(V.pivtol, V.pivtol2), V.fastu);
        if (!front_fast16(F, m, k, colbuf, dinv_s, V.cnorm + c0, V.small, gmax, fneg)) { if (tid == 0) V.hasis[s] = 0; return; }
        {
            // F(i, c), c < k: W = L d (i > c);  F(i, c), i >= c >= k: the Schur complement;  colbuf: L11^{-1} (X(i, p) at [i + 17 p])
            double* Lg = V.L + M.panel_off;
            for (int c = wave; c < k; c += NW) {
                const double di = dinv_s[c];
                for (int i = lane; i < m; i += 64) Lg[i + (size_t)c * m] = (i > c) ? F[pk(i, c)] * di : 0.0;
            }
            for (int jj = tid; jj < k; jj += NT) { V.dinv[c0 + jj] = dinv_s[jj]; V.doff[c0 + jj] = 0.0; V.ptype[c0 + jj] = 1; V.lperm[c0 + jj] = jj; }
            const int mu = m - k;
            double* Cg = V.cb + M.cb_off;
            for (int c = k + wave; c < m; c += NW)
                for (int i = c + lane; i < m; i += 64) Cg[(i - k) + (size_t)(c - k) * mu] = F[pk(i, c)];
            if (tid == 0) V.fstat[s] = make_int4(fneg, 0, 0, 0);
            double* Mg = V.minv + M.minv_off;
            for (int idx = tid; idx < k * k; idx += NT) { const int i = idx % k, c = idx / k; Mg[idx] = (i > c) ? colbuf[i + 17 * c] : (i == c ? 1.0 : 0.0); }
            if (tid == 0) V.hasis[s] = 2;
            return;
        }
    }
    // ---- tiles -> registers (full symmetric) ----
    const int ti = tid % G, tj = tid / G, row0 = ti * TS, col0 = tj * TS;
    double t[TS][TS];
    {
        int rbase[TS];                                 // packed start of column (row0 + x), minus its index: F(c, i) for c > i sits at rbase[x] + c
#pragma unroll
        for (int x = 0; x < TS; ++x) { const int i = row0 + x; rbase[x] = i * m - ((i * (i - 1)) >> 1) - i; }
#pragma unroll
        for (int y = 0; y < TS; ++y) {
            const int c = col0 + y;
            const int cbase = c * m - ((c * (c - 1)) >> 1) - c;
#pragma unroll
            for (int x = 0; x < TS; ++x) {
                const int i = row0 + x;
                const int idx = (i >= c) ? cbase + i : rbase[x] + c;
                t[x][y] = (i < m && c < m) ? F[idx] : 0.0;
            }
        }
    }
    __syncthreads();                                   // F is dead from here on: its storage becomes Lbuf
    // ---- (d) LDL^T ----
    int nneg = 0, nzero = 0, ntwo = 0, nsmall = 0, chg = 0;
    DBGSTAMP(5);
#ifdef MI355X_PIVSTAT
    ph2 = clock64();
#endif
    const double cmx = front_colmax<NT, TS>(t, cm0, k, V.cnorm + c0);
    ldlt_reg<NT, TS, false>(t, m, k, F, ld, colbuf, dinv_s, doff_s, pt_s, ord, V.pivtol, V.pivtol2, V.small, cm0, cmx, V.zpiv + c0, nneg, nzero, ntwo, nsmall, chg);
    if (chg && tid == 0) V.qstat[0] = 1;
    __syncthreads();
    DBGSTAMP(6);
#ifdef MI355X_PIVSTAT
    ph3 = clock64();
#endif
    if (V.dbg && blockIdx.x == 0 && tid == 0) V.dbg[14] = (unsigned long long)k * 1000 + m;
    // ---- (e) write back: pivot-ordered panel, pivot data, contribution block from the registers ----
    double* Lg = V.L + M.panel_off;
    for (int c = wave; c < k; c += NW)
        for (int i = lane; i < m; i += 64) {
            const int src = (i < k) ? ord[i] : i;
            Lg[i + (size_t)c * m] = (i > c) ? F[src + c * ld] : 0.0;
        }
    for (int jj = tid; jj < k; jj += NT) { V.dinv[c0 + jj] = dinv_s[jj]; V.doff[c0 + jj] = doff_s[jj]; V.ptype[c0 + jj] = pt_s[jj]; V.lperm[c0 + jj] = ord[jj]; }
    const int mu = m - k;
    double* Cg = V.cb + M.cb_off;
#pragma unroll
    for (int y = 0; y < TS; ++y)
#pragma unroll
        for (int x = 0; x < TS; ++x) {
            const int i = row0 + x, c = col0 + y;
            if (c >= k && i >= c && i < m) Cg[(i - k) + (size_t)(c - k) * mu] = t[x][y];
        }
    if (tid == 0) V.fstat[s] = make_int4(nneg, nzero, ntwo, nsmall);
    // ---- (f) L11^{-1}: pivot-ordered unit-lower block built behind Lbuf, inverted in place ----
    double* Li = F + k * ld;
    for (int idx = tid; idx < k * k; idx += NT) { const int i = idx % k, c = idx / k; Li[i + c * ldi] = (i > c) ? F[ord[i] + c * ld] : 0.0; }
    __syncthreads();
    invert_unit_lower<NT>(Li, ldi, k);
    double* Mg = V.minv + M.minv_off;
    for (int idx = tid; idx < k * k; idx += NT) { const int i = idx % k, c = idx / k; Mg[idx] = (i > c) ? Li[i + c * ldi] : (i == c ? 1.0 : 0.0); }
#ifdef MI355X_PIVSTAT
    ph4 = clock64();
    if (NT == 256 && tid == 0) {
        const int o = (TS == 6) ? 16 : 24;
        atomicAdd(&g_fstat[o + 0], (unsigned long long)(ph1 - ph0)); atomicAdd(&g_fstat[o + 1], (unsigned long long)(ph2 - ph1));
        atomicAdd(&g_fstat[o + 2], (unsigned long long)(ph3 - ph2)); atomicAdd(&g_fstat[o + 3], (unsigned long long)(ph4 - ph3));
        atomicAdd(&g_fstat[o + 4], 1ull); atomicAdd(&g_fstat[o + 5], (unsigned long long)k); atomicAdd(&g_fstat[o + 6], (unsigned long long)(M.ch1 - M.ch0));
    }
#endif
}

// ================================================================================================
// Blocked LDL^T of a pivot block with A POSTERIORI acceptance (the fast path of the big fronts' pivot blocks; SSIDS calls the
// idea a-posteriori threshold pivoting, IpSpralSolverInterface.cpp:199-204 "pivot method block").  The strict loop above decides
// one pivot at a time behind a workgroup barrier (~1 400 cycles per pivot, 255 CUs idle on the separator chains); here
//   * the k x k block sits in LDS; 16 columns at a time, ONE wavefront eliminates the 16 x 16 diagonal block in registers in natural
//     order with 1x1 pivots -- the pivot row travels by DPP inside the wavefront, no LDS, no barrier -- and inverts its unit-lower
//     factor the same way;
//   * the rows below and the remaining columns follow by v_mfma_f64_16x16x4_f64 (ldlt_blocked_static below);
//   * nothing is decided per pivot.  The block is ACCEPTED afterwards iff every pivot is clear of the zero threshold and every
//     multiplier of the block is <= gmax = 1 / max(u, u2, 1e-4) -- the threshold test at the LARGEST u Ipopt raises its solvers to (pivtolmax = 1e-4), far
//     tighter than the 1e-8 Ipopt asks for, so an accepted block satisfies the strict rule's tests at u AND at u2 (no u-sensitive
//     decision).  Otherwise nothing has been written and the caller runs the strict loop on the untouched block.
// Returns (workgroup-uniform) true when accepted: Lb = unit-lower L (strictly lower part, natural order), dinv_s = 1 / d.
// ================================================================================================
// ---- one 16 x 16 diagonal block in ONE wavefront, no LDS, no barrier: lane (i = lane & 15) holds row i, the four 16-lane DPP rows hold
// identical copies, a[c] = column c.  The pivot row travels inside the DPP row: v_fmac_f64_dpp ... row_newbcast:c (DP-ALU DPP supports
// exactly this control on gfx950) does  a[c] += a_j[lane c] * (-l)  in one instruction -- 15 - j instructions per pivot instead of a
// workgroup barrier, a column publication and 16 register-tile FMAs per thread. ----
template <int N> __device__ __forceinline__ double bcast16(const double x) { return __builtin_amdgcn_update_dpp(x, x, 0x150 + N, 0xF, 0xF, false); }      // row_newbcast:N
#define MI_FD(c) "v_fmac_f64_dpp %" #c ", %16, -%17 row_newbcast:" #c " row_mask:0xf bank_mask:0xf\n\t"
#define MI_R15 ""
#define MI_R14 MI_FD(15)
#define MI_R13 MI_FD(14) MI_R14
#define MI_R12 MI_FD(13) MI_R13
#define MI_R11 MI_FD(12) MI_R12
#define MI_R10 MI_FD(11) MI_R11
#define MI_R9 MI_FD(10) MI_R10
#define MI_R8 MI_FD(9) MI_R9
#define MI_R7 MI_FD(8) MI_R8
#define MI_R6 MI_FD(7) MI_R7
#define MI_R5 MI_FD(6) MI_R6
#define MI_R4 MI_FD(5) MI_R5
#define MI_R3 MI_FD(4) MI_R4
#define MI_R2 MI_FD(3) MI_R3
#define MI_R1 MI_FD(2) MI_R2
#define MI_R0 MI_FD(1) MI_R1
#define MI_AOPS "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), "+v"(a[8]), "+v"(a[9]), "+v"(a[10]), "+v"(a[11]), "+v"(a[12]), "+v"(a[13]), "+v"(a[14]), "+v"(a[15])
// a[c] -= t[lane c of the row] * l   for c = J+1 .. 15   (s_nop 1: a VALU-written VGPR needs two wait states before a DPP read, and the
// compiler does not pad inside an asm statement)
template <int J> __device__ __forceinline__ void rank1_dpp16(double (&a)[16], const double t, const double l)
{
#define MI_CASE(j) if constexpr (J == j) asm("s_nop 1\n\t" MI_R##j : MI_AOPS : "v"(t), "v"(l));
    MI_CASE(0) MI_CASE(1) MI_CASE(2) MI_CASE(3) MI_CASE(4) MI_CASE(5) MI_CASE(6) MI_CASE(7) MI_CASE(8) MI_CASE(9) MI_CASE(10) MI_CASE(11) MI_CASE(12) MI_CASE(13) MI_CASE(14)
#undef MI_CASE
}
// x += x[lane J of the row] * m   (one step of the row-oriented substitution for L^{-1})
template <int J> __device__ __forceinline__ void subst_dpp16(double& x, const double m)
{
    asm("s_nop 1\n\tv_fmac_f64_dpp %0, %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "+v"(x) : "v"(m), "n"(J));
}
template <int J> __device__ __forceinline__ void diag16_step(double (&a)[16], double& rsave, const int l15)
{
    const double t = a[J];
    const double d = bcast16<J>(t);
    const double ri = fast_rcp(d);
    rsave = (l15 == J) ? ri : rsave;
    const double l = t * ri;
    rank1_dpp16<J>(a, t, l);
    a[J] = l;
}
template <int J> __device__ __forceinline__ void inv16_step(const double (&a)[16], double (&x)[4], const int l15)
{
    const double m = (l15 > J) ? -a[J] : 0.0;         // rows up to J are finished
    subst_dpp16<J>(x[0], m);
    if constexpr (J >= 4) subst_dpp16<J>(x[1], m);
    if constexpr (J >= 8) subst_dpp16<J>(x[2], m);
    if constexpr (J >= 12) subst_dpp16<J>(x[3], m);
}

// Blocked LDL^T of the k x k block in Lb (both triangles valid, ld), natural order, 16 columns at a time:
//   A  wavefront 0: the 16 x 16 diagonal block in registers (diag16_step), its inverse X = L^{-1} by the same DPP substitution, kept in
//      the operand layout of v_mfma_f64_16x16x4_f64 (lane (i, r) holds X(i, r), X(i, 4 + r), X(i, 8 + r), X(i, 12 + r));
//   B  the rows below, 16 per wavefront: W21 = A21 X^T (4 MFMAs), L21 = W21 D^{-1};
//   C  the trailing 16 x 16 tiles:  T(i, c) -= L21(i, :) W21(c, :)^T  (4 MFMAs each), spread over the wavefronts.
// Nothing is decided per pivot: the block is accepted A POSTERIORI (see above).  Isb receives the four X blocks (Isb[b*272 + i + p*17]):
// the blocked substitution of the panel rows (trsm_rows_impl) needs exactly these.
// PubHook (k_grp_fused, optimistic schedule): the results of sub-block b -- row block b of L11 left of its diagonal block, the diagonal block's inverse, its
// pivots -- go to their final places in global memory (agent-coherent stores) as soon as phase A of the sub-block is through, and the link's sub-block
// counter sflag_p is raised behind them: the workgroups that solve their panel rows against this pivot block do so 16 columns at a time, IN STEP with the
// factorisation (trsm_rows_pipe), instead of starting when all 64 columns are done.  The stores of sub-blocks 0 .. nb - 2 are issued by the three
// wavefronts that would idle through phase A of the next sub-block and are acknowledged long before the barrier they are waited for at; only the last
// sub-block's publication is on the critical chain.  Writing results before the block is ACCEPTED is what V.norestore allows (a rejection raises
// qstat[5], the factorisation is repeated without any of this).
struct PubHook { double* P; size_t ldp; double* dinvg; double* Ig; int* pflag; int fbase; };
__device__ __forceinline__ void st_coh(double* p, double v);
__device__ __forceinline__ void st_coh(int* p, int v);
__device__ __forceinline__ void publish_subblock(const PubHook& H, const double* Lb, const int ld, const int k, const double* dinv_s, const double* Isb, const int b, const int t0, const int nthr)
{
    const int c16 = 16 * b;
    for (int idx = t0; idx < 16 * c16; idx += nthr) { const int i = c16 + (idx & 15), c = idx >> 4; if (i < k) st_coh(&H.P[i + (size_t)c * H.ldp], Lb[i + c * ld]); }
    for (int idx = t0; idx < 272; idx += nthr) st_coh(&H.Ig[b * 272 + idx], Isb[b * 272 + idx]);
    if (t0 < 16 && c16 + t0 < k) st_coh(&H.dinvg[c16 + t0], dinv_s[c16 + t0]);
}
__device__ __forceinline__ bool ldlt_blocked_static(double* Lb, const int ld, const int k, double* Wb, double* dinv_s, double* Isb, int* shflag,
                                                    const double zmax, const double gmax, int& nneg, unsigned long long* dbg = nullptr, unsigned long long* ts = nullptr, const PubHook* pub = nullptr)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)blockDim.x >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int nb = (k + 15) >> 4;
    if (tid == 0) *shflag = 0;
    __syncthreads();
    int neg = 0;
#define PSTAMP(i) do { if (dbg && b == 0 && blockIdx.x == 0 && blockIdx.y == 0 && lane == 0) dbg[40 + (i)] = clock64(); } while (0)
    for (int b = 0; b < nb; ++b) {
        const int c16 = 16 * b;
        if (wave == 0) {
            const int row = c16 + l15;
            double a[16];
            PSTAMP(0);
#pragma unroll
            for (int c = 0; c < 16; ++c) {                           // (identity beyond k; the load itself is unconditional: no branch per column)
                const double v = Lb[min(row, k - 1) + min(c16 + c, k - 1) * ld];
                a[c] = (row < k && c16 + c < k) ? v : ((l15 == c) ? 1.0 : 0.0);
            }
            double rsave = 1.0;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); PSTAMP(1);
            diag16_step<0>(a, rsave, l15); diag16_step<1>(a, rsave, l15); diag16_step<2>(a, rsave, l15); diag16_step<3>(a, rsave, l15);
            diag16_step<4>(a, rsave, l15); diag16_step<5>(a, rsave, l15); diag16_step<6>(a, rsave, l15); diag16_step<7>(a, rsave, l15);
            diag16_step<8>(a, rsave, l15); diag16_step<9>(a, rsave, l15); diag16_step<10>(a, rsave, l15); diag16_step<11>(a, rsave, l15);
            diag16_step<12>(a, rsave, l15); diag16_step<13>(a, rsave, l15); diag16_step<14>(a, rsave, l15); diag16_step<15>(a, rsave, l15);
            PSTAMP(2);
            // a posteriori: multipliers of the block, pivots against the zero threshold (|d| > zmax  <=>  |1/d| < 1/zmax; inf / NaN fail)
            double gm = 0.0;
#pragma unroll
            for (int c = 0; c < 15; ++c) gm = fmax(gm, (l15 > c) ? fabs(a[c]) : 0.0);
            const bool mine = row < k;
            bool bad = __ballot(gm > gmax) != 0ull;
            bad |= __ballot(mine && !(fabs(rsave) * zmax < 1.0)) != 0ull;
            neg += __popcll(__ballot(mine && l4 == 0 && rsave < 0.0));
            PSTAMP(3);
            double x[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) x[q] = (l15 == 4 * q + l4) ? 1.0 : 0.0;
            inv16_step<0>(a, x, l15); inv16_step<1>(a, x, l15); inv16_step<2>(a, x, l15); inv16_step<3>(a, x, l15); inv16_step<4>(a, x, l15);
            inv16_step<5>(a, x, l15); inv16_step<6>(a, x, l15); inv16_step<7>(a, x, l15); inv16_step<8>(a, x, l15); inv16_step<9>(a, x, l15);
            inv16_step<10>(a, x, l15); inv16_step<11>(a, x, l15); inv16_step<12>(a, x, l15); inv16_step<13>(a, x, l15); inv16_step<14>(a, x, l15);
            PSTAMP(4);
            if (dbg && blockIdx.x == 0 && blockIdx.y == 0 && lane == 0) dbg[24 + 2 * b] = clock64();
            if (bad) { if (lane == 0) *shflag = 1; }
            else {
                if (l4 == 0 && mine) {
#pragma unroll
                    for (int c = 0; c < 16; ++c) if (c16 + c < k) Lb[row + (c16 + c) * ld] = (l15 > c) ? a[c] : 0.0;
                    dinv_s[row] = rsave;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) Isb[b * 272 + l15 + (4 * q + l4) * 17] = x[q];
            }
            PSTAMP(5);
        } else if (pub && b > 0 && wave == 1 && lane == 0) {
            __hip_atomic_store(pub->pflag, pub->fbase + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // sub-blocks 0 .. b - 1 are published (their stores were acknowledged before the barrier behind phase C)
        }
        __syncthreads();
        if (ts) { if (b == 0) ts[16] = clock64(); if (b == 1) ts[19] = clock64(); if (b == 2) ts[22] = clock64(); if (b == 3) ts[25] = clock64(); }
        if (*shflag) return false;
        if (dbg && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) dbg[25 + 2 * b] = clock64();
        if (b + 1 >= nb) {
            if (pub) {      // the last sub-block: published by everybody, at once -- the panel solves of the NEXT pivot rows are waiting for exactly this
                publish_subblock(*pub, Lb, ld, k, dinv_s, Isb, b, tid, (int)blockDim.x);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (tid == 0) __hip_atomic_store(pub->pflag, pub->fbase + b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            break;
        }
        if (pub && wave >= 1) publish_subblock(*pub, Lb, ld, k, dinv_s, Isb, b, tid - 64, (int)blockDim.x - 64);
        // ---- B: rows below the diagonal block ----
        for (int t = wave; t < nb - b - 1; t += nw) {
            const int r = c16 + 16 * (t + 1) + l15;
            v4f64_ acc = (v4f64_){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double av = Isb[b * 272 + l15 + (4 * u + l4) * 17];                       // X(c = l15, p = 4u + l4)
                const double bl = Lb[min(r, k - 1) + min(c16 + 4 * u + l4, k - 1) * ld];       // (unconditional load, clamped: no branch per operand)
                const double bv = (r < k && c16 + 4 * u + l4 < k) ? bl : 0.0;                    // A21(r, p)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
            }
            bool big = false;
#pragma unroll
            for (int g = 0; g < 4; ++g) {                                                        // acc[g] = W21(r, c = l4 + 4g)
                const int c = l4 + 4 * g;
                const double l = acc[g] * dinv_s[c16 + c];
                Wb[(r - c16) + c * 65] = acc[g];
                if (r < k && c16 + c < k) { Lb[r + (c16 + c) * ld] = l; big |= fabs(l) > gmax; }
            }
            if (__ballot(big) != 0ull && lane == 0) *shflag = 1;
        }
        __syncthreads();
        if (ts) { if (b == 0) ts[17] = clock64(); if (b == 1) ts[20] = clock64(); if (b == 2) ts[23] = clock64(); }
        if (wave == 0) PSTAMP(6);
        if (*shflag) return false;
        // ---- C: rank-16 update of the trailing tiles: T(i, c) -= sum_p L(i, c16 + p) W(c, p) ----
        {
            int q = 0;
            for (int tc = b + 1; tc < nb; ++tc)
                for (int ti = tc; ti < nb; ++ti, ++q) {
                    if (q % nw != wave) continue;
                    v4f64_ acc = (v4f64_){0.0, 0.0, 0.0, 0.0};
                    const int ri = 16 * ti + l15;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const double al = Lb[min(ri, k - 1) + min(c16 + 4 * t + l4, k - 1) * ld];
                        const double av = (ri < k && c16 + 4 * t + l4 < k) ? al : 0.0;
                        const double bv = Wb[(16 * tc - c16 + l15) + (4 * t + l4) * 65];
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
                    }
                    const int cc = 16 * tc + l15;
#pragma unroll
                    for (int g = 0; g < 4; ++g) { const int rr = 16 * ti + l4 + 4 * g; if (rr < k && cc < k) Lb[rr + cc * ld] -= acc[g]; }
                }
        }
        if (pub) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (the publication stores of this sub-block, issued two phases ago)
        __syncthreads();
        if (ts) { if (b == 0) ts[18] = clock64(); if (b == 1) ts[21] = clock64(); if (b == 2) ts[24] = clock64(); }
        if (wave == 0) PSTAMP(7);
    }
#undef PSTAMP
    nneg += neg;
    return true;
}

// ================================================================================================
// Fronts of order 65 .. 128 with k <= 16 pivots (the bulk of the 256-thread front kernel's work on 2-D problems: 33 000 fronts per
// factorisation of synth_1e6, mean k = 15): the strict loop costs ~2 700 cycles per pivot there (three workgroups share a CU).  Same idea as
// the pivot blocks of the big fronts: natural order, 1x1 pivots, nothing decided per pivot, accepted A POSTERIORI --
//   A  wavefront 0: rows 0..15 of the front in registers, the k pivots eliminated by DPP (fast16_step; the non-pivot rows k..15 ride along and
//      come out holding their Schur complement entries), X = L11^{-1} by the same DPP substitution;
//   B  the rows below, 16 per wavefront and pass: W21 = A21 X^T by 4 MFMAs, multipliers W21 D^{-1} checked;
//   -- acceptance: every multiplier of the WHOLE front column (a front of this size sees all its rows) <= gmax, every pivot clear of the zero
//      threshold; on rejection NOTHING has been written into F and the caller runs the strict loop --
//   C  the trailing 16 x 16 tiles: S(i, c) -= sum_p L(i, p) W(c, p) (4 MFMAs each) on the packed lower triangle.
// F: the assembled front, lower triangle packed by columns.  On acceptance F(i, c) = W(i, c) = L(i, c) d_c for c < k < = i..., the Schur
// complement for i >= c >= k; dinv_s = 1 / d; scratch[i + 17 p] = X(i, p) (the inverse the triangular solves use).
// ================================================================================================
template <int J> __device__ __forceinline__ void fast16_step(double (&a)[16], double (&w)[16], double& rsave, const int l15)
{
    const double t = a[J];
    w[J] = t;
    const double d = bcast16<J>(t);
    const double ri = fast_rcp(d);
    rsave = (l15 == J) ? ri : rsave;
    const double l = t * ri;
    rank1_dpp16<J>(a, t, l);
    a[J] = l;
}
template <int J> __device__ __forceinline__ void fast16_inv(const double (&a)[16], double (&x)[4], const int l15, const int k)
{
    const double m = (l15 > J && l15 < k) ? -a[J] : 0.0;         // rows up to J are finished; rows from k on are not part of L11
    subst_dpp16<J>(x[0], m);
    if constexpr (J >= 4) subst_dpp16<J>(x[1], m);
    if constexpr (J >= 8) subst_dpp16<J>(x[2], m);
    if constexpr (J >= 12) subst_dpp16<J>(x[3], m);
}
__device__ __forceinline__ bool front_fast16(double* F, const int m, const int k, double* scratch, double* dinv_s, const double* cnorm, const double small, const double gmax, int& nneg)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    auto pk = [m](int i, int c) { return c * m - ((c * (c - 1)) >> 1) + (i - c); };      // i >= c
    double* Xs = scratch;                                        // 16 x 17
    int* shflag = reinterpret_cast<int*>(scratch + 280);         // [0] rejected, [1] negative pivots
    double* cmv = scratch + 288;                                 // 16 column maxima
    // zero threshold of the front: largest |entry| of the assembled pivot columns / of the input columns
    {
        const int c = tid >> 4, part = tid & 15;
        double mx = 0.0;
        if (c < k) for (int i = part; i < m; i += 16) mx = fmax(mx, fabs(F[pk(max(i, c), min(i, c))]));
        mx = fmax(mx, dpp_f64<0xB1>(mx)); mx = fmax(mx, dpp_f64<0x4E>(mx)); mx = fmax(mx, dpp_f64<0x141>(mx)); mx = fmax(mx, dpp_f64<0x140>(mx));
        if (part == 0) cmv[c] = (c < k) ? fmax(mx, cnorm[c]) : 0.0;
        if (tid == 0) { shflag[0] = 0; shflag[1] = 0; }
    }
    __syncthreads();
    double cmx = 0.0;
#pragma unroll
    for (int c = 0; c < 16; ++c) cmx = fmax(cmx, cmv[c]);
    const double zmax = fmax(small, ZERO_REL * cmx);
    // ---- A ----
    double a[16], w[16], rsave = 1.0;
    if (wave == 0) {
#pragma unroll
        for (int c = 0; c < 16; ++c) { a[c] = F[pk(max(l15, c), min(l15, c))]; w[c] = 0.0; }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#define MI_STEP(j) if (j < k) fast16_step<j>(a, w, rsave, l15);
        MI_STEP(0) MI_STEP(1) MI_STEP(2) MI_STEP(3) MI_STEP(4) MI_STEP(5) MI_STEP(6) MI_STEP(7)
        MI_STEP(8) MI_STEP(9) MI_STEP(10) MI_STEP(11) MI_STEP(12) MI_STEP(13) MI_STEP(14) MI_STEP(15)
#undef MI_STEP
        double gm = 0.0;
#pragma unroll
        for (int c = 0; c < 15; ++c) gm = fmax(gm, (c < k && l15 > c) ? fabs(a[c]) : 0.0);
        const bool mine = l15 < k;
        bool bad = __ballot(gm > gmax) != 0ull;
        bad |= __ballot(mine && !(fabs(rsave) * zmax < 1.0)) != 0ull;
        const int neg = __popcll(__ballot(mine && l4 == 0 && rsave < 0.0));
        double x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = (l15 == 4 * q + l4) ? 1.0 : 0.0;
#define MI_INV(j) if (j + 1 < k) fast16_inv<j>(a, x, l15, k);
        MI_INV(0) MI_INV(1) MI_INV(2) MI_INV(3) MI_INV(4) MI_INV(5) MI_INV(6) MI_INV(7) MI_INV(8) MI_INV(9) MI_INV(10) MI_INV(11) MI_INV(12) MI_INV(13) MI_INV(14)
#undef MI_INV
        if (bad) { if (lane == 0) shflag[0] = 1; }
        else {
#pragma unroll
            for (int q = 0; q < 4; ++q) Xs[l15 + (4 * q + l4) * 17] = x[q];      // X(i = l15, p = 4 q + l4)
            if (l4 == 0 && mine) dinv_s[l15] = rsave;
            if (lane == 0) shflag[1] = neg;
        }
    }
    __syncthreads();
    if (shflag[0]) return false;
    // ---- B: rows 16 .. m-1, W21 = A21 X^T (kept in registers until the front is accepted) ----
    const int ntl = (m + 15) >> 4;                               // 16-row tiles of the front (tile 0 = wavefront 0's rows)
    v4f64_ wacc[2];
    int wrow[2] = {-1, -1};
    {
        bool big = false;
        int slot = 0;
        for (int t = 1 + wave; t < ntl; t += 4, ++slot) {        // (m <= 128: at most 2 tiles per wavefront)
            const int r = 16 * t + l15;
            v4f64_ acc = (v4f64_){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int p = 4 * u + l4;
                const double av = (p < k) ? Xs[l15 + p * 17] : 0.0;                  // X(c = l15, p)   (zero beyond k: columns >= k are not pivots)
                const double bv = (r < m && p < k) ? F[pk(min(r, m - 1), p)] : 0.0;   // A21(r, p)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64((l15 < k) ? av : 0.0, bv, acc, 0, 0, 0);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) { const int c = l4 + 4 * g; if (c < k && r < m) big |= fabs(acc[g] * dinv_s[c]) > gmax; }      // acc[g] = W21(r, c)
            if (slot == 0) { wacc[0] = acc; wrow[0] = r; } else { wacc[1] = acc; wrow[1] = r; }
        }
        if (__ballot(big) != 0ull && lane == 0) shflag[0] = 1;
    }
    __syncthreads();
    if (shflag[0]) return false;
    // ---- accepted: W into the first k columns of F, the Schur complement of rows k..15 ----
    nneg = shflag[1];
    if (wave == 0 && l4 == 0) {
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            if (c < k) { if (l15 > c) F[pk(l15, c)] = w[c]; }
            else if (l15 >= c) F[pk(l15, c)] = a[c];
        }
    }
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
        const int r = wrow[sl];
        if (r >= 0 && r < m) {
#pragma unroll
            for (int g = 0; g < 4; ++g) { const int c = l4 + 4 * g; if (c < k) F[pk(r, c)] = wacc[sl][g]; }
        }
    }
    __syncthreads();
    // ---- C: S(i, c) -= sum_p L(i, p) W(c, p),  i >= 16, i >= c >= k ----
    {
        int q = 0;
        for (int tc = 0; tc < ntl; ++tc)
            for (int ti = max(tc, 1); ti < ntl; ++ti, ++q) {
                if ((q & 3) != wave) continue;
                v4f64_ acc = (v4f64_){0.0, 0.0, 0.0, 0.0};
                const int ri = 16 * ti + l15, rc = 16 * tc + l15;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int p = 4 * t + l4;
                    const double av = (ri < m && p < k) ? F[pk(min(ri, m - 1), p)] * dinv_s[min(p, 15)] : 0.0;       // L(ri, p)
                    const double bv = (rc < m && rc >= k && p < k) ? F[pk(min(max(rc, p), m - 1), p)] : 0.0;        // W(rc, p)   (rc >= k > p)
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
                }
                const int cc = 16 * tc + l15;
#pragma unroll
                for (int g = 0; g < 4; ++g) { const int rr = 16 * ti + l4 + 4 * g; if (rr < m && cc >= k && rr >= cc) F[pk(rr, cc)] -= acc[g]; }
            }
    }
    __syncthreads();
    return true;
}

// ================================================================================================
// Fronts of order <= 16 (the LukVl regime: 10^5 of them per tree level): FOUR fronts per wavefront, one per 16-lane DPP row, on the static-order
// path -- lane i of a row holds row i of its front in 16 registers, the pivots are eliminated by DPP (masked per front by its own pivot
// count), L11^{-1} by the same DPP substitution, everything accepted A POSTERIORI (every multiplier of the front <= gmax, every pivot clear
// of the zero threshold); a front that fails is left to the strict kernel launched behind (hasis[s] != 2).  The register-tiled kernel gives
// such a front a whole wavefront (8 x 8 threads with 2 x 2 tiles) and ~20 us of mostly latency; here four fronts share the latency and
// the instruction stream.
// ================================================================================================
template <int J> __device__ __forceinline__ void fast16_step_masked(double (&a)[16], double& rsave, const int l15, const bool on)
{
    const double t = a[J];
    const double d = bcast16<J>(t);
    const double ri = on ? fast_rcp(d) : 0.0;
    rsave = (on && l15 == J) ? ri : rsave;
    const double l = on ? t * ri : 0.0;
    rank1_dpp16<J>(a, t, l);
    a[J] = on ? l : t;
}
// DF (k_front_df): the fronts of SEVERAL tree levels in one persistent launch.  A front whose parent is handled by the same launch publishes its contribution
// block as TAGGED entries -- {value, epoch of this factorisation} in one 16-byte agent-coherent store each, a 16 x 16 square of them (cbt, cbt_off) -- and the
// parent polls the entries themselves: value and tag arrive together, so there is no flag, no wait for acknowledgements and no second round trip between a child
// finishing and its parent starting (the fence-free messages of the solve sweeps; a flag per front was measured first: 14 us per tree level, four dependent
// round trips).  Children factored by an earlier launch are read as ever.  Same arithmetic: the same bits.
__device__ __forceinline__ void st_coh(double* p, double v);
__device__ __forceinline__ void st_coh(int* p, int v);
__device__ __forceinline__ void st_tagged(v2d* p, const double v, const double ep) { const v2d m = (v2d){v, ep}; asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(p), "v"(m) : "memory"); }
// row `li` of a child's tagged 16 x 16 square (leading dimension 16): all 16 entries requested at once, one wait
__device__ __forceinline__ void ld_tagged_row16(const v2d* p, v2d (&r)[16])
{
    asm volatile("global_load_dwordx4 %0, %16, off sc1\n\tglobal_load_dwordx4 %1, %16, off offset:256 sc1\n\tglobal_load_dwordx4 %2, %16, off offset:512 sc1\n\tglobal_load_dwordx4 %3, %16, off offset:768 sc1\n\t"
                 "global_load_dwordx4 %4, %16, off offset:1024 sc1\n\tglobal_load_dwordx4 %5, %16, off offset:1280 sc1\n\tglobal_load_dwordx4 %6, %16, off offset:1536 sc1\n\tglobal_load_dwordx4 %7, %16, off offset:1792 sc1\n\t"
                 "global_load_dwordx4 %8, %16, off offset:2048 sc1\n\tglobal_load_dwordx4 %9, %16, off offset:2304 sc1\n\tglobal_load_dwordx4 %10, %16, off offset:2560 sc1\n\tglobal_load_dwordx4 %11, %16, off offset:2816 sc1\n\t"
                 "global_load_dwordx4 %12, %16, off offset:3072 sc1\n\tglobal_load_dwordx4 %13, %16, off offset:3328 sc1\n\tglobal_load_dwordx4 %14, %16, off offset:3584 sc1\n\tglobal_load_dwordx4 %15, %16, off offset:3840 sc1\n\t"
                 "s_waitcnt vmcnt(0)"
                 : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3]), "=&v"(r[4]), "=&v"(r[5]), "=&v"(r[6]), "=&v"(r[7]), "=&v"(r[8]), "=&v"(r[9]), "=&v"(r[10]), "=&v"(r[11]), "=&v"(r[12]), "=&v"(r[13]), "=&v"(r[14]), "=&v"(r[15])
                 : "v"(p) : "memory");
}
// the waits of the data-flow launches are BOUNDED (a device shared with other work may not hold the whole launch resident); once one wait has timed out
// nobody waits its own bound out; factor() repeats with the full schedule (qstat[4], qstat[6])
__device__ __forceinline__ bool df_wait_expired(const DevView& V, const int spins)
{
    if (spins > (1 << 22) || ((spins & 1023) == 0 && __hip_atomic_load(&V.qstat[6], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) { V.qstat[6] = 1; V.qstat[4] = 1; return true; }
    return false;
}
template <bool DF>
__device__ __forceinline__ void front_dpp16_body(const DevView& V, double (&Fs)[4][16 * 17], int (&relS)[4][16], const int list_off, const int nfronts, const int quad, const int top_mode, const int no_strict_behind, const int epoch)
{
    const int lane = threadIdx.x, g = lane >> 4, li = lane & 15;
    const int f = 4 * quad + g;
    const FrontMeta* Mp = V.fmeta + list_off + min(f, nfronts - 1);
    const int s = Mp->s, c0 = Mp->c0;
    const int m0 = Mp->m;
    const bool act = f < nfronts && m0 <= 16;                    // (larger fronts of the bucket: the strict kernel's)
    const int k = act ? Mp->k : 0, m = act ? m0 : 1;
    double* F = Fs[g];
    // ---- assembly: full symmetric 16 x 17 square per front ----
    const bool from_arena = act && top_mode && V.arena && V.arena_off[s] >= 0;
    const bool skip_owned = top_mode && V.arena;
    for (int idx = li; idx < 16 * 17; idx += 16) F[idx] = 0.0;
    if (from_arena) {
        const double* Ar = V.arena + V.arena_off[s];
        for (int idx = li; idx < m * m; idx += 16) { const int i = idx % m, c = idx / m; if (i >= c) { const double v = Ar[c * m - ((c * (c - 1)) >> 1) + (i - c)]; F[i + 17 * c] = v; F[c + 17 * i] = v; } }      // (packed lower triangle)
    }
    // DF: what does not depend on the children is requested before anything is waited for -- the first four child records, where my row of each child lands in
    // this front, the input entries -- so that behind a child's flag there is ONE dependent access left (its contribution block)
    int pch[4] = {-1, -1, -1, -1}, pmc[4] = {0, 0, 0, 0}, pldt[4] = {0, 0, 0, 0}, prl[4] = {0, 0, 0, 0}; const double* pC[4] = {nullptr, nullptr, nullptr, nullptr}; long long pto[4] = {-1, -1, -1, -1};
    const double ep = (double)epoch;
    if (DF && act) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (Mp->ch0 + c < Mp->ch1) {
                const ChildMeta* Cp = V.cmeta + Mp->ch0 + c;
                pch[c] = Cp->ch; pmc[c] = Cp->mc; pldt[c] = Cp->ldt; pC[c] = V.cb + Cp->cb_off;
                prl[c] = (li < pmc[c]) ? V.rel[Cp->relbase + li] : 0;
                pto[c] = V.cbt_off[pch[c]];
            }
    }
    if (act) {
        for (int q = Mp->aq0 + li; q < Mp->aq1; q += 16) {
            const int pos = V.apos[q]; const int i = pos % m, c = pos / m; const double v = V.aval[q];
            F[i + 17 * c] += v; if (i != c) F[c + 17 * i] += v;
        }
        if (DF) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (pch[c] >= 0) {
                    const int mc = pmc[c], ldt = pldt[c];
                    const bool mine = li < mc;
                    if (mine) relS[g][li] = prl[c];
                    double cv[16];
                    if (pto[c] >= 0) {      // a child of this launch: its tagged square, polled until every entry of my row carries this factorisation's tag
                        const v2d* Tp = V.cbt + pto[c] + li;
                        v2d tv[16];
                        int spins = 0;
                        while (true) {
                            ld_tagged_row16(Tp, tv);
                            bool all = true;
#pragma unroll
                            for (int b = 0; b < 16; ++b) if (mine && b <= li && tv[b].y != ep) all = false;
                            if (all) break;
                            __builtin_amdgcn_s_sleep(1);
                            if (df_wait_expired(V, ++spins)) break;
                        }
#pragma unroll
                        for (int b = 0; b < 16; ++b) cv[b] = (mine && b <= li) ? tv[b].x : 0.0;
                    } else {
                        const double* C = pC[c];
#pragma unroll
                        for (int b = 0; b < 16; ++b) cv[b] = (mine && b <= li) ? C[li + (size_t)b * ldt] : 0.0;
                    }
                    const int ra = relS[g][li];
#pragma unroll
                    for (int b = 0; b < 16; ++b)
                        if (mine && b <= li) { const int rb = relS[g][b]; F[ra + 17 * rb] += cv[b]; if (ra != rb) F[rb + 17 * ra] += cv[b]; }
                }
        }
        for (int cp = Mp->ch0 + (DF ? 4 : 0); cp < Mp->ch1; ++cp) {
            const ChildMeta* Cp = V.cmeta + cp;
            if (skip_owned && Cp->owner >= 0) continue;
            const int mc = Cp->mc, ldt = Cp->ldt;                  // (mc <= m <= 16: lane li owns row li of the child's lower triangle)
            const double* C = V.cb + Cp->cb_off;
            const bool mine = li < mc;
            if (mine) relS[g][li] = V.rel[Cp->relbase + li];
            double cv[16];
            const long long to = DF ? V.cbt_off[Cp->ch] : -1;
            if (DF && to >= 0) {      // (a fifth, sixth ... child of this launch: rare)
                const v2d* Tp = V.cbt + to + li;
                v2d tv[16];
                int spins = 0;
                while (true) {
                    ld_tagged_row16(Tp, tv);
                    bool all = true;
#pragma unroll
                    for (int b = 0; b < 16; ++b) if (mine && b <= li && tv[b].y != ep) all = false;
                    if (all) break;
                    __builtin_amdgcn_s_sleep(1);
                    if (df_wait_expired(V, ++spins)) break;
                }
#pragma unroll
                for (int b = 0; b < 16; ++b) cv[b] = (mine && b <= li) ? tv[b].x : 0.0;
            } else {
#pragma unroll
            for (int b = 0; b < 16; ++b) cv[b] = (mine && b <= li) ? C[li + (size_t)b * ldt] : 0.0;
            }
            const int ra = relS[g][li];
#pragma unroll
            for (int b = 0; b < 16; ++b)
                if (mine && b <= li) { const int rb = relS[g][b]; F[ra + 17 * rb] += cv[b]; if (ra != rb) F[rb + 17 * ra] += cv[b]; }
        }
    }
    double a[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) a[c] = F[li + 17 * c];
    // ---- zero threshold of the front: largest |entry| of its assembled pivot columns / of the input columns ----
    double cmine = 0.0;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        double mx = fabs(a[c]);
        mx = fmax(mx, dpp_f64<0xB1>(mx)); mx = fmax(mx, dpp_f64<0x4E>(mx)); mx = fmax(mx, dpp_f64<0x141>(mx)); mx = fmax(mx, dpp_f64<0x140>(mx));
        cmine = (li == c) ? mx : cmine;
    }
    double cmx = (li < k) ? fmax(cmine, V.cnorm[c0 + li]) : 0.0;
    cmx = fmax(cmx, dpp_f64<0xB1>(cmx)); cmx = fmax(cmx, dpp_f64<0x4E>(cmx)); cmx = fmax(cmx, dpp_f64<0x141>(cmx)); cmx = fmax(cmx, dpp_f64<0x140>(cmx));
    const double zmax = fmax(V.small, ZERO_REL * cmx);
    const double gmax = 1.0 / fmax(fmax(V.pivtol, V.pivtol2), V.fastu);
    // ---- elimination (every front of the wavefront walks the same steps, masked by its own pivot count) ----
    double rsave = 1.0;
    const int kw = max(max(__builtin_amdgcn_readlane(k, 0), __builtin_amdgcn_readlane(k, 16)), max(__builtin_amdgcn_readlane(k, 32), __builtin_amdgcn_readlane(k, 48)));
#define MI_STEP(j) if (j < kw) fast16_step_masked<j>(a, rsave, li, j < k);
    MI_STEP(0) MI_STEP(1) MI_STEP(2) MI_STEP(3) MI_STEP(4) MI_STEP(5) MI_STEP(6) MI_STEP(7)
    MI_STEP(8) MI_STEP(9) MI_STEP(10) MI_STEP(11) MI_STEP(12) MI_STEP(13) MI_STEP(14) MI_STEP(15)
#undef MI_STEP
    double gm = 0.0;
#pragma unroll
    for (int c = 0; c < 15; ++c) gm = fmax(gm, (c < k && li > c) ? fabs(a[c]) : 0.0);
    const bool pv = li < k;
    const unsigned long long badm = __ballot(gm > gmax) | __ballot(pv && !(fabs(rsave) * zmax < 1.0));
    const unsigned long long negm = __ballot(pv && rsave < 0.0);
    const bool ok = act && ((badm >> (16 * g)) & 0xffffull) == 0ull;
    if (act && li == 0) { V.hasis[s] = ok ? 2 : 0; if (!ok && no_strict_behind) V.qstat[4] = 1; }      // (qstat[4]: a front is left for a strict kernel the optimistic schedule did not launch: numeric.hip factor())
    const long long myto = (DF && act) ? V.cbt_off[s] : -1;
    if (DF && act && myto >= 0) {      // the parent is a front of this launch: the contribution block goes out as tagged entries before the inverse and the factor are even written
        v2d* Tg = V.cbt + myto;        // (a REJECTED front publishes too -- whatever it holds: nobody may wait for it, and qstat[4] has the factorisation repeated)
#pragma unroll
        for (int c = 0; c < 16; ++c) if (c >= k && li >= c && li < m) st_tagged(&Tg[(li - k) + 16 * (c - k)], a[c], ep);
    }
    // ---- L11^{-1}: row li of X in 16 registers, DPP substitution ----
    double x[16];
#pragma unroll
    for (int p = 0; p < 16; ++p) x[p] = (p == li) ? 1.0 : 0.0;
#define MI_INV(j) if (j + 1 < kw) { const double mj = (li > j && li < k) ? -a[j] : 0.0; _Pragma("unroll") for (int p = 0; p <= j; ++p) subst_dpp16<j>(x[p], mj); }
    MI_INV(0) MI_INV(1) MI_INV(2) MI_INV(3) MI_INV(4) MI_INV(5) MI_INV(6) MI_INV(7) MI_INV(8) MI_INV(9) MI_INV(10) MI_INV(11) MI_INV(12) MI_INV(13) MI_INV(14)
#undef MI_INV
    if (!ok) return;
    // ---- results ----
    double* Lg = V.L + Mp->panel_off;
    double* Cg = V.cb + Mp->cb_off;
    double* Mg = V.minv + Mp->minv_off;
    const int mu = m - k;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (c < k) {
            if (li < m) Lg[li + (size_t)c * m] = (li > c) ? a[c] : 0.0;
            if (li < k) Mg[li + (size_t)c * k] = (li > c) ? x[c] : (li == c ? 1.0 : 0.0);
        } else if (myto < 0 && li >= c && li < m) Cg[(li - k) + (size_t)(c - k) * mu] = a[c];      // (read by a front of a later launch -- or by nobody but the tagged copy's reader)
    }
    if (pv) { V.dinv[c0 + li] = rsave; V.doff[c0 + li] = 0.0; V.ptype[c0 + li] = 1; V.lperm[c0 + li] = li; }
    if (li == 0) V.fstat[s] = make_int4(__popcll((negm >> (16 * g)) & 0xffffull), 0, 0, 0);
}
__global__ __launch_bounds__(64) void k_front_dpp16(DevView V, int list_off, int nfronts, int top_mode, int no_strict_behind)
{
    __shared__ double Fs[4][16 * 17];
    __shared__ int relS[4][16];
    front_dpp16_body<false>(V, Fs, relS, list_off, nfronts, (int)blockIdx.x, top_mode, no_strict_behind, 0);
}

// ================================================================================================
// A front of order 17 .. 32 on ONE wavefront, static order, accepted a posteriori -- the plain statement of what k_front_dpp16 does for order <= 16, on a
// 32 x 33 square in LDS (lane = row, the two halves of the wavefront take alternate columns of the rank-1 update).  Not a fast kernel and not meant to be:
// a banded KKT system has a handful of such fronts (LukVlE1 10^6: 2 of 180 484, order 18) -- but each of them used to cost its tree level a launch of the
// strict kernel (27-32 us, 8 % of the factorisation) and, worse, would cut the run of levels k_front_df covers.  Rules as in k_front_dpp16: natural order, 1x1
// pivots, every multiplier <= gmax, every pivot clear of the zero threshold, otherwise the front is rejected (hasis 0, qstat[4]: the factorisation is repeated
// with the strict kernels).  DF as above.
// ================================================================================================
template <int NT> __device__ __forceinline__ void invert_unit_lower(double* F, const int ld, const int k);
template <bool DF>
__device__ __forceinline__ void front_lds32_body(const DevView& V, double* G, int* relS, const FrontMeta* Mp, const int no_strict_behind, const int epoch)
{
    const int lane = threadIdx.x & 63, row = lane & 31, half = lane >> 5;
    const int s = Mp->s, c0 = Mp->c0, k = Mp->k, m = Mp->m;
    constexpr int LD = 33;
    for (int idx = lane; idx < 32 * LD; idx += 64) G[idx] = 0.0;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier();
    for (int q = Mp->aq0 + lane; q < Mp->aq1; q += 64) {
        const int pos = V.apos[q]; const int i = pos % m, c = pos / m; const double v = V.aval[q];
        G[i + LD * c] += v; if (i != c) G[c + LD * i] += v;      // (one slot per position: no two lanes add to the same entry)
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier();
    for (int cp = Mp->ch0; cp < Mp->ch1; ++cp) {
        const ChildMeta* Cp = V.cmeta + cp;
        const int mc = Cp->mc, ldt = Cp->ldt;
        const double* C = V.cb + Cp->cb_off;
        const long long to = DF ? V.cbt_off[Cp->ch] : -1;      // (a child of this launch: its tagged square, leading dimension 16: a child of a one-wavefront front has at most 16 update rows... or 32)
        const int tld = mc <= 16 ? 16 : 32;
        if (lane < mc) relS[lane] = V.rel[Cp->relbase + lane];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier();
        for (int e = lane; e < mc * mc; e += 64) {
            const int a = e % mc, b = e / mc;
            if (a < b) continue;
            double v;
            if (to >= 0) {
                const v2d* q = V.cbt + to + a + tld * b;
                v2d t; int spins = 0;
                while (true) { asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(t) : "v"(q) : "memory"); if (t.y == (double)epoch) break; __builtin_amdgcn_s_sleep(1); if (df_wait_expired(V, ++spins)) break; }
                v = t.x;
            } else v = C[a + (size_t)b * ldt];
            const int ra = relS[a], rb = relS[b];
            G[ra + LD * rb] += v; if (ra != rb) G[rb + LD * ra] += v;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier();
    }
    // zero threshold: largest |entry| of the assembled pivot columns / of the input columns
    double cmx = 0.0;
    if (half == 0 && row < k) { for (int i = 0; i < m; ++i) cmx = fmax(cmx, fabs(G[i + LD * row])); cmx = fmax(cmx, V.cnorm[c0 + row]); }
    cmx = wave_max_all(cmx);
    const double zmax = fmax(V.small, ZERO_REL * cmx);
    const double gmax = 1.0 / fmax(fmax(V.pivtol, V.pivtol2), V.fastu);
    bool bad = false; int nneg = 0;
    double gm = 0.0, myd = 1.0;
    for (int j = 0; j < k; ++j) {
        const double d = G[j + LD * j];
        const double ri = fast_rcp(d);
        if (!(fabs(ri) * zmax < 1.0)) bad = true;
        if (d < 0.0) ++nneg;
        if (row == j) myd = ri;
        const double t = (row > j && row < m) ? G[row + LD * j] : 0.0;     // my row's entry of the pivot column (W), l = t / d
        const double l = t * ri;
        for (int c = j + 1 + half; c < m; c += 2) {                          // columns of the trailing square: the two halves alternate
            const double tc = G[c + LD * j];
            if (row > j && row < m) G[row + LD * c] = fma(-l, tc, G[row + LD * c]);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier();
        if (half == 0 && row > j && row < m) { G[row + LD * j] = l; gm = fmax(gm, fabs(l)); }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier();
    }
    bad = bad || (__ballot(gm > gmax) != 0ull);
    const bool ok = !bad;
    // (hasis[s] stays 0: the mark "done by the static-order kernel in front" is only reset per factorisation for fronts of order <= 16 -- a 2 left here
    // made the strict kernel of the FULL schedule skip this front in every later factorisation.  This body has no strict launch behind it.)
    if (lane == 0) { V.hasis[s] = 0; if (!ok && no_strict_behind) V.qstat[4] = 1; }
    const long long myto = DF ? V.cbt_off[s] : -1;
    if (myto >= 0) {      // (published whether accepted or not: nobody may wait for a rejected front)
        const int mu = m - k, tld = mu <= 16 ? 16 : 32;
        for (int c = k + half; c < m; c += 2) if (row >= c && row < m) st_tagged(V.cbt + myto + (row - k) + tld * (c - k), G[row + LD * c], (double)epoch);
    }
    if (!ok) return;
    double* Lg = V.L + Mp->panel_off;
    double* Cg = V.cb + Mp->cb_off;
    double* Mg = V.minv + Mp->minv_off;
    const int mu = m - k;
    for (int c = half; c < m; c += 2) {
        if (c < k) { if (row < m) Lg[row + (size_t)c * m] = (row > c) ? G[row + LD * c] : 0.0; }
        else if (myto < 0 && row >= c && row < m) Cg[(row - k) + (size_t)(c - k) * mu] = G[row + LD * c];
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier();
    // L11^{-1} in place (the strictly lower part of the leading k x k block of G; its mirror positions are free scratch): the recursive doubling every front kernel uses
    invert_unit_lower<64>(G, LD, k);
    for (int c = half; c < k; c += 2) if (row < k) Mg[row + (size_t)c * k] = (row > c) ? G[row + LD * c] : (row == c ? 1.0 : 0.0);
    if (half == 0 && row < k) { V.dinv[c0 + row] = myd; V.doff[c0 + row] = 0.0; V.ptype[c0 + row] = 1; V.lperm[c0 + row] = row; }
    if (lane == 0) V.fstat[s] = make_int4(nneg, 0, 0, 0);
}

// ================================================================================================
// SEVERAL TREE LEVELS OF SMALL FRONTS IN ONE LAUNCH (the LukVl regime above the leaf chains: 15 levels of 8 196 .. 4 fronts of order <= 18, each a launch of
// ~19 us whatever its size -- 0.34 of the 0.78 ms of a factorisation of LukVlE1 10^6: the chain front record -> child records -> child blocks -> arithmetic ->
// stores is paid per LEVEL).  A run of consecutive levels that hold nothing but one-wavefront fronts becomes one persistent launch: virtual workgroups in
// level order (four fronts of order <= 16 each, or one front of order 17 .. 32), dealt round-robin to a grid that fits the chip; a front waits for its own
// children only (flags), so the levels overlap wherever the tree allows and a front starts the moment its children are done.  All workgroups are resident
// and every workgroup takes its virtual workgroups in ascending order, children before parents: no wait can be circular.  Optimistic schedule only (a
// rejected front raises qstat[4]: the factorisation is repeated level by level with the strict kernels).
// ================================================================================================
__global__ __launch_bounds__(64) void k_front_df(DevView V, const DfLevel* lv, int nlev, int nq)
{
    __shared__ double Fs[4][16 * 17];      // (one front of order 17 .. 32 uses the four squares as its 32 x 33 one)
    __shared__ int relS[4][16];
    const int epoch = V.sepoch[2];
    int l = 0;
    DfLevel L = lv[0];
    for (int q = blockIdx.x; q < nq; q += gridDim.x) {
        while (l + 1 < nlev && q >= lv[l + 1].q0) { ++l; L = lv[l]; }
        const int loc = q - L.q0, nq16 = (L.n16 + 3) >> 2;
        const bool probe = V.dbg && loc == 0 && l >= nlev - 12 && threadIdx.x == 0;      // (development: when the first virtual workgroup of each of the last levels starts and ends, 100 MHz wall clock)
        if (probe) V.dbg[96 + 2 * (l - (nlev - 12))] = wall_clock64();
        if (loc < nq16) front_dpp16_body<true>(V, Fs, relS, L.b0, L.n16, loc, 0, 1, epoch);
        else front_lds32_body<true>(V, &Fs[0][0], &relS[0][0], V.fmeta + L.b0 + L.n16 + (loc - nq16), 1, epoch);
        if (probe) V.dbg[97 + 2 * (l - (nlev - 12))] = wall_clock64();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __builtin_amdgcn_wave_barrier();      // (the LDS squares are reused by the next virtual workgroup)
    }
}


// ================================================================================================
// LEAF CHAINS (the LukVl regime: the bottom of the tree is 10^4..10^5 chains of a few fronts of order <= 16, every front the only child of the next --
// a banded KKT system's leaf domains): a 16-lane DPP row walks its WHOLE chain, front after front, in one launch.  The contribution block of a link never
// leaves the registers it is computed in (it is extend-added into the next link's square in LDS by the lanes that hold it; only the last link's goes to
// memory, for the chain's parent), and the levels of the chains are ONE launch instead of one per level.  Same arithmetic as k_front_dpp16, step by step:
// the factors are bit-identical.  Part of the optimistic schedule only: a front that fails the a-posteriori test stops its chain and raises qstat[4];
// factor() then runs the full per-level schedule with the same values.
// ================================================================================================
__global__ __launch_bounds__(64) void k_leaf_chain(DevView V, int nchains)
{
    __shared__ double Fs[4][16 * 17];
    __shared__ int relS[4][16];
    const int lane = threadIdx.x, g = lane >> 4, li = lane & 15;
    const int ch = 4 * (int)blockIdx.x + g;
    const bool cact = ch < nchains;
    const int l0 = V.lc_ptr[min(ch, nchains - 1)];
    const int nl = cact ? V.lc_ptr[min(ch, nchains - 1) + 1] - l0 : 0;
    const int nlw = max(max(__builtin_amdgcn_readlane(nl, 0), __builtin_amdgcn_readlane(nl, 16)), max(__builtin_amdgcn_readlane(nl, 32), __builtin_amdgcn_readlane(nl, 48)));
    double* F = Fs[g];
    double a[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) a[c] = 0.0;
    int kprev = 0, mprev = 0;
    bool alive = cact;
    const double gmax = 1.0 / fmax(fmax(V.pivtol, V.pivtol2), V.fastu);
    // what a link needs from memory is requested a link ahead: its record two links ahead, its input entries (the first 48: three per lane), the scale of its
    // columns and its rows' positions in its parent one link ahead -- per link one dependent round trip is left (the record of the link after next)
    const LeafLink* Lc = V.lc_link + l0;
    const int nlc = max(nl, 1);
    LeafLink K0 = Lc[0], K1 = Lc[min(1, nlc - 1)];
    int pos0[3], pos1[3]; double val0[3], val1[3]; double cn0, cn1; int rl0, rl1, rlp = 0;      // rlp: where the previous link's row `li` sits in this link
    auto request = [&](const LeafLink& K, const bool on, int (&pos)[3], double (&val)[3], double& cn, int& rl) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { const int q = K.aq0 + li + 16 * j; const bool v = on && q < K.aq1; pos[j] = v ? V.apos[q] : -1; val[j] = v ? V.aval[q] : 0.0; }
        cn = (on && li < K.k) ? V.cnorm[K.c0 + li] : 0.0;
        rl = (on && li >= K.k && li < K.m) ? V.rel[K.relbase + li - K.k] : 0;      // (relbase of a link = where ITS rows sit in ITS parent: used by the next link)
    };
    request(K0, nl > 0, pos0, val0, cn0, rl0);
#pragma unroll 1
    for (int t = 0; t < nlw; ++t) {
        const bool act = alive && t < nl;
        const LeafLink K2 = Lc[min(t + 2, nlc - 1)];
        request(K1, t + 1 < nl, pos1, val1, cn1, rl1);
        const int s = K0.s, c0 = K0.c0;
        const int k = act ? K0.k : 0, m = act ? K0.m : 1;
        // ---- assembly: full symmetric 16 x 17 square; the child (the previous link) comes out of the registers ----
        for (int idx = li; idx < 16 * 17; idx += 16) F[idx] = 0.0;
        if (act) {
#pragma unroll
            for (int j = 0; j < 3; ++j) if (pos0[j] >= 0) { const int i = pos0[j] % m, c = pos0[j] / m; F[i + 17 * c] += val0[j]; if (i != c) F[c + 17 * i] += val0[j]; }
            for (int q = K0.aq0 + 48 + li; q < K0.aq1; q += 16) {
                const int pos = V.apos[q]; const int i = pos % m, c = pos / m; const double v = V.aval[q];
                F[i + 17 * c] += v; if (i != c) F[c + 17 * i] += v;
            }
            if (t > 0) {
                const bool mine = li >= kprev && li < mprev;                 // lane li holds row li of the child's front: its update entries are columns kprev .. li
                if (mine) relS[g][li - kprev] = rlp;
                const int ra = mine ? rlp : 0;
#pragma unroll
                for (int b = 0; b < 16; ++b)
                    if (mine && b >= kprev && b <= li) { const int rb = relS[g][b - kprev]; F[ra + 17 * rb] += a[b]; if (ra != rb) F[rb + 17 * ra] += a[b]; }
            }
        }
#pragma unroll
        for (int c = 0; c < 16; ++c) a[c] = F[li + 17 * c];
        // ---- zero threshold of the front ----
        double cmine = 0.0;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            double mx = fabs(a[c]);
            mx = fmax(mx, dpp_f64<0xB1>(mx)); mx = fmax(mx, dpp_f64<0x4E>(mx)); mx = fmax(mx, dpp_f64<0x141>(mx)); mx = fmax(mx, dpp_f64<0x140>(mx));
            cmine = (li == c) ? mx : cmine;
        }
        double cmx = (li < k) ? fmax(cmine, cn0) : 0.0;
        cmx = fmax(cmx, dpp_f64<0xB1>(cmx)); cmx = fmax(cmx, dpp_f64<0x4E>(cmx)); cmx = fmax(cmx, dpp_f64<0x141>(cmx)); cmx = fmax(cmx, dpp_f64<0x140>(cmx));
        const double zmax = fmax(V.small, ZERO_REL * cmx);
        // ---- elimination ----
        double rsave = 1.0;
        const int kw = max(max(__builtin_amdgcn_readlane(k, 0), __builtin_amdgcn_readlane(k, 16)), max(__builtin_amdgcn_readlane(k, 32), __builtin_amdgcn_readlane(k, 48)));
#define MI_STEP(j) if (j < kw) fast16_step_masked<j>(a, rsave, li, j < k);
        MI_STEP(0) MI_STEP(1) MI_STEP(2) MI_STEP(3) MI_STEP(4) MI_STEP(5) MI_STEP(6) MI_STEP(7)
        MI_STEP(8) MI_STEP(9) MI_STEP(10) MI_STEP(11) MI_STEP(12) MI_STEP(13) MI_STEP(14) MI_STEP(15)
#undef MI_STEP
        double gm = 0.0;
#pragma unroll
        for (int c = 0; c < 15; ++c) gm = fmax(gm, (c < k && li > c) ? fabs(a[c]) : 0.0);
        const bool pv = li < k;
        const unsigned long long badm = __ballot(gm > gmax) | __ballot(pv && !(fabs(rsave) * zmax < 1.0));
        const unsigned long long negm = __ballot(pv && rsave < 0.0);
        const bool ok = act && ((badm >> (16 * g)) & 0xffffull) == 0ull;
        if (act && li == 0) { V.hasis[s] = ok ? 2 : 0; if (!ok) V.qstat[4] = 1; }
        // ---- L11^{-1} ----
        double x[16];
#pragma unroll
        for (int p = 0; p < 16; ++p) x[p] = (p == li) ? 1.0 : 0.0;
#define MI_INV(j) if (j + 1 < kw) { const double mj = (li > j && li < k) ? -a[j] : 0.0; _Pragma("unroll") for (int p = 0; p <= j; ++p) subst_dpp16<j>(x[p], mj); }
        MI_INV(0) MI_INV(1) MI_INV(2) MI_INV(3) MI_INV(4) MI_INV(5) MI_INV(6) MI_INV(7) MI_INV(8) MI_INV(9) MI_INV(10) MI_INV(11) MI_INV(12) MI_INV(13) MI_INV(14)
#undef MI_INV
        if (act && !ok) alive = false;                                       // (the chain stops here: the full schedule will redo everything)
        if (ok) {
            double* Lg = V.L + K0.panel_off;
            double* Mg = V.minv + K0.minv_off;
            const bool last = t == nl - 1;
            double* Cg = V.cb + K0.cb_off;
            const int mu = m - k;
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                if (c < k) {
                    if (li < m) Lg[li + (size_t)c * m] = (li > c) ? a[c] : 0.0;
                    if (li < k) Mg[li + (size_t)c * k] = (li > c) ? x[c] : (li == c ? 1.0 : 0.0);
                } else if (last && li >= c && li < m) Cg[(li - k) + (size_t)(c - k) * mu] = a[c];
            }
            if (pv) { V.dinv[c0 + li] = rsave; V.doff[c0 + li] = 0.0; V.ptype[c0 + li] = 1; V.lperm[c0 + li] = li; }
            if (li == 0) V.fstat[s] = make_int4(__popcll((negm >> (16 * g)) & 0xffffull), 0, 0, 0);
        }
        kprev = k; mprev = m; rlp = rl0;
        K0 = K1; K1 = K2;
#pragma unroll
        for (int j = 0; j < 3; ++j) { pos0[j] = pos1[j]; val0[j] = val1[j]; }
        cn0 = cn1; rl0 = rl1;
    }
}

// pivot block of a BIG front on the register-tiled core: 4x4 tiles on 16x16 threads for k <= 64, on 32x32 threads (two-word
// alive mask) for the 128-column panels of the wide_panels option (19 ms against 28 ms with 8x8 tiles on 256 threads, but
// still slower per column than two 64-column blocks: option off by default)
__device__ __forceinline__ void chain_signal(int* flag, const int epoch);
__device__ __forceinline__ void chain_signal_coh(int* flag, const int epoch);      // (kernels_solve.hip.inc: the flag without the release fence, for data stored agent-coherently)
__device__ __forceinline__ void st_coh(double* p, double v);
__device__ __forceinline__ void st_coh(int* p, int v);
__device__ __forceinline__ void st16_coh(double* p, double v0, double v1);
template <int NAP = 2> __device__ __forceinline__ void chain_wait(const int* flag, const int epoch, int* err);
// PRE: the caller has left the assembled, fully updated block in Lb (lower triangle) AND in the panel storage; late_*: a row block's L21 the
// caller kept back in LDS, stored once the flag is up (off the critical chain)
__device__ __forceinline__ void trsm_store_l(const DevView& V, const FrontMeta& M, const double* Lr, const int ibase, const int rlim);
template <int TS, int NT, bool PRE = false>
__device__ __forceinline__ void big_diag_body(const DevView& V, const FrontMeta& M, char* smem_raw, int* flag = nullptr, const int epoch = 0, unsigned long long* ts = nullptr,
                                              const double* late_Lr = nullptr, const FrontMeta& late_M = FrontMeta(), const int late_ibase = 0, const int late_rows = 0, int* pflag = nullptr)
{
    constexpr int G = (NT == 1024) ? 32 : 16, MAXM = G * TS;
    const int tid = threadIdx.x;
    const int s = M.s, c0 = M.c0, k = M.k;
    const int ld = k | 1;
    double* Lb     = reinterpret_cast<double*>(smem_raw);   // k x k L columns (physical rows); later the pivot-ordered block / its inverse
    double* colbuf = Lb + (size_t)ld * k;
    double* dinv_s = colbuf + 4 * MAXM; double* doff_s = dinv_s + k; double* cm0 = doff_s + k;
    int* ord = reinterpret_cast<int*>(cm0 + k); int* pt_s = ord + k;
    double* P = V.L + M.panel_off;
    const size_t ldp = (size_t)M.ldp;
    int nneg = 0, nzero = 0, ntwo = 0, nsmall = 0, chg = 0;
    DBGSTAMP(0);
#ifdef MI355X_PIVSTAT
    const bool dprobe = gridDim.x == 1 && gridDim.y > 1 && tid == 0 && NT == 256;
    if (dprobe) g_dt[1] = wall_clock64();
#endif
    if (V.dbg && blockIdx.x == 0 && blockIdx.y < 4 && tid == 0) { V.dbg[32 + 8 * blockIdx.y + 5] = wall_clock64(); }
    bool fast = false;
    if constexpr (NT == 256) {
        if (V.fastpiv && k <= 64) {
            // ---- fast path: blocked LDL^T in natural order, accepted a posteriori (ldlt_blocked_static) ----
            double* Wp = reinterpret_cast<double*>(pt_s + k + (k & 1));         // 64 x 16 (ld 65): W = L D of the panel in flight
            double* Isb = Wp + 16 * 65;                                          // 4 x 272: inverses of the 16 x 16 diagonal blocks of L11
            int* shflag = reinterpret_cast<int*>(Isb + 4 * 272);
            const int i = tid & 63, cq = tid >> 6;
            DBGT(0);
            if constexpr (!PRE) {   // the block (lower part in the panel storage) -> LDS, mirrored; a chain link's own A entries are added in LDS
                double pv[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) { const int c = cq + 4 * e; pv[e] = (i < k && c < k && i >= c) ? P[i + (size_t)c * ldp] : 0.0; }
                int apos_[2]; double aval_[2]; int na = 0;
                if (M.selfasm) {
#pragma unroll
                    for (int e = 0; e < 2; ++e) { const int q = M.aq0 + tid + e * NT; if (q < M.aq1) { apos_[e] = V.apos[q]; aval_[e] = V.aval[q]; na = e + 1; } }
                }
#pragma unroll
                for (int e = 0; e < 16; ++e) { const int c = cq + 4 * e; if (i < k && c < k && i >= c) { Lb[i + c * ld] = pv[e]; Lb[c + i * ld] = pv[e]; } }
                __syncthreads();
                if (M.selfasm) {
#pragma unroll
                    for (int e = 0; e < 2; ++e) if (e < na) { const int ii = apos_[e] % M.m, cc = apos_[e] / M.m; if (ii < k) { Lb[ii + cc * ld] += aval_[e]; if (ii != cc) Lb[cc + ii * ld] += aval_[e]; } }
                    for (int q = M.aq0 + tid + 2 * NT; q < M.aq1; q += NT) { const int pos = V.apos[q]; const int ii = pos % M.m, cc = pos / M.m; if (ii < k) { const double v = V.aval[q]; Lb[ii + cc * ld] += v; if (ii != cc) Lb[cc + ii * ld] += v; } }
                    __syncthreads();
                }
            }
            DBGT(1);
            if (ts) ts[8] = clock64();
            // zero-pivot scale: the largest column scale of the block (a pivot that clears it clears its own column's)
            double cmx;
            {
                const int c = tid >> 2, part = tid & 3;
                double mx = 0.0;
                if (c < k) for (int r = part; r < k; r += 4) mx = fmax(mx, fabs(PRE ? Lb[max(r, c) + min(r, c) * ld] : Lb[r + c * ld]));
                mx = fmax(mx, dpp_f64<0xB1>(mx)); mx = fmax(mx, dpp_f64<0x4E>(mx));
                if (c < k && part == 0) mx = fmax(mx, V.cnorm[c0 + c]); else if (c >= k) mx = 0.0;
                cmx = wave_max_all(mx);
                if ((tid & 63) == 0) colbuf[tid >> 6] = cmx;
                __syncthreads();
                cmx = fmax(fmax(colbuf[0], colbuf[1]), fmax(colbuf[2], colbuf[3]));
            }
            const double zmax = fmax(V.small, ZERO_REL * cmx);
            const double gmax = 1.0 / fmax(fmax(V.pivtol, V.pivtol2), V.fastu);
            DBGT(2);
            if (ts) ts[9] = clock64();
            if (pflag) {
                const PubHook H{P, ldp, V.dinv + c0, V.isg + (size_t)M.bigidx * ISG_STRIDE, pflag, 8 * epoch};
                fast = ldlt_blocked_static(Lb, ld, k, Wp, dinv_s, Isb, shflag, zmax, gmax, nneg, V.dbg, ts, &H);
                if (!fast && tid == 0) __hip_atomic_store(pflag, 8 * epoch + 7, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (rejected: nobody may wait for a sub-block that never comes; qstat[5] below)
            } else
            fast = ldlt_blocked_static(Lb, ld, k, Wp, dinv_s, Isb, shflag, zmax, gmax, nneg, V.dbg, ts);
            DBGT(3);
            if (ts) ts[10] = clock64();
            if (fast) {
                DBGSTAMP(1);
#pragma unroll
                // (fused launches -- `flag`: what the workgroups behind the flag read is stored agent-coherently, so that the flag needs no release fence: chain_signal_coh)
                for (int e = 0; e < 16; ++e) { const int c = cq + 4 * e; if (i < k && c < k) { const double v = (i > c) ? Lb[i + c * ld] : 0.0; if (flag) st_coh(&P[i + (size_t)c * ldp], v); else P[i + (size_t)c * ldp] = v; if (i <= c) Lb[i + c * ld] = 0.0; } }
                for (int j = tid; j < k; j += NT) { doff_s[j] = 0.0; pt_s[j] = 1; ord[j] = j; }
                {   // the diagonal-block inverses travel with L11: the panel solves need exactly these
                    double* Ig = V.isg + (size_t)M.bigidx * ISG_STRIDE;
                    const int nis = ((k + 15) >> 4) * 272;
                    if (flag) { for (int idx = tid; idx < nis; idx += NT) st_coh(&Ig[idx], Isb[idx]); }
                    else for (int idx = tid; idx < nis; idx += NT) Ig[idx] = Isb[idx];
                }
                if (tid == 0) atomicAdd(&V.qstat[3], 1);
                __syncthreads();
            } else if (tid == 0) { atomicAdd(&V.qstat[2], 1); if ((PRE || pflag) && V.norestore) V.qstat[5] = 1; }      // (no intact copy of the block for the strict loop below: factor() repeats the factorisation)
        }
    }
    if (!fast) {
    if (M.selfasm) {            // pure in-place chain link (no assembly launch): the A entries of the pivot rows are added here
        for (int q = M.aq0 + tid; q < M.aq1; q += NT) { const int pos = V.apos[q]; const int i = pos % M.m, c = pos / M.m; if (i < k) P[i + (size_t)c * ldp] += V.aval[q]; }
        __syncthreads();
    }
    const int ti = tid % G, tj = tid / G, row0 = ti * TS, col0 = tj * TS;
    double t[TS][TS];
#pragma unroll
    for (int x = 0; x < TS; ++x)
#pragma unroll
        for (int y = 0; y < TS; ++y) {
            const int i = row0 + x, c = col0 + y;
            t[x][y] = (i < k && c < k) ? ((i >= c) ? P[i + (size_t)c * ldp] : P[c + (size_t)i * ldp]) : 0.0;
        }
    nneg = 0;
    const double cmx = front_colmax<NT, TS>(t, cm0, k, V.cnorm + c0);
    ldlt_reg<NT, TS, (G * TS > 64)>(t, k, k, Lb, ld, colbuf, dinv_s, doff_s, pt_s, ord, V.pivtol, V.pivtol2, V.small, cm0, cmx, V.zpiv + c0, nneg, nzero, ntwo, nsmall, chg);
    if (chg && tid == 0) V.qstat[0] = 1;
    __syncthreads();
    DBGSTAMP(1);
#ifdef MI355X_PIVSTAT
    if (dprobe) g_dt[2] = wall_clock64();
#endif
    // pivot-ordered unit-lower block: the row permutation is done IN PLACE in LDS through registers (each thread owns
    // <= 16 entries: k*k <= 16*NT), the panel gets its copy on the way -- no second k x k buffer, no global round trip
    {
        double tmp[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) { const int idx = tid + e * NT; const int i = idx % k, c = idx / k; tmp[e] = (idx < k * k && i > c) ? Lb[ord[i] + c * ld] : 0.0; }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 16; ++e) { const int idx = tid + e * NT; const int i = idx % k, c = idx / k; if (idx < k * k) { Lb[i + c * ld] = tmp[e]; P[i + (size_t)c * ldp] = tmp[e]; } }
    }
    }
    if (flag && fast) {
        for (int j = tid; j < k; j += NT) { st_coh(&V.dinv[c0 + j], dinv_s[j]); st_coh(&V.doff[c0 + j], doff_s[j]); st_coh(&V.ptype[c0 + j], pt_s[j]); st_coh(&V.lperm[c0 + j], ord[j]); }
        // (the panel workgroups count their a-posteriori failures in V.apfail[s], a word of their own that the prologue zeroes: nothing orders
        //  their increment against this store -- they wait on the sub-block flags, which are raised before it)
        if (tid == 0) { int* fs = reinterpret_cast<int*>(&V.fstat[s]); st_coh(fs, nneg); st_coh(fs + 1, nzero); st_coh(fs + 2, ntwo); st_coh(fs + 3, nsmall); st_coh(&V.hasis[s], 1); }
    } else {
    for (int j = tid; j < k; j += NT) { V.dinv[c0 + j] = dinv_s[j]; V.doff[c0 + j] = doff_s[j]; V.ptype[c0 + j] = pt_s[j]; V.lperm[c0 + j] = ord[j]; }
    if (tid == 0) { V.fstat[s] = make_int4(nneg, nzero, ntwo, nsmall); V.hasis[s] = fast ? 1 : 0; }
    }
#ifdef MI355X_PIVSTAT
    if (flag && dprobe) g_dt[5] = wall_clock64();
#endif
    if (ts) ts[11] = clock64();
    if (flag) { if (fast) chain_signal_coh(flag, epoch); else chain_signal(flag, epoch); }        // fused launch: the panel workgroups need L11, D and the pivot order -- not the inverse below
    if (ts) ts[12] = clock64();
    if (late_Lr) trsm_store_l(V, late_M, late_Lr, late_ibase, late_rows);
    if (V.dbg && blockIdx.x == 0 && blockIdx.y < 4 && tid == 0) { V.dbg[32 + 8 * blockIdx.y + 6] = wall_clock64(); }
    __syncthreads();
    DBGSTAMP(2);
#ifdef MI355X_PIVSTAT
    if (dprobe) g_dt[3] = wall_clock64();
#endif
    invert_unit_lower<NT>(Lb, ld, k);
    DBGSTAMP(3);
#ifdef MI355X_PIVSTAT
    if (dprobe) g_dt[4] = wall_clock64();
#endif
    double* Mg = V.minv + M.minv_off;
    for (int idx = tid; idx < k * k; idx += NT) { const int i = idx % k, c = idx / k; Mg[idx] = (i > c) ? Lb[i + c * ld] : (i == c ? 1.0 : 0.0); }
    if (V.dbg && blockIdx.x == 0 && tid == 0) V.dbg[15] = (unsigned long long)k;
}

// (host side: bytes of big_diag_body's LDS layout; maxm = 64 for the 256-thread, 128 for the 1024-thread instantiation)
static size_t diag_lds_bytes(int kk, int maxm)
{
    return (size_t)((kk | 1) * kk + 4 * maxm + 3 * kk) * sizeof(double) + (size_t)(2 * kk + 2) * sizeof(int) + (size_t)(16 * 65 + 4 * 272) * sizeof(double) + 64;
}
template <int TS, int NT = 256>
__global__ __launch_bounds__(NT) void k_big_diag_reg(DevView V, int list_off)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const FrontMeta M = V.fmeta[list_off + blockIdx.x];
    big_diag_body<TS, NT>(V, M, smem_raw);
}

// ------------------------------------------------------------------------------------------------
// inertia / statistics reduction (fixed order => deterministic)
// ------------------------------------------------------------------------------------------------
__global__ void k_reduce_stats(const int4* fstat, const int* apfail, const int* owner, int nsn, int rank_filter, int* out)
{
    // integer sums: order-independent, so a grid of partial sums + atomicAdd stays deterministic
    __shared__ int sh[4][256];
    int a = 0, b = 0, c = 0, d = 0;
    for (int s = blockIdx.x * 256 + threadIdx.x; s < nsn; s += gridDim.x * 256) {
        if (rank_filter >= -1 && owner[s] != rank_filter) continue;
        const int4 v = fstat[s]; a += v.x; b += v.y; c += v.z; d += v.w + apfail[s];
    }
    sh[0][threadIdx.x] = a; sh[1][threadIdx.x] = b; sh[2][threadIdx.x] = c; sh[3][threadIdx.x] = d;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (threadIdx.x < off) for (int q = 0; q < 4; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x < 4 && sh[threadIdx.x][0] != 0) atomicAdd(&out[threadIdx.x], sh[threadIdx.x][0]);
}
__global__ void k_zero_i32(int* p, int n) { if (threadIdx.x < n) p[threadIdx.x] = 0; }
// start of a factorisation in one launch: per-column flags cleared, quality flags cleared, the epoch of the flag-synchronised
// launches advanced
__global__ void k_factor_prologue(DevView V)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < V.n; i += gridDim.x * blockDim.x) { V.colfail[i] = 0; V.zpiv[i] = 0; }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < V.nsn; i += gridDim.x * blockDim.x) { V.tcnt[i] = 0; V.apfail[i] = 0; }
    if (blockIdx.x == 0 && threadIdx.x < 8) V.qstat[threadIdx.x] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) V.sepoch[2] += 1;
}

