// device_view.hip.inc -- part of numeric.hip (one translation unit; included there, inside namespace mi355x): device-side view of the symbolic structure + numeric storage, small device helpers (DPP reductions, coherent loads / stores).
// ------------------------------------------------------------------------------------------------
// device-side view of the symbolic structure + numeric storage (passed by value to kernels)
// ------------------------------------------------------------------------------------------------
// the records of the launch tables (FrontMeta, ChildMeta, GroupLink, LeafLink, ChainLink, ChainDesc, DfLevel): kernel_tables.h
constexpr int FLAG_STRIDE = 32;      // ints between two flags of the sweeps: one 128-byte line each (hundreds of workgroups poll them; side by side they would all queue at one L2 channel)

typedef double v2d __attribute__((ext_vector_type(2)));      // {value, tag}: the 16-byte messages of the solve sweeps
struct DevView {
    // symbolic
    const int* sn_colptr; const int* sn_rowptr; const int* sn_rows; const int* rel;
    const int* child_ptr; const int* child_idx; const int* sn_owner; const int* sn_parent; const int* col_owner;
    const long long* panel_off; const long long* cb_off; const long long* minv_off;
    const int* acolptr; const int* apos; const int* arow; const int* acol;
    const int* dup_ptr; const int* dup_src;
    const int* rslot_ptr; const int* rslot_idx; const int* rslot_col; int rslot_len;
    const int* level_sn;
    const FrontMeta* fmeta;   // parallel to level_sn
    const int* relinv;        // per child of a BIG parent: parent front row -> index in the child's update rows, or -1 (ChildMeta::inv)
    const GroupLink* gtab;    // links of the chain groups (FrontMeta::gbase .. gbase + gpos)
    const int* tile_tab;      // XCD-aware tile orders of the large trailing updates ((ti << 16) | tc), see k_big_schur
    const ChildMeta* cmeta;   // parallel to child_idx
    const int* perm;
    // numeric
    const double* tvals;    // triplet values (device copy)
    double* aval;           // summed + scaled values, permuted lower CSC order
    double* scale;          // symmetric scaling, permuted numbering
    double* scale2;         // second buffer (Jacobi-style equilibration sweeps)
    double* arv;            // |values| in symmetric row-view order (equilibration sweeps stream it)
    unsigned long long* rowmax;  // scratch for equilibration (bit pattern of non-negative doubles)
    double* L;              // panels
    double* cb;             // contribution blocks
    double* wbuf;           // W = L*D copies of the big fronts of the level in flight
    double* minv;           // k x k inverses of the unit-lower pivot blocks (column-major, ld = k)
    double* dinv; double* doff; int* ptype; int* lperm;
    int4*   fstat;          // per front {neg, zero, two, small}
    double* xw;             // work vector (permuted, scaled)
    double* cvec;           // forward-solve contributions, aligned with sn_rows
    double* bw; double* xacc;   // iterative refinement: scaled right-hand side and accumulated solution (permuted numbering)
    double* gpart;          // partial sums of the backward dot products of the chain groups
    double* zb;             // z = D^{-1} y of the forward sweep (pivot order); xw keeps b until the backward sweep writes x
    double* ybuf;           // y of the pivot rows (big fronts: the update rows are handled by a second, multi-workgroup launch)
    // multi-GPU top arena (full m x m squares per replicated front), null on 1 GPU
    double* arena; const long long* arena_off;
    double* top_rhs; const long long* top_rhs_off;
    // parameters
    double pivtol, pivtol2, small;   // u, the largest u IncreaseQuality may reach (decision-change tracking), absolute zero threshold
    int* colfail;           // per column of a BIG front: 1 once some multiplier of L21 exceeded 1/u (a posteriori test, k_big_trsm)
    int* qstat;             // [0]: some pivot decision of this factorisation would differ at u = pivtol2
    double* cnorm;          // inf-norm of every column of the (scaled) INPUT matrix, permuted numbering: scale of the zero-pivot test
    const ChainLink* chlink; const ChainDesc* chdesc;     // chain solve tables
    int strace_b;                    // (first backward workgroup's slot)
    unsigned long long* strace;      // development aid (MI355X_KKT_TRACE=solve=file): 4 wall-clock stamps per workgroup of the data-flow sweeps
    const int* chwg_f; const int* chwg_b; const int* chwait; int* sflag_t; int* sflag_dot; double* dpart; v2d* ytag; v2d* xtag;     // workgroup -> chain (forward / backward launch), wait lists, tail / gather flags
    int xcd_affine;                                             // levels of many big fronts: a front's workgroups on ONE XCD (k_big_schur64, k_big_trsm; MI355X_KKT_DISABLE=xcd_affine)
    int* apfail;                                                // per front: columns whose a-posteriori multiplier test failed in a panel workgroup (zeroed by the prologue; its own word, so that no store of fstat can wipe an increment)
    int* tcnt;                                                  // per front: panel-solve workgroups finished (fused pivot block + panel solve + narrow update launch), zeroed by the prologue
    double* isg; int* hasis;      // per big front: the four 16 x 16 diagonal-block inverses of L11 left by the blocked factorisation (hasis: valid), for the panel solves
    const int* lc_ptr; const LeafLink* lc_link;      // leaf chains (k_leaf_chain, k_fwd_leafchain, k_bwd_leafchain): lc_link[lc_ptr[c] .. lc_ptr[c + 1]) = chain c's fronts, the leaf first
    int* sflag_s;           // [4 * link + q]: rows of the group's link q have stored their W / L against this link (k_grp_fused)
    v2d* cbt; const long long* cbt_off;      // k_front_df: tagged contribution blocks {value, epoch} of the fronts whose parent is handled by the same launch ([front]: offset of its 16 x 16 (32 x 32) square, or -1)
    int* sflag_p;           // [link]: 8 * epoch + (16-column sub-blocks of the link's pivot block whose results are published) -- k_grp_fused in the optimistic schedule:
                            // the panel solves run IN STEP with the blocked factorisation of the pivot block (trsm_rows_pipe)
    int* sflag_b; int* sflag_d; int* sepoch;     // (sflag_d / sepoch[2]: pivot block done, fused pivot-block + panel-solve launch)              // per-supernode 'done' flags of the chain sweeps (value = epoch of the solve)
    int* zpiv;              // per column (permuted numbering): 1 if its pivot was a zero pivot (DetermineDependentRows)
    int n, nnz_a, nsn, rank;
    int fastpiv;            // pivot blocks of the big fronts: blocked LDL^T accepted a posteriori first, the strict loop as fall-back (ldlt_blocked_static)
    double fastu;           // ... accepted iff every multiplier <= 1 / max(u, u2, fastu)
    int asm_pull;           // k_big_assemble: entries summed through the inverse row maps and written once (default) / scatter-added child by child
    int norestore;          // optimistic schedule: a pivot block's blocked LDL^T works without a safety copy of its input (k_grp_fused: no copy of the updated block to
                            // the panel storage in front of it; results published while later sub-blocks are still being factored) -- a block the a-posteriori test then
                            // REJECTS cannot be handed to the strict loop intact: it raises qstat[5] and factor() repeats the factorisation with norestore = 0
    unsigned long long* dbg;   // optional phase time stamps of block 0 (development aid), may be null
};

// ------------------------------------------------------------------------------------------------
// small helpers
// ------------------------------------------------------------------------------------------------
// ---- wavefront reductions on the DPP path (row-local butterflies, then 4 readlanes): ~10x lower latency than the
// ds_bpermute shuffles on the serial pivot chain.  Results are wave-uniform. ----
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x)
{
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_f64(double x, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}
__device__ __forceinline__ double wave_max_all(double x)
{
    x = fmax(x, dpp_f64<0xB1>(x));    // quad_perm [1,0,3,2]
    x = fmax(x, dpp_f64<0x4E>(x));    // quad_perm [2,3,0,1]
    x = fmax(x, dpp_f64<0x141>(x));   // row_half_mirror
    x = fmax(x, dpp_f64<0x140>(x));   // row_mirror  -> every lane of a 16-lane row holds the row maximum
    return fmax(fmax(readlane_f64(x, 0), readlane_f64(x, 16)), fmax(readlane_f64(x, 32), readlane_f64(x, 48)));
}
__device__ __forceinline__ unsigned long long wave_or_all(unsigned long long v)
{
    int lo = (int)(v & 0xffffffffull), hi = (int)(v >> 32);
    lo |= __builtin_amdgcn_update_dpp(lo, lo, 0xB1, 0xF, 0xF, false);  hi |= __builtin_amdgcn_update_dpp(hi, hi, 0xB1, 0xF, 0xF, false);
    lo |= __builtin_amdgcn_update_dpp(lo, lo, 0x4E, 0xF, 0xF, false);  hi |= __builtin_amdgcn_update_dpp(hi, hi, 0x4E, 0xF, 0xF, false);
    lo |= __builtin_amdgcn_update_dpp(lo, lo, 0x141, 0xF, 0xF, false); hi |= __builtin_amdgcn_update_dpp(hi, hi, 0x141, 0xF, 0xF, false);
    lo |= __builtin_amdgcn_update_dpp(lo, lo, 0x140, 0xF, 0xF, false); hi |= __builtin_amdgcn_update_dpp(hi, hi, 0x140, 0xF, 0xF, false);
    const unsigned int l = (unsigned)(__builtin_amdgcn_readlane(lo, 0) | __builtin_amdgcn_readlane(lo, 16) | __builtin_amdgcn_readlane(lo, 32) | __builtin_amdgcn_readlane(lo, 48));
    const unsigned int h = (unsigned)(__builtin_amdgcn_readlane(hi, 0) | __builtin_amdgcn_readlane(hi, 16) | __builtin_amdgcn_readlane(hi, 32) | __builtin_amdgcn_readlane(hi, 48));
    return ((unsigned long long)h << 32) | l;
}
// sum over the 64 lanes on the DPP path (row-local butterflies + 4 readlanes), wave-uniform result
__device__ __forceinline__ double wave_sum_dpp(double x)
{
    x += dpp_f64<0xB1>(x);
    x += dpp_f64<0x4E>(x);
    x += dpp_f64<0x141>(x);
    x += dpp_f64<0x140>(x);
    return (readlane_f64(x, 0) + readlane_f64(x, 16)) + (readlane_f64(x, 32) + readlane_f64(x, 48));
}
__device__ __forceinline__ double wave_sum(double x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

