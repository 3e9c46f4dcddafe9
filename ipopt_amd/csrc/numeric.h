// numeric.h -- device-side numeric engine interface (implemented in numeric.hip).
// Host code (api.cpp) owns a Numeric object per solver handle.
#pragma once
#include "symbolic.h"
#include "qn_pair_host.h"      // QpSegs, QpState (host only)
#include <cstdint>
#include <string>
#include <vector>

namespace mi355x {

struct NumericOptions {
    int    device = -1;
    int    scaling = 1;
    double pivtol = 1e-8;
    double pivtolmax = 1e-4;   // the largest u IncreaseQuality can reach: the factorisation records whether any pivot decision would differ there
    double small = 1e-20;
    int    refine_steps = 0;
    int    use_graph = 1;
    int    rank = 0, nranks = 1;
    int    verbose = 0;
    void*  prewarmed_vals = nullptr;   // pinned staging buffer of prewarmed_count doubles made by Numeric::prewarm while the analysis ran (setup takes ownership)
    size_t prewarmed_count = 0;
};

// num_small = failed pivots (num_delay of MA97/SSIDS): eliminated although they failed the threshold test, because the static
// structure cannot delay them to the parent front; u_sensitive != 0: some pivot decision would differ at u = pivtolmax
// num_fast = pivot blocks of big fronts accepted on the blocked a-posteriori path (the others took the strict loop)
struct FactorStats { int num_neg = 0, num_zero = 0, num_two = 0, num_small = 0, u_sensitive = 1, num_fast = 0; };

// the two requests of a limited-memory quasi-Newton history (Numeric::lbfgs_define, lbfgs_push)
struct LbDefine {
    int rows, max_history, type;                      // type 0 BFGS / 1 SR1
    int init; double init_val, smin, smax;            // the rule of the first sigma and its bounds
    const double* dr = nullptr;                       // host, `rows` positive entries: a restoration-phase history (B0 = sigma I, or eta DR when special)
    int special = 0;
};
constexpr double LB_SR1_SIGMA_MIN = 1e-8, LB_SR1_SIGMA_MAX = 1e8;      // smin, smax of a plain SR1 history (its C entry point takes none)
struct LbPush {
    const double *s, *y;                              // host or device vectors; y is ypart when resto
    long long len = 0;                                // 0: vectors of the history's `rows`; > idx[rows-1]: x-block vectors of len entries, gathered through the row map (:323-324)
    bool device = false, resto = false;
    double eta = 0.0;                                 // a resto push only (> 0)
};

class NumericImpl;

class Numeric {
public:
    Numeric();
    ~Numeric();
    // false + error() on failure (e.g. no HIP device: there is NO CPU fallback)
    bool   setup(const Symbolic& S, const NumericOptions& opt);
    double* values_buffer();                         // pinned host buffer, nnz_in doubles
    bool   factor(const double* dvals_or_null, bool reuse_device_values, FactorStats& st);
    bool   solve_host(int nrhs, double* rhs, int ld);
    bool   solve_device(int nrhs, double* drhs, int ld);
    bool   solve_device2(int nrhs, const double* db, int ldb, double* dx, int ldx);   // out of place
    void   set_pivtol(double u);
    void   set_pivtolmax(double u);
    double last_factor_ms() const;
    void   matching_stats(double* ms, int* rounds, int* unmatched) const;      // the last matching-scaling computation (scaling modes 3-6)
    double last_solve_ms() const;
    // opt-in blocked solve of a single-GPU handle (launch_plan.h SolveBlockKind): nrhs >= 2 right-hand sides go through the tree SOLVE_RB at a time;
    // last_solve_block_ms: the time of the last solve call that took that path (0: none)
    void   set_solve_block(bool on);
    double last_solve_block_ms() const;
    double last_solve_block_top_ms() const;          // of that call: the part spent in the top part of its blocks (events around it)
    bool   solve_block_plan(int* first_top_level, int* blocked, int* bycol, int* top) const;      // the schedule the engine runs (false: not set up, or multi-rank)
    const std::string& error() const;
    static constexpr int kNumKernelKinds = 18;
    bool   profile(int reps, double* ms, int* launches);
    bool   debug_pivots(double* dinv, double* doff, int* ptype, int* lperm);      // development aid: pivot data of the last factorisation, n entries each
    bool   debug_clocks(unsigned long long* out128);        // development aid (MI355X_KKT_TRACE=clocks)   // per-kernel-kind device time (hip events), eager launches
    // multi-GPU pieces
    bool   factor_local(const double* dvals_or_null);
    bool   top_arena(double** dptr, int64_t* ndoubles);
    bool   factor_top(FactorStats& st);
    bool   solve_fwd_local(double* drhs);
    bool   top_rhs(double** dptr, int64_t* ndoubles);
    bool   solve_top_and_bwd(double* drhs);
    bool   set_scaling(int mode, const double* user_factors_orig_numbering);   // 0 none, 1 Ruiz (device), 2 the caller's factors, 3 matching (host, every factorisation), 4 matching (host, computed once, reused), 5 / 6 the same on the device
    bool   get_scaling(double* out_orig_numbering);                             // factors of the last factorisation
    void   invalidate_matching();                                                // scaling mode 4: compute the matching scaling afresh at the next factorisation
    // first touch of the device (context, code objects) and the pinned staging buffer: independent of the analysis, so the C API runs it on a
    // thread next to it (0.1-0.3 s of an Ipopt run's LinearSystemSymbolicFactorization otherwise).  Returns the buffer or nullptr.
    static int   resolve_device(int device);              // on the caller's thread: the ordinal `device` (or the current device for -1) means, -1 without a device
    static void* prewarm(int device, size_t count);
    static void prewarm_discard(void* p);
    static bool ruiz_triplet(int device, int n, int nnz, const int* irn, const int* jcn, const double* a, int base, int sweeps, double* out, std::string& err);
    bool   zero_pivots(std::vector<int>& idx0);           // columns (original numbering, 0-based) with a zero pivot in the last factorisation
    // delayed pivoting across fronts: the columns (CURRENT permuted numbering) the last factorisation could not pivot, and the re-setup of
    // everything that depends on the elimination structure once symbolic.cpp has moved them to their parent fronts (values, assembly and
    // primal-dual state, scaling factors, communicator and the pinned buffers handed to the caller survive)
    bool   failed_pivots(std::vector<int>& cols_perm);
    bool   restructure(const Symbolic& S);
    // device-side value assembly: triplet values = concatenated segments, each  scale * src + shift  from a device-resident source
    bool   assembly_define(int nseg, const int64_t* off, const int64_t* len);
    double* assembly_buffer(int seg);                      // pinned staging of the segment's source values
    bool   assembly_upload(int seg);                       // async H2D on the solver's stream
    bool   factor_assembled(const double* scale, const double* shift, FactorStats& st);
    // the 8-block primal-dual system on the device: vectors are {x, s, y_c, y_d, z_L, z_U, v_L, v_U} concatenated
    bool   pd_define(const int* dims8, const int* ixl, const int* ixu, const int* isl, const int* isu, const int* irn, const int* jcn, const int* segs, int nsegs);
    bool   pd_put_data(const double* const* arr8);
    bool   pd_put(int vec, const double* const* blocks8);
    bool   pd_get(int vec, double* const* blocks8);
    bool   pd_solve_once(int rhs, int res, double alpha, double beta);
    bool   pd_residual(int rhs, int res, int resid, const double* deltas4, double* norms3);
    // low-rank update K + V V^T - U U^T of the factored system (IpLowRankAugSystemSolver.cpp): V (rows x nv), U (rows x nu), host, column-major, on the
    // first `rows` indices of the caller's numbering (or, with a row map, on the indices it names); kept on the device across refactorisations and structure edits.  lowrank_update runs after a
    // factorisation (*which: 0 in force, 1 / 2 = M1 / M2 not positive definite); the solves refuse an update that is not current (factor_count).
    // While one is set, pd_solve_once corrects the 4-block solution and pd_residual adds V (V^T res_x) - U (U^T res_x) to the x rows.
    bool   lowrank_set(int rows, int nv, const double* V, int ldv, int nu, const double* U, int ldu);
    bool   lowrank_update(int* which);
    bool   lowrank_solve_host(int nrhs, double* rhs, int ld);
    bool   lowrank_solve_device2(int nrhs, const double* db, int ldb, double* dx, int ldx);
    bool   lowrank_clear();
    void   lowrank_info(int* rows, int* nv, int* nu, int* current, double* update_ms) const;
    // the row map (P_LowRank, ExpansionMatrix::ExpandedPosIndices): row i of V, U, S, Y, DR is the caller's index idx[i] (0-based, strictly ascending, < n;
    // lowrank_host.h lr_rowmap_check).  rows = 0 / idx = nullptr removes it.  Refused while an update is set or a history defined; while it is set every
    // lowrank_set / lbfgs_define* takes its `rows`.  _info: rows (0: none) and the largest index (-1: none), host state, answers without a device.
    bool   lowrank_rowmap(int rows, const int32_t* idx);
    void   lowrank_rowmap_info(int* rows, long long* last) const;
    void   lowrank_rowmap_copy(int32_t* idx) const;          // `rows` entries (the caller checks the capacity)
    // limited-memory BFGS (IpLimMemQuasiNewtonUpdater.cpp, BFGS "with skipping"): the (s, y) history of `rows` entries per vector stays on the device;
    // a push (host or device vectors) answers *outcome = 0 stored, V and U formed on the device and installed as the low-rank update above (not current),
    // 1 skipped, 2 stored but M not positive definite: the installed columns stay.  lbfgs_get what: 0 S, 1 Y, 2 V, 3 U, 4 D, 5 L, 6 S^T S.
    bool   lbfgs_define(const LbDefine& d);
    bool   lbfgs_push(const LbPush& p, int* outcome);
    bool   lbfgs_reset();
    bool   lbfgs_clear();
    void   lbfgs_info(int* rows, int* max_history, int* memory, double* sigma, int* skipped_in_a_row, double* push_ms) const;
    bool   lbfgs_get(int what, double* out, long long capacity);
    // limited-memory SR1 (the same file, case SR1): a history defined here answers a push with 0 or 1 only (V: memory - nneg columns, U: nneg, from
    // the eigen-split of Z = D + L + L^T - sigma S^T S) and can take its last stored push back once (lbfgs_undo; a BFGS history refuses).
    // lbfgs_sr1_info: E receives the `memory` eigenvalues of the installed split, ascending (the caller checks the capacity).
    bool   lbfgs_undo(int* undone);
    void   lbfgs_sr1_info(int* type, int* nneg, int* can_undo, double* E) const;
    // a restoration-phase history (LbDefine::dr; lbfgs_host.h "the restoration phase") takes resto pushes only (LbPush::resto; a plain push is refused,
    // and the other way round); every other lbfgs_* call serves it unchanged.  lbfgs_get what: 1 is Ypart; 10 G, 11 R, 12 eta_col, 13 dv, 14 DR.
    void   lbfgs_resto_info(int* resto, int* special, double* eta) const;
    // the quasi-Newton pair (s, y) formed from the resident Jacobians (IpLimMemQuasiNewtonUpdater.cpp:276-308; qn_pair_host.h): a column view of [J_c; J_d] over two
    // segments of the value assembly (g: their ranges, validated by qp_check before the call), a snapshot of x, grad_f and the segments' sources (store), one
    // kernel pass for s = x - x_last, y = (grad_f - gf_last) + sum (J_cur - J_last) lam (form), and the push of the formed device vectors through lbfgs_push.
    // assembly_info: number of assembly segments and the range of `seg`; qn_pair_state / qn_pair_plan: host state, answer without a device.
    int    assembly_info(int seg, long long* off, long long* len) const;
    bool   qn_pair_define(const int32_t* dims4, const int32_t* irn, const int32_t* jcn, int seg_jc, int seg_jd, const QpSegs& g);
    bool   qn_pair_store(const double* x, const double* grad_f, bool device);      // x == nullptr: roll
    bool   qn_pair_form(const double* x, const double* grad_f, const double* y_c, const double* y_d, bool device, double* amax_s);
    bool   qn_pair_push(double eta, int* outcome);
    bool   qn_pair_get(int what, double* out, long long capacity);
    void   qn_pair_info(int* defined, int* stored, int* formed, int* nx, int64_t* nnz_j, double* form_ms) const;
    void   qn_pair_plan(int* out6) const;                // {defined, lanes per column, longest column, nx, entries low, high}
    const QpState& qn_pair_state() const;
    bool   qn_pair_clear();
    long long factor_count() const;                  // bumped by every factorisation (the refactorisations of a delayed-pivot loop included) and every structure edit
    // communicator of a multi-GPU handle: with one set, factor()/solve_*() run the whole distributed sequence themselves
    bool   set_comm_rccl(const void* unique_id128);                                   // RCCL (dlopen'ed), ncclCommInitRank(nranks, id, rank)
    bool   set_comm_callback(int (*allreduce)(void* ctx, void* dptr, int64_t count, int dtype, void* hip_stream), void* ctx);
    // optional, for a callback communicator: in-place sum over the ranks [rank_lo, rank_lo + nranks_in_range) only (this rank is one of them);
    // with it a range of ranks sums its part of an exchange step among itself instead of the whole machine summing everything
    bool   set_comm_range_callback(int (*allreduce_range)(void* ctx, void* dptr, int64_t count, int dtype, void* hip_stream, int rank_lo, int nranks_in_range));
    long long exchange_bytes(int what) const;        // bytes of the arena squares (0) / top right-hand sides (1) of all exchange steps
    // host only (no device): the collectives rank `rank` of `nranks` issues for one factorisation + one solve of the structure S, and the ncclCommSplit calls
    // before them -- records of 6 ints, see comm_plan in launch_plan.cpp.  What a CPU test walks to show that every rank issues matching sequences.
    static void comm_plan(const Symbolic& S, int nranks, int rank, bool range_local, std::vector<int>& out6);
    // the communicator in use: kind 0 none / 1 callbacks / 2 RCCL; ranks the communicator itself reports (ncclCommCount; nranks for callbacks); range-local collectives on
    void comm_info(int* kind, int* ranks_seen, int* range_local, int* exchange_steps) const;
    static bool rccl_unique_id(void* out128, std::string& err);                       // ncclGetUniqueId (rank 0 creates, the launcher distributes)
private:
    NumericImpl* p_;
};

} // namespace mi355x
