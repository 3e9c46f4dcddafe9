/*
 * mi355x_kkt.h -- C ABI of the MI355X-native sparse symmetric-indefinite KKT solver
 * (supernodal multifrontal LDL^T + triangular solves, hand-written HIP for gfx950).
 *
 * This is the drop-in boundary for Ipopt's linear-solver plug-in point.  Every entry
 * point replaces one step of the reference's third-party-solver adapters:
 *
 *   mi355x_kkt_create / _destroy   <->  adapter ctor/dtor, e.g. Ma97SolverInterface
 *                                       (reference src/Algorithm/LinearSolvers/IpMa97SolverInterface.cpp:277-301)
 *   mi355x_kkt_analyse             <->  SparseSymLinearSolverInterface::InitializeStructure
 *                                       (IpSparseSymLinearSolverInterface.hpp:139) -> ma97_analyse (IpMa97SolverInterface.cpp:567,674),
 *                                       MUMPS job=1 (IpMumpsSolverInterface.cpp:385-446)
 *   mi355x_kkt_values_buffer       <->  GetValuesArrayPtr (IpSparseSymLinearSolverInterface.hpp:155)
 *   mi355x_kkt_factor              <->  the "new_matrix" half of MultiSolve (hpp:190): ma97_factor (IpMa97SolverInterface.cpp:707),
 *                                       MUMPS job=2 (IpMumpsSolverInterface.cpp:448-541); returns inertia like INFOG(12)/info.num_neg
 *   mi355x_kkt_solve               <->  the back-solve half of MultiSolve: ma97_solve (IpMa97SolverInterface.cpp:790,805),
 *                                       MUMPS job=3 (IpMumpsSolverInterface.cpp:543-583)
 *   mi355x_kkt_increase_quality    <->  IncreaseQuality (hpp:220; u <- u^0.75, IpMa97SolverInterface.cpp:822-854)
 *   mi355x_kkt_set_pivtol          <->  the ma97_u / ma27_pivtol option (IpMa97SolverInterface.cpp:93-106)
 *   mi355x_kkt_get_info            <->  struct ma97_info (hsl_ma97d.h:96-121) / MUMPS INFOG
 *
 * Conventions: plain pointers and sizes only, no C++ types, no exceptions cross this
 * boundary, no global mutable state (re-entrant per handle).  Return value of every
 * int function is a MI355X_KKT_* status that mirrors Ipopt's ESymSolverStatus
 * (IpSymLinearSolver.hpp:19-33): 0 success, 1 singular, 2 wrong inertia (never produced
 * here: the caller compares num_neg), 4 fatal.  All floating point is fp64, all
 * indices int32 (Ipopt's Index), 64-bit counters where nnz(L)/flops can overflow.
 *
 * There is NO CPU fallback: factor/solve fail with MI355X_KKT_FATAL (and a message in
 * mi355x_kkt_last_error) when no gfx950 device is usable.  Only _analyse (symbolic,
 * host C++) and the query functions work without a GPU.
 */
#ifndef MI355X_KKT_H
#define MI355X_KKT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355X_KKT_SUCCESS        0
#define MI355X_KKT_SINGULAR       1
#define MI355X_KKT_WRONG_INERTIA  2
#define MI355X_KKT_CALL_AGAIN     3
#define MI355X_KKT_FATAL          4

/* input formats, cf. EMatrixFormat (IpSparseSymLinearSolverInterface.hpp:102-114) */
#define MI355X_KKT_FMT_TRIPLET    0   /* (row[k],col[k]) k<nnz; either triangle; duplicates are summed */
#define MI355X_KKT_FMT_CSR_UPPER  1   /* row = ia[n+1], col = ja[nnz]; upper-triangular CSR == lower CSC */

typedef struct mi355x_kkt_handle_s* mi355x_kkt_handle;

typedef struct mi355x_kkt_options {
    int    device;          /* HIP device ordinal; -1 = current device                                  */
    int    index_base;      /* 1 (Ipopt/Fortran numbering, default) or 0                                */
    int    ordering;        /* 0 = nested dissection + minimum-degree leaves (default), 1 = MD only,    */
                            /* 2 = natural (identity)                                                   */
    int    matching;        /* 1 (default) = pre-pair zero-diagonal rows with a partner column so that  */
                            /* the pair is one 2x2-capable supernode; 0 = off                           */
    int    scaling;         /* 0 none, 1 (default) = symmetric Ruiz inf-norm equilibration on device,   */
                            /* 3 = maximum-product matching scaling (MC64-style; host, per factorisation), */
                            /* 4 = the same computed at the first factorisation and REUSED until          */
                            /*     IncreaseQuality asks for better (MA97's "...-reuse" switches)          */
                            /* 5 = maximum-product matching scaling ON THE DEVICE (Jacobi auction,        */
                            /*     kernels_match.hip.inc), per factorisation; 6 = the same, reused like 4 */
    int    nd_leaf;         /* ND stops splitting below this many (compressed) nodes; default 32        */
    int    nemin;           /* relaxed-supernode amalgamation: always merge below this #cols; default 8 */
    int    max_sn_cols;     /* cap on columns of an amalgamated supernode; default (and max) 64                */
    double pivtol;          /* relative pivot threshold u (default 1e-8, cf. ma97_u)                    */
    double pivtolmax;       /* upper bound for set_pivtol escalation (default 1e-4)                     */
    double small;           /* |pivot| below this (after scaling) counts as zero (default 1e-20)        */
    int    refine_steps;    /* internal iterative-refinement steps per solve, fp64 residual on device    */
                            /* (default 0: Ipopt runs its own loop, IpPDFullSpaceSolver.cpp:256-346)     */
    int    use_graph;       /* 1 (default) = replay factor/solve launch sequences as hipGraphs          */
    int    nranks;          /* multi-GPU: number of ranks sharing one matrix (default 1)                */
    int    rank;            /* multi-GPU: this rank                                                     */
    int    verbose;         /* 0 silent                                                                 */
    int    leaf_cols;       /* whole elimination subtrees of <= this many columns become one supernode  */
                            /* (default 0 = off; measured: not a win)                                               */
    int    tree_merge;      /* tree amalgamation of small non-contiguous supernodes: 1 on, 0 off,        */
                            /* -1 = on when n <= 400 000.  Default 0: measured NOT to pay    */
    int    wide_panels;     /* 1: 128-column panels on separator fronts of order >= 512 (default 0)      */
    int    chain_group;     /* links of an in-place separator chain per update/solve unit, 1..4 (default 4) */
    int    solve_group;     /* 1: triangular solves per chain group instead of per link (default 0)       */
    int    subcube;         /* multi-GPU: 1 = subtree-to-subcube mapping -- a front of the top of the tree is replicated only */
                            /* on the ranks whose subtrees lie beneath it; 0 (default) = one top replicated on all ranks      */
    int    delay_rounds;    /* delayed pivoting across fronts: columns that fail the threshold test in their front are moved to the */
                            /* parent front's supernode and the matrix is refactored, at most this many times per factor() call   */
                            /* (default 8; 0 = static pivoting: failed pivots are forced and counted in num_small)                */
    int    smart_quality;   /* IncreaseQuality: 0 (default) = raise u whenever it is below pivtolmax, as the reference adapters do     */
                            /* (IpMa97SolverInterface.cpp:822-854); 1 = answer "cannot improve" at once when the last factorisation  */
                            /* recorded that no pivot decision depends on u up to pivtolmax (skips an identical refactorisation)      */
} mi355x_kkt_options;

typedef struct mi355x_kkt_info {
    int     n;
    int     nnz_in;          /* entries handed to analyse                                               */
    int     nnz_a;           /* distinct entries of one triangle (incl. diagonal)                       */
    int64_t nnz_l;           /* entries in L incl. diagonal (sum over supernodes of trapezoid)          */
    int64_t flops_factor;    /* sum_j (c_j-1)(c_j+2), c_j = column count of L             */
    int64_t flops_solve;     /* 4 nnz(L) - 3 n per right-hand side                                      */
    int64_t bytes_factor;    /* 12 nnz(A) + 8 nnz(L) + 4 sum(rows of supernodes)                        */
    int64_t bytes_solve;     /* 2 (8 nnz(L) + 4 sum rows) + 24 n per right-hand side                    */
    int64_t sum_sn_rows;     /* sum over supernodes of front order                                      */
    int64_t cb_doubles;      /* doubles in the contribution-block arena                                 */
    int     num_sn;          /* supernodes                                                              */
    int     num_levels;      /* height of the assembly tree (launch waves per factorisation)            */
    int     maxfront;        /* largest front order                                                     */
    int     maxsupernode;    /* largest number of columns in a supernode                                */
    int     num_pairs;       /* 2x2 pre-pairs from the matching                                         */
    int     num_neg;         /* negative eigenvalues of the last factorisation                          */
    int     num_zero;        /* zero pivots (=> singular) of the last factorisation                     */
    int     num_two;         /* 2x2 pivots of the last factorisation                                    */
    int     num_small;       /* pivots of the last factorisation that FAILED the threshold tests with u */
                             /* and were eliminated anyway (static pivoting): what the delayed-pivot    */
                             /* rounds could not move (root fronts, round / growth limits, or           */
                             /* delay_rounds = 0).  0 = every pivot passed the threshold test           */
    int     num_big_fronts;  /* fronts handled by the blocked (global-memory, MFMA) path                */
    double  time_analyse;    /* host seconds, last analyse                                              */
    double  time_factor_ms;  /* device ms (hip events on the solver's stream), last factor              */
    double  time_solve_ms;   /* device ms, last solve                                                   */
    double  pivtol;          /* the u the next factorisation will use                                   */
    int     u_sensitive;     /* last factorisation: 1 if some pivot decision would differ at u=pivtolmax */
    int     num_fast_blocks; /* last factorisation: pivot blocks of big fronts accepted on the blocked a-posteriori path  */
                             /* (natural order, every multiplier <= 1/max(u, pivtolmax, 1e-4)); the other big fronts'    */
                             /* pivot blocks took the strict threshold-pivoting loop                                     */
    int     num_delayed;     /* columns moved to a parent front since analyse() because they failed the threshold tests in their own (a column */
                             /* that moved up twice counts twice): info.num_delay of MA97 (hsl_ma97d.h:103, IpMa97SolverInterface.cpp:719-779) */
    int     num_restructures;/* structure edits (+ refactorisations) those delays have cost since analyse()                                  */
    double  matching_ms;     /* scaling modes 5 / 6: device time of the last matching-scaling computation (hip events)                                */
    int     matching_rounds; /* ... its auction rounds (all phases)                                                                                    */
    int     matching_unmatched; /* ... columns left without a row when it ended (modes 3 / 4: structural deficiency found by the host algorithm)       */
    double  reserved[3];
} mi355x_kkt_info;

/* fill opts with the defaults documented above */
void mi355x_kkt_default_options(mi355x_kkt_options* opts);

/* create a solver instance; opts may be NULL (defaults) */
int  mi355x_kkt_create(mi355x_kkt_handle* h, const mi355x_kkt_options* opts);
void mi355x_kkt_destroy(mi355x_kkt_handle h);

/* Symbolic analysis, once per sparsity structure.  `vals` (nnz doubles in the same order as
 * row/col, or NULL) is used only to detect zero diagonals for the 2x2 pre-pairing; the
 * Ipopt adapter therefore analyses lazily at the first MultiSolve, as the reference's
 * MUMPS adapter does (IpMumpsSolverInterface.cpp:349-383).  row/col are copied. */
int  mi355x_kkt_analyse(mi355x_kkt_handle h, int n, int nnz, const int* row, const int* col,
                        int format, const double* vals);

/* Pinned host staging buffer of nnz doubles the caller fills before every factor()
 * (GetValuesArrayPtr contract, IpSparseSymLinearSolverInterface.hpp:155). */
double* mi355x_kkt_values_buffer(mi355x_kkt_handle h);

/* Numeric factorisation of the values currently in values_buffer (or, if dvals != NULL, of
 * nnz doubles already resident in device memory).  Outputs may be NULL. */
int  mi355x_kkt_factor(mi355x_kkt_handle h, const double* dvals, int* num_neg, int* num_zero);

/* Re-factor the device-resident copy of the last values (after set_pivtol); cf. MA97/SPRAL
 * adapters that refactor from their private val_ copy (IpMa97SolverInterface.cpp:623). */
int  mi355x_kkt_refactor(mi355x_kkt_handle h, int* num_neg, int* num_zero);

/* ---- device-side value assembly: the next row of the hot path --------------------------------------
 * Replaces, for a host that keeps the pieces of the KKT matrix apart (Ipopt's AugSystemSolver contract,
 * IpAugSystemSolver.hpp:40-120), TripletHelper::FillValues over the whole CompoundSymMatrix (IpTripletHelper.cpp:249-362,
 * driven by IpTSymLinearSolver.cpp:453-533) and the per-factorisation 8 nnz-byte upload: the triplet value array is declared
 * once as a sequence of SEGMENTS that tile [0, nnz) -- for Ipopt: W | D_x | D_s | J_c | D_c | J_d | -I | D_d in the order of
 * IpStdAugSystemSolver.cpp:263-298 -- each with a device-resident source that is uploaded only when ITS content changed
 * (_assembly_buffer: pinned staging, _assembly_upload: async copy).  _factor_assembled forms
 *        values[offset_s + i] = scale_s * source_s[i] + shift_s          (scale_s = 0: the source is not read)
 * on the device (W_factor; delta_x, delta_s, -delta_c, -delta_d as shifts; the (4,2) block as scale 0, shift -1) and factors.
 * An inertia-correction retry (IpPDFullSpaceSolver.cpp:486-640: same matrices, new deltas) therefore uploads NOTHING. */
int  mi355x_kkt_assembly_define(mi355x_kkt_handle h, int nseg, const int64_t* offset, const int64_t* length);   /* nseg <= 16 */
double* mi355x_kkt_assembly_buffer(mi355x_kkt_handle h, int seg);
int  mi355x_kkt_assembly_upload(mi355x_kkt_handle h, int seg);
int  mi355x_kkt_factor_assembled(mi355x_kkt_handle h, const double* scale, const double* shift, int* num_neg, int* num_zero);

/* ---- the 8-block primal-dual system on the device -------------------------------------------------------
 * What PDFullSpaceSolver does around the augmented-system solves on host vectors -- eliminate the bound rows into the
 * right-hand side and expand the solution again (SolveOnce, IpPDFullSpaceSolver.cpp:418-424,653-659), form the residual of the
 * UNREDUCED system (ComputeResiduals, :666-793) and its max norms (ComputeResidualRatio, :795-820) for iterative refinement --
 * with the vectors resident in device memory: one upload of the right-hand side and one download of the result per Solve
 * instead of two PCIe round trips and two single-threaded host sparse products per refinement step.  A primal-dual vector is
 * the concatenation x | s | y_c | y_d | z_L | z_U | v_L | v_U (IteratesVector's component order); the handle owns
 * MI355X_KKT_PD_NVEC of them.  W, J_c and J_d are read from the device-resident sources of the value assembly (segments
 * `segs`), the expansion matrices P are their index lists (ExpansionMatrix::ExpandedPosIndices, 0-based), the iterate's
 * multipliers and slacks are uploaded with _pd_put_data.  The inertia-correction loop, the choice of the perturbations and
 * the refinement control stay with the caller (ipopt_adapter/IpMi355xPDSystemSolver.cpp).
 *   dims8   = { n_x, n_s, n_c, n_d, n_xL, n_xU, n_sL, n_sU }          (n_x + n_s + n_c + n_d = the analysed dimension)
 *   data8   = { z_L, z_U, v_L, v_U, slack_x_L, slack_x_U, slack_s_L, slack_s_U }
 *   _pd_solve_once: res <- alpha sol + beta res with sol the solution for right-hand side `rhs` through the CURRENT factorisation
 *   _pd_residual:   resid <- K8 res - rhs with the perturbations deltas4 = { delta_x, delta_s, delta_c, delta_d };
 *                   norms3 = max norms of rhs, res, resid */
#define MI355X_KKT_PD_NVEC 4
int  mi355x_kkt_pd_define(mi355x_kkt_handle h, const int32_t* dims8, const int32_t* idx_xl, const int32_t* idx_xu, const int32_t* idx_sl,
                          const int32_t* idx_su, const int32_t* irn, const int32_t* jcn, const int32_t* segs, int nsegs);
int  mi355x_kkt_pd_put_data(mi355x_kkt_handle h, const double* const* data8);
int  mi355x_kkt_pd_put(mi355x_kkt_handle h, int vec, const double* const* blocks8);
int  mi355x_kkt_pd_get(mi355x_kkt_handle h, int vec, double* const* blocks8);
int  mi355x_kkt_pd_solve_once(mi355x_kkt_handle h, int rhs, int res, double alpha, double beta);
int  mi355x_kkt_pd_residual(mi355x_kkt_handle h, int rhs, int res, int resid, const double* deltas4, double* norms3);

/* Solve A X = B in place for nrhs right-hand sides, rhs[irhs*ld + i], host memory. */
int  mi355x_kkt_solve(mi355x_kkt_handle h, int nrhs, double* rhs_inout, int ld);
/* Same with rhs/solution resident in device memory (nrhs columns, leading dimension ld). */
int  mi355x_kkt_solve_device(mi355x_kkt_handle h, int nrhs, double* d_rhs_inout, int ld);
/* Out-of-place variant: X = A^{-1} B, B untouched.  All device buffers handed to the library must be
 * complete when the call is made (the library works on its own stream; the caller synchronises the
 * stream that produced them). */
int  mi355x_kkt_solve_device2(mi355x_kkt_handle h, int nrhs, const double* d_b, int ldb, double* d_x, int ldx);

/* ---- low-rank update of the factored system: solve with K~ = K + V V^T - U U^T -------------------------------------------------------
 * What the reference's LowRankAugSystemSolver does around an augmented-system solver when `hessian_approximation limited-memory` hands it
 * W = B0 + V V^T - U U^T (IpLowRankAugSystemSolver.cpp): factor K with W = diag(B0), solve for the columns of the update and factor two small
 * dense matrices (UpdateFactorization, :299-396), correct every later solve by Sherman-Morrison (Solve, :195-228) -- with the tall-skinny
 * algebra on the device instead of host MultiVectorMatrix products (HighRankUpdateTranspose :319,:367,:383; AddRightMultMatrix :370).
 * V is rows x nv, U is rows x nu; they act on the first `rows` indices of the caller's numbering (Ipopt's x block; zero rows below) or, with a
 * row map (_lowrank_rowmap below), on the `rows` indices it names: K~ = K + P (V V^T - U U^T) P^T.
 *   update:  Z1 = K^-1 V,  M1 = I + sym(V^T Z1),  W1 = K^-1 U,  C = M1^-1 (Z1^T U),  Z2 = W1 - Z1 C,  M2 = I - sym(U^T Z2),  sym(G) = (G + G^T) / 2
 *   solve:   x0 = K^-1 b,  x1 = x0 - Z1 M1^-1 (V^T x0),  x = x1 + Z2 M2^-1 (U^T x1)      (the reference's Z^T b taken from the running solution: in place)
 * M1 and M2 positive definite <=> K~ has K's inertia; a Cholesky failure is the reference's "wrong inertia" answer (ComputeCholeskyFactor :323, :387 -> SYMSOLVER_WRONG_INERTIA :330, :392).
 *   _lowrank_set     V, U: HOST memory, column-major V[j*ldv + i]; copied and kept on the device across refactorisations and delayed-pivot structure
 *                    edits, until the next _lowrank_set or _lowrank_clear.  Marks the update not current.
 *   _lowrank_update  after a factorisation: SUCCESS, or WRONG_INERTIA with *which_failed (may be NULL) = 1 (M1) / 2 (M2) -- then no update is in force
 *   _lowrank_solve / _lowrank_solve_device2   the contracts of _solve / _solve_device2 with K~ in the place of K.  They need a CURRENT update: one
 *                    that _lowrank_update completed on the factorisation now in the handle (every factor / refactor / factor_assembled ends it); FATAL otherwise
 *   _lowrank_clear   removes the update;  _lowrank_info   what is set, whether it is current, host ms of the last _lowrank_update (outputs may be NULL)
 * While an update is set, _pd_solve_once applies the correction to the 4-block solution (it needs a current update) and _pd_residual adds
 * V (V^T res_x) - U (U^T res_x) to the x rows, so the W segment of the assembly carries B0 only; both need rows <= n_x (under a row map: idx[rows-1] < n_x).
 * Arguments are checked before the device is touched; single-GPU handles only (nranks > 1: FATAL). */
#define MI355X_KKT_LOWRANK_MAX 32                       /* columns of V, and of U */
int  mi355x_kkt_lowrank_set(mi355x_kkt_handle h, int rows, int nv, const double* V, int ldv, int nu, const double* U, int ldu);
int  mi355x_kkt_lowrank_update(mi355x_kkt_handle h, int* which_failed);
int  mi355x_kkt_lowrank_solve(mi355x_kkt_handle h, int nrhs, double* rhs_inout, int ld);
int  mi355x_kkt_lowrank_solve_device2(mi355x_kkt_handle h, int nrhs, const double* d_b, int ldb, double* d_x, int ldx);
int  mi355x_kkt_lowrank_clear(mi355x_kkt_handle h);
int  mi355x_kkt_lowrank_info(mi355x_kkt_handle h, int* rows, int* nv, int* nu, int* current, double* update_ms);
/* The row map: the reference's P_LowRank.  `hessian_approximation_space nonlinear-variables` (the default, IpOrigIpoptNLP.cpp:127,258) gives a TNLP that
 * declares its nonlinear variables W = P (B0 + V V^T - U U^T) P^T with P an ExpansionMatrix onto an ascending index subset of x; the updater works in
 * the reduced space (IpLimMemQuasiNewtonUpdater.cpp:169-193, :313-325) and LowRankAugSystemSolver expands every column through P before its solves
 * (IpLowRankAugSystemSolver.cpp:274-290, :449-457).  Here: row i of V, U, S, Y, DR, s, y is the caller's index idx[i] -- 0-based (whatever index_base
 * says of the matrix), STRICTLY ascending, 0 <= idx[i] < n: ExpansionMatrix::ExpandedPosIndices.  rows = 0 or idx = NULL removes the map.
 *   _lowrank_rowmap      idx: HOST memory, `rows` entries, copied (once to the device, into an arena of its own).  Every argument is validated on the
 *                        host before the device is touched -- that check is why no kernel can index out of range -- FATAL names `rows`, `idx`, the
 *                        first position that is not ascending or the first value out of range.  The map is a property of the handle, stated in the
 *                        caller's numbering: it survives factorisations, delayed-pivot structure edits, _lowrank_clear, _lbfgs_reset and _lbfgs_clear
 *                        (a new _analyse ends it).  Setting or removing it while a low-rank update is set or a history is defined: FATAL (clear first).
 *   while a map is set   _lowrank_set, _lbfgs_define, _lbfgs_define_sr1, _lbfgs_define_resto take `rows` equal to the map's (FATAL otherwise); V, U, s,
 *                        y, ypart, dr and _lbfgs_get 0..3, 14 stay `rows` long, in the reduced space; _lowrank_info, _lbfgs_info, _lbfgs_get are unchanged.
 *   _lowrank_rowmap_get  *rows (0: no map) and the indices; FATAL when `capacity` (entries) is below rows; outputs may be NULL
 *   _lowrank_rowmap_check  stand-alone, HOST, no handle, no GPU: the validation itself for a system of n rows, and -- len >= 0 -- of a full-space
 *                        vector length against the map (len > idx[rows-1]); SUCCESS, or FATAL with the reason in msg (capacity bytes, may be NULL)
 * What stays with the caller, as the reference does it: B0 on the diagonal -- with ReducedDiag, sigma on the MAPPED diagonal entries and 0 elsewhere
 * (IpLowRankAugSystemSolver.cpp:286-290); for a restoration history, DR gathered through the map once, at _lbfgs_define_resto (:190-192).
 * With no map set every call runs exactly the code it ran before maps existed.  Single-GPU handles only. */
int  mi355x_kkt_lowrank_rowmap(mi355x_kkt_handle h, int rows, const int32_t* idx);
int  mi355x_kkt_lowrank_rowmap_get(mi355x_kkt_handle h, int* rows, int32_t* idx, int64_t capacity);
int  mi355x_kkt_lowrank_rowmap_check(int64_t n, int rows, const int32_t* idx, int64_t len, char* msg, int64_t capacity);

/* ---- limited-memory BFGS: the (s, y) history on the device, V and U formed there -------------------------------------------------------------
 * What the reference's LimMemQuasiNewtonUpdater does for `hessian_approximation limited-memory` with the BFGS update "with skipping" (its default),
 * IpLimMemQuasiNewtonUpdater.cpp -- with the tall products on the device instead of host MultiVectorMatrix products over the whole history: an
 * accepted step moves TWO vectors (s, y) to the device, V and U never exist in host memory.  History S = [s_1 .. s_k], Y = [y_1 .. y_k], oldest
 * first, k <= max_history, `rows` entries each (the first `rows` indices of the caller's numbering, or those of the row map, as for _lowrank_set).
 *   skip    (CheckSkippingBFGS :985-1019)  s^T y <= sqrt(eps) |s|_2 |y|_2: nothing changes.  A non-finite s^T s, s^T y or y^T y is a skip too (a
 *           stated deviation: the reference never sees one).
 *   store   (UpdateInternalData :769-818)  append the pair, or drop the oldest when the history is full; D = diag(s_i^T y_i), L (strictly lower,
 *           L_ij = s_i^T y_j, i > j) and S^T S follow by "augment" / "shift": only the new row and column are computed.
 *   sigma   (:405-432)  from the new pair: init 0 scalar1 s^T y / s^T s, 1 scalar2 y^T y / s^T y, 2 scalar3 their arithmetic, 3 scalar4 their
 *           geometric mean, 4 constant init_val; then clipped to [sigma_min, sigma_max].  Reference defaults: 0, 1, 1e-8, 1e8.  Before the first
 *           stored pair sigma = init_val.
 *   columns (:440-520)  V = Y D^(-1/2),  Lt = L D^(-1/2),  M = Lt Lt^T + sigma S^T S,  J = chol(M),  C = J^(-T),  Lbar = Lt^T C,
 *           U = sigma S C + V Lbar:  sigma I + V V^T - U U^T  is the BFGS matrix of the stored pairs started from sigma I.
 *   M not positive definite (:484-495)  the pair and sigma stay stored, the installed V, U stay what they were.
 * _lbfgs_push (host vectors of `rows`) / _lbfgs_push_device (device vectors, complete before the call; free again when it returns), *outcome (may be NULL):
 *   0  pair stored, V and U formed and INSTALLED as the handle's low-rank update, exactly as _lowrank_set(rows, memory, V, rows, memory, U, rows)
 *      would: the update is not current; the caller factors with sigma on the x diagonal and calls _lowrank_update
 *   1  skipped, nothing changed (an update that was current stays current)
 *   2  pair stored and sigma updated; M was not positive definite, the installed columns are unchanged.  The reference marks such a call "Ws",
 *      counts it as a skip (:489-495, :687-691) and keeps the W it had: the OLD sigma with the old columns.  skipped_in_a_row is 0 after it and
 *      _lbfgs_info reports the new sigma: a caller that follows the reference counts the skip itself and keeps the diagonal of its last outcome 0.
 * A push allocates no device memory while the installed shape (rows, nv, nu) stays the same (a full history).  The history survives
 * refactorisations and delayed-pivot structure edits; _lowrank_set / _lowrank_clear replace / remove the installed columns and leave it alone.
 *   _lbfgs_reset  forgets the pairs, sigma = init_val, removes the installed update;   _lbfgs_clear  undefines: frees the history
 *   _lbfgs_info   outputs may be NULL; skipped_in_a_row: pushes skipped since the last stored pair (the caller's reset policy reads it); push_ms:
 *                 host ms of the last push
 *   _lbfgs_get    what: 0 S, 1 Y (rows x memory, oldest first, column-major, ld = rows), 2 V, 3 U (the installed columns, ld = rows),
 *                 4 D (memory), 5 L, 6 S^T S (memory x memory, column-major); FATAL when `capacity` (doubles) is too small
 *   _lbfgs_coefficients  stand-alone, HOST, no handle, no GPU: C and Lbar (m x m, column-major) from S^T S, L, D (m x m, m x m, m) and sigma;
 *                 SUCCESS, SINGULAR (a D_j or a Cholesky pivot <= 0 or not finite), FATAL (m outside [0, 32] or a null array)
 * Arguments are checked before the device is touched; single-GPU handles only (nranks > 1: FATAL). */
#define MI355X_KKT_LBFGS_MAX 32                         /* = MI355X_KKT_LOWRANK_MAX: V and U have one column per stored pair */
int  mi355x_kkt_lbfgs_define(mi355x_kkt_handle h, int rows, int max_history, int init, double init_val, double sigma_min, double sigma_max);
int  mi355x_kkt_lbfgs_push(mi355x_kkt_handle h, const double* s, const double* y, int* outcome);
int  mi355x_kkt_lbfgs_push_device(mi355x_kkt_handle h, const double* d_s, const double* d_y, int* outcome);
int  mi355x_kkt_lbfgs_reset(mi355x_kkt_handle h);
int  mi355x_kkt_lbfgs_clear(mi355x_kkt_handle h);
int  mi355x_kkt_lbfgs_info(mi355x_kkt_handle h, int* rows, int* max_history, int* memory, double* sigma, int* skipped_in_a_row, double* push_ms);
int  mi355x_kkt_lbfgs_get(mi355x_kkt_handle h, int what, double* out, int64_t capacity);
int  mi355x_kkt_lbfgs_coefficients(int m, const double* sts, const double* L, const double* D, double sigma, double* C_out, double* Lbar_out);

/* ---- limited-memory SR1: the same history, V and U from an eigen-split; one stored push can be taken back ---------------------------------------
 * `limited_memory_update_type sr1` of the same updater (IpLimMemQuasiNewtonUpdater.cpp :523-671, SplitEigenvalues :873-983).  A history defined by
 * _lbfgs_define_sr1 (the arguments of _lbfgs_define without the two clips) is served by the SAME _lbfgs_push / _push_device / _reset / _clear /
 * _info / _get; a push then works like this, D, L, S^T S being those of the BFGS history (same augment / shift):
 *   skip    no curvature test: only a non-finite s^T s, s^T y or y^T y, or the eigenvalue rule below
 *   sigma   (:551-578)  the new pair is the only stored one: init_val; otherwise with t = max(1e-8, |s^T y|): scalar1 t / s^T s, scalar2 y^T y / t,
 *           scalar3 / scalar4 their arithmetic / geometric mean, constant init_val.  NOT clipped.
 *   split   Z = D + L + L^T - sigma S^T S = Q diag(E) Q^T, E ascending, nneg of them < 0; emax = max(|E_0|, |E_(m-1)|), emin the |E_j| next to the
 *           sign change (E_0, -E_(m-1) or min(-E_(nneg-1), E_nneg)); the push is SKIPPED when emax = 0 or emin / emax < 1e-12 (:890-928)
 *   columns W = Y - sigma S, Qs[:, j] = Q[:, j] / sqrt(|E_j|):  U = W Qs[:, :nneg] (nu = nneg columns), V = W Qs[:, nneg:] (nv = memory - nneg):
 *           sigma I + V V^T - U U^T = sigma I + W Z^-1 W^T is the SR1 matrix of the stored pairs started from sigma I
 * Outcomes are 0 (stored, V and U installed as _lowrank_set(rows, nv, V, rows, nu, U, rows) would) and 1 (skipped) only.  A skipped push changes
 * NOTHING but skipped_in_a_row: the pair is committed only after the split rule has passed (the reference restores its backup, :624-628).
 * The split nv + nu = memory moves from push to push: the update's buffers get room for max_history columns on each side, so a push allocates nothing.
 *   _lbfgs_undo   SR1 only (a BFGS history: FATAL).  Takes the last stored push back (the reference's "Undoing most recent SR1 update", :523-532):
 *                 pairs -- the evicted one included --, D, L, S^T S, sigma and the split are those before that push, V and U are formed again from
 *                 them (bitwise what that earlier push installed; memory 0: the update is removed) and are not current; skipped_in_a_row is its
 *                 value before the undone push plus one; *undone (may be NULL) = 1.  One level: after a skipped push, an undo, _reset, _define*,
 *                 _clear there is nothing to undo and the call succeeds with *undone = 0, nothing changed.
 *                 The reference's own counter (lm_skipped_iter_, read by its limited_memory_max_skipping reset) is NOT part of what it restores: a
 *                 call that undoes (info_regu_x > 0, mark "Wb") adds one to it whether the push that follows is stored or skipped (:674-691), so
 *                 two such calls in a row reset the history (recorded: tests/golden/qn_sr1_517.qnrec, records 8-10).  skipped_in_a_row does not
 *                 follow that rule -- a stored push zeroes it --: the reset policy of an SR1 caller counts on its own (tests/test_qn_oracle.py Caller).
 *   _lbfgs_sr1_info  outputs may be NULL; type 0 BFGS / 1 SR1; nneg, E (the `memory` eigenvalues of the installed split, ascending; FATAL when
 *                 `capacity` is below memory) and can_undo are 0 / untouched for a BFGS history
 *   _lbfgs_sr1_coefficients  stand-alone, HOST, no handle, no GPU: E (m), Qs (m x m, column-major) and nneg from S^T S, L, D and sigma; SUCCESS,
 *                 SINGULAR (the split rule says skip: E and nneg are set, Qs is not scaled), FATAL (m outside [0, 32], a null array, or the cyclic
 *                 Jacobi eigen-solver did not converge within its 30 sweeps) */
#define MI355X_KKT_LBFGS_BFGS 0
#define MI355X_KKT_LBFGS_SR1  1
int  mi355x_kkt_lbfgs_define_sr1(mi355x_kkt_handle h, int rows, int max_history, int init, double init_val);
int  mi355x_kkt_lbfgs_undo(mi355x_kkt_handle h, int* undone);
int  mi355x_kkt_lbfgs_sr1_info(mi355x_kkt_handle h, int* type, int* nneg, int* can_undo, double* E, int capacity);
int  mi355x_kkt_lbfgs_sr1_coefficients(int m, const double* sts, const double* L, const double* D, double sigma, double* E_out, double* Qs_out, int* nneg_out);

/* ---- the restoration phase: Ypart in the history, eta per push, B0 = sigma I or eta D_R -----------------------------------------------------------
 * The `update_for_resto_` half of the same updater (IpLimMemQuasiNewtonUpdater.cpp UpdateHessian :141-343, :359-700, UpdateInternalData :820-868,
 * SetW, RecalcY/D/L :1338-1433), `limited_memory_special_for_resto` included.  Once per history: DR (`rows` positive entries, the restoration NLP's
 * DR_x), type (0 BFGS, 1 SR1) and special (0/1).  Per push: s, ypart (y WITHOUT the objective part) and eta = Eta(mu) > 0.  With o the element-wise
 * product, and restating the reference as it is:
 *   y_new   = ypart + eta DR o s (:337-341): the BFGS skip test, sigma, s^T y_new and y_new^T y_new use it.
 *   stored Y  = Ypart + eta S, WITHOUT DR (RecalcY is handed S in the place of DR o S, :864), with the CURRENT eta in every column; D_j = S_j^T Y_j and
 *           L_ij = S_i^T Y_j (i > j) are those of this Y and change with every eta.  Nothing is recomputed over the vectors: G = S^T Ypart, S^T S
 *           and, when special, R = S^T (DR o S) grow by one row and column per push, and D = diag(G) + eta diag(S^T S), L = G + eta S^T S below
 *           the diagonal.
 *   BFGS    the skip test of _lbfgs_push on (s, y_new); then D, L at the new eta, and when min D is not > 0 the push is SKIPPED (outcome 1, nothing
 *           but skipped_in_a_row changes, :387-399).  sigma as for _lbfgs_push from (s^T s, s^T y_new, y_new^T y_new); special: sigma stays -1 and is
 *           never used.  V takes only a NEW LAST COLUMN y_new / sqrt(s^T y_new) (:440-451): older columns stay what they were when pushed, although
 *           eta may have changed since (per pair the eta and the scale of its push are kept, and the column is formed from the ring).  d = D^(-1/2),
 *           Lt = L diag(d), M = Lt Lt^T + sigma S^T S, or + eta R when special; C, Lbar as for _lbfgs_push; U = sigma S C + V Lbar, or
 *           eta (DR o S) C + V Lbar.  M not positive definite: outcome 2, the pair and its V column are stored, the installed columns stay.
 *   SR1     no curvature test; sigma by the SR1 rule from (s^T s, s^T y_new, y_new^T y_new), not when special; Z = D + L + L^T - sigma S^T S, or
 *           - eta R; the split rule of _lbfgs_define_sr1 (a skip changes nothing but the counter); W = Y - sigma S, or Y - eta DR o S, Y the stored
 *           one above; U, V = W Qs split as there.  _lbfgs_undo works as for a plain SR1 history (eta and the Gram matrices come back too).
 *   B0      sigma I, or the vector eta DR when special (SetW :1343-1355): the caller puts it on the x diagonal before factoring, as it puts sigma.
 * The reference's |s|_max < 100 eps skip (:350-357) and its limited_memory_max_skipping reset stay with the caller, as the reset policy does.
 * A history defined by _lbfgs_define_resto is pushed by _lbfgs_push_resto / _push_resto_device ONLY (_lbfgs_push / _push_device on it: FATAL, and
 * the other way round); _reset (sigma = -1 when special, else init_val), _clear, _undo, _info, _sr1_info and _get serve it unchanged.  _lbfgs_get:
 * what 1 is Ypart, 4 and 5 are D, L at the eta of the last stored push; 10 G (memory x memory: diagonal and strictly lower part), 11 R (memory x
 * memory; zero unless special), 12 eta_col, 13 dv (memory; dv is 0 for SR1), 14 DR (rows); 10..14 on a plain history: FATAL.
 *   _lbfgs_resto_info  outputs may be NULL; resto 1 for such a history, special, eta of the last stored push (-1 before the first)
 * Arguments are checked before the device is touched (dr null or with an entry that is not positive and finite, eta not positive and finite, type
 * outside {0, 1}, special outside {0, 1}); single-GPU handles only.  A push costs what a plain push costs plus one more streamed vector per kernel. */
int  mi355x_kkt_lbfgs_define_resto(mi355x_kkt_handle h, int rows, int max_history, int type, int special, int init, double init_val, double sigma_min,
                                   double sigma_max, const double* dr);
int  mi355x_kkt_lbfgs_push_resto(mi355x_kkt_handle h, const double* s, const double* ypart, double eta, int* outcome);
int  mi355x_kkt_lbfgs_push_resto_device(mi355x_kkt_handle h, const double* d_s, const double* d_ypart, double eta, int* outcome);
int  mi355x_kkt_lbfgs_resto_info(mi355x_kkt_handle h, int* resto, int* special, double* eta);
/* Pushing FULL-SPACE vectors under a row map (the reference's P_LM^T s_full, P_LM^T y_full, IpLimMemQuasiNewtonUpdater.cpp:323-324): sx, yx (ypartx) are
 * x-block vectors of `len` entries, len > idx[rows-1]; HOST memory, or -- on_device != 0 -- device memory, complete before the call and free again when
 * it returns.  One launch gathers s[i] = sx[idx[i]], y[i] = yx[idx[i]] into the history's staging pair; then the call IS _lbfgs_push / _lbfgs_push_resto
 * of that pair: the same outcomes, the one download, the one synchronisation, the same bits.  No map set, len too small: FATAL, answered before the
 * device is touched.  _lbfgs_push* themselves keep taking reduced vectors of `rows` entries, with or without a map. */
int  mi355x_kkt_lbfgs_push_mapped(mi355x_kkt_handle h, const double* sx, const double* yx, int64_t len, int on_device, int* outcome);
int  mi355x_kkt_lbfgs_push_resto_mapped(mi355x_kkt_handle h, const double* sx, const double* ypartx, int64_t len, int on_device, double eta, int* outcome);

/* ---- the quasi-Newton pair (s, y) formed on the device from the resident Jacobians ---------------------------------------------------------------
 * What the same updater does before every update (IpLimMemQuasiNewtonUpdater.cpp:276-308):  s = x_k - x_(k-1) (:282) and
 *   y = (grad_f_k - grad_f_(k-1)) + J_c,k^T y_c + J_d,k^T y_d - J_c,k-1^T y_c - J_d,k-1^T y_d   (:304-307; the restoration phase drops the grad_f term: ypart, :297-300)
 * -- there four host products over nnz(J) per iteration.  Here the current Jacobian values are the device-resident sources of two segments of the value
 * assembly (_assembly_define / _assembly_upload), the previous ones a snapshot kept next to them, and one kernel pass forms
 *   s[j] = x[j] - x_last[j],   y[j] = (grad_f[j] - gf_last[j]) + sum over the entries (i, t) of column j of (J_cur[t] - J_last[t]) lam[i],   lam = y_c | y_d.
 * The difference PER ENTRY is a stated deviation from the reference's order of four products: an entry that did not change contributes an exact 0 (linear
 * constraints contribute exactly nothing), the cancellation happens before the multiplication; the difference to the reference's order is rounding only
 * (tests/support/qn_pair_spec.py: both orders within (k_j + 4) 2^-52 (|gf_j| + |gf_last_j| + sum (|J_cur| + |J_last|) |lam|), k_j entries in column j).
 * Every sum runs in a fixed order, there are no atomics on doubles: the result is bitwise reproducible.
 *   _qn_pair_check   stand-alone, HOST, no handle, no GPU: the validation _define performs on dims4 = {nx, ns, nc, nd}, the 1-based triplets and the two
 *                  ranges [off, off + len) of the triplet list; SUCCESS, or FATAL with the reason in msg (capacity bytes, may be NULL)
 *   _qn_pair_define  needs _analyse and _assembly_define.  irn, jcn: the 1-based triplets of _analyse, as _pd_define takes them; seg_jc, seg_jd: the assembly
 *                  segments that hold J_c and J_d (negative, or a segment of length 0: the block is absent).  nx + ns + nc + nd = n, ns = nd; every entry
 *                  of the J_c segment has one index in the x block [1, nx] and the other in the c block, of the J_d segment in the x and the d block
 *                  (either orientation; duplicates stay separate and sum).  FATAL names the argument and the first offending triplet position; nothing
 *                  reaches the device before the check has passed, which is why no kernel can index out of range.  The definition is stated in the
 *                  caller's numbering: it survives factorisations and delayed-pivot structure edits; a new _analyse or _assembly_define ends it.
 *   _qn_pair_store   the reference's last_x_ = curr_x, last_grad_f_, last_jac_c_, last_jac_d_ (:243-246, :700-703): x_last <- x, gf_last <- grad_f (NULL: the restoration
 *                  variant, y will be ypart), J_last <- a COPY of the segments' current device SOURCES (not of the assembled values: scale and shift of
 *                  _factor_assembled do not enter; a later _assembly_upload does not change it).  x == NULL: "roll" -- x and grad_f are those the last _form
 *                  was given, nothing is uploaded (FATAL when no pair is formed).  Marks "stored", clears "formed".
 *   _qn_pair_form    FATAL unless something is stored, and when grad_f is NULL here but was not in _store or the other way round.  x, grad_f (nx), y_c (nc),
 *                  y_d (nd): host memory, or -- on_device != 0 -- device memory, complete before the call and free again when it returns.  Reads whatever
 *                  the segment sources hold NOW: upload the current Jacobians first.  *amax_s (may be NULL) = max |s|, over the indices of the row map
 *                  when one is set (_lowrank_rowmap), over all nx otherwise (a NaN counts as +inf): what the reference's skip of a tiny step needs
 *                  (s_new->Amax() < 100 eps, :350-357 -- that test stays with the caller).  One download (the scalar) and one synchronisation, only when
 *                  amax_s is not NULL (device vectors: one synchronisation either way, they are free when the call returns).
 *   _qn_pair_push    FATAL unless a pair is formed and a history defined.  Pushes the formed DEVICE vectors through the existing paths, no vector makes a host
 *                  round trip: with a row map the path of _lbfgs_push_mapped / _push_resto_mapped (on_device, len = nx; the map must lie inside the x
 *                  block), without one that of _lbfgs_push_device / _push_resto_device on the first `rows` entries (rows <= nx, else FATAL).  A restoration
 *                  history takes eta and needs a pair formed without grad_f; a plain history ignores eta and needs one formed with grad_f; a mismatch
 *                  is FATAL.  Outcomes are those of the push that ran; bitwise the same as pushing the vectors of _get by hand.
 *   _qn_pair_get     what: 0 s, 1 y (nx; need a formed pair), 2 x_last, 3 grad_f_last (nx; FATAL on a snapshot stored without grad_f), 4 Jc_last, 5 Jd_last
 *                  (the segment lengths; 2..5 need a stored snapshot); FATAL when `capacity` (doubles) is too small
 *   _qn_pair_info    outputs may be NULL; nnz_j: entries of the column view; form_ms: host ms of the last _form
 *   _qn_pair_clear   undefines: frees the view, the snapshot and the pair
 * The kernel runs 1, 8 or 64 lanes per column, picked per definition from the structure alone (mean and longest column: qn_pair_host.h qp_pick_lpc);
 * _get_launch_plan "qn_pair" reports it.  Arguments and the state rules are checked before the device is touched; single-GPU handles only. */
int  mi355x_kkt_qn_pair_check(int64_t nnz, const int32_t* dims4, const int32_t* irn, const int32_t* jcn, int64_t off_jc, int64_t len_jc, int64_t off_jd, int64_t len_jd,
                              char* msg, int64_t capacity);
int  mi355x_kkt_qn_pair_define(mi355x_kkt_handle h, const int32_t* dims4, const int32_t* irn, const int32_t* jcn, int seg_jc, int seg_jd);
int  mi355x_kkt_qn_pair_store(mi355x_kkt_handle h, const double* x, const double* grad_f, int on_device);
int  mi355x_kkt_qn_pair_form(mi355x_kkt_handle h, const double* x, const double* grad_f, const double* y_c, const double* y_d, int on_device, double* amax_s);
int  mi355x_kkt_qn_pair_push(mi355x_kkt_handle h, double eta, int* outcome);
int  mi355x_kkt_qn_pair_get(mi355x_kkt_handle h, int what, double* out, int64_t capacity);
int  mi355x_kkt_qn_pair_info(mi355x_kkt_handle h, int* defined, int* stored, int* formed, int* nx, int64_t* nnz_j, double* form_ms);
int  mi355x_kkt_qn_pair_clear(mi355x_kkt_handle h);

int  mi355x_kkt_set_pivtol(mi355x_kkt_handle h, double u);
int  mi355x_kkt_set_pivtolmax(mi355x_kkt_handle h, double umax);
/* IncreaseQuality (IpSparseSymLinearSolverInterface.hpp:220): raises u <- min(pivtolmax, u^0.75) (the rule of
 * IpMa97SolverInterface.cpp:822-854, IpMa27TSolverInterface.cpp:724-740) and returns 1 -- the caller then refactors,
 * mi355x_kkt_refactor -- or returns 0 when u is at its maximum (with opts.smart_quality = 1 also when the last factorisation found
 * that no pivot decision depends on u up to pivtolmax: nothing a refactorisation could improve).  *new_u (may be NULL) receives the new u. */
int  mi355x_kkt_increase_quality(mi355x_kkt_handle h, double* new_u);
int  mi355x_kkt_get_info(mi355x_kkt_handle h, mi355x_kkt_info* info);
/* Symmetric scaling at run time (the option `scaling` only sets the initial mode): 0 none, 1 Ruiz inf-norm equilibration
 * on the device (the algorithm of MC77), 2 the caller's factors (n doubles, caller's numbering; copied), 3 maximum-product
 * matching scaling (the job of MC64: Duff & Koster 2001; host algorithm, recomputed at every factorisation while selected), 4 the same computed once and
 * reused until mi355x_kkt_increase_quality or a new _set_scaling (IpMa97SolverInterface.cpp:725-771: SWITCH_AT_START_REUSE / ON_DEMAND_REUSE), 5 / 6 = the job of
 * 3 / 4 done on the device by a Jacobi auction (feasible duals by construction: |s_i a_ij s_j| <= 1 on every entry; the matched entries of the unsymmetrised
 * scaling are >= e^(-1/64); info.matching_ms / _rounds / _unmatched describe the last computation).  _get_scaling returns the factors the last
 * factorisation used.  Together they give the MA97 call protocol its meaning: control.scaling > 0 => compute and hand back in
 * scale[], control.scaling == 0 with scale != NULL => reuse the caller-held factors, else none (IpMa97SolverInterface.cpp:641-678). */
int  mi355x_kkt_set_scaling(mi355x_kkt_handle h, int mode, const double* user_factors);
int  mi355x_kkt_get_scaling(mi355x_kkt_handle h, double* factors_out);
/* Stand-alone (no handle): Ruiz factors of a triplet matrix computed on the device -- the hook for a host that scales outside
 * the solver, i.e. Ipopt's TSymScalingMethod (IpTSymLinearSolver.cpp:429-441,511-514; cf. IpMc19TSymScalingMethod.cpp:100-204). */
int  mi355x_kkt_ruiz_scaling(int device, int n, int nnz, const int* irn, const int* jcn, const double* a, int index_base,
                             int sweeps, double* factors_out);
/* Stand-alone, HOST (no GPU needed): symmetric maximum-product matching scaling of a triplet matrix -- what HSL's MC64 provides
 * to MA97 / SPRAL (`ma97_scaling mc64`, `spral_scaling matching`): |s_i a_ij s_j| <= 1 with equality on a maximum transversal.
 * *num_unmatched (may be NULL) = structural rank deficiency. */
int  mi355x_kkt_matching_scaling(int n, int nnz, const int* irn, const int* jcn, const double* a, int index_base,
                                 double* factors_out, int* num_unmatched);
/* The columns (caller's index base) whose pivot was numerically zero in the last factorisation, ascending; *count = how
 * many there are (idx may be NULL / shorter).  This is what DetermineDependentRows needs
 * (IpSparseSymLinearSolverInterface.hpp:240-255; MUMPS' PIVNUL_LIST, IpMumpsSolverInterface.cpp:617-709). */
int  mi355x_kkt_zero_pivots(mi355x_kkt_handle h, int* idx, int capacity, int* count);
/* Delayed pivoting across fronts -- what MA27 / MA57 / MA97 / MUMPS / SPRAL do with a fully-summed column that finds no acceptable pivot in
 * its front (Duff & Reid 1983; consequences read at IpMa97SolverInterface.cpp:719-779, IpMa27TSolverInterface.cpp:565-622,
 * IpSpralSolverInterface.cpp:199-204).  factor / refactor / factor_assembled do it themselves (opts.delay_rounds); the two pieces are exposed:
 *   _failed_pivots   the columns (caller's index base, ascending) the last factorisation eliminated although they failed the threshold tests
 *   _delay_columns   move the given columns from their front's supernode to the parent front's and rebuild the symbolic structures (host work;
 *                    a handle with a device sets the numeric side up again; the next factor() uses the new structure).  *moved = columns
 *                    that moved (a root front has no parent); a column that has been moved before climbs 2, 4, 8 ... tree levels. */
int  mi355x_kkt_failed_pivots(mi355x_kkt_handle h, int* idx, int capacity, int* count);
int  mi355x_kkt_delay_columns(mi355x_kkt_handle h, const int* cols, int count, int* moved);
int  mi355x_kkt_set_delay_rounds(mi355x_kkt_handle h, int rounds);      /* opts.delay_rounds at run time (0 = static pivoting) */
const char* mi355x_kkt_last_error(mi355x_kkt_handle h);

/* ---- symbolic introspection (host logic tests, debugging; sizes via get_info) ---- */
/* what: 0 perm[n] (new->old), 1 sn_colptr[num_sn+1], 2 sn_rowptr[num_sn+1], 3 sn_rows[sum_sn_rows],
 *       4 sn_parent[num_sn], 5 sn_level[num_sn], 6 rel[sum_sn_rows] (position of each update row in the
 *       parent's front, -1 for pivot rows), 7 aperm_colptr[n+1], 8 aperm_row[nnz_a] (permuted lower CSC),
 *       9 trip2slot[nnz_in] (triplet -> permuted CSC slot), 10 pair_of[n] (old index of the 2x2 partner or -1),
 *       11 sn_owner[num_sn] (multi-GPU rank owning the supernode, -1 = replicated top),
 *       12 apos[nnz_a] (row + col*m position of each permuted-CSC slot inside its supernode panel),
 *       13 level_ptr[num_levels*4+1], 14 level_sn[num_sn] (launch schedule: buckets (level, front class)),
 *       15 grp_pos[num_sn], 16 grp_rem[num_sn] (chain groups: position in the group, columns of the later links),
 *       17 alias_child[num_sn] (in-place chains: the child whose contribution block hosts this front, or -1),
 *       18 sn_glo[num_sn], 19 sn_gsz[num_sn] (multi-GPU: the range of ranks [glo, glo + gsz) that holds the front: one rank for an owned
 *       front, all ranks for the classic replicated top, the ranks beneath it with opts.subcube), 20 sn_gdepth[num_sn] (bisections of the
 *       machine above that range = the exchange step the front belongs to),
 *       21 dup_ptr[nnz_a + 1], 22 dup_src[nnz_in] (the triplets of every CSC slot in ascending order: the order in which the device sums
 *       duplicates), 23 sn_class[num_sn] (kernel class of the front: 0 order <= 32, 1 <= 64, 2 <= 128, 3 the blocked path, order > 128),
 *       24 rslot_ptr[n + 1], 25 rslot_idx[rslot_ptr[n]], 26 rslot_col[rslot_ptr[n]] (the symmetric row view of the permuted pattern the equilibration
 *       sweeps and the device refinement gather over: for every row its entries of both triangles -- CSC slot and the other index -- by ascending other index).
 *       sn_parent (4) is the parent in the ASSEMBLY tree: a side child of an in-place chain link may hang on a lower link of that chain (finish_analysis 9b).
 *  27   the storage plan of the contribution blocks, 5 ints: {window of tree levels after which a dead block's space is written again (0: every block
 *       resident), then as (low, high) 32-bit halves: doubles of all blocks if every one were resident, doubles of the blocks that are never reused};
 *       info.cb_doubles is what the plan needs.  Blocks that only carry a contribution to their parent are RECYCLED over the level schedule where that
 *       saves a quarter of the pool (MI355X_KKT_RECYCLE=0/1 forces it off / on) -- the workspace a multifrontal code keeps as a stack
 *       (IpMumpsSolverInterface.cpp:151-177, ICNTL(14)), here with static addresses.
 *  28   the offset (doubles, inside the contribution-block arena) of every front's block as (low, high) halves: 2 * num_sn ints. */
int  mi355x_kkt_get_symbolic(mi355x_kkt_handle h, int what, int* out, int64_t capacity);

/* ---- launch-plan introspection (host only: works after the analysis, needs no device): the launch plan rank `rank` of `nranks` (the world
 * size of the analysis) would run.  *count = ints of array `what`; out == NULL only queries the count.  what:
 *   "level_list" the launch list (entries of the buckets, of the solve units, of the join lists and of the grouped schedules), "tiny16" /
 *   "tiny_split" / "mid_split" / "big_split" (per level: leading fronts of the sorted single-GPU WAVE / LDS128 / BIG buckets taken by another kernel),
 *   "<s>.ptr|base|maxm|maxk|last0|last1|allsolo" for schedule <s> = single, local (own subtrees), stage<d> (replicated fronts of exchange step d),
 *   "lc_ptr" / "lc_fronts" (leaf chains: their fronts, leaf first), "df_runs" ({lv0, lv1, tab0, nlev, nq} per k_front_df run),
 *   "chain_segs" (9 ints per data-flow sweep segment), "chain_links" ({s, k, koff, fi} per link), "chain_descs" ({link0, nlinks, tail, ktot, s0, init}
 *   per chain), "join" ({base, count, maxm, who} per kind), "exchange" ({step, glo, gsz, arena doubles, top-rhs doubles} per range),
 *   "qn_pair" {defined, lanes per column of k_qn_pair (1, 8 or 64), longest column, nx, entries of the column view as (low, high) halves} -- the launch of
 *   _qn_pair_form (state of the handle, not of the analysis),
 *   "col_owner", "stat_owner", "scalars" {levels, exchange steps, leaf-chain levels, leaf chains, look-ahead, grouped, tfuse fronts, big fronts, stages}.
 *   What a system REACHES -- the fields the kernels and the launch code branch on (the tests show with them that a fixture runs the path it names):
 *   "path_bits" one int per launch-list entry: 1 contribution block formed by its update (tfuse), 2 assembles itself (selfasm), 4 solo (fused forward
 *   solve), 8 split (look-ahead), 16 has an XCD tile table, 32 has a second one (part 2 of a split update), 64 asmcut != 0, 128 k_big_assemble2's
 *   fast path is open to it, 256 in place on a child;  "asm_fast_ok" (per entry: children that kernel pulls, 0 = not for it), "asmcut" (per entry);
 *   "levels" 10 ints per level {la_tiles1, la_tiles2, la_full, lv_asm_skip, lv_narrow_tiles, part_tiles[0], part_tiles[1], wave_mmin (2^30: no such
 *   front), wave_mmax, wave_kmax};  "groups" 11 ints per level of the single-GPU / own-subtree grouped schedule {g0, g1, split, nrb, tiles64, tiles,
 *   la1, la2, p1t, la3, nsplit};  "path_scalars" {pair_solve, la_any, ints of the tile tables, grp_cut_level, solve_group, cb_window};
 *   "inputs" the settings the plan is built with {chain_solve, fuse_dt, fastpiv, asm_pull, leafchain, front_df, tfuse, fuse_upd, selfasm, grouped,
 *   xcd_tiles, lookahead, pair_solve, p1_small, la_wgs, la_min_nt, grp_rbw_max, chain_solve_maxc, fuse_dt_maxwg, la_min_tiles, side_small}.
 *   The factor schedule -- every launch and stream operation of a factorisation between the equilibration and the statistics, in issue order:
 *   "factor.single.full" / "factor.single.opt" (one GPU: every strict launch / the optimistic schedule), "factor.local", "factor.stage<d>" (multi-rank),
 *   13 ints per record {op, stream, kind, gx, gy, block, level, b0, lds, a0, a1, a2, a3}:
 *   op  0 k_leaf_chain, 1 k_front_df, 2 k_front_dpp16, 3 k_front_reg<64,2>, 4 <64,4>, 5 <64,8>, 6 <256,6,true,4>, 7 <256,8,true>, 8 <256,6>, 9 <256,8>,
 *       10 k_big_assemble, 11 k_big_assemble2, 12 k_grp_fused, 13 k_big_diag_trsm, 14 k_big_diag_reg<4>, 15 <4,1024>, 16 k_big_trsm<false>, 17 <true>,
 *       18 k_big_schur64, 19 k_big_schur, 20 k_big_schur_p1, 21 k_big_schur_q, and the stream operations 22 fork (event A of (a0, level) recorded on the
 *       main stream, the look-ahead stream waits for it), 23 fork-done (event B of (a0, level) recorded on the look-ahead stream), 24 join (the main
 *       stream waits for event B of (a0, a1); level: where the join stands), 25 side-open, 26 side-close (the side stream of `level`);
 *   stream 0 main, 1 look-ahead, 2 side;  kind: MI355X_KKT_KERNEL_* the profile books the launch under (-1: a stream operation);
 *   gx, gy: the grid in workgroups -- but op 1: virtual workgroups (clamped to the resident ones at launch), op 19: 128 x 128 tiles, op 11: columns
 *   (chunks of 16 per workgroup);  block: threads (0: the kernel's own: op 19);  b0: first launch-list entry;  lds: dynamic LDS bytes where the plan
 *   knows them (ops 3-9, 11; the pivot-block and panel kernels size theirs at launch from a[]);  a0..a3, the kernel's integer arguments, per op:
 *   0 {chains, last level}  1 {tab0, levels, virtual workgroups, last level}  2 {fronts, top_mode, raise-the-flag}  3-9 {flags}  10 {top_mode}
 *   11 {top_mode, ldi, maxch}  12 {staged, rbw}  13 {row blocks, kk}  14-17 {kk}  19 {part}  21 {tiles of part 2}  22-24 {event index: 0 the
 *   single-GPU schedule, 1 + i grouped schedule i;  24: a1 the level of the fork}.
 *   The solve-block schedule (mi355x_kkt_set_solve_block; nranks = 1 only): "solve.single.block", the launches of ONE block of right-hand sides, the same
 *   13 ints per record, in the order  bulk forward | top part of one column | bulk backward  (the loads, stores and refinement kernels around them are
 *   element-wise launches per column and not listed).  `stream` holds the way the record is issued: 0 blocked (one launch of the kernel's *_rb form takes
 *   every active column), 1 by column (the one-column kernel, once per active column; consecutive records of this kind are issued column by column), 2 top part (the levels from the first chain segment up: every
 *   column runs through all records of kind 2 on its own, one column after the other).  op:
 *       0 k_bump_epoch, 1 k_fwd_leafchain, 2 k_bwd_leafchain, 3 k_fwd_pair<16,16>, 4 k_fwd_pair<16>, 5 k_fwd_pair<32>, 6 k_bwd_pair<16,16>, 7 k_bwd_pair<16>,
 *       8 k_bwd_pair<32>, 9 k_fwd_mid<1>, 10 k_fwd_mid<2>, 11 k_bwd_mid<1>, 12 k_bwd_mid<2>, 13 k_fwd<64> (order <= 32), 14 k_fwd<64> (order <= 64),
 *       15 k_fwd<256>, 16 k_bwd<64> (order <= 32), 17 k_bwd<64> (order <= 64), 18 k_bwd<256>, 19 k_fwd_solo64, 20 k_fwd_solo, 21 k_fwd_grp,
 *       22 k_fwd_grp_upd, 23 k_bwd_dot64, 24 k_bwd_fin64, 25 k_bwd_grp_dot, 26 k_bwd_grp, 27 k_fwd_chain, 28 k_bwd_chain;
 *   b0: first launch-list entry (27, 28: first workgroup record; 1, 2: 0);  a0: fronts (3-8) / chains (1, 2) of the launch, else 0;  a1..a3: 0. */
int  mi355x_kkt_get_launch_plan(mi355x_kkt_handle h, int nranks, int rank, const char* what, int* out, int64_t capacity, int64_t* count);

/* ---- blocks of right-hand sides in the solves (single-GPU handles; opt-in).  on != 0: a solve call with nrhs >= 2 (solve, solve_device*, the inner solves
 * of lowrank_update / lowrank_solve*) takes its right-hand sides through the bulk of the tree MI355X_KKT_SOLVE_BLOCK at a time -- one launch per (level,
 * class) for all columns of a block where the kernel has a blocked form, the front's part of L read once --, and through the chain sweeps at the top of
 * the tree one column after the other.  Every solution column is bit for bit what a solve of its own gives.  A remainder of one column, nrhs = 1 and
 * mi355x_kkt_profile take the usual path.  0 (the default): off.  Valid before and after the analysis; a multi-GPU handle is refused (FATAL).
 * _solve_block_info (any pointer may be NULL; after the analysis, needs no device): the switch, the width, the first level of the top part (num_levels:
 * no chain sweep), the launches of ONE FULL block of the current plan -- blocked launches, launches by column (width x the records of that kind), the
 * launches of the top part PER COLUMN -- and the time of the last solve call that took the blocked path (0: none). ---- */
#define MI355X_KKT_SOLVE_BLOCK 4
int  mi355x_kkt_set_solve_block(mi355x_kkt_handle h, int on);
int  mi355x_kkt_solve_block_info(mi355x_kkt_handle h, int* on, int* width, int* first_top_level, int* blocked_launches, int* bycol_launches, int* top_launches_per_column, double* last_ms);

/* ---- measurement: device time per kernel kind (hip events around every launch of an eager, graph-less factor + one
 * solve -- on the stream the kernel is launched on: the look-ahead parts of the largest trailing updates run, and are
 * measured, on the solver's second stream exactly as in a timed factorisation --, accumulated over `reps` repetitions).
 * ms/launches need MI355X_KKT_KERNEL_COUNT entries.  Used by bench.py for the roofline of the dominant kernel. ---- */
#define MI355X_KKT_KERNEL_GATHER_SCALE  0   /* value gather + Ruiz equilibration                                   */
#define MI355X_KKT_KERNEL_FRONT_WAVE    1   /* k_front_dpp16 + k_front_reg<64,*> : fronts of order <= 32            */
#define MI355X_KKT_KERNEL_FRONT_LDS64   2   /* k_front_reg<64,8>  : order <= 64, one wavefront each                */
#define MI355X_KKT_KERNEL_FRONT_LDS128  3   /* k_front_reg<256,*> : order <= 128                                   */
#define MI355X_KKT_KERNEL_BIG_ASSEMBLE  4
#define MI355X_KKT_KERNEL_BIG_DIAG      5
#define MI355X_KKT_KERNEL_BIG_TRSM      6
#define MI355X_KKT_KERNEL_BIG_SCHUR     7   /* fp64 MFMA frontal update                                            */
#define MI355X_KKT_KERNEL_STATS         8
#define MI355X_KKT_KERNEL_SOLVE_PERM    9
#define MI355X_KKT_KERNEL_FWD_WAVE     10
#define MI355X_KKT_KERNEL_FWD_LDS      11
#define MI355X_KKT_KERNEL_FWD_BIG      12
#define MI355X_KKT_KERNEL_BWD_WAVE     13
#define MI355X_KKT_KERNEL_BWD_LDS      14
#define MI355X_KKT_KERNEL_BWD_BIG      15
#define MI355X_KKT_KERNEL_FWD_BIG_UPD 16   /* chain groups: update of the entries beyond the group (many workgroups) */
#define MI355X_KKT_KERNEL_BWD_BIG_DOT 17   /* chain groups: partial L21^T x of the rows beyond the group             */
#define MI355X_KKT_KERNEL_COUNT        18
int  mi355x_kkt_profile(mi355x_kkt_handle h, int reps, double* ms, int* launches, int capacity);

/* ---- multi-GPU (one process per GPU; subtrees sharded, top of the tree replicated) ----
 * Create every rank's handle with opts.nranks = P, opts.rank = r, analyse the SAME structure on every rank, then give the
 * handle a communicator.  From then on the ordinary entry points (factor / refactor / solve / solve_device*) run the
 * distributed sequence themselves, on the solver's stream, without host synchronisation between the phases:
 *     factor:  own subtrees -> all-reduce(top arena: lower triangles of the join fronts, fp64 sum) -> replicated top -> all-reduce(inertia counters)
 *     solve :  local forward -> all-reduce(top rhs) -> replicated top fwd/bwd -> local backward -> all-reduce(solution)
 * Inputs (values, right-hand sides) are identical on every rank, outputs (inertia, status, solution) too -- which is what
 * Ipopt needs when every rank runs the same (deterministic) algorithm around its share of the linear algebra; cf. the
 * knobs the reference exposes for SPRAL's multi-GPU mode (IpSpralSolverInterface.cpp:55-67).
 *   _comm_unique_id        rank 0: ncclGetUniqueId -> 128 bytes the launcher hands to every rank (file, MPI, torch store ...)
 *   _set_comm_rccl         ncclCommInitRank(nranks, id, rank) on the handle's device: RCCL over xGMI.  librccl.so is
 *                          dlopen()ed here; single-GPU users never load it
 *   _set_comm_callbacks    a host that has its own communication layer supplies the one collective we need: in-place sum over
 *                          the ranks of `count` elements of DEVICE memory (dtype 0 = fp64, 1 = int32), ordered after the work
 *                          already enqueued on `hip_stream` and complete (or stream-ordered) when it returns; 0 = success */
typedef int (*mi355x_kkt_allreduce_fn)(void* ctx, void* dptr, int64_t count, int dtype, void* hip_stream);
int  mi355x_kkt_comm_unique_id(void* out128);
int  mi355x_kkt_set_comm_rccl(mi355x_kkt_handle h, const void* unique_id128);
int  mi355x_kkt_set_comm_callbacks(mi355x_kkt_handle h, mi355x_kkt_allreduce_fn fn, void* ctx);
/*   _comm_shm_id           rank 0: creates a POSIX shared-memory segment for `nranks` ranks of ONE node and writes its name into out128 (handed to
 *                          the other ranks like the RCCL id)
 *   _set_comm_shm          every rank: attaches (rank 0 unlinks the name once all have) and installs a host-staged sum -- device -> slot, sum of
 *                          the slots in rank order (bitwise the same on every rank), -> device -- for both collectives above.  For ranks that
 *                          SHARE a device (RCCL refuses that), bring-up and the one-GPU test box; the production path is RCCL.  A peer that does
 *                          not arrive within MI355X_KKT_SHM_TIMEOUT_S (300) fails the call: never a hang.  The communicator in the adapter has the
 *                          reference's MPI_Init-inside-the-interface as its precedent (IpMumpsSolverInterface.cpp:58-75). */
int  mi355x_kkt_comm_shm_id(void* out128, int nranks);
void mi355x_kkt_comm_shm_discard(const void* id128);      /* rank 0: the id could not be handed to the other ranks after all -- unlink the segment nobody attached to */
int  mi355x_kkt_set_comm_shm(mi355x_kkt_handle h, const void* id128);
/* Range-local exchange.  A replicated front is held by a RANGE of ranks [rank_lo, rank_lo + nranks_in_range) and what it receives comes from
 * ranks of that range only, so its arena square (lower triangle, packed) and its top right-hand side are summed among those ranks alone:
 * with RCCL through one sub-communicator per exchange step (ncclCommSplit, created by _set_comm_rccl; without it -- or with
 * MI355X_KKT_DISABLE=subcomm -- every step is ONE all-reduce over the whole communicator, ranks outside a range contributing zeros), with a
 * callback communicator through this optional second callback (same contract as mi355x_kkt_allreduce_fn, plus the range; ctx is the one
 * given to _set_comm_callbacks; only ranks of the range call it).
 *   _exchange_bytes   bytes of all arena squares / all top right-hand sides of the current structure (what the exchange steps move) */
typedef int (*mi355x_kkt_allreduce_range_fn)(void* ctx, void* dptr, int64_t count, int dtype, void* hip_stream, int rank_lo, int nranks_in_range);
int  mi355x_kkt_set_comm_range_callback(mi355x_kkt_handle h, mi355x_kkt_allreduce_range_fn fn);
int  mi355x_kkt_exchange_bytes(mi355x_kkt_handle h, int64_t* arena_bytes, int64_t* rhs_bytes);
/* What ONE rank of the handle's nranks will ask of its communicator, in order, for one factorisation + one solve -- and the ncclCommSplit calls
 * _set_comm_rccl makes before them.  HOST ONLY (needs _analyse, not a device): a launcher or a test can check on any machine that all ranks
 * issue matching sequences (same communicator, same count, same order) before an 8-GPU job is started; the reference's only counterpart is
 * MUMPS' own MPI layer behind IpMumpsSolverInterface.cpp:191-245.  Records of 6 ints {what, step, colour, range size, count, dtype}:
 *   what 0 = ncclCommSplit(colour, key = rank) (colour -1 = NCCL_SPLIT_NOCOLOR), 1 = sum of arena squares, 2 = inertia / pivot statistics,
 *        3 = sum of top right-hand sides, 4 = sum of the solution pieces;  colour = first rank of the range whose sub-communicator carries the
 *        collective, -2 = the whole communicator;  dtype 0 = fp64, 1 = int32;  range_local = 0: the fall-back of one whole-communicator sum per step.
 *   _comm_info   the communicator in use: kind 0 none / 1 callbacks / 2 RCCL, the size the communicator itself reports (ncclCommCount), whether
 *                range-local collectives are on (ncclCommSplit succeeded everywhere / a range callback is set), exchange steps of the structure */
int  mi355x_kkt_comm_plan(mi355x_kkt_handle h, int rank, int range_local, int* records6, int capacity_records, int* count);
int  mi355x_kkt_comm_info(mi355x_kkt_handle h, int* kind, int* ranks_seen, int* range_local, int* exchange_steps);
/* The phases are also exposed one by one (a caller that wants to overlap or replace the collectives): */
/* The top-of-tree fronts live in one contiguous device buffer ("top arena").  After
 * factor_local() each rank holds its own subtrees' Schur contributions there; the caller
 * sums the arena over ranks (RCCL all-reduce) and calls factor_top().  See DESIGN.md (e). */
int  mi355x_kkt_factor_local(mi355x_kkt_handle h, const double* dvals);
int  mi355x_kkt_top_arena(mi355x_kkt_handle h, double** dptr, int64_t* ndoubles);
int  mi355x_kkt_factor_top(mi355x_kkt_handle h, int* num_neg_local, int* num_zero_local);
int  mi355x_kkt_solve_fwd_local(mi355x_kkt_handle h, double* d_rhs);
int  mi355x_kkt_top_rhs(mi355x_kkt_handle h, double** dptr, int64_t* ndoubles);
int  mi355x_kkt_solve_top_and_bwd(mi355x_kkt_handle h, double* d_rhs);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_KKT_H */
