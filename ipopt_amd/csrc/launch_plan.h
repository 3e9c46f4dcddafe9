// launch_plan.h -- the launch plan of the numeric phase: every launch the factorisation and the solves make, and the tables the kernels
// read, computed on the host from the symbolic structure alone (launch_plan.cpp; no device).  numeric.hip materialises it on the device.
#pragma once
#include "symbolic.h"
#include "kernel_tables.h"
#include <cstddef>
#include <string>
#include <vector>

namespace mi355x {

// what the plan depends on besides the structure: the rank, and the MI355X_KKT_DISABLE / _TUNE settings it reads (env_knobs.h)
struct PlanInputs {
    int nranks = 1, rank = 0;
    bool multi = false;                  // the multi-rank schedule (nranks > 1, or MI355X_KKT_FORCE_MULTI)
    int verbose = 0;
    bool chain_solve = true, fuse_dt = true, fastpiv = true, asm_pull = true, leafchain = true, front_df = true, tfuse = true, fuse_upd = true,
         selfasm = true, grouped = true, xcd_tiles = true, lookahead = true, pair_solve = true, p1_small = true;
    bool side_small = true;              // a handful of small fronts beside a level's bulk go to the side stream (build_factor_schedule)
    bool mid_solve = true;               // fronts of order 33..128 on the solves' level launches: k_fwd_mid / k_bwd_mid (numeric.hip solve_level reads the same knob)
    int la_wgs = 1 << 20, la_min_nt = 8, grp_rbw_max = 8, chain_solve_maxc = 128, fuse_dt_maxwg = 448;
    long long la_min_tiles = 4000;
    double fastpiv_floor = 1e-4;         // (0.01 up to r03a: 9 % of the synth_1e6 blocks then took the strict loop and set the pace of their level: 23.1 -> 22.0 ms)
    // the factor pool in pieces (numeric.hip setup): a linear offset lin of the  L | cb  layout lies at lin + pool_delta[i] from V.L, i = the last
    // pool_cut <= lin.  Empty: one piece, the identity.
    std::vector<long long> pool_cut, pool_delta;
};
PlanInputs plan_inputs_from_env(int nranks, int rank, bool multi, int verbose);

// buckets (level, class) of the fronts of one schedule and their launch geometry
struct Sched { std::vector<int> ptr; int base = 0; std::vector<int> maxm, maxk, tiles, tiles64, last0, last1; std::vector<char> allsolo; };   // last0/1: per level, the group-last BIG fronts (solve units)
// grouped schedule: per level the chain groups whose FIRST link sits there (entries = FrontMeta of the LAST link, sorted by order, split at 1024
// rows like the BIG buckets), launch geometry, look-ahead tiles
struct GrpSched { std::vector<int> g0, g1, split, nrb, tiles64, tiles, la1, la2, p1t, la3, nsplit; };      // p1t: 64 x 64 tiles of a split front's part 1, la3: tiles of the fronts not split, nsplit: split fronts (among the large ones)
// a run of consecutive levels of pure chain links, one data-flow launch per sweep
struct ChainSeg { int lv0, lv1, desc0, ndesc, nwg_f, nwg_b, maxtail, wgf0, wgb0; };
// Exchange steps (subtree-to-subcube mapping; the classic replicated top is the case of ONE step): a replicated front is held by a range of
// ranks; what its children OUTSIDE that range -- subtrees owned by one rank, fronts of a sub-range -- contribute travels through the front's
// arena square / top-rhs accumulator, written by ONE reporting rank per child (its owner; the first rank of its range) and summed over the
// ranks, all ranges of one depth in one collective, deepest first.  join[c]: the fronts this rank reports a child of kind c to
// (c = 0: own subtree roots, c = 1 + d: fronts of its depth-d range) and the code those children carry in ChildMeta::owner.
struct JoinList { int base = 0, count = 0, maxm = 0, who = -1; };
struct RangeSeg { int d, glo, gsz; long long abeg, aend, tbeg, tend; };      // the part of a step of every range of ranks [glo, glo + gsz)
// runs of consecutive tree levels that hold nothing but one-wavefront fronts (order <= 32): one persistent data-flow launch each (k_front_df)
struct DfRun { int lv0, lv1, tab0, nlev, nq; };

// kernel kinds for the profiling entry point (order = include/mi355x_kkt.h MI355X_KKT_KERNEL_*)
enum KernelKind { KK_GATHER_SCALE = 0, KK_FRONT_WAVE, KK_FRONT_LDS64, KK_FRONT_LDS128, KK_BIG_ASSEMBLE, KK_BIG_DIAG, KK_BIG_TRSM,
                  KK_BIG_SCHUR, KK_STATS, KK_SOLVE_PERM, KK_FWD_WAVE, KK_FWD_LDS, KK_FWD_BIG, KK_BWD_WAVE, KK_BWD_LDS, KK_BWD_BIG, KK_FWD_BIG_UPD, KK_BWD_BIG_DOT, KK_COUNT };
// One record of a factor schedule: a kernel instantiation the factorisation launches, or a stream operation.  The values are exported
// (mi355x_kkt_get_launch_plan "factor.*", include/mi355x_kkt.h): append, do not renumber.
enum FactorOp { FO_LEAF_CHAIN = 0, FO_FRONT_DF, FO_FRONT_DPP16, FO_REG_64_2, FO_REG_64_4, FO_REG_64_8, FO_REG_256_6_FAST4, FO_REG_256_8_FAST, FO_REG_256_6, FO_REG_256_8,
                FO_ASSEMBLE, FO_ASSEMBLE2, FO_GRP_FUSED, FO_DIAG_TRSM, FO_DIAG_REG, FO_DIAG_REG_1024, FO_TRSM, FO_TRSM_WIDE, FO_SCHUR64, FO_SCHUR, FO_SCHUR_P1, FO_SCHUR_Q,
                FO_FORK,            // event A of (a[0], lv) recorded on the main stream, the look-ahead stream waits for it
                FO_FORK_DONE,       // event B of (a[0], lv) recorded on the look-ahead stream
                FO_JOIN,            // the main stream waits for event B of (a[0], lv)
                FO_SIDE_OPEN,       // the side stream waits for what the main stream holds so far (side event F of level lv)
                FO_SIDE_CLOSE,      // the main stream waits for the side stream (side event J of level lv)
                FO_COUNT };
enum FactorStream { FS_MAIN = 0, FS_LOOKAHEAD = 1, FS_SIDE = 2 };
// gx, gy: the grid in workgroups, but for FO_FRONT_DF (gx: virtual workgroups; the executor clamps to what is resident), FO_SCHUR (gx: 128 x 128 tiles)
// and FO_ASSEMBLE2 (gx: columns) -- the kernel's own compile-time geometry (SCHUR_GM, ASM_CH) turns those into workgroups in the executor; block = 0:
// the kernel's own (FO_SCHUR: SCHUR_NT).  lds: dynamic LDS bytes where the plan knows them; the pivot-block and panel kernels size theirs from a[] with
// the functions beside their device layouts (diag_lds_bytes, trsm_lds_bytes).  Events are named by (a[0] = index into the executor's look-ahead
// events: 0 the single-GPU schedule, 1 + i the grouped schedule P.grp[i]; lv -- FO_JOIN: a[1], the level of the fork it waits for), never by handle.  a[]: the kernel's integer arguments behind b0, per op:
//   LEAF_CHAIN {chains, last level}  FRONT_DF {tab0, levels, virtual workgroups, last level}  FRONT_DPP16 {fronts, top_mode, raise-the-flag}  REG_* {flags}
//   ASSEMBLE {top_mode}  ASSEMBLE2 {top_mode, ldi, maxch}  GRP_FUSED {staged, rbw}  DIAG_TRSM {row blocks, kk}  DIAG_REG* {kk}  TRSM* {kk}
//   SCHUR {part}  SCHUR_Q {tiles of part 2}
struct FactorLaunch { int op, stream, kind, gx, gy, block, lv, b0, lds, a[4]; };      // kind: KernelKind (-1: a stream operation); b0: first launch-list entry
constexpr int FACTOR_LAUNCH_INTS = 13;       // the exported row: the fields in this order
constexpr int SIDE_MAX_FRONTS = 16;

// ---- the solve-block schedule (single-GPU handles, mi355x_kkt_set_solve_block): the right-hand sides of one call travel through the tree SOLVE_RB at a
//      time.  One record per launch of ONE block, in the field layout of FactorLaunch; `stream` holds the SolveBlockKind:
//        SB_BLOCKED  one launch of the *_rb form of the kernel takes all active columns
//        SB_BYCOL    the launch is issued once per active column, the work vectors of the DevView pointing at that column
//                    (a run of consecutive by-column records goes column by column: the pair of launches of a big-front level shares scratch)
//        SB_TOP      a launch of the top part (levels >= first_top_level: from the first chain segment up), which every column runs through on its own, one
//                    column after the other: epoch bump, forward walk, backward walk
//      The records stand in the order  bulk forward | top part of ONE column | bulk backward;  the executor (numeric.hip run_solve_block) repeats the middle
//      range per column.  The values are exported ("solve.single.block", include/mi355x_kkt.h): append, do not renumber.
//      b0: first launch-list entry (FWD/BWD_CHAIN: first workgroup record), a[0]: fronts / chains of the launch (0 where the kernel takes none), a[1]: top_mode (0).
constexpr int SOLVE_RB = 4;                  // columns per block (compile-time width of the *_rb kernels)
constexpr int SOLVE_MID_KMAX = 64;           // = MID_KMAX of kernels_solve.hip.inc: the pivot count k_fwd_mid / k_bwd_mid take
enum SolveOp { SO_BUMP_EPOCH = 0, SO_FWD_LEAFCHAIN, SO_BWD_LEAFCHAIN, SO_FWD_PAIR16_16, SO_FWD_PAIR16, SO_FWD_PAIR32, SO_BWD_PAIR16_16, SO_BWD_PAIR16, SO_BWD_PAIR32,
               SO_FWD_MID1, SO_FWD_MID2, SO_BWD_MID1, SO_BWD_MID2,
               SO_FWD_WAVE, SO_FWD_LDS64, SO_FWD_LDS128, SO_BWD_WAVE, SO_BWD_LDS64, SO_BWD_LDS128,      // k_fwd<64> (LDS for order 32 / 64), k_fwd<256>; k_bwd likewise
               SO_FWD_SOLO64, SO_FWD_SOLO, SO_FWD_GRP, SO_FWD_GRP_UPD, SO_BWD_DOT64, SO_BWD_FIN64, SO_BWD_GRP_DOT, SO_BWD_GRP,
               SO_FWD_CHAIN, SO_BWD_CHAIN, SO_COUNT };
enum SolveBlockKind { SB_BLOCKED = 0, SB_BYCOL = 1, SB_TOP = 2 };
struct SolveBlockSchedule {
    std::vector<FactorLaunch> rec;
    int first_top_level = 0;                 // L*: the first level >= the leaf-chain prefix that starts a chain segment (nlevels: none)
    int top0 = 0, top1 = 0;                  // rec[top0, top1): the top part of one column
    int blocked = 0, bycol = 0, top = 0;     // launches of one FULL block: blocked records, SOLVE_RB x by-column records; top records of ONE column
};

struct ExchangeLayout {
    std::vector<long long> aoff, troff;                  // per front: its arena square / top-rhs accumulator, or -1
    std::vector<long long> abeg, aend, tbeg, tend;       // per step: its part of the arena / of the top right-hand sides
    std::vector<RangeSeg> rsegs;                         // ... and inside a step the part of every range of ranks
    long long arena_doubles = 0, toprhs_doubles = 0;
};
ExchangeLayout exchange_layout(const Symbolic& Sy, int ndepth);
void comm_plan(const Symbolic& S, int nranks, int rank, bool range_local, std::vector<int>& out6);

struct LaunchPlan {
    int nlevels = 0;
    // the launch list (DevView::level_sn, FrontMeta parallel to it): the single-GPU buckets (level_ptr order, each sorted by front order), the
    // multi-rank schedules and join lists, the single-GPU solve units, the grouped schedules
    std::vector<int> lvl_list;
    Sched single;                                        // every front; its buckets are Symbolic::level_ptr
    int ndepth = 1;
    Sched local; std::vector<Sched> stage;              // multi-rank: the rank's own subtrees; stage[d]: the replicated fronts of exchange step d it holds
    std::vector<JoinList> join;
    ExchangeLayout ex;
    // single-GPU buckets: leading fronts of order <= 16 (FC_WAVE), <= 96 (FC_LDS128), <= 1024 (FC_BIG)
    std::vector<int> tiny16, tiny_split, mid_split, big_split, part_tiles[2];
    std::vector<size_t> mid_lds, reg_lds;                // LDS need of the register-tiled front kernel: the <= 96 part, every (level, class) bucket
    std::vector<int> wave_kmax, wave_mmax, wave_mmin;
    bool pair_solve = true;                              // solves of the order <= 32 fronts: two fronts per wavefront (k_fwd_pair / k_bwd_pair)
    // data-flow solve sweeps
    std::vector<ChainSeg> chain_segs; std::vector<int> seg_at_lv0, seg_at_lv1;      // level -> segment index (or -1)
    std::vector<char> in_seg;
    std::vector<ChainLink> chl; std::vector<ChainDesc> chd; std::vector<int> chwait, wgf, wgb;
    int ntailflags = 0, ndots = 0;
    // look-ahead of the group-end trailing updates (single-GPU schedule): per level the grids of the two parts
    std::vector<int> la_tiles1, la_tiles2; std::vector<char> la_full;
    bool la_any = false;
    std::vector<int> tile_tab;                           // XCD-aware tile orders of the large full updates
    std::vector<char> lv_asm_skip;                       // every big front of the level is a pure in-place chain link: no assembly launch at all
    std::vector<int> lv_narrow_tiles;                    // > 0: every big front of the level is a chain link with a narrow update; the 64 x 64 tiles of the largest one
    bool grouped = false;
    std::vector<GrpSched> grp;                           // [0]: every front (one GPU) / the rank's own subtrees; [1 + d]: replicated fronts of step d
    std::vector<char> asm_fast_ok; std::vector<int> asmcut;      // per launch-list entry: k_big_assemble2's fast path (children it pulls, 0: not for it); FrontMeta::asmcut (-1: nothing to assemble)
    int ntfuse = 0, nbig = 0;
    std::string error;                                   // non-empty: no plan (an internal inconsistency)
    int lc_levels = 0, lc_nchains = 0;                   // leaf chains: the tree levels below lc_levels are lc_nchains chains of fronts of order <= 16
    std::vector<int> lc_ptr; std::vector<LeafLink> lc_link;
    std::vector<DfRun> df_runs; std::vector<int> df_run_at; std::vector<DfLevel> df_tab; std::vector<long long> cbt_off; long long cbt_len = 0;
    // the tables
    std::vector<FrontMeta> fmeta; std::vector<ChildMeta> cmeta; std::vector<GroupLink> gtab; std::vector<int> relinv;
    std::vector<long long> panel_off, cb_off;            // remapped pool offsets
    std::vector<int> stat_owner, col_owner;
    // the factor schedules this handle can run (NumericImpl::setup: build_factor_schedule): one GPU, [0] the full one, [1] the optimistic one; multi-rank
    std::vector<FactorLaunch> factor_single[2], factor_local; std::vector<std::vector<FactorLaunch>> factor_stage;
    SolveBlockSchedule solve_block;                      // one GPU: the blocked solve (NumericImpl::setup: build_solve_block_schedule)
};
LaunchPlan build_launch_plan(const Symbolic& Sy, const PlanInputs& in);
// The factor schedule of one Sched as a flat list: every launch and every stream operation of the factorisation between the equilibration and the
// statistics, in the order the executor (numeric.hip run_factor_list) issues them.  which: 0 = P.single, 1 = P.local, 2 + d = P.stage[d] (top_mode
// and the grouped schedule P.grp[...] follow from it).  optimistic: the schedule without the strict launches the static-order kernels make idle.
std::vector<FactorLaunch> build_factor_schedule(const LaunchPlan& P, const Symbolic& Sy, const PlanInputs& in, int which, bool optimistic);
// The launches of one block of right-hand sides on the single-GPU schedule P.single (see SolveBlockKind): the per-class launch choice of numeric.hip
// solve_level and the level walk of solve_sweep, restated as a list.
SolveBlockSchedule build_solve_block_schedule(const LaunchPlan& P, const Symbolic& Sy, const PlanInputs& in);

} // namespace mi355x
