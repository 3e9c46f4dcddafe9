// launch_plan.cpp -- host only (no HIP header, no device): the launch plan of the numeric phase, see launch_plan.h.  What numeric.hip's
// setup used to compute between its allocations; the kernels read the tables exactly as built here.
#include "launch_plan.h"
#include "env_knobs.h"
#include <algorithm>
#include <cstdio>
#include <map>

namespace mi355x {

PlanInputs plan_inputs_from_env(int nranks, int rank, bool multi, int verbose)
{
    PlanInputs in;
    in.nranks = nranks; in.rank = rank; in.multi = multi; in.verbose = verbose;
    in.chain_solve = !knob_disabled("chain_solve"); in.fuse_dt = !knob_disabled("fuse_dt"); in.fastpiv = !knob_disabled("fastpiv");
    in.asm_pull = !knob_disabled("asm_pull"); in.leafchain = !knob_disabled("leafchain"); in.front_df = !knob_disabled("front_df");
    in.tfuse = !knob_disabled("tfuse"); in.fuse_upd = !knob_disabled("fuse_upd"); in.selfasm = !knob_disabled("selfasm");
    in.grouped = !knob_disabled("grouped"); in.xcd_tiles = !knob_disabled("xcd_tiles"); in.lookahead = !knob_disabled("lookahead");
    in.pair_solve = !knob_disabled("pair_solve"); in.p1_small = !knob_disabled("p1_small"); in.side_small = !knob_disabled("side_small");
    in.mid_solve = !knob_disabled("mid_solve");
    in.la_wgs = (int)std::max(1ll, knob_int("la_wgs", in.la_wgs));
    in.la_min_nt = (int)std::max(3ll, knob_int("la_min_nt", in.la_min_nt));
    in.la_min_tiles = knob_int("la_min_tiles", in.la_min_tiles);     // (tests force 0)
    in.grp_rbw_max = (int)std::max(1ll, knob_int("grp_rbw_max", in.grp_rbw_max));
    in.chain_solve_maxc = (int)std::max(1ll, knob_int("chain_solve_maxc", in.chain_solve_maxc));
    in.fuse_dt_maxwg = (int)knob_int("fuse_dt_maxwg", in.fuse_dt_maxwg);
    knob_tune("fastpiv_floor", &in.fastpiv_floor);
    return in;
}

static int order_of(const Symbolic& Sy, int s) { return Sy.sn_rowptr[s + 1] - Sy.sn_rowptr[s]; }
static int cols_of(const Symbolic& Sy, int s) { return Sy.sn_colptr[s + 1] - Sy.sn_colptr[s]; }
static int nchild(const Symbolic& Sy, int s) { return Sy.child_ptr[s + 1] - Sy.child_ptr[s]; }
static int tri_tiles(int nt) { const int t = nt * (nt + 1) / 2; return nt >= 12 ? (t + 7) / 8 * 8 : t; }    // large ones: multiple of 8 (XCD-aware order)
// tiles of the trailing update of front s: 64 x 64 / 128 x 128 tiles of the whole lower triangle, or (not the last link of a chain group)
// only the tile columns of the group's remaining panels
static int schur_tiles64(const Symbolic& Sy, int s)
{
    const int nt = (order_of(Sy, s) - cols_of(Sy, s) + 63) / 64;
    return Sy.grp_rem[s] > 0 ? nt * ((Sy.grp_rem[s] + 63) / 64) : nt * (nt + 1) / 2;
}
static int schur_tiles(const Symbolic& Sy, int s)
{
    const int nt = (order_of(Sy, s) - cols_of(Sy, s) + 127) / 128;
    return Sy.grp_rem[s] > 0 ? nt * ((Sy.grp_rem[s] + 127) / 128) : tri_tiles(nt);
}
// LDS bytes of the register-tiled front kernel (k_front_reg) on a front of order m with k pivots, instantiated for fronts of order <= maxm
static size_t front_lds(size_t m, size_t k, size_t maxm)
{
    const size_t ld = m | 1, ldi = k | 1;
    return (std::max(m * (m + 1) / 2, k * ld + k * ldi) + 4 * maxm + 3 * k) * sizeof(double) + 2 * k * sizeof(int) + 64;
}
// a child goes through the arena / the top-rhs accumulators when its parent is a replicated front of ANOTHER range of ranks
static bool same_range(const Symbolic& Sy, int a, int b) { return Sy.sn_owner[a] < 0 && Sy.sn_owner[b] < 0 && Sy.sn_glo[a] == Sy.sn_glo[b] && Sy.sn_gsz[a] == Sy.sn_gsz[b]; }
static bool crosses(const Symbolic& Sy, int c) { const int pa = Sy.sn_parent[c]; return pa >= 0 && Sy.sn_owner[pa] < 0 && !same_range(Sy, c, pa); }

// The layout of the exchange steps (a function of the symbolic structure only, the same on every rank; the C ABI's mi355x_kkt_comm_plan walks it
// on a machine without a GPU): top-rhs accumulators for every replicated front; arena squares only for those with a child from outside their range
// (the joins): that is all the all-reduce has to carry (A is replicated input, not reduced).  Only the LOWER triangle of a square travels (packed by
// columns, the layout the front kernels assemble into), and inside a step the squares are grouped by the range of ranks that holds their front: what
// a front receives comes from ranks of its own range only, so a range sums its part among its own ranks (sub-communicator / range callback) -- the
// other ranks neither send nor receive it.
ExchangeLayout exchange_layout(const Symbolic& Sy, int ndepth)
{
    ExchangeLayout X;
    X.aoff.assign(Sy.num_sn, -1); X.troff.assign(Sy.num_sn, -1);
    std::vector<char> is_join(Sy.num_sn, 0);
    for (int c = 0; c < Sy.num_sn; ++c) if (crosses(Sy, c)) is_join[Sy.sn_parent[c]] = 1;
    X.abeg.assign(ndepth, 0); X.aend.assign(ndepth, 0); X.tbeg.assign(ndepth, 0); X.tend.assign(ndepth, 0);
    for (int d = 0; d < ndepth; ++d) {
        X.abeg[d] = X.arena_doubles; X.tbeg[d] = X.toprhs_doubles;
        std::vector<std::pair<int, int>> ranges;
        for (int s = 0; s < Sy.num_sn; ++s) if (Sy.sn_owner[s] < 0 && Sy.sn_gdepth[s] == d) {
            const std::pair<int, int> rg(Sy.sn_glo[s], Sy.sn_gsz[s]);
            if (std::find(ranges.begin(), ranges.end(), rg) == ranges.end()) ranges.push_back(rg);
        }
        std::sort(ranges.begin(), ranges.end());
        for (const auto& rg : ranges) {
            RangeSeg sg{d, rg.first, rg.second, X.arena_doubles, 0, X.toprhs_doubles, 0};
            for (int s = 0; s < Sy.num_sn; ++s) if (Sy.sn_owner[s] < 0 && Sy.sn_gdepth[s] == d && Sy.sn_glo[s] == rg.first && Sy.sn_gsz[s] == rg.second) {
                const long long m = order_of(Sy, s);
                X.troff[s] = X.toprhs_doubles; X.toprhs_doubles += m;
                if (is_join[s]) { X.aoff[s] = X.arena_doubles; X.arena_doubles += m * (m + 1) / 2; }
            }
            sg.aend = X.arena_doubles; sg.tend = X.toprhs_doubles;
            X.rsegs.push_back(sg);
        }
        X.aend[d] = X.arena_doubles; X.tend[d] = X.toprhs_doubles;
    }
    return X;
}

// The collectives ONE rank issues, in order, for a factorisation and for one solve -- and the ncclCommSplit calls of make_subcomms() before them:
// records of 6 ints {what, depth, colour, range size, count, dtype}; what: 0 = ncclCommSplit (colour -1: NCCL_SPLIT_NOCOLOR, key = rank), 1 = all-reduce of
// arena squares, 2 = inertia / pivot statistics, 3 = all-reduce of top right-hand sides, 4 = solution pieces; colour = first rank of the range (sub-communicator
// of that step) or -2 = the whole communicator.  The SAME walk as factor_dist / solve_dist / make_subcomms / exchange_step, without a device.
void comm_plan(const Symbolic& Sy, int nranks, int rank, bool range_local, std::vector<int>& out)
{
    const int ndepth = std::max(1, Sy.num_gdepths);
    const ExchangeLayout X = exchange_layout(Sy, ndepth);
    auto rec = [&](int what, int d, int colour, int gsz, long long count, int dtype) { out.push_back(what); out.push_back(d); out.push_back(colour); out.push_back(gsz); out.push_back((int)std::min<long long>(count, 0x7fffffffll)); out.push_back(dtype); };
    if (range_local)
        for (int d = 0; d < ndepth; ++d) {
            bool partial = false; int color = -1;
            for (const RangeSeg& sg : X.rsegs) if (sg.d == d && sg.gsz < nranks) { partial = true; if (sg.glo <= rank && rank < sg.glo + sg.gsz) color = sg.glo; }
            if (partial) rec(0, d, color, 0, 0, 1);
        }
    auto step = [&](int d, int what) {
        if (range_local) {
            for (const RangeSeg& sg : X.rsegs) {
                if (sg.d != d || !(sg.glo <= rank && rank < sg.glo + sg.gsz)) continue;
                const long long cnt = what == 1 ? sg.aend - sg.abeg : sg.tend - sg.tbeg;
                if (cnt > 0) rec(what, d, sg.gsz >= nranks ? -2 : sg.glo, sg.gsz, cnt, 0);
            }
        } else {
            const long long cnt = what == 1 ? X.aend[d] - X.abeg[d] : X.tend[d] - X.tbeg[d];
            if (cnt > 0) rec(what, d, -2, nranks, cnt, 0);
        }
    };
    for (int d = ndepth - 1; d >= 0; --d) step(d, 1);
    rec(2, 0, -2, nranks, 8, 1);
    for (int d = ndepth - 1; d >= 0; --d) step(d, 3);
    if (Sy.n > 0) rec(4, 0, -2, nranks, Sy.n, 0);
}

LaunchPlan build_launch_plan(const Symbolic& Sy, const PlanInputs& in)
{
    LaunchPlan P;
    const int NL = Sy.num_levels, NS = Sy.num_sn;
    const bool multi = in.multi;
    P.nlevels = NL;
    auto bucket0 = [&](int lv, int fc) { return Sy.level_ptr[(size_t)lv * FC_COUNT + fc]; };          // the single-GPU bucket (lv, fc) is [bucket0(lv, fc), bucket0(lv, fc + 1))
    auto pool_remap = [&](long long lin) {
        if (in.pool_cut.empty()) return lin;
        const size_t i = (size_t)(std::upper_bound(in.pool_cut.begin(), in.pool_cut.end(), lin) - in.pool_cut.begin()) - 1; return lin + in.pool_delta[i]; };
    P.panel_off.resize(NS); P.cb_off.resize(NS);
    for (int sn = 0; sn < NS; ++sn) {
        P.panel_off[sn] = pool_remap(Sy.panel_off[sn]);                                    // panel of a front, relative to V.L
        P.cb_off[sn] = pool_remap(Sy.l_doubles + Sy.cb_off[sn]) - Sy.l_doubles;            // contribution block, relative to V.cb = V.L + l_doubles
    }
    std::vector<int>& L = P.lvl_list;
    L.assign(Sy.level_sn.begin(), Sy.level_sn.end());
    std::vector<char> solve_entry;      // parallel to L: 1 = entry of a solve-unit list
    // the fronts of a schedule: 0 = every front (one GPU), 1 = the rank's own subtrees, 2 + d = the replicated fronts of exchange step d held by this rank
    auto in_sched = [&](int which, int s) {
        if (which == 0) return true;
        if (which == 1) return Sy.sn_owner[s] == in.rank;
        return Sy.sn_owner[s] < 0 && Sy.sn_glo[s] <= in.rank && in.rank < Sy.sn_glo[s] + Sy.sn_gsz[s] && Sy.sn_gdepth[s] == which - 2;
    };
    // the buckets (level, class) of a schedule, ascending front index, their launch geometry and solve units.  The single-GPU buckets are the
    // leading part of the launch list already; a multi-rank schedule's are appended to it.
    auto build_sched = [&](Sched& sc, int which) {
        sc.ptr.assign((size_t)NL * FC_COUNT + 1, 0); sc.base = which == 0 ? 0 : (int)L.size();
        sc.maxm.assign(NL, 0); sc.maxk.assign(NL, 0); sc.tiles.assign(NL, 0); sc.tiles64.assign(NL, 0);
        std::vector<std::vector<int>> bucket((size_t)NL * FC_COUNT);
        for (int s = 0; s < NS; ++s) {
            if (!in_sched(which, s)) continue;
            const int lv = Sy.sn_level[s];
            bucket[(size_t)lv * FC_COUNT + Sy.sn_class[s]].push_back(s);
            if (Sy.sn_class[s] == FC_BIG) { sc.maxm[lv] = std::max(sc.maxm[lv], order_of(Sy, s)); sc.maxk[lv] = std::max(sc.maxk[lv], cols_of(Sy, s));
                                            sc.tiles[lv] = std::max(sc.tiles[lv], schur_tiles(Sy, s)); sc.tiles64[lv] = std::max(sc.tiles64[lv], schur_tiles64(Sy, s)); }
        }
        for (size_t b = 0; b < bucket.size(); ++b) {
            sc.ptr[b + 1] = sc.ptr[b] + (int)bucket[b].size();
            if (which != 0) L.insert(L.end(), bucket[b].begin(), bucket[b].end());
        }
        sc.last0.assign(NL, 0); sc.last1.assign(NL, 0); sc.allsolo.assign(NL, 0);
        for (int lv = 0; lv < NL; ++lv) {
            sc.last0[lv] = (int)L.size();
            bool all = true;      // every solve unit of the level is one link with nothing to gather (fused forward kernel)
            for (int sn : bucket[(size_t)lv * FC_COUNT + FC_BIG]) if (Sy.grp_rem[sn] == 0 || !Sy.solve_group) {
                L.push_back(sn); solve_entry.resize(L.size(), 0); solve_entry.back() = 1;
                if (!((Sy.alias_child[sn] >= 0 && nchild(Sy, sn) == 1) || (Sy.alias_child[sn] < 0 && nchild(Sy, sn) == 0))) all = false;
            }
            sc.last1[lv] = (int)L.size();
            sc.allsolo[lv] = (!Sy.solve_group && all && sc.last1[lv] > sc.last0[lv]) ? 1 : 0;
        }
    };
    P.ex.aoff.assign(NS, -1); P.ex.troff.assign(NS, -1);
    P.col_owner.assign(Sy.n, 0);
    if (multi) {
        const int R = std::max(1, in.nranks);
        P.ndepth = std::max(1, Sy.num_gdepths);
        build_sched(P.local, 1);
        P.stage.assign(P.ndepth, Sched());
        for (int d = 0; d < P.ndepth; ++d) build_sched(P.stage[d], 2 + d);
        P.ex = exchange_layout(Sy, P.ndepth);
        // what this rank reports: its own subtree roots (kind 0), and -- as the first rank of its depth-d range -- that range's fronts (kind 1 + d)
        P.join.assign(P.ndepth + 1, JoinList());
        for (int c = 0; c <= P.ndepth; ++c) {
            JoinList& J = P.join[c]; J.base = (int)L.size(); J.who = in.rank + R * c;
            std::vector<char> listed(NS, 0);
            for (int ch = 0; ch < NS; ++ch) {
                if (!crosses(Sy, ch)) continue;
                const bool rep = c == 0 ? Sy.sn_owner[ch] == in.rank : (Sy.sn_owner[ch] < 0 && Sy.sn_gdepth[ch] == c - 1 && Sy.sn_glo[ch] == in.rank);
                if (rep) listed[Sy.sn_parent[ch]] = 1;
            }
            for (int s = 0; s < NS; ++s) if (listed[s]) { L.push_back(s); ++J.count; J.maxm = std::max(J.maxm, order_of(Sy, s)); }
        }
        // the solution pieces are summed over the ranks: a column is reported by its owner / by the first rank of its front's range
        for (int s = 0; s < NS; ++s) {
            const int o = Sy.sn_owner[s] >= 0 ? Sy.sn_owner[s] : (Sy.sn_glo[s] == in.rank ? in.rank : R);
            for (int j = Sy.sn_colptr[s]; j < Sy.sn_colptr[s + 1]; ++j) P.col_owner[j] = o;
        }
    }
    // the single-GPU buckets sorted by front order (stable); returns the number of leading fronts of order <= maxorder
    auto sort_split = [&](int lv, int fc, int maxorder) {
        const int b0 = bucket0(lv, fc), b1 = bucket0(lv, fc + 1);
        std::stable_sort(L.begin() + b0, L.begin() + b1, [&](int a, int b) { return order_of(Sy, a) < order_of(Sy, b); });
        int q = b0; while (q < b1 && order_of(Sy, L[q]) <= maxorder) ++q;
        return q - b0;
    };
    P.tiny_split.assign(NL, 0); P.tiny16.assign(NL, 0); P.mid_split.assign(NL, 0); P.mid_lds.assign(NL, 0); P.big_split.assign(NL, 0);
    for (int h = 0; h < 2; ++h) P.part_tiles[h].assign(NL, 0);
    for (int lv = 0; lv < NL; ++lv) {
        // FC_WAVE: fronts of order <= 16 first.  When there are many of them (throughput regime) they run on the 2x2-tile instantiation, whose small
        // register footprint doubles the number of resident wavefronts.
        P.tiny16[lv] = sort_split(lv, FC_WAVE, 16);
        P.tiny_split[lv] = P.tiny16[lv] >= 2048 ? P.tiny16[lv] : 0;
        // FC_LDS128: fronts of order <= 96 first; they run on the 6x6-tile instantiation (half the registers and LDS of the 8x8 one => two workgroups per CU)
        const int nmid = sort_split(lv, FC_LDS128, 96);
        for (int q = bucket0(lv, FC_LDS128); q < bucket0(lv, FC_LDS128) + nmid; ++q) P.mid_lds[lv] = std::max(P.mid_lds[lv], front_lds(order_of(Sy, L[q]), cols_of(Sy, L[q]), 96));
        P.mid_split[lv] = nmid >= 256 ? nmid : 0;
        // FC_BIG: split at 1024 rows.  The two halves are launched separately: tighter rectangular grids on heterogeneous levels, and the small fronts
        // (a handful of tiles, K = 16..64) take the 256-thread 64 x 64 trailing-update kernel while the large ones take the 1024-thread one.
        P.big_split[lv] = sort_split(lv, FC_BIG, 1024);
        for (int e = bucket0(lv, FC_BIG); e < bucket0(lv, FC_BIG + 1); ++e) {
            const int sn = L[e], h = e < bucket0(lv, FC_BIG) + P.big_split[lv] ? 0 : 1;
            P.part_tiles[h][lv] = std::max(P.part_tiles[h][lv], h == 0 ? schur_tiles64(Sy, sn) : schur_tiles(Sy, sn));
        }
    }
    build_sched(P.single, 0);
    // ---- sync-free (data-flow) sweeps over the latency-bound top of the tree: a SEGMENT is a run of consecutive levels whose fronts are
    // all BIG with <= 64 pivots and of which there are at most chain_maxc per level; its fronts are cut into CHAINS (maximal runs of
    // in-place links: every link after the first has the previous link as its only child and shares its vector), and ONE launch per
    // sweep runs the whole segment: workgroups wait on flags for exactly what they consume (see k_fwd_chain / k_bwd_chain) ----
    auto& chl = P.chl; auto& chd = P.chd; auto& chwait = P.chwait; auto& wgf = P.wgf; auto& wgb = P.wgb;
    P.seg_at_lv0.assign(NL, -1); P.seg_at_lv1.assign(NL, -1);
    P.pair_solve = in.pair_solve && !multi;
    P.wave_kmax.assign(NL, 0); P.wave_mmax.assign(NL, 0); P.wave_mmin.assign(NL, 1 << 30);
    for (int sn = 0; sn < NS; ++sn) if (Sy.sn_class[sn] == FC_WAVE) {
        const int lv = Sy.sn_level[sn];
        P.wave_kmax[lv] = std::max(P.wave_kmax[lv], cols_of(Sy, sn)); P.wave_mmax[lv] = std::max(P.wave_mmax[lv], order_of(Sy, sn)); P.wave_mmin[lv] = std::min(P.wave_mmin[lv], order_of(Sy, sn));
    }
    if (!Sy.solve_group && in.chain_solve) {
        auto cnt = [&](int l) { return bucket0(l, FC_COUNT) - bucket0(l, 0); };
        // multi-GPU: only runs of >= 4 levels made of pure links of the replicated top (nothing to gather inside the launch: the
        // distributed sweeps exchange the joins between launches)
        auto pure = [&](int sn) { return Sy.sn_class[sn] == FC_BIG && Sy.alias_child[sn] >= 0 && nchild(Sy, sn) == 1 && cols_of(Sy, sn) <= 64; };
        std::vector<char> lvok(NL, 0);
        for (int lv = 0; lv < NL; ++lv) {
            const int a = bucket0(lv, 0), b = bucket0(lv, FC_COUNT);
            bool ok = b > a && b - a <= in.chain_solve_maxc;
            for (int q = a; q < b && ok; ++q) {
                const int sn = Sy.level_sn[q];
                if (multi) ok = pure(sn) && Sy.sn_level[Sy.alias_child[sn]] == lv - 1 && Sy.sn_owner[sn] < 0 && Sy.sn_gdepth[sn] == 0 && Sy.sn_gsz[sn] >= in.nranks;
                else       ok = cols_of(Sy, sn) <= 64;          // (any class: to the sweeps a small front is a one-link chain like any other)
            }
            lvok[lv] = ok ? 1 : 0;
        }
        std::vector<int> chain_of(NS, -1);
        P.in_seg.assign(NS, 0);
        for (int lv = 0; lv < NL; ) {
            if (!lvok[lv]) { ++lv; continue; }
            int e = lv;
            while (e + 1 < NL && lvok[e + 1] && (!multi || cnt(e + 1) == cnt(lv))) ++e;
            if (e - lv + 1 >= (multi ? 4 : 2)) {
                ChainSeg sg{lv, e, (int)chd.size(), 0, 0, 0, 0, (int)wgf.size(), (int)wgb.size()};
                // chains, in the order of their first links' levels
                const size_t chl0 = chl.size();
                for (int l = lv; l <= e; ++l)
                    for (int q = bucket0(l, 0); q < bucket0(l, FC_COUNT); ++q) {
                        const int sn = Sy.level_sn[q], ac = Sy.alias_child[sn];
                        P.in_seg[sn] = 1;
                        ChainLink K{}; K.panel_off = P.panel_off[sn]; K.minv_off = Sy.minv_off[sn]; K.c0 = Sy.sn_colptr[sn]; K.k = cols_of(Sy, sn); K.ldp = Sy.sn_ldp[sn];
                        K.s = sn; K.r0 = Sy.sn_rowptr[sn];
                        const int cprev = (ac >= 0 && nchild(Sy, sn) == 1 && Sy.sn_level[ac] >= lv) ? chain_of[ac] : -1;
                        if (cprev >= 0) {          // next link of its child's chain (the child is that chain's last link so far)
                            ChainDesc& D = chd[cprev];
                            K.koff = D.ktot; D.ktot += K.k; D.nlinks++; D.tail = order_of(Sy, sn) - K.k; K.fi = cprev;
                            chain_of[sn] = cprev;
                        } else {
                            ChainDesc D{}; D.cvb = Sy.cv_off[sn]; D.nlinks = 1; D.ktot = K.k; D.tail = order_of(Sy, sn) - K.k; D.ch0 = Sy.child_ptr[sn]; D.ch1 = Sy.child_ptr[sn + 1];
                            D.alias0 = ac >= 0 ? 1 : 0; D.s0 = sn;
                            K.koff = 0; K.fi = (int)chd.size();
                            chain_of[sn] = (int)chd.size(); chd.push_back(D);
                        }
                        chl.push_back(K);
                    }
                sg.ndesc = (int)chd.size() - sg.desc0;
                {   // flatten: links chain by chain, bottom link first
                    std::vector<ChainLink> part(chl.begin() + chl0, chl.end());
                    std::stable_sort(part.begin(), part.end(), [](const ChainLink& x, const ChainLink& y) { return x.fi < y.fi; });
                    std::copy(part.begin(), part.end(), chl.begin() + chl0);
                    int cur = -1;
                    for (size_t t = chl0; t < chl.size(); ++t) { if (chl[t].fi != cur) { cur = chl[t].fi; chd[cur].link0 = (int)t; } }
                    for (size_t t = chl0; t < chl.size(); ++t) chl[t].fi = (int)t;
                }
                // workgroups: forward in chain order (children's chains first), backward in reverse (parents first)
                for (int d = sg.desc0; d < sg.desc0 + sg.ndesc; ++d) {
                    ChainDesc& D = chd[d];
                    const int nt = (D.tail + 63) / 64;
                    D.wg0f = sg.nwg_f; D.tf0 = P.ntailflags; P.ntailflags += nt;
                    for (int w = 0; w < D.nlinks + nt; ++w) wgf.push_back(d);
                    sg.nwg_f += D.nlinks + nt; sg.maxtail = std::max(sg.maxtail, D.tail);
                }
                for (int d = sg.desc0 + sg.ndesc - 1; d >= sg.desc0; --d) {      // per chain: its dot workgroups (256 rows beyond the chain x one link each), then its links
                    ChainDesc& D = chd[d];
                    const int nw = D.nlinks * ((D.tail + 255) / 256 + 1);
                    D.wg0b = sg.nwg_b; sg.nwg_b += nw;
                    D.dot0 = P.ndots; P.ndots += D.nlinks * ((D.tail + 255) / 256);
                    for (int w = 0; w < nw; ++w) wgb.push_back(d);
                }
                // what a chain waits for: forward, the rows beyond each child chain of its first link (all of them before anything is
                // gathered); backward, the bottom link of the chain its parent lives in
                for (int d = sg.desc0; d < sg.desc0 + sg.ndesc; ++d) {
                    ChainDesc& D = chd[d];
                    D.gw0 = (int)chwait.size();
                    bool gathers = false;
                    for (int q = D.ch0; q < D.ch1; ++q) {
                        const int c = Sy.child_idx[q];
                        if (c != Sy.alias_child[D.s0]) gathers = true;
                        if (Sy.sn_level[c] < lv || chain_of[c] < 0) continue;
                        const ChainDesc& X = chd[chain_of[c]];
                        for (int b = 0; b < (X.tail + 63) / 64; ++b) chwait.push_back(X.tf0 + b);
                    }
                    D.gw1 = (int)chwait.size();
                    // 0: the vector is in place (in-place link of a front below the segment), 1: fresh vector, nothing to gather, 2: gather step
                    D.init = (gathers || D.gw1 > D.gw0) ? 2 : (D.alias0 ? 0 : 1);
                    if (multi && D.init != 0) { P.error = "internal: chain segment with a gather in a distributed schedule"; fprintf(stderr, "[mi355x_kkt] %s\n", P.error.c_str()); return P; }
                    const int last = chl[D.link0 + D.nlinks - 1].s, par = Sy.sn_parent[last];
                    D.pw0 = (int)chwait.size();
                    if (par >= 0 && Sy.sn_level[par] <= e && chain_of[par] >= 0) { const ChainDesc& Q = chd[chain_of[par]]; for (int t = 0; t < Q.nlinks; ++t) chwait.push_back(Q.link0 + t); }
                    D.pw1 = (int)chwait.size();
                }
                P.seg_at_lv0[lv] = P.seg_at_lv1[e] = (int)P.chain_segs.size(); P.chain_segs.push_back(sg);
            }
            lv = e + 1;
        }
        if (in.verbose) { int nl = 0; for (auto& sg : P.chain_segs) nl += sg.lv1 - sg.lv0 + 1; fprintf(stderr, "[mi355x_kkt] data-flow solve sweeps: %d segments covering %d of %d levels, %d chains, %d links\n", (int)P.chain_segs.size(), nl, NL, (int)chd.size(), (int)chl.size()); }
    }
    std::vector<int> bigidx_of(NS, 0);
    for (int sn = 0; sn < NS; ++sn) if (Sy.sn_class[sn] == FC_BIG) bigidx_of[sn] = P.nbig++;
    // (multi-GPU: not for a front at a subtree join -- its square comes out of the all-reduced arena)
    auto selfasm = [&](int sn) { return (!multi || P.ex.aoff[sn] < 0) && in.selfasm && Sy.alias_child[sn] >= 0 && nchild(Sy, sn) == 1; };
    // chain-group tables: for every BIG front the links of its group up to and including itself
    std::vector<int> gbase_of(NS, 0), gcols_of(NS, 0);
    for (int sn = 0; sn < NS; ++sn) {
        gcols_of[sn] = cols_of(Sy, sn);
        if (Sy.sn_class[sn] != FC_BIG) continue;
        std::vector<int> links(Sy.grp_pos[sn] + 1);
        int cur = sn;
        for (int j = Sy.grp_pos[sn]; j >= 0; --j) { links[j] = cur; if (j > 0) cur = Sy.alias_child[cur]; }
        gbase_of[sn] = (int)P.gtab.size(); gcols_of[sn] = 0;
        for (int l : links) {
            GroupLink G;
            G.panel_off = P.panel_off[l]; G.wb = Sy.wb_off[l]; G.minv_off = Sy.minv_off[l]; G.cv = Sy.cv_off[l]; G.tr = P.ex.troff[l];
            G.c0 = Sy.sn_colptr[l]; G.k = cols_of(Sy, l); G.r0 = Sy.sn_rowptr[l]; G.m = order_of(Sy, l);
            G.ldp = Sy.sn_ldp[l]; G.ch0 = Sy.child_ptr[l]; G.ch1 = Sy.child_ptr[l + 1]; G.alias = Sy.alias_child[l] >= 0 ? 1 : 0;
            G.t_off = P.cb_off[l]; G.ldt = Sy.sn_ldt[l]; G.s = l; G.aq0 = Sy.acolptr[G.c0]; G.aq1 = Sy.acolptr[G.c0 + G.k]; G.bigidx = bigidx_of[l];
            G.selfasm = selfasm(l) ? 1 : 0;
            P.gtab.push_back(G); gcols_of[sn] += G.k;
        }
    }
    // look-ahead candidates: group-last BIG fronts (>= la_min_nt = 8 tile rows; 12 before part 1 had its 64 x 64 tiles) whose chain continues with a PURE next group (links
    // whose only child is the chain child: nothing but the chain itself writes into the front before the next full update)
    auto upd_rows = [&](int sn) { return order_of(Sy, sn) - cols_of(Sy, sn); };
    std::vector<char> split_of(NS, 0);
    P.la_tiles1.assign(NL, 0); P.la_tiles2.assign(NL, 0); P.la_full.assign(NL, 0);
    {
        std::vector<int> alias_parent(NS, -1);
        for (int sn = 0; sn < NS; ++sn) if (Sy.alias_child[sn] >= 0) alias_parent[Sy.alias_child[sn]] = sn;
        long long la_total = 0;      // part-2 tiles of the split updates
        int nsmall = 0, nend = 0, nimpure = 0, nfull = 0, nsplit = 0;
        for (int sn = 0; sn < NS; ++sn) {
            if (Sy.sn_class[sn] != FC_BIG) continue;
            const int lv = Sy.sn_level[sn];
            if (Sy.grp_rem[sn] != 0) { P.la_tiles1[lv] = std::max(P.la_tiles1[lv], schur_tiles(Sy, sn)); continue; }
            P.la_full[lv] = 1;
            const int nt = (upd_rows(sn) + 127) / 128;
            bool ok = in.lookahead && !multi && nt >= in.la_min_nt && alias_parent[sn] >= 0;
            for (int p = alias_parent[sn]; ok && p >= 0; p = alias_parent[p]) {
                if (nchild(Sy, p) != 1) ok = false;
                if (Sy.grp_rem[p] == 0) break;
            }
            split_of[sn] = ok ? 1 : 0;
            P.la_tiles1[lv] = std::max(P.la_tiles1[lv], ok ? 2 * nt - 1 : tri_tiles(nt));
            if (ok) { P.la_tiles2[lv] = std::max(P.la_tiles2[lv], ((nt - 2) * (nt - 1) / 2 + 7) / 8 * 8); la_total += (long long)(nt - 2) * (nt - 1) / 2; }
            ++nfull; nsplit += ok ? 1 : 0;
            if (!ok) { if (nt < in.la_min_nt) ++nsmall; else if (alias_parent[sn] < 0) ++nend; else ++nimpure; }
        }
        if (in.verbose)
            fprintf(stderr, "[mi355x_kkt] look-ahead: %d of %d group-end updates split (%lld part-2 tiles); not split: %d small, %d chain ends, %d impure next group\n",
                    nsplit, nfull, la_total, nsmall, nend, nimpure);
        // look-ahead costs the graph replay (see factor()): only worth it when a good part of the flops is in split updates
        P.la_any = la_total >= in.la_min_tiles && la_total > 0;
        if (!P.la_any) { std::fill(split_of.begin(), split_of.end(), 0); std::fill(P.la_tiles2.begin(), P.la_tiles2.end(), 0); std::fill(P.la_tiles1.begin(), P.la_tiles1.end(), 0); }
    }
    // XCD-aware tile orders for the large (>= 12 tile rows) full updates, one table per triangle size
    std::vector<int> ttab_of(NS, -1), ttab2_of(NS, -1);
    {
        std::map<int, int> tab_at;
        auto table_for = [&](int n) {
            auto it = tab_at.find(n);
            if (it != tab_at.end()) return it->second;
            const int at = (int)P.tile_tab.size(), S8 = 8, nst = (n + S8 - 1) / S8;
            for (int I = 0; I < nst; ++I) for (int J = 0; J <= I; ++J)
                for (int a = 0; a < S8; ++a) for (int b = 0; b < S8; ++b) {
                    const int ti = I * S8 + a, tc = J * S8 + b;
                    if (ti < n && tc <= ti) P.tile_tab.push_back((ti << 16) | tc);
                }
            tab_at[n] = at; return at;
        };
        for (int sn = 0; sn < NS; ++sn) if (in.xcd_tiles && Sy.sn_class[sn] == FC_BIG && Sy.grp_rem[sn] == 0) {
            const int nt = (upd_rows(sn) + 127) / 128;
            if (nt < 12) continue;
            ttab_of[sn] = table_for(nt);
            if (split_of[sn]) ttab2_of[sn] = table_for(nt - 2);
        }
    }
    // per level: every big front a pure in-place chain link (no assembly launch); every big front a chain link that is not the last of its group
    // (the narrow trailing updates ride in the fused pivot-block + panel-solve launch)
    P.lv_asm_skip.assign(NL, 0); P.lv_narrow_tiles.assign(NL, 0);
    for (int lv = 0; lv < NL && !multi; ++lv) {
        const int b0 = bucket0(lv, FC_BIG), b1 = bucket0(lv, FC_BIG + 1);
        bool pure = true, narrow = true; int tl = 0;
        for (int q = b0; q < b1; ++q) {
            const int sn = Sy.level_sn[q];
            if (!(Sy.alias_child[sn] >= 0 && nchild(Sy, sn) == 1)) pure = false;
            if (Sy.grp_rem[sn] <= 0) narrow = false;
            tl = std::max(tl, schur_tiles64(Sy, sn));
        }
        P.lv_asm_skip[lv] = (in.selfasm && b1 > b0 && pure) ? 1 : 0;
        P.lv_narrow_tiles[lv] = (in.fuse_upd && b1 > b0 && narrow) ? tl : 0;
    }
    // ---- grouped schedule: every chain group is factored at the level of its first link (k_grp_fused + update) ----
    // (an in-place chain never crosses an ownership boundary -- symbolic.cpp only aliases fronts of one owner and one range of ranks -- so neither does a group)
    P.grouped = Sy.maxsupernode <= 64 && in.selfasm && in.grouped;
    auto build_groups = [&](GrpSched& G, int which) {
        for (auto* v : {&G.g0, &G.g1, &G.split, &G.nrb, &G.tiles64, &G.tiles, &G.la1, &G.la2, &G.p1t, &G.la3, &G.nsplit}) v->assign(NL, 0);
        if (!P.grouped) return;
        std::vector<std::vector<int>> at(NL);
        for (int sn = 0; sn < NS; ++sn) if (Sy.sn_class[sn] == FC_BIG && Sy.grp_rem[sn] == 0 && in_sched(which, sn)) {
            int first = sn;
            for (int j = Sy.grp_pos[sn]; j > 0; --j) first = Sy.alias_child[first];
            if (Sy.sn_level[first] >= Sy.grp_cut_level) at[Sy.sn_level[first]].push_back(sn);      // (groups do not straddle the cut: symbolic.cpp)
        }
        int ng = 0;
        for (int lv = 0; lv < NL; ++lv) {
            std::stable_sort(at[lv].begin(), at[lv].end(), [&](int a, int b) { return order_of(Sy, a) < order_of(Sy, b); });
            G.g0[lv] = (int)L.size();
            int nsmall = 0;
            for (int sn : at[lv]) {
                L.push_back(sn); ++ng;
                const int mu = upd_rows(sn), nt = (mu + 127) / 128;
                G.nrb[lv] = std::max(G.nrb[lv], (mu + 63) / 64);
                if (order_of(Sy, sn) <= 1024) { ++nsmall; G.tiles64[lv] = std::max(G.tiles64[lv], schur_tiles64(Sy, sn)); continue; }
                G.tiles[lv] = std::max(G.tiles[lv], schur_tiles(Sy, sn));
                G.la1[lv] = std::max(G.la1[lv], split_of[sn] ? 2 * nt - 1 : tri_tiles(nt));
                if (split_of[sn]) {
                    G.la2[lv] = std::max(G.la2[lv], ((nt - 2) * (nt - 1) / 2 + 7) / 8 * 8);
                    const int n64 = (mu + 63) / 64; int c = 0; for (int tc = 0; tc < 4 && tc < n64; ++tc) c += n64 - tc; G.p1t[lv] = std::max(G.p1t[lv], c); ++G.nsplit[lv];
                } else G.la3[lv] = std::max(G.la3[lv], tri_tiles(nt));
            }
            G.split[lv] = nsmall; G.g1[lv] = (int)L.size();
        }
        if (in.verbose) fprintf(stderr, "[mi355x_kkt] grouped schedule%s: %d chain groups factored in one launch each (tree levels >= %d)\n",
                                which == 0 ? "" : (which == 1 ? " (own subtrees)" : " (replicated fronts of one exchange step)"), ng, Sy.grp_cut_level);
    };
    P.grp.assign(multi ? 1 + P.ndepth : 1, GrpSched());
    for (size_t i = 0; i < P.grp.size(); ++i) build_groups(P.grp[i], multi ? 1 + (int)i : 0);
    // tfuse: the contribution block of a front is formed by its trailing update (T = sum of the children's contributions - L21 W21^T, written once) instead of
    // being assembled, read back and written again.  A front that is a unit of its own -- assembled (not in place on a child), its update one launch of
    // k_big_schur64 / k_big_schur -- or (round 5) a whole CHAIN GROUP whose first link is assembled: that link's assembly stops at the group's columns
    // (asmcut: the panels of all the group's links), the trailing block of the LAST link is formed by the group-end update out of the FIRST link's children.
    std::vector<char> tfuse_of(NS, 0);
    std::vector<int> asmcut_of(NS, 0);
    if (!multi && in.tfuse)
        for (int sn = 0; sn < NS; ++sn) {
            if (Sy.sn_class[sn] != FC_BIG || Sy.grp_rem[sn] != 0) continue;      // (the last link of its group, or a front of its own)
            int first = sn;
            for (int j = 0; j < Sy.grp_pos[sn]; ++j) first = Sy.alias_child[first];
            if (Sy.alias_child[first] >= 0 || upd_rows(sn) <= 0 || nchild(Sy, first) > 96) continue;
            tfuse_of[sn] = 1; ++P.ntfuse;
            asmcut_of[first] = order_of(Sy, first) - upd_rows(sn);      // (= k of a front of its own, the group's columns otherwise)
        }
    if (in.verbose) fprintf(stderr, "[mi355x_kkt] contribution blocks formed by their update (not assembled): %d of %d big fronts\n", P.ntfuse, Sy.num_big);
    P.fmeta.resize(L.size()); P.asm_fast_ok.assign(L.size(), 0); P.asmcut.assign(L.size(), 0);
    for (size_t q = 0; q < L.size(); ++q) {
        const int sn = L[q];
        FrontMeta& M = P.fmeta[q];
        int nside = 0;      // children that are not the chain child
        for (int c = Sy.child_ptr[sn]; c < Sy.child_ptr[sn + 1]; ++c) if (Sy.child_idx[c] != Sy.alias_child[sn]) ++nside;
        // (the number of children the front brings to k_big_assemble2's row maps -- a front with more than ASM_MAXCH falls back to the column routine
        // inside the kernel; 0: not for that kernel; a pure in-place link has nothing to assemble either way)
        P.asm_fast_ok[q] = (Sy.alias_child[sn] >= 0 && nside == 0) ? 1 : (Sy.alias_child[sn] < 0 ? (nside <= 6 ? std::max(nside, 1) : 0) : 0);
        M.tfuse = tfuse_of[sn]; M.asmcut = asmcut_of[sn];
        M.s = sn; M.c0 = Sy.sn_colptr[sn]; M.k = cols_of(Sy, sn); M.r0 = Sy.sn_rowptr[sn]; M.m = order_of(Sy, sn);
        M.aq0 = Sy.acolptr[M.c0]; M.aq1 = Sy.acolptr[M.c0 + M.k]; M.ch0 = Sy.child_ptr[sn]; M.ch1 = Sy.child_ptr[sn + 1]; M.alias = Sy.alias_child[sn] >= 0 ? 1 : 0;
        M.ldp = Sy.sn_ldp[sn]; M.ldt = Sy.sn_ldt[sn];
        M.panel_off = P.panel_off[sn]; M.cb_off = P.cb_off[sn]; M.minv_off = Sy.minv_off[sn];
        M.cv = Sy.cv_off[sn]; M.wb = Sy.wb_off[sn]; M.gpart = Sy.gpart_off[sn];
        M.gbase = gbase_of[sn]; M.gpos = Sy.grp_pos[sn]; M.grem = Sy.grp_rem[sn]; M.gcols = gcols_of[sn]; M.split = split_of[sn]; M.ttab = ttab_of[sn]; M.ttab2 = ttab2_of[sn];
        M.selfasm = (Sy.sn_class[sn] == FC_BIG && selfasm(sn)) ? 1 : 0; M.bigidx = bigidx_of[sn];
        // 1: in-place chain link whose only child is the chain child, 2: no children at all => the fused forward kernel applies
        M.solo = (Sy.alias_child[sn] >= 0 && nchild(Sy, sn) == 1) ? 1 : ((Sy.alias_child[sn] < 0 && nchild(Sy, sn) == 0) ? 2 : 0);
        P.asmcut[q] = (M.selfasm && !M.asmcut) ? -1 : M.asmcut;
        if (q < solve_entry.size() && solve_entry[q] && !Sy.solve_group) {     // per-link solves: every front is its own unit
            M.gbase += M.gpos; M.gpos = 0; M.grem = 0; M.gcols = M.k;
        }
    }
    // ChildMeta::owner as the kernels read it: -1 = assembled directly by the parent (same owner / same range of ranks); otherwise the child
    // reaches its (replicated) parent through the arena and the value says who reports it and in which exchange step: reporting rank
    // + nranks * (0 for an owned subtree root, 1 + depth for a front of a sub-range) -- the `who` of k_arena_assemble / k_top_rhs_assemble
    auto child_code = [&](int ch) {
        const int pa = Sy.sn_parent[ch];
        if (!multi || pa < 0 || Sy.sn_owner[pa] >= 0 || Sy.sn_owner[ch] >= 0) return Sy.sn_owner[ch];
        if (same_range(Sy, ch, pa)) return -1;
        return Sy.sn_glo[ch] + std::max(1, in.nranks) * (1 + Sy.sn_gdepth[ch]);
    };
    auto& cm = P.cmeta;
    cm.resize(Sy.child_idx.size());
    for (size_t q = 0; q < cm.size(); ++q) {
        const int ch = Sy.child_idx[q]; const int kc = cols_of(Sy, ch);
        cm[q].ch = ch; cm[q].relbase = Sy.sn_rowptr[ch] + kc; cm[q].mc = Sy.sn_rowptr[ch + 1] - cm[q].relbase;
        cm[q].owner = child_code(ch); cm[q].cb_off = P.cb_off[ch]; cm[q].ldt = Sy.sn_ldt[ch]; cm[q].aliased = 0; cm[q].cvbase = Sy.cv_off[ch] + kc;
        cm[q].rlo = cm[q].mc > 0 ? Sy.rel[cm[q].relbase] : (1 << 30); cm[q].rhi = cm[q].mc > 0 ? Sy.rel[cm[q].relbase + cm[q].mc - 1] : -1;      // (rel is ascending)
        cm[q].inv = 0;
    }
    // inverse relative indices for the children of BIG parents (k_big_assemble: one load instead of a binary search per column)
    for (int sn = 0; sn < NS; ++sn) {
        if (Sy.alias_child[sn] >= 0)
            for (int q = Sy.child_ptr[sn]; q < Sy.child_ptr[sn + 1]; ++q) if (Sy.child_idx[q] == Sy.alias_child[sn]) cm[q].aliased = 1;
        if (Sy.sn_class[sn] != FC_BIG && !(sn < (int)P.in_seg.size() && P.in_seg[sn])) continue;
        for (int q = Sy.child_ptr[sn]; q < Sy.child_ptr[sn + 1]; ++q) {
            if (cm[q].aliased) continue;
            cm[q].inv = (long long)P.relinv.size();
            P.relinv.resize(P.relinv.size() + order_of(Sy, sn), -1);
            int* inv = P.relinv.data() + cm[q].inv;
            for (int a = 0; a < cm[q].mc; ++a) inv[Sy.rel[cm[q].relbase + a]] = a;
        }
    }
    // leaf chains (k_leaf_chain): the levels below lc_levels hold nothing but fronts of order <= 16 with at most one child -- every such front is a
    // link of the chain that starts at its leaf
    std::vector<int> lcf;
    if (!multi && in.fastpiv && in.leafchain) {
        int LC = 0;
        for (; LC < NL && LC < 16; ++LC) {
            bool okl = bucket0(LC, FC_WAVE + 1) == bucket0(LC, FC_COUNT);      // (no front of another class)
            for (int q = bucket0(LC, FC_WAVE); q < bucket0(LC, FC_WAVE + 1) && okl; ++q)
                if (order_of(Sy, L[q]) > 16 || nchild(Sy, L[q]) > 1) okl = false;
            if (!okl || bucket0(LC, FC_WAVE + 1) == bucket0(LC, FC_WAVE)) break;
        }
        if (LC >= 2) {
            P.lc_levels = LC;
            std::vector<int> fmw(NS, -1);
            for (int q = bucket0(0, FC_WAVE); q < bucket0(LC - 1, FC_WAVE + 1); ++q) fmw[L[q]] = q;
            P.lc_ptr.push_back(0);
            for (int q = bucket0(0, FC_WAVE); q < bucket0(0, FC_WAVE + 1); ++q) {
                for (int cur = L[q]; cur >= 0 && Sy.sn_level[cur] < LC; cur = Sy.sn_parent[cur]) lcf.push_back(fmw[cur]);
                P.lc_ptr.push_back((int)lcf.size());
            }
            P.lc_nchains = (int)P.lc_ptr.size() - 1;
            if ((int)lcf.size() != bucket0(LC - 1, FC_WAVE + 1) - bucket0(0, FC_WAVE)) { P.lc_levels = 0; P.lc_nchains = 0; }   // (cannot happen: every front below LC is on exactly one chain)
            if (in.verbose && P.lc_levels) fprintf(stderr, "[mi355x_kkt] leaf chains: %d chains over the bottom %d levels (%zu fronts) in one launch per sweep\n", P.lc_nchains, P.lc_levels, lcf.size());
        }
    }
    if (P.lc_ptr.empty()) P.lc_ptr.push_back(0);
    for (int q : lcf) {
        const FrontMeta& M = P.fmeta[q]; LeafLink K;
        K.s = M.s; K.c0 = M.c0; K.k = M.k; K.m = M.m; K.aq0 = M.aq0; K.aq1 = M.aq1; K.ldp = M.ldp; K.r0 = M.r0; K.pad = 0;
        K.relbase = M.r0 + M.k;                                  // (V.rel + relbase: where the front's update rows sit in its parent)
        K.panel_off = M.panel_off; K.minv_off = M.minv_off; K.cb_off = M.cb_off; K.cv = M.cv;
        P.lc_link.push_back(K);
    }
    if (P.lc_link.empty()) P.lc_link.push_back(LeafLink());
    // k_front_df: maximal runs of >= 2 consecutive levels (above the leaf chains) whose fronts are all one-wavefront fronts
    P.df_run_at.assign(NL, -1); P.cbt_off.assign(std::max(NS, 1), -1);
    std::vector<int> run_of(std::max(NS, 1), -1);
    if (!multi && in.fastpiv && in.front_df) {
        auto pure = [&](int lv) { return bucket0(lv, FC_WAVE + 1) > bucket0(lv, FC_WAVE) && bucket0(lv, FC_WAVE + 1) - bucket0(lv, FC_WAVE) == bucket0(lv, FC_COUNT) - bucket0(lv, 0); };
        for (int lv = P.lc_levels; lv < NL; ) {
            if (!pure(lv)) { ++lv; continue; }
            int e = lv; while (e + 1 < NL && pure(e + 1)) ++e;
            if (e > lv) {
                DfRun R{lv, e, (int)P.df_tab.size(), e - lv + 1, 0};
                for (int l = lv; l <= e; ++l) {
                    const int w0 = bucket0(l, FC_WAVE), w1 = bucket0(l, FC_WAVE + 1);
                    P.df_tab.push_back(DfLevel{w0, P.tiny16[l], w1 - w0, R.nq});
                    R.nq += (P.tiny16[l] + 3) / 4 + (w1 - w0 - P.tiny16[l]);
                    for (int q = w0; q < w1; ++q) run_of[L[q]] = (int)P.df_runs.size();
                }
                P.df_run_at[lv] = (int)P.df_runs.size(); P.df_runs.push_back(R);
            }
            lv = e + 1;
        }
    }
    // tagged contribution blocks: for every front of a run whose PARENT is a front of the same run
    for (int sn = 0; sn < NS; ++sn) {
        const int pa = Sy.sn_parent[sn];
        if (run_of[sn] < 0 || pa < 0 || run_of[pa] != run_of[sn] || upd_rows(sn) <= 0) continue;
        P.cbt_off[sn] = P.cbt_len; P.cbt_len += upd_rows(sn) <= 16 ? 256 : 1024;
    }
    if (P.df_tab.empty()) P.df_tab.push_back(DfLevel{0, 0, 0, 0});
    // the inertia / pivot counts are summed over the ranks: a replicated front is counted by the first rank of its range (-1 in this rank's view), -3 = not here
    P.stat_owner.assign(Sy.sn_owner.begin(), Sy.sn_owner.end());
    if (multi) for (int sn = 0; sn < NS; ++sn) if (Sy.sn_owner[sn] < 0) P.stat_owner[sn] = Sy.sn_glo[sn] == in.rank ? -1 : -3;
    // exact LDS need of the register-tiled front kernel per (level, class) bucket
    P.reg_lds.assign((size_t)NL * FC_COUNT, 0);
    for (int s = 0; s < NS; ++s) {
        size_t& r = P.reg_lds[(size_t)Sy.sn_level[s] * FC_COUNT + Sy.sn_class[s]];
        r = std::max(r, front_lds(order_of(Sy, s), cols_of(Sy, s), Sy.sn_class[s] == FC_WAVE ? 32 : (Sy.sn_class[s] == FC_LDS64 ? 64 : 128)));
    }
    return P;
}

// ---- the factor schedule: which kernel runs, with what grid, LDS size, stream and stream order -- every condition of the factorisation's launches
//      once, here (DESIGN.md "Where a launch is decided"); numeric.hip run_factor_list walks the list ----
std::vector<FactorLaunch> build_factor_schedule(const LaunchPlan& P, const Symbolic& Sy, const PlanInputs& in, int which, bool optimistic)
{
    std::vector<FactorLaunch> out;
    const Sched& sc = which == 0 ? P.single : which == 1 ? P.local : P.stage[which - 2];
    if (sc.ptr.empty()) return out;                      // (a schedule this plan does not have: the multi-rank ones of a single-GPU plan)
    const int NL = P.nlevels;
    const bool sg = which == 0;                          // single-GPU schedule: the buckets are sorted by order; leaf chains, data-flow runs, side stream
    const bool multi = in.multi, single = sg && !multi;
    const int top_mode = which >= 2 ? 1 : 0;             // the replicated fronts of an exchange step
    const int gi = top_mode ? 1 + (which - 2) : 0;       // the grouped schedule P.grp[gi] (the multi-GPU schedules have their own group lists)
    int fork_ev = -1, fork_lv = -1;                      // the look-ahead fork that no join has waited for yet: its events (a[0], lv)
    auto bucket0 = [&](int lv, int fc) { return sc.base + sc.ptr[(size_t)lv * FC_COUNT + fc]; };      // bucket (lv, fc) of sc is [bucket0(lv, fc), bucket0(lv, fc + 1)) of the launch list
    auto put = [&](int op, int strm, int kind, int lv, int b0, int gx, int gy, int block, size_t lds, int a0 = 0, int a1 = 0, int a2 = 0, int a3 = 0) {
        out.push_back(FactorLaunch{op, strm, kind, gx, gy, block, lv, b0, (int)lds, {a0, a1, a2, a3}}); };
    // The look-ahead fork, behind part 1 on the main stream: A recorded there, part 2 of the fronts [b0, b0 + nb) on the second stream behind A (128 x 128
    // tiles on 16 wavefronts, or quarter tiles on 4 wavefronts that fit on the CUs a k_grp_fused workgroup occupies: kernels_big.hip.inc k_big_schur_q / _w),
    // B recorded behind it -- what join() makes the main stream wait for before a later launch may touch what part 2 reads or writes
    auto fork = [&](int ev, int lv, int b0, int nb, int ntiles) {
        const int nvirt = ((ntiles + 7) / 8) * 32;
        const int wgs = (int)std::min<long long>(nvirt, 4ll * in.la_wgs);
        put(FO_FORK, FS_MAIN, -1, lv, b0, 1, 1, 0, 0, ev);
        put(FO_SCHUR_Q, FS_LOOKAHEAD, KK_BIG_SCHUR, lv, b0, wgs, nb, 256, 0, ntiles);
        put(FO_FORK_DONE, FS_LOOKAHEAD, -1, lv, b0, 1, 1, 0, 0, ev);
        fork_ev = ev; fork_lv = lv;
    };
    auto join = [&](int lv) { if (fork_ev >= 0) { put(FO_JOIN, FS_MAIN, -1, lv, 0, 1, 1, 0, 0, fork_ev, fork_lv); fork_ev = -1; } };      // (a[1]: the level of the fork; lv: where the join stands)
    // The column-chunk kernel pays where a level is MANY fronts of a few hundred rows (short columns: the one-wavefront-per-column kernel runs at the
    // latency of its load chain there) and every front can take its fast path (at most ASM_MAXCH children to pull, not an in-place link with other
    // children, no arena): measured 4.1 -> 2.0 ms per factorisation on synth_1e6, but 3.4 -> 8.7 ms on MBndryCntrl_3D 30, whose levels are a
    // handful of fronts of ~1000 rows with a dozen children each -- there the column kernel has four times the workgroups and no preamble.
    auto assemble = [&](int strm, int lv, int mm, int nfronts, int b0) {
        const int ldi = (mm + 15) & ~15;                    // the children's inverse row maps of one front in LDS: ASM_MAXCH x ldi ints (78 KiB at the largest front of synth_1e6)
        // (... which has to FIT: a level of >= 32 fast-path fronts whose largest order exceeds ~6 780 -- a 3-D problem, or fronts enlarged by a
        // delayed-pivot edit -- would make the launch fail instead of falling back to the column kernel: ADVICE r04)
        // Round 5: a front whose contribution block is formed by its update (asmcut) has only its panel columns assembled; a launch of such fronts has no
        // workgroups behind the largest asmcut.  (MI355X_KKT_ASM2_WIDE: this kernel also for levels of a few dozen fronts with up to ASM_MAXCH = 16 children each
        // once only their panel columns are assembled -- the MBndryCntrl_3D family; measured slower there than the column kernel, 7.65 against 7.16 ms.)
        bool v2 = !top_mode;
        int maxch = 1, ncut = 0, cutmax = 0;
        for (int q = b0; q < b0 + nfronts && v2; ++q) { v2 = P.asm_fast_ok[q] != 0; maxch = std::max(maxch, (int)P.asm_fast_ok[q]); if (P.asmcut[q]) { ++ncut; cutmax = std::max(cutmax, P.asmcut[q] > 0 ? P.asmcut[q] : 0); } }
        v2 = v2 && (size_t)maxch * ldi * sizeof(int) <= (size_t)158 * 1024 && (nfronts >= 32 && maxch <= 6);
        if (!v2) { put(FO_ASSEMBLE, strm, KK_BIG_ASSEMBLE, lv, b0, (mm + 3) / 4, nfronts, 256, 0, top_mode); return; }
        const int ncols = (ncut == nfronts) ? std::min(mm, cutmax) : mm;      // (every front stops at its asmcut: no workgroups for the columns behind the largest of them)
        if (ncols <= 0) return;                                               // (every front of the list has its whole block formed by its update: nothing to assemble -- a grid of 0 workgroups is refused by the runtime, met on the multi-rank schedule)
        put(FO_ASSEMBLE2, strm, KK_BIG_ASSEMBLE, lv, b0, ncols, nfronts, 256, (size_t)maxch * ldi * sizeof(int), top_mode, ldi, maxch);
    };
    // the chain groups whose first link sits on level lv: pivot blocks + leading blocks, rows below, rank-(<= 256) updates
    auto groups = [&](int strm, int lv) {
        const GrpSched& G = P.grp[gi];
        const int b0 = G.g0[lv], b1 = G.g1[lv], bs = b0 + G.split[lv];
        if (b1 == b0) return;
        {
            // as many 64-row blocks per row-block workgroup as it takes for the launch to fit the chip (one workgroup per CU)
            int rbw = 1;
            while (rbw < in.grp_rbw_max && (b1 - b0) * (4 + (G.nrb[lv] + rbw - 1) / rbw) > 256) rbw *= 2;
            const int nrbw = (G.nrb[lv] + rbw - 1) / rbw;
            const int st = ((b1 - b0) * (4 + nrbw) <= 256) ? 1 : 0;
            put(FO_GRP_FUSED, strm, KK_BIG_DIAG, lv, b0, b1 - b0, 4 + nrbw, 256, 0, st, rbw);
        }
        if (bs > b0 && G.tiles64[lv] > 0) put(FO_SCHUR64, strm, KK_BIG_SCHUR, lv, b0, G.tiles64[lv], bs - b0, 256, 0);
        if (b1 == bs) return;
        const int nb = b1 - bs;
        join(lv);      // a full update may touch what an earlier part 2 is still writing
        if (G.la2[lv] > 0) {      // (also while profile() records its events: the per-kernel times are those of the TIMED schedule, look-ahead stream included)
            // part 1 in 64 x 64 tiles where the 128 x 128 ones would leave most of the chip idle (k_big_schur_p1); the fronts of the list that are not split
            // get their whole update from a launch of their own then
            if (in.p1_small && G.la1[lv] * nb <= 512) {
                put(FO_SCHUR_P1, strm, KK_BIG_SCHUR, lv, bs, G.p1t[lv], nb, 1024, 0);
                if (G.nsplit[lv] < nb) put(FO_SCHUR, strm, KK_BIG_SCHUR, lv, bs, G.la3[lv], nb, 0, 0, 4);
            } else put(FO_SCHUR, strm, KK_BIG_SCHUR, lv, bs, G.la1[lv], nb, 0, 0, 1);
            fork(1 + gi, lv, bs, nb, G.la2[lv]);
        } else if (G.tiles[lv] > 0) put(FO_SCHUR, strm, KK_BIG_SCHUR, lv, bs, G.tiles[lv], nb, 0, 0, 0);
    };
    // the big-front launches of one level: assembly, pivot blocks and TRSM over the whole list [b0, b1); the trailing update with
    // 64 x 64 tiles / 256 threads on the fronts [b0, bs) of order <= 1024 (a handful of tiles, K = 16..64 each) and with
    // 128 x 128 tiles / 1024 threads on [bs, b1)
    auto big = [&](int strm, int lv, int b0, int bs, int b1, int mm, int kk, int tiles_small, int tiles) {
        const int nball = b1 - b0;
        if (!(single && P.lv_asm_skip[lv])) assemble(strm, lv, mm, nball, b0);
        const int nrb = (mm + 63) / 64;
        if (in.fuse_dt && (single || multi) && kk <= 64 && nball * (1 + nrb) <= in.fuse_dt_maxwg) {      // (multi-GPU: local subtrees and replicated top alike; the per-kernel profile books the fused launch under the pivot blocks)
            // few fronts on the level: pivot block + panel solve in one flag-synchronised launch (k_big_diag_trsm)
            const int ntu = (P.lv_narrow_tiles[lv] > 0 && nball * (1 + nrb + P.lv_narrow_tiles[lv]) <= 256) ? P.lv_narrow_tiles[lv] : 0;      // (one workgroup per CU: the far part of a group-end update may own the rest of the chip)
            put(FO_DIAG_TRSM, strm, KK_BIG_DIAG, lv, b0, nball, 1 + nrb + ntu, 256, 0, nrb, kk);
            if (ntu > 0) return;         // ... and so did the narrow updates
        } else if (kk <= 64) {
            put(FO_DIAG_REG, strm, KK_BIG_DIAG, lv, b0, nball, 1, 256, 0, kk);
            put(FO_TRSM, strm, KK_BIG_TRSM, lv, b0, (mm + 63) / 64, nball, 256, 0, kk);
        } else {
            put(FO_DIAG_REG_1024, strm, KK_BIG_DIAG, lv, b0, nball, 1, 1024, 0, kk);
            put(FO_TRSM_WIDE, strm, KK_BIG_TRSM, lv, b0, (mm + 63) / 64, nball, 256, 0, kk);
        }
        if (bs > b0 && tiles_small > 0) put(FO_SCHUR64, strm, KK_BIG_SCHUR, lv, b0, tiles_small, bs - b0, 256, 0);
        if (b1 == bs) return;
        const int nb = b1 - bs;
        if (single && P.la_full[lv]) join(lv);       // a full update may touch what an earlier part 2 is still writing
        if (single && P.la_tiles2[lv] > 0) {
            put(FO_SCHUR, strm, KK_BIG_SCHUR, lv, bs, P.la_tiles1[lv], nb, 0, 0, 1);
            fork(0, lv, bs, nb, P.la_tiles2[lv]);
        } else if (tiles > 0) put(FO_SCHUR, strm, KK_BIG_SCHUR, lv, bs, tiles, nb, 0, 0, 0);
    };
    // one (level, class) bucket of fronts
    auto bucket = [&](int strm, int lv, int fc) {
        const int b0 = bucket0(lv, fc), b1 = bucket0(lv, fc + 1), nb = b1 - b0;
        if (nb == 0) return;
        const size_t rl = P.reg_lds[(size_t)lv * FC_COUNT + fc];
        if (fc == FC_WAVE) {
            const int nt = sg ? P.tiny_split[lv] : 0;
            int fl = top_mode;
            if (in.fastpiv && P.wave_mmin[lv] <= 16) {      // fronts of order <= 16: four per wavefront on the static-order path first; what it accepts is skipped below
                const int n16 = sg ? P.tiny16[lv] : nb;
                // (the kernel raises qstat[4] for a front it rejects only when NO strict launch follows -- optimistic && n16 == nb: behind a strict
                // launch the rejected front is simply the strict kernel's, and raising the flag there made factor() repeat the whole factorisation
                // with the full schedule and drop the optimistic one for the life of the handle: ADVICE r04)
                if (n16 > 0) { put(FO_FRONT_DPP16, strm, KK_FRONT_WAVE, lv, b0, (n16 + 3) / 4, 1, 64, 0, n16, top_mode, (optimistic && n16 == nb) ? 1 : 0); fl |= 2; }
                // OPTIMISTIC schedule: every front of the bucket has order <= 16 and the static-order kernel accepts (nearly) everything it is given
                // (LukVlE1 10^6: all 164 000 fronts) -- the strict launch behind it would find nothing to do, 4-8 us each, 21 of them per
                // factorisation.  It is left out; a front the kernel rejects raises qstat[4] and factor() runs the full schedule again.
                if (optimistic && n16 == nb) return;
            }
            if (nt > 0) put(FO_REG_64_2, strm, KK_FRONT_WAVE, lv, b0, nt, 1, 64, rl, fl);
            if (nb - nt > 0) put(FO_REG_64_4, strm, KK_FRONT_WAVE, lv, b0 + nt, nb - nt, 1, 64, rl, fl);
        } else if (fc == FC_LDS64) {
            put(FO_REG_64_8, strm, KK_FRONT_LDS64, lv, b0, nb, 1, 64, rl, top_mode);
        } else if (fc == FC_LDS128) {
            const int nm = sg ? P.mid_split[lv] : 0;
            const int fl = top_mode | (in.fastpiv ? 2 : 0);
            // (measured and not kept, r05: in the optimistic schedule the strict launch only on the fronts with > 16 pivots and on a device-built list of
            // the fronts the static-order launch rejected -- 342 of them on synth_1e6 -- instead of the whole bucket: 18.21 against 18.16 ms.  The
            // 60-150 us of the strict launches are those fronts' own latency chains, not the workgroups that find nothing to do.)
            if (in.fastpiv) {      // fronts with <= 16 pivots: static-order path first; what it accepts is skipped by the launch behind it
                // (<256, 6, true> cut to 128 VGPRs = 4 workgroups per CU: 2.24 -> 2.13 ms of front_lds128 on synth_1e6; the same cut of <256, 8, true> gained nothing and is gone)
                if (nm > 0) put(FO_REG_256_6_FAST4, strm, KK_FRONT_LDS128, lv, b0, nm, 1, 256, P.mid_lds[lv], top_mode);
                if (nb - nm > 0) put(FO_REG_256_8_FAST, strm, KK_FRONT_LDS128, lv, b0 + nm, nb - nm, 1, 256, rl, top_mode);
            }
            if (nm > 0) put(FO_REG_256_6, strm, KK_FRONT_LDS128, lv, b0, nm, 1, 256, P.mid_lds[lv], fl);
            if (nb - nm > 0) put(FO_REG_256_8, strm, KK_FRONT_LDS128, lv, b0 + nm, nb - nm, 1, 256, rl, fl);
        } else {
            const int mm = sc.maxm[lv], kk = sc.maxk[lv];
            if ((single || multi) && P.grouped && lv >= Sy.grp_cut_level) {
                // the chain groups whose first link sits on this level, one launch each
                if (!(single && P.lv_asm_skip[lv])) assemble(strm, lv, mm, nb, b0);
                groups(strm, lv);
            } else if (!single) { const bool sm = mm <= 640; big(strm, lv, b0, sm ? b1 : b0, b1, mm, kk, sm ? sc.tiles64[lv] : 0, sm ? 0 : sc.tiles[lv]); }
            else big(strm, lv, b0, b0 + P.big_split[lv], b1, mm, kk, P.part_tiles[0][lv], P.part_tiles[1][lv]);
        }
    };
    const int lc = (sg && optimistic && P.lc_levels > 0) ? P.lc_levels : 0;      // the leaf chains: one launch for their levels (optimistic schedule only: no strict kernel behind it)
    if (lc > 0) put(FO_LEAF_CHAIN, FS_MAIN, KK_FRONT_WAVE, 0, bucket0(0, FC_WAVE), (P.lc_nchains + 3) / 4, 1, 64, 0, P.lc_nchains, lc - 1);
    for (int lv = lc; lv < NL; ++lv) {
        if (sg && optimistic && P.df_run_at[lv] >= 0) {      // a run of levels of one-wavefront fronts: one persistent data-flow launch (optimistic schedule only: no strict kernels behind it)
            const DfRun& R = P.df_runs[P.df_run_at[lv]];
            put(FO_FRONT_DF, FS_MAIN, KK_FRONT_WAVE, lv, bucket0(lv, FC_WAVE), R.nq, 1, 64, 0, R.tab0, R.nlev, R.nq, R.lv1);
            lv = R.lv1; continue;
        }
        // recycled contribution blocks (symbolic.cpp step 12a): whatever earlier levels put on the look-ahead streams is through before a level >= lv may
        // write into the space of a block they read.  (The runs above and the leaf-chain prefix skip this join: ADVICE.md item 1.)
        if (sg && Sy.cb_window > 0 && lv % Sy.cb_window == 0) join(lv);
        int lvl_fronts = 0, lvl_max = 0;
        for (int fc = 0; fc < FC_COUNT; ++fc) { const int nb = bucket0(lv, fc + 1) - bucket0(lv, fc); lvl_fronts += nb; lvl_max = std::max(lvl_max, nb); }
        bool side_open = false;
        for (int fc = 0; fc < FC_COUNT; ++fc) {
            const int nb = bucket0(lv, fc + 1) - bucket0(lv, fc);
            if (nb == 0) continue;
            // A handful of small fronts on a level whose bulk is elsewhere (synth_1e6: 3 fronts of order <= 128 next to 2 045 big ones; one front of order <= 64
            // next to 943 of order <= 128) is a launch of 1-3 workgroups running their strict pivot loops for 40-90 us with the chip idle.  The buckets of one
            // level are independent: in the eager (multi-stream) schedule such a bucket goes to the side stream, next to the level's main launches.
            // (the eager schedule only: a multi-stream hipGraph is what factor_once() avoids; not next to the three-stream chain look-ahead)
            const bool side = sg && in.side_small && P.la_any && !multi && fc != FC_BIG && nb <= SIDE_MAX_FRONTS && lvl_max >= 8 * nb && lvl_fronts > nb;
            if (side && !side_open) { put(FO_SIDE_OPEN, FS_MAIN, -1, lv, 0, 1, 1, 0, 0); side_open = true; }      // behind the level below
            bucket(side ? FS_SIDE : FS_MAIN, lv, fc);
        }
        if (side_open) put(FO_SIDE_CLOSE, FS_SIDE, -1, lv, 0, 1, 1, 0, 0);      // the level above reads what they wrote
    }
    join(NL);      // (no fork outlives its list: the multi-rank schedules never fork -- build_launch_plan splits no update there -- and the single-GPU one ends here)
    return out;
}

// ---- the solve-block schedule: the launches of one block of right-hand sides (launch_plan.h SolveBlockKind).  level() is numeric.hip solve_level for the
//      single-GPU schedule (top_mode 0), walk() the level loop of solve_sweep over [lv_lo, lv_hi) with its chain segments ----
SolveBlockSchedule build_solve_block_schedule(const LaunchPlan& P, const Symbolic& Sy, const PlanInputs& in)
{
    SolveBlockSchedule B;
    const Sched& sc = P.single;
    const int NL = P.nlevels;
    if (in.multi || sc.ptr.empty()) { B.first_top_level = NL; return B; }
    auto bucket0 = [&](int lv, int fc) { return sc.base + sc.ptr[(size_t)lv * FC_COUNT + fc]; };
    auto put = [&](int op, int sb, int kind, int lv, int b0, int gx, int gy, int block, size_t lds, int a0 = 0) {
        B.rec.push_back(FactorLaunch{op, sb, kind, gx, gy, block, lv, b0, (int)lds, {a0, 0, 0, 0}}); };
    auto lds_solve = [](int mmax, int kmax) { return (size_t)(mmax + 3 * kmax) * sizeof(double) + 16; };
    const bool pair = P.pair_solve, mid = in.mid_solve && Sy.maxsupernode <= SOLVE_MID_KMAX;
    // bulk: the kernels that have a blocked form go as SB_BLOCKED, the others as SB_BYCOL; top: everything SB_TOP
    auto level = [&](int lv, bool forward, bool top) {
        const int blk = top ? SB_TOP : SB_BLOCKED, col = top ? SB_TOP : SB_BYCOL;
        for (int fc = 0; fc < FC_COUNT; ++fc) {
            const int b0 = bucket0(lv, fc), nb = bucket0(lv, fc + 1) - b0;
            if (nb == 0) continue;
            const int g0 = sc.last0[lv], ng = sc.last1[lv] - g0, mm = sc.maxm[lv];
            if (forward) {
                if (fc == FC_WAVE && pair && P.wave_mmax[lv] <= 16) put(SO_FWD_PAIR16_16, blk, KK_FWD_WAVE, lv, b0, (nb + 3) / 4, 1, 64, 0, nb);
                else if (fc == FC_WAVE && pair && P.wave_kmax[lv] <= 16) put(SO_FWD_PAIR16, blk, KK_FWD_WAVE, lv, b0, (nb + 1) / 2, 1, 64, 0, nb);
                else if (fc == FC_WAVE && pair) put(SO_FWD_PAIR32, blk, KK_FWD_WAVE, lv, b0, (nb + 1) / 2, 1, 64, 0, nb);
                else if (fc == FC_WAVE) put(SO_FWD_WAVE, col, KK_FWD_WAVE, lv, b0, nb, 1, 64, lds_solve(32, 32));
                else if (fc == FC_LDS64 && mid) put(SO_FWD_MID1, blk, KK_FWD_LDS, lv, b0, nb, 1, 64, 0);
                else if (fc == FC_LDS128 && mid) put(SO_FWD_MID2, blk, KK_FWD_LDS, lv, b0, nb, 1, 64, 0);
                else if (fc == FC_LDS64) put(SO_FWD_LDS64, col, KK_FWD_LDS, lv, b0, nb, 1, 64, lds_solve(64, 64));
                else if (fc == FC_LDS128) put(SO_FWD_LDS128, col, KK_FWD_LDS, lv, b0, nb, 1, 256, lds_solve(128, 128));
                else if (ng <= 0) continue;
                else if (sc.allsolo[lv] && sc.maxk[lv] <= 64) put(SO_FWD_SOLO64, col, KK_FWD_BIG, lv, g0, (mm + 63) / 64 + 1, ng, 256, 0);
                else if (sc.allsolo[lv]) put(SO_FWD_SOLO, col, KK_FWD_BIG, lv, g0, (mm + 63) / 64 + 1, ng, 256, 0);
                else { put(SO_FWD_GRP, col, KK_FWD_BIG, lv, g0, ng, 1, 256, 0);
                       put(SO_FWD_GRP_UPD, col, KK_FWD_BIG_UPD, lv, g0, (mm + 63) / 64, ng, 256, 0); }
            } else {
                if (fc == FC_WAVE && pair && P.wave_mmax[lv] <= 16) put(SO_BWD_PAIR16_16, blk, KK_BWD_WAVE, lv, b0, (nb + 3) / 4, 1, 64, 0, nb);
                else if (fc == FC_WAVE && pair && P.wave_kmax[lv] <= 16) put(SO_BWD_PAIR16, blk, KK_BWD_WAVE, lv, b0, (nb + 1) / 2, 1, 64, 0, nb);
                else if (fc == FC_WAVE && pair) put(SO_BWD_PAIR32, blk, KK_BWD_WAVE, lv, b0, (nb + 1) / 2, 1, 64, 0, nb);
                else if (fc == FC_WAVE) put(SO_BWD_WAVE, col, KK_BWD_WAVE, lv, b0, nb, 1, 64, lds_solve(32, 32));
                else if (fc == FC_LDS64 && mid) put(SO_BWD_MID1, blk, KK_BWD_LDS, lv, b0, nb, 1, 64, 0);
                else if (fc == FC_LDS128 && mid) put(SO_BWD_MID2, blk, KK_BWD_LDS, lv, b0, nb, 1, 64, 0);
                else if (fc == FC_LDS64) put(SO_BWD_LDS64, col, KK_BWD_LDS, lv, b0, nb, 1, 64, lds_solve(64, 64));
                else if (fc == FC_LDS128) put(SO_BWD_LDS128, col, KK_BWD_LDS, lv, b0, nb, 1, 256, lds_solve(128, 128));
                else if (ng <= 0) continue;
                else if (!Sy.solve_group && sc.maxk[lv] <= 64) {
                    put(SO_BWD_DOT64, col, KK_BWD_BIG_DOT, lv, g0, (mm + 255) / 256, ng, 256, 0);
                    put(SO_BWD_FIN64, col, KK_BWD_BIG, lv, g0, ng, 1, 256, 0);
                } else {
                    put(SO_BWD_GRP_DOT, col, KK_BWD_BIG_DOT, lv, g0, (mm + 255) / 256, ng, 256, 0);
                    put(SO_BWD_GRP, col, KK_BWD_BIG, lv, g0, ng, 1, 256, 0); }
            }
        }
    };
    auto walk = [&](int lv_lo, int lv_hi, bool forward, bool top) {
        for (int q = lv_lo; q < lv_hi; ++q) {
            const int lv = forward ? q : lv_hi - 1 + lv_lo - q;
            const int sgi = forward ? P.seg_at_lv0[lv] : P.seg_at_lv1[lv];
            if (sgi < 0) { level(lv, forward, top); continue; }
            const ChainSeg& sg = P.chain_segs[sgi];
            if (forward) put(SO_FWD_CHAIN, SB_TOP, KK_FWD_BIG, lv, sg.wgf0, sg.nwg_f, 1, 320, 0);
            else put(SO_BWD_CHAIN, SB_TOP, KK_BWD_BIG, lv, sg.wgb0, sg.nwg_b, 1, 320, 0);
            q += sg.lv1 - sg.lv0;
        }
    };
    int lcs = (P.pair_solve && P.lc_levels > 0) ? P.lc_levels : 0;
    for (int lv = 0; lv < lcs; ++lv) if (P.seg_at_lv0[lv] >= 0) { lcs = 0; break; }
    int ls = NL;
    for (int lv = lcs; lv < NL; ++lv) if (P.seg_at_lv0[lv] >= 0) { ls = lv; break; }
    B.first_top_level = ls;
    if (lcs > 0) put(SO_FWD_LEAFCHAIN, SB_BLOCKED, KK_FWD_WAVE, 0, 0, (P.lc_nchains + 3) / 4, 1, 64, 0, P.lc_nchains);
    walk(lcs, ls, true, false);
    B.top0 = (int)B.rec.size();
    if (ls < NL) {
        put(SO_BUMP_EPOCH, SB_TOP, KK_SOLVE_PERM, ls, 0, 1, 1, 64, 0);
        walk(ls, NL, true, true);
        walk(ls, NL, false, true);
    }
    B.top1 = (int)B.rec.size();
    walk(lcs, ls, false, false);
    if (lcs > 0) put(SO_BWD_LEAFCHAIN, SB_BLOCKED, KK_BWD_WAVE, 0, 0, (P.lc_nchains + 3) / 4, 1, 64, 0, P.lc_nchains);
    for (const FactorLaunch& r : B.rec) { if (r.stream == SB_BLOCKED) ++B.blocked; else if (r.stream == SB_BYCOL) B.bycol += SOLVE_RB; else ++B.top; }
    return B;
}

} // namespace mi355x
