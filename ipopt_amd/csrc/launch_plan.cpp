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
    in.pair_solve = !knob_disabled("pair_solve"); in.p1_small = !knob_disabled("p1_small");
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

} // namespace mi355x
