// factor_schedule_check.cpp -- stand-alone CPU program (own main, no device, nothing preloaded), built with AddressSanitizer and UBSan by
// tests/test_factor_schedule.py together with symbolic.cpp, matching_scaling.cpp and launch_plan.cpp: a 2-D grid KKT pattern is analysed, the launch
// plan and every factor schedule of it are built -- one GPU in both variants, every rank of a 2-rank world -- and every record is walked with its
// indices checked against the arrays the executor and the kernels would index with them.
#include "launch_plan.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace mi355x;

static int g_fail = 0;
static long g_ops[FO_COUNT] = {0};
#define CHECK(c) do { if (!(c)) { if (++g_fail <= 20) std::printf("FAIL line %d: %s\n", __LINE__, #c); } } while (0)

// primal variables on an nx x ny grid (5-point coupling, `dof` per node, dense inside a node), one constraint row per node coupling the node's variables
static void grid_kkt(int nx, int ny, int dof, std::vector<int>& row, std::vector<int>& col, std::vector<double>& val, int& n)
{
    const int np = nx * ny * dof;
    n = np + nx * ny;
    auto var = [&](int i, int j, int d) { return (i * ny + j) * dof + d + 1; };      // 1-based
    auto put = [&](int r, int c, double v) { row.push_back(r > c ? r : c); col.push_back(r > c ? c : r); val.push_back(v); };
    for (int i = 0; i < nx; ++i) for (int j = 0; j < ny; ++j) {
        for (int d = 0; d < dof; ++d) {
            for (int e = 0; e <= d; ++e) put(var(i, j, d), var(i, j, e), d == e ? 8.0 + 0.01 * ((i * 7 + j * 3 + d) % 11) : -0.5);
            if (i + 1 < nx) put(var(i + 1, j, d), var(i, j, d), -1.0);
            if (j + 1 < ny) put(var(i, j + 1, d), var(i, j, d), -1.0);
            put(np + i * ny + j + 1, var(i, j, d), 1.0 + 0.1 * d);
        }
        put(np + i * ny + j + 1, np + i * ny + j + 1, -1e-8);
    }
}

static void walk(const LaunchPlan& P, const Symbolic& Sy, const std::vector<FactorLaunch>& list, int which)
{
    const int nlist = (int)P.lvl_list.size(), NL = P.nlevels;
    CHECK(P.fmeta.size() == P.lvl_list.size() && P.asm_fast_ok.size() == P.lvl_list.size());
    int pending_ev = -1, pending_lv = -1;
    for (const FactorLaunch& r : list) {
        CHECK(r.op >= 0 && r.op < FO_COUNT);
        if (r.op >= 0 && r.op < FO_COUNT) ++g_ops[r.op];
        CHECK(r.stream >= FS_MAIN && r.stream <= FS_SIDE);
        CHECK(r.gx > 0 && r.gy > 0 && r.block >= 0 && r.block <= 1024 && r.lds >= 0 && r.lds <= 160 * 1024);
        const bool stream_op = r.op >= FO_FORK;
        CHECK((r.kind == -1) == stream_op && r.kind < KK_COUNT);
        CHECK(r.lv >= 0 && (r.lv < NL || (r.op == FO_JOIN && r.lv == NL)));
        int count = 0;      // launch-list entries [b0, b0 + count) the kernel reads fmeta of
        switch (r.op) {
        case FO_LEAF_CHAIN: CHECK(r.a[0] == P.lc_nchains && (int)P.lc_ptr.size() == r.a[0] + 1 && P.lc_ptr[r.a[0]] <= (int)P.lc_link.size() && r.a[1] == P.lc_levels - 1); break;
        case FO_FRONT_DF:
            CHECK(r.a[0] >= 0 && r.a[1] > 0 && r.a[0] + r.a[1] <= (int)P.df_tab.size() && r.a[3] < NL);
            for (int l = 0; l < r.a[1] && r.a[0] + l < (int)P.df_tab.size(); ++l) { const DfLevel& D = P.df_tab[r.a[0] + l]; CHECK(D.b0 >= 0 && D.n16 <= D.nb && D.b0 + D.nb <= nlist && D.q0 < r.a[2]); }
            break;
        case FO_FRONT_DPP16: count = r.a[0]; CHECK(r.gx == (r.a[0] + 3) / 4); break;
        case FO_REG_64_2: case FO_REG_64_4: case FO_REG_64_8: case FO_REG_256_6_FAST4: case FO_REG_256_8_FAST: case FO_REG_256_6: case FO_REG_256_8:
        case FO_DIAG_REG: case FO_DIAG_REG_1024: case FO_DIAG_TRSM: case FO_GRP_FUSED: count = r.gx; break;
        default: count = stream_op ? 0 : r.gy; break;
        }
        CHECK(r.b0 >= 0 && r.b0 + count <= nlist);
        for (int q = r.b0; q < r.b0 + count && q < nlist; ++q) {
            const int sn = P.lvl_list[q];
            CHECK(sn >= 0 && sn < Sy.num_sn && P.fmeta[q].s == sn);
            if (r.op >= FO_ASSEMBLE && r.op <= FO_SCHUR_Q) { CHECK(Sy.sn_class[sn] == FC_BIG); CHECK(P.fmeta[q].bigidx >= 0 && P.fmeta[q].bigidx < P.nbig); CHECK(P.fmeta[q].gbase >= 0 && P.fmeta[q].gbase + P.fmeta[q].gpos < (int)P.gtab.size()); }
            if (r.op == FO_ASSEMBLE2) CHECK(P.asm_fast_ok[q] >= 1 && P.asm_fast_ok[q] <= r.a[2] && P.fmeta[q].m <= r.a[1]);
            if (r.op == FO_DIAG_REG || r.op == FO_DIAG_REG_1024 || r.op == FO_TRSM || r.op == FO_TRSM_WIDE) CHECK(P.fmeta[q].k <= r.a[0]);
            if (r.op == FO_DIAG_TRSM) CHECK(P.fmeta[q].k <= r.a[1] && (P.fmeta[q].m + 63) / 64 <= r.a[0]);
        }
        if (r.op == FO_ASSEMBLE2) CHECK(r.lds == r.a[1] * r.a[2] * (int)sizeof(int) && r.a[2] <= 16);
        if (stream_op && r.op <= FO_JOIN) {      // the events the executor owns: [0] P.la_tiles2, [1 + i] P.grp[i].la2
            const int ev = r.a[0], lv = r.op == FO_JOIN ? r.a[1] : r.lv;
            CHECK(ev >= 0 && ev <= (int)P.grp.size() && lv >= 0 && lv < NL);
            if (ev >= 0 && ev <= (int)P.grp.size() && lv >= 0 && lv < NL) CHECK((ev == 0 ? P.la_tiles2[lv] : P.grp[ev - 1].la2[lv]) > 0);      // (setup creates the events of exactly these levels)
            if (r.op == FO_FORK_DONE) { pending_ev = ev; pending_lv = lv; }
            if (r.op == FO_JOIN) { CHECK(ev == pending_ev && lv == pending_lv); pending_ev = -1; }
        }
        if (which != 0) CHECK(r.stream == FS_MAIN);
    }
    CHECK(pending_ev == -1);
}

int main()
{
    std::vector<int> row, col; std::vector<double> val; int n = 0;
    grid_kkt(48, 44, 3, row, col, val, n);
    long records = 0;
    for (int nranks = 1; nranks <= 2; ++nranks) {
        SymbolicOptions so; so.nranks = nranks;
        Symbolic Sy;
        if (!analyse(Sy, so, n, (int)row.size(), row.data(), col.data(), 0, val.data())) { std::printf("analyse failed\n"); return 1; }
        for (int rank = 0; rank < nranks; ++rank) {
            PlanInputs in; in.nranks = nranks; in.rank = rank; in.multi = nranks > 1;
            in.la_min_nt = 3; in.la_min_tiles = 0;      // (look-ahead on whatever this small system splits)
            const LaunchPlan P = build_launch_plan(Sy, in);
            if (!P.error.empty()) { std::printf("plan: %s\n", P.error.c_str()); return 1; }
            if (nranks == 1)
                for (int o = 0; o < 2; ++o) { const auto list = build_factor_schedule(P, Sy, in, 0, o != 0); CHECK(!list.empty()); walk(P, Sy, list, 0); records += (long)list.size(); }
            else {
                CHECK(build_factor_schedule(P, Sy, in, 2 + P.ndepth - 1, false).size() + build_factor_schedule(P, Sy, in, 1, false).size() > 0);
                for (int w = 1; w < 2 + P.ndepth; ++w) { const auto list = build_factor_schedule(P, Sy, in, w, false); walk(P, Sy, list, w); records += (long)list.size(); }
            }
        }
    }
    std::printf("%ld records walked, %d failures; per op:", records, g_fail);
    for (int o = 0; o < FO_COUNT; ++o) std::printf(" %ld", g_ops[o]);
    std::printf("\n");
    CHECK(g_ops[FO_GRP_FUSED] + g_ops[FO_DIAG_TRSM] + g_ops[FO_DIAG_REG] > 0 && g_ops[FO_SCHUR64] > 0);      // (the system reaches the blocked path)
    if (g_fail) return 1;
    std::printf("ok\n");
    return 0;
}
