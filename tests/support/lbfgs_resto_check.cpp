// Stand-alone host program for tests/test_resto_abi.py: the restoration-phase transitions of a limited-memory history (LbResto, lb_push_bfgs_resto,
// lb_push_sr1_resto, lb_undo_resto in ipopt_amd/csrc/lbfgs_host.h, which is all it includes), built with -fsanitize=address,undefined and run on the
// CPU.  As tests/support/lbfgs_state_check.cpp it plays the device's part with host arrays of `slots` columns of 7 rows (the 3 m + 6 dots of a push are
// plain loops; after a stored push the pair goes into slot lb_slot(P, st, m - 1)) and keeps, next to the library's state, a model by the rule alone: the
// list of live pairs with the eta and 1 / sqrt(s^T y_new) of their push.  After every push it checks m, head, skipped, the columns through the slot
// map, and BITWISE against a recomputation from scratch with the same dot functions: G = S^T Ypart, S^T S, R = S^T (DR o S) (zero unless special),
// D_j = fma(eta, (S^T S)_jj, G_jj), L_ij = fma(eta, (S^T S)_ij, G_ij) at the eta of the push -- so for every pair stored earlier at ANOTHER eta --, eta,
// eta_col, dv, sigma by the rule (-1 when special), and that the coefficients are those of lb_coefficients / lb_sr1_coefficients on that state (with R and
// eta in the place of S^T S and sigma when special).  max_history 1, 2, 3, 32, both types, special 0 / 1, eta cycling 0.3, 0.3, 0.1, 0.03 over
// 2 max_history + 3 pushes (eviction at several eta), and the special pushes:
//   BFGS  s^T y_new <= 0 and a NaN entry: skips that move only the counter.  The min D skip: a pair with s^T ypart = -0.05 s^T s is stored at eta 0.3
//         (D = 0.25 s^T s, s^T y_new >= 0.025 s^T s as DR >= 0.25); a good pair pushed at eta 0.03 recomputes that D to -0.02 s^T s: skipped, LbState
//         and LbResto memcmp-equal but for the counter; the same pair at eta 0.3 is stored.  The Cholesky failure by rounding (not special, constant
//         sigma 1, DR_0 = 1): s = 2 e_0, ypart = 2^-62 s, eta = 2^-62 twice: D = 2^-59, the second pivot is (2^-59 + 4) - 4 = 0 exactly: LB_PUSH_NOT_PD with
//         the pair, its eta and dv stored.
//   SR1   a repeated newest pair at the same eta (two equal rows of Z) and a NaN entry are skips: both values memcmp-equal but for skipped, the backup
//         invalid.  Every stored push is undone once (both values bitwise those before, skipped + 1, eta back), a second undo answers 0, and the push
//         repeated gives bitwise the state of the first time.
// Exit status 0 and "ok": every check passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "lbfgs_host.h"

using namespace mi355x;

static constexpr int ROWS = 7;
static const double ETAS[4] = {0.3, 0.3, 0.1, 0.03};

struct Vec { double v[ROWS]; };
struct Pair { Vec s, y; double eta = 0.0, dv = 0.0; };      // y is ypart

static Vec DR;
static double dot(const double* a, const double* b) { double t = 0.0; for (int i = 0; i < ROWS; ++i) t += a[i] * b[i]; return t; }
static double wdot(const double* a, const double* b) { double t = 0.0; for (int i = 0; i < ROWS; ++i) t += (DR.v[i] * a[i]) * b[i]; return t; }      // (DR o a)^T b
static bool same(const void* a, const void* b, size_t n) { return std::memcmp(a, b, n) == 0; }

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); ++bad; } } while (0)

static Pair make_pair(int k, int type)
{
    Pair p;
    for (int i = 0; i < ROWS; ++i) {
        p.s.v[i] = std::sin(1.0 + 0.7 * k + 1.3 * i);
        const double sign = type == 1 && i % 2 == 1 ? -1.0 : 1.0;
        p.y.v[i] = sign * (1.0 + 0.25 * i) * p.s.v[i] + (type == 1 ? 0.1 : 0.05) * std::cos(0.9 * k + 2.0 * i);
    }
    return p;
}
static Pair with_nan(Pair p) { p.y.v[3] = std::numeric_limits<double>::quiet_NaN(); return p; }

struct Both { LbState st; LbResto rs; };
static bool same_but_skipped(Both a, const Both& b, int skipped)
{
    if (a.st.skipped != skipped) return false;
    a.st.skipped = b.st.skipped;
    return same(&a.st, &b.st, sizeof a.st) && same(&a.rs, &b.rs, sizeof a.rs);
}

struct Run {
    LbParams P; Both now, backup; bool backup_valid = false;
    std::vector<Vec> S, Y;              // `slots` columns: the device's ring (Y holds Ypart)
    std::vector<Pair> live;             // the model, oldest first
    int head = 0, skipped = 0; double eta = -1.0;
    double h[LBH_NDOT_RESTO]; LbRestoDots d;
    std::vector<double> coef = std::vector<double>(LBH_NCOEF_RESTO);

    Run(int type, int special, int max_history, int init, double init_val) : P(lb_params_resto(type, special, max_history, init, init_val, 1e-8, 1e8)), S(P.slots), Y(P.slots) {
        now.st = lb_fresh_resto(P);
        for (int c = 0; c < P.slots; ++c) for (int i = 0; i < ROWS; ++i) S[c].v[i] = Y[c].v[i] = 0.0;
    }
    void dots(const Pair& p) {
        const int m = now.st.m;
        for (int j = 0; j < m; ++j) {
            const int c = lb_slot(P, now.st, j);
            h[j] = dot(p.s.v, S[c].v); h[m + j] = dot(p.s.v, Y[c].v); h[2 * m + j] = P.special ? wdot(p.s.v, S[c].v) : 0.0;
        }
        Vec ds; for (int i = 0; i < ROWS; ++i) ds.v[i] = DR.v[i] * p.s.v[i];
        double* q = h + 3 * m;
        q[0] = dot(p.s.v, p.s.v); q[1] = dot(p.s.v, p.y.v); q[2] = dot(p.y.v, p.y.v); q[3] = dot(p.s.v, ds.v); q[4] = dot(p.y.v, ds.v); q[5] = dot(ds.v, ds.v);
        d = LbRestoDots{h, h + m, h + 2 * m, q[0], q[1], q[2], q[3], q[4], q[5]};
    }
    int push(const Pair& p, double e) {
        dots(p);
        const int r = P.type == 1 ? lb_push_sr1_resto(P, now.st, now.rs, backup.st, backup.rs, backup_valid, d, e) : lb_push_bfgs_resto(P, now.st, now.rs, d, e, coef.data());
        if (r == LB_PUSH_STORED || r == LB_PUSH_NOT_PD) { const int c = lb_slot(P, now.st, now.st.m - 1); S[c] = p.s; Y[c] = p.y; }
        return r;
    }
    // the model stores p, pushed at e (call after dots(p): d holds its dots)
    void model_store(Pair p, double e) {
        p.eta = e; p.dv = P.type == 1 ? 0.0 : 1.0 / std::sqrt(lb_resto_sy(d, e));
        if ((int)live.size() == P.max_history) { live.erase(live.begin()); head = (head + 1) % P.slots; }
        live.push_back(p); skipped = 0; eta = e;
    }
    void check(const char* what, int push_no) {
        const LbState& st = now.st; const LbResto& rs = now.rs;
        const int m = (int)live.size();
        CHECK(st.m == m && st.head == head && st.skipped == skipped, "%s, push %d: type %d special %d max %d: m %d (model %d), head %d (%d), skipped %d (%d)", what, push_no, P.type, P.special,
              P.max_history, st.m, m, st.head, head, st.skipped, skipped);
        if (st.m != m || st.head != head) return;
        CHECK(same(&rs.eta, &eta, sizeof eta), "%s, push %d: eta %.17g, model %.17g", what, push_no, rs.eta, eta);
        for (int j = 0; j < m; ++j) {
            const int c = lb_slot(P, st, j);
            CHECK(c >= 0 && c < P.slots, "%s, push %d: slot %d of column %d", what, push_no, c, j);
            CHECK(same(S[c].v, live[j].s.v, sizeof(Vec)) && same(Y[c].v, live[j].y.v, sizeof(Vec)), "%s, push %d: logical column %d (slot %d) is not pair %d of the model", what, push_no, j, c, j);
            CHECK(same(&rs.eta_col[j], &live[j].eta, sizeof(double)) && same(&rs.dv[j], &live[j].dv, sizeof(double)), "%s, push %d: eta_col / dv of column %d: %.17g %.17g, model %.17g %.17g",
                  what, push_no, j, rs.eta_col[j], rs.dv[j], live[j].eta, live[j].dv);
        }
        for (int j = 0; j < m; ++j)
            for (int i = 0; i < m; ++i) {
                const int a = i + j * LBH_MAX;
                const double sts = dot(live[i].s.v, live[j].s.v);      // (the newer vector first, as the dots of a push have it; dot is symmetric bit for bit)
                const double g = i >= j ? dot(live[i].s.v, live[j].y.v) : 0.0;
                const double r = !P.special ? 0.0 : i >= j ? wdot(live[i].s.v, live[j].s.v) : wdot(live[j].s.v, live[i].s.v);
                const double l = i > j ? std::fma(eta, sts, g) : 0.0;
                const double gl = i > j ? g : 0.0;
                CHECK(same(&st.STS[a], &sts, 8) && same(&st.L[a], &l, 8) && same(&rs.GL[a], &gl, 8) && same(&rs.R[a], &r, 8),
                      "%s, push %d: type %d special %d max %d: (%d, %d): S^T S %.17g L %.17g G %.17g R %.17g, from scratch %.17g %.17g %.17g %.17g", what, push_no, P.type, P.special, P.max_history, i, j,
                      st.STS[a], st.L[a], rs.GL[a], rs.R[a], sts, l, gl, r);
                if (i == j) {
                    const double dd = std::fma(eta, sts, g);
                    CHECK(same(&st.D[j], &dd, 8) && same(&rs.GD[j], &g, 8), "%s, push %d: D[%d] %.17g G %.17g, from scratch %.17g %.17g", what, push_no, j, st.D[j], rs.GD[j], dd, g);
                }
            }
    }
    // the coefficients a stored push left are those of the helpers on the stored state
    void check_coefficients(const char* what, int push_no, double e) {
        const LbState& st = now.st; const LbResto& rs = now.rs;
        if (P.type == 0) {
            std::vector<double> c2(LBH_NCOEF_RESTO, 0.0); double dd[LBH_MAX];
            const bool ok = lb_coefficients(st.m, P.special ? rs.R : st.STS, st.L, LBH_MAX, st.D, P.special ? e : st.sigma, dd, c2.data() + LBH_MAX, c2.data() + LBH_MAX + LBH_MAX * LBH_MAX, LBH_MAX);
            for (int j = 0; j < st.m; ++j) { c2[j] = live[j].dv; c2[LBH_NCOEF + j] = live[j].eta; }
            CHECK(ok && same(c2.data(), coef.data(), LBH_NCOEF_RESTO * sizeof(double)), "%s, push %d: special %d max %d: the coefficients are not dv, lb_coefficients, eta_col of the stored state", what, push_no, P.special, P.max_history);
        } else {
            LbState c; int nneg = -1;
            const int rc = lb_sr1_coefficients(st.m, P.special ? rs.R : st.STS, st.L, LBH_MAX, st.D, P.special ? e : st.sigma, c.E, c.Qs, LBH_MAX, &nneg);
            CHECK(rc == LB_SR1_OK && nneg == st.nneg && same(c.E, st.E, sizeof c.E) && same(c.Qs, st.Qs, sizeof c.Qs), "%s, push %d: special %d max %d: E, Qs, nneg are not lb_sr1_coefficients of the stored state", what, push_no, P.special, P.max_history);
        }
    }
};

static void run_bfgs(int max_history, int special)
{
    Run R(0, special, max_history, 0, 1.0);
    const int npush = 2 * max_history + 3;
    int stored = 0, notpd = 0;
    for (int k = 0; k < npush; ++k) {
        const double eta = ETAS[k % 4];
        if (k == 2 || k == max_history + 2) {
            for (int kind = 0; kind < 2; ++kind) {
                Pair q = make_pair(100 + k, 0);
                if (kind == 0) for (int i = 0; i < ROWS; ++i) q.y.v[i] = -3.0 * q.s.v[i]; else q = with_nan(q);
                const Both before = R.now; const std::vector<Vec> S0 = R.S;
                const int r = R.push(q, eta);
                ++R.skipped;
                CHECK(r == LB_PUSH_SKIPPED && same_but_skipped(R.now, before, before.st.skipped + 1), "BFGS special %d max %d push %d: a pair with %s is a skip that moves only the counter (answer %d)",
                      special, max_history, k, kind == 0 ? "s^T y_new <= 0" : "a NaN entry", r);
                CHECK(same(S0.data(), R.S.data(), S0.size() * sizeof(Vec)), "BFGS max %d push %d: a skip wrote a column", max_history, k);
                R.check("BFGS skip", k);
            }
        }
        const Pair p = make_pair(k, 0);
        R.dots(p);
        const double ss = R.d.ss, sy = lb_resto_sy(R.d, eta), yy = lb_resto_yy(R.d, eta);
        CHECK(!lb_skip(ss, sy, yy), "BFGS max %d push %d: the pair of the test has no positive curvature", max_history, k);
        const int r = R.push(p, eta);
        R.model_store(p, eta);
        CHECK(r == LB_PUSH_STORED || r == LB_PUSH_NOT_PD, "BFGS special %d max %d push %d: answer %d", special, max_history, k, r);
        stored += r == LB_PUSH_STORED; notpd += r == LB_PUSH_NOT_PD;
        R.check("BFGS push", k);
        const double sigma = special ? -1.0 : lb_sigma(R.P.init, R.P.init_val, R.P.smin, R.P.smax, ss, sy, yy);
        CHECK(same(&R.now.st.sigma, &sigma, sizeof sigma), "BFGS special %d max %d push %d: sigma %.17g, by the rule %.17g", special, max_history, k, R.now.st.sigma, sigma);
        if (r == LB_PUSH_STORED) R.check_coefficients("BFGS push", k, eta);
    }
    CHECK(stored >= npush - 1, "BFGS special %d max %d: only %d of %d pushes had coefficients", special, max_history, stored, npush);
    std::printf("BFGS special %d max_history %2d: %d pushes, %d with coefficients, %d not positive definite, m %d head %d\n", special, max_history, npush, stored, notpd, R.now.st.m, R.now.st.head);
}

// the recomputed D of an OLDER pair turns negative when eta drops (the head of this file)
static void run_bfgs_min_d(int max_history, int special)
{
    Run R(0, special, max_history, 0, 1.0);
    Pair a = make_pair(0, 0);
    for (int i = 0; i < ROWS; ++i) a.y.v[i] = -0.05 * a.s.v[i];
    int r = R.push(a, 0.3); R.model_store(a, 0.3);
    CHECK(r == LB_PUSH_STORED && R.now.st.D[0] > 0.0, "min D special %d max %d: the pair with negative s^T ypart is stored at eta 0.3 (answer %d, D %.3g)", special, max_history, r, R.now.st.D[0]);
    R.check("min D first", 0);
    const Pair p = make_pair(1, 0);
    const Both before = R.now; const std::vector<Vec> S0 = R.S, Y0 = R.Y;
    r = R.push(p, 0.03); ++R.skipped;
    CHECK(r == LB_PUSH_SKIPPED && same_but_skipped(R.now, before, 1), "min D special %d max %d: a push that recomputes an older D to <= 0 is a skip that moves only the counter (answer %d)", special, max_history, r);
    CHECK(same(S0.data(), R.S.data(), S0.size() * sizeof(Vec)) && same(Y0.data(), R.Y.data(), Y0.size() * sizeof(Vec)), "min D max %d: a skip wrote a column", max_history);
    R.check("min D skip", 1);
    r = R.push(p, 0.3); R.model_store(p, 0.3);
    CHECK(r == LB_PUSH_STORED, "min D special %d max %d: the same pair at eta 0.3 is stored (answer %d)", special, max_history, r);
    R.check("min D stored", 2);
    R.check_coefficients("min D stored", 2, 0.3);
    const Pair q = make_pair(2, 0);
    r = R.push(q, 0.03);
    if (max_history == 2) { R.model_store(q, 0.03); CHECK(r == LB_PUSH_STORED, "min D max 2: once the bad pair is evicted the small eta is fine (answer %d)", r); }
    else { ++R.skipped; CHECK(r == LB_PUSH_SKIPPED, "min D max %d: the bad pair is still live: skipped again (answer %d)", max_history, r); }
    R.check("min D last", 3);
}

static void run_bfgs_not_pd(int max_history)
{
    Run R(0, 0, max_history, 4, 1.0);                                         // not special, sigma = 1 constant
    const double eta = std::ldexp(1.0, -62);
    Pair p;
    for (int i = 0; i < ROWS; ++i) { p.s.v[i] = i == 0 ? 2.0 : 0.0; p.y.v[i] = std::ldexp(p.s.v[i], -62); }
    for (int k = 0; k < max_history + 2; ++k) {
        const int r = R.push(p, eta);
        R.model_store(p, eta);
        CHECK(r == (k == 0 ? LB_PUSH_STORED : LB_PUSH_NOT_PD), "not-PD max %d push %d: answer %d", max_history, k, r);
        R.check("not-PD push", k);
        CHECK(R.now.st.sigma == 1.0 && R.now.st.D[0] == std::ldexp(1.0, -59), "not-PD max %d push %d: sigma %.17g D %.17g", max_history, k, R.now.st.sigma, R.now.st.D[0]);
    }
    CHECK(R.now.st.m == max_history && R.now.st.head == 2 % R.P.slots, "not-PD max %d: m %d head %d after two evictions", max_history, R.now.st.m, R.now.st.head);
}

static void run_sr1(int max_history, int special)
{
    Run R(1, special, max_history, 4, 0.75);                                  // constant sigma (not used when special)
    const int npush = 2 * max_history + 3;
    int evicting_undos = 0;
    auto skip_case = [&](const Pair& q, double e, const char* what, int k) {
        const Both before = R.now; const std::vector<Vec> S0 = R.S, Y0 = R.Y;
        const int r = R.push(q, e);
        ++R.skipped;
        CHECK(r == LB_PUSH_SKIPPED && same_but_skipped(R.now, before, before.st.skipped + 1) && !R.backup_valid, "SR1 special %d max %d push %d: %s is a skip: the state but for the counter stays, the backup goes (answer %d, backup %d)",
              special, max_history, k, what, r, (int)R.backup_valid);
        CHECK(same(S0.data(), R.S.data(), S0.size() * sizeof(Vec)) && same(Y0.data(), R.Y.data(), Y0.size() * sizeof(Vec)), "SR1 max %d push %d: a skip wrote a column", max_history, k);
        const Both after = R.now;
        CHECK(lb_undo_resto(R.now.st, R.now.rs, R.backup.st, R.backup.rs, R.backup_valid) == 0 && same(&after.st, &R.now.st, sizeof after.st) && same(&after.rs, &R.now.rs, sizeof after.rs),
              "SR1 max %d push %d: an undo after a skip answers 0 and changes nothing", max_history, k);
        R.check("SR1 skip", k);
    };
    for (int k = 0; k < npush; ++k) {
        const double eta = ETAS[k % 4];
        if (k == 2 || k == max_history + 2) {
            if (max_history >= 2) skip_case(R.live.back(), R.eta, "a repeated newest pair", k);
            skip_case(with_nan(make_pair(100 + k, 1)), eta, "a NaN entry", k);
        }
        const Pair p = make_pair(k, 1);
        const Both before = R.now; const std::vector<Pair> live0 = R.live; const int head0 = R.head, skipped0 = R.skipped; const double eta0 = R.eta;
        int r = R.push(p, eta);
        R.model_store(p, eta);
        CHECK(r == LB_PUSH_STORED && R.backup_valid && same(&R.backup.st, &before.st, sizeof before.st) && same(&R.backup.rs, &before.rs, sizeof before.rs),
              "SR1 special %d max %d push %d: stored, and the backup is the state before (answer %d, backup %d)", special, max_history, k, r, (int)R.backup_valid);
        if (r != LB_PUSH_STORED) return;
        R.check("SR1 push", k);
        const double sigma = special ? -1.0 : lb_sr1_sigma(R.P.init, R.P.init_val, R.now.st.m, R.d.ss, lb_resto_sy(R.d, eta), lb_resto_yy(R.d, eta));
        CHECK(same(&R.now.st.sigma, &sigma, sizeof sigma), "SR1 special %d max %d push %d: sigma %.17g, by the rule %.17g", special, max_history, k, R.now.st.sigma, sigma);
        R.check_coefficients("SR1 push", k, eta);
        const Both first = R.now;
        const bool evicted = before.st.m == max_history;
        CHECK(lb_undo_resto(R.now.st, R.now.rs, R.backup.st, R.backup.rs, R.backup_valid) == 1 && !R.backup_valid && same_but_skipped(R.now, before, before.st.skipped + 1),
              "SR1 special %d max %d push %d: undo restores both values, skipped + 1", special, max_history, k);
        R.live = live0; R.head = head0; R.skipped = skipped0 + 1; R.eta = eta0;
        R.check(evicted ? "SR1 undo of an evicting push" : "SR1 undo", k);
        evicting_undos += evicted;
        const Both undone = R.now;
        CHECK(lb_undo_resto(R.now.st, R.now.rs, R.backup.st, R.backup.rs, R.backup_valid) == 0 && same(&undone.st, &R.now.st, sizeof undone.st) && same(&undone.rs, &R.now.rs, sizeof undone.rs),
              "SR1 max %d push %d: a second undo answers 0 and changes nothing", max_history, k);
        r = R.push(p, eta);
        R.model_store(p, eta);
        CHECK(r == LB_PUSH_STORED && same(&first.st, &R.now.st, sizeof first.st) && same(&first.rs, &R.now.rs, sizeof first.rs), "SR1 special %d max %d push %d: the push repeated after its undo gives another state (answer %d)", special, max_history, k, r);
        R.check("SR1 push again", k);
    }
    CHECK(evicting_undos >= max_history + 3, "SR1 max %d: only %d undos of evicting pushes", max_history, evicting_undos);
    std::printf("SR1  special %d max_history %2d: %d pushes, each undone and repeated (%d evicting), m %d head %d nneg %d\n", special, max_history, npush, evicting_undos, R.now.st.m, R.now.st.head, R.now.st.nneg);
}

int main()
{
    for (int i = 0; i < ROWS; ++i) DR.v[i] = 1.0 - 0.75 * ((i * 3) % ROWS) / 6.0;      // 1, 0.625, 0.25, 0.75, 0.375, 0.875, 0.5: in [0.25, 1], DR_0 = 1
    for (int i = 0; i < ROWS; ++i) CHECK(DR.v[i] >= 0.25 && DR.v[i] <= 1.0, "DR[%d] = %g", i, DR.v[i]);
    const int mh[4] = {1, 2, 3, 32};
    for (int q = 0; q < 4; ++q)
        for (int special = 0; special < 2; ++special) {
            run_bfgs(mh[q], special);
            if (mh[q] >= 2) run_bfgs_min_d(mh[q], special);
            if (mh[q] >= 2 && !special) run_bfgs_not_pd(mh[q]);
            run_sr1(mh[q], special);
        }
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
