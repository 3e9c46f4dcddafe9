// Stand-alone host program for tests/test_sr1_abi.py: the state machine of a limited-memory history (LbParams, LbState, lb_push_bfgs, lb_push_sr1,
// lb_undo, lb_slot in ipopt_amd/csrc/lbfgs_host.h), built with -fsanitize=address,undefined and run on the CPU.  It plays the device's part with host
// arrays of `slots` columns of 7 rows: the dots of a push are one plain loop, and after a stored push the pair is written into slot lb_slot(P, st, m - 1),
// which is all the form kernel does to the ring.  Next to the library's state it keeps the list of live pairs by the rule alone (append; drop the
// oldest when full) and after every push checks m, head, skipped, the columns read through the slot map, and D, L, S^T S BITWISE against those
// recomputed from scratch with the same dot function.  max_history 1, 2, 3, 32, both kinds, 2 max_history + 3 ordinary pushes and the special ones:
//   BFGS  s^T y <= 0 and a NaN entry are skips that move only the counter; a push whose lb_coefficients fails answers LB_PUSH_NOT_PD with the pair stored
//         and the head advanced.  M = Lt Lt^T + sigma S^T S of accepted pairs is positive definite in exact arithmetic, and a D entry is the s^T y that
//         passed the skip test, so neither "indefinite M" nor "D <= 0" can be had from real vectors; ROUNDING is used: the pair s = 2 e_0, y = 2^-62 s
//         repeated, sigma = 1 constant: the second pivot is (2^-60 + 4) - 2 * 2 = 0 exactly in binary64.
//         lb_undo on a BFGS state: the contract of lbfgs_host.h is that it answers 0 and changes nothing (no backup is ever valid); the refusal as an
//         error is the caller's (numeric.hip lbfgs_undo), not the host function's.
//   SR1   a repeated newest pair (constant sigma: Z has two equal columns) and a NaN entry are skips: LbState is memcmp-equal but for skipped, the backup
//         is invalid, an undo answers 0.  Every stored push is undone once: the state is bitwise the one before with skipped + 1, the logical columns
//         are the earlier ones (also when the push evicted a pair: the spare slot; max_history 1 has two slots), a second undo answers 0 and changes
//         nothing; the push is then repeated and must give bitwise the state it gave the first time.
// Exit status 0 and "ok": every check passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "lbfgs_host.h"

using namespace mi355x;

static constexpr int ROWS = 7;
static_assert(sizeof(LbState) == 4 * sizeof(int) + (1 + 2 * LBH_MAX + 3 * LBH_MAX * LBH_MAX) * sizeof(double), "LbState has no padding: memcmp compares values");

struct Vec { double v[ROWS]; };
struct Pair { Vec s, y; };

static double dot(const double* a, const double* b) { double t = 0.0; for (int i = 0; i < ROWS; ++i) t += a[i] * b[i]; return t; }
static bool same(const void* a, const void* b, size_t n) { return std::memcmp(a, b, n) == 0; }
static bool same_but_skipped(LbState a, const LbState& b, int skipped) { if (a.skipped != skipped) return false; a.skipped = b.skipped; return same(&a, &b, sizeof a); }

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); ++bad; } } while (0)

// pair k of a run: BFGS pairs have positive curvature (y = diag(1 + i / 4) s + a little), SR1 pairs mixed signs
static Pair make_pair(int k, int type)
{
    Pair p;
    for (int i = 0; i < ROWS; ++i) {
        p.s.v[i] = std::sin(1.0 + 0.7 * k + 1.3 * i);
        const double sign = type == 1 && i % 3 == 1 ? -1.0 : 1.0;
        p.y.v[i] = sign * (1.0 + 0.25 * i) * p.s.v[i] + (type == 1 ? 0.1 : 0.05) * std::cos(0.9 * k + 2.0 * i);
    }
    return p;
}

struct Run {
    LbParams P; LbState st, backup; bool backup_valid = false;
    std::vector<Vec> S, Y;              // `slots` columns: the device's ring
    std::vector<Pair> live;             // the model: the stored pairs by the rule alone, oldest first
    int head = 0, skipped = 0;          // the model's ring head and skip counter
    double h[2 * LBH_MAX + 3];          // the downloaded dots: sS (m), sY (m), ss, sy, yy
    std::vector<double> coef = std::vector<double>(LBH_NCOEF);

    Run(int type, int max_history, int init, double init_val) : P(lb_params(type, max_history, init, init_val, 1e-8, 1e8)), st(lb_fresh(P)), S(P.slots), Y(P.slots) {
        for (int c = 0; c < P.slots; ++c) for (int i = 0; i < ROWS; ++i) S[c].v[i] = Y[c].v[i] = 0.0;
    }
    void dots(const Pair& p) {
        const int m = st.m;
        for (int j = 0; j < m; ++j) { h[j] = dot(p.s.v, S[lb_slot(P, st, j)].v); h[m + j] = dot(p.s.v, Y[lb_slot(P, st, j)].v); }
        h[2 * m] = dot(p.s.v, p.s.v); h[2 * m + 1] = dot(p.s.v, p.y.v); h[2 * m + 2] = dot(p.y.v, p.y.v);
    }
    int push(const Pair& p) {
        dots(p);
        const int m = st.m;
        const int r = P.type == 1 ? lb_push_sr1(P, st, backup, backup_valid, h, h + m, h[2 * m], h[2 * m + 1], h[2 * m + 2])
                                  : lb_push_bfgs(P, st, h, h + m, h[2 * m], h[2 * m + 1], h[2 * m + 2], coef.data());
        if (r == LB_PUSH_STORED || r == LB_PUSH_NOT_PD) {                     // the form kernel (or the two slot copies of outcome 2)
            const int c = lb_slot(P, st, st.m - 1);
            S[c] = p.s; Y[c] = p.y;
        }
        return r;
    }
    void model_store(const Pair& p) {
        if ((int)live.size() == P.max_history) { live.erase(live.begin()); head = (head + 1) % P.slots; }
        live.push_back(p); skipped = 0;
    }
    // m, head, skipped, the columns through the slot map, and D, L, S^T S from scratch
    void check(const char* what, int push_no) {
        const int m = (int)live.size();
        CHECK(st.m == m && st.head == head && st.skipped == skipped, "%s, push %d: type %d max %d: m %d (model %d), head %d (%d), skipped %d (%d)", what, push_no, P.type, P.max_history,
              st.m, m, st.head, head, st.skipped, skipped);
        if (st.m != m || st.head != head) return;
        for (int j = 0; j < m; ++j) {
            const int c = lb_slot(P, st, j);
            CHECK(c >= 0 && c < P.slots, "%s, push %d: slot %d of column %d", what, push_no, c, j);
            CHECK(same(S[c].v, live[j].s.v, sizeof(Vec)) && same(Y[c].v, live[j].y.v, sizeof(Vec)), "%s, push %d: type %d max %d: logical column %d (slot %d) is not pair %d of the model",
                  what, push_no, P.type, P.max_history, j, c, j);
        }
        for (int j = 0; j < m; ++j)
            for (int i = 0; i < m; ++i) {
                const double sts = dot(live[i].s.v, live[j].s.v), l = i > j ? dot(live[i].s.v, live[j].y.v) : 0.0;
                CHECK(same(&st.STS[i + j * LBH_MAX], &sts, sizeof sts) && same(&st.L[i + j * LBH_MAX], &l, sizeof l), "%s, push %d: type %d max %d: S^T S / L (%d, %d): %.17g %.17g, from scratch %.17g %.17g",
                      what, push_no, P.type, P.max_history, i, j, st.STS[i + j * LBH_MAX], st.L[i + j * LBH_MAX], sts, l);
                if (i == j) { const double d = dot(live[j].s.v, live[j].y.v); CHECK(same(&st.D[j], &d, sizeof d), "%s, push %d: D[%d] %.17g, from scratch %.17g", what, push_no, j, st.D[j], d); }
            }
    }
};

static Pair with_nan(Pair p) { p.y.v[3] = std::numeric_limits<double>::quiet_NaN(); return p; }

static void run_bfgs(int max_history)
{
    Run R(0, max_history, 0, 1.0);                                            // sigma = s^T y / s^T s, clipped
    const int npush = 2 * max_history + 3;
    int stored = 0, notpd = 0;
    for (int k = 0; k < npush; ++k) {
        if (k == 2 || k == max_history + 2) {                                 // the two skips, once with a short and once with a full history
            for (int kind = 0; kind < 2; ++kind) {
                Pair q = make_pair(100 + k, 0);
                if (kind == 0) for (int i = 0; i < ROWS; ++i) q.y.v[i] = -q.s.v[i]; else q = with_nan(q);
                const LbState before = R.st; const std::vector<Vec> S0 = R.S;
                const int r = R.push(q);
                ++R.skipped;
                CHECK(r == LB_PUSH_SKIPPED && same_but_skipped(R.st, before, before.skipped + 1), "BFGS max %d push %d: a pair with %s is a skip that moves only the counter (answer %d)",
                      max_history, k, kind == 0 ? "s^T y <= 0" : "a NaN entry", r);
                CHECK(same(S0.data(), R.S.data(), S0.size() * sizeof(Vec)), "BFGS max %d push %d: a skip wrote a column", max_history, k);
                R.check("BFGS skip", k);
            }
        }
        const Pair p = make_pair(k, 0);
        R.dots(p);
        const int m0 = R.st.m; const double ss = R.h[2 * m0], sy = R.h[2 * m0 + 1], yy = R.h[2 * m0 + 2];
        CHECK(sy > std::sqrt(std::numeric_limits<double>::epsilon()) * std::sqrt(ss) * std::sqrt(yy), "BFGS max %d push %d: the pair of the test has no positive curvature", max_history, k);
        const int r = R.push(p);
        R.model_store(p);
        CHECK(r == LB_PUSH_STORED || r == LB_PUSH_NOT_PD, "BFGS max %d push %d: answer %d", max_history, k, r);
        stored += r == LB_PUSH_STORED; notpd += r == LB_PUSH_NOT_PD;
        R.check("BFGS push", k);
        const double sigma = lb_sigma(R.P.init, R.P.init_val, R.P.smin, R.P.smax, ss, sy, yy);
        CHECK(same(&R.st.sigma, &sigma, sizeof sigma), "BFGS max %d push %d: sigma %.17g, by the rule %.17g", max_history, k, R.st.sigma, sigma);
        if (r == LB_PUSH_STORED) {                                            // the coefficients are those of the state
            std::vector<double> c2(LBH_NCOEF, 0.0);
            const bool ok = lb_coefficients(R.st.m, R.st.STS, R.st.L, LBH_MAX, R.st.D, R.st.sigma, c2.data(), c2.data() + LBH_MAX, c2.data() + LBH_MAX + LBH_MAX * LBH_MAX, LBH_MAX);
            CHECK(ok && same(c2.data(), R.coef.data(), LBH_NCOEF * sizeof(double)), "BFGS max %d push %d: the coefficients are not lb_coefficients of the stored state", max_history, k);
        }
        const LbState after = R.st;                                           // undo on a BFGS state: 0, nothing changes
        CHECK(!R.backup_valid && lb_undo(R.st, R.backup, R.backup_valid) == 0 && same(&after, &R.st, sizeof after), "BFGS max %d push %d: lb_undo must answer 0 and change nothing", max_history, k);
    }
    std::printf("BFGS max_history %2d: %d pushes, %d with coefficients, %d not positive definite, m %d head %d\n", max_history, npush, stored, notpd, R.st.m, R.st.head);
}

// lb_coefficients fails by rounding (the head of this file): the pair is stored, the head moves once the history is full
static void run_bfgs_not_pd(int max_history)
{
    Run R(0, max_history, 4, 1.0);                                            // sigma = 1, constant
    Pair p;
    for (int i = 0; i < ROWS; ++i) { p.s.v[i] = i == 0 ? 2.0 : 0.0; p.y.v[i] = std::ldexp(p.s.v[i], -62); }
    for (int k = 0; k < max_history + 2; ++k) {
        const int r = R.push(p);
        R.model_store(p);
        CHECK(r == (k == 0 ? LB_PUSH_STORED : LB_PUSH_NOT_PD), "not-PD max %d push %d: answer %d", max_history, k, r);
        R.check("not-PD push", k);
        CHECK(R.st.sigma == 1.0, "not-PD max %d push %d: sigma %.17g", max_history, k, R.st.sigma);
    }
    CHECK(R.st.m == max_history && R.st.head == 2 % R.P.slots, "not-PD max %d: m %d head %d after two evictions", max_history, R.st.m, R.st.head);
}

static void run_sr1(int max_history)
{
    Run R(1, max_history, 4, 0.75);                                           // constant sigma: a repeated newest pair makes Z singular
    const int npush = 2 * max_history + 3;
    int evicting_undos = 0;
    auto skip_case = [&](const Pair& q, const char* what, int k) {
        const LbState before = R.st; const std::vector<Vec> S0 = R.S, Y0 = R.Y;
        const int r = R.push(q);
        ++R.skipped;
        CHECK(r == LB_PUSH_SKIPPED && same_but_skipped(R.st, before, before.skipped + 1) && !R.backup_valid, "SR1 max %d push %d: %s is a skip: the state but for the counter stays, the backup goes (answer %d, backup %d)",
              max_history, k, what, r, (int)R.backup_valid);
        CHECK(same(S0.data(), R.S.data(), S0.size() * sizeof(Vec)) && same(Y0.data(), R.Y.data(), Y0.size() * sizeof(Vec)), "SR1 max %d push %d: a skip wrote a column", max_history, k);
        const LbState after = R.st;
        CHECK(lb_undo(R.st, R.backup, R.backup_valid) == 0 && same(&after, &R.st, sizeof after), "SR1 max %d push %d: an undo after a skip answers 0 and changes nothing", max_history, k);
        R.check("SR1 skip", k);
    };
    for (int k = 0; k < npush; ++k) {
        if (k == 2 || k == max_history + 2) {
            if (max_history >= 2) skip_case(R.live.back(), "a repeated newest pair", k);      // (max_history 1: the repeat replaces the only pair, nothing is singular)
            skip_case(with_nan(make_pair(100 + k, 1)), "a NaN entry", k);
        }
        const Pair p = make_pair(k, 1);
        const LbState before = R.st; const std::vector<Pair> live0 = R.live; const int head0 = R.head, skipped0 = R.skipped;
        R.dots(p);
        const int m0 = before.m; const double ss = R.h[2 * m0], sy = R.h[2 * m0 + 1], yy = R.h[2 * m0 + 2];
        int r = R.push(p);
        R.model_store(p);
        CHECK(r == LB_PUSH_STORED && R.backup_valid && same(&R.backup, &before, sizeof before), "SR1 max %d push %d: stored, and the backup is the state before (answer %d, backup %d)", max_history, k, r, (int)R.backup_valid);
        if (r != LB_PUSH_STORED) return;
        R.check("SR1 push", k);
        const double sigma = lb_sr1_sigma(R.P.init, R.P.init_val, R.st.m, ss, sy, yy);
        CHECK(same(&R.st.sigma, &sigma, sizeof sigma), "SR1 max %d push %d: sigma %.17g, by the rule %.17g", max_history, k, R.st.sigma, sigma);
        {                                                                     // E, Qs, nneg are the split of the stored state
            LbState c; int nneg = -1;
            const int rc = lb_sr1_coefficients(R.st.m, R.st.STS, R.st.L, LBH_MAX, R.st.D, R.st.sigma, c.E, c.Qs, LBH_MAX, &nneg);
            CHECK(rc == LB_SR1_OK && nneg == R.st.nneg && same(c.E, R.st.E, sizeof c.E) && same(c.Qs, R.st.Qs, sizeof c.Qs), "SR1 max %d push %d: E, Qs, nneg are not lb_sr1_coefficients of the stored state", max_history, k);
        }
        const LbState first = R.st;
        // undo: the state before with skipped + 1, the earlier columns through the slot map (the arrays are not touched: the evicted pair kept its slot)
        const bool evicted = m0 == max_history;
        CHECK(lb_undo(R.st, R.backup, R.backup_valid) == 1 && !R.backup_valid && same_but_skipped(R.st, before, before.skipped + 1), "SR1 max %d push %d: undo restores the state before, skipped + 1", max_history, k);
        R.live = live0; R.head = head0; R.skipped = skipped0 + 1;
        R.check(evicted ? "SR1 undo of an evicting push" : "SR1 undo", k);
        evicting_undos += evicted;
        const LbState undone = R.st;
        CHECK(lb_undo(R.st, R.backup, R.backup_valid) == 0 && same(&undone, &R.st, sizeof undone), "SR1 max %d push %d: a second undo answers 0 and changes nothing", max_history, k);
        // the same push again: bitwise the state of the first time (the counter of the undo is gone: a stored push zeroes it)
        r = R.push(p);
        R.model_store(p);
        CHECK(r == LB_PUSH_STORED && same(&first, &R.st, sizeof first), "SR1 max %d push %d: the push repeated after its undo gives another state (answer %d)", max_history, k, r);
        R.check("SR1 push again", k);
    }
    CHECK(evicting_undos >= max_history + 3, "SR1 max %d: only %d undos of evicting pushes", max_history, evicting_undos);
    std::printf("SR1  max_history %2d: %d pushes, each undone and repeated (%d evicting), m %d head %d nneg %d\n", max_history, npush, evicting_undos, R.st.m, R.st.head, R.st.nneg);
}

int main()
{
    const int mh[4] = {1, 2, 3, 32};
    for (int q = 0; q < 4; ++q) {
        run_bfgs(mh[q]);
        if (mh[q] >= 2) run_bfgs_not_pd(mh[q]);                               // (one pair alone: M = sigma s^T s > 0)
        run_sr1(mh[q]);
    }
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
