// Stand-alone host program for tests/test_qn_pair_abi.py: the host side of the quasi-Newton pair formed on the device (ipopt_amd/csrc/qn_pair_host.h),
// built with -fsanitize=address,undefined and run on the CPU.
//   qp_check   accepts the structures below and names what is wrong with the hostile ones: ns != nd, a segment outside the triplets, overlapping
//              segments, a J_c triplet whose row lies in the d block, a triplet with both indices in x, an index out of range -- with the FIRST
//              offending triplet position
//   qp_build   the column view (ptr, interleaved (i, u), longest column) of small structures against arrays written down by hand: both blocks with
//              duplicates and a column with no entry; the J_c segment in upper orientation and BEHIND the J_d segment in the triplet list; an empty
//              J_c block; an empty J_d block; no block at all; nx = 0
//   qp_pick_lpc  the rule on its thresholds
//   QpState    the rules of store / form / push / get in the order the C ABI applies them: form before store, push before form, push with no history,
//              the grad_f mismatch both ways, the history kinds, the row map against nx, rows against nx, get of every array in every state
// Exit status 0 and "ok": every check passed.
#include <cstdio>
#include <cstdint>
#include <string>
#include <vector>
#include "qn_pair_host.h"

using namespace mi355x;

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); ++bad; } } while (0)
typedef std::vector<int32_t> IV;

static bool has(const std::string& s, const char* w) { return s.find(w) != std::string::npos; }

static void view_is(const char* what, const int32_t* dims, const IV& irn, const IV& jcn, const QpSegs& g, const IV& ptr, const IV& ent, int maxlen)
{
    std::string why;
    const bool ok = qp_check((long long)irn.size(), dims, irn.data(), jcn.data(), g, why);
    CHECK(ok, "%s: %s", what, why.c_str());
    if (!ok) return;
    QpView v;
    qp_build(dims, irn.data(), jcn.data(), g, v);
    CHECK(v.ptr == ptr, "%s: ptr", what);
    CHECK(v.ent == ent, "%s: ent", what);
    CHECK(v.maxlen == maxlen, "%s: maxlen %d", what, v.maxlen);
}

static void refused(const char* what, long long nnz, const int32_t* dims, const IV& irn, const IV& jcn, const QpSegs& g, const char* word1, const char* word2)
{
    std::string why;
    CHECK(!qp_check(nnz, dims, irn.data(), jcn.data(), g, why), "%s: accepted", what);
    CHECK(has(why, word1) && has(why, word2), "%s: '%s' does not name '%s' and '%s'", what, why.c_str(), word1, word2);
}

int main()
{
    // nx = 4, ns = nd = 2, nc = 2: x 1..4, s 5..6, c 7..8, d 9..10.  Triplets: 2 diagonal entries | J_c (5) | 1 diagonal | J_d (4)
    const int32_t dims[4] = {4, 2, 2, 2};
    {
        //            diag  diag | J_c: (7,1) (8,1) (7,3) (7,1)dup (8,4) | diag | J_d: (9,3) (10,1) (9,3)dup (10,4)
        const IV irn = {1,   2,    7,    8,    7,    7,       8,           5,     9,    10,   9,        10};
        const IV jcn = {1,   2,    1,    1,    3,    1,       4,           5,     3,    1,    3,        4};
        const QpSegs g{2, 5, 8, 4};
        // column 0: J_c u = 0 (i 0), 1 (i 1), 3 (i 0), then J_d u = 6 (i 2 + 1);  column 1: nothing;  column 2: u = 2 (i 0), 5 (i 2), 7 (i 2);  column 3: u = 4 (i 1), 8 (i 3)
        view_is("both blocks", dims, irn, jcn, g, {0, 4, 4, 7, 9}, {0, 0, 1, 1, 0, 3, 3, 6,   0, 2, 2, 5, 2, 7,   1, 4, 3, 8}, 4);
        // the same J_c in UPPER orientation (x index first), and the J_d segment IN FRONT of it in the triplet list
        const IV irn2 = {9, 10, 9, 10,   1, 1, 3, 1, 4,   1};
        const IV jcn2 = {3, 1,  3, 4,    7, 8, 7, 7, 8,   1};
        view_is("upper J_c behind J_d", dims, irn2, jcn2, QpSegs{4, 5, 0, 4}, {0, 4, 4, 7, 9}, {0, 0, 1, 1, 0, 3, 3, 6,   0, 2, 2, 5, 2, 7,   1, 4, 3, 8}, 4);
        view_is("no J_c", dims, irn, jcn, QpSegs{0, 0, 8, 4}, {0, 1, 1, 3, 4}, {3, 1,   2, 0, 2, 2,   3, 3}, 2);
        view_is("no J_d", dims, irn, jcn, QpSegs{2, 5, 0, 0}, {0, 3, 3, 4, 5}, {0, 0, 1, 1, 0, 3,   0, 2,   1, 4}, 3);
        view_is("no block", dims, irn, jcn, QpSegs{}, {0, 0, 0, 0, 0}, {}, 0);
        const int32_t none[4] = {0, 0, 0, 0};
        view_is("nx = 0", none, IV{}, IV{}, QpSegs{}, {0}, {}, 0);

        const int32_t uneven[4] = {4, 2, 2, 3};
        refused("ns != nd", 12, uneven, irn, jcn, g, "ns", "nd");
        refused("segment beyond the triplets", 12, dims, irn, jcn, QpSegs{2, 5, 8, 5}, "J_d segment", "12 triplets");
        refused("negative length", 12, dims, irn, jcn, QpSegs{2, -1, 8, 4}, "J_c segment", "triplets");
        refused("overlap", 12, dims, irn, jcn, QpSegs{2, 5, 6, 4}, "overlap", "J_d");
        IV r = irn, c = jcn;
        r[4] = 9;                                                                    // the J_c triplet at position 4 gets a row of the d block
        refused("J_c row in d", 12, dims, r, c, g, "J_c triplet at position 4", "c block [7, 8]");
        r = irn; r[6] = 2; r[5] = 3;                                                 // positions 5 and 6 both lie in x: the first is named
        refused("both in x", 12, dims, r, c, g, "position 5", "both indices lie in the x block");
        r = irn; r[9] = 8;                                                           // a J_d triplet with a row of the c block
        refused("J_d row in c", 12, dims, r, c, g, "J_d triplet at position 9", "d block [9, 10]");
        r = irn; r[8] = 11;
        refused("out of range", 12, dims, r, c, g, "J_d triplet at position 8", "(11, 3)");
        r = irn; c = jcn; c[2] = 0;
        refused("zero index", 12, dims, r, c, g, "J_c triplet at position 2", "(7, 0)");
        r = irn; c = jcn; r[3] = 5; c[3] = 8;                                        // s block against c block: no x index
        refused("no x index", 12, dims, r, c, g, "position 3", "x block [1, 4]");
        std::string why;
        CHECK(!qp_check(12, nullptr, irn.data(), jcn.data(), g, why) && has(why, "dims4"), "null dims4: %s", why.c_str());
        CHECK(!qp_check(12, dims, nullptr, jcn.data(), g, why) && has(why, "irn"), "null irn: %s", why.c_str());
        CHECK(!qp_check(12, dims, irn.data(), nullptr, g, why) && has(why, "jcn"), "null jcn: %s", why.c_str());
        CHECK(qp_check(12, dims, nullptr, nullptr, QpSegs{}, why), "no block needs no triplets: %s", why.c_str());
    }
    // the rule of the lanes per column
    CHECK(qp_pick_lpc(100, 399, 256) == 1 && qp_pick_lpc(100, 400, 256) == 8 && qp_pick_lpc(100, 399, 257) == 64 && qp_pick_lpc(100, 4000, 257) == 64 && qp_pick_lpc(0, 0, 0) == 8, "qp_pick_lpc");
    // the state rules
    {
        QpState s; std::string why;
        CHECK(!qp_store_ok(s, false, why) && has(why, "qn_pair_define"), "store undefined");
        CHECK(!qp_form_ok(s, true, why) && has(why, "qn_pair_define"), "form undefined");
        CHECK(!qp_push_ok(s, 4, false, 0, -1, why) && has(why, "qn_pair_define"), "push undefined");
        CHECK(qp_get_need(s, 0, why) < 0 && has(why, "qn_pair_define"), "get undefined");
        CHECK(qp_get_need(s, 6, why) < 0 && has(why, "what") && qp_get_need(s, -1, why) < 0, "get what");
        s.defined = true; s.nx = 4; s.nc = 2; s.nd = 2; s.len_jc = 5; s.len_jd = 3;
        CHECK(qp_store_ok(s, false, why), "store");
        CHECK(!qp_store_ok(s, true, why) && has(why, "roll"), "roll with nothing formed");
        CHECK(!qp_form_ok(s, true, why) && has(why, "qn_pair_store first"), "form before store: %s", why.c_str());
        CHECK(qp_get_need(s, 2, why) < 0 && has(why, "stored"), "get x_last before store");
        s.stored = true; s.stored_gf = true;
        CHECK(qp_form_ok(s, true, why), "form");
        CHECK(!qp_form_ok(s, false, why) && has(why, "grad_f is null"), "grad_f missing in form: %s", why.c_str());
        CHECK(!qp_push_ok(s, 4, false, 0, -1, why) && has(why, "qn_pair_form first"), "push before form: %s", why.c_str());
        CHECK(qp_get_need(s, 0, why) < 0 && has(why, "formed"), "get s before form");
        CHECK(qp_get_need(s, 2, why) == 4 && qp_get_need(s, 3, why) == 4 && qp_get_need(s, 4, why) == 5 && qp_get_need(s, 5, why) == 3, "get sizes");
        s.formed = true; s.formed_gf = true;
        CHECK(qp_get_need(s, 0, why) == 4 && qp_get_need(s, 1, why) == 4, "get s, y");
        CHECK(qp_store_ok(s, true, why), "roll");
        CHECK(!qp_push_ok(s, 0, false, 0, -1, why) && has(why, "no history"), "push with no history: %s", why.c_str());
        CHECK(qp_push_ok(s, 4, false, 0, -1, why) && qp_push_ok(s, 3, false, 0, -1, why), "push");
        CHECK(!qp_push_ok(s, 5, false, 0, -1, why) && has(why, "rows") && has(why, "nx"), "rows > nx");
        CHECK(!qp_push_ok(s, 4, true, 0, -1, why) && has(why, "without grad_f"), "resto history, plain pair");
        CHECK(qp_push_ok(s, 2, false, 2, 3, why), "mapped push");
        CHECK(!qp_push_ok(s, 2, false, 2, 4, why) && has(why, "row map"), "map beyond x");
        s.stored_gf = false; s.formed_gf = false;
        CHECK(!qp_form_ok(s, true, why) && has(why, "grad_f is given"), "grad_f given to form only: %s", why.c_str());
        CHECK(qp_form_ok(s, false, why), "resto form");
        CHECK(qp_push_ok(s, 4, true, 0, -1, why), "resto push");
        CHECK(!qp_push_ok(s, 4, false, 0, -1, why) && has(why, "with grad_f"), "plain history, resto pair");
        CHECK(qp_get_need(s, 3, why) < 0 && has(why, "grad_f"), "get grad_f_last of a resto snapshot");
    }
    if (bad) { std::printf("%d checks failed\n", bad); return 1; }
    std::printf("ok\n");
    return 0;
}
