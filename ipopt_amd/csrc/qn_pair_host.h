// qn_pair_host.h -- the host side of the quasi-Newton pair (s, y) formed on the device (numeric.hip qn_pair_*; reference
// IpLimMemQuasiNewtonUpdater.cpp:276-308): the validation of a definition, the column view of [J_c; J_d] the kernel walks, the rule that picks the
// kernel's lanes per column, and the state rules of store / form / push / get.  No HIP in here: a stand-alone host program can include it
// (tests/support/qn_pair_host_check.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace mi355x {

// The J_c and J_d segments of the value assembly as ranges [off, off + len) of the triplet list; len == 0: the block is absent.
struct QpSegs { long long off_jc = 0, len_jc = 0, off_jd = 0, len_jd = 0; };

// dims4 = {nx, ns, nc, nd}; (irn, jcn) the 1-based triplets of analyse(), nnz of them.  Every entry of the J_c range must have one index in the x range
// [0, nx) and the other in the c range [nx + ns, nx + ns + nc); for J_d the other index lies in the d range [nx + ns + nc, n).  Either orientation.
// This check is the reason k_qn_pair cannot index out of range: nothing reaches the device before it has passed.
// false: `why` names the offending argument and, for a triplet, its position in the triplet list (the FIRST offending one).
inline bool qp_check(long long nnz, const int32_t* dims4, const int32_t* irn, const int32_t* jcn, const QpSegs& g, std::string& why)
{
    if (nnz < 0) { why = "nnz must be >= 0"; return false; }
    if (!dims4) { why = "dims4 is null"; return false; }
    for (int q = 0; q < 4; ++q) if (dims4[q] < 0) { why = "dims4[" + std::to_string(q) + "] = " + std::to_string(dims4[q]) + " must be >= 0"; return false; }
    const long long nx = dims4[0], ns = dims4[1], nc = dims4[2], nd = dims4[3], n = nx + ns + nc + nd;
    if (n > 0x7fffffffll) { why = "dims4 must sum to less than 2^31"; return false; }
    if (ns != nd) { why = "dims4: ns = " + std::to_string(ns) + " must equal nd = " + std::to_string(nd); return false; }
    if (g.len_jc < 0 || g.off_jc < 0 || g.off_jc + g.len_jc > nnz) { why = "the J_c segment [" + std::to_string(g.off_jc) + ", +" + std::to_string(g.len_jc) + ") is not inside the " + std::to_string(nnz) + " triplets"; return false; }
    if (g.len_jd < 0 || g.off_jd < 0 || g.off_jd + g.len_jd > nnz) { why = "the J_d segment [" + std::to_string(g.off_jd) + ", +" + std::to_string(g.len_jd) + ") is not inside the " + std::to_string(nnz) + " triplets"; return false; }
    if (g.len_jc > 0 && g.len_jd > 0 && g.off_jc < g.off_jd + g.len_jd && g.off_jd < g.off_jc + g.len_jc) { why = "the J_c and J_d segments overlap"; return false; }
    if (g.len_jc + g.len_jd > 0x7fffffffll) { why = "the J_c and J_d segments must hold less than 2^31 entries"; return false; }
    if (g.len_jc + g.len_jd > 0 && (!irn || !jcn)) { why = !irn ? "irn is null" : "jcn is null"; return false; }
    for (int blk = 0; blk < 2; ++blk) {
        const long long off = blk ? g.off_jd : g.off_jc, len = blk ? g.len_jd : g.len_jc;
        const long long lo = blk ? nx + ns + nc : nx + ns, hi = blk ? n : nx + ns + nc;
        const char* name = blk ? "J_d" : "J_c";
        for (long long t = off; t < off + len; ++t) {
            const long long a = (long long)irn[t] - 1, b = (long long)jcn[t] - 1;
            const bool ax = a >= 0 && a < nx, bx = b >= 0 && b < nx, am = a >= lo && a < hi, bm = b >= lo && b < hi;
            if ((ax && bm) || (bx && am)) continue;
            why = std::string("irn / jcn: the ") + name + " triplet at position " + std::to_string(t) + " is (" + std::to_string(irn[t]) + ", " + std::to_string(jcn[t]) + "): "
                + (ax && bx ? "both indices lie in the x block" : "one index must lie in the x block [1, " + std::to_string(nx) + "] and the other in the " + (blk ? "d" : "c") + " block [" + std::to_string(lo + 1) + ", " + std::to_string(hi) + "]");
            return false;
        }
    }
    return true;
}

// The column view of [J_c; J_d]: column j of the x block holds the entries ent[2 p], ent[2 p + 1] = (i, u), p in [ptr[j], ptr[j + 1]): i the position of the
// entry's multiplier in y_c | y_d (a J_d row r counts nc + r), u its slot in the concatenation J_c segment | J_d segment (what J_last is indexed with; the
// current value is the J_c source at u, or the J_d source at u - len_jc).  Entries of a column in ascending u: slot order, J_c's before J_d's; duplicate
// triplets stay separate entries and sum.  (i, u) interleaved: ONE 8-byte load per entry.  Only for arguments qp_check has passed.
struct QpView { std::vector<int32_t> ptr, ent; int maxlen = 0; };
inline void qp_build(const int32_t* dims4, const int32_t* irn, const int32_t* jcn, const QpSegs& g, QpView& v)
{
    const int nx = dims4[0], ns = dims4[1], nc = dims4[2];
    const long long nent = g.len_jc + g.len_jd;
    v.ptr.assign((size_t)nx + 1, 0); v.ent.assign(2 * (size_t)nent, 0); v.maxlen = 0;
    auto column = [&](long long t) { const int a = irn[t] - 1, b = jcn[t] - 1; return a < nx ? a : b; };      // (one of the two is the x index: qp_check)
    for (int blk = 0; blk < 2; ++blk) { const long long off = blk ? g.off_jd : g.off_jc, len = blk ? g.len_jd : g.len_jc; for (long long t = off; t < off + len; ++t) v.ptr[(size_t)column(t) + 1]++; }
    for (int j = 0; j < nx; ++j) { v.maxlen = v.ptr[j + 1] > v.maxlen ? v.ptr[j + 1] : v.maxlen; v.ptr[j + 1] += v.ptr[j]; }
    std::vector<int32_t> fill(v.ptr.begin(), v.ptr.end() - 1);
    for (int blk = 0; blk < 2; ++blk) {
        const long long off = blk ? g.off_jd : g.off_jc, len = blk ? g.len_jd : g.len_jc;
        const int base = blk ? nx + ns + nc : nx + ns;
        for (long long t = off; t < off + len; ++t) {
            const int a = irn[t] - 1, b = jcn[t] - 1, j = a < nx ? a : b, r = (a < nx ? b : a) - base;
            const size_t p = (size_t)fill[j]++;
            v.ent[2 * p] = (blk ? nc : 0) + r; v.ent[2 * p + 1] = (int32_t)((blk ? g.len_jc : 0) + (t - off));
        }
    }
}

// Lanes per column of k_qn_pair<LPC>, from the STRUCTURE alone (the same structure always runs the same instantiation, so the order of every sum is a
// property of the definition):  a column beyond 256 entries -> 64 (one wavefront per column: a lane walking such a column alone is the whole launch's
// critical path);  else a mean below 4 entries per column -> 1 (with more lanes most of them idle);  else 8.
inline int qp_pick_lpc(long long nx, long long nent, int maxlen)
{
    if (maxlen > 256) return 64;
    if (nent < 4 * nx) return 1;
    return 8;
}

// What the handle knows about its pair, on the host: every rule below answers without a device.
struct QpState {
    bool defined = false, stored = false, formed = false;
    bool stored_gf = false, formed_gf = false;      // the snapshot / the formed pair carries grad_f (false: the restoration variant, y is ypart)
    int nx = 0, nc = 0, nd = 0; long long len_jc = 0, len_jd = 0;
};
inline bool qp_store_ok(const QpState& s, bool roll, std::string& why)
{
    if (!s.defined) { why = "nothing is defined (qn_pair_define first)"; return false; }
    if (roll && !s.formed) { why = "x is null (roll) but no pair is formed: there are no vectors to take over (qn_pair_form first, or pass x)"; return false; }
    return true;
}
inline bool qp_form_ok(const QpState& s, bool has_gf, std::string& why)
{
    if (!s.defined) { why = "nothing is defined (qn_pair_define first)"; return false; }
    if (!s.stored) { why = "nothing is stored (qn_pair_store first)"; return false; }
    if (has_gf != s.stored_gf) { why = has_gf ? "grad_f is given but qn_pair_store was given none (the restoration variant): both calls take it or neither" : "grad_f is null but qn_pair_store was given one: both calls take it or neither"; return false; }
    return true;
}
// hist_rows: rows of the defined history (0: none), hist_resto: it is a restoration-phase history; map_rows / map_last: the row map (0 / -1: none)
inline bool qp_push_ok(const QpState& s, int hist_rows, bool hist_resto, int map_rows, long long map_last, std::string& why)
{
    if (!s.defined) { why = "nothing is defined (qn_pair_define first)"; return false; }
    if (!s.formed) { why = "no pair is formed (qn_pair_form first)"; return false; }
    if (hist_rows <= 0) { why = "no history is defined (lbfgs_define, lbfgs_define_sr1 or lbfgs_define_resto first)"; return false; }
    if (hist_resto && s.formed_gf) { why = "a restoration-phase history takes ypart: the pair must be formed without grad_f"; return false; }
    if (!hist_resto && !s.formed_gf) { why = "a plain history takes y: the pair must be formed with grad_f"; return false; }
    if (map_rows > 0) { if (map_last >= s.nx) { why = "the row map reaches beyond the x block (idx[rows-1] = " + std::to_string(map_last) + " must be < nx = " + std::to_string(s.nx) + ")"; return false; } }
    else if (hist_rows > s.nx) { why = "the history has rows = " + std::to_string(hist_rows) + " > nx = " + std::to_string(s.nx); return false; }
    return true;
}
// doubles of array `what` of qn_pair_get (0 s, 1 y, 2 x_last, 3 grad_f_last, 4 Jc_last, 5 Jd_last), or -1 and why
inline long long qp_get_need(const QpState& s, int what, std::string& why)
{
    if (what < 0 || what > 5) { why = "what must be in [0, 5] (s, y, x_last, grad_f_last, Jc_last, Jd_last)"; return -1; }
    if (!s.defined) { why = "nothing is defined (qn_pair_define first)"; return -1; }
    if (what <= 1 && !s.formed) { why = "no pair is formed (qn_pair_form first)"; return -1; }
    if (what >= 2 && !s.stored) { why = "nothing is stored (qn_pair_store first)"; return -1; }
    if (what == 3 && !s.stored_gf) { why = "what 3 (grad_f_last): the snapshot was stored without grad_f (the restoration variant)"; return -1; }
    return what <= 3 ? s.nx : what == 4 ? s.len_jc : s.len_jd;
}

} // namespace mi355x
