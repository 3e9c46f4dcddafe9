// lbfgs_host.h -- the small dense algebra of the limited-memory BFGS updater (numeric.hip lbfgs_push and the stand-alone
// mi355x_kkt_lbfgs_coefficients share it; reference IpLimMemQuasiNewtonUpdater.cpp: CheckSkippingBFGS :985-1019, sigma :405-432,
// UpdateInternalData :769-818, the columns :440-520): plain host loops with a fixed order, column-major with an explicit leading
// dimension, at most 32 pairs.  No HIP in here: a stand-alone host program can include it.  Behind the BFGS part, the SR1 update of the same
// updater (:523-671, SplitEigenvalues :873-983): sigma, a cyclic Jacobi eigen-solver and the split of Z = D + L + L^T - sigma S^T S.
//
// At the end, the state machine of a history: LbParams (the constants), LbState (what a push can change) and the transitions.  They take the dots
// of the new pair (sS[j] = s^T S_j, sY[j] = s^T Y_j over the stored pairs, oldest first; ss, sy, yy), call the helpers above in a fixed order and
// touch no device; the caller (numeric.hip, or tests/support/lbfgs_state_check.cpp) owns the columns and moves them AFTER the transition:
//   lb_slot(P, st, j)     the physical column slot of logical pair j (oldest first): (head + j) % slots, BFGS and SR1 alike.  P.slots >= 1.
//   lb_push_bfgs          LB_PUSH_SKIPPED: lb_skip held, only `skipped` grew.  Otherwise skipped = 0, sigma, head advanced when the history was
//                         full, D, L, S^T S augmented / shifted; the caller writes the pair into lb_slot(P, st, st.m - 1).  LB_PUSH_STORED: coef
//                         holds d, C, Lbar (lb_coefficients).  LB_PUSH_NOT_PD: lb_coefficients failed; the pair IS stored, coef is not valid.
//   lb_push_sr1           works on a copy.  LB_PUSH_SKIPPED (a dot is not finite, or the split rule): st is untouched but for skipped + 1, and the
//                         backup is invalidated.  LB_PUSH_FAILED (the eigen-solver): nothing changes at all.  LB_PUSH_STORED: backup = st as it
//                         was, st = the copy with skipped = 0; the caller writes the pair into lb_slot(P, st, st.m - 1), which with slots =
//                         max_history + 1 is never the slot of a pair that is live in the backup.
//   lb_undo               1: st = backup with skipped = backup.skipped + 1, the backup is invalidated (one level).  0: no valid backup, nothing
//                         changes.  It does not look at the type: a BFGS history never has a valid backup, so it answers 0 there; refusing an
//                         undo on a BFGS history as an error is the caller's business (lbfgs_undo in numeric.hip does).
// Last, the restoration phase (LbParams::resto): LbResto, the value that travels with LbState there, and lb_push_bfgs_resto, lb_push_sr1_resto,
// lb_undo_resto, which take 3 m + 6 dots and eta.  A plain history never sees that part.
#pragma once
#include <cmath>
#include <limits>
#include "lowrank_host.h"      // lr_cholesky

namespace mi355x {

static constexpr int LBH_MAX = 32;      // pairs (MI355X_KKT_LBFGS_MAX)

// the pair (s, y) is not stored: s^T y <= sqrt(eps) |s| |y|, or one of the three dots is not finite (the reference never sees such a pair)
inline bool lb_skip(double ss, double sy, double yy)
{
    if (!std::isfinite(ss) || !std::isfinite(sy) || !std::isfinite(yy)) return true;
    return sy <= std::sqrt(std::numeric_limits<double>::epsilon()) * std::sqrt(ss) * std::sqrt(yy);
}

// sigma of B0 = sigma I from the new pair: init 0..3 = scalar1..4, 4 = constant; then clipped to [smin, smax]
inline double lb_sigma(int init, double init_val, double smin, double smax, double ss, double sy, double yy)
{
    double sg = init_val;
    switch (init) {
    case 0: sg = sy / ss; break;
    case 1: sg = yy / sy; break;
    case 2: sg = (sy / ss + yy / sy) / 2.0; break;
    case 3: sg = std::sqrt((sy / ss) * (yy / sy)); break;
    default: break;
    }
    return std::fmax(std::fmin(smax, sg), smin);
}

// D (m), L (strictly lower; L_ij = s_i^T y_j, i > j) and S^T S of m stored pairs, leading dimension LBH_MAX, take the new pair: "augment"
// while m < max_history, "shift" (the oldest pair leaves) when the history is full.  sS[j] = s^T S_j and sY[j] = s^T Y_j over the m pairs stored
// BEFORE the call (oldest first), ss = s^T s, sy = s^T y.  Only the new row and column are computed.  Returns the new m.
inline int lb_store(int m, int max_history, double* D, double* L, double* STS, const double* sS, const double* sY, double ss, double sy)
{
    const int ld = LBH_MAX;
    int off = 0;
    if (m == max_history) {                                          // shift: entry (i, j) <- (i + 1, j + 1)
        for (int j = 0; j + 1 < m; ++j) {
            D[j] = D[j + 1];
            for (int i = 0; i + 1 < m; ++i) { L[i + j * ld] = L[i + 1 + (j + 1) * ld]; STS[i + j * ld] = STS[i + 1 + (j + 1) * ld]; }
        }
        off = 1; --m;
    }
    for (int j = 0; j < m; ++j) {
        L[m + j * ld] = sY[j + off]; L[j + m * ld] = 0.0;
        STS[m + j * ld] = STS[j + m * ld] = sS[j + off];
    }
    L[m + m * ld] = 0.0; STS[m + m * ld] = ss; D[m] = sy;
    return m + 1;
}

// d = D^(-1/2);  Lt = L diag(d);  M = Lt Lt^T + sigma S^T S;  J = chol(M);  C = J^(-T) (upper);  Lbar = Lt^T C (strictly upper): then with
// V = Y diag(d) and U = sigma S C + V Lbar,  sigma I + V V^T - U U^T  is the BFGS matrix of the pairs started from sigma I.
// sts, L have leading dimension ldi; C, Lbar leading dimension ldo; d (m) may be null.  false: a D_j or a Cholesky pivot is <= 0 or not finite.
inline bool lb_coefficients(int m, const double* sts, const double* L, int ldi, const double* D, double sigma, double* d, double* C, double* Lbar, int ldo)
{
    double dd[LBH_MAX], Lt[LBH_MAX * LBH_MAX], J[LBH_MAX * LBH_MAX];
    for (int j = 0; j < m; ++j) {
        if (!(D[j] > 0.0) || !std::isfinite(D[j])) return false;
        dd[j] = 1.0 / std::sqrt(D[j]);
        if (d) d[j] = dd[j];
    }
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) Lt[i + j * m] = i > j ? L[i + j * ldi] * dd[j] : 0.0;
    for (int j = 0; j < m; ++j)
        for (int i = j; i < m; ++i) {
            double s = 0.0;
            for (int k = 0; k < j; ++k) s += Lt[i + k * m] * Lt[j + k * m];      // (Lt is strictly lower: k < min(i, j) = j)
            s += sigma * (0.5 * (sts[i + j * ldi] + sts[j + i * ldi]));
            J[i + j * m] = J[j + i * m] = s;
        }
    if (!lr_cholesky(J, m)) return false;
    // C = J^-T: column i of J^-1 by forward substitution on e_i, stored as row i of C
    for (int i = 0; i < m; ++i) {
        for (int r = 0; r < m; ++r) {
            if (r < i) { C[i + r * ldo] = 0.0; continue; }
            double s = r == i ? 1.0 : 0.0;
            for (int k = i; k < r; ++k) s -= J[r + k * m] * C[i + k * ldo];
            C[i + r * ldo] = s / J[r + r * m];
        }
    }
    // after the loop above C[i + r ldo] = (J^-1)[r, i] = (J^-T)[i, r]: upper triangular
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) {
            double s = 0.0;
            for (int k = i + 1; k <= j; ++k) s += Lt[k + i * m] * C[k + j * ldo];
            Lbar[i + j * ldo] = s;
        }
    return true;
}

// ---- limited-memory SR1 (reference :523-671, SplitEigenvalues :873-983) ----
// sigma of B0 = sigma I for an SR1 push, m_after = the pairs stored once the new one is in: the only pair -> init_val; otherwise the BFGS formulas with
// t = max(1e-8, |s^T y|) in the place of s^T y.  Not clipped (the reference does not clip here).
inline double lb_sr1_sigma(int init, double init_val, int m_after, double ss, double sy, double yy)
{
    if (m_after <= 1) return init_val;
    const double t = std::fmax(1e-8, std::fabs(sy));
    switch (init) {
    case 0: return t / ss;
    case 1: return yy / t;
    case 2: return (t / ss + yy / t) / 2.0;
    case 3: return std::sqrt((t / ss) * (yy / t));
    default: return init_val;
    }
}

static constexpr int LBH_JACOBI_SWEEPS = 30;

// Cyclic Jacobi for the symmetric m x m A (column-major, leading dimension m, both triangles kept; destroyed): A = Q diag(E) Q^T, E ascending (ties by
// the index the value had on the diagonal), Q's columns (leading dimension ldq) in E's order.  A sweep visits (p, q), p < q, by rows.
//   skip    the rotation of (p, q) is skipped when  |a_pq| <= u min(|a_pp|, |a_qq|)  or  |a_pq| <= u^2 |A|_F,  u = 2^-53, |A|_F of the matrix given
//   rotate  theta = (a_qq - a_pp) / (2 a_pq),  t = sign(theta) / (|theta| + sqrt(theta^2 + 1)),  c = 1 / sqrt(t^2 + 1),  s = t c
//   stop    after the first sweep that rotated nothing; false when LBH_JACOBI_SWEEPS sweeps all rotated something (a NaN ends here as well)
inline bool lb_jacobi(int m, double* A, double* E, double* Q, int ldq)
{
    const double u = std::ldexp(1.0, -53);
    double fro = 0.0;
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) { fro += A[i + j * m] * A[i + j * m]; Q[i + j * ldq] = i == j ? 1.0 : 0.0; }
    const double floor_ = u * u * std::sqrt(fro);
    bool converged = false;
    for (int sweep = 0; sweep < LBH_JACOBI_SWEEPS && !converged; ++sweep) {
        int rotated = 0;
        for (int p = 0; p + 1 < m; ++p)
            for (int q = p + 1; q < m; ++q) {
                const double apq = A[p + q * m], app = A[p + p * m], aqq = A[q + q * m], g = std::fabs(apq);
                if (g <= u * std::fmin(std::fabs(app), std::fabs(aqq)) || g <= floor_) continue;
                ++rotated;
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                A[p + p * m] = app - t * apq; A[q + q * m] = aqq + t * apq; A[p + q * m] = A[q + p * m] = 0.0;
                for (int k = 0; k < m; ++k) {
                    if (k != p && k != q) {
                        const double akp = A[k + p * m], akq = A[k + q * m];
                        A[k + p * m] = A[p + k * m] = c * akp - s * akq;
                        A[k + q * m] = A[q + k * m] = s * akp + c * akq;
                    }
                    const double qkp = Q[k + p * ldq], qkq = Q[k + q * ldq];
                    Q[k + p * ldq] = c * qkp - s * qkq;
                    Q[k + q * ldq] = s * qkp + c * qkq;
                }
            }
        converged = rotated == 0;
    }
    if (!converged) return false;
    int idx[LBH_MAX]; double col[LBH_MAX * LBH_MAX];
    for (int j = 0; j < m; ++j) {                                      // insertion sort of the indices: stable, so ties keep their index order
        int k = j;
        while (k > 0 && A[idx[k - 1] + idx[k - 1] * m] > A[j + j * m]) { idx[k] = idx[k - 1]; --k; }
        idx[k] = j;
    }
    for (int j = 0; j < m; ++j) { E[j] = A[idx[j] + idx[j] * m]; for (int i = 0; i < m; ++i) col[i + j * m] = Q[i + idx[j] * ldq]; }
    for (int j = 0; j < m; ++j) for (int i = 0; i < m; ++i) Q[i + j * ldq] = col[i + j * m];
    return true;
}

enum { LB_SR1_OK = 0, LB_SR1_SKIP = 1, LB_SR1_FAILED = 2 };

// Z = D + L + L^T - sigma sym(S^T S) = Q diag(E) Q^T (E ascending, *nneg of them < 0);  Qs[:, j] = Q[:, j] / sqrt(|E_j|):  with W = Y - sigma S,
// U = W Qs[:, :nneg], V = W Qs[:, nneg:],  sigma I + V V^T - U U^T = sigma I + W Z^-1 W^T  is the SR1 matrix of the pairs started from sigma I.
// sts, L leading dimension ld; Qs leading dimension ldo.  LB_SR1_SKIP: emax = max(|E_0|, |E_(m-1)|) is 0, or emin / emax < 1e-12 with emin the
// |E_j| next to the sign change (E_0, -E_(m-1), or min(-E_(nneg-1), E_nneg)): E is set, Qs is not.  LB_SR1_FAILED: the eigen-solver ran out of sweeps.
inline int lb_sr1_coefficients(int m, const double* sts, const double* L, int ld, const double* D, double sigma, double* E, double* Qs, int ldo, int* nneg)
{
    double Z[LBH_MAX * LBH_MAX];
    *nneg = 0;
    if (m == 0) return LB_SR1_OK;
    for (int j = 0; j < m; ++j) {
        Z[j + j * m] = D[j] - sigma * sts[j + j * ld];
        for (int i = j + 1; i < m; ++i) Z[i + j * m] = Z[j + i * m] = L[i + j * ld] - sigma * (0.5 * (sts[i + j * ld] + sts[j + i * ld]));
    }
    if (!lb_jacobi(m, Z, E, Qs, ldo)) return LB_SR1_FAILED;
    int nn = 0;
    for (int j = 0; j < m; ++j) if (E[j] < 0.0) ++nn;
    *nneg = nn;
    const double emax = std::fmax(std::fabs(E[0]), std::fabs(E[m - 1]));
    if (emax == 0.0) return LB_SR1_SKIP;
    const double emin = nn == 0 ? E[0] : nn == m ? -E[m - 1] : std::fmin(-E[nn - 1], E[nn]);
    if (emin / emax < 1e-12) return LB_SR1_SKIP;
    for (int j = 0; j < m; ++j) {
        const double r = std::sqrt(std::fabs(E[j]));
        for (int i = 0; i < m; ++i) Qs[i + j * ldo] = Qs[i + j * ldo] / r;
    }
    return LB_SR1_OK;
}

// ---- the state of a history and its transitions (see the head of this file) ----
struct LbParams {                       // the constants of a history, set by define and never by a push.  type: 0 BFGS, 1 SR1
    int type = 0, max_history = 0, slots = 0, init = 0;      // slots = max_history (BFGS) or max_history + 1 (SR1: the pair a push evicts survives that push)
    double init_val = 1.0, smin = 1e-8, smax = 1e8;
    int resto = 0, special = 0;         // resto: a restoration-phase history (lb_push_*_resto below); special: its B0 is eta D_R, not sigma I
};
struct LbState {                        // everything a push can change; a plain value: copied, assigned and compared as a whole
    int m = 0, head = 0, nneg = 0, skipped = 0;
    double sigma = 1.0, D[LBH_MAX] = {}, L[LBH_MAX * LBH_MAX] = {}, STS[LBH_MAX * LBH_MAX] = {}, E[LBH_MAX] = {}, Qs[LBH_MAX * LBH_MAX] = {};
};
static constexpr int LBH_NCOEF = LBH_MAX + 2 * LBH_MAX * LBH_MAX;      // d, C, Lbar of a BFGS push, in this order

inline LbParams lb_params(int type, int max_history, int init, double init_val, double smin, double smax)
{ return LbParams{type, max_history, max_history + (type == 1 ? 1 : 0), init, init_val, smin, smax}; }
inline LbState lb_fresh(const LbParams& P) { LbState st; st.sigma = P.init_val; return st; }
inline int lb_slot(const LbParams& P, const LbState& st, int j) { return (st.head + j) % P.slots; }

enum { LB_PUSH_STORED = 0, LB_PUSH_SKIPPED = 1, LB_PUSH_NOT_PD = 2, LB_PUSH_FAILED = -1 };
// sS, sY: the dots of s with the st.m stored pairs, oldest first.  coef: LBH_NCOEF doubles (zeroed here; valid on LB_PUSH_STORED only).
inline int lb_push_bfgs(const LbParams& P, LbState& st, const double* sS, const double* sY, double ss, double sy, double yy, double* coef)
{
    if (lb_skip(ss, sy, yy)) { ++st.skipped; return LB_PUSH_SKIPPED; }
    st.skipped = 0;
    st.sigma = lb_sigma(P.init, P.init_val, P.smin, P.smax, ss, sy, yy);
    if (st.m == P.max_history) st.head = lb_slot(P, st, 1);           // the oldest pair leaves
    st.m = lb_store(st.m, P.max_history, st.D, st.L, st.STS, sS, sY, ss, sy);
    for (int e = 0; e < LBH_NCOEF; ++e) coef[e] = 0.0;
    return lb_coefficients(st.m, st.STS, st.L, LBH_MAX, st.D, st.sigma, coef, coef + LBH_MAX, coef + LBH_MAX + LBH_MAX * LBH_MAX, LBH_MAX) ? LB_PUSH_STORED : LB_PUSH_NOT_PD;
}

inline int lb_push_sr1(const LbParams& P, LbState& st, LbState& backup, bool& backup_valid, const double* sS, const double* sY, double ss, double sy, double yy)
{
    if (!std::isfinite(ss) || !std::isfinite(sy) || !std::isfinite(yy)) { ++st.skipped; backup_valid = false; return LB_PUSH_SKIPPED; }
    LbState c = st;                                                    // the candidate: committed only when the split rule passes
    c.m = lb_store(st.m, P.max_history, c.D, c.L, c.STS, sS, sY, ss, sy);
    c.sigma = lb_sr1_sigma(P.init, P.init_val, c.m, ss, sy, yy);
    for (int e = 0; e < LBH_MAX * LBH_MAX; ++e) { c.Qs[e] = 0.0; if (e < LBH_MAX) c.E[e] = 0.0; }
    const int r = lb_sr1_coefficients(c.m, c.STS, c.L, LBH_MAX, c.D, c.sigma, c.E, c.Qs, LBH_MAX, &c.nneg);
    if (r == LB_SR1_FAILED) return LB_PUSH_FAILED;
    if (r == LB_SR1_SKIP) { ++st.skipped; backup_valid = false; return LB_PUSH_SKIPPED; }
    if (st.m == P.max_history) c.head = lb_slot(P, st, 1);            // the oldest pair leaves the window; its slot is the spare one now
    c.skipped = 0;
    backup = st; backup_valid = true; st = c;
    return LB_PUSH_STORED;
}

inline int lb_undo(LbState& st, const LbState& backup, bool& backup_valid)
{
    if (!backup_valid) return 0;
    st = backup; st.skipped = backup.skipped + 1; backup_valid = false;
    return 1;
}

// ---- the restoration phase (reference update_for_resto_: UpdateHessian :331-343, :372-400, UpdateInternalData :820-868, RecalcY/D/L :1382-1433) ----
// Per push the caller gives s, ypart (y without the objective part) and eta; DR (rows positive entries) is fixed per history.  With o the element-wise
// product:  y_new = ypart + eta DR o s  serves the BFGS skip test, sigma and the new column of V;  the STORED Y is  Ypart + eta S  -- WITHOUT DR: the
// reference hands S to RecalcY in the place of DR o S (:864) -- with the CURRENT eta in every column, and D, L are those of (S, that Y).  Nothing is
// recomputed over the vectors here: with G = S^T Ypart (diagonal GD, strictly lower part GL), S^T S and, when special, R = S^T (DR o S), which grow by
// one row and column per push like D, L, S^T S of a plain history,
//   D_j = fma(eta, (S^T S)_jj, G_jj)      L_ij = fma(eta, (S^T S)_ij, G_ij)  (i > j)
// for any eta.  LbState keeps its layout (D, L are the recomputed ones, so lbfgs_get serves them unchanged); what the restoration phase adds is a second
// plain value, LbResto, that travels with it: copied, assigned and compared as a whole, backed up with it.
//   BFGS   V takes only a new last column  v = y_new / sqrt(s^T y_new)  (:440-451): older columns keep the eta and the scale of THEIR push, so per stored
//          pair eta_col[j] and dv[j] = 1 / sqrt(s^T y_new) are kept and V_j = (Ypart_j + eta_col[j] DR o S_j) dv[j] is formed from the ring.
//          d = D^(-1/2) of the recomputed D, M = Lt Lt^T + sigma S^T S, or + eta R when special; U = sigma S C + V Lbar, or eta (DR o S) C + V Lbar.
//          The push is SKIPPED, nothing but the counter changes, when the recomputed min D is not > 0 (:387-399; a NaN counts).  special: sigma stays -1.
//   SR1    no curvature test; sigma by lb_sr1_sigma on (s^T s, s^T y_new, y_new^T y_new) unless special; Z = D + L + L^T - sigma S^T S, or - eta R;
//          W = Y - sigma S, or Y - eta DR o S, Y the stored one above.  dv is not used (0).
// The reference's |s|_max < 100 eps skip (:350-357) and its limited_memory_max_skipping reset stay with the caller.
struct LbResto {
    double eta = -1.0;                  // of the last stored push (the reference's last_eta_ starts at -1)
    double GD[LBH_MAX] = {}, GL[LBH_MAX * LBH_MAX] = {}, R[LBH_MAX * LBH_MAX] = {}, eta_col[LBH_MAX] = {}, dv[LBH_MAX] = {};
};
// the downloaded dots of a resto push, over the m pairs stored before it (oldest first): sS = s^T S_j, sYp = s^T Ypart_j, sR = s^T (DR o S_j) (read
// only when special); ss = s^T s, syp = s^T ypart, ypyp = ypart^T ypart, sDs = s^T (DR o s), ypDs = ypart^T (DR o s), DsDs = (DR o s)^T (DR o s)
struct LbRestoDots { const double *sS, *sYp, *sR; double ss, syp, ypyp, sDs, ypDs, DsDs; };
static constexpr int LBH_NDOT_RESTO = 3 * LBH_MAX + 6;                 // the dots in the order of LbRestoDots
static constexpr int LBH_NCOEF_RESTO = LBH_NCOEF + LBH_MAX;            // dv, C, Lbar (the layout of LBH_NCOEF, dv in the place of d), then eta_col

inline LbParams lb_params_resto(int type, int special, int max_history, int init, double init_val, double smin, double smax)
{ LbParams P = lb_params(type, max_history, init, init_val, smin, smax); P.resto = 1; P.special = special ? 1 : 0; return P; }
inline LbState lb_fresh_resto(const LbParams& P) { LbState st; st.sigma = P.special ? -1.0 : P.init_val; return st; }
inline double lb_resto_sy(const LbRestoDots& d, double eta) { return std::fma(eta, d.sDs, d.syp); }                                  // s^T y_new
inline double lb_resto_yy(const LbRestoDots& d, double eta) { return std::fma(eta, std::fma(eta, d.DsDs, 2.0 * d.ypDs), d.ypyp); }   // y_new^T y_new

// the candidate of a push: G, S^T S, R, eta_col, dv take the new pair (augment / shift), then D, L are recomputed at eta.  Returns the new m.
inline int lb_resto_store(const LbParams& P, LbState& c, LbResto& r, const LbRestoDots& d, double eta, double dv_new)
{
    const int ld = LBH_MAX, m0 = c.m, full = m0 == P.max_history;
    if (full) for (int j = 0; j + 1 < m0; ++j) { r.eta_col[j] = r.eta_col[j + 1]; r.dv[j] = r.dv[j + 1]; }
    if (P.special) {                                                  // R like S^T S in lb_store
        int m = m0, off = 0;
        if (full) {
            for (int j = 0; j + 1 < m; ++j) for (int i = 0; i + 1 < m; ++i) r.R[i + j * ld] = r.R[i + 1 + (j + 1) * ld];
            off = 1; --m;
        }
        for (int j = 0; j < m; ++j) r.R[m + j * ld] = r.R[j + m * ld] = d.sR[j + off];
        r.R[m + m * ld] = d.sDs;
    }
    const int m = lb_store(m0, P.max_history, r.GD, r.GL, c.STS, d.sS, d.sYp, d.ss, d.syp);
    r.eta = eta; r.eta_col[m - 1] = eta; r.dv[m - 1] = dv_new;
    for (int j = 0; j < m; ++j) {
        c.D[j] = std::fma(eta, c.STS[j + j * ld], r.GD[j]);
        for (int i = 0; i < m; ++i) c.L[i + j * ld] = i > j ? std::fma(eta, c.STS[i + j * ld], r.GL[i + j * ld]) : 0.0;
    }
    c.m = m;
    return m;
}

// coef: LBH_NCOEF_RESTO doubles (zeroed here; valid on LB_PUSH_STORED only).  Works on a copy: a skip -- the curvature test on (s, y_new), or a
// recomputed D_j that is not > 0 -- leaves st, rs untouched but for st.skipped + 1.  LB_PUSH_NOT_PD: the pair, its eta and dv ARE stored.
inline int lb_push_bfgs_resto(const LbParams& P, LbState& st, LbResto& rs, const LbRestoDots& d, double eta, double* coef)
{
    const double sy = lb_resto_sy(d, eta), yy = lb_resto_yy(d, eta);
    if (lb_skip(d.ss, sy, yy)) { ++st.skipped; return LB_PUSH_SKIPPED; }
    LbState c = st; LbResto r = rs;
    if (st.m == P.max_history) c.head = lb_slot(P, st, 1);
    const int m = lb_resto_store(P, c, r, d, eta, 1.0 / std::sqrt(sy));
    for (int j = 0; j < m; ++j) if (!(c.D[j] > 0.0)) { ++st.skipped; return LB_PUSH_SKIPPED; }
    c.skipped = 0;
    c.sigma = P.special ? -1.0 : lb_sigma(P.init, P.init_val, P.smin, P.smax, d.ss, sy, yy);
    st = c; rs = r;
    for (int e = 0; e < LBH_NCOEF_RESTO; ++e) coef[e] = 0.0;
    double dd[LBH_MAX];
    const bool ok = lb_coefficients(m, P.special ? rs.R : st.STS, st.L, LBH_MAX, st.D, P.special ? eta : st.sigma, dd, coef + LBH_MAX, coef + LBH_MAX + LBH_MAX * LBH_MAX, LBH_MAX);
    for (int j = 0; j < m; ++j) { coef[j] = rs.dv[j]; coef[LBH_NCOEF + j] = rs.eta_col[j]; }
    return ok ? LB_PUSH_STORED : LB_PUSH_NOT_PD;
}

// as lb_push_sr1: LB_PUSH_SKIPPED leaves st, rs untouched but for skipped + 1 and invalidates the backup; LB_PUSH_FAILED changes nothing; LB_PUSH_STORED:
// (backup, rs_backup) = (st, rs) as they were
inline int lb_push_sr1_resto(const LbParams& P, LbState& st, LbResto& rs, LbState& backup, LbResto& rs_backup, bool& backup_valid, const LbRestoDots& d, double eta)
{
    const double sy = lb_resto_sy(d, eta), yy = lb_resto_yy(d, eta);
    if (!std::isfinite(d.ss) || !std::isfinite(sy) || !std::isfinite(yy)) { ++st.skipped; backup_valid = false; return LB_PUSH_SKIPPED; }
    LbState c = st; LbResto r = rs;
    const int m = lb_resto_store(P, c, r, d, eta, 0.0);
    c.sigma = P.special ? -1.0 : lb_sr1_sigma(P.init, P.init_val, m, d.ss, sy, yy);
    for (int e = 0; e < LBH_MAX * LBH_MAX; ++e) { c.Qs[e] = 0.0; if (e < LBH_MAX) c.E[e] = 0.0; }
    const int rc = lb_sr1_coefficients(m, P.special ? r.R : c.STS, c.L, LBH_MAX, c.D, P.special ? eta : c.sigma, c.E, c.Qs, LBH_MAX, &c.nneg);
    if (rc == LB_SR1_FAILED) return LB_PUSH_FAILED;
    if (rc == LB_SR1_SKIP) { ++st.skipped; backup_valid = false; return LB_PUSH_SKIPPED; }
    if (st.m == P.max_history) c.head = lb_slot(P, st, 1);
    c.skipped = 0;
    backup = st; rs_backup = rs; backup_valid = true; st = c; rs = r;
    return LB_PUSH_STORED;
}

inline int lb_undo_resto(LbState& st, LbResto& rs, const LbState& backup, const LbResto& rs_backup, bool& backup_valid)
{
    if (!lb_undo(st, backup, backup_valid)) return 0;
    rs = rs_backup;
    return 1;
}

} // namespace mi355x
