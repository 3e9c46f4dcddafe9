// kernels_qn_pair.hip.inc -- the quasi-Newton pair (s, y) from the device-resident Jacobians (IpLimMemQuasiNewtonUpdater.cpp:276-308):
//   s[j] = x[j] - x_last[j]
//   y[j] = (grad_f[j] - gf_last[j]) + sum over the entries (i, u) of column j of [J_c; J_d], in view order, of (J_cur[u] - J_last[u]) * lam[i]
// lam = y_c | y_d, J_cur the CURRENT sources of the J_c / J_d assembly segments, J_last their snapshot (qn_pair_store).  The difference is taken PER
// ENTRY (a stated deviation from the reference's four separate transposed products, :297-300 / :304-307): an entry that did not change contributes an
// exact 0, the cancellation happens before the multiplication.  RESTO: the restoration variant, y is ypart (no gradient term; gf, gfl are not read).
// The column view (qn_pair_host.h QpView) is what makes y a GATHER: one column per group of LPC lanes, no atomics on doubles, every sum in a fixed
// order => bitwise reproducible.  Lane `sub` of a group walks the entries sub, sub + LPC, ... of its column sequentially; the partial sums meet in the
// xor-shuffle tree (the shape of k_ruiz_sweep<LPR>), lane 0 adds the gradient difference and writes.  Per entry: ONE 8-byte load of (i, u), two 8-byte
// values through u, the gathered lam[i]; per column five streamed vectors (x, x_last, gf, gf_last in; s, y out: six with both outputs).
// Bounds: ptr, ent come from qp_build on triplets qp_check has passed: i < nc + nd, u < len_jc + len_jd, ptr[nx] = len_jc + len_jd.
struct QpDev {
    int nx, len_jc;
    const int* ptr; const int2* ent;
    const double *jc, *jd, *jlast, *lam;            // jc: u < len_jc reads jc[u]; jd: otherwise jd[u - len_jc]
    const double *x, *xl, *gf, *gfl;
    double *s, *y;
};
template <int LPC, bool RESTO>
__global__ __launch_bounds__(256) void k_qn_pair(QpDev Q)
{
    constexpr int CPW = 64 / LPC;                                   // columns per wavefront
    const int sub = threadIdx.x & (LPC - 1);
    const long long ncol = ((long long)Q.nx + CPW - 1) / CPW * CPW;       // padded: a wavefront leaves the loop as a whole, every lane of a shuffle group reaches the shuffle
    const long long stride = ((long long)gridDim.x * blockDim.x) / LPC;
    for (long long j = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / LPC; j < ncol; j += stride) {
        double acc = 0.0;
        if (j < Q.nx) {
            const int p1 = Q.ptr[j + 1];
            for (int p = Q.ptr[j] + sub; p < p1; p += LPC) {
                const int2 e = Q.ent[p];
                const double cur = e.y < Q.len_jc ? Q.jc[e.y] : Q.jd[e.y - Q.len_jc];
                acc += (cur - Q.jlast[e.y]) * Q.lam[e.x];
            }
        }
#pragma unroll
        for (int m = 1; m < LPC; m <<= 1) acc += __shfl_xor(acc, m);
        if (j < Q.nx && sub == 0) {
            Q.s[j] = Q.x[j] - Q.xl[j];
            Q.y[j] = RESTO ? acc : (Q.gf[j] - Q.gfl[j]) + acc;
        }
    }
}
// max |s| over the `rows` indices of the row map (map != null), or over the first `rows` entries: the order-preserving atomicMax on the bit pattern
// (pd_amax: one atomic per wavefront, NaN counts as +inf).  Max is exact and order independent => deterministic.  *acc is zeroed before the launch.
__global__ __launch_bounds__(256) void k_qn_amax(const double* s, int rows, const int* map, unsigned long long* acc)
{
    const long long npad = ((long long)rows + 63) / 64 * 64;        // (whole wavefronts: pd_amax reduces over all 64 lanes)
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npad; i += (long long)gridDim.x * blockDim.x)
        pd_amax(acc, i < rows ? s[map ? map[i] : i] : 0.0);
}
