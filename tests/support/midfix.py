"""The fixtures of the mid-front solve tests (tests/test_mid_solve_reach.py on the host, tests/test_gpu_mid_solve.py on the device): systems whose
fronts of order 33 .. 128 (classes FC_LDS64 / FC_LDS128) go through the LEVEL launches of the solve sweeps -- k_fwd_mid / k_bwd_mid, or k_fwd / k_bwd
under MI355X_KKT_DISABLE=mid_solve -- and not through the chain sweeps.  Data and references are computed once per process and never written to."""
import functools

import numpy as np

from tests.support import kktgen, pathfix, reach as R

NO_CHAINS = "chain_solve_maxc=1"      # MI355X_KKT_TUNE: no level is handed to the chain sweeps

# name -> (generator, solver options, MI355X_KKT_TUNE, MI355X_KKT_DISABLE of BOTH legs)
FIXTURES = {
    # both edges of both classes (order 33, 64, 65, 128), k = 16 / 17 / 63 / 64, k = order (no update rows), fronts with and without a child
    "mid_edges": (lambda: kktgen.block_diag(
        kktgen.clique_kkt([33], 0, 0, seed=1), kktgen.clique_kkt([64], 0, 0, seed=2), kktgen.clique_kkt([128], 0, 0, seed=3),
        kktgen.clique_kkt([128, 128], 112, 0, seed=4), kktgen.clique_kkt([128, 128], 111, 0, seed=5), kktgen.clique_kkt([65, 65], 49, 0, seed=7),
        kktgen.clique_kkt([64, 64], 48, 0, seed=8), kktgen.clique_kkt([33, 33], 17, 0, seed=9), kktgen.clique_kkt([100], 0, 20, seed=10),
        kktgen.clique_kkt([120], 0, 8, seed=11)), {}, NO_CHAINS, None),
    "grid24": (lambda: kktgen.grid_kkt(24, 24, dof=3, ncon=2, seed=15), {}, None, "chain_solve"),
    # the benchmark's situation in small: mid fronts on level launches next to live chain sweeps, default schedule
    "grid48x44": (lambda: kktgen.grid_kkt(48, 44, dof=3, ncon=2, seed=3), {}, None, None),
    # 2x2 pivots inside fronts of the two classes (strict pivoting, no scaling, no delays); inertia from the factorisation, no accuracy claim
    "hostile16": (lambda: kktgen.hostile_grid_kkt(16, 16, seed=3) + (None,), dict(pivtol=0.01, scaling=0, delay_rounds=0), None, "chain_solve,fastpiv"),
}
# (order, k, children) of the mid fronts of mid_edges, as analysed when the fixture was written
MID_EDGES_SHAPES = [(33, 33, 0), (64, 64, 0), (128, 63, 0), (65, 63, 1), (128, 16, 0), (128, 63, 1), (128, 17, 0), (65, 16, 0), (64, 16, 0), (64, 64, 1),
                    (33, 16, 0), (33, 33, 1), (109, 54, 0), (63, 48, 1), (124, 64, 0)]


def disable_list(name, mid_off):
    base = FIXTURES[name][3]
    return ",".join(x for x in (base, "mid_solve" if mid_off else None) if x) or None


@functools.lru_cache(maxsize=None)
def system(name):
    """as pathfix.system: triplets, scipy matrix, the three right-hand sides (K 1, a random vector, K random), inertia by construction (or None)"""
    gen, opts, tune, _ = FIXTURES[name]
    n, r, c, v, neg = gen()
    K = kktgen.to_scipy(n, r, c, v)
    rng = np.random.default_rng(4)
    B = np.stack([K @ np.ones(n), rng.standard_normal(n), K @ rng.standard_normal(n)])
    for a in (B, v):
        a.setflags(write=False)
    return dict(name=name, n=n, r=r, c=c, v=v, neg=neg, K=K, B=B, opts=dict(opts), tune=tune)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(reference refined with longdouble residuals, plain fp64 solve, negative eigenvalues by LAPACK or None)"""
    S = system(name)
    ref, plain = pathfix.refined_solve(S["K"], S["B"])
    eig_neg = int((np.linalg.eigvalsh(S["K"].toarray()) < 0).sum()) if S["n"] <= pathfix.EIG_MAX else None
    ref.setflags(write=False); plain.setflags(write=False)
    return ref, plain, eig_neg


def mid_fronts(s):
    """the fronts of order 33 .. 128 of an analysed handle under the MI355X_KKT_DISABLE / MI355X_KKT_TUNE of the moment:
    (level launches: list of (class, order, k, children, level, supernode); the same for those on levels inside a chain segment; levels with a live chain sweep)"""
    I = s.info()
    nl, nsn = I.num_levels, I.num_sn
    order = np.diff(s.symbolic(2, nsn + 1)); cols = np.diff(s.symbolic(1, nsn + 1))
    parent, cls, level = s.symbolic(4, nsn), s.symbolic(23, nsn), s.symbolic(5, nsn)
    nchild = np.bincount(parent[parent >= 0], minlength=nsn)
    in_seg = np.zeros(nl, dtype=bool)
    for lv0, lv1, *_ in s.launch_plan("chain_segs").reshape(-1, 9):
        in_seg[lv0:lv1 + 1] = True
    on_level, in_chain = [], []
    for f in np.nonzero((cls == R.FC_LDS64) | (cls == R.FC_LDS128))[0]:
        rec = (int(cls[f]), int(order[f]), int(cols[f]), int(nchild[f]), int(level[f]), int(f))
        (in_chain if in_seg[level[f]] else on_level).append(rec)
    return on_level, in_chain, int(in_seg.sum())
