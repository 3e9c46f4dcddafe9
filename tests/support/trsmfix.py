"""The fixtures of the trsm_regs A/B tests (tests/test_trsm_regs_reach.py on the host, tests/test_gpu_trsm_regs.py on the device): the smallest systems
that reach each branch of trsm_rows_regs (kernels_big.hip.inc), with their right-hand sides and longdouble-refined references, computed once per
process and never written to.

BASE: an FO_TRSM record -- a pivot-block launch followed by k_big_trsm -- is what a level of MANY big fronts gets (synth_1e6: 28 per factorisation).
The levels of these small systems hold a handful of fronts, which the default plan gives to k_grp_fused (chain groups) and k_big_diag_trsm (fuse_dt:
pivot block + panel solve in one launch), both on trsm_rows_impl: none of them has an FO_TRSM record by default (tests/test_trsm_regs_reach.py
shows the counts).  Both legs of every test therefore run with MI355X_KKT_DISABLE=grouped,fuse_dt -- the per-link schedule, FO_DIAG_REG + FO_TRSM on
every level of big fronts -- and differ in `trsm_regs` alone."""
import functools

import numpy as np

from tests.support import kktgen, pathfix

BASE = "grouped,fuse_dt"
KNOB = "trsm_regs"
FWD_TOL = 1e-7             # forward error against the refined reference, relative to max(1, |x_ref|) (tests/test_gpu_fast_paths.py)
FWD_TOL_HOSTILE = 1e-6     # the hostile grid's cap (tests/test_gpu_pivoting.py test_hostile_grid_hip_equals_the_specification)


def _hostile(u):
    return dict(gen=lambda: kktgen.hostile_grid_kkt(16, 16, seed=3) + (None,), opts=dict(pivtol=u, scaling=0, pivtolmax=max(u, 1e-4), delay_rounds=0),      # (static pivoting: ONE factorisation is compared)
                fwd=FWD_TOL_HOSTILE, hostile=u)


def _clique(msc):
    return dict(gen=lambda: kktgen.clique_kkt([331], 0, 0, seed=2), opts=dict(max_sn_cols=msc), fwd=FWD_TOL, hostile=None)


# name -> generator, solver options, forward-error cap; what it reaches: see the table in tests/test_gpu_trsm_regs.py
FIXTURES = {
    "grid24": dict(gen=pathfix.FIXTURES["grid24"][0], opts={}, fwd=FWD_TOL, hostile=None),
    "clique331_sn8": _clique(8),
    "clique331_sn40": _clique(40),
    "clique331_sn64": _clique(64),
    "hostile_1e-8": _hostile(1e-8),
    "hostile_0.01": _hostile(0.01),
}


@functools.lru_cache(maxsize=None)
def system(name):
    """triplets, scipy matrix, the three right-hand sides of pathfix.system (K 1, a random vector, K random), inertia by construction or None"""
    F = FIXTURES[name]
    n, r, c, v, neg = F["gen"]()
    K = kktgen.to_scipy(n, r, c, v)
    rng = np.random.default_rng(4)
    B = np.stack([K @ np.ones(n), rng.standard_normal(n), K @ rng.standard_normal(n)])
    for a in (B, v):
        a.setflags(write=False)
    return dict(name=name, n=n, r=r, c=c, v=v, neg=neg, K=K, B=B, opts=dict(F["opts"]), fwd=F["fwd"], hostile=F["hostile"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """(longdouble-refined reference solutions, plain fp64 LAPACK solutions) -- pathfix.refined_solve"""
    S = system(name)
    ref, plain = pathfix.refined_solve(S["K"], S["B"])
    ref.setflags(write=False); plain.setflags(write=False)
    return ref, plain
