"""The fixtures of the big-front solve tests (tests/test_big_solve_reach.py on the host, tests/test_gpu_big_solve.py on the device): systems whose fronts
above 128 rows have PRESCRIBED edge shapes -- chains of more than 64 links, narrow links, rows beyond a chain on both sides of 64 and of 256, a chain head
that gathers more than four children, a panel wider than 64 columns, solve units of several narrow links and of exactly 256 columns, more than 768 rows
beyond a unit -- and go through every big-front solve kernel of kernels_solve.hip.inc on three legs (LEGS).  tests/support/reach.py solve_reach says
what a leg launches.  Data and references are computed once per process and never written to."""
import functools

import numpy as np

import ipopt_amd
from tests.support import kktgen, pathfix

# leg -> (solver options on top of the fixture's, MI355X_KKT_TUNE, MI355X_KKT_DISABLE)
# (chain_solve_maxc=1 cannot stand in for chain_solve: a tree with one front per level keeps its segment under it)
LEGS = {
    "sweeps": ({}, None, None),                           # default schedule: the segments go to k_fwd_chain / k_bwd_chain
    "levels": ({}, None, "chain_solve"),                  # every level launched on its own: k_fwd_solo64 / k_fwd_solo / k_fwd_grp + k_fwd_grp_upd, k_bwd_dot64 + k_bwd_fin64
    "groups": (dict(solve_group=1), None, None),          # one solve unit per chain group: k_fwd_grp + k_fwd_grp_upd, k_bwd_grp_dot + k_bwd_grp
}


def _tails():
    return kktgen.block_diag(*([kktgen.clique_kkt([s + 189, s + 130], s, 0, seed=s) for s in (255, 256, 257)] +
                               [kktgen.clique_kkt([s + 140, s + 130], s, 0, seed=s) for s in (63, 64, 65)]))


# name -> (generator, solver options, columns handed to delay_columns after the analysis (1-based) or None, legs)
FIXTURES = {
    "chain_long2": (lambda: kktgen.clique_kkt([330], 0, 0, seed=2), dict(max_sn_cols=2), None, ("sweeps", "levels")),
    "chain_long7": (lambda: kktgen.clique_kkt([600], 0, 0, seed=1), dict(max_sn_cols=8), None, ("sweeps", "levels", "groups")),
    # the two fixtures that solve on an EDITED structure.  Of 30-odd delay sets tried on this system (a plain one such as (5, 70, 71, 200, 333) gives k in
    # {62, 63, 64}), these two were kept: the first overfills a 64-column link, which splits off a ONE-column link of a front of 160 rows in the middle
    # of the chain (k in {1, 60 .. 64}, 9 links); the second moves 4 / 3 / 2 / 1 columns out of four consecutive links, which leaves a chain group of
    # four links of 64 columns: a solve unit of exactly 256 columns
    "chain_delayed": (lambda: kktgen.clique_kkt([600], 0, 0, seed=1), {}, (332, 486, 458, 478, 350, 513, 172), ("sweeps", "levels", "groups")),
    "chain_delayed256": (lambda: kktgen.clique_kkt([600], 0, 0, seed=1), {}, (190, 191, 192, 193, 253, 254, 255, 316, 317, 379), ("sweeps", "levels", "groups")),
    "tails": (_tails, {}, None, ("sweeps", "levels")),
    "star6": (lambda: kktgen.star_kkt(6, 140, 150, 200, seed=6), {}, None, ("sweeps", "levels", "groups")),
    "wide": (lambda: kktgen.clique_kkt([600], 0, 0, seed=1), dict(wide_panels=1), None, ("sweeps", "levels", "groups")),
    "indef": (lambda: kktgen.clique_kkt([600], 0, 60, seed=1), {}, None, ("sweeps", "levels")),
    # more than 768 rows beyond a unit: four and five 256-row blocks of partial sums, the unrolled-by-four body of the `nch` loops and its remainder
    "tall": (lambda: kktgen.clique_kkt([1100], 0, 0, seed=3), {}, None, ("sweeps", "levels", "groups")),
}
CASES = [(name, leg) for name in FIXTURES for leg in FIXTURES[name][3]]


@functools.lru_cache(maxsize=None)
def system(name):
    """as pathfix.system: triplets, scipy matrix, the three right-hand sides (K 1, a random vector, K random), inertia by construction"""
    gen, opts, delayed, legs = FIXTURES[name]
    n, r, c, v, neg = gen()
    K = kktgen.to_scipy(n, r, c, v)
    rng = np.random.default_rng(4)
    B = np.stack([K @ np.ones(n), rng.standard_normal(n), K @ rng.standard_normal(n)])
    for a in (B, v):
        a.setflags(write=False)
    return dict(name=name, n=n, r=r, c=c, v=v, neg=neg, K=K, B=B, opts=dict(opts), delayed=delayed, legs=legs)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(reference refined with longdouble residuals, plain fp64 solve, negative eigenvalues by LAPACK)"""
    S = system(name)
    assert S["n"] <= pathfix.EIG_MAX
    ref, plain = pathfix.refined_solve(S["K"], S["B"])
    eig_neg = int((np.linalg.eigvalsh(S["K"].toarray()) < 0).sum())
    ref.setflags(write=False); plain.setflags(write=False)
    return ref, plain, eig_neg


def e_plain(name):
    """the discrepancy between plain fp64 LAPACK and the refined reference, relative to max(1, |x_ref|): what the reference itself is good for"""
    ref, plain, _ = reference(name)
    return max(np.abs(plain[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max()) for k in range(3))


def tol_f(name):
    """forward-error bound of the device legs: three digits above the reference's own discrepancy (another elimination order, equilibration, a-posteriori
    pivot acceptance with multipliers up to 1e4 where partial pivoting admits 1), never below 1e-12 nor above the suite's 1e-7"""
    return min(1e-7, max(1e-12, 1000.0 * e_plain(name)))


def leg_knobs(leg):
    """the leg's MI355X_KKT_TUNE / MI355X_KKT_DISABLE, to be held from the set-up of the handle to its last solve"""
    _, tune, disable = LEGS[leg]
    return pathfix.knobs(disable, tune)


def handle(name, leg, **more):
    """a handle analysed (and edited, where the fixture delays columns) for the leg; call under leg_knobs(leg)"""
    S = system(name)
    s = ipopt_amd.KKTSolver(**{**S["opts"], **LEGS[leg][0], **more})
    s.initialize_structure(S["n"], S["r"], S["c"], vals=S["v"])
    if S["delayed"] is not None:
        s.delay_columns(list(S["delayed"]))
    return s
