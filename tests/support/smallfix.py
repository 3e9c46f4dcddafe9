"""The fixtures of the small-front tests (tests/test_small_front_reach.py on the host, tests/test_gpu_small_fronts.py on the device): systems whose
one-wavefront fronts (class FC_WAVE, order <= 32) have PRESCRIBED edge shapes -- leaf chains of 1 .. 16 links up to the 16-level cap, links of more than
48 input entries, a chain count that is no multiple of four, a chain that goes on inside the data-flow run; fronts of order 17 .. 32 with k on both sides
of 16 and k = order = 32, children of 15 .. 18 update rows under a parent of the same run (both tagged-square sizes), more than four gathered children;
tiny pivots at prescribed places, which the static-order kernels must reject -- and go through the factor and solve kernels of the class on seven
legs (LEGS): all but k_front_reg<64, 2>, which launch_plan.cpp gives a level of >= 2 048 fronts of order <= 16 and no system of n <= 1000 can reach.  tests/support/reach.py small_reach says what a leg launches.  Data and references are computed once per process and never written to."""
import functools

import numpy as np

import ipopt_amd
from tests.support import kktgen, pathfix

C, S = kktgen.clique_kkt, kktgen.star_kkt
LEVELS = "chain_solve_maxc=1"      # MI355X_KKT_TUNE: no level is handed to the chain sweeps
# leg -> (MI355X_KKT_TUNE, MI355X_KKT_DISABLE, in a child process)
LEGS = {
    "default": (None, None, False),                          # optimistic schedule: k_leaf_chain + k_front_df; solves by the chain sweeps
    "levels": (LEVELS, None, False),                         # the same factorisation; solves by k_*_leafchain and the pair kernels
    "nopair": (LEVELS, "pair_solve", False),                 # solves by k_fwd<64> / k_bwd<64>
    "noleaf": (LEVELS, "leafchain", False),                  # the data-flow run starts at level 0
    "nodf": (LEVELS, "front_df,leafchain", False),           # per-level k_front_dpp16, strict k_front_reg<64, 4> for the orders 17 .. 32
    "strict": (LEVELS, "fastpiv", False),                    # strict kernels only
    "full": (LEVELS, "optimistic", True),                    # the full schedule (`optimistic` is read once per process)
}
IN_PROCESS = [leg for leg in LEGS if not LEGS[leg][2]]
TINY = 1e-6                        # an assembled pivot against O(1) couplings: static-order multipliers ~1e6 > 1 / max(u, pivtolmax, 1e-4) = 1e4

LEAF_OPTS = dict(ordering=2, matching=0, nemin=1, max_sn_cols=4)
PIVOT_OPTS = dict(scaling=0, delay_rounds=0)      # the statistics are the specification's (mirror.py knows no equilibration), and an edit stays local


def _leaf_parts(w8):
    """leaf_edges, and (w8) without the two components whose first front under max_sn_cols=8 has more than 16 rows (it would sit on level 0: no leaf chains)"""
    return [C([16] * 3, 8, 0, seed=1), C([9] * 7, 4, 0, seed=2), C([16], 0, 0, seed=6), C([1], 0, 0, seed=7),
            C([16] * 20, 8, 0, seed=5), C([16, 16, 16], 1, 0, seed=8), C([12] * 5, 6, 0, seed=9), C([3], 0, 0, seed=10),
            C([7] * 2, 3, 0, seed=11)] + ([] if w8 else [C([16] * 4, 12, 0, seed=12)]) + [C([10] * 3, 5, 0, seed=13)] + \
           ([] if w8 else [C([13] * 2, 2, 2, seed=14)]) + [C([2], 0, 0, seed=15), C([5, 6], 1, 0, seed=16), C([16] * 6 + [20] * 3, 8, 0, seed=17)]


def leaf_edges():
    return kktgen.block_diag(*_leaf_parts(False))


def leaf_edges_w8():
    return kktgen.block_diag(*_leaf_parts(True))


def wave_edges():
    return kktgen.block_diag(C([32, 32], 15, 0, seed=1), C([32, 32], 17, 0, seed=2), C([32, 32], 16, 0, seed=3), S(6, 3, 5, 20, seed=4),
                             S(5, 14, 18, 30, seed=5), C([17, 17, 17], 9, 0, seed=6), C([32], 0, 0, seed=7), C([17], 0, 0, seed=8),
                             C([16, 16, 16], 8, 0, seed=9), C([24, 32, 20], 10, 0, seed=10), S(3, 16, 16, 32, seed=11),
                             C([31, 31], 30, 0, seed=12), C([18, 9, 4], 3, 0, seed=13), C([24, 32, 32], 10, 0, seed=15))


# the edited variables (0-based) of the reject fixtures and the kind of front each one sits in: tests/test_small_front_reach.py checks every kind
#   first / middle / last   a link of a leaf chain (k_leaf_chain: `alive = false`); the middle one shares its wavefront with three healthy chains
#   df_two                  BOTH pivots of a front with k = 2 above the leaf chains, child and parent in the data-flow run: the strict kernel must take a 2x2 pivot
#   small / wave            a front of order <= 16 / of order 17 .. 32 (with a child) whose parent is in the same data-flow run: "a rejected front publishes too"
#   all_three               every pivot of a front with k = 3 (the default ordering leaves no front with k = 2): a 2x2 pivot again
LEAF_TINY = {352: "first", 388: "middle", 83: "last", 142: "df_two", 143: "df_two"}
WAVE_TINY = {588: "small", 613: "wave", 150: "all_three", 151: "all_three", 152: "all_three"}


def with_tiny_pivots(base, variables):
    """the matrix of the fixture `base` with the diagonal entries of `variables` chosen so that each of them is TINY in its front AS ASSEMBLED, i.e. after
    the contributions of everything eliminated below that front (a tiny entry of the matrix itself survives only in a leaf front: one child's update
    moves it by O(1)).  The elimination order is the one the analysis of `base` gives under the options of the edited fixture; the contributions are a
    dense Schur complement, front after front, so that an edit below is seen above.  Against O(1) couplings the static-order multipliers are ~1e6."""
    sys_ = FIXTURES[base][0]()
    n, r, c, v, _ = sys_
    K = kktgen.to_scipy(n, r, c, v).toarray()
    s = ipopt_amd.KKTSolver(**REJECT_OPTS[base])
    s.initialize_structure(n, r, c, vals=v)
    T = fronts(s)
    s.close()
    variables = sorted(variables)
    of = front_of(T, variables)
    for f in sorted(set(of)):
        X = [x for x, g in zip(variables, of) if g == f]
        E = T["perm"][:T["colptr"][f]]
        A = K[np.ix_(X, X)] - (K[np.ix_(X, E)] @ np.linalg.solve(K[np.ix_(E, E)], K[np.ix_(E, X)]) if len(E) else 0.0)
        for i, x in enumerate(X):
            K[x, x] += TINY - A[i, i]
    return kktgen.with_diagonal(sys_, variables, [K[x, x] for x in variables])


# name -> (generator, solver options, the fixture it is an edit of or None, legs)
ALL = tuple(LEGS)
REJECT_OPTS = {"leaf_edges": dict(LEAF_OPTS, **PIVOT_OPTS), "wave_edges": dict(PIVOT_OPTS)}
FIXTURES = {
    "leaf_edges": (leaf_edges, LEAF_OPTS, None, ALL),
    "leaf_edges_w8": (leaf_edges_w8, dict(LEAF_OPTS, max_sn_cols=8), None, tuple(IN_PROCESS)),
    "wave_edges": (wave_edges, {}, None, ALL),
    "leaf_reject": (lambda: with_tiny_pivots("leaf_edges", LEAF_TINY), REJECT_OPTS["leaf_edges"], "leaf_edges", ALL),
    "wave_reject": (lambda: with_tiny_pivots("wave_edges", WAVE_TINY), REJECT_OPTS["wave_edges"], "wave_edges", tuple(IN_PROCESS)),
    "band_hostile": (lambda: kktgen.hostile_band_kkt(300, seed=2, frac=0.15, tiny=1e-2) + (None,), dict(pivtol=0.01, **PIVOT_OPTS), None, tuple(IN_PROCESS)),
}
CASES = [(name, leg) for name in FIXTURES for leg in FIXTURES[name][3] if leg in IN_PROCESS]
CHILD_CASES = [(name, leg) for name in FIXTURES for leg in FIXTURES[name][3] if leg not in IN_PROCESS]


@functools.lru_cache(maxsize=None)
def _data(name):
    """the fixture's matrix, right-hand sides and inertia: computed once per process"""
    gen, opts, base, legs = FIXTURES[name]
    n, r, c, v, neg = gen()
    assert n <= 1000
    K = kktgen.to_scipy(n, r, c, v)
    if neg is None:
        neg = int((np.linalg.eigvalsh(K.toarray()) < 0).sum())
    rng = np.random.default_rng(4)
    B = np.stack([K @ np.ones(n), rng.standard_normal(n), K @ rng.standard_normal(n)])
    for a in (B, v):
        a.setflags(write=False)
    return dict(name=name, n=n, r=r, c=c, v=v, neg=neg, K=K, B=B, base=base, legs=legs, u=float(opts.get("pivtol", 1e-8)))


def system(name, opts_of=None):
    """as pathfix.system: triplets, scipy matrix, the three right-hand sides (K 1, a random vector, K random); the inertia by LAPACK's eigenvalues where
    an edit has changed the one by construction.  opts_of: the matrix of `name` under the options of another fixture (the unedited matrix of a reject
    fixture under that fixture's options: what its untouched fronts are compared with).  A dict of the caller's own around the shared, read-only data."""
    return dict(_data(name), opts=dict(FIXTURES[opts_of or name][1]))


@functools.lru_cache(maxsize=None)
def reference(name):
    """(reference refined with longdouble residuals, plain fp64 solve, negative eigenvalues by LAPACK)"""
    Sy = system(name)
    ref, plain = pathfix.refined_solve(Sy["K"], Sy["B"])
    eig_neg = int((np.linalg.eigvalsh(Sy["K"].toarray()) < 0).sum())
    ref.setflags(write=False); plain.setflags(write=False)
    return ref, plain, eig_neg


def relmax(a, b):
    return max(np.abs(a[k] - b[k]).max() / max(1.0, np.abs(b[k]).max()) for k in range(len(a)))


def e_plain(name):
    """the discrepancy between plain fp64 LAPACK and the refined reference, relative to max(1, |x_ref|): what the reference itself is good for"""
    ref, plain, _ = reference(name)
    return relmax(plain, ref)


def tol_f(name):
    """the forward-error bound of tests/support/bigfix.py: three digits above the reference's own discrepancy, never below 1e-12 nor above 1e-7"""
    return min(1e-7, max(1e-12, 1000.0 * e_plain(name)))


def leg_knobs(leg):
    """the leg's MI355X_KKT_TUNE / MI355X_KKT_DISABLE, to be held from the set-up of the handle to its last solve"""
    tune, disable, _ = LEGS[leg]
    return pathfix.knobs(disable, tune)


def handle(name, opts_of=None, **more):
    """a handle analysed for the fixture; call under leg_knobs(leg)"""
    Sy = system(name, opts_of)
    s = ipopt_amd.KKTSolver(**{**Sy["opts"], **more})
    s.initialize_structure(Sy["n"], Sy["r"], Sy["c"], vals=Sy["v"])
    return s


def fronts(s):
    """(first permuted column of every supernode and one past the last, order, pivot columns, parent, level, the permutation: permuted -> original variable)"""
    I = s.info()
    nsn = I.num_sn
    colptr = s.symbolic(1, nsn + 1)
    return dict(colptr=colptr, order=np.diff(s.symbolic(2, nsn + 1)), cols=np.diff(colptr), parent=s.symbolic(4, nsn), level=s.symbolic(5, nsn),
                perm=s.symbolic(0, I.n), cls=s.symbolic(23, nsn))


def front_of(T, variables):
    """the supernode that eliminates each original variable"""
    where = np.empty(len(T["perm"]), dtype=np.int64)
    where[T["perm"]] = np.arange(len(T["perm"]))
    return [int(np.searchsorted(T["colptr"], where[x], side="right") - 1) for x in variables]


def touched(T, variables):
    """mask over the supernodes: the subtree of the front holds an edited variable (its numbers may differ from the unedited system's)"""
    nsn = len(T["parent"])
    hit = np.zeros(nsn, dtype=bool)
    for f in front_of(T, variables):
        while f >= 0 and not hit[f]:
            hit[f] = True; f = int(T["parent"][f])
    return hit


@functools.lru_cache(maxsize=None)
def spec(name, fast=True):
    """the pivoting specification (tests/support/mirror.py factor_solve_pivoted, host only) on the fixture at its own u: (statistics in the order of
    info(): num_neg, num_zero, num_two, num_delay; the supernodes whose pivot order is not the natural one or that hold a 2x2 pivot -- what the strict
    kernels leave behind where a static-order kernel has rejected a front; the solutions of the three right-hand sides).  fast=False: the strict rule
    on every front, as under MI355X_KKT_DISABLE=fastpiv."""
    from tests.support import mirror
    Sy = system(name)
    s = handle(name)
    sym = mirror.fetch(s)
    u = Sy["u"]
    xs = []
    for k in range(3):
        x, st = mirror.factor_solve_pivoted(sym, np.array(Sy["v"]), Sy["B"][k], u=u, u2=max(u, 1e-4), fast_blocks=fast, debug=(k == 0))
        if k == 0:
            odd = tuple(int(f) for f, c0, kk, m, P, pt, d in st["dbg"] if not np.array_equal(P, np.arange(kk)) or (np.asarray(pt) != 1).any())
            stats = (st["num_neg"], st["num_zero"], st["num_two"], st["num_delay"])
        xs.append(x)
    s.close()
    xs = np.stack(xs); xs.setflags(write=False)
    return stats, odd, xs


def spec_error(name):
    """the specification's own forward error against the refined reference, relative to max(1, |x_ref|)"""
    return relmax(spec(name)[2], reference(name)[0])


def fwd_bound(name):
    """the forward-error bound of a device leg: tol_f; on band_hostile, where u = 0.01 admits multipliers of 100, not below ten times the error of the
    specification (the same pivots in numpy) -- both terms come from references, never from the device"""
    return max(tol_f(name), 10.0 * spec_error(name)) if name == "band_hostile" else tol_f(name)
