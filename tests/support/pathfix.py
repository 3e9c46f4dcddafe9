"""The fixtures of the fast-path A/B tests (tests/test_reach.py on the host, tests/test_gpu_fast_paths.py on the device) and their high-precision
reference solutions.  A fixture is the smallest system found to REACH the path it is used for (tests/support/reach.py says what it reaches); its
data -- matrix, right-hand sides, reference, inertia -- are computed once per process and shared, unchanged, by every test that needs them."""
import functools
import os

import numpy as np

from tests.support import kktgen

LA_TUNE = "la_min_nt=3,la_min_tiles=0"        # look-ahead on fronts of >= 3 tile rows, however few tiles are split (the default asks for 8 rows / 4 000 tiles)

# name -> (generator, solver options, MI355X_KKT_TUNE or None)
FIXTURES = {
    # one dense clique + 100 constraint rows: ONE chain of 31 big fronts, orders 173 .. 1703, 14 above 1024 rows, 5 with >= 12 tile rows of 128
    "clique1700": (lambda: kktgen.clique_kkt([1700], 0, 100, seed=1), {}, None),
    # two disjoint cliques whose chains hold a front of order exactly 1024 and one of 1025: both sides of the big_split edge on one level
    "clique_edge": (lambda: kktgen.clique_kkt([1201, 1202], 0, 120, seed=1), {}, None),
    # a clique without constraint rows -- a chain of pure in-place links (chain groups of several links, selfasm) whose group-end updates above 1024 rows
    # are split by the look-ahead -- beside a small grid, whose handful of small fronts per level then ride on the side stream
    "clique_grid": (lambda: kktgen.block_diag(kktgen.clique_kkt([1700], 0, 0, seed=1), kktgen.grid_kkt(24, 24, dof=3, ncon=2, seed=15)), {}, LA_TUNE),
    "grid24": (lambda: kktgen.grid_kkt(24, 24, dof=3, ncon=2, seed=15), {}, None),
    "grid30": (lambda: kktgen.grid_kkt(30, 30, dof=3, ncon=2, seed=3), {}, None),
    "grid48x44": (lambda: kktgen.grid_kkt(48, 44, dof=3, ncon=2, seed=3), {}, None),
    "grid64x56": (lambda: kktgen.grid_kkt(64, 56, dof=3, ncon=2, seed=3), {}, None),
    "grid110x90_la": (lambda: kktgen.grid_kkt(110, 90, dof=3, ncon=2, seed=31), {}, LA_TUNE),
    "grid110x90_wide": (lambda: kktgen.grid_kkt(110, 90, dof=3, ncon=2, seed=31), dict(wide_panels=1), None),
    "lukvl1000": (lambda: kktgen.lukvl_like(1000, seed=11), {}, None),
    "lukvl12000": (lambda: kktgen.lukvl_like(12000, seed=11), {}, None),
    "lukvl40000": (lambda: kktgen.lukvl_like(40000, seed=41), {}, None),
}
DENSE_MAX = 5000      # up to here the reference is a dense LAPACK solve (SuperLU above)
EIG_MAX = 3000        # up to here the inertia is also counted from LAPACK's eigenvalues


# The A/B table.  (knob, fixture, reach: "plan" = the exported plan differs between the legs | "info" = info() tells them apart | "inferred" = only
# the structural precondition can be shown, equality class of the two legs' solutions, the one-line reason read off the two kernels)
BITWISE, ROUNDING, OTHER_PIVOTS = "bitwise", "rounding", "other pivots"

# (knob, fixture, reach: observed in the plan | inferred from its precondition, equality class, why)
TABLE = [
    ("tfuse", "grid24", "plan", BITWISE,
     "k_big_schur64 / k_big_schur write tv - acc either way: tv is the assembled block, or (tfuse) the children added in list order from 0 as the assembly kernels add them to the T columns, which carry no A entries; acc is the same product"),
    ("tfuse", "clique1700", "plan", BITWISE, "as above, on the 128 x 128 update of the fronts above 1024 rows too"),
    ("tfuse", "clique_edge", "plan", BITWISE, "as above, fronts of order 1024 and 1025 on one level"),
    ("grouped", "grid24", "plan", BITWISE, "groups of ONE link: k_grp_fused factors the pivot block with big_diag_body and solves the rows with k_big_trsm's arithmetic, as the per-link launches do"),
    ("grouped", "clique1700", "plan", BITWISE, "as above; fronts on both sides of 1024 rows"),
    ("grouped", "clique_edge", "plan", BITWISE, "as above; big_split = 1 on the level of the 1024 / 1025 fronts in the plain leg"),
    ("grouped", "grid30", "plan", ROUNDING,
     "groups of several links: a pivot-row block of k_grp_fused loads its own pivot block and adds link q's A entries at the START, the updates of the links before q are subtracted afterwards, (x + a) - u; the per-link launches subtract link p's narrow update first and add the A entries when link q is factored, (x - u) + a"),
    ("grouped", "clique_grid", "plan", ROUNDING, "as above; groups of up to four in-place links"),
    ("selfasm", "grid30", "plan", ROUNDING,
     "the A entries of a pure in-place link are one addition per entry in its own kernels as in the assembly kernel -- but P.grouped needs selfasm (launch_plan.cpp), so the plain leg is also the per-link schedule: the order of `grouped` above"),
    ("selfasm", "clique_grid", "plan", ROUNDING, "as above, 24 in-place links"),
    ("xcd_tiles", "clique1700", "plan", BITWISE, "tile order only: every tile is computed by one workgroup, whichever comes first"),
    ("xcd_tiles", "clique_grid", "plan", BITWISE, "as above, with the second table of a split update"),
    ("xcd_affine", "grid48x44", "inferred", BITWISE, "workgroup-to-front order only (k_big_schur64, k_big_trsm over >= 16 fronts)"),
    ("fuse_upd", "grid64x56", "plan", BITWISE, "the narrow update tiles ride in k_big_diag_trsm's launch: the same products in the same k order on the same operands"),
    ("fuse_dt", "grid30", "plan", BITWISE, "pivot block + panel solve in one flag-synchronised launch: the same arithmetic (test_fused_pivot_block_and_panel_solve_is_bitwise_identical)"),
    ("asm_pull", "grid48x44", "inferred", ROUNDING,
     "panel columns: the pull form writes (sum of the children) and adds the A entries behind it, the scatter form zero-fills, adds the A entries FIRST and the children behind them"),
    ("lookahead", "clique_grid", "plan", BITWISE, "part 1 / part 2 of a split update are the same tiles on two streams (test_lookahead_split_updates_are_exact_and_reproducible)"),
    ("p1_small", "clique_grid", "plan", BITWISE, "part 1 in 64 x 64 tiles: the same k order per entry as the 128 x 128 tiles"),
    ("side_small", "clique_grid", "plan", BITWISE, "stream only: the same launches on a third stream"),
    ("norestore", "clique_grid", "inferred", BITWISE, "only the safety copy of a pivot block is left out; no pivot block of this fixture is rejected"),
    ("front_df", "lukvl1000", "plan", ROUNDING,
     "the fronts of order 17 .. 32: k_front_df eliminates them in natural order on one wavefront (front_lds32_body: pivot reciprocal, rank-1 updates by half-wavefronts), the per-level schedule hands them to the strict k_front_reg<64, 4> (pivot search, register tiles) -- the same pivot statistics here, another operation order per entry; the fronts of order <= 16 run front_dpp16_body either way"),
    ("pair_solve", "lukvl12000", "plan", ROUNDING,
     "k_fwd<64> / k_bwd<64> sum every dot product in two interleaved accumulators (even and odd columns, a0 + a1), k_fwd_pair / k_bwd_pair in one accumulator in column order"),
    ("fastpiv", "grid24", "info", OTHER_PIVOTS, "pivot blocks of the big fronts: blocked LDL^T in natural order accepted a posteriori against the strict Bunch-Kaufman loop -- another factorisation"),
    ("fastpiv", "lukvl1000", "plan", OTHER_PIVOTS, "static-order kernels of the small fronts (with the leaf chains and data-flow runs built on them) against the strict loop: another factorisation"),
    ("fastpiv", "lukvl40000", "plan", OTHER_PIVOTS, "as above; the plain leg is where k_front_reg<64, 2> runs (>= 2 048 fronts of order <= 16 on a level)"),
]
# `optimistic` is read at the first factorisation of a process: both legs in a fresh child each (reach inferred: leaf chains / data-flow runs / dropped strict launches)
OPTIMISTIC = [
    ("lukvl1000", ROUNDING, "the data-flow run is part of the optimistic schedule only: the order of `front_df` above (fronts of order 17 .. 32 by another kernel); the leaf chains and the strict launches left out change no bit"),
    ("lukvl40000", ROUNDING, "as above; the plain leg runs k_front_reg<64, 2> behind the static-order kernel, which finds every front done"),
]


class knobs:
    """MI355X_KKT_DISABLE / MI355X_KKT_TUNE for the duration of a block (both are read when a handle is set up, and at every get_launch_plan)"""
    def __init__(self, disable=None, tune=None):
        self.new = {"MI355X_KKT_DISABLE": disable, "MI355X_KKT_TUNE": tune}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.new}
        for k, v in self.new.items():
            os.environ.pop(k, None)
            if v:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def refined_solve(K, B):
    """(reference, plain fp64 solve) of K X^T = B^T: a dense LAPACK (n <= DENSE_MAX) or SuperLU factorisation, refined with residuals formed in
    numpy.longdouble until the correction stops shrinking.  The plain solve is returned beside it: a fixture qualifies only where the two agree
    to 1e-9, so that the conditioning cannot hide a kernel's error behind the forward-error cap."""
    import scipy.linalg as sla
    import scipy.sparse.linalg as spla
    n = K.shape[0]
    if n <= DENSE_MAX:
        Kd = K.toarray()
        lu = sla.lu_factor(Kd)
        solve = lambda r: sla.lu_solve(lu, r)
        Kl = Kd.astype(np.longdouble)
        resid = lambda b, x: b - Kl @ x
    else:
        lu = spla.splu(K.tocsc())
        solve = lu.solve
        C = K.tocoo()
        row, col, val = C.row, C.col, C.data.astype(np.longdouble)

        def resid(b, x):
            r = b.copy()
            np.subtract.at(r, row, val * x[col])
            return r
    ref, plain = [], []
    for b in np.atleast_2d(B):
        bl = b.astype(np.longdouble)
        x0 = solve(b)
        x, last = x0.astype(np.longdouble), np.inf
        for _ in range(12):
            d = solve(np.asarray(resid(bl, x), dtype=np.float64))
            step = float(np.abs(d).max())
            if not step < 0.5 * last:        # the correction no longer shrinks: x is at the accuracy of its own representation
                break
            x, last = x + d.astype(np.longdouble), step
        ref.append(np.asarray(x, dtype=np.float64)); plain.append(x0)
    return np.stack(ref), np.stack(plain)


@functools.lru_cache(maxsize=None)
def system(name):
    """the fixture's data: triplets, scipy matrix, the three right-hand sides (K 1, a random vector, K random), the inertia by construction,
    solver options and tunables"""
    gen, opts, tune = FIXTURES[name]
    n, r, c, v, neg = gen()
    K = kktgen.to_scipy(n, r, c, v)
    rng = np.random.default_rng(4)
    B = np.stack([K @ np.ones(n), rng.standard_normal(n), K @ rng.standard_normal(n)])
    for a in (B, v):
        a.setflags(write=False)
    return dict(name=name, n=n, r=r, c=c, v=v, neg=neg, K=K, B=B, opts=dict(opts), tune=tune)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(reference solutions, plain fp64 solutions, negative eigenvalues by LAPACK or None) of the fixture -- computed once, never written to"""
    S = system(name)
    ref, plain = refined_solve(S["K"], S["B"])
    eig_neg = int((np.linalg.eigvalsh(S["K"].toarray()) < 0).sum()) if S["n"] <= EIG_MAX else None
    ref.setflags(write=False); plain.setflags(write=False)
    return ref, plain, eig_neg
