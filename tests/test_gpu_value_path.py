"""-m gpu: the value path -- everything between the caller's numbers and the factorisation -- against the plain numpy references of
tests/support/value_spec.py (longdouble): the in-solver Ruiz equilibration in its three variants, the keep-the-factors shortcut of
factor_assembled across call histories, the 8-block primal-dual kernels at the shapes where they can go wrong, the segment assembly
and the gather of duplicates.  Every tolerance is a derived bound or a figure the suite already uses; nothing here times anything.

Before the fixes to numeric.hip that came with this file (the assembly marked dirty by factor() / refactor() and by assembly_define,
scale_valid set where the equilibrating sequence is launched) test_keep_history_1 [graph and eager], test_keep_history_2 and
test_keep_history_3 failed: the kept factors were those of another matrix (1, 2), and the shortcut stayed off for good after a
redundant set_scaling(1) (3)."""
import math

import numpy as np
import pytest
import torch      # (before the library is loaded: torch brings its own HIP runtime)

import ipopt_amd
from ipopt_amd import kkt
from tests.support import kktgen, value_spec as vs

pytestmark = pytest.mark.gpu
LD = np.longdouble
U = 2.0 ** -53
RES_TOL = 1e-12           # the suite's scaled-residual bound (tests/test_gpu_parity.py)
# Relative error bound of the Ruiz factors against the longdouble iteration, 16 u:
#   sweep 0,  s = 1 / sqrt(max |a|):  one rounding for the square root, one for the division                         -> 2 u
#   each later sweep,  s_new = s_i / sqrt(s_i * max_j(|a_ij| s_j)) = sqrt(s_i / (|a_ij| s_j)):  the square root HALVES the errors the
#   two factors bring along (e_i / 2 + e_j / 2 <= e), the two products under it cost 2 u / 2, the root and the division 1 u each -> e + 3 u
#   four sweeps: 2 u + 3 * 3 u = 11 u; a position with two duplicates is summed with one more rounding (u / 2 per sweep: 13 u).  Head-room to 16 u.
# This assumes a correctly rounded fp64 sqrt and division on the device: the library is built without any fast-math flag (ipopt_amd/Makefile:
# -O3 only).  A later flag change that relaxes either breaks this bound, and this test is meant to fail then.
RUIZ_TOL = 16 * U


def sres(K, x, b):
    return np.abs(K @ x - b).max() / (abs(K).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max() + 1e-300)


def fresh(n, r, c, vals, b=None, **opts):
    """a new handle given host-assembled values: (handle, status, negative eigenvalues, solution, scaling factors)"""
    s = ipopt_amd.KKTSolver(**opts)
    s.initialize_structure(n, r, c, vals=vals)
    s.values()[:] = vals
    x = None if b is None else b.copy()
    st = s.multi_solve(True, x)
    return s, st, s.number_of_neg_evals(), x, s.get_scaling()


def ruiz_close(got, want):
    err = np.abs(got.astype(LD) / want - 1)
    return float(err.max(initial=0.0))


# ------------------------------------------------------------------------------------------------
# 1. equilibration against the reference
# ------------------------------------------------------------------------------------------------
_SYSTEMS = {}


def _system(name):
    if not _SYSTEMS:
        _SYSTEMS.update(vs.ruiz_systems())
    return _SYSTEMS[name]


@pytest.mark.parametrize("name", ["lukvl_2lanes_fused", "lukvl_2lanes_fused_odd", "grid_8lanes_fused_odd", "grid_8lanes_rowview_odd"])
def test_ruiz_factors_of_each_variant_match_the_longdouble_iteration(name):
    n, r, c, v, variant = _system(name)
    assert vs.ruiz_variant(n, r, c) == variant and n % 8 != 0            # the kernel variant this system is here for (enqueue_scaling)
    s, st, neg, x, f = fresh(n, r, c, v, np.ones(n))
    assert st == 0
    want = vs.ruiz_spec(n, r, c, v)
    err = ruiz_close(f, want)
    print(f"{name}: n = {n}, rslot_len / n = {vs.rslot_len(n, r, c) / n:.2f}, max relative error {err / U:.2f} u")
    assert err <= RUIZ_TOL


def test_ruiz_factors_over_sixteen_orders_of_magnitude():
    n, r, c, v, neg = kktgen.grid_kkt(9, 7, dof=2, ncon=1, seed=2, sigma_exp=8.0)
    s, st, got_neg, x, f = fresh(n, r, c, v, np.ones(n))
    assert st == 0 and got_neg == neg
    err = ruiz_close(f, vs.ruiz_spec(n, r, c, v))
    print(f"sigma_exp = 8: max relative error {err / U:.2f} u")
    assert err <= RUIZ_TOL


def test_a_row_of_stored_zeros_keeps_factor_one_and_the_matrix_is_singular():
    n, r, c, v, neg = kktgen.lukvl_like(101, seed=4)
    row = 37
    v = v.copy(); v[(r == row) | (c == row)] = 0.0
    s, st, _, _, f = fresh(n, r, c, v)
    assert st == kkt.SINGULAR                                             # (the ordinary status of a singular matrix, not a fault)
    want = vs.ruiz_spec(n, r, c, v)
    assert f[row - 1] == 1.0 and float(want[row - 1]) == 1.0
    assert ruiz_close(f, want) <= RUIZ_TOL


def test_ruiz_factors_with_duplicates_and_both_triangles():
    # values are multiples of 2^-10 of moderate size: every sum of duplicates is exact in fp64 whatever the order of the gather
    rng = np.random.default_rng(8)
    n = 37
    pr = rng.integers(1, n + 1, 150); pc = rng.integers(1, n + 1, 150)
    r = np.concatenate([np.arange(1, n + 1), pr, pc[:60], pr[:30]]).astype(np.int32)      # the first 60 again in the OTHER triangle, 30 of them a third time
    c = np.concatenate([np.arange(1, n + 1), pc, pr[:60], pc[:30]]).astype(np.int32)
    v = np.concatenate([64.0 + rng.integers(0, 1024, n), rng.integers(-2048, 2048, 240)]) / 1024.0
    s, st, _, _, f = fresh(n, r, c, v)
    assert (r > c).any() and (r < c).any()
    assert ruiz_close(f, vs.ruiz_spec(n, r, c, v)) <= RUIZ_TOL


def test_ruiz_factor_of_a_one_by_one_system_and_scaling_off():
    one = np.array([1], np.int32)
    s, st, neg, x, f = fresh(1, one, one, np.array([-4.0]), np.array([8.0]))
    assert st == 0 and neg == 1 and f[0] == 0.5 and x[0] == -2.0
    n, r, c, v, neg = _system("lukvl_2lanes_fused")[:4] + (1001,)
    s, st, got_neg, x, f = fresh(n, r, c, v, np.ones(n), scaling=0)
    assert st == 0 and got_neg == neg and np.all(f == 1.0)


@pytest.mark.parametrize("case", ["base0", "duplicates", "one_sweep", "zero_row"])
def test_standalone_ruiz_routine_matches_the_triplet_iteration(case):
    """mi355x_kkt_ruiz_scaling takes the maximum over the TRIPLETS (vs.ruiz_triplet_spec), not over summed entries like the solver: with
    duplicates of one position the two differ, and the reference here is the triplet one.  Same error bound: s = 1 exactly at the start, each
    sweep  s / sqrt(|a| s_i s_j)  inherits e and adds 2 u / 2 + 1 u + 1 u = 3 u."""
    n, r, c, v, _ = kktgen.lukvl_like(257, seed=9)
    base, sweeps = 1, 4
    if case == "base0":
        r, c, base = r - 1, c - 1, 0
    elif case == "duplicates":
        r = np.concatenate([r, [5, 5, 5, 9, 8]]).astype(np.int32); c = np.concatenate([c, [5, 5, 5, 8, 9]]).astype(np.int32)
        v = np.concatenate([v, [1e16, 1.0, -1e16, 50.0, -70.0]])
    elif case == "one_sweep":
        sweeps = 1
    elif case == "zero_row":
        v = v.copy(); v[(r == 100) | (c == 100)] = 0.0
    r = np.ascontiguousarray(r, dtype=np.int32); c = np.ascontiguousarray(c, dtype=np.int32); v = np.ascontiguousarray(v)
    out = np.zeros(n)
    assert kkt.load_library().mi355x_kkt_ruiz_scaling(0, n, len(v), r.ctypes.data, c.ctypes.data, v.ctypes.data, base, sweeps, out.ctypes.data) == 0
    want = vs.ruiz_triplet_spec(n, r, c, v, sweeps=sweeps, base=base)
    assert ruiz_close(out, want) <= RUIZ_TOL
    if case == "zero_row":
        assert out[99] == 1.0
    if case == "duplicates":
        assert ruiz_close(out, vs.ruiz_spec(n, r, c, v)) > 1e-3          # (the summed-entry iteration is another one)


# ------------------------------------------------------------------------------------------------
# 2. the keep-the-factors shortcut across call histories
# ------------------------------------------------------------------------------------------------
class KeepHistory:
    """One handle walked through a history, every factorisation checked against a fresh handle given the same host-assembled values.
      case (a): get_scaling() is the Ruiz factors of the matrix just factored -- bitwise those of the fresh handle -- and status, inertia and
                solution are bitwise the fresh handle's;
      case (b): get_scaling() is bitwise the factors of THIS handle's previous factorisation (and not the fresh handle's); status and inertia
                equal the fresh handle's, scaled residual <= RES_TOL, solution within 1e-9 (the figure of the existing keep-path test)."""

    def __init__(self, **opts):
        self.F = F = vs.keep_fixture()
        self.opts = opts
        self.srcs = (F["hv"], F["Sigma"], F["jv"])
        self.s = ipopt_amd.KKTSolver(**opts)
        self.s.initialize_structure(F["n"], F["r"], F["c"], vals=vs.keep_host_vals(F, 0.0, 0.0))
        self.define(upload=True)
        self.prev = None
        self.delayed = None

    def define(self, upload):
        self.s.assembly_define(self.F["lens"])
        if upload:
            for q, v in enumerate(self.srcs):
                self.s.assembly_set(q, v)
        else:
            self.srcs = tuple(np.zeros_like(v) for v in self.srcs)

    def fresh(self, vals):
        F = self.F
        s2 = ipopt_amd.KKTSolver(**self.opts)
        s2.initialize_structure(F["n"], F["r"], F["c"], vals=vs.keep_host_vals(F, 0.0, 0.0))      # (the analysis the walked handle had: it may look at the values)
        if self.delayed is not None:
            assert s2.delay_columns(self.delayed) == self.moved
        s2.values()[:] = vals
        x2 = F["b"].copy()
        st2 = s2.multi_solve(True, x2)
        return st2, s2.number_of_neg_evals(), x2, s2.get_scaling()

    def check(self, st, neg, x, vals, case):
        F = self.F
        st2, neg2, x2, f2 = self.fresh(vals)
        f = self.s.get_scaling()
        assert (st, neg) == (st2, neg2) and st == 0
        if case == "a":
            assert np.array_equal(f, f2), "the factors are not those of the matrix just factored"
            assert np.array_equal(x, x2)
        else:
            assert self.prev is not None and np.array_equal(f, self.prev), "the factors of the previous factorisation were not kept"
            assert not np.array_equal(f, f2)
            K = kktgen.to_scipy(F["n"], F["r"], F["c"], vals)
            assert sres(K, x, F["b"]) <= RES_TOL
            assert np.abs(x - x2).max() <= 1e-9 * np.abs(x2).max()
        self.prev = f

    def assembled(self, dx, dc, case):
        F = self.F
        st, neg, zero = self.s.factor_assembled(F["scale"], [0.0, dx, 0.0, -dc])
        x = F["b"].copy(); self.s.multi_solve(False, x)
        self.check(st, neg, x, vs.keep_host_vals(F, dx, dc, self.srcs), case)

    def host(self, vals):
        self.s.values()[:] = vals
        x = self.F["b"].copy()
        st = self.s.multi_solve(True, x)
        self.check(st, self.s.number_of_neg_evals(), x, vals, "a")


@pytest.mark.parametrize("use_graph", [1, 0], ids=["graph", "eager"])
def test_keep_history_1_a_host_factorisation_of_another_matrix_in_between(use_graph):
    h = KeepHistory(use_graph=use_graph)
    h.assembled(1e-4, 0.0, "a")
    h.host(vs.keep_other_matrix(h.F))                     # V.scale now belongs to B
    h.assembled(1e-2, 1e-8, "a")                          # same segment scales, nothing uploaded: still not a delta-only retry of the LAST factorisation
    h.assembled(1.0, 1e-8, "b")                           # ... and this one is


def test_keep_history_1_with_the_shortcut_disabled_equilibrates_every_time(monkeypatch):
    monkeypatch.setenv("MI355X_KKT_DISABLE", "keep_scale")
    h = KeepHistory()
    h.assembled(1e-4, 0.0, "a")
    h.host(vs.keep_other_matrix(h.F))
    h.assembled(1e-2, 1e-8, "a")
    h.assembled(1.0, 1e-8, "a")


def test_keep_history_2_assembly_define_zeroes_the_sources():
    h = KeepHistory()
    h.assembled(1e-4, 0.0, "a")
    h.define(upload=False)                                # the sources are zero again, no assembly_set
    h.assembled(2.0, 1.0, "a")                            # the matrix is the shifts alone: diag(2 I, -I), regular


def test_keep_history_3_a_redundant_mode_call_does_not_switch_the_shortcut_off_for_good():
    h = KeepHistory()
    h.assembled(1e-4, 0.0, "a")
    h.s.set_scaling(1)                                    # mode 1 is already active: the captured sequences stay, the factors are asked for afresh
    h.assembled(1e-4, 0.0, "a")
    h.assembled(1e-2, 1e-8, "b")
    h.assembled(1.0, 1e-8, "b")


def test_keep_history_4_delta_only_retries_along_the_whole_ladder():
    """delta_x = 1e-4 * 100^k, k = 0..6, delta_c = 1e-8 from the third on, all with the factors of the first factorisation.  On the kept path
    cnorm stays at the 1 the last equilibration wrote while the diagonal grows by twelve orders of magnitude, so the zero-pivot threshold
    small * cnorm belongs to another matrix: tried over this whole range, status and inertia stay those of a freshly equilibrated handle and the
    residual stays <= RES_TOL, so the kept path does not refresh cnorm."""
    h = KeepHistory()
    h.assembled(0.0, 0.0, "a")
    for dx, dc in vs.KEEP_LADDER:
        h.assembled(dx, dc, "b")


def test_keep_history_5_a_new_pivot_threshold_equilibrates_afresh():
    h = KeepHistory()
    h.assembled(0.0, 0.0, "a")
    h.assembled(1e-4, 0.0, "b")
    h.opts = dict(h.opts, pivtol=1e-6); h.s.set_pivtol(1e-6)
    h.assembled(1e-2, 1e-8, "a")
    h.assembled(1.0, 1e-8, "b")


def test_keep_history_6_an_upload_of_identical_values_is_still_an_upload():
    h = KeepHistory()
    h.assembled(0.0, 0.0, "a")
    h.assembled(1e-4, 0.0, "b")
    h.s.assembly_set(1, h.F["Sigma"])
    h.assembled(1e-2, 1e-8, "a")


def test_keep_history_7_a_structure_edit_equilibrates_afresh():
    h = KeepHistory()
    h.assembled(0.0, 0.0, "a")
    h.assembled(1e-4, 0.0, "b")
    h.delayed = np.array([3, 4, 150, 301], dtype=np.int32)
    h.moved = h.s.delay_columns(h.delayed)
    assert h.moved > 0
    h.assembled(1e-2, 1e-8, "a")                          # on the edited structure (the fresh handle gets the same edit)
    h.assembled(1.0, 1e-8, "b")


# ------------------------------------------------------------------------------------------------
# 3. primal-dual kernels
# ------------------------------------------------------------------------------------------------
def pd_handle(P, deltas, segs):
    irn, jcn, lens, srcs = vs.pd_kkt_triplets(P)
    shift = vs.pd_shift(deltas)
    n4 = P["nx"] + P["ns"] + P["nc"] + P["nd"]
    vals0 = np.concatenate([sc * np.asarray(v) + sh for sc, sh, v in zip(vs.PD_SCALE, shift, srcs)])
    s = ipopt_amd.KKTSolver()
    s.initialize_structure(n4, irn, jcn, vals=vals0)
    s.assembly_define(lens)
    for q, v in enumerate(srcs):
        s.assembly_set(q, v)
    st, neg, zero = s.factor_assembled(vs.PD_SCALE, shift)
    assert st == 0 and neg == P["nc"] + P["nd"]
    nb = [len(P[k]) for k in ("ixl", "ixu", "isl", "isu")]
    s.pd_define([P["nx"], P["ns"], P["nc"], P["nd"]] + nb, P["ixl"], P["ixu"], P["isl"], P["isu"], irn, jcn, segs)
    s.pd_put_data([P[k] for k in ("zl", "zu", "vl", "vu", "sxl", "sxu", "ssl", "ssu")])
    return s


def check_residual_and_norms(s, P, deltas, trip, rhs, res):
    """pd_residual against K8 res - rhs row by row.  Bound: a row is a sum of k_row products and the right-hand side, accumulated one term after the
    other; the standard bound for such a dot product is gamma_(k+1) <= (k + 2) u (1 + ...) times sum |terms|; the x and s rows are finished in a second
    kernel (two more additions).  2 (k_row + 4) u (|K8| |res| + |rhs|)_row covers it with a factor 2 in hand, contracted products (FMA) included --
    they only remove roundings.  The three norms are maxima: exact, compared with the maxima of what the device itself holds."""
    n8 = trip[3]
    s.pd_put(0, vs.pd_split(P, rhs)); s.pd_put(1, vs.pd_split(P, res))
    nr = s.pd_residual(0, 1, 2, deltas)
    resid = np.concatenate(s.pd_get(2))
    y, ya, k, _ = vs.k8_apply(P, deltas, res, trip)
    want = y - rhs.astype(LD)
    bound = 2 * (k + 4) * U * (ya + np.abs(rhs))
    bad = np.flatnonzero(~(np.abs(resid.astype(LD) - want) <= bound))
    assert bad.size == 0, (bad[:8], resid[bad[:8]], want[bad[:8]])
    assert nr[0] == np.abs(rhs).max(initial=0.0) and nr[1] == np.abs(res).max(initial=0.0) and nr[2] == np.abs(resid).max(initial=0.0)
    return resid


def check_solve(s, P, deltas, trip, rhs, nrm):
    """pd_solve_once by substitution: the longdouble residual of the returned vector in the 8-block system, scaled by ||K8|| ||x|| + ||rhs||, <= RES_TOL
    (the reduced system is quasi-definite with a diagonally dominant (1,1) block: tests/test_value_spec.py)"""
    n8 = trip[3]
    s.pd_put(0, vs.pd_split(P, rhs))
    s.pd_put(1, vs.pd_split(P, np.full(n8, np.nan)))                     # beta = 0 must not read the target
    s.pd_solve_once(0, 1, 1.0, 0.0)
    sol = np.concatenate(s.pd_get(1))
    assert np.all(np.isfinite(sol))
    y, _, _, _ = vs.k8_apply(P, deltas, sol, trip)
    r = float(np.abs(y - rhs.astype(LD)).max()) / (float(nrm) * np.abs(sol).max() + np.abs(rhs).max())
    assert r <= RES_TOL, r
    return sol


@pytest.mark.parametrize("name", sorted(vs.PD_SHAPES))
def test_pd_kernels_at_the_shapes_where_they_can_go_wrong(name):
    P, deltas, segs = vs.pd_shape(name)
    s = pd_handle(P, deltas, segs)
    trip = vs.k8_triplets(P, deltas)
    n8 = trip[3]; n4 = P["nx"] + P["ns"] + P["nc"] + P["nd"]
    nrm = vs.k8_apply(P, deltas, np.zeros(n8), trip)[3]
    rng = np.random.default_rng(7)
    rhs = rng.standard_normal(n8); pert = rng.standard_normal(n8)
    check_residual_and_norms(s, P, deltas, trip, rhs, pert)
    sol = check_solve(s, P, deltas, trip, rhs, nrm)
    # localising a failure: the expansion of the device's own x | s blocks (3 roundings per entry: product, difference, quotient) ...
    exp8, bnd = vs.pd_expand(P, rhs, sol[:n4])
    assert np.all(np.abs(sol.astype(LD) - exp8) <= (3 * U + 4 * U * U) * bnd)
    # ... and the reduction: the 4-block solve of the host-reduced right-hand side through the same factorisation (1e-9: the suite's agreement figure)
    aug = vs.pd_reduce(P, rhs, dtype=np.float64)
    s.multi_solve(False, aug)
    assert np.abs(aug - sol[:n4]).max() <= 1e-9 * np.abs(sol[:n4]).max()
    # res <- alpha sol + beta res: the same solve every time (no atomics on fp data), so `sol` is the reference; one product and one sum or one
    # fused operation per term: 2 u (|alpha sol| + |beta res|) covers either; beta = 0 starts from NaN and must not read it
    for alpha, beta in vs.PD_COEFFS:
        s.pd_put(1, vs.pd_split(P, pert if beta != 0.0 else np.full(n8, np.nan)))
        s.pd_solve_once(0, 1, alpha, beta)
        got = np.concatenate(s.pd_get(1))
        assert np.all(np.isfinite(got)), (alpha, beta)
        want = vs.pd_combine(alpha, sol, beta, pert)
        scale = abs(alpha) * np.abs(sol) + (abs(beta) * np.abs(pert) if beta != 0.0 else 0.0)
        assert np.all(np.abs(got.astype(LD) - want) <= 2 * U * (1 + U) * scale), (alpha, beta)
        if (alpha, beta) == (1.0, 0.0):
            assert np.array_equal(got, sol)
        if (alpha, beta) == (1.0, 1.0):
            assert np.array_equal(got, pert + sol)
        if (alpha, beta) == (-1.0, 1.0):
            assert np.array_equal(got, pert - sol)
    # special values (arithmetic inputs, not faults): a NaN in res counts as +inf, all-zero vectors have norms exactly 0
    if n8:
        bad = pert.copy(); bad[n8 // 2] = np.nan
        s.pd_put(0, vs.pd_split(P, rhs)); s.pd_put(1, vs.pd_split(P, bad))
        nr = s.pd_residual(0, 1, 2, deltas)
        assert nr[0] == np.abs(rhs).max() and nr[1] == np.inf and nr[2] == np.inf
    s.pd_put(0, vs.pd_split(P, np.zeros(n8))); s.pd_put(1, vs.pd_split(P, np.zeros(n8)))
    nr = s.pd_residual(0, 1, 2, deltas)
    assert np.array_equal(nr, np.zeros(3)) and not np.signbit(nr).any()


def test_pd_segment_order_does_not_matter():
    P, deltas, _ = vs.pd_shape("segs_5_0_3")
    rng = np.random.default_rng(3)
    n8 = int(vs.pd_offsets(P)[-1])
    rhs = rng.standard_normal(n8); res = rng.standard_normal(n8)
    out = []
    for segs in ([5, 0, 3], [0, 3, 5]):
        s = pd_handle(P, deltas, segs)
        s.pd_put(0, vs.pd_split(P, rhs)); s.pd_put(1, vs.pd_split(P, res))
        s.pd_residual(0, 1, 2, deltas)
        out.append(np.concatenate(s.pd_get(2)))
    assert np.array_equal(out[0], out[1])


def test_pd_kernels_beyond_one_launch_of_threads():
    """nx = 560 000 with every x lower-bounded, ns = nd = 8 000, nc = 20 000: n4 and nxl are both beyond the 2048 x 256 threads grid1d launches at most,
    so every kernel walks its grid-stride loop more than once."""
    P, deltas, segs = vs.pd_shape(vs.PD_LARGE)
    assert len(P["ixl"]) > 2048 * 256
    s = pd_handle(P, deltas, segs)
    trip = vs.k8_triplets(P, deltas)
    n8 = trip[3]
    rng = np.random.default_rng(7)
    rhs = rng.standard_normal(n8); pert = rng.standard_normal(n8)
    check_residual_and_norms(s, P, deltas, trip, rhs, pert)
    nrm = vs._rowsum(n8, trip[0], np.abs(trip[2])).max()
    check_solve(s, P, deltas, trip, rhs, nrm)


# ------------------------------------------------------------------------------------------------
# 4. assembly and gather
# ------------------------------------------------------------------------------------------------
def _segmented_system(nseg, seed=1):
    """a diagonally dominant tridiagonal system whose triplets are cut into nseg segments (some of length 0)"""
    rng = np.random.default_rng(seed)
    n = 200
    r = np.concatenate([np.arange(n), np.arange(1, n)]).astype(np.int32) + 1
    c = np.concatenate([np.arange(n), np.arange(n - 1)]).astype(np.int32) + 1
    src = np.concatenate([rng.uniform(1.0, 2.0, n) * 10.0 ** rng.uniform(0, 2, n), rng.uniform(-0.02, 0.02, n - 1)])
    cuts = np.sort(rng.integers(0, 2 * n - 1, nseg - 1))
    if nseg >= 4:
        cuts[1] = cuts[0]                                 # a segment of length 0 in the middle ...
        cuts[-1] = 2 * n - 1                              # ... and one at the end
    lens = np.diff(np.concatenate([[0], cuts, [2 * n - 1]]))
    return n, r, c, src, [int(x) for x in lens], rng.standard_normal(n)


def _assembled_vs_host(n, r, c, srcs, lens, scales, shifts, b, host_vals, junk=None):
    s = ipopt_amd.KKTSolver()
    s.initialize_structure(n, r, c, vals=host_vals)
    s.assembly_define(lens)
    for q, v in enumerate(srcs):
        s.assembly_set(q, v if junk is None or scales[q] != 0.0 else junk[: lens[q]])
    st, neg, zero = s.factor_assembled(scales, shifts)
    x = b.copy(); s.multi_solve(False, x)
    s2, st2, neg2, x2, _ = fresh(n, r, c, host_vals, b)
    assert (st, neg) == (st2, neg2)
    return st, x, x2


def test_assembly_with_scales_zero_and_one_is_bitwise_the_host_expression():
    """16 segments (the limit), two of length 0, scales 0 and +-1, non-zero shifts; the sources of the scale-0 segments hold NaN and Inf and must not be read
    into the result: such a segment is exactly its shift."""
    n, r, c, src, lens, b = _segmented_system(16)
    assert len(lens) == 16 and lens.count(0) >= 2
    off = np.concatenate([[0], np.cumsum(lens)])
    srcs = [src[off[q]:off[q + 1]] for q in range(16)]
    scales = np.array([1.0, -1.0, 0.0, 1.0] * 4); shifts = np.array([0.0, 0.5, 3.0, -0.25] * 4)
    host = np.concatenate([(sc * v if sc != 0.0 else np.zeros(len(v))) + sh for sc, sh, v in zip(scales, shifts, srcs)])
    assert np.array_equal(host, vs.assemble_spec(scales, shifts, srcs).astype(np.float64))
    junk = np.tile([np.nan, np.inf, -np.inf], 2 * n)
    st, x, x2 = _assembled_vs_host(n, r, c, srcs, lens, scales, shifts, b, host, junk=junk)
    assert np.all(np.isfinite(x)) and np.array_equal(x, x2)


def test_assembly_with_general_scales_is_within_one_ulp_of_the_exact_expression():
    """scales 0.3 and -2.5 with non-zero shifts: sc * src + sh may or may not be contracted to one fused operation; either way every value is within
    1 ulp of the longdouble expression, so the solution must satisfy the system of the longdouble-rounded values to RES_TOL (and agree with that
    system's own solution to 1e-9)."""
    n, r, c, src, lens, b = _segmented_system(5, seed=2)
    off = np.concatenate([[0], np.cumsum(lens)])
    srcs = [src[off[q]:off[q + 1]] for q in range(5)]
    # |diagonal| >= 0.3 and |off-diagonal| <= 2.5 * 0.02 + 0.0625 whatever segment an entry falls into: strictly diagonally dominant, well-conditioned once equilibrated
    scales = np.array([0.3, -2.5, 0.3, -2.5, 0.3]); shifts = np.array([1e-3, -0.05, 0.0625, 1e-8, 0.03])
    host = vs.assemble_spec(scales, shifts, srcs).astype(np.float64)
    st, x, x2 = _assembled_vs_host(n, r, c, srcs, lens, scales, shifts, b, host)
    K = kktgen.to_scipy(n, r, c, host)
    assert st == 0 and sres(K, x, b) <= RES_TOL and np.abs(x - x2).max() <= 1e-9 * np.abs(x2).max()


def test_assembled_values_read_off_a_diagonal_system():
    """a diagonal matrix with scaling off: x = b / a reads every assembled value off, so each one can be held against the longdouble expression: within
    1 ulp for general scales (fused or not), bitwise the host expression for scales 0 and +-1"""
    rng = np.random.default_rng(4)
    n = 300
    idx = np.arange(1, n + 1, dtype=np.int32)
    src = rng.uniform(1.0, 2.0, n) * 10.0 ** rng.uniform(-3, 3, n)
    lens = [60, 0, 60, 60, 60, 60]
    off = np.concatenate([[0], np.cumsum(lens)])
    srcs = [src[off[q]:off[q + 1]] for q in range(6)]
    scales = np.array([0.3, 1.0, -2.5, 0.0, 1.0, -1.0]); shifts = np.array([1e-4, 0.0, -1e-4, -1e-8, 0.75, -0.5])
    want = vs.assemble_spec(scales, shifts, srcs)
    s = ipopt_amd.KKTSolver(scaling=0)
    s.initialize_structure(n, idx, idx, vals=want.astype(np.float64))
    s.assembly_define(lens)
    for q, v in enumerate(srcs):
        s.assembly_set(q, v if scales[q] != 0.0 else np.full(lens[q], np.nan))
    st, neg, zero = s.factor_assembled(scales, shifts)
    assert st == 0
    b = np.exp2(np.floor(np.log2(np.abs(want.astype(np.float64)))) + 60).astype(np.float64)      # powers of two: b / a and its inverse lose nothing that matters below
    x = b.copy(); s.multi_solve(False, x)
    a = (b.astype(LD) / x.astype(LD))                                     # a (1 + 2 u at most: one division on the device, none here in fp64)
    ulp = np.spacing(np.abs(want.astype(np.float64))).astype(LD)
    assert np.all(np.abs(a - want) <= ulp + 3 * U * np.abs(want))
    for q in (3, 4, 5):                                                   # scales 0 and +-1: the device value is the host's fp64 value, so is x = b / a
        sl = slice(off[q], off[q + 1])
        hostv = (scales[q] * srcs[q] if scales[q] != 0.0 else np.zeros(lens[q])) + shifts[q]
        assert np.array_equal(x[sl], b[sl] / hostv)


def test_a_seventeenth_segment_is_refused():
    n = 40
    idx = np.arange(1, n + 1, dtype=np.int32)
    s = ipopt_amd.KKTSolver(scaling=0)                                     # (x = b / a bitwise: no equilibration in between)
    s.initialize_structure(n, idx, idx, vals=np.ones(n))
    with pytest.raises(ipopt_amd.KKTError, match="segments"):
        s.assembly_define([2] * 16 + [8])
    s.assembly_define([2] * 15 + [10])                                     # 16 are fine, and the handle is still usable
    for q in range(16):
        s.assembly_set(q, np.full(2 if q < 15 else 10, float(q + 1)))
    st, neg, zero = s.factor_assembled(np.ones(16), np.zeros(16))
    x = np.ones(n); s.multi_solve(False, x)
    assert st == 0 and np.array_equal(x, 1.0 / np.repeat(np.arange(1.0, 17.0), [2] * 15 + [10]))


def test_gather_of_duplicates_is_ordered_and_reproducible():
    """positions with 1, 2, 7 and 1000 duplicates (the last the cancelling triple 1e16, 1, -1e16 repeated), each a 1 x 1 block of its own: with scaling off
    x = b / a reads the gathered sum off.  Any order of summation stays within (d - 1) u sum |v| of the exact sum (math.fsum); two handles agree bitwise."""
    n, r, c, v, dup = vs.gather_fixture()
    xs = []
    for _ in range(2):
        s, st, neg, x, f = fresh(n, r, c, v, np.ones(n), scaling=0)
        assert st == 0
        xs.append(x)
    assert np.array_equal(xs[0], xs[1])
    for row, d in dup.items():
        exact = math.fsum(d)
        bound = (len(d) - 1) * U * math.fsum(abs(t) for t in d)
        a = 1.0 / LD(xs[0][row])                                           # (one rounding of the division on the device: u |a| more)
        assert abs(float(a - LD(exact))) <= bound + 2 * U * abs(exact), (row, float(a), exact)
    assert xs[0][0] == 1.0 / 2.5 and xs[0][1] == 1.0 / (0.1 + 0.2)        # one or two duplicates: exactly the fp64 value / sum
