"""CPU: the references of tests/support/value_spec.py against dense brute force, and the properties of the shared fixtures that the
GPU tests of the value path (tests/test_gpu_value_path.py) rely on: which equilibration variant each system meets, that the primal-dual
shapes are well-conditioned by construction, that the histories of the kept-scaling tests can tell their two cases apart."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import pd_oracle as po
from tests.support import kktgen, value_spec as vs

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)


def _dense_sym(n, r, c, v):
    A = np.zeros((n, n), dtype=LD)
    for i, j, a in zip(r - 1, c - 1, v):
        A[max(i, j), min(i, j)] += LD(a)
    return A + np.tril(A, -1).T


def _random_triplets(n, nnz, seed, dup=True):
    rng = np.random.default_rng(seed)
    r = rng.integers(1, n + 1, nnz); c = rng.integers(1, n + 1, nnz)
    v = rng.standard_normal(nnz) * 10.0 ** rng.uniform(-4, 4, nnz)
    if not dup:
        key = np.maximum(r, c) * (n + 1) + np.minimum(r, c)
        _, first = np.unique(key, return_index=True)
        r, c, v = r[first], c[first], v[first]
    return r.astype(np.int32), c.astype(np.int32), v


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ruiz_spec_equals_the_dense_jacobi_iteration(seed):
    n = 23
    r, c, v = _random_triplets(n, 90, seed)
    v[r == 7] = 0.0; v[c == 7] = 0.0                                # a row of stored zeros keeps its factor
    A = np.abs(_dense_sym(n, r, c, v))
    s = np.ones(n, dtype=LD)
    for k in range(4):
        mx = (A * s[None, :]).max(axis=1) * s
        s = np.where(mx > 0, s / np.sqrt(np.where(mx > 0, mx, 1)), s)
    got = vs.ruiz_spec(n, r, c, v)
    assert np.abs(got / s - 1).max() <= 16 * EPS_LD
    assert got[6] == 1.0
    pat = np.zeros((n, n), dtype=bool); pat[r - 1, c - 1] = True; pat |= pat.T      # (stored zeros stay in the pattern)
    assert vs.rslot_len(n, r, c) == int(pat.sum())


def test_ruiz_triplet_spec_takes_the_maximum_over_triplets_not_over_summed_entries():
    n = 19
    r, c, v = _random_triplets(n, 60, 5, dup=False)
    a, b = vs.ruiz_spec(n, r, c, v), vs.ruiz_triplet_spec(n, r, c, v)
    assert np.abs(a / b - 1).max() <= 64 * EPS_LD                   # no duplicates: one iteration, two ways to write it
    # the cancelling triple on one position: 1e16 for the triplet routine, 1 for the solver
    r2 = np.array([1, 1, 1, 2], dtype=np.int32); c2 = np.array([1, 1, 1, 2], dtype=np.int32); v2 = np.array([1e16, 1.0, -1e16, 4.0])
    assert float(vs.ruiz_spec(2, r2, c2, v2, sweeps=1)[0]) == 1.0 and float(vs.ruiz_triplet_spec(2, r2, c2, v2, sweeps=1)[0]) == 1e-8
    assert float(vs.ruiz_triplet_spec(2, r2 - 1, c2 - 1, v2, sweeps=1, base=0)[1]) == 0.5


def test_each_equilibration_variant_is_met_by_the_system_named_for_it():
    seen = set()
    for name, (n, r, c, v, variant) in vs.ruiz_systems().items():
        ln = vs.rslot_len(n, r, c)
        got = 0 if ln < 8 * n else (1 if ln < 16 * n else 2)
        assert got == variant == vs.ruiz_variant(n, r, c), (name, ln / n)
        assert n % 8 != 0, name
        seen.add((variant, n % 2))
    assert {(0, 1), (1, 1), (2, 1)} <= seen                          # an odd order in every variant
    n, r, c, v, _ = kktgen.grid_kkt(9, 7, dof=2, ncon=1, seed=2, sigma_exp=8.0)
    a = np.abs(v[v != 0])
    assert a.max() / a.min() >= 1e12                                 # the wide-range edge case really is wide


def _pd_record(P, deltas):
    sx, ss = vs.sigma(P)
    return dict(P, W=P["wt"], Jc=P["jct"], Jd=P["jdt"], deltas=np.array(deltas), sigma_x=sx, sigma_s=ss)


@pytest.mark.parametrize("name", sorted(vs.PD_SHAPES))
def test_pd_spec_equals_the_dense_eight_block_system(name):
    P, deltas, segs = vs.pd_shape(name)
    K = po.k8_dense(_pd_record(P, deltas)).astype(LD)
    n8 = K.shape[0]
    rng = np.random.default_rng(3)
    v = rng.standard_normal(n8)
    y, ya, k, nrm = vs.k8_apply(P, deltas, v)
    scale = np.abs(K) @ np.abs(v).astype(LD)
    tol = 8 * vs.U * scale                                           # (the dense matrix sums its duplicates and W + delta_x I in fp64)
    assert np.all(np.abs(y - K @ v.astype(LD)) <= tol)
    assert np.all(ya >= scale - tol)      # term by term: duplicates of opposite sign count with their moduli (|a1| + |a2| >= |a1 + a2|)
    assert float(nrm) >= float(np.abs(K).sum(axis=1).max()) * (1 - 1e-15)
    assert np.all(k >= (K != 0).sum(axis=1))                         # duplicates are separate terms: never fewer than the dense row holds
    # reduction + 4-block solve + expansion solves the 8-block system
    n4 = P["nx"] + P["ns"] + P["nc"] + P["nd"]
    rhs = rng.standard_normal(n8)
    sol8 = po.solve_once(_pd_record(P, deltas), rhs)
    A4 = _augmented_dense(P, deltas)
    aug = vs.pd_reduce(P, rhs)
    assert np.abs(A4 @ sol8[:n4] - aug.astype(float)).max() <= 1e-11 * max(1.0, np.abs(aug).max())
    exp8, bnd = vs.pd_expand(P, rhs, sol8[:n4])
    assert np.abs(exp8.astype(float) - sol8).max() <= 1e-12 * max(1.0, np.abs(sol8).max())
    assert np.array_equal(vs.pd_reduce(P, rhs, dtype=np.float64), vs.pd_reduce(P, rhs, dtype=np.float64)) and np.abs(vs.pd_reduce(P, rhs, dtype=np.float64) - aug).max() <= 8 * vs.U * np.abs(aug).max()


def _augmented_dense(P, deltas):
    irn, jcn, lens, srcs = vs.pd_kkt_triplets(P)
    vals = np.concatenate([sc * np.asarray(s) + sh for sc, sh, s in zip(vs.PD_SCALE, vs.pd_shift(deltas), srcs)])
    n4 = P["nx"] + P["ns"] + P["nc"] + P["nd"]
    return _dense_sym(n4, irn, jcn, vals).astype(float)


@pytest.mark.parametrize("name", sorted(vs.PD_SHAPES) + ["large"])
def test_pd_shapes_are_well_conditioned_by_construction(name):
    """(1,1) block strictly diagonally dominant with a positive diagonal => positive definite; (s,s) block Sigma_s + delta_s > 0 wherever there are slacks;
    delta_c > 0 => the augmented system is symmetric quasi-definite, its inertia (nx + ns, nc + nd, 0), every pivot order stable."""
    P, deltas, segs = vs.pd_shape(name if name != "large" else vs.PD_LARGE)
    assert vs.pd_dominance_margin(P, deltas[0]) >= 1.0
    _, ss = vs.sigma(P)
    assert P["ns"] == 0 or (ss + deltas[1]).min() >= 0.05
    assert deltas[2] > 0 and P["ns"] == P["nd"]
    for k in ("sxl", "sxu", "ssl", "ssu", "zl", "zu", "vl", "vu"):
        assert np.all(np.asarray(P[k]) >= 0.1)
    wr, wc, wv = P["wt"]
    assert (wr > wc).any() and (wr < wc).any()                       # both triangles
    key = np.maximum(wr, wc) * P["nx"] + np.minimum(wr, wc)
    assert np.unique(key).shape[0] < key.shape[0]                    # duplicates
    for t, m in ((P["jct"], P["nc"]), (P["jdt"], P["nd"])):
        if m:
            cnt = np.bincount(t[0], minlength=m)
            assert cnt.min() >= 2 and cnt.max() <= 3
    if name != "large":
        n4 = P["nx"] + P["ns"] + P["nc"] + P["nd"]
        ev = np.linalg.eigvalsh(_augmented_dense(P, deltas))
        assert int((ev < 0).sum()) == P["nc"] + P["nd"] and np.abs(ev).min() >= 1e-4
    o = vs.pd_offsets(P)
    if name.startswith("n4_"):
        assert (o[4], o[8]) == {"n4_63_len8_127": (63, 127), "n4_64_len8_128": (64, 128), "n4_65_len8_129": (65, 129)}[name]
    if name == "large":
        assert len(P["ixl"]) > 2048 * 256 and o[4] > 2048 * 256


def test_the_large_pd_reference_is_quick():
    import time
    P, deltas, _ = vs.pd_shape(vs.PD_LARGE)
    t0 = time.perf_counter()
    trip = vs.k8_triplets(P, deltas)
    y, ya, k, nrm = vs.k8_apply(P, deltas, np.ones(trip[3]), trip)
    assert time.perf_counter() - t0 < 20.0 and np.isfinite(float(nrm))       # (about a second; the limit only catches a quadratic slip)


def test_assemble_spec_is_the_exactly_rounded_expression():
    rng = np.random.default_rng(2)
    src = rng.standard_normal(50) * 10.0 ** rng.uniform(-5, 5, 50)
    for sc, sh in ((0.3, 1e-4), (-2.5, -7.0), (1.0, 0.25), (-1.0, 1e-8), (0.0, -1e-8)):
        got = vs.assemble_spec([sc], [sh], [src])
        for a, g in zip(src, got):
            exact = Fraction(sc) * Fraction(a) + Fraction(sh) if sc != 0.0 else Fraction(sh)
            assert abs(Fraction(float(g)) - exact) <= abs(exact) * Fraction(1, 2 ** 52)      # (longdouble carries 64 bits: rounding to fp64 is within 1 ulp of exact)
        if sc in (1.0, -1.0, 0.0):
            assert np.array_equal(got.astype(np.float64), (sc * src if sc != 0.0 else np.zeros(50)) + sh)
    bad = np.array([np.nan, np.inf, -np.inf, 1.0])
    assert np.array_equal(vs.assemble_spec([0.0], [-1e-8], [bad]).astype(np.float64), np.full(4, -1e-8))
    assert vs.assemble_spec([], [], []).shape == (0,)


def test_keep_histories_can_tell_fresh_factors_from_kept_ones():
    """Case (a) and case (b) of the kept-scaling contract are told apart by get_scaling(): that needs the Ruiz factors of consecutive matrices
    of every history to DIFFER by far more than rounding.  Also: the matrices of the histories are regular."""
    F = vs.keep_fixture()
    n, r, c = F["n"], F["r"], F["c"]
    ruiz = lambda vals: vs.ruiz_spec(n, r, c, vals).astype(float)
    far = lambda a, b: np.abs(a / b - 1).max() >= 1e-6
    A0, A1 = vs.keep_host_vals(F, 1e-4, 0.0), vs.keep_host_vals(F, 1e-2, 1e-8)
    B = vs.keep_other_matrix(F)
    assert far(ruiz(A0), ruiz(A1)) and far(ruiz(B), ruiz(A1)) and far(ruiz(B), ruiz(A0))
    lad = [ruiz(vs.keep_host_vals(F, dx, dc)) for dx, dc in vs.KEEP_LADDER]
    assert all(far(lad[k], lad[k + 1]) for k in range(len(lad) - 1)) and all(far(lad[0], f) for f in lad[1:])
    # history 2: sources zero, the matrix is the shifts alone -- diag(dx I, -dc I), regular for dx = 2, dc = 1
    zero = (0 * F["hv"], 0 * F["Sigma"], 0 * F["jv"])
    Z = _dense_sym(n, r, c, vs.keep_host_vals(F, 2.0, 1.0, zero)).astype(float)
    assert np.array_equal(Z, np.diag(np.diag(Z))) and np.all(np.diag(Z)[: F["nx"]] == 2.0) and np.all(np.diag(Z)[F["nx"]:] == -1.0)
    assert far(ruiz(vs.keep_host_vals(F, 2.0, 1.0, zero)), ruiz(A0))
    # every matrix of the histories is regular with inertia (nx, m, 0) by construction: H + Sigma + dx I is strictly diagonally dominant with a positive
    # diagonal, and row i of J is the only one with an entry in column 2 i + 1 (full row rank) -- Sylvester; B is a congruence of such a matrix
    H = _dense_sym(F["nx"], r[: 2 * F["nx"] - 1], c[: 2 * F["nx"] - 1], F["hv"]).astype(float)
    assert np.all(2 * np.diag(H) - np.abs(H).sum(axis=1) > 1.0) and np.all(F["Sigma"] > 0)
    J = np.zeros((F["m"], F["nx"])); J[(r - 1 - F["nx"])[-4 * F["m"]:-F["m"]], (c - 1)[-4 * F["m"]:-F["m"]]] = F["jv"]
    anchors = J[:, 1::2][:, : F["m"]]
    assert np.all(np.abs(np.diag(anchors)) >= 1.0) and np.count_nonzero(anchors) == F["m"]


def test_gather_fixture_reads_each_sum_off_a_decoupled_block():
    n, r, c, v, dup = vs.gather_fixture()
    assert sorted(len(d) for d in dup.values()) == [1, 2, 7, 1000]
    A = _dense_sym(n, r, c, v).astype(float)
    for row, d in dup.items():
        assert np.count_nonzero(A[row]) == 1 and math.fsum(d) != 0.0                 # decoupled, and the exact sum is not zero
    assert math.fsum(dup[3]) == 333.0 + 2.0 ** 40                                     # 333 x (1e16 + 1 - 1e16) + 2^40
    bound = (len(dup[3]) - 1) * vs.U * math.fsum(abs(x) for x in dup[3])
    assert bound > 1e16 * vs.U                                                        # (honest: the bound of a cancelling sum is wide; the narrow ones are rows 1 and 2)
    assert (r > c).any() and (r < c).any()
