"""Host only (no device): the fixtures of tests/test_gpu_mid_solve.py take their fronts of order 33 .. 128 through the LEVEL launches of the solve
sweeps (solve_level: k_fwd_mid / k_bwd_mid, or k_fwd / k_bwd under MI355X_KKT_DISABLE=mid_solve), not through the chain sweeps -- in both legs, which
differ by `mid_solve` alone (numeric.hip reads it: nothing in the plan moves).  The shapes are pinned, so that a later change of the ordering or of a
threshold fails here instead of silently emptying the GPU test."""
import functools

import numpy as np
import pytest

import ipopt_amd
from tests.support import midfix, pathfix, reach as R


@functools.lru_cache(maxsize=None)
def analysed(name):
    S = midfix.system(name)
    with pathfix.knobs(midfix.disable_list(name, False), S["tune"]):
        s = ipopt_amd.KKTSolver(**S["opts"])
        s.initialize_structure(S["n"], S["r"], S["c"], vals=S["v"])
    return s


def mid(name, mid_off=False):
    S = midfix.system(name)
    with pathfix.knobs(midfix.disable_list(name, mid_off), S["tune"]):
        return midfix.mid_fronts(analysed(name)) + (R.plan_arrays(analysed(name)),)


def count(fronts, cls):
    return sum(1 for f in fronts if f[0] == cls)


def span(fronts, field):
    return min(f[field] for f in fronts), max(f[field] for f in fronts)


@pytest.mark.parametrize("fixture", sorted(midfix.FIXTURES))
def test_both_legs_have_the_same_plan_and_no_wide_panel(fixture):
    """`mid_solve` switches kernels inside solve_level only; solve_level takes the new kernels for supernodes of <= 64 columns"""
    on, off = mid(fixture), mid(fixture, True)
    assert R.plan_diff(on[3], off[3]) == [] and on[:3] == off[:3]
    assert analysed(fixture).info().maxsupernode <= 64
    assert len(on[0]) > 0


def test_mid_edges_shapes():
    S = midfix.system("mid_edges")
    level, chain, nseg = mid("mid_edges")[:3]
    assert S["n"] == 972 and S["neg"] == 28
    assert chain == [] and nseg == 0
    shapes = [(o, k, ch) for _, o, k, ch, _, _ in level]
    assert sorted(set(shapes)) == sorted(midfix.MID_EDGES_SHAPES), shapes
    assert {o for o, _, _ in shapes} >= {33, 64, 65, 128} and {k for _, k, _ in shapes} >= {16, 17, 63, 64}
    assert any(o == k for o, k, _ in shapes)                                # no update rows
    assert all((c == R.FC_LDS64) == (o <= 64) for c, o, *_ in level)
    with pathfix.knobs(None, None):                                         # the default schedule would hand all four levels to the chain sweeps
        dl, dc, dseg = midfix.mid_fronts(analysed("mid_edges"))
    assert dl == [] and len(dc) == len(level) and dseg == 4


def test_grid24_shapes():
    level, chain, nseg = mid("grid24")[:3]
    assert midfix.system("grid24")["n"] == 2880
    assert chain == [] and nseg == 0
    assert (count(level, R.FC_LDS64), count(level, R.FC_LDS128)) == (35, 89)
    assert span(level, 1) == (40, 120) and span(level, 2) == (5, 63) and span(level, 3) == (0, 2)


def test_grid48x44_shapes():
    """the default schedule: mid fronts on level launches NEXT TO live chain sweeps"""
    level, chain, nseg = mid("grid48x44")[:3]
    assert midfix.FIXTURES["grid48x44"][2:] == (None, None)
    assert nseg > 0 and len(chain) > 0
    assert (count(level, R.FC_LDS64), count(level, R.FC_LDS128)) == (52, 223)
    assert span(level, 2) == (10, 30) and span(level, 3)[1] == 2


def test_hostile16_shapes():
    level, chain, nseg = mid("hostile16")[:3]
    assert chain == [] and nseg == 0
    assert len(level) == 32 and span(level, 2) == (2, 62)
    assert count(level, R.FC_LDS64) > 0 and count(level, R.FC_LDS128) > 0
    assert span(level, 3)[1] == 4                                           # all four batched child slots of k_fwd_mid are used


def test_mid_edges_reference_is_not_hidden_by_conditioning():
    """plain fp64 within 1e-9 of the refined reference (measured 1.1e-13), inertia 28 by LAPACK's eigenvalues"""
    ref, plain, eig_neg = midfix.reference("mid_edges")
    assert eig_neg == 28
    assert max(np.abs(plain[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max()) for k in range(3)) <= 1e-9
