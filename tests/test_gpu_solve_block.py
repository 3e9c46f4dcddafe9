"""-m gpu: blocks of right-hand sides in the solves (mi355x_kkt_set_solve_block; numeric.hip solve_block, the *_rb kernels of kernels_solve.hip.inc) on the
rows of tests/support/blockfix.py.  No tolerance appears in this file: equality of bits against the existing path is the specification; the accuracy of
the existing path is pinned by the tests of the fixtures' own files.

Per row ONE handle and ONE factorisation (run once per process, whatever its outcome: once() of tests/test_gpu_small_fronts.py); the row first asserts,
from its own handle's plan, the reach facts it stands on (the pins of tests/test_solve_block_plan.py).  Then for nrhs in (2, W, W + 1, 2 W + 1), W = the
block width, with the fixture's three right-hand sides (K 1, random, K random) repeated cyclically:
  1. with the switch on, every column is bitwise the solution of multi_solve on that right-hand side alone with the switch off;
  2. the same with the switch on under MI355X_KKT_DISABLE=solve_ctx, and with the switch off and all nrhs columns in one call (the contexts, where their
     one-off measurement picks them): all three ways to give a column give the same bits;
  3. equal right-hand sides in different slots give equal bits (follows from 1 with the cyclic repetition, asserted on its own);
  4. a repeated blocked call gives the same bits;
  5. solve_block_info reports the plan's counts and a positive last_ms; a call with the switch off leaves last_ms unchanged.
Isolation (leaf_edges.levels, mid_edges): in a block of W columns one is replaced by zeros and one by 1e300 x random -- the untouched columns keep their
bits, the zero column's solution is exactly zero.  Refinement (grid48x44, refine_steps = 1): blocked columns bitwise the single solves.  Low-rank (grid24
of tests/test_gpu_lowrank.py, nv = nu = 5): lowrank_update + lowrank_solve with the switch on bitwise those with it off, which == 0 in both.

Restructure (chain_delayed under the `levels` knobs, a handle of its own): a blocked solve on the unedited structure, so that the block's buffers exist,
then delay_columns and a new factorisation -- the schedule is the edited structure's (pinned), blocked columns bitwise the single solves before and after.

Measured on an MI355X when the tests were written: all 29 tests passed, the file in 3.9 s.  A first version of the executor issued the by-column records
record by record instead of column by column, and chain_delayed.levels failed at once (columns off by 0.1 .. 0.2: k_bwd_dot64 of the next column had
overwritten the partial sums k_bwd_fin64 was about to read).

That the tests can fail was tried once with a library built with two mutations: (1) the loop over the children beyond the fourth skipped in the blocked
pair kernel (fwd_pair_front with NC > 1); (2) the column stride of cvec one entry short in the gather of the blocked forward mid kernel (fwd_mid_front).
10 of 29 tests failed and nothing else did:
  (1) test_every_column...[wave_edges.levels], the one row with six gathered children on a pair level;
  (2) test_every_column...[mid_edges], [grid48x44], [hostile16], [tails.levels], [star6.groups], [chain_delayed.levels] -- every row with a blocked mid
      launch whose fronts have a child --, test_columns_of_a_block_do_not_touch_each_other[mid_edges], the refinement and the restructure test.
leaf_edges.*, leaf_edges_w8.levels, mid_edges.nomid, the info tests and the low-rank test passed.  NOT reached by any row: the loop over the children beyond the fourth of fwd_mid_front -- no fixture of the table has a
front of order 33 .. 128 with more than four children on a level launch (counted on the host for every row) --, so that loop is covered by reading only.
"""
import os

import numpy as np
import pytest
import torch      # noqa: F401  (before the library is loaded: torch brings its own HIP runtime)

import ipopt_amd
from ipopt_amd import kkt
from tests.support import blockfix as BF
from tests.test_gpu_small_fronts import once
from tests.test_solve_block_plan import PINNED

pytestmark = pytest.mark.gpu
W = BF.WIDTH
NRHS = (2, W, W + 1, 2 * W + 1)


class also_disabled:
    """MI355X_KKT_DISABLE of the moment plus one more name, for the duration of a block"""
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.old = os.environ.get("MI355X_KKT_DISABLE")
        os.environ["MI355X_KKT_DISABLE"] = ",".join(x for x in (self.old, self.name) if x)

    def __exit__(self, *exc):
        os.environ.pop("MI355X_KKT_DISABLE", None)
        if self.old is not None:
            os.environ["MI355X_KKT_DISABLE"] = self.old


def solved(s, B):
    X = np.array(B, dtype=np.float64, order="C")
    assert s.multi_solve(False, X) == kkt.SUCCESS
    return X


def _run_row(row, isolate, **opts):
    S = BF.system(row)
    out = dict(cols={}, again={}, noctx={}, off={}, info={})
    with BF.knobs(row):
        s = BF.handle(row, **opts)
        out["facts"] = BF.facts(s)
        out["expected"] = BF.expected(s)[1:]
        s.values()[:] = S["v"]
        out["st"] = int(s.multi_solve(True, None, S["neg"] is not None, S["neg"] or 0))
        assert out["st"] == kkt.SUCCESS
        assert s.solve_block_info()["last_ms"] == 0.0
        out["single"] = np.stack([solved(s, S["B"][k]) for k in range(3)])
        for nrhs in NRHS:
            Bn = np.stack([S["B"][j % 3] for j in range(nrhs)])
            s.set_solve_block(True)
            out["cols"][nrhs] = solved(s, Bn)
            i1 = s.solve_block_info()
            out["again"][nrhs] = solved(s, Bn)
            with also_disabled("solve_ctx"):
                out["noctx"][nrhs] = solved(s, Bn)
            i2 = s.solve_block_info()
            s.set_solve_block(False)
            out["off"][nrhs] = solved(s, Bn)
            i3 = s.solve_block_info()
            out["info"][nrhs] = (i1, i2, i3)
        if isolate:
            rng = np.random.default_rng(9)
            Bi = np.stack([S["B"][j % 3] for j in range(W)])
            Bi[1] = 0.0
            Bi[2] = 1e300 * rng.standard_normal(S["n"])
            s.set_solve_block(True)
            with np.errstate(all="ignore"):
                out["isolated"] = solved(s, Bi)
            s.set_solve_block(False)
        s.close()
    return out


def run_row(row, isolate=False, **opts):
    return once(("solve_block", row, tuple(sorted(opts.items()))), lambda: _run_row(row, isolate or row in ISOLATED, **opts))


ISOLATED = ("leaf_edges.levels", "mid_edges")


def check_reach(row, out):
    ls, nl, counts, blocked, bycol, top = PINNED[row]
    F = out["facts"]
    assert (F["first_top_level"], F["num_levels"], F["counts"], F["blocked"], F["bycol"], F["top"]) == PINNED[row]
    assert out["expected"] == (ls, counts)


@pytest.mark.parametrize("row", sorted(BF.ROWS))
def test_every_column_of_a_block_is_bitwise_its_own_solve(row):
    out = run_row(row)
    check_reach(row, out)
    single = out["single"]
    for nrhs in NRHS:
        want = np.stack([single[j % 3] for j in range(nrhs)])
        for way in ("cols", "again", "noctx", "off"):
            got = out[way][nrhs]
            bad = [j for j in range(nrhs) if not np.array_equal(got[j], want[j])]
            print(f"{row} nrhs {nrhs} {way}: columns that differ from their own solve {bad}" +
                  (f", max |difference| {np.nanmax(np.abs(got[bad] - want[bad])):.3e}" if bad else ""))
    for nrhs in NRHS:
        want = np.stack([single[j % 3] for j in range(nrhs)])
        assert np.array_equal(out["cols"][nrhs], want), f"nrhs {nrhs}: switch on"                                   # 1
        assert np.array_equal(out["noctx"][nrhs], want), f"nrhs {nrhs}: switch on, solve_ctx disabled"               # 2
        assert np.array_equal(out["off"][nrhs], want), f"nrhs {nrhs}: switch off, all columns in one call"           # 2
        for j in range(3, nrhs):
            assert np.array_equal(out["cols"][nrhs][j], out["cols"][nrhs][j - 3]), f"nrhs {nrhs}: slots {j - 3} and {j}"      # 3
        assert np.array_equal(out["again"][nrhs], out["cols"][nrhs]), f"nrhs {nrhs}: repeated call"                   # 4


@pytest.mark.parametrize("row", sorted(BF.ROWS))
def test_info_reports_the_plan_and_the_time_of_the_last_blocked_call(row):
    out = run_row(row)
    ls, nl, counts, *_ = PINNED[row]
    for nrhs in NRHS:
        i1, i2, i3 = out["info"][nrhs]
        for i in (i1, i2, i3):
            assert (i["width"], i["first_top_level"], i["blocked_launches"], i["bycol_launches"], i["top_launches_per_column"]) == (W, ls) + counts
        assert i1["on"] and i2["on"] and not i3["on"]
        assert i1["last_ms"] > 0.0 and i2["last_ms"] > 0.0
        assert i3["last_ms"] == i2["last_ms"]              # the call with the switch off left it alone


@pytest.mark.parametrize("row", ISOLATED)
def test_columns_of_a_block_do_not_touch_each_other(row):
    out = run_row(row)
    X, single = out["isolated"], out["single"]
    assert np.array_equal(X[0], single[0]) and np.array_equal(X[3], single[3 % 3])
    assert np.all(X[1] == 0.0)
    assert not np.array_equal(X[2], single[2])


def test_refinement_runs_by_column_around_the_blocked_core():
    out = run_row("grid48x44", refine_steps=1)
    check_reach("grid48x44", out)
    for nrhs in NRHS:
        assert np.array_equal(out["cols"][nrhs], np.stack([out["single"][j % 3] for j in range(nrhs)])), f"nrhs {nrhs}"


def _restructured():
    """chain_delayed: a blocked solve on the UNEDITED structure first (the block's buffers exist), then the edit, then blocked solves again"""
    from tests.support import bigfix
    S = bigfix.system("chain_delayed")
    Bn = np.stack([S["B"][j % 3] for j in range(W + 1)])
    with bigfix.leg_knobs("levels"):
        s = ipopt_amd.KKTSolver(**S["opts"])
        s.initialize_structure(S["n"], S["r"], S["c"], vals=S["v"])
        s.values()[:] = S["v"]
        assert s.multi_solve(True, None, True, S["neg"]) == kkt.SUCCESS
        before = dict(BF.facts(s), single=np.stack([solved(s, S["B"][k]) for k in range(3)]))
        s.set_solve_block(True)
        before["cols"] = solved(s, Bn)
        s.delay_columns(list(S["delayed"]))
        s.values()[:] = S["v"]
        assert s.multi_solve(True, None, True, S["neg"]) == kkt.SUCCESS
        after = dict(BF.facts(s), cols=solved(s, Bn), again=solved(s, Bn))
        s.set_solve_block(False)
        after["single"] = np.stack([solved(s, S["B"][k]) for k in range(3)])
        s.close()
    return before, after


def test_the_buffers_and_the_plan_follow_a_restructure():
    before, after = once(("solve_block", "restructured"), _restructured)
    ls, nl, counts, blocked, bycol, top = PINNED["chain_delayed.levels"]
    assert (after["first_top_level"], after["num_levels"], after["counts"], after["blocked"], after["bycol"], after["top"]) == PINNED["chain_delayed.levels"]
    assert (before["counts"], before["num_levels"]) != (after["counts"], after["num_levels"])      # the edit changed the schedule
    for F in (before, after):
        assert np.array_equal(F["cols"], np.stack([F["single"][j % 3] for j in range(W + 1)]))
    assert np.array_equal(after["again"], after["cols"])


def _lowrank():
    from tests.test_gpu_lowrank import factored, reference, system
    S, Rf = system(1728), reference(1728, 5, 5)
    res = {}
    s = factored(S)
    s.lowrank_set(Rf["V"], Rf["U"])
    for on in (False, True):
        s.set_solve_block(on)
        st = s.lowrank_update()
        X = Rf["B"].copy()
        s.lowrank_solve(X)
        res[on] = (st, X, s.solve_block_info()["last_ms"])
    s.close()
    return res


def test_lowrank_update_and_solve_with_blocked_inner_solves():
    res = once(("solve_block", "lowrank"), _lowrank)
    assert res[False][0] == res[True][0] == (kkt.SUCCESS, 0)
    assert res[False][2] == 0.0 and res[True][2] > 0.0                # the inner solves took the blocked path
    assert np.array_equal(res[False][1], res[True][1])
