"""-m gpu: the kernels of the one-wavefront fronts (class FC_WAVE, order <= 32) -- factor: k_leaf_chain, k_front_df with front_dpp16_body<true> and
front_lds32_body, k_front_dpp16, k_front_reg<64, 4>; solve: k_fwd_leafchain / k_bwd_leafchain, k_fwd_pair / k_bwd_pair<16, 16>, <16> and <32>,
k_fwd<64> / k_bwd<64>; host: the fall-back and the back-off of the optimistic schedule in NumericImpl::factor -- on fronts of PRESCRIBED edge shapes
(tests/support/smallfix.py), against a reference refined with longdouble residuals and against the pivoting specification (tests/support/mirror.py).
tests/test_small_front_reach.py shows on the host what a leg launches and pins the shapes; every test here first asserts, from its own handle, the reach
facts it stands on.

Legs (smallfix.LEGS), knobs held from the set-up of the handle to its last solve:
  default  optimistic schedule: k_leaf_chain and k_front_df; solves by the chain sweeps
  levels   MI355X_KKT_TUNE=chain_solve_maxc=1: the same factorisation; solves by k_*_leafchain and the pair kernels
  nopair   levels + MI355X_KKT_DISABLE=pair_solve: solves by k_fwd<64> / k_bwd<64>
  noleaf   levels + DISABLE=leafchain: the data-flow run starts at level 0
  nodf     levels + DISABLE=front_df,leafchain: per-level k_front_dpp16, the strict k_front_reg<64, 4> for the orders 17 .. 32
  strict   levels + DISABLE=fastpiv: strict kernels only
  full     levels + DISABLE=optimistic: the full schedule, in a child process (`optimistic` is read once per process); leaf_edges, wave_edges, leaf_reject

Per leg, over three right-hand sides (K 1, a random vector, K random): status SUCCESS; the inertia of LAPACK's eigenvalues; scaled residual <= 1e-12;
forward error against the refined reference, relative to max(1, |x_ref|), <= tol_f = min(1e-7, max(1e-12, 1000 e_plain)) (tests/test_gpu_big_solve.py;
on band_hostile not below ten times the specification's own error, which is smaller here); a repeated solve and a repeated factor-and-solve bitwise
the same; pivot statistics (num_neg, num_zero, num_two, num_small) those of the specification -- with fast_blocks=False on the strict leg.

Between the legs of a fixture (pivot data = dinv, doff, ptype, lperm of mi355x_kkt_debug_pivots):
  default, levels, nopair   one factorisation: pivot data bitwise equal, solutions within 2 tol_f
  noleaf against levels     pivot data bitwise equal (the leaf chains are front_dpp16_body's arithmetic step by step); solutions bitwise equal
  nodf, full against levels equal statistics; pivot data bitwise equal on the fronts of order <= 16 whose subtree holds no front of order 17 .. 32 (those go to
                            another kernel, and what they hand up differs in the last bits), ptype / lperm equal and dinv / doff within 1e-11 max(1, |.|)
                            everywhere else
  strict against levels     another factorisation: the specification's statistics with fast_blocks=False; solutions within 2 tol_f
Reject fixtures: on the prescribed fronts lperm is not the identity or ptype shows a 2x2 pivot (the static-order bodies write lperm = li: the strict
kernel was there), on no other front; every front of order <= 16 whose subtree holds no edited variable has pivot data bitwise those of the UNEDITED
matrix under the same options (the untouched fronts of order 17 .. 32, which the fall-back hands to k_front_reg<64, 4> and the unedited run to
front_lds32_body: same ptype / lperm, dinv / doff within 1e-11); the fall-back (levels leg) is bitwise the child under DISABLE=optimistic.
Every leg and every child is run ONCE per process, whatever its outcome: a later test that needs one that failed fails with the recorded text.
Back-off: ten factor-and-solves of leaf_reject in one child with verbose=1 -- ten bitwise equal solutions and pivot arrays, the fall-back message after
calls 1 and 9 only, none for a healthy handle afterwards.

Measured on an MI355X when the tests were written.  Every leg: all three statuses SUCCESS, the solve repeated and the factor-and-solve repeated bitwise
equal (pivot arrays included), statistics (num_neg, num_zero, num_two, num_small) equal to the specification's.  launches = (k_leaf_chain, k_front_df,
k_front_dpp16, k_front_reg<64, 4>, k_front_reg<64, 2>) records of the schedule the leg's first factorisation walks (the optimistic one; `full`: the full
one); lc = levels of the k_*_leafchain prefix; pair = levels of k_*_pair<16, 16> / <16> / <32>; k64 = levels of k_fwd<64> / k_bwd<64>; seg = levels
left to the chain sweeps; bound = tol_f as computed on that machine:
  fixture        leg      launches        lc   pair     k64  seg   statistics     residual  forward   bound
  leaf_edges     default  (1,1,0,0,0)       0  0/0/0      0   62   (2,0,0,0)      1.75e-16  1.55e-15  2.78e-12
  leaf_edges     levels   (1,1,0,0,0)      16  11/6/0     0   29   (2,0,0,0)      1.75e-16  1.55e-15  2.78e-12
  leaf_edges     nopair   (1,1,0,0,0)       0  0/0/0     33   29   (2,0,0,0)      1.75e-16  1.55e-15  2.78e-12
  leaf_edges     noleaf   (0,1,0,0,0)       0  27/6/0     0   29   (2,0,0,0)      1.75e-16  1.55e-15  2.78e-12
  leaf_edges     nodf     (0,0,62,6,0)      0  27/6/0     0   29   (2,0,0,0)      1.75e-16  1.55e-15  2.78e-12
  leaf_edges     strict   (0,0,0,62,0)      0  27/6/0     0   29   (2,0,0,0)      1.75e-16  1.55e-15  2.78e-12
  leaf_edges_w8  default  (1,1,0,0,0)       0  0/0/0      0   22   (0,0,0,0)      2.42e-16  6.66e-16  1.00e-12
  leaf_edges_w8  levels   (1,1,0,0,0)       6  4/3/0      0    9   (0,0,0,0)      2.42e-16  5.55e-16  1.00e-12
  leaf_edges_w8  nopair   (1,1,0,0,0)       0  0/0/0     13    9   (0,0,0,0)      2.42e-16  6.66e-16  1.00e-12
  leaf_edges_w8  noleaf   (0,1,0,0,0)       0  10/3/0     0    9   (0,0,0,0)      2.42e-16  5.55e-16  1.00e-12
  leaf_edges_w8  nodf     (0,0,22,3,0)      0  10/3/0     0    9   (0,0,0,0)      2.42e-16  5.55e-16  1.00e-12
  leaf_edges_w8  strict   (0,0,0,22,0)      0  10/3/0     0    9   (0,0,0,0)      2.42e-16  5.55e-16  1.00e-12
  wave_edges     default  (0,1,0,0,0)       0  0/0/0      0    3   (0,0,0,0)      2.81e-16  7.77e-16  1.00e-12
  wave_edges     levels   (0,1,0,0,0)       0  0/0/3      0    0   (0,0,0,0)      2.25e-16  1.11e-15  1.00e-12
  wave_edges     nopair   (0,1,0,0,0)       0  0/0/0      3    0   (0,0,0,0)      2.81e-16  8.88e-16  1.00e-12
  wave_edges     noleaf   (0,1,0,0,0)       0  0/0/3      0    0   (0,0,0,0)      2.25e-16  1.11e-15  1.00e-12
  wave_edges     nodf     (0,0,2,3,0)       0  0/0/3      0    0   (0,0,0,0)      2.25e-16  1.11e-15  1.00e-12
  wave_edges     strict   (0,0,0,3,0)       0  0/0/3      0    0   (0,0,0,0)      2.25e-16  1.11e-15  1.00e-12
  leaf_reject    default  (1,1,0,0,0)       0  0/0/0      0   62   (6,0,1,0)      1.75e-16  2.22e-15  1.14e-10
  leaf_reject    levels   (1,1,0,0,0)      16  11/6/0     0   29   (6,0,1,0)      1.75e-16  2.66e-15  1.14e-10
  leaf_reject    nopair   (1,1,0,0,0)       0  0/0/0     33   29   (6,0,1,0)      1.75e-16  2.35e-15  1.14e-10
  leaf_reject    noleaf   (0,1,0,0,0)       0  27/6/0     0   29   (6,0,1,0)      1.75e-16  2.66e-15  1.14e-10
  leaf_reject    nodf     (0,0,62,6,0)      0  27/6/0     0   29   (6,0,1,0)      1.75e-16  2.66e-15  1.14e-10
  leaf_reject    strict   (0,0,0,62,0)      0  27/6/0     0   29   (6,0,1,0)      1.75e-16  2.66e-15  1.14e-10
  wave_reject    default  (0,1,0,0,0)       0  0/0/0      0    3   (4,0,1,0)      2.25e-16  7.77e-15  8.26e-10
  wave_reject    levels   (0,1,0,0,0)       0  0/0/3      0    0   (4,0,1,0)      2.81e-16  6.44e-15  8.26e-10
  wave_reject    nopair   (0,1,0,0,0)       0  0/0/0      3    0   (4,0,1,0)      1.69e-16  1.09e-14  8.26e-10
  wave_reject    noleaf   (0,1,0,0,0)       0  0/0/3      0    0   (4,0,1,0)      2.81e-16  6.44e-15  8.26e-10
  wave_reject    nodf     (0,0,2,3,0)       0  0/0/3      0    0   (4,0,1,0)      2.81e-16  6.44e-15  8.26e-10
  wave_reject    strict   (0,0,0,3,0)       0  0/0/3      0    0   (4,0,1,0)      2.81e-16  2.91e-14  8.26e-10
  band_hostile   default  (1,1,0,0,0)       0  0/0/0      0    8   (298,0,14,0)   1.35e-15  6.44e-15  2.00e-12
  band_hostile   levels   (1,1,0,0,0)       3  2/1/0      0    2   (298,0,14,0)   1.26e-15  1.09e-14  2.00e-12
  band_hostile   nopair   (1,1,0,0,0)       0  0/0/0      6    2   (298,0,14,0)   2.42e-15  1.42e-14  2.00e-12
  band_hostile   noleaf   (0,1,0,0,0)       0  5/1/0      0    2   (298,0,14,0)   1.26e-15  1.09e-14  2.00e-12
  band_hostile   nodf     (0,0,8,1,0)       0  5/1/0      0    2   (298,0,14,0)   1.26e-15  1.09e-14  2.00e-12
  band_hostile   strict   (0,0,0,8,0)       0  5/1/0      0    2   (298,0,23,0)   4.53e-16  2.89e-15  2.00e-12
  leaf_edges     full     (0,0,62,62,0)    16  11/6/0     0   29   (2,0,0,0)      1.75e-16  1.55e-15  2.78e-12
  wave_edges     full     (0,0,2,3,0)       0  0/0/3      0    0   (0,0,0,0)      2.25e-16  1.11e-15  1.00e-12
  leaf_reject    full     (0,0,62,62,0)    16  11/6/0     0   29   (6,0,1,0)      1.75e-16  2.66e-15  1.14e-10
Between the legs (against `levels`): the four pivot arrays were bitwise equal on EVERY front for default, nopair, noleaf, nodf and full on every fixture --
the fronts of order 17 .. 32 included, where only rounding agreement is asked of nodf and full: on these systems the strict k_front_reg<64, 4> finds
the natural order and the same bits as front_lds32_body.  Solutions: noleaf, nodf and full bitwise equal to levels on every fixture (k_*_leafchain against
k_*_pair<16, 16>: one definition of the front body), asserted for noleaf and for the fall-back against full; default (chain sweeps) and nopair
(k_fwd<64> / k_bwd<64>) differ from levels by 5.6e-16 .. 1.4e-14, never bitwise; strict by 0 (leaf_edges, leaf_reject: bitwise) .. 3.6e-14.
Reject fixtures, default and levels legs: the strict kernel's signature on supernodes 30, 52, 125, 136 of leaf_reject (2x2 pivot in 52) and 8, 34, 36 of
wave_reject (2x2 pivot in 8) and on no other; all 125 of 186 and 5 of 38 untouched fronts of order <= 16 bitwise equal to the unedited run, and so were
the 6 and 27 untouched fronts of order 17 .. 32, of which only rounding agreement is asked (another kernel in the two runs); levels bitwise the child
under DISABLE=optimistic.  Back-off: the fall-back message after calls 1 and 9, ten bitwise equal results, none for the healthy handle.  The whole
file ran in 16 s (four child processes of 2 .. 3 s).  No kernel had to be changed.

That the tests can fail was tried once with a library built with three arithmetic mutations: (1) the stride of the tagged contribution square fixed at
16 in front_lds32_body -- on the writing side as well: with the reader alone the parent waits for entries nobody tags and the launch runs into its own
time-out, which is a stall and not an arithmetic fault; (2) the remainder loop behind the 48 prefetched input entries of k_leaf_chain skipped; (3) the
loop of k_fwd_pair over the children beyond the fourth skipped.  22 of 48 tests failed and nothing else did:
  (1) wave_edges [default], [nopair] (residual 9.2e-4; neither leg runs a pair kernel), and with (3) on [levels], [noleaf], [full]; wave_reject passes on
      its default and nopair legs, as it must: the fall-back discards what the data-flow run computed;
  (2) leaf_edges [default], [levels], [nopair] (residual 7.5e-4) and leaf_edges_w8 on the same legs (wrong inertia: status 2); their noleaf, nodf and
      strict legs, which do not launch k_leaf_chain, passed; the back-off test failed on the healthy handle's residual; leaf_reject passes (fall-back);
  (3) wave_edges and wave_reject [levels], [noleaf], [nodf], [strict], wave_edges [full] (residual 2.5e-3);
  with them the between-the-legs tests of leaf_edges, leaf_edges_w8, wave_edges and wave_reject.  band_hostile and leaf_reject never failed.
"""
import hashlib
import json
import os
import subprocess
import sys
import ctypes as C

import numpy as np
import pytest
import torch      # noqa: F401  (before the library is loaded: torch brings its own HIP runtime)

from ipopt_amd import kkt
from tests.support import reach as R, smallfix as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES_TOL = 1e-12            # scaled residual, as in test_gpu_parity.py
ROUND_TOL = 1e-11          # two operation orders of the same factorisation (tests/test_gpu_fast_paths.py)
FALLBACK = "met a front for the strict kernels, running the full one"
PIV = ("dinv", "doff", "ptype", "lperm")


def sres(K, x, b):
    return np.abs(K @ x - b).max() / (abs(K).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max() + 1e-300)


def pivots(s, n):
    dinv, doff = np.zeros(n), np.zeros(n)
    pt, lp = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    s.lib.mi355x_kkt_debug_pivots.argtypes = [C.c_void_p] * 5
    assert s.lib.mi355x_kkt_debug_pivots(s._h, dinv.ctypes.data, doff.ctypes.data, pt.ctypes.data, lp.ctypes.data) == 0
    return dinv, doff, pt, lp


def stats_of(I):
    return (int(I.num_neg), int(I.num_zero), int(I.num_two), int(I.num_small))


def factor_and_solves(name, leg, opts_of=None, **more):
    """factor + solve the three right-hand sides; solve again; factor and solve again -- under the knobs of the leg"""
    S = X.system(name)
    with X.leg_knobs(leg):
        s = X.handle(name, opts_of, **more)
        facts = R.small_reach(s)
        T = X.fronts(s)
        s.values()[:] = S["v"]
        x = S["B"].copy()
        st = s.multi_solve(True, x, True, S["neg"])
        I = s.info()
        piv = pivots(s, S["n"])
        x2 = S["B"].copy()
        st2 = s.multi_solve(False, x2)
        x3 = S["B"].copy()
        st3 = s.multi_solve(True, x3, True, S["neg"])
        piv3 = pivots(s, S["n"])
        neg = int(s.number_of_neg_evals())
        s.close()
    return dict(st=(int(st), int(st2), int(st3)), neg=neg, stats=stats_of(I), x=x, piv=piv, facts=facts, T=T, solve_again=bool(np.array_equal(x, x2)),
                factor_again=bool(np.array_equal(x, x3) and all(np.array_equal(a, b) for a, b in zip(piv, piv3))))


def child_main(name, leg, out):
    """one leg in a process of its own (`optimistic` is read at the first factorisation of a process)"""
    leg_ = factor_and_solves(name, leg)
    np.savez(out, x=leg_["x"], **dict(zip(PIV, leg_["piv"])))
    keep = {k: leg_[k] for k in ("st", "neg", "stats", "solve_again", "factor_again")}
    keep["sha256"] = hashlib.sha256(leg_["x"].tobytes()).hexdigest()
    keep["counts"] = leg_["facts"]["solve_level_counts"]
    print("LEG " + json.dumps(keep))


def child_backoff(out):
    """ten factor-and-solves of the SAME values of leaf_reject on one handle with verbose=1, then a healthy handle: what factor() says, call by call"""
    S = X.system("leaf_reject")
    xs, pv, sts = [], [], []
    with X.leg_knobs("default"):
        s = X.handle("leaf_reject", verbose=1)
        for i in range(10):
            sys.stderr.write(f"CALL {i + 1}\n"); sys.stderr.flush()
            s.values()[:] = S["v"]
            x = S["B"].copy()
            sts.append(int(s.multi_solve(True, x, True, S["neg"])))
            xs.append(x); pv.append(pivots(s, S["n"]))
        s.close()
        sys.stderr.write("HEALTHY\n"); sys.stderr.flush()
        H = X.system("leaf_edges")
        h = X.handle("leaf_edges", verbose=1)
        h.values()[:] = H["v"]
        xh = H["B"].copy()
        sth = int(h.multi_solve(True, xh, True, H["neg"]))
        h.close()
        sys.stderr.write("END\n"); sys.stderr.flush()
    np.savez(out, x=np.stack(xs), xh=xh, **{w: np.stack([p[i] for p in pv]) for i, w in enumerate(PIV)})
    print("LEG " + json.dumps(dict(st=sts, sth=sth)))


OUTCOME = {}      # what was run once, and how it ended: a result, or the text of its failure -- nothing is started a second time in a process


def once(key, run):
    """run() the first time the key is asked for; afterwards its result -- or, if it failed (a fault, an abort, a time limit, an assertion), pytest.fail with
    the recorded text: a leg or a child that has failed is not started on the device again by the next test that needs it"""
    if key not in OUTCOME:
        try:
            OUTCOME[key] = (True, run())
        except BaseException as e:      # (a failed assertion, subprocess.TimeoutExpired, a HIP error surfacing as an exception ... all count)
            OUTCOME[key] = (False, f"{key}: failed when it was first run and is not run again: {type(e).__name__}: {e}"[:4000])
            raise
    ok, value = OUTCOME[key]
    if not ok:
        pytest.fail(value)
    return value


def run_child(code, path):
    """one child process, started once (callers go through once()): a fresh process, since nothing replaces the program of one that holds the device"""
    p = subprocess.run([sys.executable, "-c", "from tests.test_gpu_small_fronts import child_main, child_backoff; " + code], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, f"exit status {p.returncode}: " + p.stdout[-2000:] + p.stderr[-2000:]
    leg = json.loads(next(l for l in p.stdout.splitlines() if l.startswith("LEG "))[4:])
    Z = np.load(path)
    return leg, {w: Z[w] for w in Z.files}, p.stderr


def run_leg(name, leg, opts_of=None):
    """a leg of a fixture, ONCE per process whether it succeeds or not: in this process, or (`full`) in a child -- one child at a time, no second try.
    opts_of: the matrix of `name` under the options of that fixture"""
    return once((name, leg, opts_of), lambda: _run_leg(name, leg, opts_of))


def _run_leg(name, leg, opts_of):
    if X.LEGS[leg][2]:
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "leg.npz")
            out, Z, _ = run_child(f"child_main({name!r}, {leg!r}, {path!r})", path)
        out["x"] = Z["x"]; out["piv"] = tuple(Z[w] for w in PIV)
        assert hashlib.sha256(out["x"].tobytes()).hexdigest() == out["sha256"]
        out["st"] = tuple(out["st"]); out["stats"] = tuple(out["stats"])
        with X.leg_knobs(leg):
            s = X.handle(name)
            out["facts"] = R.small_reach(s); out["T"] = X.fronts(s)
            s.close()
        assert out["facts"]["solve_level_counts"] == out["counts"]
    else:
        out = factor_and_solves(name, leg, opts_of)
    out["x"].setflags(write=False)
    for a in out["piv"]:
        a.setflags(write=False)
    return out


def check_reach(name, leg, F):
    """the facts the leg stands on, from the handle that ran it"""
    base = X.system(name)["base"] or name
    lc, df, dpp, reg4, reg2 = F["opt"]
    c = F["solve_level_counts"]
    assert F["classes"] == [R.FC_WAVE]
    if leg in ("default", "levels", "nopair", "full"):
        assert df == 1 and (dpp, reg4) == (0, 0) and lc == (1 if base != "wave_edges" else 0)
    if leg == "default":
        assert F["seg_levels"] == F["num_levels"]
    if leg in ("levels", "full"):
        assert c["k64"] == 0 and c["16x16"] + c["16"] + c["32"] > 0 and (F["leafchain_solve"] > 0 or base == "wave_edges")
    if leg == "nopair":
        assert c["k64"] > 0 and F["leafchain_solve"] == 0 and c["16x16"] + c["16"] + c["32"] == 0
    if leg == "noleaf":
        assert lc == 0 and df == 1 and F["df_runs"][0][0] == 0
    if leg == "nodf":
        assert (lc, df) == (0, 0) and dpp > 0 and reg4 > 0
    if leg == "strict":
        assert (lc, df, dpp) == (0, 0, 0) and reg4 == F["num_levels"]
    if base == "leaf_edges":
        assert F["lc_levels"] == (16 if leg not in ("noleaf", "nodf", "strict") else 0) and F["num_levels"] == 62
        if leg in ("default", "levels", "nopair", "full"):
            assert dict(F["chain_lengths"])[16] == 2 and dict(F["chain_lengths"])[1] == 3 and F["lc_nchains"] == 15 and F["links_over_48_entries"] == 3
        if leg == "levels":
            assert c["16x16"] > 0 and c["16"] > 0 and F["leafchain_solve"] == 16
    if base == "leaf_edges_w8" and leg in ("default", "levels", "nopair"):
        assert F["link_max_entries"] == 100 and F["lc_nchains"] == 13
    if base == "wave_edges":
        assert (32, 32, 0) in F["shapes"] and F["max_gathered"] == 6 and F["wave_k_over_16"] == 14
        if df:      # the tagged squares of both sizes, five children of 18 rows under a front of 30, six gathered children
            assert {15, 16, 17, 18} <= set(F["tagged_rows"]) and F["tagged32"] == 6 and F["tagged_parents_17_32_children"] == 5 and F["df_max_gathered"] == 6
        if leg in ("levels", "noleaf", "nodf", "strict", "full"):
            assert c["32"] == 3 and F["pair32_k_over_16"] == 14 and F["max_gathered_on_levels"] == 6


@pytest.mark.parametrize("fixture,leg", X.CASES + X.CHILD_CASES)
def test_small_fronts_against_the_refined_reference(fixture, leg):
    S = X.system(fixture)
    ref, _, eig_neg = X.reference(fixture)
    tol = X.fwd_bound(fixture)
    out = run_leg(fixture, leg)
    F = out["facts"]
    check_reach(fixture, leg, F)
    res = max(sres(S["K"], out["x"][k], S["B"][k]) for k in range(3))
    fwd = X.relmax(out["x"], ref)
    spec = X.spec(fixture, leg != "strict")[0]
    c = F["solve_level_counts"]
    print(f"{fixture} [{leg}]: status {out['st']} neg {out['neg']} stats {out['stats']} specification {spec} residual {res:.2e} forward {fwd:.2e} bound {tol:.2e} "
          f"solve again bitwise {out['solve_again']} factor again bitwise {out['factor_again']} | factor launches opt {F['opt']} full {F['full']} | solve levels "
          f"leafchain {F['leafchain_solve']} pair<16,16>/<16>/<32> {c['16x16']}/{c['16']}/{c['32']} k64 {c['k64']} chain sweeps {F['seg_levels']}")
    assert out["st"] == (kkt.SUCCESS,) * 3
    assert out["neg"] == S["neg"] == eig_neg and out["stats"][0] == S["neg"]
    assert res <= RES_TOL
    assert fwd <= tol
    assert out["solve_again"]
    assert out["factor_again"]
    assert out["stats"] == spec


def piv_diff(a, b, T, fronts_):
    """(the arrays that differ on the columns of the given fronts, worst difference of dinv / doff relative to max(1, |.|))"""
    cols = np.concatenate([np.arange(T["colptr"][f], T["colptr"][f + 1]) for f in fronts_]) if len(fronts_) else np.zeros(0, dtype=int)
    bad = [w for w, p, q in zip(PIV, a, b) if not np.array_equal(p[cols], q[cols])]
    d = max((float((np.abs(p[cols] - q[cols]) / np.maximum(1.0, np.abs(q[cols]))).max()) for p, q in zip(a[:2], b[:2])), default=0.0) if len(cols) else 0.0
    return bad, d


def has_wide_below(T):
    """mask over the supernodes: the subtree of the front holds a front of order 17 .. 32 (itself included)"""
    wide = T["order"] > 16
    for f in range(len(wide)):      # (children come before their parents)
        p = int(T["parent"][f])
        if p >= 0 and wide[f]:
            wide[p] = True
    return wide


@pytest.mark.parametrize("fixture", sorted(X.FIXTURES))
def test_the_legs_of_a_fixture_agree(fixture):
    legs = X.FIXTURES[fixture][3]
    tol = X.fwd_bound(fixture)
    outs = {leg: run_leg(fixture, leg) for leg in legs}
    L = outs["levels"]
    T = L["T"]
    every = np.arange(len(T["cols"]))
    narrow = every[~has_wide_below(T)]
    for leg in legs:
        if leg == "levels":
            continue
        o = outs[leg]
        d = X.relmax(o["x"], L["x"])
        bad, dp = piv_diff(o["piv"], L["piv"], T, every)
        bad16, _ = piv_diff(o["piv"], L["piv"], T, narrow)
        print(f"{fixture}: {leg} against levels: solutions differ by {d:.2e} (2 x bound {2 * tol:.2e}), bitwise {np.array_equal(o['x'], L['x'])}; pivot arrays that differ "
              f"{bad or 'none'} (dinv / doff by {dp:.2e}), on the {len(narrow)} of {len(every)} fronts with nothing of order 17 .. 32 below: {bad16 or 'none'}")
        assert d <= 2 * tol, leg
        if leg == "strict":
            continue
        assert o["stats"] == L["stats"], leg
        if leg in ("default", "nopair", "noleaf"):
            assert not bad, leg
        else:      # nodf, full: the fronts of order 17 .. 32 by another kernel
            assert not bad16, leg
            assert not {"ptype", "lperm"} & set(bad) and dp <= ROUND_TOL, leg
        if leg == "noleaf" or (leg == "full" and X.system(fixture)["base"]):      # the same solve schedule on the same factor / the fall-back IS the full schedule
            assert np.array_equal(o["x"], L["x"]), leg


@pytest.mark.parametrize("fixture", ["leaf_reject", "wave_reject"])
def test_rejected_fronts_go_to_the_strict_kernel_and_nothing_else_changes(fixture):
    S = X.system(fixture)
    tiny = sorted(X.LEAF_TINY if fixture == "leaf_reject" else X.WAVE_TINY)
    for leg in ("default", "levels"):
        out = run_leg(fixture, leg)
        base = run_leg(S["base"], leg, fixture)      # the unedited matrix under the options of the edited one
        T = out["T"]
        assert all(np.array_equal(T[k], base["T"][k]) for k in T)
        prescribed = sorted(set(X.front_of(T, tiny)))
        dinv, doff, ptype, lperm = out["piv"]
        strict_sign = [f for f in range(len(T["cols"]))
                       if not np.array_equal(lperm[T["colptr"][f]:T["colptr"][f + 1]], np.arange(T["cols"][f])) or (ptype[T["colptr"][f]:T["colptr"][f + 1]] != 1).any()]
        two = [f for f in prescribed if (ptype[T["colptr"][f]:T["colptr"][f + 1]] == 2).any()]
        # every front of order <= 16 with no edited variable in its subtree -- those above a front of order 17 .. 32 included, although that front went to
        # k_front_reg<64, 4> here (the fall-back walks the full schedule) and to front_lds32_body in the unedited run (the optimistic one)
        touched = X.touched(T, tiny)
        clean = [f for f in range(len(T["cols"])) if not touched[f] and T["order"][f] <= 16]
        wide = [f for f in range(len(T["cols"])) if not touched[f] and T["order"][f] > 16]
        bad, _ = piv_diff(out["piv"], base["piv"], T, clean)
        bad_wide, dw = piv_diff(out["piv"], base["piv"], T, wide)
        print(f"{fixture} [{leg}]: prescribed fronts {prescribed}, strict kernel's signature on {strict_sign}, 2x2 pivot in {two}; {len(clean)} of {len(T['cols'])} fronts compared with the "
              f"unedited run (statistics {base['stats']}): arrays that differ {bad or 'none'}; on the {len(wide)} untouched fronts of order 17 .. 32: {bad_wide or 'none'} ({dw:.2e})")
        assert base["st"] == (kkt.SUCCESS,) * 3 and base["stats"][1:] == (0, 0, 0)
        assert strict_sign == prescribed
        assert len(two) == 1 and out["stats"][2] == 1
        assert len(clean) >= 4 and not bad
        assert not {"ptype", "lperm"} & set(bad_wide) and dw <= ROUND_TOL      # (another kernel in the two runs: to rounding)
    # the fall-back reruns the full schedule on the same values: bitwise the process that never tried the optimistic one
    if "full" in S["legs"]:
        a, b = run_leg(fixture, "levels"), run_leg(fixture, "full")
        assert np.array_equal(a["x"], b["x"]) and all(np.array_equal(p, q) for p, q in zip(a["piv"], b["piv"]))


def test_back_off_after_a_fall_back(tmp_path):
    """factor(): a fall-back sets a wait of 8 factorisations on the full schedule, the 9th call tries the optimistic one again (and falls back again: wait 16).
    Whatever schedule ran, the same values give the same bits -- a front left marked by the optimistic attempt (hasis) would be skipped by the full one"""
    path = str(tmp_path / "backoff.npz")
    out, Z, err = once("back-off child", lambda: run_child(f"child_backoff({path!r})", path))
    S, H = X.system("leaf_reject"), X.system("leaf_edges")
    assert out["st"] == [kkt.SUCCESS] * 10 and out["sth"] == kkt.SUCCESS
    said, where = {}, None
    for line in err.splitlines():
        if line.startswith("CALL ") or line in ("HEALTHY", "END"):
            where = line; said[where] = 0
        elif FALLBACK in line:
            said[where] += 1
    print("fall-back messages:", said)
    assert said == {**{f"CALL {i}": (1 if i in (1, 9) else 0) for i in range(1, 11)}, "HEALTHY": 0, "END": 0}
    for w in ("x",) + PIV:
        assert all(np.array_equal(Z[w][0], Z[w][i]) for i in range(1, 10)), w
    assert max(sres(S["K"], Z["x"][0][k], S["B"][k]) for k in range(3)) <= RES_TOL
    assert np.array_equal(Z["x"][0], run_leg("leaf_reject", "default")["x"])
    assert np.array_equal(Z["xh"], run_leg("leaf_edges", "default")["x"])
    assert max(sres(H["K"], Z["xh"][k], H["B"][k]) for k in range(3)) <= RES_TOL
