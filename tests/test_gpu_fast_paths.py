"""-m gpu: every KEPT fast path against the plain path underneath it (MI355X_KKT_DISABLE=<knob>, ipopt_amd/csrc/env_knobs.h), on the smallest fixture
that REACHES the path -- tests/test_reach.py shows on the host that it does, and that switching the knob changes the plan there.

Both legs of a test: status SUCCESS; inertia exactly the fixture's (by construction, and by LAPACK's eigenvalues where n <= 3 000); scaled residual
<= 1e-12 (the project's bound, test_gpu_parity.sres); forward error <= 1e-7 max(1, |x_ref|) against a reference refined with longdouble residuals
(tests/support/pathfix.py; the fixtures are those on which a plain fp64 solve is within 1e-9 of it, so the cap hides nothing); a repeated
factor-and-solve of the same handle bitwise the same.  Between the legs: equal pivot statistics for every knob that does not change pivot decisions,
and solutions bitwise equal where both legs do the same floating-point operations in the same order per entry -- to rounding (1e-11 max(1, |x|),
the bound of test_sync_free_chain_sweeps...) only where the table says in which sum the order differs.

Measured on an MI355X when the table (tests/support/pathfix.py) was written -- worst scaled residual / forward error of the two legs, and the
difference between them: tfuse, xcd_tiles, xcd_affine, fuse_upd, fuse_dt, lookahead, p1_small, side_small, norestore and grouped on one-link groups
0 (bitwise) at residuals <= 1.4e-15 and forward errors <= 5.6e-13; grouped / selfasm on groups of several links 4.4e-16 (clique_grid) and 3.3e-14
(grid30); asm_pull 2.9e-13; front_df 5.7e-14; pair_solve 7.4e-13 (forward 5.2e-13 with, 7.5e-13 without); optimistic 5.7e-14 and 4.7e-14
(forward 1.0e-12 on lukvl40000); fastpiv 4.6e-13 (grid24), 3.3e-13 (lukvl1000, num_two 0 -> 9), 6.3e-13 (lukvl40000, num_two 0 -> 393)."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch      # noqa: F401  (before the library is loaded: torch brings its own HIP runtime)

import ipopt_amd
from ipopt_amd import kkt
from tests.support import pathfix

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES_TOL = 1e-12            # scaled residual, as in test_gpu_parity.py
FWD_TOL = 1e-7             # forward error against the refined reference, relative to max(1, |x_ref|)
ROUND_TOL = 1e-11          # two summation orders of the same factorisation (test_sync_free_chain_sweeps_match_the_level_by_level_solves)
BITWISE, ROUNDING, OTHER_PIVOTS, TABLE, OPTIMISTIC = pathfix.BITWISE, pathfix.ROUNDING, pathfix.OTHER_PIVOTS, pathfix.TABLE, pathfix.OPTIMISTIC


def sres(K, x, b):
    return np.abs(K @ x - b).max() / (abs(K).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max() + 1e-300)


def run_leg(name, disable):
    """factor + solve the fixture's three right-hand sides, twice, on a handle set up with MI355X_KKT_DISABLE=disable"""
    S = pathfix.system(name)
    with pathfix.knobs(disable, S["tune"]):
        s = ipopt_amd.KKTSolver(**S["opts"])
        s.initialize_structure(S["n"], S["r"], S["c"], vals=S["v"])
        s.values()[:] = S["v"]
        x = S["B"].copy()
        st = s.multi_solve(True, x, True, S["neg"])
        I = s.info()
        x2 = S["B"].copy()
        st2 = s.multi_solve(True, x2, True, S["neg"])
    leg = dict(st=int(st), st2=int(st2), neg=int(s.number_of_neg_evals()), num_two=I.num_two, num_small=I.num_small, num_zero=I.num_zero,
               num_fast=I.num_fast_blocks, x=x, repeat_equal=bool(np.array_equal(x, x2)))
    del s
    return leg


@functools.lru_cache(maxsize=None)
def default_leg(name):
    return run_leg(name, None)


def figures(name, leg):
    """(worst scaled residual, worst forward error relative to max(1, |x_ref|)) of a leg over the right-hand sides"""
    S = pathfix.system(name)
    ref, _, _ = pathfix.reference(name)
    res = max(sres(S["K"], leg["x"][k], S["B"][k]) for k in range(3))
    fwd = max(np.abs(leg["x"][k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max()) for k in range(3))
    return float(res), float(fwd)


def check_leg(name, leg, label):
    S = pathfix.system(name)
    _, _, eig_neg = pathfix.reference(name)
    res, fwd = figures(name, leg)
    print(f"{name} [{label}]: status {leg['st']} neg {leg['neg']} two {leg['num_two']} small {leg['num_small']} zero {leg['num_zero']} fast {leg['num_fast']} "
          f"residual {res:.2e} forward {fwd:.2e} repeat bitwise {leg['repeat_equal']}")
    assert leg["st"] == leg["st2"] == kkt.SUCCESS
    assert leg["neg"] == S["neg"] and (eig_neg is None or eig_neg == S["neg"])
    assert res <= RES_TOL
    assert fwd <= FWD_TOL
    assert leg["repeat_equal"]


def between(a, b):
    """(bitwise equal, worst difference relative to max(1, |x|)) of two legs' solutions"""
    d = max(np.abs(a["x"][k] - b["x"][k]).max() / max(1.0, np.abs(a["x"][k]).max()) for k in range(3))
    return bool(np.array_equal(a["x"], b["x"])), float(d)


def check_between(on, off, cls, label):
    same, d = between(on, off)
    print(f"{label}: legs bitwise {same}, difference {d:.2e} ({cls})")
    if cls != OTHER_PIVOTS:
        assert (on["num_two"], on["num_small"], on["num_zero"]) == (off["num_two"], off["num_small"], off["num_zero"])
    if cls == BITWISE:
        assert same
    elif cls == ROUNDING:
        assert d <= ROUND_TOL


@pytest.mark.parametrize("knob,fixture,how,cls,why", TABLE, ids=[f"{t[0]}-{t[1]}" for t in TABLE])
def test_fast_path_against_its_plain_path(knob, fixture, how, cls, why):
    on = default_leg(fixture)
    off = run_leg(fixture, knob)
    check_leg(fixture, on, "default")
    check_leg(fixture, off, "MI355X_KKT_DISABLE=" + knob)
    if knob == "fastpiv":      # reach observed in info(): pivot blocks of big fronts taken by the blocked static-order path (the band systems have no big front: the plan shows it there)
        assert off["num_fast"] == 0 and (on["num_fast"] > 0 or how != "info")
    check_between(on, off, cls, f"{knob} on {fixture}")


def child_main(name, disable, out):
    """one leg in a process of its own (`optimistic` is read once per process)"""
    leg = run_leg(name, disable)
    np.save(out, leg.pop("x"))
    leg["sha256"] = hashlib.sha256(np.load(out).tobytes()).hexdigest()
    print("LEG " + json.dumps(leg))


def child_leg(name, disable, path):
    code = f"from tests.test_gpu_fast_paths import child_main; child_main({name!r}, {disable!r}, {str(path)!r})"
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)      # (a fresh process: nothing replaces the program of one that holds the device)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    leg = json.loads(next(l for l in p.stdout.splitlines() if l.startswith("LEG "))[4:])
    leg["x"] = np.load(path)
    assert hashlib.sha256(leg["x"].tobytes()).hexdigest() == leg["sha256"]
    return leg


@pytest.mark.parametrize("fixture,cls,why", OPTIMISTIC, ids=[t[0] for t in OPTIMISTIC])
def test_optimistic_schedule_against_the_full_one(fixture, cls, why, tmp_path):
    """reach is INFERRED (tests/test_reach.py: leaf chains, a data-flow run, levels whose strict launch the optimistic schedule drops): neither info() nor
    the profile -- which switches the optimistic schedule off -- can tell the legs apart.  One child at a time, no second try."""
    on = child_leg(fixture, None, tmp_path / "on.npy")
    off = child_leg(fixture, "optimistic", tmp_path / "off.npy")
    check_leg(fixture, on, "default (child)")
    check_leg(fixture, off, "MI355X_KKT_DISABLE=optimistic (child)")
    same, d = between(on, off)
    print(f"optimistic on {fixture}: legs bitwise {same}, difference {d:.2e} ({cls})")
    assert same if cls == BITWISE else d <= ROUND_TOL

