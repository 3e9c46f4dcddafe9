"""On the device: what a factorisation LAUNCHED is what the host said it would launch.  The per-kind launch counts of the profiling entry point (hip
events around every launch of the eager schedule) against the records of the exported factor schedule "factor.single.full", on three fixtures:
grid30 (grouped, fused pivot-block + panel launch), clique_grid (two look-ahead forks, part 1 in 64 x 64 tiles, a side bucket) and lukvl1000 (the
levels the optimistic schedule would hand to the leaf chains and a data-flow run).

profile() walks the schedule of the handle's LAST factorisation -- optimistic or full -- so the leg runs where the full one is what a factorisation
takes: under MI355X_KKT_DISABLE=optimistic, which is read once per process, hence in one child process for the three fixtures.  profile(reps) zeroes
its counters and then adds every repetition: launches = reps x the launches of one factorisation + one solve."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ipopt_amd
from ipopt_amd import kkt
from tests.support import pathfix, reach as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["grid30", "clique_grid", "lukvl1000"]
KINDS = ["front_wave", "front_lds64", "front_lds128", "big_assemble", "big_diag", "big_trsm", "big_schur"]      # KK_FRONT_WAVE .. KK_BIG_SCHUR = 1 .. 7
REPS = 2


def child_main():
    out = {}
    for name in FIXTURES:
        S = pathfix.system(name)
        with pathfix.knobs("optimistic", S["tune"]):
            s = ipopt_amd.KKTSolver(**S["opts"])
            s.initialize_structure(S["n"], S["r"], S["c"], vals=S["v"])
            s.values()[:] = S["v"]
            x = S["B"].copy()
            st = s.multi_solve(True, x, True, S["neg"])
            prof = [int(v[1]) for v in s.profile(REPS).values()]
            full = s.launch_plan("factor.single.full").reshape(-1, R.REC)
        out[name] = dict(status=int(st), launches=prof, full=[int(np.sum(full[:, R.KIND] == k)) for k in range(len(prof))],
                         streams=[int(np.sum((full[:, R.STREAM] == q) & (full[:, R.KIND] >= 0))) for q in range(3)])
        del s
    print("COUNTS " + json.dumps(out))


def test_the_device_launches_what_the_host_schedule_lists():
    code = "from tests.test_gpu_factor_schedule import child_main; child_main()"
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)      # (a fresh process: nothing replaces the program of one that holds the device)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    got = json.loads(next(l for l in p.stdout.splitlines() if l.startswith("COUNTS "))[7:])
    names = list(kkt.KERNEL_KINDS)
    assert names[1:8] == KINDS
    for name in FIXTURES:
        G = got[name]
        print(name, "launches per kind over %d repetitions:" % REPS, dict(zip(names, G["launches"])), "records of factor.single.full:", dict(zip(names, G["full"])),
              "launch records per stream:", G["streams"])
        assert G["status"] == kkt.SUCCESS
        for k in range(1, 8):
            assert G["launches"][k] == REPS * G["full"][k], (name, names[k], G["launches"][k], G["full"][k])
        assert sum(G["full"][1:8]) == sum(G["streams"]) > 0
    # the fixtures reach what they are here for: look-ahead and side streams on clique_grid, the fused and grouped launches on grid30
    assert got["clique_grid"]["streams"][1] >= 2 and got["clique_grid"]["streams"][2] >= 1
    assert got["grid30"]["full"][5] >= 1 and got["lukvl1000"]["full"][1] >= 1
