"""Row maps (mi355x_kkt_lowrank_rowmap, mi355x_kkt_lbfgs_push_mapped; K + P (V V^T - U U^T) P^T with nv = nu = 12): three comparisons on bench workloads,
each measured in ONE run with the two sides alternating (comparison 1 on one handle that is switched between them), host clock around calls that end in a device synchronisation, medians after warm-up.
  1. the cost of a map: lowrank_update, a corrected solve and a push under (a) every second x index, (b) a contiguous block of 60 % of x starting at
     n_x / 5 -- against the unmapped call with the SAME number of rows (the first `rows` indices).  No pass bar: the ratios are recorded.
  2. why anyone wants it: the mapped push (two full-space host vectors up, V and U formed on the device) against the only route there was -- the numpy
     specification forms V and U, the host zero-pads them to n_x rows, lowrank_set uploads the 2 m columns.
  3. no regression of the unmapped path: unmapped lowrank_update, corrected solve and lbfgs_push of this tree against a built checkout of the parent
     commit (--parent-tree PATH; each side in fresh child processes, A B A B), next to the spread of the same tool on this tree against itself (A/A).
     Without --parent-tree the comparison is recorded as not measured.
usage: python tools/rowmap_time.py [--parent-tree PATH] [workload ...]      (writes profiles/rowmap_time.json)"""
import os, sys, time, json, subprocess
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = len(sys.argv) > 1 and sys.argv[1] == "--child"
ROOT = sys.argv[2] if CHILD else HERE          # (a child measures the tree it is given: this one, or the parent's)
sys.path.insert(0, ROOT)
import numpy as np, torch
import ipopt_amd, bench
from ipopt_amd import kkt
from tests.support import lbfgs_spec as lb

NV = NU = 12
KHIST = 6
REPS, WARM = 15, 3


def timed(call):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def alternate(calls, reps=REPS, warm=WARM):
    """calls: name -> callable; every repetition runs each once, in order; -> name -> median ms"""
    t = {k: [] for k in calls}
    for i in range(warm + reps):
        for k, f in calls.items():
            ms = timed(f)
            if i >= warm:
                t[k].append(ms)
    return {k: float(np.median(v)) for k, v in t.items()}


def factored(wl):
    n, r, c, v, neg = bench.make_workload(wl)
    s = ipopt_amd.KKTSolver(device=0)
    s.initialize_structure(n, r, c, vals=v)
    dv = torch.tensor(v, dtype=torch.float64, device="cuda")
    st = s.factor_device(dv.data_ptr())
    assert st[0] == 0 and st[1] == neg
    return s, n, n - neg


def columns(rows, seed=3):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((rows, NV)) / np.sqrt(rows), rng.standard_normal((rows, NU)) / np.sqrt(rows)


def set_until_admissible(handles, V, U):
    """M1 is positive definite for any V; U is halved until M2 is as well on every handle (tools/lowrank_time.py)"""
    for _ in range(60):
        ok = True
        for s in handles:
            s.lowrank_set(V, U)
            ok = ok and s.lowrank_update() == (kkt.SUCCESS, 0)
        if ok:
            return U
        U = 0.5 * U
    raise RuntimeError("no admissible U")


def pool_of(length, k, seed=3):
    Sp, Yp = lb.make_pairs(length, k + 1, seed=seed)
    return [(np.ascontiguousarray(Sp[:, j]), np.ascontiguousarray(Yp[:, j])) for j in range(k + 1)]


def unmapped_three(s, n, rows):
    """medians of the three unmapped calls on a factored handle: what a child reports"""
    V, U = columns(rows)
    set_until_admissible([s], V, U)
    b = torch.randn(n, dtype=torch.float64, device="cuda"); x = torch.empty_like(b)
    out = alternate({"lowrank_update_ms": s.lowrank_update, "corrected_solve_ms": lambda: s.lowrank_solve_device2(b.data_ptr(), x.data_ptr())})
    s.lowrank_clear()
    pool = pool_of(rows, KHIST)
    s.lbfgs_define(rows, KHIST)
    for j in range(KHIST):
        assert s.lbfgs_push(*pool[j]) == kkt.LBFGS_STORED
    it = iter(range(KHIST, 10 ** 6))
    out.update(alternate({"lbfgs_push_ms": lambda: s.lbfgs_push(*pool[next(it) % (KHIST + 1)])}))
    s.lbfgs_clear(); s.lowrank_clear()
    return out


if CHILD:
    s, n, nx = factored(sys.argv[3])
    print(json.dumps(unmapped_three(s, n, nx)), flush=True)
    sys.exit(0)

args = sys.argv[1:]
parent = None
if "--parent-tree" in args:
    i = args.index("--parent-tree"); parent = os.path.abspath(args[i + 1]); del args[i:i + 2]
results = []
for wl in (args or ["grid_1e5", "lukvle1_1e6"]):
    sm, n, nx = factored(wl)          # the handle of comparison 1, switched between a map and none, and the mapped side of comparison 2
    su, _, _ = factored(wl)           # the host route of comparison 2: n_x rows, no map
    out = {"workload": wl, "kkt_dim": n, "n_x": nx, "nv": NV, "nu": NU, "max_history": KHIST, "maps": {},
           "samples": "comparison 1: 7 switches per side after 2 (update 1, solves 5 after 1 per switch), pushes 3 switches of 7 after 1; comparison 2: 7 after 2; comparison 3: 15 after 3 per child",
           "timing": "host clock around calls that end in a device synchronisation; the two sides of every comparison alternate in one run; medians"}
    b = torch.randn(n, dtype=torch.float64, device="cuda"); x = torch.empty_like(b)
    torch.cuda.synchronize()
    maps = {"every_second_index": np.arange(0, nx, 2, dtype=np.int32), "block_60_percent_at_one_fifth": np.arange(nx // 5, nx // 5 + (3 * nx) // 5, dtype=np.int32)}
    for name, idx in maps.items():
        rows = idx.size
        V, U = columns(rows)
        full = pool_of(nx, KHIST)
        red = [(np.ascontiguousarray(a[idx]), np.ascontiguousarray(c[idx])) for a, c in full]

        # comparison 1 runs on ONE handle that is switched between the two sides: the time of lowrank_update differs by tens of per cent between two
        # handles of one process on the same system, which a two-handle comparison would book to the map
        def switch(mapped, cols=True):
            sm.lbfgs_clear(); sm.lowrank_clear()
            sm.lowrank_rowmap(idx if mapped else None)
            if cols:
                sm.lowrank_set(V, U)
        for _ in range(60):
            ok = True
            for mapped in (True, False):
                switch(mapped)
                ok = ok and sm.lowrank_update() == (kkt.SUCCESS, 0)
            if ok:
                break
            U = 0.5 * U
        assert ok
        raw = {k: [] for k in ("mapped_update", "unmapped_update", "mapped_solve", "unmapped_solve", "mapped_push", "unmapped_push")}
        for rep in range(2 + 7):
            for mapped in (True, False):
                side = "mapped_" if mapped else "unmapped_"
                switch(mapped)
                ms = timed(sm.lowrank_update)
                solves = [timed(lambda: sm.lowrank_solve_device2(b.data_ptr(), x.data_ptr())) for _ in range(1 + 5)][1:]
                if rep >= 2:
                    raw[side + "update"].append(ms); raw[side + "solve"] += solves
        for rep in range(1 + 3):
            for mapped in (True, False):
                side = "mapped_" if mapped else "unmapped_"
                switch(mapped, cols=False)
                sm.lbfgs_define(rows, KHIST)
                push = (lambda j: sm.lbfgs_push_mapped(*full[j % (KHIST + 1)])) if mapped else (lambda j: sm.lbfgs_push(*red[j % (KHIST + 1)]))
                for j in range(KHIST + WARM):
                    assert push(j) == kkt.LBFGS_STORED
                pushes = [timed(lambda: push(j)) for j in range(KHIST + WARM, KHIST + WARM + 7)]
                if rep >= 1:
                    raw[side + "push"] += pushes
        t = {k: float(np.median(v)) for k, v in raw.items()}
        # comparison 2: the mapped push against the host route on the unmapped handle (n_x rows, zero-padded columns)
        switch(True, cols=False)
        sm.lbfgs_define(rows, KHIST)
        H = lb.History(rows, KHIST)
        for j in range(KHIST):
            assert sm.lbfgs_push_mapped(*full[j]) == kkt.LBFGS_STORED and H.push(*red[j]) == lb.STORED
        assert np.array_equal(sm.lbfgs_get("S"), H.S)
        Vp, Up = np.zeros((nx, KHIST), order="F"), np.zeros((nx, KHIST), order="F")

        def host_route(pair):
            sx, yx = pair
            assert H.push(sx[idx], yx[idx]) == lb.STORED
            Vp[idx] = H.V; Up[idx] = H.U
            su.lowrank_set(Vp, Up)
        its = [iter(range(KHIST, 10 ** 6)) for _ in range(2)]
        t2 = alternate({"mapped_push": lambda: sm.lbfgs_push_mapped(*full[next(its[0]) % (KHIST + 1)]),
                        "host_spec_zero_pad_lowrank_set": lambda: host_route(full[next(its[1]) % (KHIST + 1)])}, reps=7, warm=2)
        sm.lbfgs_clear(); sm.lowrank_clear(); su.lowrank_clear()
        out["maps"][name] = {"rows": int(rows), "ms": t,
                             "ratio_mapped_over_unmapped": {k: t["mapped_" + k] / t["unmapped_" + k] for k in ("update", "solve", "push")},
                             "push_against_host_route_ms": t2, "host_route_over_mapped_push": t2["host_spec_zero_pad_lowrank_set"] / t2["mapped_push"]}
        print(json.dumps({wl: {name: out["maps"][name]}}), flush=True)
    sm.lowrank_rowmap(None)
    sm.close(); su.close()
    del b, x
    torch.cuda.synchronize()
    # 3. the unmapped path of this tree against the parent's, each run in a fresh process, A B A B; A/A: this tree's two runs
    if parent:
        runs = {"this": [], "parent": []}
        for side in ("this", "parent", "this", "parent"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", HERE if side == "this" else parent, wl], capture_output=True, text=True)
            line = [l for l in p.stdout.splitlines() if l.startswith("{")]
            if p.returncode != 0 or not line:
                print(p.stdout[-2000:], p.stderr[-2000:]); sys.exit(1)      # (nothing more is started on the device behind a failed child)
            runs[side].append(json.loads(line[-1]))
        keys = list(runs["this"][0])
        mean = lambda side, k: 0.5 * (runs[side][0][k] + runs[side][1][k])
        out["unmapped_against_parent"] = {"runs_ms": runs,
                                          "this_over_parent": {k: mean("this", k) / mean("parent", k) for k in keys},
                                          "a_a_spread_this_tree": {k: abs(runs["this"][0][k] - runs["this"][1][k]) / mean("this", k) for k in keys}}
    else:
        out["unmapped_against_parent"] = "not measured (no --parent-tree)"
    print(json.dumps({wl: {"unmapped_against_parent": out["unmapped_against_parent"]}}), flush=True)
    results.append(out)
os.makedirs(os.path.join(HERE, "profiles"), exist_ok=True)
with open(os.path.join(HERE, "profiles", "rowmap_time.json"), "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
