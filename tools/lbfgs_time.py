"""Limited-memory BFGS pushes (mi355x_kkt_lbfgs_*): time of lbfgs_push with a FULL history of max_history 6 and 12 on bench workloads, next to its
yardstick measured in the same run on the same machine: the host route -- the numpy specification (tests/support/lbfgs_spec.py, float64) takes the
same pair, updates D, L, S^T S, forms V and U over the whole history, and lowrank_set uploads all 2 m columns.  Host clock around calls that end in a
device synchronisation, median of repeated calls after warm-up; the pairs cycle through a pool of max_history + 1 (a pair has left the history before
it comes round again).  Both routes end with the same columns installed: their largest relative difference is recorded.  No gate, no target.
usage: python tools/lbfgs_time.py [workload ...]      (writes profiles/lbfgs_time.json)"""
import os, sys, time, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import ipopt_amd, bench
from ipopt_amd import kkt
from tests.support import lbfgs_spec as lb

REPS, WARM = 11, 2
HBM_ACHIEVABLE = 6.3e12      # bytes / s


def timed(call):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def stats(t):
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}


results = []
for wl in (sys.argv[1:] or ["grid_1e5", "lukvle1_1e6"]):
    n, r, c, v, neg = bench.make_workload(wl)
    rows = n - neg                                             # the x block (the generators return neg = number of constraints)
    s = ipopt_amd.KKTSolver(device=0)
    s.initialize_structure(n, r, c, vals=v)
    for k in (6, 12):
        Sp, Yp = lb.make_pairs(rows, k + 1, seed=3)
        pool = [(np.ascontiguousarray(Sp[:, j]), np.ascontiguousarray(Yp[:, j])) for j in range(k + 1)]
        del Sp, Yp
        # device route
        s.lbfgs_define(rows, k)
        for j in range(k):
            assert s.lbfgs_push(*pool[j % (k + 1)]) == kkt.LBFGS_STORED
        t_dev = []
        for j in range(k, k + WARM + REPS):
            ms = timed(lambda: s.lbfgs_push(*pool[j % (k + 1)]))
            if j >= k + WARM:
                t_dev.append(ms)
        Vd, Ud, sigma_d = s.lbfgs_get("V"), s.lbfgs_get("U"), s.lbfgs_info()["sigma"]
        s.lbfgs_clear()
        # host route: the same pushes
        H = lb.History(rows, k)
        for j in range(k):
            assert H.push(*pool[j % (k + 1)]) == lb.STORED
        t_host, t_host_algebra = [], []

        def host_push(pair):
            t0 = time.perf_counter()
            assert H.push(*pair) == lb.STORED
            t_alg = 1e3 * (time.perf_counter() - t0)
            s.lowrank_set(H.V, H.U)
            return t_alg
        for j in range(k, k + WARM + REPS):
            alg = []
            ms = timed(lambda: alg.append(host_push(pool[j % (k + 1)])))
            if j >= k + WARM:
                t_host.append(ms); t_host_algebra.append(alg[0])
        scale = max(np.abs(H.V).max(), np.abs(H.U).max())
        diff = float(max(np.abs(Vd - H.V).max(), np.abs(Ud - H.U).max()) / scale)
        dev_ms, host_ms = stats(t_dev), stats(t_host)
        out = {"workload": wl, "kkt_dim": n, "rows": rows, "max_history": k, "memory": k, "reps": REPS, "warm": WARM,
               "lbfgs_push_ms": dev_ms,
               "host_route_ms": host_ms, "host_route_numpy_algebra_ms": stats(t_host_algebra),
               "winner": "device" if dev_ms["median"] < host_ms["median"] else "host", "host_over_device": host_ms["median"] / dev_ms["median"],
               "columns_max_relative_difference": diff, "sigma_device": sigma_d, "sigma_host": float(H.sigma),
               "model_dots_bytes": (2 * k + 2) * rows * 8, "model_form_bytes": (2 * (k - 1) + 2 + 2 + 2 * k) * rows * 8,
               "model_stream_ms_at_6.3TBps": 1e3 * ((2 * k + 2) + (4 * k + 2)) * rows * 8 / HBM_ACHIEVABLE,
               "model_host_upload_bytes": 2 * k * rows * 8,
               "timing": "host clock around one push, a device synchronisation before and after; median after warm-up; both routes in the same run"}
        print(json.dumps(out), flush=True)
        results.append(out)
        del Vd, Ud, H, pool
        s.lowrank_clear()
    s.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "lbfgs_time.json"), "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
