"""Limited-memory SR1 pushes (mi355x_kkt_lbfgs_define_sr1 + lbfgs_push): time of a push with a FULL history of max_history 6 and 12 on bench
workloads, next to two yardsticks measured in the same run on the same machine:
  host route   the numpy specification (tests/support/sr1_spec.py, float64) takes the same pair, updates D, L, S^T S, splits Z, forms V and U over
               the whole history, and lowrank_set uploads all m columns
  BFGS push    lbfgs_push on a BFGS history of the same shape on a second handle, alternating with the SR1 push: it moves the same bytes but for m
               columns less to write
Host clock around calls that end in a device synchronisation, median of repeated calls after warm-up; the pairs cycle through a pool of
max_history + 2 (a pair has left the history, and the SR1 ring's spare slot, before it comes round again).  No gate, no target.
usage: python tools/sr1_time.py [workload ...]      (writes profiles/sr1_time.json)"""
import os, sys, time, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import ipopt_amd, bench
from ipopt_amd import kkt
from tests.support import sr1_spec as sr

REPS, WARM = 11, 2
HBM_ACHIEVABLE = 6.3e12      # bytes / s


def timed(call):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def stats(t):
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}


def device_routes(handles, pool, k):
    """the same pushes on every handle, ALTERNATING between the handles push by push -> per handle (times of REPS pushes with a full history, all outcomes)"""
    P = len(pool)
    outcomes = [[h.lbfgs_push(*pool[j % P]) for j in range(k)] for h in handles]
    t = [[] for _ in handles]
    for j in range(k, k + WARM + REPS):
        for q, h in enumerate(handles):
            oc = []
            ms = timed(lambda: oc.append(h.lbfgs_push(*pool[j % P])))
            outcomes[q].append(oc[0])
            if j >= k + WARM:
                t[q].append(ms)
    return list(zip(t, outcomes))


results = []
for wl in (sys.argv[1:] or ["grid_1e5", "lukvle1_1e6"]):
    n, r, c, v, neg = bench.make_workload(wl)
    rows = n - neg                                             # the x block (the generators return neg = number of constraints)
    s = ipopt_amd.KKTSolver(device=0)
    s.initialize_structure(n, r, c, vals=v)
    s2 = ipopt_amd.KKTSolver(device=0)                         # the BFGS history lives on a handle of its own, so that the two pushes can alternate
    s2.initialize_structure(n, r, c, vals=v)
    for k in (6, 12):
        Sp, Yp = sr.make_pairs(rows, k + 2, seed=3)
        pool = [(np.ascontiguousarray(Sp[:, j]), np.ascontiguousarray(Yp[:, j])) for j in range(k + 2)]
        del Sp, Yp
        s.lbfgs_define_sr1(rows, k)
        s2.lbfgs_define(rows, k)
        (t_sr1, oc_sr1), (t_bfgs, oc_bfgs) = device_routes([s, s2], pool, k)
        Vd, Ud, sigma_d, nneg_d = s.lbfgs_get("V"), s.lbfgs_get("U"), s.lbfgs_info()["sigma"], s.lbfgs_sr1_info()["nneg"]
        s.lbfgs_clear(); s.lowrank_clear()
        s2.lbfgs_clear(); s2.lowrank_clear()
        # host route: the same pushes
        H = sr.History(rows, k)
        oc_host = [H.push(*pool[j % (k + 2)]) for j in range(k)]
        t_host, t_host_algebra = [], []

        def host_push(pair):
            t0 = time.perf_counter()
            oc_host.append(H.push(*pair))
            t_alg = 1e3 * (time.perf_counter() - t0)
            s.lowrank_set(H.V, H.U)
            return t_alg
        for j in range(k, k + WARM + REPS):
            alg = []
            ms = timed(lambda: alg.append(host_push(pool[j % (k + 2)])))
            if j >= k + WARM:
                t_host.append(ms); t_host_algebra.append(alg[0])
        op = lambda V, U: V[:256] @ V[:256].T - U[:256] @ U[:256].T                                          # (the leading 256 x 256 block of V V^T - U U^T)
        Bd, Bh = op(Vd, Ud), op(H.V, H.U)
        diff = float(np.abs(Bd - Bh).max() / np.abs(Bh).max())
        sr1_ms, bfgs_ms, host_ms = stats(t_sr1), stats(t_bfgs), stats(t_host)
        out = {"workload": wl, "kkt_dim": n, "rows": rows, "max_history": k, "memory": k, "reps": REPS, "warm": WARM,
               "sr1_push_ms": sr1_ms, "bfgs_push_ms": bfgs_ms,
               "host_route_ms": host_ms, "host_route_numpy_algebra_ms": stats(t_host_algebra),
               "sr1_over_bfgs": sr1_ms["median"] / bfgs_ms["median"], "host_over_sr1": host_ms["median"] / sr1_ms["median"],
               "sr1_outcomes_not_stored": int(sum(o != kkt.LBFGS_STORED for o in oc_sr1)), "bfgs_outcomes_not_stored": int(sum(o != kkt.LBFGS_STORED for o in oc_bfgs)),
               "host_outcomes_not_stored": int(sum(o != sr.STORED for o in oc_host)),
               "nneg_device": nneg_d, "nneg_host": int(H.nneg), "operator_max_relative_difference": diff, "sigma_device": sigma_d, "sigma_host": float(H.sigma),
               "model_dots_bytes": (2 * k + 2) * rows * 8, "model_form_bytes": (2 * (k - 1) + 2 + 2 + k) * rows * 8,
               "model_stream_ms_at_6.3TBps": 1e3 * ((2 * k + 2) + (3 * k + 2)) * rows * 8 / HBM_ACHIEVABLE,
               "model_host_upload_bytes": k * rows * 8,
               "timing": "host clock around one push, a device synchronisation before and after; median after warm-up; the three routes in the same run, the SR1 and the BFGS push alternating"}
        print(json.dumps(out), flush=True)
        results.append(out)
        del Vd, Ud, H, pool
        s.lowrank_clear()
    s.close(); s2.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "sr1_time.json"), "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
