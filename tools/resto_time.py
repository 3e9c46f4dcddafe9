"""Restoration-phase limited-memory pushes (mi355x_kkt_lbfgs_define_resto + lbfgs_push_resto): time of a push with a FULL history of max_history 6
and 12 on bench workloads, both update types, B0 = sigma I and B0 = eta DR, next to two yardsticks measured in the same run on the same machine:
  plain push   lbfgs_push of the same (s, ypart) on a plain history of the same type and shape on a second handle, ALTERNATING with the resto push:
               the resto push reads one more vector (DR) per kernel, (2 m + 3) / (2 m + 2) of the bytes, and reduces 3 m + 6 dots instead of 2 m + 3
  host route   the numpy transcription of the reference's flow (tests/support/resto_spec.py Literal, float64) takes the same pair, recomputes Y, D, L
               and the Gram matrices over the whole history, forms V and U, and lowrank_set uploads the columns
Host clock around calls that end in a device synchronisation, median of repeated calls after warm-up; the pairs cycle through a pool of
max_history + 2, eta through 0.3, 0.3, 0.1, 0.03.  No gate, no target.
usage: python tools/resto_time.py [workload ...]      (writes profiles/resto_time.json)"""
import os, sys, time, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import ipopt_amd, bench
from ipopt_amd import kkt
from tests.support import resto_spec as rs

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
    s2 = ipopt_amd.KKTSolver(device=0)                         # the plain history lives on a handle of its own, so that the two pushes can alternate
    s2.initialize_structure(n, r, c, vals=v)
    for k in (6, 12):
        for type_, special in ((rs.BFGS, False), (rs.BFGS, True), (rs.SR1, False), (rs.SR1, True)):
            Sp, Yp, DR = rs.make_resto(rows, k + 2, seed=3, sr1=type_ == rs.SR1)
            P = k + 2
            pool = [(np.ascontiguousarray(Sp[:, j]), np.ascontiguousarray(Yp[:, j])) for j in range(P)]
            del Sp, Yp
            eta = lambda j: rs.ETAS[j % 4]
            s.lbfgs_define_resto(rows, DR, max_history=k, type=type_, special=special)
            (s2.lbfgs_define_sr1 if type_ == rs.SR1 else s2.lbfgs_define)(rows, k)
            oc_resto = [s.lbfgs_push_resto(*pool[j % P], eta(j)) for j in range(k)]
            oc_plain = [s2.lbfgs_push(*pool[j % P]) for j in range(k)]
            t_resto, t_plain = [], []
            for j in range(k, k + WARM + REPS):
                oc = []
                a = timed(lambda: oc.append(s.lbfgs_push_resto(*pool[j % P], eta(j))))
                b = timed(lambda: oc.append(s2.lbfgs_push(*pool[j % P])))
                oc_resto.append(oc[0]); oc_plain.append(oc[1])
                if j >= k + WARM:
                    t_resto.append(a); t_plain.append(b)
            Vd, Ud = s.lbfgs_get("V"), s.lbfgs_get("U")
            s.lbfgs_clear(); s.lowrank_clear(); s2.lbfgs_clear(); s2.lowrank_clear()
            # host route: the same pushes through the literal flow
            H = rs.Literal(rows, k, DR, type=type_, special=special)
            oc_host = [H.push(*pool[j % P], eta(j)) for j in range(k)]
            t_host, t_host_algebra = [], []

            def host_push(j):
                t0 = time.perf_counter()
                oc_host.append(H.push(*pool[j % P], eta(j)))
                t_alg = 1e3 * (time.perf_counter() - t0)
                s.lowrank_set(H.V, H.U)
                return t_alg
            for j in range(k, k + WARM + REPS):
                alg = []
                ms = timed(lambda: alg.append(host_push(j)))
                if j >= k + WARM:
                    t_host.append(ms); t_host_algebra.append(alg[0])
            op = lambda V, U: V[:256] @ V[:256].T - U[:256] @ U[:256].T                                      # (the leading 256 x 256 block of V V^T - U U^T)
            Bd, Bh = op(Vd, Ud), op(H.V, H.U)
            diff = float(np.abs(Bd - Bh).max() / np.abs(Bh).max())
            resto_ms, plain_ms, host_ms = stats(t_resto), stats(t_plain), stats(t_host)
            nform = (4 * k + 2) if type_ == rs.BFGS else (3 * k + 2)                                         # columns read and written by the plain form kernel
            out = {"workload": wl, "kkt_dim": n, "rows": rows, "max_history": k, "memory": k, "type": "sr1" if type_ == rs.SR1 else "bfgs", "special": bool(special),
                   "reps": REPS, "warm": WARM, "resto_push_ms": resto_ms, "plain_push_ms": plain_ms,
                   "host_route_ms": host_ms, "host_route_numpy_algebra_ms": stats(t_host_algebra),
                   "resto_over_plain": resto_ms["median"] / plain_ms["median"], "host_over_resto": host_ms["median"] / resto_ms["median"],
                   "resto_outcomes_not_stored": int(sum(o != kkt.LBFGS_STORED for o in oc_resto)), "plain_outcomes_not_stored": int(sum(o != kkt.LBFGS_STORED for o in oc_plain)),
                   "host_outcomes_not_stored": int(sum(o != rs.STORED for o in oc_host)),
                   "operator_max_relative_difference": diff,
                   "model_resto_bytes": ((2 * k + 3) + nform + 1) * rows * 8, "model_plain_bytes": ((2 * k + 2) + nform) * rows * 8,
                   "model_resto_stream_ms_at_6.3TBps": 1e3 * ((2 * k + 3) + nform + 1) * rows * 8 / HBM_ACHIEVABLE,
                   "timing": "host clock around one push, a device synchronisation before and after; median after warm-up; the three routes in the same run, the resto and the plain push alternating"}
            print(json.dumps(out), flush=True)
            results.append(out)
            del Vd, Ud, H, pool
            s.lowrank_clear()
    s.close(); s2.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "resto_time.json"), "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
