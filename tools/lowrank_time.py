"""Low-rank-updated solves (mi355x_kkt_lowrank_*, K + V V^T - U U^T with nv = nu = 12 on the x block): time of lowrank_update, of a plain solve and of a
corrected solve on bench workloads -- host clock around calls that end in a synchronisation of the solver's stream, median of repeated calls after
warm-up -- next to their yardsticks: 24 plain solves for the update; for the extra time of a corrected solve the bytes its six kernels stream,
(2 rows + 2 n) * 12 * 8 per right-hand side, over the achievable HBM rate (6.3 TB/s), plus six dependent launch boundaries.  No gate, no target.
usage: python tools/lowrank_time.py [workload ...]      (writes profiles/lowrank_time.json)"""
import os, sys, time, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import ipopt_amd, bench
from ipopt_amd import kkt
from tests.support import kktgen

NV = NU = 12
HBM_ACHIEVABLE = 6.3e12      # bytes / s


def median_ms(call, reps, warm=3):
    for _ in range(warm):
        call()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        call()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), float(min(t)), float(max(t))


results = []
for wl in (sys.argv[1:] or ["grid_1e5", "lukvle1_1e6"]):
    n, r, c, v, neg = bench.make_workload(wl)
    rows = n - neg                                             # the x block (the generators return neg = number of constraints)
    s = ipopt_amd.KKTSolver(device=0)
    s.initialize_structure(n, r, c, vals=v)
    dv = torch.tensor(v, dtype=torch.float64, device="cuda")
    st = s.factor_device(dv.data_ptr())
    assert st[0] == 0 and st[1] == neg
    rng = np.random.default_rng(3)
    V = rng.standard_normal((rows, NV)) / np.sqrt(rows); U = rng.standard_normal((rows, NU)) / np.sqrt(rows)
    # M1 = I + V^T (K^-1)_xx V is positive definite for any V; U is halved until M2 = I - U^T ((K + V V^T)^-1)_xx U is as well
    halvings = 0
    while True:
        s.lowrank_set(V, U)
        if s.lowrank_update() == (kkt.SUCCESS, 0):
            break
        U *= 0.5; halvings += 1
        assert halvings < 60
    b = torch.tensor(rng.standard_normal(n), dtype=torch.float64, device="cuda"); x = torch.empty_like(b)
    torch.cuda.synchronize()
    upd = median_ms(lambda: s.lowrank_update(), 5, warm=1)
    plain = median_ms(lambda: s.solve_device2(b.data_ptr(), x.data_ptr()), 30)
    corr = median_ms(lambda: s.lowrank_solve_device2(b.data_ptr(), x.data_ptr()), 30)
    # what was computed: the corrected solution against K~ applied through the sparse K (no dense matrix at this size)
    K = kktgen.to_scipy(n, r, c, v)
    xh, bh = x.cpu().numpy(), b.cpu().numpy()
    kx = K @ xh; kx[:rows] += V @ (V.T @ xh[:rows]) - U @ (U.T @ xh[:rows])
    rowsum = np.asarray(abs(K).sum(axis=1)).ravel(); rowsum[:rows] += np.abs(V) @ np.abs(V).sum(axis=0) + np.abs(U) @ np.abs(U).sum(axis=0)
    sres = float(np.abs(kx - bh).max() / (rowsum.max() * np.abs(xh).max() + np.abs(bh).max()))
    stream_bytes = (2 * rows + 2 * n) * 12 * 8
    out = {"workload": wl, "kkt_dim": n, "rows": rows, "nv": NV, "nu": NU, "u_halvings": halvings, "reps": {"update": 5, "solves": 30},
           "lowrank_update_ms": {"median": upd[0], "min": upd[1], "max": upd[2]},
           "plain_solve_ms": {"median": plain[0], "min": plain[1], "max": plain[2]},
           "corrected_solve_ms": {"median": corr[0], "min": corr[1], "max": corr[2]},
           "corrected_minus_plain_ms": corr[0] - plain[0],
           "corrected_solve_scaled_residual": sres,
           "yardstick_update_24_plain_solves_ms": 24 * plain[0],
           "yardstick_correction_stream_bytes": stream_bytes,
           "yardstick_correction_stream_ms_at_6.3TBps": 1e3 * stream_bytes / HBM_ACHIEVABLE,
           "yardstick_correction_launch_boundaries": 6,
           "timing": "host clock around synchronous calls (each ends in a synchronisation of the solver's stream), median after warm-up"}
    print(json.dumps(out), flush=True)
    results.append(out)
    s.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "lowrank_time.json"), "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
