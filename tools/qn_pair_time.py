"""The quasi-Newton pair formed on the device (mi355x_kkt_qn_pair_*): time of form + push on bench workloads next to its yardstick measured in the same
run, the two sides ALTERNATING: the host route -- four scipy.sparse transposed products and the vector sums in float64 form (s, y)
(IpLimMemQuasiNewtonUpdater.cpp:282, :304-307), then lbfgs_push uploads them.  x block = n - neg; the Jacobian = the entries with row >= n - neg and
col < n - neg (one J_c block, ns = nd = 0); the triplets are reordered into two assembly segments, rest | J.  Per iterate: the current J is uploaded into
its segment (both routes need it there for the factorisation: not timed), then timed
    form (host vectors) + push         form + push with device vectors         store(None), the roll
and on a second handle the host route.  Host clock around calls, a device synchronisation before and after; median after warm-up.  Also recorded: the
bytes the kernel streams and their time at 6.3 TB/s, which instantiation (lanes per column) ran, and what the other two measured (form alone, device
vectors, no amax: MI355X_KKT_TUNE=qn_lpc).  No gate, no target.
--parent-tree DIR: before anything else, the paths that existed before against the parent commit -- DIR is a built checkout of it (its own library AND its
own Python binding: this tree's binding asks the library for symbols the parent does not have) --, fresh processes in the order A B A B (A = DIR's
tools, B = this tree's): tools/lbfgs_time.py and tools/lowrank_time.py; the A/A and B/B spreads of their medians are written next to the B - A differences.
usage: python tools/qn_pair_time.py [--parent-tree DIR] [workload ...]      (writes profiles/qn_pair_time.json)"""
import os, sys, time, json, subprocess
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM = 11, 2
HBM_ACHIEVABLE = 6.3e12      # bytes / s
args = sys.argv[1:]
parent_tree = None
if args and args[0] == "--parent-tree":
    parent_tree, args = os.path.abspath(args[1]), args[2:]
workloads = args or ["grid_1e5", "lukvle1_1e6"]


def existing_paths_vs_parent():
    """fresh processes A B A B of the two existing tools; their own output files are put back as they were"""
    keep = {}
    for f in ("lbfgs_time.json", "lowrank_time.json"):
        p = os.path.join(ROOT, "profiles", f)
        keep[p] = open(p, "rb").read() if os.path.exists(p) else None
    runs = {"lbfgs_time.py": {"A": [], "B": []}, "lowrank_time.py": {"A": [], "B": []}}
    try:
        for side in "ABAB":
            for tool in runs:
                env = dict(os.environ)
                env.pop("MI355X_KKT_LIBRARY", None); env.pop("PYTHONPATH", None)
                tree = parent_tree if side == "A" else ROOT
                t0 = time.perf_counter()
                out = subprocess.run([sys.executable, os.path.join(tree, "tools", tool)] + workloads, env=env, cwd=tree, capture_output=True, text=True, timeout=400)
                print(f"[{side}] {tool}: exit {out.returncode} after {time.perf_counter() - t0:.0f} s", file=sys.stderr, flush=True)
                if out.returncode != 0:                                               # (nothing more is started after a child that failed)
                    raise SystemExit(f"{tool} ({side}) failed:\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
                recs = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
                key = "lbfgs_push_ms" if tool == "lbfgs_time.py" else "lowrank_update_ms"
                runs[tool][side].append({(r["workload"] + (f":m{r['max_history']}" if "max_history" in r else "")): r[key]["median"] for r in recs})
    finally:
        for p, data in keep.items():
            if data is not None:
                open(p, "wb").write(data)
    report = {}
    for tool, ab in runs.items():
        for case in ab["A"][0]:
            a, b = [r[case] for r in ab["A"]], [r[case] for r in ab["B"]]
            spread = max(abs(a[0] - a[1]), abs(b[0] - b[1]))
            diff = sum(b) / 2 - sum(a) / 2
            report[f"{tool}:{case}"] = {"parent_median_ms": a, "this_median_ms": b, "same_code_spread_ms": spread, "this_minus_parent_ms": diff,
                                        "within_spread": bool(abs(diff) <= spread)}
    return {"order": "A B A B, fresh processes; A = a built checkout of the parent commit, B = this tree", "what": "lbfgs_push_ms / lowrank_update_ms medians of the tools", "cases": report}


ab_report = existing_paths_vs_parent() if parent_tree else None
if ab_report:
    print(json.dumps(ab_report), flush=True)

import numpy as np, torch, scipy.sparse as sp
import ipopt_amd, bench
from ipopt_amd import kkt


def timed(call):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def stats(t):
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}


def dev(v):
    return torch.tensor(np.ascontiguousarray(v), dtype=torch.float64, device="cuda")


results = []
for wl in workloads:
    n, r, c, v, neg = bench.make_workload(wl)
    nx, nc = n - neg, neg
    r = np.asarray(r, dtype=np.int32); c = np.asarray(c, dtype=np.int32); v = np.asarray(v, dtype=np.float64)
    isj = (r - 1 >= nx) & (c - 1 < nx)
    order = np.concatenate([np.flatnonzero(~isj), np.flatnonzero(isj)])
    r, c, v = r[order], c[order], v[order]
    nrest, nj = int((~isj).sum()), int(isj.sum())
    jr, jc = r[nrest:] - 1 - nx, c[nrest:] - 1
    J0 = v[nrest:].copy()
    rng = np.random.default_rng(3)
    K = 6
    steps = [0.1 * rng.standard_normal(nx) for _ in range(K + 1)]
    curv = [2.0 + rng.random(nx) for _ in range(K + 1)]
    Jpool = [J0 * (1.0 + 0.01 * rng.standard_normal(nj)) for _ in range(3)]
    yc = 0.01 * rng.standard_normal(nc)
    # the host route's matrices: one CSR structure, the data replaced per iterate (through the permutation scipy sorted the triplets with)
    coo = sp.coo_matrix((np.arange(1, nj + 1, dtype=np.float64), (jr, jc)), shape=(nc, nx)).tocsr()
    perm = coo.data.astype(np.int64) - 1 if coo.nnz == nj else None      # (duplicates would have been summed: then build per iterate)
    def jmat(vals):
        if perm is None:
            return sp.coo_matrix((vals, (jr, jc)), shape=(nc, nx)).tocsr()
        return sp.csr_matrix((vals[perm], coo.indices, coo.indptr), shape=(nc, nx))

    A = ipopt_amd.KKTSolver(device=0); B = ipopt_amd.KKTSolver(device=0)
    for s in (A, B):
        s.initialize_structure(n, r, c, vals=v)
        s.lbfgs_define(nx, K)
    A.assembly_define([nrest, nj])
    A.assembly_set(0, v[:nrest]); A.assembly_set(1, J0)
    A.qn_pair_define([nx, 0, nc, 0], r, c, 1, -1)
    info = A.qn_pair_info()
    x, gf = rng.standard_normal(nx), rng.standard_normal(nx)
    A.qn_pair_store(x, gf)
    Jl = jmat(J0)
    t = {"form_push_host": [], "form_push_device": [], "roll": [], "host_route": [], "host_route_products": []}
    dyc = dev(yc)
    out_dev, out_host = [], []
    max_dy = 0.0
    for k in range(2 * (WARM + REPS)):
        use_device_vectors = k % 2 == 1
        d = steps[k % (K + 1)]
        x1, gf1, J1 = x + d, gf + curv[k % (K + 1)] * d, Jpool[k % 3]
        A.assembly_set(1, J1)
        Jc = jmat(J1)
        dx, dgf = dev(x1), dev(gf1)

        def device_route():
            if use_device_vectors:
                A.qn_pair_form_device(dx.data_ptr(), dgf.data_ptr(), dyc.data_ptr(), None)
            else:
                A.qn_pair_form(x1, gf1, yc, None)
            out_dev.append(A.qn_pair_push())

        def host_route():
            t0 = time.perf_counter()
            sv = x1 - x
            yv = (gf1 - gf) + Jc.T @ yc + np.zeros(nx) - Jl.T @ yc - np.zeros(nx)      # (J_d is absent on these workloads: two of the four products are empty)
            tp = 1e3 * (time.perf_counter() - t0)
            out_host.append(B.lbfgs_push(sv, yv))
            return tp, yv

        got = []
        if k % 4 < 2:                                                                  # the two sides alternate, and so does which of them goes first
            ms_d = timed(device_route); ms_h = timed(lambda: got.append(host_route()))
        else:
            ms_h = timed(lambda: got.append(host_route())); ms_d = timed(device_route)
        yd_ = A.qn_pair_get("y")
        max_dy = max(max_dy, float(np.abs(yd_ - got[0][1]).max() / np.abs(got[0][1]).max()))
        ms_r = timed(lambda: A.qn_pair_store())
        if k >= 2 * WARM:
            t["form_push_device" if use_device_vectors else "form_push_host"].append(ms_d)
            t["host_route"].append(ms_h); t["host_route_products"].append(got[0][0]); t["roll"].append(ms_r)
        x, gf, Jl = x1, gf1, Jc
    assert out_dev == out_host, (out_dev, out_host)
    # the other instantiations: form alone, device vectors, nothing downloaded
    lpc_ms = {}
    dx, dgf = dev(x), dev(gf)
    for lpc in (1, 8, 64):
        os.environ["MI355X_KKT_TUNE"] = f"qn_lpc={lpc}"
        A.qn_pair_define([nx, 0, nc, 0], r, c, 1, -1)
        assert A.qn_pair_info()["lpc"] == lpc
        A.qn_pair_store(x, gf)
        ts = [timed(lambda: A.qn_pair_form_device(dx.data_ptr(), dgf.data_ptr(), dyc.data_ptr(), None, amax=False)) for _ in range(WARM + REPS)][WARM:]
        lpc_ms[str(lpc)] = stats(ts)
    os.environ.pop("MI355X_KKT_TUNE")
    bytes_kernel = 32 * nj + 52 * nx
    dev_h, dev_d, host = stats(t["form_push_host"]), stats(t["form_push_device"]), stats(t["host_route"])
    out = {"workload": wl, "kkt_dim": n, "nx": nx, "nc": nc, "nnz_j": nj, "mean_column": nj / max(nx, 1), "max_column": info["max_column"], "lpc": info["lpc"],
           "max_history": K, "reps": REPS, "warm": WARM, "outcomes": sorted(set(out_dev)),
           "form_push_host_vectors_ms": dev_h, "form_push_device_vectors_ms": dev_d, "roll_store_ms": stats(t["roll"]),
           "host_route_ms": host, "host_route_products_and_sums_ms": stats(t["host_route_products"]),
           "host_over_device_host_vectors": host["median"] / dev_h["median"], "host_over_device_device_vectors": host["median"] / dev_d["median"],
           "y_max_relative_difference_to_host_route": max_dy,
           "kernel_bytes": bytes_kernel, "kernel_stream_ms_at_6.3TBps": 1e3 * bytes_kernel / HBM_ACHIEVABLE,
           "form_alone_device_vectors_ms_by_lpc": lpc_ms,
           "timing": "host clock around the calls, a device synchronisation before and after; median after warm-up; device and host route alternate in one run"}
    print(json.dumps(out), flush=True)
    results.append(out)
    A.close(); B.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "qn_pair_time.json"), "w") as f:
    json.dump({"workloads": results, "existing_paths_vs_parent": ab_report}, f, indent=1)
    f.write("\n")
