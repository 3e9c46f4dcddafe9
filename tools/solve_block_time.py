"""Blocks of right-hand sides in the solves (mi355x_kkt_set_solve_block) against the two existing ways to solve nrhs right-hand sides in one call, on
bench workloads, one process per workload: nrhs = 8 and 24 through
  sequential   MI355X_KKT_DISABLE=solve_ctx: one solve behind the other (measured TWICE per round: the spread of the tool),
  default      the solve contexts where their one-off measurement picks them,
  blocked      the switch on,
alternating in one run on one handle (a round = sequential, default, blocked, sequential), medians over the rounds; the split of a blocked call into its
top part (chain sweeps, column by column) and the rest, from device events; then lowrank_update and a corrected
solve with nv = nu = 12 (tools/lowrank_time.py's columns), switch off and on.  Host clock around calls that end in a synchronisation of the solver's
stream.  Every blocked result is compared bitwise with the sequential one.  No gate, no target.
usage: python tools/solve_block_time.py workload [--out file.json]      (appends the workload's record to profiles/solve_block_time.json, or to --out)"""
import os, sys, time, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ctypes as C
import numpy as np, torch
import ipopt_amd, bench
from ipopt_amd import kkt

NV = NU = 12
ROUNDS = 7


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            os.environ.pop(k, None)
            if v:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def timed(call):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def stats(t):
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}


args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "solve_block_time.json")
if "--out" in sys.argv:
    args.remove(out_path)
wl = args[0] if args else "grid_1e5"
n, r, c, v, neg = bench.make_workload(wl)
rows = n - neg
s = ipopt_amd.KKTSolver(device=0)
s.initialize_structure(n, r, c, vals=v)
dv = torch.tensor(v, dtype=torch.float64, device="cuda")
st = s.factor_device(dv.data_ptr())
assert st[0] == 0 and st[1] == neg
rng = np.random.default_rng(3)
B = torch.tensor(rng.standard_normal((24, n)), dtype=torch.float64, device="cuda")
info = s.solve_block_info()
out = {"workload": wl, "kkt_dim": n, "num_levels": int(s.info().num_levels), "rounds": ROUNDS,
       "plan": {k: info[k] for k in ("width", "first_top_level", "blocked_launches", "bycol_launches", "top_launches_per_column")},
       "timing": "host clock around synchronous calls, median over alternating rounds after two warm-up rounds"}
one = torch.empty(n, dtype=torch.float64, device="cuda")
out["single_solve_ms"] = stats([timed(lambda: s.solve_device2(B[0].data_ptr(), one.data_ptr())) for _ in range(3 + 15)][3:])
for nrhs in (8, 24):
    X = {m: torch.empty((nrhs, n), dtype=torch.float64, device="cuda") for m in ("sequential", "default", "blocked", "sequential_again")}
    T = {m: [] for m in X}

    def run(mode):
        s.set_solve_block(mode == "blocked")
        with env(MI355X_KKT_DISABLE="solve_ctx" if mode.startswith("sequential") else None):
            return timed(lambda: s.solve_device2(B.data_ptr(), X[mode].data_ptr(), nrhs=nrhs))

    for rnd in range(2 + ROUNDS):
        for mode in X:
            t = run(mode)
            if rnd >= 2:
                T[mode].append(t)
    s.set_solve_block(False)
    res = {m: stats(T[m]) for m in T}
    seq = res["sequential"]["median"]
    res["spread_sequential_twice"] = abs(res["sequential_again"]["median"] - seq) / seq
    res["blocked_over_sequential"] = res["blocked"]["median"] / seq
    res["blocked_over_default"] = res["blocked"]["median"] / res["default"]["median"]
    res["blocked_over_better_existing"] = res["blocked"]["median"] / min(seq, res["default"]["median"])
    res["blocked_bitwise_equal_to_sequential"] = bool(torch.equal(X["blocked"], X["sequential"]))
    res["default_bitwise_equal_to_sequential"] = bool(torch.equal(X["default"], X["sequential"]))
    # the split of a blocked call (events around the top part of every block): one more blocked call, read back
    s.set_solve_block(True)
    s.solve_device2(B.data_ptr(), X["blocked"].data_ptr(), nrhs=nrhs)
    s.set_solve_block(False)
    tot, top = C.c_double(0.0), C.c_double(0.0)
    assert s.lib.mi355x_kkt_debug_solve_block_split(s._h, C.byref(tot), C.byref(top)) == 0
    res["blocked_device_ms"] = {"total": tot.value, "top_part": top.value, "bulk_and_rest": tot.value - top.value}
    # the top part is nrhs times what one column's is by construction: with a free bulk the call could not take less than its top part
    res["bound_blocked_over_sequential_at_free_bulk"] = top.value / seq
    out[f"nrhs{nrhs}"] = res
# the low-rank route: nv + nu inner solves per update
V = rng.standard_normal((rows, NV)) / np.sqrt(rows); U = rng.standard_normal((rows, NU)) / np.sqrt(rows)
halvings = 0
while True:
    s.lowrank_set(V, U)
    if s.lowrank_update() == (kkt.SUCCESS, 0):
        break
    U *= 0.5; halvings += 1
    assert halvings < 60
b = B[0].clone(); xo = torch.empty_like(b); xb = torch.empty_like(b)
T = {"update_off": [], "update_on": [], "corrected_off": [], "corrected_on": []}
for rnd in range(1 + 5):
    for on in (False, True):
        s.set_solve_block(on)
        tu = timed(lambda: s.lowrank_update())
        tc = timed(lambda: s.lowrank_solve_device2(b.data_ptr(), (xb if on else xo).data_ptr()))
        if rnd >= 1:
            T["update_on" if on else "update_off"].append(tu); T["corrected_on" if on else "corrected_off"].append(tc)
s.set_solve_block(False)
lr = {k: stats(t) for k, t in T.items()}
lr["update_on_over_off"] = lr["update_on"]["median"] / lr["update_off"]["median"]
lr["corrected_solution_bitwise_equal"] = bool(torch.equal(xo, xb))
lr["nv"] = NV; lr["nu"] = NU; lr["u_halvings"] = halvings
out["lowrank"] = lr
print(json.dumps(out), flush=True)
s.close()
results = []
if os.path.exists(out_path):
    with open(out_path) as f:
        results = [x for x in json.load(f) if x.get("workload") != wl]
results.append(out)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
