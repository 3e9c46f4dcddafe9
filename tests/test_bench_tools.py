"""bench.py's own machinery, on the CPU: the self-launch of `--gpus N`, and the machine-code hash that keys the cached rocprof / PMC figures."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_bench_gpus_2_launches_itself_and_the_ranks_agree_on_their_collectives():
    """`python bench.py --gpus 2` as typed, no launcher around it (VERDICT r04 "missing" 1: it used to call init_process_group without a rendezvous):
    bench.py re-executes itself under torch.distributed.run with one rank per GPU.  On this CPU-only box the ranks go as far as a box without
    a GPU can -- rendezvous, per-rank analysis with (nranks, rank), the collective plans of both ranks played against each other -- and stop
    before the first HIP call (MI355X_KKT_BENCH_DRYRUN)."""
    env = dict(os.environ, MI355X_KKT_BENCH_DRYRUN="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "lukvle1_1e4", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]                     # ONE JSON line, from rank 0
    j = json.loads(lines[0])
    assert j["dry_run"] and j["n_gpus"] == 2 and j["ranks_seen"] == 2 and j["plan_ok"] and j["collectives_per_factor_plus_solve"] >= 3


def test_without_the_dry_run_a_box_without_a_gpu_fails_loudly_not_silently():
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "MI355X_KKT_BENCH_DRYRUN"):
        env.pop(k, None)
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the real --gpus 2 run is the driver's")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "lukvle1_1e4", "--steps", "1", "--warmup", "1"],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert p.returncode != 0 and not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]      # no line, no CPU fallback


KERNEL = r"""
#include <hip/hip_runtime.h>
__global__ void k_probe_axpy(double* y, const double* x, double a, int n) { int i = blockIdx.x * blockDim.x + threadIdx.x; if (i < n) y[i] = %s; }
__global__ void k_other(int* p) { p[threadIdx.x] = 1; }
void launch(double* y, const double* x, int n) { hipLaunchKernelGGL(k_probe_axpy, dim3(1), dim3(64), 0, 0, y, x, 2.0, n); }
"""


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_kernel_code_hash_survives_a_rebuild_and_sees_a_changed_kernel(tmp_path):
    """The hash is over the FUNC bytes of the kernel only: two builds of the same source whose code objects differ in their build-specific
    `__hip_cuid_*` symbol (random compilation-unit ids here; different paths in a rebuild on another box) hash the same -- the cached rocprof / PMC
    figures stay on the bench line after build() -- and a different kernel body does not."""
    sys.path.insert(0, ROOT)
    import bench

    def build(tag, body):
        src, lib = tmp_path / f"probe_{tag}.hip", tmp_path / f"libprobe_{tag}.so"
        src.write_text(KERNEL % body)
        subprocess.run([HIPCC, "-O3", "-fPIC", "-shared", "-fuse-cuid=random", "--offload-arch=gfx950", str(src), "-o", str(lib)], check=True, capture_output=True, timeout=300)
        return str(lib)

    a, b, c = build("a", "a * x[i] + y[i]"), build("b", "a * x[i] + y[i]"), build("c", "a * x[i] - y[i]")
    ha, hb, hc = (bench.kernel_code_hash("k_probe_axpy", lib=x) for x in (a, b, c))
    assert ha is not None and ha == hb and ha != hc
    syms = [subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-s", "-W", x], capture_output=True, text=True).stdout for x in (a, b)]
    cuid = [[w for w in s.split() if w.startswith("__hip_cuid_")] for s in syms]
    assert cuid[0] and cuid[1] and cuid[0] != cuid[1]            # the two builds really differ where round 4's hash looked
    assert bench.kernel_code_hash("k_no_such_kernel", lib=a) is None


def test_host_only_model_tools_run_without_a_device():
    """tools/level_model.py (per-level work model) and tools/mem_plan.py (what a recycling plan of the contribution blocks would need) are host tools: they run
    on a box without a GPU, and their totals are consistent with the analysis (every block resident = Info.cb_doubles)."""
    import re
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mem_plan.py"), "grid_1e5", "0", "8"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = p.stdout
    tot = float(re.search(r"every block resident: ([0-9.]+) GiB", out).group(1))
    pools = [float(x) for x in re.findall(r"-> pool\s+([0-9.]+) GiB", out)]
    assert len(pools) == 2 and 0.0 < pools[0] <= pools[1] <= tot + 0.01
    sys.path.insert(0, ROOT)
    import bench, ipopt_amd
    n, r, c, v, _ = bench.make_workload("grid_1e5")
    s = ipopt_amd.KKTSolver(device=-1)
    s.initialize_structure(n, r, c, vals=v)
    assert abs(8.0 * s.info().cb_doubles / 2 ** 30 - tot) <= 0.01
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "level_model.py"), "grid_1e5"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0 and "big fronts=" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


def test_dump_outputs_writes_float64_and_samples_a_large_array_the_same_way_every_time(tmp_path):
    """bench.py --dump-outputs: every output as DIR/<name>.npy in float64; an array over the size limit becomes a fixed, seeded sample of its
    elements with their indices beside it, so that two runs (two builds) can be compared output for output."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    x = np.linspace(0.0, 1.0, 1000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x": x, "inertia": (0, 7, 0)}, limit=1024)
    for d in ("a", "b"):
        assert sorted(os.listdir(tmp_path / d)) == ["inertia.npy", "x.npy", "x_index.npy"]
    xa, ia = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "a" / "x_index.npy")
    assert xa.dtype == np.float64 and xa.size == 1024 // 16 and xa.nbytes + ia.nbytes <= 1024
    assert np.array_equal(xa, x[ia.astype(np.int64)]) and np.all(np.diff(ia) > 0)
    assert np.array_equal(xa, np.load(tmp_path / "b" / "x.npy")) and np.array_equal(ia, np.load(tmp_path / "b" / "x_index.npy"))
    assert np.load(tmp_path / "a" / "inertia.npy").tolist() == [0.0, 7.0, 0.0]
    bench.dump_outputs(str(tmp_path / "c"), {"x": x})
    assert os.listdir(tmp_path / "c") == ["x.npy"] and np.array_equal(np.load(tmp_path / "c" / "x.npy"), x)
