"""-m 'not gpu': the limited-memory SR1 entry points of the C ABI (mi355x_kkt_lbfgs_define_sr1, _lbfgs_undo, _lbfgs_sr1_info,
_lbfgs_sr1_coefficients) are exported and listed, check every argument BEFORE the device is touched (naming the offending argument), refuse an
unanalysed and a multi-GPU handle, and -- with valid arguments and no device -- fail loudly.  mi355x_kkt_lbfgs_sr1_coefficients needs neither a handle
nor a device: its split is held to the longdouble specification (tests/support/sr1_spec.py) by the project's rule e_lib <= 64 max(e_64, 2^-52), e the
largest deviation relative to the largest entry and e_64 the float64 specification's own, on Z^-1 = Qs+ Qs+^T - Qs- Qs-^T and on the two halves
separately (never column by column: sign and rotation of eigenvectors are not determined); it answers SINGULAR where the split rule says skip.
The host header itself runs under AddressSanitizer and UBSan in two stand-alone programs: the eigen-split (tests/support/sr1_host_check.cpp) and the
state machine of a history, BFGS and SR1: push, skip, eviction, the spare slot and undo (tests/support/lbfgs_state_check.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ipopt_amd
from ipopt_amd import kkt
from tests.support import lbfgs_spec as lb
from tests.support import sr1_spec as sr

SR1 = ["mi355x_kkt_lbfgs_define_sr1", "mi355x_kkt_lbfgs_undo", "mi355x_kkt_lbfgs_sr1_info", "mi355x_kkt_lbfgs_sr1_coefficients"]
N = 6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def analysed(**opts):
    s = ipopt_amd.KKTSolver(**opts)
    s.initialize_structure(N, np.arange(1, N + 1), np.arange(1, N + 1), vals=np.ones(N))
    return s


def test_sr1_symbols_are_exported_and_listed():
    lib = C.CDLL(ipopt_amd.library_path())
    for name in SR1:
        assert hasattr(lib, name), name
        assert name in kkt.ABI_SYMBOLS
    assert (kkt.LBFGS_BFGS, kkt.LBFGS_SR1) == (0, 1)
    for name in ("lbfgs_define_sr1", "lbfgs_undo", "lbfgs_sr1_info"):
        assert callable(getattr(ipopt_amd.KKTSolver, name))
    assert callable(kkt.lbfgs_sr1_coefficients)


def test_every_argument_is_checked_before_the_device_and_named():
    s = analysed()
    lib, h = s.lib, s._h
    E = np.zeros(32)

    def refused(call, word, *args):
        assert call(h, *args) == kkt.FATAL
        assert word in s.last_error(), (word, s.last_error())

    d = lib.mi355x_kkt_lbfgs_define_sr1
    refused(d, "rows", 0, 6, 0, 1.0)
    refused(d, "rows", N + 1, 6, 0, 1.0)
    refused(d, "max_history", N, 0, 0, 1.0)
    refused(d, "max_history", N, 33, 0, 1.0)
    refused(d, "init ", N, 6, -1, 1.0)
    refused(d, "init ", N, 6, 5, 1.0)
    refused(d, "init_val", N, 6, 4, 0.0)
    refused(d, "init_val", N, 6, 4, float("nan"))
    refused(d, "init_val", N, 6, 4, float("inf"))
    assert "lbfgs_define_sr1" in s.last_error()
    refused(lib.mi355x_kkt_lbfgs_sr1_info, "capacity", None, None, None, E.ctypes.data, -1)
    assert "lbfgs_sr1_info" in s.last_error()


def test_a_handle_that_is_not_analysed_is_refused():
    s = ipopt_amd.KKTSolver()
    lib, h = s.lib, s._h
    for st in (lib.mi355x_kkt_lbfgs_define_sr1(h, N, 6, 0, 1.0), lib.mi355x_kkt_lbfgs_undo(h, None),
               lib.mi355x_kkt_lbfgs_sr1_info(h, None, None, None, None, 0)):
        assert st == kkt.FATAL and "not analysed" in s.last_error()


def test_a_multi_gpu_handle_is_refused():
    s = analysed(nranks=2, rank=0)
    for call in (lambda: s.lbfgs_define_sr1(N, 6), s.lbfgs_undo, s.lbfgs_sr1_info):
        with pytest.raises(ipopt_amd.KKTError, match="not supported on a multi-GPU handle"):
            call()


@pytest.mark.skipif(_has_gpu(), reason="only meaningful on a machine without a GPU")
def test_valid_arguments_without_a_device_fail_loudly():
    s = analysed()
    lib, h = s.lib, s._h
    u = C.c_int(7)
    for st in (lib.mi355x_kkt_lbfgs_define_sr1(h, N, 6, 0, 1.0), lib.mi355x_kkt_lbfgs_undo(h, C.byref(u)),
               lib.mi355x_kkt_lbfgs_sr1_info(h, None, None, None, None, 0)):
        assert st == kkt.FATAL and "no usable HIP device" in s.last_error()
    assert u.value == 0
    with pytest.raises(ipopt_amd.KKTError, match="no usable HIP device"):
        s.lbfgs_define_sr1(N, 6)


def halves(Qs, nneg):
    P, M = Qs[:, nneg:] @ Qs[:, nneg:].T, Qs[:, :nneg] @ Qs[:, :nneg].T
    return {"Z^-1": P - M, "Qs+ Qs+^T": P, "Qs- Qs-^T": M}


@pytest.mark.parametrize("m", [1, 2, 6, 32])
def test_the_split_is_held_to_the_longdouble_specification(m):
    rows = 300
    S, Y = sr.make_pairs(rows, m, seed=40 + m)
    H64, Hld = sr.History(rows, m), sr.History(rows, m, dtype=np.longdouble)
    for j in range(m):
        assert H64.push(S[:, j], Y[:, j]) == sr.STORED and Hld.push(S[:, j], Y[:, j]) == sr.STORED
    st, E, Qs, nneg = kkt.lbfgs_sr1_coefficients(H64.STS, H64.L, H64.D, H64.sigma)
    assert st == kkt.SUCCESS and nneg == H64.nneg == Hld.nneg
    assert np.all(np.diff(E) >= 0) and int(np.sum(E < 0)) == nneg
    got, h64, hld = halves(Qs, nneg), halves(H64.Qs, nneg), halves(Hld.Qs, nneg)
    for name in got:
        big = np.abs(hld[name]).max()
        if not big > 0:                                                              # (an empty half: nneg = 0 or m)
            assert not got[name].any()
            continue
        e_lib, e_64 = float(np.abs(got[name] - hld[name]).max() / big), float(np.abs(h64[name] - hld[name]).max() / big)
        print(f"m = {m}: {name}: e_lib {e_lib:.2e} e_64 {e_64:.2e} ratio {e_lib / max(e_64, 2.0 ** -52):.2f}")
        assert e_lib <= 64.0 * max(e_64, 2.0 ** -52), (name, e_lib, e_64)


@pytest.mark.parametrize("rows", [180, 517])
def test_a_repeated_newest_pair_answers_singular(rows):
    """pairs 0, 1, 2, 2 with the constant sigma 1.0: two equal rows of Z, emin / emax is 6.8e-17 (rows 180) / 1.2e-17 (517) in exact arithmetic"""
    Sp, Yp = sr.make_pairs(rows, 4, seed=5)
    S, Y = Sp[:, [0, 1, 2, 2]], Yp[:, [0, 1, 2, 2]]
    D, L, sts = lb.recomputed(S, Y)
    assert sr.coefficients(sts, L, D, 1.0)[1] is None                                # the float64 specification skips as well
    st, E, _, nneg = kkt.lbfgs_sr1_coefficients(sts, L, D, 1.0)
    nn, emin, emax = sr.split(E)
    print(f"rows {rows}: E {E}, emin / emax {emin / emax:.2e}")
    assert st == kkt.SINGULAR and nneg == nn and emin / emax < 1e-12
    st, _, _, _ = kkt.lbfgs_sr1_coefficients(sts[:3, :3], L[:3, :3], D[:3], 1.0)     # without the repeat it is fine
    assert st == kkt.SUCCESS


def test_the_zero_matrix_is_singular_and_m_33_is_fatal():
    st, E, _, nneg = kkt.lbfgs_sr1_coefficients(np.zeros((3, 3)), np.zeros((3, 3)), np.zeros(3), 1.0)
    assert st == kkt.SINGULAR and nneg == 0 and not E.any()
    assert kkt.lbfgs_sr1_coefficients(np.zeros((0, 0)), np.zeros((0, 0)), np.zeros(0), 1.0)[0] == kkt.SUCCESS
    with pytest.raises(ipopt_amd.KKTError, match="m must be in"):
        kkt.lbfgs_sr1_coefficients(np.eye(33), np.zeros((33, 33)), np.ones(33), 1.0)
    assert C.CDLL(ipopt_amd.library_path()).mi355x_kkt_lbfgs_sr1_coefficients(33, None, None, None, C.c_double(1.0), None, None, None) == kkt.FATAL


def _run_host_program_under_sanitizers(tmp_path, name, sources=()):
    """tests/support/<name>.cpp, a stand-alone program with its own main, on the CPU: nothing is loaded into python under a sanitizer.  sources: host-only
    files of ipopt_amd/csrc it is linked with, compiled with the same flags (side by side: the analysis alone takes most of a minute)"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread"]
    probe = tmp_path / "probe.cpp"; probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    csrc = os.path.join(ROOT, "ipopt_amd", "csrc")
    units = [os.path.join(ROOT, "tests", "support", name + ".cpp")] + [os.path.join(csrc, f) for f in sources]
    objs = [str(tmp_path / (os.path.basename(u) + ".o")) for u in units]
    jobs = [subprocess.Popen([cxx, *flags, "-I", csrc, "-c", u, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for u, o in zip(units, objs)]
    for j in jobs:
        out, _ = j.communicate()
        assert j.returncode == 0, out
    exe = tmp_path / name
    build = subprocess.run([cxx, *flags, *objs, "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok")


def test_the_host_header_is_clean_under_address_and_ub_sanitizers(tmp_path):
    _run_host_program_under_sanitizers(tmp_path, "sr1_host_check")


def test_the_history_state_machine_on_the_cpu_under_sanitizers(tmp_path):
    """push, skip, eviction, the SR1 spare slot and undo of lbfgs_host.h against a model kept by the rule alone, D, L, S^T S bitwise against a recomputation"""
    _run_host_program_under_sanitizers(tmp_path, "lbfgs_state_check")
