"""-m 'not gpu': the limited-memory BFGS entry points of the C ABI (mi355x_kkt_lbfgs_*) are exported and listed, check every argument BEFORE the
device is touched (naming the offending argument), refuse an unanalysed and a multi-GPU handle, and -- with valid arguments and no device -- fail
loudly: there is no host stand-in for the history.  mi355x_kkt_lbfgs_coefficients is the one entry point that needs neither a handle nor a device: it
is held to the float64 specification (tests/support/lbfgs_spec.py) to 1e-13 relative -- two orderings of the same sums over at most 32 terms on a
system with cond(M) <= 5 -- and answers SINGULAR on the exact recipe of a vanishing Cholesky pivot."""
import ctypes as C

import numpy as np
import pytest

import ipopt_amd
from ipopt_amd import kkt
from tests.support import lbfgs_spec as lb

LBFGS = ["mi355x_kkt_lbfgs_define", "mi355x_kkt_lbfgs_push", "mi355x_kkt_lbfgs_push_device", "mi355x_kkt_lbfgs_reset", "mi355x_kkt_lbfgs_clear",
         "mi355x_kkt_lbfgs_info", "mi355x_kkt_lbfgs_get", "mi355x_kkt_lbfgs_coefficients"]
N = 6


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


def test_lbfgs_symbols_are_exported_and_listed():
    lib = C.CDLL(ipopt_amd.library_path())
    for name in LBFGS:
        assert hasattr(lib, name), name
        assert name in kkt.ABI_SYMBOLS
    assert kkt.LBFGS_MAX == kkt.LOWRANK_MAX == 32
    for name in ("lbfgs_define", "lbfgs_push", "lbfgs_push_device", "lbfgs_reset", "lbfgs_clear", "lbfgs_info", "lbfgs_get"):
        assert callable(getattr(ipopt_amd.KKTSolver, name))


def test_every_argument_is_checked_before_the_device_and_named():
    s = analysed()
    lib, h = s.lib, s._h
    v = np.ones(N); p = v.ctypes.data
    oc = C.c_int(7)

    def refused(call, word, *args):
        assert call(h, *args) == kkt.FATAL
        assert word in s.last_error(), (word, s.last_error())

    d = lib.mi355x_kkt_lbfgs_define
    refused(d, "rows", 0, 6, 0, 1.0, 1e-8, 1e8)
    refused(d, "rows", N + 1, 6, 0, 1.0, 1e-8, 1e8)
    refused(d, "max_history", N, 0, 0, 1.0, 1e-8, 1e8)
    refused(d, "max_history", N, 33, 0, 1.0, 1e-8, 1e8)
    refused(d, "init ", N, 6, -1, 1.0, 1e-8, 1e8)
    refused(d, "init ", N, 6, 5, 1.0, 1e-8, 1e8)
    refused(d, "init_val", N, 6, 4, 0.0, 1e-8, 1e8)
    refused(d, "init_val", N, 6, 4, float("nan"), 1e-8, 1e8)
    refused(d, "sigma_min", N, 6, 0, 1.0, 0.0, 1e8)
    refused(d, "sigma_max", N, 6, 0, 1.0, 1e-3, 1e-4)
    refused(d, "sigma_max", N, 6, 0, 1.0, 1e-3, float("inf"))
    assert "lbfgs_define" in s.last_error()
    refused(lib.mi355x_kkt_lbfgs_push, "s is null", None, p, C.byref(oc))
    refused(lib.mi355x_kkt_lbfgs_push, "y is null", p, None, C.byref(oc))
    assert oc.value == 1 and "lbfgs_push" in s.last_error()                          # a refused push stored nothing
    refused(lib.mi355x_kkt_lbfgs_push_device, "d_s", None, C.c_void_p(8), None)
    refused(lib.mi355x_kkt_lbfgs_push_device, "d_y", C.c_void_p(8), None, None)
    assert "lbfgs_push_device" in s.last_error()
    refused(lib.mi355x_kkt_lbfgs_get, "what", -1, p, N)
    refused(lib.mi355x_kkt_lbfgs_get, "what", 7, p, N)
    refused(lib.mi355x_kkt_lbfgs_get, "capacity", 0, p, -1)
    refused(lib.mi355x_kkt_lbfgs_get, "out", 0, None, N)
    assert "lbfgs_get" in s.last_error()


def test_a_handle_that_is_not_analysed_is_refused():
    s = ipopt_amd.KKTSolver()
    v = np.ones(N); p = v.ctypes.data
    lib, h = s.lib, s._h
    for st in (lib.mi355x_kkt_lbfgs_define(h, N, 6, 0, 1.0, 1e-8, 1e8), lib.mi355x_kkt_lbfgs_push(h, p, p, None),
               lib.mi355x_kkt_lbfgs_push_device(h, C.c_void_p(8), C.c_void_p(8), None), lib.mi355x_kkt_lbfgs_reset(h), lib.mi355x_kkt_lbfgs_clear(h),
               lib.mi355x_kkt_lbfgs_info(h, None, None, None, None, None, None), lib.mi355x_kkt_lbfgs_get(h, 0, p, N)):
        assert st == kkt.FATAL and "not analysed" in s.last_error()


def test_a_multi_gpu_handle_is_refused():
    s = analysed(nranks=2, rank=0)
    v = np.ones(N)
    for call in (lambda: s.lbfgs_define(N, 6), lambda: s.lbfgs_push(v, v), lambda: s.lbfgs_push_device(8, 8), s.lbfgs_reset, s.lbfgs_clear, s.lbfgs_info,
                 lambda: s.lbfgs_get("S")):
        with pytest.raises(ipopt_amd.KKTError, match="not supported on a multi-GPU handle"):
            call()


@pytest.mark.skipif(_has_gpu(), reason="only meaningful on a machine without a GPU")
def test_valid_arguments_without_a_device_fail_loudly():
    s = analysed()
    v = np.ones(N); p = v.ctypes.data
    lib, h = s.lib, s._h
    oc = C.c_int(0)
    for st in (lib.mi355x_kkt_lbfgs_define(h, N, 6, 0, 1.0, 1e-8, 1e8), lib.mi355x_kkt_lbfgs_push(h, p, p, C.byref(oc)),
               lib.mi355x_kkt_lbfgs_push_device(h, C.c_void_p(8), C.c_void_p(8), C.byref(oc)), lib.mi355x_kkt_lbfgs_reset(h), lib.mi355x_kkt_lbfgs_clear(h),
               lib.mi355x_kkt_lbfgs_info(h, None, None, None, None, None, None), lib.mi355x_kkt_lbfgs_get(h, 0, p, N)):
        assert st == kkt.FATAL and "no usable HIP device" in s.last_error()
    with pytest.raises(ipopt_amd.KKTError, match="no usable HIP device"):
        s.lbfgs_define(N, 6)


@pytest.mark.parametrize("m", [1, 2, 6, 32])
def test_coefficients_agree_with_the_float64_specification(m):
    rows = 300
    S, Y = lb.make_pairs(rows, m, seed=40 + m)
    H = lb.History(rows, m)
    for j in range(m):
        assert H.push(S[:, j], Y[:, j]) == lb.STORED
    d, Cs, Ls = lb.coefficients(H.STS, H.L, H.D, H.sigma)
    st, Cm, Lbar = kkt.lbfgs_coefficients(H.STS, H.L, H.D, H.sigma)
    assert st == kkt.SUCCESS
    eC = np.abs(Cm - Cs).max() / np.abs(Cs).max()
    eL = np.abs(Lbar - Ls).max() / max(np.abs(Ls).max(), np.abs(Cs).max())          # (m = 1: Lbar is the 1 x 1 zero)
    print(f"m = {m}: C {eC:.2e}, Lbar {eL:.2e}")
    assert eC <= 1e-13 and eL <= 1e-13
    assert np.all(np.tril(Cm, -1) == 0.0) and np.all(np.tril(Lbar) == 0.0)          # C upper, Lbar strictly upper triangular


def test_coefficients_answer_singular_on_the_vanishing_pivot():
    """init constant 1e8, s = e_1, y = 1e-9 e_1 pushed twice: M = [[1e8, 1e8], [1e8, 1e8]] in float64, the second Cholesky pivot is exactly 0"""
    sts = np.ones((2, 2)); L = np.array([[0.0, 0.0], [1e-9, 0.0]]); D = np.array([1e-9, 1e-9])
    assert lb.coefficients(sts, L, D, 1e8) is None                                   # the float64 specification fails as well
    st, _, _ = kkt.lbfgs_coefficients(sts, L, D, 1e8)
    assert st == kkt.SINGULAR
    st, Cm, _ = kkt.lbfgs_coefficients(sts[:1, :1], L[:1, :1], D[:1], 1e8)           # the first push alone is fine
    assert st == kkt.SUCCESS and Cm[0, 0] == 1e-4
    assert kkt.lbfgs_coefficients(sts, L, np.array([1e-9, 0.0]), 1e8)[0] == kkt.SINGULAR
    assert kkt.lbfgs_coefficients(sts, L, np.array([1e-9, np.nan]), 1e8)[0] == kkt.SINGULAR
    with pytest.raises(ipopt_amd.KKTError):
        kkt.lbfgs_coefficients(np.eye(33), np.zeros((33, 33)), np.ones(33), 1.0)
