"""-m 'not gpu': the low-rank entry points of the C ABI (mi355x_kkt_lowrank_*) are exported, check every argument BEFORE the device is touched
(so the checks answer on a machine without one, naming the offending argument), refuse a multi-GPU handle, and -- with valid arguments and no
device -- fail loudly like factor / solve do: there is no host stand-in for the tall-skinny algebra."""
import ctypes as C

import numpy as np
import pytest

import ipopt_amd
from ipopt_amd import kkt

LOWRANK = ["mi355x_kkt_lowrank_set", "mi355x_kkt_lowrank_update", "mi355x_kkt_lowrank_solve", "mi355x_kkt_lowrank_solve_device2",
           "mi355x_kkt_lowrank_clear", "mi355x_kkt_lowrank_info"]
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


def test_lowrank_symbols_are_exported_and_declared():
    lib = C.CDLL(ipopt_amd.library_path())
    for name in LOWRANK:
        assert hasattr(lib, name), name
        assert name in kkt.ABI_SYMBOLS
    assert kkt.LOWRANK_MAX == 32


def test_every_argument_is_checked_before_the_device_and_named():
    s = analysed()
    lib, h = s.lib, s._h
    A = np.asfortranarray(np.ones((N, 33)))
    p = A.ctypes.data

    def refused(word, *args):
        assert lib.mi355x_kkt_lowrank_set(h, *args) == kkt.FATAL
        assert word in s.last_error() and "lowrank_set" in s.last_error(), (word, s.last_error())

    refused("rows", -1, 1, p, N, 1, p, N)
    refused("rows", N + 1, 1, p, N + 1, 1, p, N + 1)
    refused("nv", 2, -1, p, N, 1, p, N)
    refused("nv", 2, 33, p, N, 1, p, N)
    refused("nu", 2, 1, p, N, -1, p, N)
    refused("nu", 2, 1, p, N, 33, p, N)
    refused("ldv", 4, 2, p, 3, 1, p, N)
    refused("ldu", 4, 2, p, N, 1, p, 3)
    refused("V", 4, 2, None, N, 1, p, N)
    refused("U", 4, 2, p, N, 1, None, N)
    # the solves: counts, pointers, leading dimensions
    x = np.ones((2, N))
    for call, word, args in [(lib.mi355x_kkt_lowrank_solve, "nrhs", (-1, x.ctypes.data, N)),
                             (lib.mi355x_kkt_lowrank_solve, "rhs_inout", (1, None, N)),
                             (lib.mi355x_kkt_lowrank_solve, "ld", (2, x.ctypes.data, N - 1)),
                             (lib.mi355x_kkt_lowrank_solve_device2, "nrhs", (-1, None, N, None, N)),
                             (lib.mi355x_kkt_lowrank_solve_device2, "d_b", (1, None, N, C.c_void_p(8), N)),
                             (lib.mi355x_kkt_lowrank_solve_device2, "d_x", (1, C.c_void_p(8), N, None, N)),
                             (lib.mi355x_kkt_lowrank_solve_device2, "ldb", (2, C.c_void_p(8), N - 1, C.c_void_p(8), N)),
                             (lib.mi355x_kkt_lowrank_solve_device2, "ldx", (2, C.c_void_p(8), N, C.c_void_p(8), N - 1))]:
        assert call(h, *args) == kkt.FATAL
        assert word in s.last_error(), (word, s.last_error())


def test_a_handle_that_is_not_analysed_is_refused():
    s = ipopt_amd.KKTSolver()
    A = np.asfortranarray(np.ones((N, 2)))
    which = C.c_int(0)
    for st in (s.lib.mi355x_kkt_lowrank_set(s._h, 0, 0, None, 1, 0, None, 1), s.lib.mi355x_kkt_lowrank_update(s._h, C.byref(which)),
               s.lib.mi355x_kkt_lowrank_solve(s._h, 1, A.ctypes.data, N), s.lib.mi355x_kkt_lowrank_clear(s._h),
               s.lib.mi355x_kkt_lowrank_info(s._h, None, None, None, None, None)):
        assert st == kkt.FATAL and "not analysed" in s.last_error()


def test_a_multi_gpu_handle_is_refused():
    s = analysed(nranks=2, rank=0)
    A = np.asfortranarray(np.ones((N, 2)))
    with pytest.raises(ipopt_amd.KKTError, match="not supported on a multi-GPU handle"):
        s.lowrank_set(A, A)
    with pytest.raises(ipopt_amd.KKTError, match="not supported on a multi-GPU handle"):
        s.lowrank_update()
    with pytest.raises(ipopt_amd.KKTError, match="not supported on a multi-GPU handle"):
        s.lowrank_solve(np.ones(N))
    with pytest.raises(ipopt_amd.KKTError, match="not supported on a multi-GPU handle"):
        s.lowrank_clear()


@pytest.mark.skipif(_has_gpu(), reason="only meaningful on a machine without a GPU")
def test_valid_arguments_without_a_device_fail_loudly():
    s = analysed()
    A = np.asfortranarray(np.ones((N, 2)))
    for call in (lambda: s.lowrank_set(A, A), lambda: s.lowrank_set(None, None, rows=0), s.lowrank_update, lambda: s.lowrank_solve(np.ones(N)),
                 lambda: s.lowrank_solve_device2(8, 8), s.lowrank_clear, s.lowrank_info):
        with pytest.raises(ipopt_amd.KKTError, match="no usable HIP device"):
            call()
