"""-m 'not gpu': the restoration-phase entry points of the C ABI (mi355x_kkt_lbfgs_define_resto, _lbfgs_push_resto, _lbfgs_push_resto_device,
_lbfgs_resto_info) are exported and listed, check every argument BEFORE the device is touched (naming the offending argument): dr null or with an
entry that is not positive and finite, eta not positive and finite, type and special outside {0, 1}; they refuse an unanalysed and a multi-GPU
handle, and -- with valid arguments and no device -- fail loudly.  That a plain history refuses _lbfgs_push_resto and a restoration-phase history
_lbfgs_push needs a defined history, hence a device: tests/test_gpu_resto.py.
The host transitions (lb_push_bfgs_resto, lb_push_sr1_resto, lb_undo_resto of lbfgs_host.h) run under AddressSanitizer and UBSan in a stand-alone
program, tests/support/lbfgs_resto_check.cpp: eviction, eta changes, both skips, undo and the Cholesky-fails outcome against a model kept by the rule."""
import ctypes as C

import numpy as np
import pytest

import ipopt_amd
from ipopt_amd import kkt
from tests.test_sr1_abi import N, _has_gpu, _run_host_program_under_sanitizers, analysed

RESTO = ["mi355x_kkt_lbfgs_define_resto", "mi355x_kkt_lbfgs_push_resto", "mi355x_kkt_lbfgs_push_resto_device", "mi355x_kkt_lbfgs_resto_info"]


def test_resto_symbols_are_exported_and_listed():
    lib = C.CDLL(ipopt_amd.library_path())
    for name in RESTO:
        assert hasattr(lib, name), name
        assert name in kkt.ABI_SYMBOLS
    for name in ("lbfgs_define_resto", "lbfgs_push_resto", "lbfgs_push_resto_device", "lbfgs_resto_info"):
        assert callable(getattr(ipopt_amd.KKTSolver, name))


def test_every_argument_is_checked_before_the_device_and_named():
    s = analysed()
    lib, h = s.lib, s._h
    dr = np.full(N, 0.5); p = dr.ctypes.data
    oc = C.c_int(7)

    def refused(call, word, *args):
        assert call(h, *args) == kkt.FATAL
        assert word in s.last_error(), (word, s.last_error())

    d = lib.mi355x_kkt_lbfgs_define_resto
    refused(d, "rows", 0, 6, 0, 0, 0, 1.0, 1e-8, 1e8, p)
    refused(d, "rows", N + 1, 6, 0, 0, 0, 1.0, 1e-8, 1e8, p)
    refused(d, "max_history", N, 0, 0, 0, 0, 1.0, 1e-8, 1e8, p)
    refused(d, "max_history", N, 33, 0, 0, 0, 1.0, 1e-8, 1e8, p)
    refused(d, "type", N, 6, -1, 0, 0, 1.0, 1e-8, 1e8, p)
    refused(d, "type", N, 6, 2, 0, 0, 1.0, 1e-8, 1e8, p)
    refused(d, "special", N, 6, 0, 2, 0, 1.0, 1e-8, 1e8, p)
    refused(d, "special", N, 6, 1, -1, 0, 1.0, 1e-8, 1e8, p)
    refused(d, "init ", N, 6, 0, 0, 5, 1.0, 1e-8, 1e8, p)
    refused(d, "init_val", N, 6, 0, 0, 4, 0.0, 1e-8, 1e8, p)
    refused(d, "sigma_min", N, 6, 0, 0, 0, 1.0, 0.0, 1e8, p)
    refused(d, "sigma_max", N, 6, 0, 0, 0, 1.0, 1e-3, 1e-4, p)
    refused(d, "dr is null", N, 6, 0, 0, 0, 1.0, 1e-8, 1e8, None)
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        for type_ in (0, 1):
            for special in (0, 1):
                dr2 = dr.copy(); dr2[N - 2] = bad
                refused(d, "dr must be positive and finite", N, 6, type_, special, 0, 1.0, 1e-8, 1e8, dr2.ctypes.data)
                assert f"entry {N - 2}" in s.last_error()
    assert "lbfgs_define_resto" in s.last_error()
    e = C.c_double
    refused(lib.mi355x_kkt_lbfgs_push_resto, "s is null", None, p, e(0.3), C.byref(oc))
    refused(lib.mi355x_kkt_lbfgs_push_resto, "ypart is null", p, None, e(0.3), C.byref(oc))
    for bad in (0.0, -0.3, float("nan"), float("inf")):
        refused(lib.mi355x_kkt_lbfgs_push_resto, "eta", p, p, e(bad), C.byref(oc))
        refused(lib.mi355x_kkt_lbfgs_push_resto_device, "eta", C.c_void_p(8), C.c_void_p(8), e(bad), C.byref(oc))
    assert oc.value == 1                                                             # a refused push stored nothing
    refused(lib.mi355x_kkt_lbfgs_push_resto_device, "d_s", None, C.c_void_p(8), e(0.3), None)
    refused(lib.mi355x_kkt_lbfgs_push_resto_device, "d_ypart", C.c_void_p(8), None, e(0.3), None)
    assert "lbfgs_push_resto_device" in s.last_error()
    refused(lib.mi355x_kkt_lbfgs_get, "what", 9, p, N)
    refused(lib.mi355x_kkt_lbfgs_get, "what", 15, p, N)
    with pytest.raises(ipopt_amd.KKTError, match="dr must be a vector"):
        s.lbfgs_define_resto(N, np.ones(N - 1))
    with pytest.raises(ipopt_amd.KKTError, match="dr is null"):
        s.lbfgs_define_resto(N, None)


def test_a_handle_that_is_not_analysed_is_refused():
    s = ipopt_amd.KKTSolver()
    v = np.ones(N); p = v.ctypes.data
    lib, h = s.lib, s._h
    for st in (lib.mi355x_kkt_lbfgs_define_resto(h, N, 6, 0, 0, 0, 1.0, 1e-8, 1e8, p), lib.mi355x_kkt_lbfgs_push_resto(h, p, p, C.c_double(0.3), None),
               lib.mi355x_kkt_lbfgs_push_resto_device(h, C.c_void_p(8), C.c_void_p(8), C.c_double(0.3), None), lib.mi355x_kkt_lbfgs_resto_info(h, None, None, None)):
        assert st == kkt.FATAL and "not analysed" in s.last_error()


def test_a_multi_gpu_handle_is_refused():
    s = analysed(nranks=2, rank=0)
    v = np.ones(N)
    for call in (lambda: s.lbfgs_define_resto(N, v), lambda: s.lbfgs_push_resto(v, v, 0.3), lambda: s.lbfgs_push_resto_device(8, 8, 0.3), s.lbfgs_resto_info):
        with pytest.raises(ipopt_amd.KKTError, match="not supported on a multi-GPU handle"):
            call()


@pytest.mark.skipif(_has_gpu(), reason="only meaningful on a machine without a GPU")
def test_valid_arguments_without_a_device_fail_loudly():
    s = analysed()
    v = np.ones(N); p = v.ctypes.data
    lib, h = s.lib, s._h
    oc, r, eta = C.c_int(0), C.c_int(7), C.c_double(7.0)
    for st in (lib.mi355x_kkt_lbfgs_define_resto(h, N, 6, 1, 1, 0, 1.0, 1e-8, 1e8, p), lib.mi355x_kkt_lbfgs_push_resto(h, p, p, C.c_double(0.3), C.byref(oc)),
               lib.mi355x_kkt_lbfgs_push_resto_device(h, C.c_void_p(8), C.c_void_p(8), C.c_double(0.3), C.byref(oc)),
               lib.mi355x_kkt_lbfgs_resto_info(h, C.byref(r), None, C.byref(eta))):
        assert st == kkt.FATAL and "no usable HIP device" in s.last_error()
    assert oc.value == 1 and r.value == 0 and eta.value == 0.0
    with pytest.raises(ipopt_amd.KKTError, match="no usable HIP device"):
        s.lbfgs_define_resto(N, v, type=kkt.LBFGS_SR1, special=True)


def test_the_resto_transitions_on_the_cpu_under_sanitizers(tmp_path):
    """push, both skips, eviction at changing eta, undo and the Cholesky failure of lbfgs_host.h's restoration-phase transitions against a model kept by the
    rule alone; G, S^T S, R, D, L bitwise against a recomputation"""
    _run_host_program_under_sanitizers(tmp_path, "lbfgs_resto_check")
