"""-m 'not gpu': the entry points of the quasi-Newton pair formed on the device (mi355x_kkt_qn_pair_*) are exported and listed, check every argument and
every state rule BEFORE the device is touched (naming what is wrong), refuse an unanalysed and a multi-GPU handle, and -- with valid arguments and no
device -- fail loudly: there is no host stand-in for the kernel.  The value assembly a definition sits on needs a device, so on a machine without one
a handle answers what can be asked of it there -- dims4 against n, ns against nd, the segment indices, form before store, push before form, get with a
bad capacity -- and the validation of the triplets is asked of mi355x_kkt_qn_pair_check, which needs neither a handle nor a device and is the code
qn_pair_define runs.  The rules that need a stored or formed pair (the grad_f mismatch, push with no history, get with a capacity below the array) are
host functions of ipopt_amd/csrc/qn_pair_host.h: the stand-alone program tests/support/qn_pair_host_check.cpp walks them, and the column view of small
structures against arrays written down by hand, under AddressSanitizer and UBSan; tests/test_gpu_qn_pair.py asks them of a handle with a device.
Nothing is loaded into python under a sanitizer."""
import ctypes as C

import numpy as np
import pytest

import ipopt_amd
from ipopt_amd import kkt
from tests.support import qn_pair_spec as qp
from tests.test_sr1_abi import _run_host_program_under_sanitizers

QN_PAIR = ["mi355x_kkt_qn_pair_check", "mi355x_kkt_qn_pair_define", "mi355x_kkt_qn_pair_store", "mi355x_kkt_qn_pair_form", "mi355x_kkt_qn_pair_push",
           "mi355x_kkt_qn_pair_get", "mi355x_kkt_qn_pair_info", "mi355x_kkt_qn_pair_clear"]
N = 6
DIMS = np.array([3, 1, 1, 1], dtype=np.int32)


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


def test_qn_pair_symbols_are_exported_and_listed():
    lib = C.CDLL(ipopt_amd.library_path())
    for name in QN_PAIR:
        assert hasattr(lib, name), name
        assert name in kkt.ABI_SYMBOLS
    for name in ("qn_pair_define", "qn_pair_store", "qn_pair_store_device", "qn_pair_form", "qn_pair_form_device", "qn_pair_push", "qn_pair_get", "qn_pair_info",
                 "qn_pair_clear"):
        assert callable(getattr(ipopt_amd.KKTSolver, name))
    assert callable(kkt.qn_pair_check)


def test_every_argument_is_checked_before_the_device_and_named():
    s = analysed()
    lib, h = s.lib, s._h
    v = np.ones(N); p = v.ctypes.data
    irn = np.arange(1, N + 1, dtype=np.int32); ip = irn.ctypes.data
    oc = C.c_int(7)

    def refused(call, word, *args):
        assert call(h, *args) == kkt.FATAL
        assert word in s.last_error(), (word, s.last_error())

    d = lib.mi355x_kkt_qn_pair_define
    refused(d, "dims4 is null", None, ip, ip, -1, -1)
    refused(d, "must equal n = 6", np.array([3, 1, 1, 2], dtype=np.int32).ctypes.data, ip, ip, -1, -1)        # dims not summing to n
    refused(d, "ns = 2 must equal nd = 0", np.array([3, 2, 1, 0], dtype=np.int32).ctypes.data, ip, ip, -1, -1)
    refused(d, "seg_jc = 3 is out of range", DIMS.ctypes.data, ip, ip, 3, -1)                                # (no assembly on this handle: every index is)
    refused(d, "seg_jd = 0 is out of range", DIMS.ctypes.data, ip, ip, -1, 0)
    assert "qn_pair_define" in s.last_error()
    refused(lib.mi355x_kkt_qn_pair_store, "grad_f", None, p, 0)                                              # a roll takes no grad_f
    refused(lib.mi355x_kkt_qn_pair_store, "qn_pair_define first", p, p, 0)
    refused(lib.mi355x_kkt_qn_pair_store, "qn_pair_define first", None, None, 0)
    assert "qn_pair_store" in s.last_error()
    refused(lib.mi355x_kkt_qn_pair_form, "x is null", None, p, p, p, 0, None)
    refused(lib.mi355x_kkt_qn_pair_form, "qn_pair_define first", p, p, p, p, 0, None)                        # form before store, before define
    assert "qn_pair_form" in s.last_error()
    refused(lib.mi355x_kkt_qn_pair_push, "qn_pair_define first", 1.0, C.byref(oc))                           # push before form
    assert oc.value == 1 and "qn_pair_push" in s.last_error()                                                # a refused push stored nothing
    refused(lib.mi355x_kkt_qn_pair_get, "what", -1, p, N)
    refused(lib.mi355x_kkt_qn_pair_get, "what", 6, p, N)
    refused(lib.mi355x_kkt_qn_pair_get, "capacity", 0, p, -1)
    refused(lib.mi355x_kkt_qn_pair_get, "out is null", 0, None, N)
    refused(lib.mi355x_kkt_qn_pair_get, "qn_pair_define first", 0, p, N)
    assert "qn_pair_get" in s.last_error()


def test_a_handle_that_is_not_analysed_is_refused():
    s = ipopt_amd.KKTSolver()
    v = np.ones(N); p = v.ctypes.data
    irn = np.arange(1, N + 1, dtype=np.int32); ip = irn.ctypes.data
    lib, h = s.lib, s._h
    for st in (lib.mi355x_kkt_qn_pair_define(h, DIMS.ctypes.data, ip, ip, -1, -1), lib.mi355x_kkt_qn_pair_store(h, p, p, 0),
               lib.mi355x_kkt_qn_pair_form(h, p, p, p, p, 0, None), lib.mi355x_kkt_qn_pair_push(h, 1.0, None), lib.mi355x_kkt_qn_pair_get(h, 0, p, N),
               lib.mi355x_kkt_qn_pair_info(h, None, None, None, None, None, None), lib.mi355x_kkt_qn_pair_clear(h)):
        assert st == kkt.FATAL and "not analysed" in s.last_error()


def test_a_multi_gpu_handle_is_refused():
    s = analysed(nranks=2, rank=0)
    v = np.ones(N); p = v.ctypes.data
    irn = np.arange(1, N + 1, dtype=np.int32); ip = irn.ctypes.data
    lib, h = s.lib, s._h
    for st in (lib.mi355x_kkt_qn_pair_define(h, DIMS.ctypes.data, ip, ip, -1, -1), lib.mi355x_kkt_qn_pair_store(h, p, p, 0),
               lib.mi355x_kkt_qn_pair_form(h, p, p, p, p, 0, None), lib.mi355x_kkt_qn_pair_push(h, 1.0, None), lib.mi355x_kkt_qn_pair_get(h, 0, p, N),
               lib.mi355x_kkt_qn_pair_info(h, None, None, None, None, None, None), lib.mi355x_kkt_qn_pair_clear(h)):
        assert st == kkt.FATAL and "not supported on a multi-GPU handle" in s.last_error()
    with pytest.raises(ipopt_amd.KKTError, match="not supported on a multi-GPU handle"):
        s.qn_pair_clear()


@pytest.mark.skipif(_has_gpu(), reason="only meaningful on a machine without a GPU")
def test_valid_arguments_without_a_device_fail_loudly():
    s = analysed()
    irn = np.arange(1, N + 1, dtype=np.int32); ip = irn.ctypes.data
    lib, h = s.lib, s._h
    for st in (lib.mi355x_kkt_qn_pair_define(h, DIMS.ctypes.data, ip, ip, -1, -1), lib.mi355x_kkt_qn_pair_info(h, None, None, None, None, None, None),
               lib.mi355x_kkt_qn_pair_clear(h)):
        assert st == kkt.FATAL and "no usable HIP device" in s.last_error()
    with pytest.raises(ipopt_amd.KKTError, match="no usable HIP device"):
        s.qn_pair_define(DIMS, irn, irn, -1, -1)
    # nothing can be defined without a device: the other calls say so, as errors
    for call in (lambda: s.qn_pair_store(np.ones(0)), lambda: s.qn_pair_form(np.ones(0), None, None, None), s.qn_pair_push, lambda: s.qn_pair_get("s")):
        with pytest.raises(ipopt_amd.KKTError):
            call()


def test_qn_pair_check_answers_without_a_handle():
    """the validation of qn_pair_define, on the triplets of a case of the GPU tests and on hostile copies of them"""
    c = next(x for x in qp.INPUTS() if x["name"] == "duplicates")
    n, irn, jcn, lens = qp.system(c)
    off = np.concatenate([[0], np.cumsum(lens)])
    dims = [c["nx"], c["ns"], c["nc"], c["nd"]]
    segs = (off[qp.SEG_JC], lens[qp.SEG_JC], off[qp.SEG_JD], lens[qp.SEG_JD])
    nnz = len(irn)
    assert kkt.qn_pair_check(nnz, dims, irn, jcn, *segs) == (True, "")
    assert kkt.qn_pair_check(nnz, dims, jcn, irn, *segs) == (True, "")                                       # either orientation
    assert kkt.qn_pair_check(nnz, dims, irn, jcn, 0, 0, 0, 0) == (True, "")                                  # both blocks absent

    def refused(words, *args):
        ok, why = kkt.qn_pair_check(*args)
        assert not ok and all(w in why for w in words), why

    refused(["ns", "nd"], nnz, [c["nx"], c["ns"] + 1, c["nc"], c["nd"]], irn, jcn, *segs)
    refused(["dims4[2]"], nnz, [c["nx"], c["ns"], -1, c["nd"]], irn, jcn, *segs)
    refused(["J_c segment", "not inside"], nnz, dims, irn, jcn, segs[0], nnz, segs[2], segs[3])               # a segment out of range
    refused(["J_d segment", "not inside"], nnz, dims, irn, jcn, segs[0], segs[1], -1, segs[3])
    refused(["overlap"], nnz, dims, irn, jcn, segs[0], segs[1], segs[0] + 1, 2)
    t = int(off[qp.SEG_JC]) + 5
    bad = irn.copy(); bad[t] = c["nx"] + c["ns"] + c["nc"] + 1                                               # a J_c triplet whose row lies in the d block
    refused([f"J_c triplet at position {t}", "c block"], nnz, dims, bad, jcn, *segs)
    bad = irn.copy(); bad[t] = 2; bad[t + 3] = 1                                                             # both indices in x: the first is named
    refused([f"position {t}", "both indices lie in the x block"], nnz, dims, bad, jcn, *segs)
    t = int(off[qp.SEG_JD]) + 1
    bad = irn.copy(); bad[t] = c["nx"] + c["ns"] + 1                                                         # a J_d triplet whose row lies in the c block
    refused([f"J_d triplet at position {t}", "d block"], nnz, dims, bad, jcn, *segs)
    bad = jcn.copy(); bad[t] = 0
    refused([f"J_d triplet at position {t}"], nnz, dims, irn, bad, *segs)
    assert C.CDLL(ipopt_amd.library_path()).mi355x_kkt_qn_pair_check(C.c_int64(4), None, None, None, C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0), None, C.c_int64(0)) == kkt.FATAL


def test_the_host_header_under_address_and_ub_sanitizers(tmp_path):
    """the column view against arrays written down by hand (an empty block, duplicates, both orientations, a column with no entry), the validation and the
    state rules of store / form / push / get: tests/support/qn_pair_host_check.cpp"""
    _run_host_program_under_sanitizers(tmp_path, "qn_pair_host_check")
