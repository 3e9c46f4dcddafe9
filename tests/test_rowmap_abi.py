"""-m 'not gpu': the row-map entry points of the C ABI (mi355x_kkt_lowrank_rowmap, _rowmap_get, _rowmap_check, mi355x_kkt_lbfgs_push_mapped,
_push_resto_mapped) are exported, validate every argument BEFORE the device is touched (so each refusal answers on a machine without one and names
its argument) and refuse a multi-GPU handle.  The validation is load-bearing -- it is the reason no kernel reading through the map can index out of
range -- so it is also reachable on its own (_rowmap_check: host only, no handle), which is how `len` <= idx[rows-1] is answered here: without a
device no map can be set on a handle."""
import ctypes as C

import numpy as np
import pytest

import ipopt_amd
from ipopt_amd import kkt

ROWMAP = ["mi355x_kkt_lowrank_rowmap", "mi355x_kkt_lowrank_rowmap_get", "mi355x_kkt_lowrank_rowmap_check", "mi355x_kkt_lbfgs_push_mapped",
          "mi355x_kkt_lbfgs_push_resto_mapped"]
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


def i32(*v):
    return np.array(v, dtype=np.int32)


def test_rowmap_symbols_are_exported_and_declared():
    lib = C.CDLL(ipopt_amd.library_path())
    for name in ROWMAP:
        assert hasattr(lib, name), name
        assert name in kkt.ABI_SYMBOLS
    for method in ("lowrank_rowmap", "lowrank_rowmap_info", "lbfgs_push_mapped", "lbfgs_push_resto_mapped", "lbfgs_push_mapped_device",
                   "lbfgs_push_resto_mapped_device"):
        assert callable(getattr(ipopt_amd.KKTSolver, method))


REFUSALS = [("rows", -1, i32(0, 1)), ("rows", N + 1, i32(0, 1, 2, 3, 4, 5, 6)),
            ("idx[1] = -1", 3, i32(0, -1, 2)),                         # an index < 0 (the FIRST value out of range is named)
            ("idx[0] = -4", 2, i32(-4, -3)),
            ("idx[2] = 6", 3, i32(0, 1, N)),                           # an index >= n
            ("idx[1] = 9", 3, i32(0, 9, 11)),
            ("position 2", 4, i32(0, 3, 3, 5)),                        # equal neighbours (the FIRST position that is not ascending)
            ("position 1", 4, i32(4, 2, 3, 5))]                        # descending neighbours


@pytest.mark.parametrize("word,rows,idx", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_every_argument_of_the_map_is_checked_before_the_device_and_named(word, rows, idx):
    s = analysed()
    assert s.lib.mi355x_kkt_lowrank_rowmap(s._h, rows, idx.ctypes.data) == kkt.FATAL
    assert word in s.last_error() and "lowrank_rowmap" in s.last_error(), (word, s.last_error())
    ok, why = kkt.lowrank_rowmap_check(N, idx[:rows] if 0 <= rows <= idx.size else idx)      # the same function, without a handle
    if word != "rows":
        assert not ok and word in why, (word, why)


def test_the_stand_alone_check_accepts_what_is_valid_and_answers_len():
    assert kkt.lowrank_rowmap_check(N, i32(0, 2, 5)) == (True, "")
    assert kkt.lowrank_rowmap_check(N, i32()) == (True, "")
    assert kkt.lowrank_rowmap_check(N, np.arange(N)) == (True, "")
    assert kkt.lowrank_rowmap_check(N, i32(0, 2, 4), length=5) == (True, "")
    for length in (4, 3, 0):                                            # len <= idx[rows-1]
        ok, why = kkt.lowrank_rowmap_check(N, i32(0, 2, 4), length=length)
        assert not ok and "len" in why and "idx[rows-1]" in why, why
    ok, why = kkt.lowrank_rowmap_check(N, i32(), length=3)              # a vector length against no map
    assert not ok and "no row map" in why
    lib = C.CDLL(ipopt_amd.library_path())
    lib.mi355x_kkt_lowrank_rowmap_check.argtypes = [C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_char_p, C.c_int64]
    assert lib.mi355x_kkt_lowrank_rowmap_check(N, -1, None, -1, None, 0) == kkt.FATAL          # the message is optional
    assert lib.mi355x_kkt_lowrank_rowmap_check(-1, 0, None, -1, None, 0) == kkt.FATAL
    buf = C.create_string_buffer(8)                                     # a short buffer is filled and terminated, never overrun
    assert lib.mi355x_kkt_lowrank_rowmap_check(N, N + 1, None, -1, buf, 8) == kkt.FATAL and buf.value == b"rows mu"


def test_a_mapped_push_without_a_map_is_refused_before_the_device_and_named():
    s = analysed()
    x = np.ones(N)
    oc = C.c_int(7)
    for on_device in (0, 1):
        assert s.lib.mi355x_kkt_lbfgs_push_mapped(s._h, x.ctypes.data, x.ctypes.data, N, on_device, C.byref(oc)) == kkt.FATAL
        assert "lbfgs_push_mapped" in s.last_error() and "no row map" in s.last_error(), s.last_error()
        assert oc.value == 1
        assert s.lib.mi355x_kkt_lbfgs_push_resto_mapped(s._h, x.ctypes.data, x.ctypes.data, N, on_device, 0.5, C.byref(oc)) == kkt.FATAL
        assert "lbfgs_push_resto_mapped" in s.last_error() and "no row map" in s.last_error(), s.last_error()
    with pytest.raises(ipopt_amd.KKTError, match="no row map"):
        s.lbfgs_push_mapped(x, x)
    with pytest.raises(ipopt_amd.KKTError, match="no row map"):
        s.lbfgs_push_resto_mapped(x, x, 0.5)
    for call, word, args in [(s.lib.mi355x_kkt_lbfgs_push_mapped, "sx", (None, x.ctypes.data, N, 0, None)),
                             (s.lib.mi355x_kkt_lbfgs_push_mapped, "yx", (x.ctypes.data, None, N, 0, None)),
                             (s.lib.mi355x_kkt_lbfgs_push_resto_mapped, "ypartx", (x.ctypes.data, None, N, 0, 0.5, None)),
                             (s.lib.mi355x_kkt_lbfgs_push_resto_mapped, "eta", (x.ctypes.data, x.ctypes.data, N, 0, 0.0, None)),
                             (s.lib.mi355x_kkt_lbfgs_push_resto_mapped, "eta", (x.ctypes.data, x.ctypes.data, N, 0, float("nan"), None))]:
        assert call(s._h, *args) == kkt.FATAL
        assert word in s.last_error(), (word, s.last_error())
    with pytest.raises(ipopt_amd.KKTError, match="one length"):
        s.lbfgs_push_mapped(np.ones(N), np.ones(N - 1))


def test_rowmap_get_reports_no_map_and_checks_its_capacity():
    s = analysed()
    r = C.c_int(5)
    assert s.lib.mi355x_kkt_lowrank_rowmap_get(s._h, C.byref(r), None, 0) == kkt.SUCCESS and r.value == 0
    assert s.lib.mi355x_kkt_lowrank_rowmap_get(s._h, None, None, 0) == kkt.SUCCESS                # outputs may be NULL
    assert s.lowrank_rowmap_info() is None
    out = i32(0, 0)
    assert s.lib.mi355x_kkt_lowrank_rowmap_get(s._h, C.byref(r), out.ctypes.data, -1) == kkt.FATAL
    assert "capacity" in s.last_error() and "lowrank_rowmap_get" in s.last_error()


def test_a_handle_that_is_not_analysed_is_refused():
    s = ipopt_amd.KKTSolver()
    x = np.ones(N); idx = i32(0, 1)
    for st in (s.lib.mi355x_kkt_lowrank_rowmap(s._h, 2, idx.ctypes.data), s.lib.mi355x_kkt_lowrank_rowmap_get(s._h, None, None, 0),
               s.lib.mi355x_kkt_lbfgs_push_mapped(s._h, x.ctypes.data, x.ctypes.data, N, 0, None),
               s.lib.mi355x_kkt_lbfgs_push_resto_mapped(s._h, x.ctypes.data, x.ctypes.data, N, 0, 0.5, None)):
        assert st == kkt.FATAL and "not analysed" in s.last_error()


def test_a_multi_gpu_handle_is_refused():
    s = analysed(nranks=2, rank=0)
    x = np.ones(N)
    for call in (lambda: s.lowrank_rowmap(i32(0, 2)), lambda: s.lowrank_rowmap(None), s.lowrank_rowmap_info, lambda: s.lbfgs_push_mapped(x, x),
                 lambda: s.lbfgs_push_resto_mapped(x, x, 0.5), lambda: s.lbfgs_push_mapped_device(8, 8, N),
                 lambda: s.lbfgs_push_resto_mapped_device(8, 8, N, 0.5)):
        with pytest.raises(ipopt_amd.KKTError, match="not supported on a multi-GPU handle"):
            call()
    with pytest.raises(ipopt_amd.KKTError, match="idx"):                 # the arguments are still checked first
        s.lowrank_rowmap(i32(2, 0))


@pytest.mark.skipif(_has_gpu(), reason="only meaningful on a machine without a GPU")
def test_valid_arguments_without_a_device_fail_loudly():
    s = analysed()
    for call in (lambda: s.lowrank_rowmap(i32(0, 2, 5)), lambda: s.lowrank_rowmap(None)):
        with pytest.raises(ipopt_amd.KKTError, match="no usable HIP device"):
            call()
    assert s.lowrank_rowmap_info() is None                               # host state: answers without a device
