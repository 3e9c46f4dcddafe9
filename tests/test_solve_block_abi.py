"""Host only (no device): the switch of the solve-block path through the C ABI and its Python wrapper -- mi355x_kkt_set_solve_block /
mi355x_kkt_solve_block_info before and after the analysis, the refusal on a multi-GPU handle, null-pointer arguments."""
import ctypes as C

import numpy as np
import pytest

import ipopt_amd
from ipopt_amd import kkt
from tests.support import blockfix as BF, kktgen


def analysed(**opts):
    n, r, c, v, _ = kktgen.lukvl_like(300)
    s = ipopt_amd.KKTSolver(**opts)
    s.initialize_structure(n, r, c, vals=v)
    return s


def test_round_trip_before_and_after_the_analysis():
    s = ipopt_amd.KKTSolver()
    before = s.solve_block_info()
    assert before == dict(on=False, width=BF.WIDTH, first_top_level=0, blocked_launches=0, bycol_launches=0, top_launches_per_column=0, last_ms=0.0)
    s.set_solve_block(True)
    assert s.solve_block_info()["on"] is True
    n, r, c, v, _ = kktgen.lukvl_like(300)
    s.initialize_structure(n, r, c, vals=v)
    after = s.solve_block_info()
    assert after["on"] is True and after["width"] == BF.WIDTH and after["last_ms"] == 0.0      # the switch survives the analysis
    rec, ls, counts = BF.expected(s)
    assert after["first_top_level"] == ls and (after["blocked_launches"], after["bycol_launches"], after["top_launches_per_column"]) == counts
    assert sum(counts) > 0
    s.set_solve_block(False)
    assert s.solve_block_info() == dict(after, on=False)
    s.set_solve_block(7)
    assert s.solve_block_info()["on"] is True
    s.close()


def test_a_multi_gpu_handle_is_refused():
    s = analysed(nranks=2, rank=0)
    with pytest.raises(kkt.KKTError, match="set_solve_block: not supported on a multi-GPU handle"):
        s.set_solve_block(True)
    assert s.lib.mi355x_kkt_set_solve_block(s._h, 0) == kkt.FATAL      # switching it off is refused alike: the call is a single-GPU one
    info = s.solve_block_info()
    assert info["on"] is False and info["blocked_launches"] == info["bycol_launches"] == info["top_launches_per_column"] == 0
    with pytest.raises(kkt.KKTError, match="single-GPU"):
        s.launch_plan("solve.single.block", nranks=2, rank=0)
    s.close()


def test_null_pointer_arguments():
    s = analysed()
    lib = s.lib
    assert lib.mi355x_kkt_set_solve_block(None, 1) == kkt.FATAL
    assert lib.mi355x_kkt_solve_block_info(None, None, None, None, None, None, None, None) == kkt.FATAL
    assert lib.mi355x_kkt_solve_block_info(s._h, None, None, None, None, None, None, None) == 0      # every output is optional
    w, ms = C.c_int(-1), C.c_double(-1.0)
    assert lib.mi355x_kkt_solve_block_info(s._h, None, C.byref(w), None, None, None, None, C.byref(ms)) == 0
    assert w.value == BF.WIDTH and ms.value == 0.0
    s.close()


def test_the_exported_schedule_has_whole_records():
    s = analysed()
    assert s.launch_plan("solve.single.block").size % 13 == 0 and np.all(BF.schedule(s)[:, 1] <= BF.SB_TOP)
    s.close()
