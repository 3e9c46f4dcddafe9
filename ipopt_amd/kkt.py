"""ctypes binding of include/mi355x_kkt.h.

Mirrors, method for method, the contract of the reference's SparseSymLinearSolverInterface
(reference src/Algorithm/LinearSolvers/IpSparseSymLinearSolverInterface.hpp:98-256):
``initialize_structure`` / ``values`` / ``multi_solve`` / ``number_of_neg_evals`` /
``increase_quality`` / ``provides_inertia`` -- same argument meaning, same status codes
(IpSymLinearSolver.hpp:19-33) -- so the parity tests read like the reference's adapters' callers
(IpTSymLinearSolver.cpp:159-312).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

STATUS = {0: "SUCCESS", 1: "SINGULAR", 2: "WRONG_INERTIA", 3: "CALL_AGAIN", 4: "FATAL_ERROR"}
SUCCESS, SINGULAR, WRONG_INERTIA, CALL_AGAIN, FATAL = 0, 1, 2, 3, 4
FMT_TRIPLET, FMT_CSR_UPPER = 0, 1


class KKTError(RuntimeError):
    pass


class _Options(C.Structure):
    _fields_ = [("device", C.c_int), ("index_base", C.c_int), ("ordering", C.c_int), ("matching", C.c_int),
                ("scaling", C.c_int), ("nd_leaf", C.c_int), ("nemin", C.c_int), ("max_sn_cols", C.c_int),
                ("pivtol", C.c_double), ("pivtolmax", C.c_double), ("small", C.c_double),
                ("refine_steps", C.c_int), ("use_graph", C.c_int), ("nranks", C.c_int), ("rank", C.c_int),
                ("verbose", C.c_int), ("leaf_cols", C.c_int), ("tree_merge", C.c_int), ("wide_panels", C.c_int), ("chain_group", C.c_int), ("solve_group", C.c_int), ("subcube", C.c_int), ("delay_rounds", C.c_int), ("smart_quality", C.c_int)]


class _Info(C.Structure):
    _fields_ = [("n", C.c_int), ("nnz_in", C.c_int), ("nnz_a", C.c_int), ("nnz_l", C.c_int64),
                ("flops_factor", C.c_int64), ("flops_solve", C.c_int64), ("bytes_factor", C.c_int64),
                ("bytes_solve", C.c_int64), ("sum_sn_rows", C.c_int64), ("cb_doubles", C.c_int64),
                ("num_sn", C.c_int), ("num_levels", C.c_int), ("maxfront", C.c_int), ("maxsupernode", C.c_int),
                ("num_pairs", C.c_int), ("num_neg", C.c_int), ("num_zero", C.c_int), ("num_two", C.c_int),
                ("num_small", C.c_int), ("num_big_fronts", C.c_int), ("time_analyse", C.c_double),
                ("time_factor_ms", C.c_double), ("time_solve_ms", C.c_double), ("pivtol", C.c_double), ("u_sensitive", C.c_int),
                ("num_fast_blocks", C.c_int), ("num_delayed", C.c_int), ("num_restructures", C.c_int), ("matching_ms", C.c_double), ("matching_rounds", C.c_int), ("matching_unmatched", C.c_int), ("reserved", C.c_double * 3)]


@dataclass
class KKTInfo:
    n: int; nnz_in: int; nnz_a: int; nnz_l: int; flops_factor: int; flops_solve: int; bytes_factor: int
    bytes_solve: int; sum_sn_rows: int; cb_doubles: int; num_sn: int; num_levels: int; maxfront: int
    maxsupernode: int; num_pairs: int; num_neg: int; num_zero: int; num_two: int; num_small: int
    num_big_fronts: int; time_analyse: float; time_factor_ms: float; time_solve_ms: float; pivtol: float; u_sensitive: int; num_fast_blocks: int; num_delayed: int; num_restructures: int
    matching_ms: float; matching_rounds: int; matching_unmatched: int


def library_path() -> str:
    # (MI355X_KKT_LIBRARY: development aid -- an A/B variant of the library built by `make variant`, see ipopt_amd/Makefile)
    return os.environ.get("MI355X_KKT_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libmi355x_kkt.so")


_LIB = None
# int (*)(void* ctx, void* dptr, int64_t count, int dtype, void* hip_stream)  -- mi355x_kkt_allreduce_fn
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p)
ALLREDUCE_RANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_int)      # + rank_lo, nranks_in_range

# every symbol include/mi355x_kkt.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "mi355x_kkt_default_options", "mi355x_kkt_create", "mi355x_kkt_destroy", "mi355x_kkt_analyse",
    "mi355x_kkt_values_buffer", "mi355x_kkt_factor", "mi355x_kkt_refactor", "mi355x_kkt_solve",
    "mi355x_kkt_solve_device", "mi355x_kkt_solve_device2", "mi355x_kkt_set_pivtol", "mi355x_kkt_set_pivtolmax", "mi355x_kkt_increase_quality",
    "mi355x_kkt_get_info", "mi355x_kkt_last_error",
    "mi355x_kkt_get_symbolic", "mi355x_kkt_get_launch_plan", "mi355x_kkt_factor_local", "mi355x_kkt_top_arena", "mi355x_kkt_factor_top",
    "mi355x_kkt_solve_fwd_local", "mi355x_kkt_top_rhs", "mi355x_kkt_solve_top_and_bwd", "mi355x_kkt_profile",
    "mi355x_kkt_comm_unique_id", "mi355x_kkt_set_comm_rccl", "mi355x_kkt_comm_shm_id", "mi355x_kkt_comm_shm_discard", "mi355x_kkt_set_comm_shm", "mi355x_kkt_set_comm_callbacks", "mi355x_kkt_set_comm_range_callback", "mi355x_kkt_exchange_bytes", "mi355x_kkt_comm_plan", "mi355x_kkt_comm_info",
    "mi355x_kkt_set_scaling", "mi355x_kkt_get_scaling", "mi355x_kkt_ruiz_scaling", "mi355x_kkt_matching_scaling", "mi355x_kkt_zero_pivots", "mi355x_kkt_failed_pivots", "mi355x_kkt_delay_columns", "mi355x_kkt_set_delay_rounds", "mi355x_kkt_assembly_define", "mi355x_kkt_assembly_buffer", "mi355x_kkt_assembly_upload", "mi355x_kkt_factor_assembled",
    "mi355x_kkt_pd_define", "mi355x_kkt_pd_put_data", "mi355x_kkt_pd_put", "mi355x_kkt_pd_get", "mi355x_kkt_pd_solve_once", "mi355x_kkt_pd_residual",
    "mi355x_kkt_set_solve_block", "mi355x_kkt_solve_block_info",
    "mi355x_kkt_lowrank_set", "mi355x_kkt_lowrank_update", "mi355x_kkt_lowrank_solve", "mi355x_kkt_lowrank_solve_device2", "mi355x_kkt_lowrank_clear", "mi355x_kkt_lowrank_info",
    "mi355x_kkt_lbfgs_define", "mi355x_kkt_lbfgs_push", "mi355x_kkt_lbfgs_push_device", "mi355x_kkt_lbfgs_reset", "mi355x_kkt_lbfgs_clear", "mi355x_kkt_lbfgs_info", "mi355x_kkt_lbfgs_get", "mi355x_kkt_lbfgs_coefficients",
    "mi355x_kkt_lbfgs_define_sr1", "mi355x_kkt_lbfgs_undo", "mi355x_kkt_lbfgs_sr1_info", "mi355x_kkt_lbfgs_sr1_coefficients",
    "mi355x_kkt_lbfgs_define_resto", "mi355x_kkt_lbfgs_push_resto", "mi355x_kkt_lbfgs_push_resto_device", "mi355x_kkt_lbfgs_resto_info",
    "mi355x_kkt_lowrank_rowmap", "mi355x_kkt_lowrank_rowmap_get", "mi355x_kkt_lowrank_rowmap_check", "mi355x_kkt_lbfgs_push_mapped", "mi355x_kkt_lbfgs_push_resto_mapped",
    "mi355x_kkt_qn_pair_check", "mi355x_kkt_qn_pair_define", "mi355x_kkt_qn_pair_store", "mi355x_kkt_qn_pair_form", "mi355x_kkt_qn_pair_push", "mi355x_kkt_qn_pair_get", "mi355x_kkt_qn_pair_info", "mi355x_kkt_qn_pair_clear",
]
LOWRANK_MAX = 32
LBFGS_MAX = 32
LBFGS_INIT = {"scalar1": 0, "scalar2": 1, "scalar3": 2, "scalar4": 3, "constant": 4}      # limited_memory_initialization
LBFGS_STORED, LBFGS_SKIPPED, LBFGS_NOT_POSDEF = 0, 1, 2                                     # outcome of a push
LBFGS_BFGS, LBFGS_SR1 = 0, 1                                                                # limited_memory_update_type of a history
KERNEL_KINDS = ["gather_scale", "front_wave", "front_lds64", "front_lds128", "big_assemble", "big_diag", "big_trsm", "big_schur",
                "stats", "solve_perm", "fwd_wave", "fwd_lds", "fwd_big", "bwd_wave", "bwd_lds", "bwd_big", "fwd_big_upd", "bwd_big_dot"]


def load_library():
    """dlopen the in-tree HIP library.  Fails loudly if it has not been built: there is no
    Python/numpy stand-in for the product path."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise KKTError(f"{path} is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(path)
    vp, ip, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)
    lib.mi355x_kkt_default_options.argtypes = [C.POINTER(_Options)]
    lib.mi355x_kkt_default_options.restype = None
    lib.mi355x_kkt_create.argtypes = [C.POINTER(vp), C.POINTER(_Options)]
    lib.mi355x_kkt_destroy.argtypes = [vp]
    lib.mi355x_kkt_destroy.restype = None
    lib.mi355x_kkt_analyse.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_int, vp]
    lib.mi355x_kkt_values_buffer.argtypes = [vp]
    lib.mi355x_kkt_values_buffer.restype = dp
    lib.mi355x_kkt_factor.argtypes = [vp, vp, ip, ip]
    lib.mi355x_kkt_refactor.argtypes = [vp, ip, ip]
    lib.mi355x_kkt_solve.argtypes = [vp, C.c_int, vp, C.c_int]
    lib.mi355x_kkt_solve_device.argtypes = [vp, C.c_int, vp, C.c_int]
    lib.mi355x_kkt_solve_device2.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int]
    lib.mi355x_kkt_set_pivtol.argtypes = [vp, C.c_double]
    lib.mi355x_kkt_set_pivtolmax.argtypes = [vp, C.c_double]
    lib.mi355x_kkt_increase_quality.argtypes = [vp, dp]
    lib.mi355x_kkt_get_info.argtypes = [vp, C.POINTER(_Info)]
    lib.mi355x_kkt_last_error.argtypes = [vp]
    lib.mi355x_kkt_last_error.restype = C.c_char_p
    lib.mi355x_kkt_get_symbolic.argtypes = [vp, C.c_int, vp, C.c_int64]
    lib.mi355x_kkt_get_launch_plan.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, vp, C.c_int64, C.POINTER(C.c_int64)]
    lib.mi355x_kkt_profile.argtypes = [vp, C.c_int, vp, vp, C.c_int]
    lib.mi355x_kkt_factor_local.argtypes = [vp, vp]
    lib.mi355x_kkt_top_arena.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64)]
    lib.mi355x_kkt_factor_top.argtypes = [vp, ip, ip]
    lib.mi355x_kkt_solve_fwd_local.argtypes = [vp, vp]
    lib.mi355x_kkt_top_rhs.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64)]
    lib.mi355x_kkt_solve_top_and_bwd.argtypes = [vp, vp]
    lib.mi355x_kkt_comm_unique_id.argtypes = [vp]
    lib.mi355x_kkt_set_scaling.argtypes = [vp, C.c_int, vp]
    lib.mi355x_kkt_get_scaling.argtypes = [vp, vp]
    lib.mi355x_kkt_ruiz_scaling.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp]
    lib.mi355x_kkt_matching_scaling.argtypes = [C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, ip]
    lib.mi355x_kkt_zero_pivots.argtypes = [vp, vp, C.c_int, ip]
    lib.mi355x_kkt_failed_pivots.argtypes = [vp, vp, C.c_int, ip]
    lib.mi355x_kkt_delay_columns.argtypes = [vp, vp, C.c_int, ip]
    lib.mi355x_kkt_set_delay_rounds.argtypes = [vp, C.c_int]
    lib.mi355x_kkt_assembly_define.argtypes = [vp, C.c_int, vp, vp]
    lib.mi355x_kkt_assembly_buffer.argtypes = [vp, C.c_int]
    lib.mi355x_kkt_assembly_buffer.restype = dp
    lib.mi355x_kkt_assembly_upload.argtypes = [vp, C.c_int]
    lib.mi355x_kkt_factor_assembled.argtypes = [vp, vp, vp, ip, ip]
    lib.mi355x_kkt_pd_define.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int]
    lib.mi355x_kkt_pd_put_data.argtypes = [vp, vp]
    lib.mi355x_kkt_pd_put.argtypes = [vp, C.c_int, vp]
    lib.mi355x_kkt_pd_get.argtypes = [vp, C.c_int, vp]
    lib.mi355x_kkt_pd_solve_once.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double]
    lib.mi355x_kkt_pd_residual.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.mi355x_kkt_lowrank_set.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int]
    lib.mi355x_kkt_lowrank_update.argtypes = [vp, ip]
    lib.mi355x_kkt_lowrank_solve.argtypes = [vp, C.c_int, vp, C.c_int]
    lib.mi355x_kkt_lowrank_solve_device2.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int]
    lib.mi355x_kkt_set_solve_block.argtypes = [vp, C.c_int]
    lib.mi355x_kkt_solve_block_info.argtypes = [vp] + [C.POINTER(C.c_int)] * 6 + [C.POINTER(C.c_double)]
    lib.mi355x_kkt_lowrank_clear.argtypes = [vp]
    lib.mi355x_kkt_lowrank_info.argtypes = [vp, ip, ip, ip, ip, dp]
    lib.mi355x_kkt_lbfgs_define.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double]
    lib.mi355x_kkt_lbfgs_push.argtypes = [vp, vp, vp, ip]
    lib.mi355x_kkt_lbfgs_push_device.argtypes = [vp, vp, vp, ip]
    lib.mi355x_kkt_lbfgs_reset.argtypes = [vp]
    lib.mi355x_kkt_lbfgs_clear.argtypes = [vp]
    lib.mi355x_kkt_lbfgs_info.argtypes = [vp, ip, ip, ip, dp, ip, dp]
    lib.mi355x_kkt_lbfgs_get.argtypes = [vp, C.c_int, vp, C.c_int64]
    lib.mi355x_kkt_lbfgs_coefficients.argtypes = [C.c_int, vp, vp, vp, C.c_double, vp, vp]
    lib.mi355x_kkt_lbfgs_define_sr1.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_double]
    lib.mi355x_kkt_lbfgs_undo.argtypes = [vp, ip]
    lib.mi355x_kkt_lbfgs_sr1_info.argtypes = [vp, ip, ip, ip, vp, C.c_int]
    lib.mi355x_kkt_lbfgs_sr1_coefficients.argtypes = [C.c_int, vp, vp, vp, C.c_double, vp, vp, ip]
    lib.mi355x_kkt_lbfgs_define_resto.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, vp]
    lib.mi355x_kkt_lbfgs_push_resto.argtypes = [vp, vp, vp, C.c_double, ip]
    lib.mi355x_kkt_lbfgs_push_resto_device.argtypes = [vp, vp, vp, C.c_double, ip]
    lib.mi355x_kkt_lbfgs_resto_info.argtypes = [vp, ip, ip, dp]
    lib.mi355x_kkt_lowrank_rowmap.argtypes = [vp, C.c_int, vp]
    lib.mi355x_kkt_lowrank_rowmap_get.argtypes = [vp, ip, vp, C.c_int64]
    lib.mi355x_kkt_lowrank_rowmap_check.argtypes = [C.c_int64, C.c_int, vp, C.c_int64, C.c_char_p, C.c_int64]
    lib.mi355x_kkt_lbfgs_push_mapped.argtypes = [vp, vp, vp, C.c_int64, C.c_int, ip]
    lib.mi355x_kkt_lbfgs_push_resto_mapped.argtypes = [vp, vp, vp, C.c_int64, C.c_int, C.c_double, ip]
    lib.mi355x_kkt_qn_pair_check.argtypes = [C.c_int64, vp, vp, vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_char_p, C.c_int64]
    lib.mi355x_kkt_qn_pair_define.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int]
    lib.mi355x_kkt_qn_pair_store.argtypes = [vp, vp, vp, C.c_int]
    lib.mi355x_kkt_qn_pair_form.argtypes = [vp, vp, vp, vp, vp, C.c_int, dp]
    lib.mi355x_kkt_qn_pair_push.argtypes = [vp, C.c_double, ip]
    lib.mi355x_kkt_qn_pair_get.argtypes = [vp, C.c_int, vp, C.c_int64]
    lib.mi355x_kkt_qn_pair_info.argtypes = [vp, ip, ip, ip, ip, C.POINTER(C.c_int64), dp]
    lib.mi355x_kkt_qn_pair_clear.argtypes = [vp]
    lib.mi355x_kkt_set_comm_rccl.argtypes = [vp, vp]
    lib.mi355x_kkt_comm_shm_id.argtypes = [vp, C.c_int]
    lib.mi355x_kkt_set_comm_shm.argtypes = [vp, vp]
    lib.mi355x_kkt_set_comm_callbacks.argtypes = [vp, ALLREDUCE_FN, vp]
    lib.mi355x_kkt_set_comm_range_callback.argtypes = [vp, ALLREDUCE_RANGE_FN]
    lib.mi355x_kkt_exchange_bytes.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.mi355x_kkt_comm_plan.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, ip]
    lib.mi355x_kkt_comm_info.argtypes = [vp, ip, ip, ip, ip]
    _LIB = lib
    return lib


def lbfgs_coefficients(sts, L, D, sigma):
    """host only, no handle, no GPU: (status, C, Lbar) of include/mi355x_kkt.h's mi355x_kkt_lbfgs_coefficients; status SUCCESS or SINGULAR"""
    D = np.ascontiguousarray(D, dtype=np.float64); m = D.shape[0]
    sts = np.asfortranarray(sts, dtype=np.float64); L = np.asfortranarray(L, dtype=np.float64)
    if sts.shape != (m, m) or L.shape != (m, m):
        raise KKTError("lbfgs_coefficients: S^T S and L must be m x m, D of m")
    Cm = np.zeros((m, m), order="F"); Lbar = np.zeros((m, m), order="F")
    st = load_library().mi355x_kkt_lbfgs_coefficients(m, sts.ctypes.data, L.ctypes.data, D.ctypes.data, float(sigma), Cm.ctypes.data, Lbar.ctypes.data)
    if st == FATAL:
        raise KKTError("lbfgs_coefficients: m must be in [0, 32]")
    return st, Cm, Lbar


def lbfgs_sr1_coefficients(sts, L, D, sigma):
    """host only, no handle, no GPU: (status, E, Qs, nneg) of include/mi355x_kkt.h's mi355x_kkt_lbfgs_sr1_coefficients; status SUCCESS, or SINGULAR
    when the split rule says skip (then Qs is not scaled)"""
    D = np.ascontiguousarray(D, dtype=np.float64); m = D.shape[0]
    sts = np.asfortranarray(sts, dtype=np.float64); L = np.asfortranarray(L, dtype=np.float64)
    if sts.shape != (m, m) or L.shape != (m, m):
        raise KKTError("lbfgs_sr1_coefficients: S^T S and L must be m x m, D of m")
    E = np.zeros(m); Qs = np.zeros((m, m), order="F"); nneg = C.c_int(0)
    st = load_library().mi355x_kkt_lbfgs_sr1_coefficients(m, sts.ctypes.data, L.ctypes.data, D.ctypes.data, float(sigma), E.ctypes.data, Qs.ctypes.data, C.byref(nneg))
    if st == FATAL:
        raise KKTError("lbfgs_sr1_coefficients: m must be in [0, 32]" if not 0 <= m <= LBFGS_MAX else "lbfgs_sr1_coefficients: the eigen-solver did not converge")
    return st, E, Qs, nneg.value


def lowrank_rowmap_check(n, idx, length=-1):
    """host only, no handle, no GPU: (ok, reason) of include/mi355x_kkt.h's mi355x_kkt_lowrank_rowmap_check -- the validation every row map passes before the
    device is touched (0-based, strictly ascending, < n) and, with length >= 0, that a full-space vector of `length` entries covers the map"""
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    msg = C.create_string_buffer(512)
    st = load_library().mi355x_kkt_lowrank_rowmap_check(int(n), idx.size, idx.ctypes.data if idx.size else None, int(length), msg, 512)
    return st == 0, msg.value.decode()


def qn_pair_check(nnz, dims4, irn, jcn, off_jc, len_jc, off_jd, len_jd):
    """host only, no handle, no GPU: (ok, reason) of include/mi355x_kkt.h's mi355x_kkt_qn_pair_check -- the validation qn_pair_define performs on
    dims4 = (nx, ns, nc, nd), the 1-based triplets and the ranges [off, off + len) of the J_c and J_d segments in the triplet list"""
    d = np.ascontiguousarray(dims4, dtype=np.int32)
    if d.shape != (4,):
        raise KKTError("qn_pair_check: dims4 must hold nx, ns, nc, nd")
    r = np.ascontiguousarray(irn, dtype=np.int32); c = np.ascontiguousarray(jcn, dtype=np.int32)
    if r.ndim != 1 or r.shape != c.shape or r.size < int(nnz):
        raise KKTError("qn_pair_check: irn and jcn must be vectors of nnz entries")
    msg = C.create_string_buffer(512)
    st = load_library().mi355x_kkt_qn_pair_check(int(nnz), d.ctypes.data, r.ctypes.data if r.size else None, c.ctypes.data if c.size else None,
                                                 int(off_jc), int(len_jc), int(off_jd), int(len_jd), msg, 512)
    return st == 0, msg.value.decode()


class KKTSolver:
    """One solver instance == one ``mi355x_kkt_handle``."""

    def __init__(self, **opts):
        self.lib = load_library()
        o = _Options()
        self.lib.mi355x_kkt_default_options(C.byref(o))
        for k, v in opts.items():
            if not hasattr(o, k):
                raise KKTError(f"unknown option {k}")
            setattr(o, k, v)
        self._opts = o
        self._h = C.c_void_p()
        if self.lib.mi355x_kkt_create(C.byref(self._h), C.byref(o)) != 0:
            raise KKTError("mi355x_kkt_create failed")
        self._nnz = 0
        self._n = 0
        self._neg = 0
        self.pivtol = o.pivtol
        self.pivtolmax = o.pivtolmax

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.mi355x_kkt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self) -> str:
        return self.lib.mi355x_kkt_last_error(self._h).decode()

    # --- InitializeStructure (IpSparseSymLinearSolverInterface.hpp:139) ---
    def initialize_structure(self, n, row, col, fmt=FMT_TRIPLET, vals=None) -> int:
        row = np.ascontiguousarray(row, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        nnz = int(col.shape[0])
        v = None
        if vals is not None:
            v = np.ascontiguousarray(vals, dtype=np.float64)
            assert v.shape[0] == nnz
        st = self.lib.mi355x_kkt_analyse(self._h, int(n), nnz, row.ctypes.data, col.ctypes.data, int(fmt),
                                         v.ctypes.data if v is not None else None)
        if st != 0:
            raise KKTError("analyse: " + self.last_error())
        self._nnz, self._n = nnz, int(n)
        return st

    # --- GetValuesArrayPtr (hpp:155) ---
    def values(self) -> np.ndarray:
        p = self.lib.mi355x_kkt_values_buffer(self._h)
        if not p:
            raise KKTError("values_buffer: " + self.last_error())
        return np.ctypeslib.as_array(p, shape=(max(self._nnz, 1),))[: self._nnz]

    # --- MultiSolve (hpp:190) ---
    def multi_solve(self, new_matrix: bool, rhs: np.ndarray | None, check_neg_evals=False, number_of_neg_evals=0) -> int:
        if new_matrix or self._pending_refactor():
            neg, zero = C.c_int(0), C.c_int(0)
            if new_matrix:
                st = self.lib.mi355x_kkt_factor(self._h, None, C.byref(neg), C.byref(zero))
            else:
                st = self.lib.mi355x_kkt_refactor(self._h, C.byref(neg), C.byref(zero))
            self._refactor = False
            if st == FATAL:
                raise KKTError("factor: " + self.last_error())
            self._neg = neg.value
            if st == SINGULAR:
                return SINGULAR
            if check_neg_evals and self._neg != number_of_neg_evals:
                return WRONG_INERTIA
        if rhs is not None and rhs.size:
            assert rhs.dtype == np.float64 and rhs.flags.c_contiguous
            nrhs = 1 if rhs.ndim == 1 else rhs.shape[0]
            st = self.lib.mi355x_kkt_solve(self._h, nrhs, rhs.ctypes.data, self._n)
            if st != 0:
                raise KKTError("solve: " + self.last_error())
        return SUCCESS

    def factor_device(self, dvals_ptr: int):
        neg, zero = C.c_int(0), C.c_int(0)
        st = self.lib.mi355x_kkt_factor(self._h, C.c_void_p(dvals_ptr), C.byref(neg), C.byref(zero))
        if st == FATAL:
            raise KKTError("factor: " + self.last_error())
        self._neg = neg.value
        return st, neg.value, zero.value

    def solve_device(self, drhs_ptr: int, nrhs=1):
        st = self.lib.mi355x_kkt_solve_device(self._h, nrhs, C.c_void_p(drhs_ptr), self._n)
        if st != 0:
            raise KKTError("solve_device: " + self.last_error())

    def solve_device2(self, db_ptr: int, dx_ptr: int, nrhs=1):
        st = self.lib.mi355x_kkt_solve_device2(self._h, nrhs, C.c_void_p(db_ptr), self._n, C.c_void_p(dx_ptr), self._n)
        if st != 0:
            raise KKTError("solve_device2: " + self.last_error())

    # --- device-side value assembly: segments  values[off + i] = scale * src[i] + shift ---
    def assembly_define(self, lengths):
        ln = np.asarray(lengths, dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int64)
        if self.lib.mi355x_kkt_assembly_define(self._h, len(ln), off.ctypes.data, ln.ctypes.data) != 0:
            raise KKTError("assembly_define: " + self.last_error())
        self._seg_len = ln
        self._qn_dims = self._qn_segs = None      # (a new assembly ends a qn_pair definition)

    def assembly_set(self, seg, values):
        p = self.lib.mi355x_kkt_assembly_buffer(self._h, int(seg))
        n = int(self._seg_len[seg])
        if n:
            np.ctypeslib.as_array(p, shape=(n,))[:] = values
        if self.lib.mi355x_kkt_assembly_upload(self._h, int(seg)) != 0:
            raise KKTError("assembly_upload: " + self.last_error())

    def factor_assembled(self, scale, shift):
        sc = np.ascontiguousarray(scale, dtype=np.float64); sh = np.ascontiguousarray(shift, dtype=np.float64)
        neg, zero = C.c_int(0), C.c_int(0)
        st = self.lib.mi355x_kkt_factor_assembled(self._h, sc.ctypes.data, sh.ctypes.data, C.byref(neg), C.byref(zero))
        if st == FATAL:
            raise KKTError("factor_assembled: " + self.last_error())
        self._neg = neg.value
        return st, neg.value, zero.value

    # --- the 8-block primal-dual system on the device: vectors are lists of 8 arrays x|s|y_c|y_d|z_L|z_U|v_L|v_U ---
    def pd_define(self, dims8, idx_xl, idx_xu, idx_sl, idx_su, irn, jcn, segs):
        d = np.ascontiguousarray(dims8, dtype=np.int32)
        ix = [np.ascontiguousarray(a, dtype=np.int32) for a in (idx_xl, idx_xu, idx_sl, idx_su)]
        r = np.ascontiguousarray(irn, dtype=np.int32); c = np.ascontiguousarray(jcn, dtype=np.int32); sg = np.ascontiguousarray(segs, dtype=np.int32)
        if self.lib.mi355x_kkt_pd_define(self._h, d.ctypes.data, ix[0].ctypes.data, ix[1].ctypes.data, ix[2].ctypes.data, ix[3].ctypes.data,
                                         r.ctypes.data, c.ctypes.data, sg.ctypes.data, len(sg)) != 0:
            raise KKTError("pd_define: " + self.last_error())
        self._pd_len = [int(v) for v in d]

    @staticmethod
    def _ptr_array(arrs):
        keep = [np.ascontiguousarray(a, dtype=np.float64) for a in arrs]
        return (C.c_void_p * 8)(*[a.ctypes.data if a.size else None for a in keep]), keep

    def pd_put_data(self, data8):
        pa, keep = self._ptr_array(data8)
        if self.lib.mi355x_kkt_pd_put_data(self._h, pa) != 0:
            raise KKTError("pd_put_data: " + self.last_error())

    def pd_put(self, vec, blocks8):
        pa, keep = self._ptr_array(blocks8)
        if self.lib.mi355x_kkt_pd_put(self._h, int(vec), pa) != 0:
            raise KKTError("pd_put: " + self.last_error())

    def pd_get(self, vec):
        out = [np.zeros(n) for n in self._pd_len]
        pa = (C.c_void_p * 8)(*[a.ctypes.data if a.size else None for a in out])
        if self.lib.mi355x_kkt_pd_get(self._h, int(vec), pa) != 0:
            raise KKTError("pd_get: " + self.last_error())
        return out

    def pd_solve_once(self, rhs, res, alpha=1.0, beta=0.0):
        if self.lib.mi355x_kkt_pd_solve_once(self._h, int(rhs), int(res), float(alpha), float(beta)) != 0:
            raise KKTError("pd_solve_once: " + self.last_error())

    def pd_residual(self, rhs, res, resid, deltas4):
        d = np.ascontiguousarray(deltas4, dtype=np.float64); nr = np.zeros(3)
        if self.lib.mi355x_kkt_pd_residual(self._h, int(rhs), int(res), int(resid), d.ctypes.data, nr.ctypes.data) != 0:
            raise KKTError("pd_residual: " + self.last_error())
        return nr

    # --- low-rank update of the factored system, K + V V^T - U U^T (include/mi355x_kkt.h; reference IpLowRankAugSystemSolver.cpp) ---
    def lowrank_set(self, V, U, rows=None):
        """V (rows x nv) and U (rows x nu), numpy, acting on the first `rows` indices, or on those of the row map (lowrank_rowmap); None or zero columns = that half is absent"""
        def prep(A):
            if A is None:
                return None
            A = np.asarray(A, dtype=np.float64)
            return np.asfortranarray(A.reshape(-1, 1) if A.ndim == 1 else A)
        Vf, Uf = prep(V), prep(U)
        if rows is None:
            rows = Vf.shape[0] if Vf is not None else (Uf.shape[0] if Uf is not None else 0)
        for A in (Vf, Uf):
            if A is not None and A.shape[0] != rows:
                raise KKTError("lowrank_set: V and U must have `rows` rows")
        nv = 0 if Vf is None else Vf.shape[1]; nu = 0 if Uf is None else Uf.shape[1]
        st = self.lib.mi355x_kkt_lowrank_set(self._h, int(rows), nv, Vf.ctypes.data if nv and rows else None, max(int(rows), 1),
                                             nu, Uf.ctypes.data if nu and rows else None, max(int(rows), 1))
        if st != 0:
            raise KKTError("lowrank_set: " + self.last_error())

    def lowrank_update(self):
        """after a factorisation: (status, which) -- (SUCCESS, 0), or (WRONG_INERTIA, 1 | 2) when M1 | M2 is not positive definite"""
        which = C.c_int(0)
        st = self.lib.mi355x_kkt_lowrank_update(self._h, C.byref(which))
        if st == FATAL:
            raise KKTError("lowrank_update: " + self.last_error())
        return st, which.value

    def lowrank_solve(self, rhs: np.ndarray):
        """in place, like multi_solve's right-hand side: one vector of n, or (nrhs, n) C-contiguous"""
        assert rhs.dtype == np.float64 and rhs.flags.c_contiguous
        nrhs = 1 if rhs.ndim == 1 else rhs.shape[0]
        if self.lib.mi355x_kkt_lowrank_solve(self._h, nrhs, rhs.ctypes.data, self._n) != 0:
            raise KKTError("lowrank_solve: " + self.last_error())

    def lowrank_solve_device2(self, db_ptr: int, dx_ptr: int, nrhs=1, ldb=None, ldx=None):
        st = self.lib.mi355x_kkt_lowrank_solve_device2(self._h, nrhs, C.c_void_p(db_ptr), self._n if ldb is None else int(ldb),
                                                       C.c_void_p(dx_ptr), self._n if ldx is None else int(ldx))
        if st != 0:
            raise KKTError("lowrank_solve_device2: " + self.last_error())

    def lowrank_clear(self):
        if self.lib.mi355x_kkt_lowrank_clear(self._h) != 0:
            raise KKTError("lowrank_clear: " + self.last_error())

    def lowrank_info(self) -> dict:
        r, v, u, c, ms = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0.0)
        if self.lib.mi355x_kkt_lowrank_info(self._h, C.byref(r), C.byref(v), C.byref(u), C.byref(c), C.byref(ms)) != 0:
            raise KKTError("lowrank_info: " + self.last_error())
        return {"rows": r.value, "nv": v.value, "nu": u.value, "current": bool(c.value), "update_ms": ms.value}

    # --- blocks of right-hand sides in the solves (include/mi355x_kkt.h mi355x_kkt_set_solve_block): opt-in, single-GPU handles ---
    def set_solve_block(self, on) -> None:
        """on: solve calls with nrhs >= 2 take their right-hand sides through the tree SOLVE_BLOCK at a time (same bits per column as a solve of its own)."""
        if self.lib.mi355x_kkt_set_solve_block(self._h, 1 if on else 0) != 0:
            raise KKTError("set_solve_block: " + self.last_error())

    def solve_block_info(self) -> dict:
        o, w, lv, nb, nc, nt, ms = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0.0)
        if self.lib.mi355x_kkt_solve_block_info(self._h, C.byref(o), C.byref(w), C.byref(lv), C.byref(nb), C.byref(nc), C.byref(nt), C.byref(ms)) != 0:
            raise KKTError("solve_block_info: " + self.last_error())
        return {"on": bool(o.value), "width": w.value, "first_top_level": lv.value, "blocked_launches": nb.value, "bycol_launches": nc.value,
                "top_launches_per_column": nt.value, "last_ms": ms.value}

    # --- the row map (the reference's P_LowRank): row i of V, U, S, Y, DR is the caller's index idx[i] ---
    def lowrank_rowmap(self, idx):
        """idx: 0-based, strictly ascending indices below n (ExpansionMatrix::ExpandedPosIndices), or None / empty to remove the map; refused while an update
        is set or a history defined.  While it is set, lowrank_set and the lbfgs_define* calls take len(idx) rows."""
        if idx is None:
            st = self.lib.mi355x_kkt_lowrank_rowmap(self._h, 0, None)
        else:
            a = np.asarray(idx)
            if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)) or (a.size and (a.min() < -2**31 or a.max() >= 2**31)):
                raise KKTError("lowrank_rowmap: idx must be a vector of int32 indices")
            a = np.ascontiguousarray(a, dtype=np.int32)
            st = self.lib.mi355x_kkt_lowrank_rowmap(self._h, a.size, a.ctypes.data if a.size else None)
        if st != 0:
            raise KKTError("lowrank_rowmap: " + self.last_error())

    def lowrank_rowmap_info(self):
        """None when no map is set, else the indices (int32)"""
        r = C.c_int(0)
        if self.lib.mi355x_kkt_lowrank_rowmap_get(self._h, C.byref(r), None, 0) != 0:
            raise KKTError("lowrank_rowmap_info: " + self.last_error())
        if r.value == 0:
            return None
        out = np.zeros(r.value, dtype=np.int32)
        if self.lib.mi355x_kkt_lowrank_rowmap_get(self._h, C.byref(r), out.ctypes.data, out.size) != 0:
            raise KKTError("lowrank_rowmap_info: " + self.last_error())
        return out

    # --- limited-memory BFGS: the (s, y) history on the device, V and U formed there (include/mi355x_kkt.h; reference IpLimMemQuasiNewtonUpdater.cpp) ---
    def lbfgs_define(self, rows, max_history=6, init="scalar1", init_val=1.0, sigma_min=1e-8, sigma_max=1e8):
        """init: a name of LBFGS_INIT or its number"""
        st = self.lib.mi355x_kkt_lbfgs_define(self._h, int(rows), int(max_history), LBFGS_INIT.get(init, init), init_val, sigma_min, sigma_max)
        if st != 0:
            raise KKTError("lbfgs_define: " + self.last_error())

    def lbfgs_push(self, s: np.ndarray, y: np.ndarray) -> int:
        """host vectors of `rows`; -> outcome: LBFGS_STORED (V, U installed as the low-rank update), LBFGS_SKIPPED, LBFGS_NOT_POSDEF"""
        rows = self.lbfgs_info()["rows"]
        s = np.ascontiguousarray(s, dtype=np.float64); y = np.ascontiguousarray(y, dtype=np.float64)
        if rows and (s.shape != (rows,) or y.shape != (rows,)):      # (rows = 0: nothing is defined, which the library says itself)
            raise KKTError("lbfgs_push: s and y must be vectors of `rows`")
        oc = C.c_int(0)
        if self.lib.mi355x_kkt_lbfgs_push(self._h, s.ctypes.data, y.ctypes.data, C.byref(oc)) != 0:
            raise KKTError("lbfgs_push: " + self.last_error())
        return oc.value

    def lbfgs_push_device(self, ds_ptr: int, dy_ptr: int) -> int:
        """device vectors of `rows`, complete before the call"""
        oc = C.c_int(0)
        if self.lib.mi355x_kkt_lbfgs_push_device(self._h, C.c_void_p(ds_ptr), C.c_void_p(dy_ptr), C.byref(oc)) != 0:
            raise KKTError("lbfgs_push_device: " + self.last_error())
        return oc.value

    def lbfgs_reset(self):
        if self.lib.mi355x_kkt_lbfgs_reset(self._h) != 0:
            raise KKTError("lbfgs_reset: " + self.last_error())

    def lbfgs_clear(self):
        if self.lib.mi355x_kkt_lbfgs_clear(self._h) != 0:
            raise KKTError("lbfgs_clear: " + self.last_error())

    def lbfgs_info(self) -> dict:
        r, mh, m, sk, sg, ms = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0.0), C.c_double(0.0)
        if self.lib.mi355x_kkt_lbfgs_info(self._h, C.byref(r), C.byref(mh), C.byref(m), C.byref(sg), C.byref(sk), C.byref(ms)) != 0:
            raise KKTError("lbfgs_info: " + self.last_error())
        return {"rows": r.value, "max_history": mh.value, "memory": m.value, "sigma": sg.value, "skipped_in_a_row": sk.value, "push_ms": ms.value}

    def lbfgs_get(self, what) -> np.ndarray:
        """what: "S" | "Y" (rows x memory, oldest first), "V" | "U" (the installed columns), "D" (memory), "L" | "STS" (memory x memory), or 0..6;
        a restoration-phase history: "Y" | "Ypart" is Ypart, and "G" | "R" (memory x memory), "eta_col" | "dv" (memory), "DR" (rows), or 10..14"""
        w = {"S": 0, "Y": 1, "Ypart": 1, "V": 2, "U": 3, "D": 4, "L": 5, "STS": 6, "G": 10, "R": 11, "eta_col": 12, "dv": 13, "DR": 14}.get(what, what)
        I = self.lbfgs_info(); m = I["memory"]
        if w in (2, 3):
            lr = self.lowrank_info()
            shape = (lr["rows"], lr["nv"] if w == 2 else lr["nu"])
        else:
            shape = (I["rows"], m) if w in (0, 1) else (m,) if w in (4, 12, 13) else (I["rows"],) if w == 14 else (m, m)
        out = np.zeros(shape, dtype=np.float64, order="F")
        if self.lib.mi355x_kkt_lbfgs_get(self._h, int(w), out.ctypes.data if out.size else None, out.size) != 0:
            raise KKTError("lbfgs_get: " + self.last_error())
        return out

    # --- limited-memory SR1: the same history and calls; V (memory - nneg columns), U (nneg) from the eigen-split of Z; one push can be taken back ---
    def lbfgs_define_sr1(self, rows, max_history=6, init="scalar1", init_val=1.0):
        """init: a name of LBFGS_INIT or its number; sigma is not clipped"""
        st = self.lib.mi355x_kkt_lbfgs_define_sr1(self._h, int(rows), int(max_history), LBFGS_INIT.get(init, init), init_val)
        if st != 0:
            raise KKTError("lbfgs_define_sr1: " + self.last_error())

    def lbfgs_undo(self) -> int:
        """takes the last stored push of an SR1 history back; -> 1, or 0 when there is nothing to undo"""
        u = C.c_int(0)
        if self.lib.mi355x_kkt_lbfgs_undo(self._h, C.byref(u)) != 0:
            raise KKTError("lbfgs_undo: " + self.last_error())
        return u.value

    def lbfgs_sr1_info(self) -> dict:
        """type LBFGS_BFGS | LBFGS_SR1, nneg, can_undo, E: the `memory` eigenvalues of the installed split, ascending (empty for a BFGS history)"""
        t, nn, cu = C.c_int(0), C.c_int(0), C.c_int(0)
        E = np.zeros(LBFGS_MAX)
        if self.lib.mi355x_kkt_lbfgs_sr1_info(self._h, C.byref(t), C.byref(nn), C.byref(cu), E.ctypes.data, LBFGS_MAX) != 0:
            raise KKTError("lbfgs_sr1_info: " + self.last_error())
        m = self.lbfgs_info()["memory"] if t.value == LBFGS_SR1 else 0
        return {"type": t.value, "nneg": nn.value, "can_undo": bool(cu.value), "E": E[:m].copy()}

    # --- the restoration phase: Ypart in the history, eta per push, the fixed scaling DR; B0 = sigma I, or eta DR when special ---
    def lbfgs_define_resto(self, rows, dr, max_history=6, type=LBFGS_BFGS, special=False, init="scalar1", init_val=1.0, sigma_min=1e-8, sigma_max=1e8):
        """dr: host vector of `rows` positive entries; type LBFGS_BFGS | LBFGS_SR1; special: B0 = eta dr (sigma stays -1)"""
        rows = int(rows)
        dr = None if dr is None else np.ascontiguousarray(dr, dtype=np.float64)
        if dr is not None and dr.shape != (rows,):
            raise KKTError("lbfgs_define_resto: dr must be a vector of `rows`")
        st = self.lib.mi355x_kkt_lbfgs_define_resto(self._h, rows, int(max_history), int(type), int(special), LBFGS_INIT.get(init, init), init_val, sigma_min, sigma_max,
                                                    None if dr is None else dr.ctypes.data)
        if st != 0:
            raise KKTError("lbfgs_define_resto: " + self.last_error())

    def lbfgs_push_resto(self, s: np.ndarray, ypart: np.ndarray, eta: float) -> int:
        """host vectors of `rows`, eta > 0; -> outcome as lbfgs_push"""
        rows = self.lbfgs_info()["rows"]
        s = np.ascontiguousarray(s, dtype=np.float64); ypart = np.ascontiguousarray(ypart, dtype=np.float64)
        if rows and (s.shape != (rows,) or ypart.shape != (rows,)):
            raise KKTError("lbfgs_push_resto: s and ypart must be vectors of `rows`")
        oc = C.c_int(0)
        if self.lib.mi355x_kkt_lbfgs_push_resto(self._h, s.ctypes.data, ypart.ctypes.data, float(eta), C.byref(oc)) != 0:
            raise KKTError("lbfgs_push_resto: " + self.last_error())
        return oc.value

    def lbfgs_push_resto_device(self, ds_ptr: int, dypart_ptr: int, eta: float) -> int:
        """device vectors of `rows`, complete before the call"""
        oc = C.c_int(0)
        if self.lib.mi355x_kkt_lbfgs_push_resto_device(self._h, C.c_void_p(ds_ptr), C.c_void_p(dypart_ptr), float(eta), C.byref(oc)) != 0:
            raise KKTError("lbfgs_push_resto_device: " + self.last_error())
        return oc.value

    # --- pushes of full-space (x-block) vectors under a row map: gathered on the device, then the plain push (IpLimMemQuasiNewtonUpdater.cpp:323-324) ---
    def lbfgs_push_mapped(self, sx: np.ndarray, yx: np.ndarray) -> int:
        """host x-block vectors of equal length > idx[rows-1]; -> outcome as lbfgs_push of (sx[idx], yx[idx]), bit for bit"""
        sx = np.ascontiguousarray(sx, dtype=np.float64); yx = np.ascontiguousarray(yx, dtype=np.float64)
        if sx.ndim != 1 or sx.shape != yx.shape:
            raise KKTError("lbfgs_push_mapped: sx and yx must be vectors of one length")
        return self._push_mapped("lbfgs_push_mapped", sx.ctypes.data, yx.ctypes.data, sx.size, 0, None)

    def lbfgs_push_resto_mapped(self, sx: np.ndarray, ypartx: np.ndarray, eta: float) -> int:
        """host x-block vectors of equal length > idx[rows-1], eta > 0; -> outcome as lbfgs_push_resto of the gathered vectors"""
        sx = np.ascontiguousarray(sx, dtype=np.float64); ypartx = np.ascontiguousarray(ypartx, dtype=np.float64)
        if sx.ndim != 1 or sx.shape != ypartx.shape:
            raise KKTError("lbfgs_push_resto_mapped: sx and ypartx must be vectors of one length")
        return self._push_mapped("lbfgs_push_resto_mapped", sx.ctypes.data, ypartx.ctypes.data, sx.size, 0, eta)

    def lbfgs_push_mapped_device(self, dsx_ptr: int, dyx_ptr: int, length: int) -> int:
        """device x-block vectors of `length` entries, complete before the call"""
        return self._push_mapped("lbfgs_push_mapped", C.c_void_p(dsx_ptr), C.c_void_p(dyx_ptr), length, 1, None)

    def lbfgs_push_resto_mapped_device(self, dsx_ptr: int, dypartx_ptr: int, length: int, eta: float) -> int:
        """device x-block vectors of `length` entries, complete before the call"""
        return self._push_mapped("lbfgs_push_resto_mapped", C.c_void_p(dsx_ptr), C.c_void_p(dypartx_ptr), length, 1, eta)

    def _push_mapped(self, name, ps, py, length, on_device, eta):
        oc = C.c_int(0)
        if eta is None:
            st = self.lib.mi355x_kkt_lbfgs_push_mapped(self._h, ps, py, int(length), on_device, C.byref(oc))
        else:
            st = self.lib.mi355x_kkt_lbfgs_push_resto_mapped(self._h, ps, py, int(length), on_device, float(eta), C.byref(oc))
        if st != 0:
            raise KKTError(name + ": " + self.last_error())
        return oc.value

    def lbfgs_resto_info(self) -> dict:
        """resto: a restoration-phase history is defined; special; eta of its last stored push (-1 before the first)"""
        r, sp, eta = C.c_int(0), C.c_int(0), C.c_double(0.0)
        if self.lib.mi355x_kkt_lbfgs_resto_info(self._h, C.byref(r), C.byref(sp), C.byref(eta)) != 0:
            raise KKTError("lbfgs_resto_info: " + self.last_error())
        return {"resto": bool(r.value), "special": bool(sp.value), "eta": eta.value}

    # --- the quasi-Newton pair (s, y) formed on the device from the resident Jacobians (include/mi355x_kkt.h; reference IpLimMemQuasiNewtonUpdater.cpp:276-308) ---
    def qn_pair_define(self, dims4, irn, jcn, seg_jc, seg_jd):
        """dims4 = (nx, ns, nc, nd); irn, jcn: the 1-based triplets of initialize_structure; seg_jc, seg_jd: the assembly segments of J_c, J_d (negative: absent)"""
        d = np.ascontiguousarray(dims4, dtype=np.int32)
        if d.shape != (4,):
            raise KKTError("qn_pair_define: dims4 must hold nx, ns, nc, nd")
        r = np.ascontiguousarray(irn, dtype=np.int32); c = np.ascontiguousarray(jcn, dtype=np.int32)
        if r.shape != (self._nnz,) or c.shape != (self._nnz,):
            raise KKTError("qn_pair_define: irn and jcn must be the nnz triplets of initialize_structure")
        if self.lib.mi355x_kkt_qn_pair_define(self._h, d.ctypes.data, r.ctypes.data if r.size else None, c.ctypes.data if c.size else None, int(seg_jc), int(seg_jd)) != 0:
            raise KKTError("qn_pair_define: " + self.last_error())
        self._qn_dims = [int(v) for v in d]
        self._qn_segs = tuple(int(self._seg_len[q]) if q >= 0 else 0 for q in (int(seg_jc), int(seg_jd)))

    def _qn_vec(self, name, v, k):
        if v is None:
            return None
        v = np.ascontiguousarray(v, dtype=np.float64)
        if k is not None and v.shape != (k,):      # (k None: nothing is defined, which the library says itself)
            raise KKTError(f"{name} must be a vector of {k}")
        return v

    def _qn_len(self):
        return getattr(self, "_qn_dims", None) or [None, None, None, None]

    def qn_pair_store(self, x=None, grad_f=None):
        """x, grad_f: host vectors of nx; grad_f None: the restoration variant; x None: roll (the vectors of the last qn_pair_form become the snapshot's)"""
        nx = self._qn_len()[0]
        x = self._qn_vec("qn_pair_store: x", x, nx); grad_f = self._qn_vec("qn_pair_store: grad_f", grad_f, nx)
        if self.lib.mi355x_kkt_qn_pair_store(self._h, None if x is None else x.ctypes.data, None if grad_f is None else grad_f.ctypes.data, 0) != 0:
            raise KKTError("qn_pair_store: " + self.last_error())

    def qn_pair_store_device(self, dx_ptr, dgf_ptr=None):
        """device vectors of nx, complete before the call; dgf_ptr None / 0: the restoration variant"""
        if self.lib.mi355x_kkt_qn_pair_store(self._h, C.c_void_p(dx_ptr), C.c_void_p(dgf_ptr) if dgf_ptr else None, 1) != 0:
            raise KKTError("qn_pair_store: " + self.last_error())

    def qn_pair_form(self, x, grad_f, y_c, y_d, amax=True):
        """host vectors of nx, nx, nc, nd (grad_f None: the restoration variant; y_c / y_d may be None or empty for an absent block); -> max |s| (over the
        row map's indices when one is set), or None with amax=False (then nothing is downloaded)"""
        nx, _, nc, nd = self._qn_len()
        x = self._qn_vec("qn_pair_form: x", x, nx); grad_f = self._qn_vec("qn_pair_form: grad_f", grad_f, nx)
        y_c = self._qn_vec("qn_pair_form: y_c", y_c if nc else None, nc); y_d = self._qn_vec("qn_pair_form: y_d", y_d if nd else None, nd)
        p = lambda v: None if v is None else v.ctypes.data      # (a vector of 0 entries still has an address: grad_f of nx = 0 is not "absent")
        a = C.c_double(0.0)
        if self.lib.mi355x_kkt_qn_pair_form(self._h, p(x), p(grad_f), p(y_c), p(y_d), 0, C.byref(a) if amax else None) != 0:
            raise KKTError("qn_pair_form: " + self.last_error())
        return a.value if amax else None

    def qn_pair_form_device(self, dx_ptr, dgf_ptr, dyc_ptr, dyd_ptr, amax=True):
        """device vectors, complete before the call and free again when it returns; a pointer None / 0: absent"""
        q = lambda v: C.c_void_p(v) if v else None
        a = C.c_double(0.0)
        if self.lib.mi355x_kkt_qn_pair_form(self._h, q(dx_ptr), q(dgf_ptr), q(dyc_ptr), q(dyd_ptr), 1, C.byref(a) if amax else None) != 0:
            raise KKTError("qn_pair_form: " + self.last_error())
        return a.value if amax else None

    def qn_pair_push(self, eta=0.0) -> int:
        """the formed device vectors into the defined history (eta: a restoration-phase history only); -> outcome as lbfgs_push"""
        oc = C.c_int(0)
        if self.lib.mi355x_kkt_qn_pair_push(self._h, float(eta), C.byref(oc)) != 0:
            raise KKTError("qn_pair_push: " + self.last_error())
        return oc.value

    def qn_pair_get(self, what) -> np.ndarray:
        """what: "s" | "y" | "x_last" | "grad_f_last" | "Jc_last" | "Jd_last", or 0..5"""
        w = {"s": 0, "y": 1, "x_last": 2, "grad_f_last": 3, "Jc_last": 4, "Jd_last": 5}.get(what, what)
        I = self.qn_pair_info()
        out = np.zeros(I["nx"] if w <= 3 else I["len_jc"] if w == 4 else I["len_jd"])
        if self.lib.mi355x_kkt_qn_pair_get(self._h, int(w), out.ctypes.data if out.size else None, out.size) != 0:
            raise KKTError("qn_pair_get: " + self.last_error())
        return out

    def qn_pair_info(self) -> dict:
        """defined, stored, formed, nx, nnz_j (entries of the column view), form_ms; and from the launch report: lpc (lanes per column of the kernel),
        max_column (its longest column); len_jc, len_jd as qn_pair_define saw the segments"""
        d, st, f, nx, nz, ms = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0), C.c_double(0.0)
        if self.lib.mi355x_kkt_qn_pair_info(self._h, C.byref(d), C.byref(st), C.byref(f), C.byref(nx), C.byref(nz), C.byref(ms)) != 0:
            raise KKTError("qn_pair_info: " + self.last_error())
        plan = self.launch_plan("qn_pair")
        out = {"defined": bool(d.value), "stored": bool(st.value), "formed": bool(f.value), "nx": nx.value, "nnz_j": nz.value, "form_ms": ms.value,
               "lpc": int(plan[1]), "max_column": int(plan[2]), "len_jc": 0, "len_jd": 0}
        if d.value and getattr(self, "_qn_segs", None) is not None:
            out["len_jc"], out["len_jd"] = self._qn_segs
        return out

    def qn_pair_clear(self):
        if self.lib.mi355x_kkt_qn_pair_clear(self._h) != 0:
            raise KKTError("qn_pair_clear: " + self.last_error())
        self._qn_dims = self._qn_segs = None

    # --- multi-GPU communicator (include/mi355x_kkt.h): after one of these, multi_solve / factor_device / solve_device* of a
    #     handle created with nranks > 1 run the distributed sequence inside the library ---
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        if load_library().mi355x_kkt_comm_unique_id(buf) != 0:
            raise KKTError("comm_unique_id: librccl.so not loadable / ncclGetUniqueId failed")
        return buf.raw

    def set_comm_rccl(self, unique_id: bytes):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        if self.lib.mi355x_kkt_set_comm_rccl(self._h, buf) != 0:
            raise KKTError("set_comm_rccl: " + self.last_error())

    @staticmethod
    def comm_shm_id(nranks: int) -> bytes:
        """rank 0: create the shared-memory segment of a host-staged communicator for ranks of one node (they may share a device)"""
        buf = C.create_string_buffer(128)
        if load_library().mi355x_kkt_comm_shm_id(buf, int(nranks)) != 0:
            raise KKTError("comm_shm_id: shm_open / mmap failed")
        return buf.raw

    def set_comm_shm(self, shm_id: bytes):
        buf = C.create_string_buffer(bytes(shm_id), 128)
        if self.lib.mi355x_kkt_set_comm_shm(self._h, buf) != 0:
            raise KKTError("set_comm_shm: " + self.last_error())

    def set_comm_callback(self, fn, fn_range=None):
        """fn(dptr: int, count: int, dtype: int (0 fp64, 1 int32), hip_stream: int) -> None; must leave the buffer summed over the ranks.
        fn_range(dptr, count, dtype, hip_stream, rank_lo, nranks_in_range) (optional): the same over a range of ranks only"""
        def _wrap(f):
            def _cb(ctx, *a):
                try:
                    f(*[int(x or 0) for x in a])
                    return 0
                except Exception:          # never let an exception cross the C ABI
                    import traceback; traceback.print_exc()
                    return 1
            return _cb
        self._comm_cb = ALLREDUCE_FN(_wrap(fn))       # keep the thunks alive as long as the handle
        if self.lib.mi355x_kkt_set_comm_callbacks(self._h, self._comm_cb, None) != 0:
            raise KKTError("set_comm_callbacks: " + self.last_error())
        if fn_range is not None:
            self._comm_range_cb = ALLREDUCE_RANGE_FN(_wrap(fn_range))
            if self.lib.mi355x_kkt_set_comm_range_callback(self._h, self._comm_range_cb) != 0:
                raise KKTError("set_comm_range_callback: " + self.last_error())

    def exchange_bytes(self):
        """(bytes of all arena squares, bytes of all top right-hand sides) of the current multi-GPU structure"""
        a, t = C.c_int64(0), C.c_int64(0)
        if self.lib.mi355x_kkt_exchange_bytes(self._h, C.byref(a), C.byref(t)) != 0:
            raise KKTError("exchange_bytes: no device-side set-up")
        return a.value, t.value

    def comm_plan(self, rank, range_local=True):
        """host only: the collectives rank `rank` issues for one factorisation + one solve (and the ncclCommSplit calls before them) as an (k, 6) int array
        {what, step, colour, range size, count, dtype} -- include/mi355x_kkt.h mi355x_kkt_comm_plan.  Needs the analysis, not a device."""
        cnt = C.c_int(0)
        if self.lib.mi355x_kkt_comm_plan(self._h, int(rank), int(bool(range_local)), None, 0, C.byref(cnt)) != 0:
            raise KKTError("comm_plan: " + self.last_error())
        out = np.zeros((max(cnt.value, 1), 6), dtype=np.int32)
        if self.lib.mi355x_kkt_comm_plan(self._h, int(rank), int(bool(range_local)), out.ctypes.data, cnt.value, C.byref(cnt)) != 0:
            raise KKTError("comm_plan: " + self.last_error())
        return out[:cnt.value]

    def comm_info(self):
        """{kind: 0 none / 1 callbacks / 2 rccl, ranks_seen (ncclCommCount), range_local, exchange_steps} of the communicator in use"""
        k, r, l, e = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        if self.lib.mi355x_kkt_comm_info(self._h, C.byref(k), C.byref(r), C.byref(l), C.byref(e)) != 0:
            raise KKTError("comm_info: " + self.last_error())
        return {"kind": ("none", "callbacks", "rccl")[k.value], "ranks_seen": r.value, "range_local": bool(l.value), "exchange_steps": e.value}

    _refactor = False

    def _pending_refactor(self):
        return self._refactor

    def number_of_neg_evals(self) -> int:
        return self._neg

    # --- IncreaseQuality (hpp:220): u <- min(umax, u^0.75), as MA97/SPRAL/MA27 adapters do; False when u is at its
    #     maximum OR the last factorisation found no pivot decision that depends on u (nothing a refactorisation could change) ---
    def increase_quality(self) -> bool:
        u = C.c_double(0.0)
        if self.lib.mi355x_kkt_increase_quality(self._h, C.byref(u)) == 0:
            return False
        self.pivtol = u.value
        self._refactor = True
        return True

    def set_pivtol(self, u: float):
        if self.lib.mi355x_kkt_set_pivtol(self._h, float(u)) != 0:
            raise KKTError("set_pivtol: " + self.last_error())
        self.pivtol = float(u)

    @staticmethod
    def provides_inertia() -> bool:
        return True

    def set_scaling(self, mode: int, factors=None):
        f = None if factors is None else np.ascontiguousarray(factors, dtype=np.float64)
        if self.lib.mi355x_kkt_set_scaling(self._h, int(mode), f.ctypes.data if f is not None else None) != 0:
            raise KKTError("set_scaling: " + self.last_error())

    def get_scaling(self) -> np.ndarray:
        out = np.zeros(max(self._n, 1))
        if self.lib.mi355x_kkt_get_scaling(self._h, out.ctypes.data) != 0:
            raise KKTError("get_scaling: " + self.last_error())
        return out[: self._n]

    # --- DetermineDependentRows support (hpp:240-255): columns with a zero pivot in the last factorisation (caller's index base) ---
    def zero_pivots(self) -> np.ndarray:
        cnt = C.c_int(0)
        if self.lib.mi355x_kkt_zero_pivots(self._h, None, 0, C.byref(cnt)) != 0:
            raise KKTError("zero_pivots: " + self.last_error())
        out = np.zeros(max(cnt.value, 1), dtype=np.int32)
        self.lib.mi355x_kkt_zero_pivots(self._h, out.ctypes.data, cnt.value, C.byref(cnt))
        return out[:cnt.value]

    # --- delayed pivoting across fronts (include/mi355x_kkt.h): what the last factorisation had to force, and the structural edit ---
    def failed_pivots(self) -> np.ndarray:
        cnt = C.c_int(0)
        if self.lib.mi355x_kkt_failed_pivots(self._h, None, 0, C.byref(cnt)) != 0:
            raise KKTError("failed_pivots: " + self.last_error())
        out = np.zeros(max(cnt.value, 1), dtype=np.int32)
        self.lib.mi355x_kkt_failed_pivots(self._h, out.ctypes.data, cnt.value, C.byref(cnt))
        return out[:cnt.value]

    def delay_columns(self, cols) -> int:
        """move the columns (caller's index base) to their parent fronts; returns how many moved"""
        c = np.ascontiguousarray(cols, dtype=np.int32)
        moved = C.c_int(0)
        if self.lib.mi355x_kkt_delay_columns(self._h, c.ctypes.data, int(c.shape[0]), C.byref(moved)) != 0:
            raise KKTError("delay_columns: " + self.last_error())
        return moved.value

    def set_delay_rounds(self, rounds: int):
        if self.lib.mi355x_kkt_set_delay_rounds(self._h, int(rounds)) != 0:
            raise KKTError("set_delay_rounds: rounds >= 0")

    def info(self) -> KKTInfo:
        i = _Info()
        self.lib.mi355x_kkt_get_info(self._h, C.byref(i))
        return KKTInfo(**{f: getattr(i, f) for f in KKTInfo.__dataclass_fields__})

    def profile(self, reps=1) -> dict:
        """{kernel kind: (total device ms over reps, launches over reps)} from hip events around every launch."""
        ms = np.zeros(len(KERNEL_KINDS)); ln = np.zeros(len(KERNEL_KINDS), dtype=np.int32)
        if self.lib.mi355x_kkt_profile(self._h, int(reps), ms.ctypes.data, ln.ctypes.data, len(KERNEL_KINDS)) != 0:
            raise KKTError("profile: " + self.last_error())
        return {k: (float(ms[i]), int(ln[i])) for i, k in enumerate(KERNEL_KINDS)}

    def launch_plan(self, what: str, nranks: int = 1, rank: int = 0) -> np.ndarray:
        """host only: array `what` of the launch plan rank `rank` of `nranks` would run (include/mi355x_kkt.h mi355x_kkt_get_launch_plan)."""
        cnt = C.c_int64(0)
        if self.lib.mi355x_kkt_get_launch_plan(self._h, int(nranks), int(rank), what.encode(), None, 0, C.byref(cnt)) != 0:
            raise KKTError("get_launch_plan: " + self.last_error())
        out = np.zeros(max(cnt.value, 1), dtype=np.int32)
        if self.lib.mi355x_kkt_get_launch_plan(self._h, int(nranks), int(rank), what.encode(), out.ctypes.data, out.shape[0], C.byref(cnt)) != 0:
            raise KKTError("get_launch_plan: " + self.last_error())
        return out[:cnt.value]

    def symbolic(self, what: int, size: int) -> np.ndarray:
        out = np.empty(max(size, 1), dtype=np.int32)
        if self.lib.mi355x_kkt_get_symbolic(self._h, what, out.ctypes.data, out.shape[0]) != 0:
            raise KKTError("get_symbolic: " + self.last_error())
        return out[:size]
