"""-m gpu: the recorded quasi-Newton updates and low-rank solves of the reference (tests/golden/*.qnrec, see tests/test_qn_oracle.py) through
the device: the (s, y) pairs the reference's updater formed -- skipped pairs, clipped sigma, steps shrinking towards convergence, ill-conditioned M
and Z -- are pushed into a history on a handle of rows = nx with the recorded options and the caller rules of tests/test_qn_oracle.py (Caller);
after every record the handle must say what the reference did (outcome, memory, nu), hold the stored pairs bitwise, and sigma, V, U (BFGS) or
sigma I + V V^T - U U^T (SR1) must agree with the longdouble specification under that module's bound, e_dev in the place of e_ref, and with the
recording under the same bound (max|A_dev - A_rec| / max|A_ld| in the place of e_ref).  qn_bfgs_517 is pushed through lbfgs_push_device, the
others through the host entry point.  Measured, worst ratio of the device against the recording to that bound's 1/64 (64 allowed): qn_bfgs_180
0.75, qn_bfgs_517 1.12, qn_bfgs_1728 2.72, qn_sr1_180 1.73, qn_sr1_517 0.80.

Every recorded solve that returned success goes through analyse -> factor (recorded inertia required where the reference required it) ->
lowrank_set (recorded V, U times sqrt(W_factor)) -> lowrank_update -> lowrank_solve: scaled residual <= RES_TOL against the dense updated matrix,
solution within FIX_TOL of the refined dense solve (tests/test_gpu_lowrank.py's tolerances).  A recorded solve the reference answered "wrong
inertia" must be refused by the factorisation's inertia or by lowrank_update.  On qn_bfgs_180 the chain also runs with the columns the pushes
installed: push -> factor with the handle's sigma -> lowrank_update -> lowrank_solve, as a product would run it."""
import numpy as np
import pytest
import torch      # (before the library is loaded: see tests/test_gpu_parity.py)

import ipopt_amd
from ipopt_amd import kkt
from oracle import qn_oracle as qn
from tests.test_gpu_lowrank import sres, RES_TOL, FIX_TOL
from tests.test_qn_oracle import (FIXTURES, RESET, bound, comparisons, dev, fixture, kappa_of, replay, solve_reference, used_solves)

pytestmark = pytest.mark.gpu
DEVICE_PUSH = {"qn_bfgs_517"}


def analysed(name):
    """a handle analysed on the 4-block structure of the fixture's solve records -> (solver, triplet rows, cols)"""
    n, r, c, v, _ = qn.aug_matrix(fixture(name)[2][0])
    s = ipopt_amd.KKTSolver()
    s.initialize_structure(n, r, c, vals=v)
    return s, r, c


def set_values(s, r, c, rec, diag=None):
    """the values of solve record `rec` into the handle (diag: another W diagonal than the recorded one)"""
    if diag is not None:
        rec = dict(rec, diag=diag)
    _, r2, c2, v2, _ = qn.aug_matrix(rec)
    assert np.array_equal(r2, r) and np.array_equal(c2, c)
    s.values()[:] = v2


def chain(s, rec, Kt, x_hp, what):
    """lowrank_update -> lowrank_solve on a factored handle with columns set, checked against the dense updated matrix Kt and x_hp"""
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    assert s.lowrank_info()["current"]
    x = rec["rhs"].copy()
    s.lowrank_solve(x)
    res, err = sres(Kt, x, rec["rhs"]), np.abs(x - x_hp).max()
    print(f"{what}: scaled residual {res:.2e}, |x - x_hp| {err:.2e} (|x_hp| {np.abs(x_hp).max():.2e})")
    assert res <= RES_TOL
    assert err <= FIX_TOL * max(1.0, np.abs(x_hp).max())


class DeviceHistory:
    """push / undo / reset of the handle's history, for tests.test_qn_oracle.Caller"""

    def __init__(self, s, on_device):
        self.s, self.on_device = s, on_device

    def push(self, sv, yv):
        if not self.on_device:
            return self.s.lbfgs_push(sv, yv)
        ds = torch.tensor(sv, dtype=torch.float64, device="cuda"); dy = torch.tensor(yv, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        return self.s.lbfgs_push_device(ds.data_ptr(), dy.data_ptr())

    def undo(self):
        return self.s.lbfgs_undo()

    def reset(self):
        self.s.lbfgs_reset()


def installed_on(s, nx):
    """(sigma, V, U) installed on the handle; no update installed: zero columns"""
    lri = s.lowrank_info()
    z = np.zeros((nx, 0))
    return s.lbfgs_info()["sigma"], (s.lbfgs_get("V") if lri["nv"] else z), (s.lbfgs_get("U") if lri["nu"] else z)


@pytest.mark.parametrize("name", FIXTURES)
def test_the_device_history_reproduces_the_recorded_updates(name):
    header, updates, solves = fixture(name)
    nx, sr1 = header["nx"], header["update_type"] == "sr1"
    s, r, c = analysed(name)
    if sr1:
        s.lbfgs_define_sr1(nx, header["max_history"], header["initialization"], header["init_val"])
    else:
        s.lbfgs_define(nx, header["max_history"], header["initialization"], header["init_val"], header["sigma_min"], header["sigma_max"])
    got, chains = {}, []

    def got_of(i, rec):
        got[i] = installed_on(s, nx)
        return got[i]

    def after(i, rec, want, H64, Hld):
        info, lri = s.lbfgs_info(), s.lowrank_info()
        assert info["memory"] == Hld.memory
        assert (lri["nv"], lri["nu"]) == (rec["nv"], rec["nu"])
        if sr1:
            assert s.lbfgs_sr1_info()["nneg"] == (rec["nu"] if want != RESET else 0)
        assert np.array_equal(s.lbfgs_get("S"), H64.S) and np.array_equal(s.lbfgs_get("Y"), H64.Y)      # bitwise the stored pairs, oldest first
        kappa = kappa_of(header, Hld)
        recorded = (rec["diag"][0], rec["V"], rec["U"])
        for (what, A, A64, Ald), (_, Arec, _, _) in zip(comparisons(header, got[i], H64, Hld), comparisons(header, recorded, H64, Hld)):
            e, e_64 = float(np.abs(A - Arec).max() / np.abs(Ald).max()), dev(A64, Ald)
            print(f"{name} record {i}: {what}: device against the recording {e:.2e} e_64 {e_64:.2e} kappa {kappa:.2e} ratio {e / (max(e_64, 2.0 ** -52) * max(1.0, kappa / 5.0)):.2f}")
            assert e <= bound(e_64, kappa), (name, i, what, e, e_64, kappa)
        if name == "qn_bfgs_180":                                                                         # push -> factor -> update -> solve
            for k in used_solves(name):
                srec = solves[k]
                if srec["iter"] != rec["iter"] or not lri["nv"]:
                    continue
                sg, V, U = got[i]
                set_values(s, r, c, srec, diag=np.full(nx, sg))
                assert s.multi_solve(True, None, srec["check_neg"], srec["num_neg"]) == kkt.SUCCESS
                Kt = qn.aug_matrix(dict(srec, diag=np.full(nx, sg)))[4].toarray()
                Kt[:nx, :nx] += V @ V.T - U @ U.T
                chain(s, srec, Kt, solve_reference(name, k)[1], f"{name} solve {k} with the pushed columns (memory {info['memory']})")
                chains.append(k)

    replay(name, got_of, hist=DeviceHistory(s, name in DEVICE_PUSH), after=after, label="e_dev")
    if name == "qn_bfgs_180":                                                                             # every used solve with columns ran the chain, once
        assert chains == [k for k in used_solves(name) if solves[k]["nv"] > 0] and chains
    s.lbfgs_clear()


@pytest.mark.parametrize("name", FIXTURES)
def test_the_recorded_solves_through_factor_update_and_solve(name):
    header, _, solves = fixture(name)
    nx = header["nx"]
    s, r, c = analysed(name)
    used = used_solves(name)
    for k, rec in enumerate(solves):
        f = np.sqrt(rec["W_factor"])
        set_values(s, r, c, rec)
        st = s.multi_solve(True, None, rec["check_neg"], rec["num_neg"])
        if k not in used:
            assert rec["status"] == kkt.WRONG_INERTIA and rec["check_neg"]                                # (ESymSolverStatus and the library's codes agree on 0 and 2)
            if st == kkt.SUCCESS:
                s.lowrank_set(f * rec["V"], f * rec["U"], rows=nx)
                st = s.lowrank_update()[0]
            # (the device pivots on its own: a failure here is a finding to read against the recorded system, not noise)
            print(f"{name} solve {k}: the reference said wrong inertia, the device says {st}")
            assert st == kkt.WRONG_INERTIA
            continue
        assert st == kkt.SUCCESS
        s.lowrank_set(f * rec["V"], f * rec["U"], rows=nx)
        Kt, x_hp = solve_reference(name, k)
        chain(s, rec, Kt, x_hp, f"{name} solve {k} (iteration {rec['iter']}, nv {rec['nv']}, nu {rec['nu']})")
