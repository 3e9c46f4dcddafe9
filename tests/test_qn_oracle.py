"""The quasi-Newton specifications against what the UNMODIFIED reference did: tests/golden/*.qnrec (oracle/ref_driver --record-qn,
tests/golden/make_golden.sh; reader oracle/qn_oracle.py) hold, per UpdateHessian call of a reference run with `hessian_approximation
limited-memory`, the pair (s, y) its updater formed and the W = sigma I + V V^T - U U^T it left behind, and per Solve of its low-rank
augmented-system solver what that was given and returned.  The recorded pairs are replayed through tests/support/lbfgs_spec.py /
sr1_spec.py in float64 and in longdouble; the test plays the caller and applies the rules include/mi355x_kkt.h leaves to it, as the
reference applies them (IpLimMemQuasiNewtonUpdater.cpp:226-274, :350-357, :523-532, :674-691):
  * |s|_max < 100 eps: the pair is not pushed, a skip;
  * `max_skipping` skips in a row: the next call resets the history and takes no pair (mark Wr);
  * SR1, info_regu_x > 0: undo before the push (mark Wb) -- and that call adds one to the skip counter whether its push is stored or
    not, where a stored push otherwise zeroes it.  The handle's own skipped_in_a_row does not follow that rule (an undo followed by a
    stored push leaves 0), which is why the counter is the caller's here.

Bound (the rule of tests/test_gpu_lbfgs.py, widened for conditioning): e = max|A - A_ld| / max|A_ld|, e_ref <= 64 max(e_64, 2^-52)
max(1, kappa / 5), kappa = cond_2(M) (BFGS) or emax / emin of Z (SR1) of the longdouble specification of that record.

Measured per fixture: worst e_ref / (max(e_64, 2^-52) max(1, kappa / 5)) (allowed: 64); records that needed the kappa factor, i.e. had
e_ref > 64 max(e_64, 2^-52); largest kappa of the run; worst e_ref / max(e_64, 2^-52) without the factor:
    qn_bfgs_180   1.00   0 of 15   5.6e11 (the last records before convergence)   2.6
    qn_bfgs_517   1.00   0 of 11   5.9e4                                          2.0
    qn_bfgs_1728  4.04   0 of  9   2.3e2                                          4.0
    qn_sr1_180    1.00   3 of 22   9.7e10                                         4135 (records 7, 13, 14: kappa 1e6, the reference's LAPACK
                                                                                  eigen-solver against the Jacobi rule of the specification)
    qn_sr1_517    1.00   0 of 12   1.1e4                                          2.5
The device (tests/test_gpu_qn_replay.py, e_dev in the place of e_ref): 1.75, 0.24, 1.32, 1.00, 0.68 with the factor, and 3.7, 2.4, 1.3, 8.1,
1.4 without it: the device never needed it.
No difference between the specifications and the reference was found in what the recordings reach.  They reach no Cholesky failure of M
(outcome 2) and no |s|_max skip (mark WS).
"""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import qn_oracle as qn
from tests.support import lbfgs_spec as lb
from tests.support import lowrank_spec as lr
from tests.support import pathfix
from tests.support import sr1_spec as sr

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["qn_bfgs_180", "qn_bfgs_517", "qn_bfgs_1728", "qn_sr1_180", "qn_sr1_517"]
FIX_TOL = 1e-7                                       # tests/test_gpu_lowrank.py
EPS = np.finfo(np.float64).eps
STORED, SKIPPED, RESET, FIRST = "stored", "skipped", "reset", "first"


@functools.lru_cache(maxsize=None)
def fixture(name):
    header, updates, solves = qn.read_qnrec(os.path.join(GOLDEN, name + ".qnrec"))
    for r in updates + solves:
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return header, updates, solves


def recorded_outcome(rec):
    """what the reference did on this call, from the recording alone"""
    if not rec["has_pair"]:
        return FIRST
    if "Wr" in rec["info"]:
        return RESET
    return STORED if rec["w_changed"] and "Ws" not in rec["info"] else SKIPPED


def new_history(header, dtype):
    if header["update_type"] == "bfgs":
        return lb.History(header["nx"], header["max_history"], header["initialization"], header["init_val"], header["sigma_min"], header["sigma_max"], dtype=dtype)
    return sr.History(header["nx"], header["max_history"], header["initialization"], header["init_val"], dtype=dtype)


class Caller:
    """the caller's side of a history: the three rules of the module docstring around push / undo / reset of `hist` (a specification History, or
    anything with push(s, y) -> outcome, undo(), reset())"""

    def __init__(self, header, hist):
        self.sr1 = header["update_type"] == "sr1"
        self.max_skipping = header["max_skipping"]
        self.h = hist
        self.skipped = 0

    def step(self, rec):
        if not rec["has_pair"]:
            return FIRST
        if self.skipped >= self.max_skipping:
            self.h.reset(); self.skipped = 0
            return RESET
        if rec["amax_s"] < 100.0 * EPS:
            self.skipped += 1
            return SKIPPED
        retro = self.sr1 and rec["regu_x"] > 0.0
        if retro:
            self.h.undo()
        stored = self.h.push(rec["s"], rec["y"]) == lb.STORED      # (lb.NOT_POSDEF: the reference marks Ws and counts a skip, :489-495, :687-691)
        self.skipped = self.skipped + 1 if (retro or not stored) else 0
        return STORED if stored else SKIPPED


def dev(A, Ald):
    return float(np.abs(A - Ald).max() / np.abs(Ald).max())


def kappa_of(header, Hld):
    """cond_2(M) of the BFGS history / emax / emin of the SR1 history's Z, from the longdouble specification (1 for an empty history)"""
    if Hld.memory == 0:
        return 1.0
    if header["update_type"] == "bfgs":
        d = 1 / np.sqrt(Hld.D)
        Lt = np.tril(Hld.L, -1) * d[None, :]
        M = Lt @ Lt.T + Hld.sigma * Hld.STS
        return float(np.linalg.cond(M.astype(np.float64)))
    _, emin, emax = sr.split(Hld.E)
    return float(emax / emin)


def bound(e_64, kappa):
    return 64.0 * max(e_64, 2.0 ** -52) * max(1.0, kappa / 5.0)


def installed(H):
    """(sigma, V, U) a caller would hand to the solver: the installed columns (none: zero columns)"""
    z = np.zeros((H.rows, 0), dtype=H.dt)
    return H.sigma, (z if H.V is None else H.V), (z if H.U is None else H.U)


def comparisons(header, got, H64, Hld):
    """[(name, A, A_64, A_ld)] for one record: got = (sigma, V, U) of the recording (or of the device), against the two specifications"""
    sg, V, U = got
    s64, V64, U64 = installed(H64)
    sld, Vld, Uld = installed(Hld)
    out = [("sigma", np.array([sg]), np.array([s64]), np.array([sld]))]
    if header["update_type"] == "bfgs":
        for name, A, A64, Ald in (("V", V, V64, Vld), ("U", U, U64, Uld)):
            assert A.shape == Ald.shape == A64.shape, name
            out += [(f"{name}[:, {j}]", A[:, j], A64[:, j], Ald[:, j]) for j in range(A.shape[1])]
    else:
        assert U.shape == Uld.shape and V.shape == Vld.shape, "nv / nu"
        if Hld.memory:
            Brec, B64, Bld = lb.dense(V, U, sg), lb.dense(V64, U64, s64), lb.dense(Vld, Uld, sld)
            Brc, _ = sr.recursive_sr1(Hld.S, Hld.Y, Hld.sigma)
            out += [("sigma I + V V^T - U U^T", Brec, B64, Bld), ("the same against recursive SR1", Brec, B64, Brc), ("specification against recursive SR1", Bld, B64, Brc)]
    return out


def replay(name, got_of, hist=None, after=None, label="e_ref"):
    """replays fixture `name`; got_of(i, rec) -> (sigma, V, U) to hold against the specifications; hist: a third history pushed alongside (the device);
    after(i, rec, outcome, H64, Hld): further checks per record; label: what the printed deviation of `got_of` is called (e_ref: the recording, e_dev: the device).  -> (worst ratio to the kappa-scaled bound's 1/64, records that would miss the bound without its kappa factor)"""
    header, updates, _ = fixture(name)
    H64, Hld = new_history(header, np.float64), new_history(header, np.longdouble)
    callers = [Caller(header, H64), Caller(header, Hld)] + ([Caller(header, hist)] if hist is not None else [])
    worst, needed = 0.0, 0
    for i, rec in enumerate(updates):
        want = recorded_outcome(rec)
        outs = [c.step(rec) for c in callers]
        assert all(o == want for o in outs), (name, i, rec["info"], want, outs)
        assert ("Wb" in rec["info"]) == (header["update_type"] == "sr1" and rec["regu_x"] > 0.0 and want != RESET), (name, i)
        assert Hld.memory == H64.memory
        kappa = kappa_of(header, Hld)
        over = False
        for what, A, A64, Ald in comparisons(header, got_of(i, rec), H64, Hld):
            e_ref, e_64 = dev(A, Ald), dev(A64, Ald)
            ratio = e_ref / (max(e_64, 2.0 ** -52) * max(1.0, kappa / 5.0))
            worst = max(worst, ratio)
            print(f"{name} record {i} ({want}, memory {Hld.memory}): {what}: {label} {e_ref:.2e} e_64 {e_64:.2e} kappa {kappa:.2e} ratio {ratio:.2f}")
            over |= e_ref > bound(e_64, 1.0)
            assert e_ref <= bound(e_64, kappa), (name, i, what, e_ref, e_64, kappa)
        needed += over
        if after is not None:
            after(i, rec, want, H64, Hld)
    print(f"{name}: worst ratio {worst:.2f} (allowed 64), {needed} of {len(updates)} records needed the kappa factor")
    return worst, needed


@pytest.mark.parametrize("name", FIXTURES)
def test_the_specification_reproduces_the_recorded_updates(name):
    header, updates, _ = fixture(name)
    nx = header["nx"]

    def got_of(i, rec):
        assert np.all(rec["diag"] == rec["diag"][0]) and rec["diag"].shape == (nx,)
        return rec["diag"][0], rec["V"], rec["U"]

    def after(i, rec, want, H64, Hld):
        _, Vld, Uld = installed(Hld)
        assert (rec["nv"], rec["nu"]) == (Vld.shape[1], Uld.shape[1])
        if header["update_type"] == "bfgs":
            assert rec["nv"] == rec["nu"] == (Hld.memory if want != RESET else 0)
        else:
            assert rec["nv"] + rec["nu"] == Hld.memory and rec["nu"] == Hld.nneg
        if want == SKIPPED:                                                  # the reference leaves IpData().W() alone
            prev = updates[i - 1]
            assert all(np.array_equal(rec[k], prev[k]) for k in ("diag", "V", "U"))
        if want in (FIRST, RESET):
            assert rec["nv"] == rec["nu"] == 0 and rec["diag"][0] == header["init_val"]

    replay(name, got_of, after=after)


def test_the_fixtures_hold_the_cases_they_were_chosen_for():
    shift = skipped = sr1_nu = sr1_both = False
    for name in FIXTURES:
        header, updates, solves = fixture(name)
        outs = [recorded_outcome(r) for r in updates]
        assert outs[0] == FIRST and not updates[0]["has_pair"] and STORED in outs
        skipped |= any(o == SKIPPED and "Ws" in r["info"] for o, r in zip(outs, updates))
        if header["update_type"] == "bfgs":
            full = [i for i, r in enumerate(updates) if r["nv"] == header["max_history"]]
            shift |= any(outs[i] == STORED and i - 1 in full for i in full)      # stored while the memory was already full
        else:
            sr1_nu |= any(r["nu"] > 0 for r in updates)
            sr1_both |= any(r["nu"] > 0 and r["nv"] > 0 for r in updates)
        used = [r for r in solves if r["status"] == qn.SUCCESS]
        assert used, name
    assert shift and skipped and sr1_nu and sr1_both
    assert any(r["nv"] > 0 and r["nu"] > 0 and r["status"] == qn.SUCCESS for n in FIXTURES for r in fixture(n)[2])


@functools.lru_cache(maxsize=None)
def solve_reference(name, k):
    """(dense updated matrix, x_hp) of solve record k: computed once, shared with the device test, never written"""
    rec = fixture(name)[2][k]
    Kt = qn.dense_updated(rec)
    ref, _ = pathfix.refined_solve(sp.csc_matrix(Kt), rec["rhs"][None, :])
    Kt.setflags(write=False); ref.setflags(write=False)
    return Kt, ref[0]


def used_solves(name):
    return [k for k, r in enumerate(fixture(name)[2]) if r["status"] == qn.SUCCESS]


@pytest.mark.parametrize("name", FIXTURES)
def test_the_recorded_solves_and_the_low_rank_specification_agree_with_a_refined_dense_solve(name):
    for k, rec in enumerate(fixture(name)[2]):
        if k in used_solves(name):
            continue
        # the reference answered "wrong inertia" (the only other answer in the fixtures): the specification must refuse the system too, by K's inertia or by M1 / M2
        assert rec["status"] == 2 and rec["check_neg"]
        K = qn.aug_matrix(rec)[4].toarray()
        assert lr.num_neg(K) != rec["num_neg"] or lr.update(K, np.sqrt(rec["W_factor"]) * rec["V"], np.sqrt(rec["W_factor"]) * rec["U"])["which"] != 0
    for k in used_solves(name):
        rec = fixture(name)[2][k]
        Kt, x_hp = solve_reference(name, k)
        tol = FIX_TOL * max(1.0, np.abs(x_hp).max())
        e_ref = np.abs(rec["sol"] - x_hp).max()
        K = qn.aug_matrix(rec)[4].toarray()
        f = np.sqrt(rec["W_factor"])
        V, U = f * rec["V"], f * rec["U"]
        upd = lr.update(K, V, U)
        assert upd["which"] == 0
        e_spec = np.abs(lr.solve(K, V, U, upd, rec["rhs"]) - x_hp).max()
        print(f"{name} solve {k} (iteration {rec['iter']}, nv {rec['nv']}, nu {rec['nu']}): |x_ref - x_hp| {e_ref:.2e}, |x_spec - x_hp| {e_spec:.2e}, allowed {tol:.2e}")
        assert e_ref <= tol and e_spec <= tol
        if rec["check_neg"]:
            assert rec["neg_after"] == rec["num_neg"] == rec["nc"] + rec["nd"]
