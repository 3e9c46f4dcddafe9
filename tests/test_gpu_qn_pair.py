"""-m gpu: the quasi-Newton pair (s, y) formed on the device from the resident Jacobians (mi355x_kkt_qn_pair_*; reference
IpLimMemQuasiNewtonUpdater.cpp:276-308) against tests/support/qn_pair_spec.py.  The systems are built as tests/test_gpu_pd_system.py builds them, segments
W | D_x | D_s | J_c | D_c | J_d | -I | D_d.  What is asserted of a formed pair (check): s bitwise x - x_last; |y - pair_ld| <= bound -- the derived bound
(k_j + 4) 2^-52 (|gf_j| + |gf_last_j| + sum (|J_cur| + |J_last|) |lam|) that tests/test_qn_pair_spec.py shows the REFERENCE's own order to satisfy on these very
inputs -- and exactly 0 where the bound is 0; amax_s bitwise max |s|; the instantiation of k_qn_pair that ran (get_launch_plan "qn_pair") is the one the
structure asks for.  Every device call's status is checked (the Python methods raise on any status but success); nothing is retried."""
import ctypes as C

import numpy as np
import pytest
import torch      # (before the library is loaded: see tests/test_gpu_parity.py)

import ipopt_amd
from ipopt_amd import kkt
from tests.support import qn_pair_spec as qp
from tests.test_gpu_lowrank import sres, RES_TOL

pytestmark = pytest.mark.gpu
SCALE = np.array([1, 1, 1, 1, 0, 1, 0, 0], dtype=float)
DELTA = 1e-2


def handle(c, define=True, **opts):
    """a handle analysed on the system of case c, the assembly defined, J_last in the J segments, W = 0, D_x = D_s = 1"""
    n, irn, jcn, lens = qp.system(c)
    s = ipopt_amd.KKTSolver(**opts)
    s.initialize_structure(n, irn, jcn, vals=np.ones(len(irn)))
    s.assembly_define(lens)
    for q, v in enumerate([np.zeros(lens[0]), np.ones(lens[1]), np.ones(lens[2]), c["Jc_last"], np.zeros(lens[4]), c["Jd_last"], np.zeros(lens[6]), np.zeros(lens[7])]):
        s.assembly_set(q, v)
    if define:
        s.qn_pair_define([c["nx"], c["ns"], c["nc"], c["nd"]], irn, jcn, qp.SEG_JC, qp.SEG_JD)
    return s


def set_j(s, jc, jd):
    s.assembly_set(qp.SEG_JC, jc); s.assembly_set(qp.SEG_JD, jd)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check(s, c, resto, stored=False, idx=None):
    """store (unless stored) -> the current Jacobians -> form, against the specification; -> (s, y)"""
    if not stored:
        set_j(s, c["Jc_last"], c["Jd_last"])
        s.qn_pair_store(c["x_last"], None if resto else c["gf_last"])
    set_j(s, c["Jc_cur"], c["Jd_cur"])
    amax = s.qn_pair_form(c["x"], None if resto else c["gf"], c["yc"], c["yd"])
    I = s.qn_pair_info()
    assert I["defined"] and I["stored"] and I["formed"] and I["nx"] == c["nx"] and I["nnz_j"] == len(c["jc"][0]) + len(c["jd"][0])
    sv, yv = s.qn_pair_get("s"), s.qn_pair_get("y")
    _, y_ld = qp.pair_ld(c, resto)
    b = qp.bound(c, resto)
    err = np.abs(yv.astype(np.longdouble) - y_ld).astype(float)
    ratio = float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    print(f"{c['name']} resto {resto}: lpc {I['lpc']}, longest column {I['max_column']}, device / bound {ratio:.3f}")
    assert np.array_equal(bits(sv), bits(c["x"] - c["x_last"]))
    assert np.all(err <= b), (c["name"], ratio)
    assert np.all(yv[b == 0] == 0.0)
    want = np.abs(sv if idx is None else sv[idx]).max()
    assert bits(amax) == bits(want), (amax, want)
    assert I["lpc"] == qp.expected_lpc(c) and I["max_column"] == int(qp.column_lengths(c).max(initial=0))
    return sv, yv


def test_shapes_at_which_the_kernel_can_go_wrong():
    """nx 1, 63, 64, 65, 257; columns of 0, 1, 64, 65, 257 and 300 entries; nc = 0 and nd = 0 alone; duplicate triplets; J_c in upper orientation;
    multipliers with zeros and both signs (tests/test_qn_pair_spec.py asserts these properties of the inputs) -- plain and restoration variant on one
    handle each; every instantiation of the kernel must have run"""
    reached = set()
    for c in qp.SHAPES():
        s = handle(c)
        check(s, c, False)
        check(s, c, True)
        reached.add(s.qn_pair_info()["lpc"])
        s.qn_pair_clear()
        assert not s.qn_pair_info()["defined"]
        s.close()
    assert reached == {1, 8, 64}


@pytest.mark.parametrize("which", range(len(qp.RECORDED)), ids=[f"{n}:{a}->{b}" for n, a, b in qp.RECORDED])
def test_recorded_structures(which):
    """The J_c / J_d triplets of the solve records of two consecutive iterations of the reference (tests/golden/*.qnrec) as J_last and J_cur; qn_bfgs_517
    has a J_d only.  The recordings hold neither grad_f nor the multipliers, so the recorded y itself cannot be re-formed: x, grad_f and the multipliers
    are seeded random, the checks are those of the synthetic shapes."""
    c = qp.recorded_case(*qp.RECORDED[which])
    s = handle(c)
    check(s, c, False)
    check(s, c, True)


def test_the_snapshot_is_a_copy():
    c = next(x for x in qp.SHAPES() if x["name"] == "nx64")
    s = handle(c, scaling=0)
    _, y0 = check(s, c, False)                                                       # store, THEN assembly_set with the new J, then form: against the old J
    assert np.array_equal(bits(s.qn_pair_get("Jc_last")), bits(c["Jc_last"])) and np.array_equal(bits(s.qn_pair_get("Jd_last")), bits(c["Jd_last"]))
    # a second store with the same x and grad_f (the sources now hold J_cur), then form: nothing moved
    s.qn_pair_store(c["x"], c["gf"])
    assert s.qn_pair_form(c["x"], c["gf"], c["yc"], c["yd"]) == 0.0
    assert not s.qn_pair_get("s").any() and not s.qn_pair_get("y").any()
    # a factorisation between store and form, with a non-unit scale on the J segments: the sources, not the assembled values, are read
    set_j(s, c["Jc_last"], c["Jd_last"])
    s.qn_pair_store(c["x_last"], c["gf_last"])
    set_j(s, c["Jc_cur"], c["Jd_cur"])
    scale = SCALE.copy(); scale[qp.SEG_JC] = 0.5; scale[qp.SEG_JD] = 0.25
    st, neg, _ = s.factor_assembled(scale, np.array([0, 0, 0, 0, -DELTA, 0, -1, -DELTA], dtype=float))
    assert st == kkt.SUCCESS and neg == c["nc"] + c["nd"]
    _, y1 = check(s, c, False, stored=True)
    assert np.array_equal(bits(y1), bits(y0))


def test_roll():
    c = next(x for x in qp.SHAPES() if x["name"] == "nx65")
    a, b = handle(c), handle(c)
    check(a, c, False)
    a.qn_pair_store()                                                                # roll: the vectors of the form, the sources as they are now
    Ia = a.qn_pair_info()
    assert Ia["stored"] and not Ia["formed"]
    set_j(b, c["Jc_cur"], c["Jd_cur"])
    b.qn_pair_store(c["x"], c["gf"])
    for what in ("x_last", "grad_f_last", "Jc_last", "Jd_last"):
        assert np.array_equal(bits(a.qn_pair_get(what)), bits(b.qn_pair_get(what))), what
    assert np.array_equal(bits(a.qn_pair_get("x_last")), bits(c["x"])) and np.array_equal(bits(a.qn_pair_get("Jc_last")), bits(c["Jc_cur"]))
    # ... and the rolled snapshot serves the next form
    rng = np.random.default_rng(3)
    c2 = dict(c, x_last=c["x"], gf_last=c["gf"], Jc_last=c["Jc_cur"], Jd_last=c["Jd_cur"], x=c["x"] + 1e-3 * rng.standard_normal(c["nx"]), gf=c["gf"] + rng.standard_normal(c["nx"]),
              Jc_cur=c["Jc_cur"] + 0.1 * rng.standard_normal(len(c["Jc_cur"])), Jd_cur=c["Jd_cur"] * 1.5)
    check(a, c2, False, stored=True)
    with pytest.raises(ipopt_amd.KKTError, match="roll"):
        b.qn_pair_store()                                                            # nothing formed on b


def test_restoration_equals_the_plain_variant_with_zero_gradients():
    c = next(x for x in qp.SHAPES() if x["name"] == "columns")
    s = handle(c)
    z = dict(c, gf=np.zeros(c["nx"]), gf_last=np.zeros(c["nx"]))
    _, y_p = check(s, z, False)
    assert not s.qn_pair_get("grad_f_last").any()
    _, y_r = check(s, c, True)
    assert np.array_equal(bits(y_r), bits(y_p))
    with pytest.raises(ipopt_amd.KKTError, match="restoration"):
        s.qn_pair_get("grad_f_last")                                                 # a snapshot stored without grad_f has none to hand out


def iterates(c, k, seed):
    """k + 1 iterates on the structure of c with positive curvature along the steps: (x, gf, Jc, Jd) each, and small multipliers"""
    rng = np.random.default_rng(seed)
    out = [(c["x_last"], c["gf_last"], c["Jc_last"], c["Jd_last"])]
    for _ in range(k):
        x, gf, jc, jd = out[-1]
        d = 0.1 * rng.standard_normal(c["nx"])
        out.append((x + d, gf + (2.0 + rng.random(c["nx"])) * d, jc + 0.05 * rng.standard_normal(len(jc)), jd + 0.05 * rng.standard_normal(len(jd))))
    return out, 0.05 * c["yc"], 0.05 * c["yd"]


def dev(v):
    return torch.tensor(np.ascontiguousarray(v), dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("variant", ["plain", "mapped", "resto_sr1"])
def test_push_is_bitwise_the_push_of_the_fetched_vectors(variant):
    """handle A: form -> push; handle B: the device push of A's s and y (lbfgs_push_device; under a row map of every second index
    lbfgs_push_mapped_device; a restoration-phase SR1 history with two values of eta lbfgs_push_resto_device): the histories, the installed columns, sigma,
    memory and the outcomes agree bit for bit"""
    c = next(x for x in qp.SHAPES() if x["name"] == "nx64")
    nx = c["nx"]
    resto = variant == "resto_sr1"
    A, B = handle(c), handle(c, define=False)
    idx = np.arange(0, nx, 2, dtype=np.int32) if variant == "mapped" else None
    rows = nx if idx is None else len(idx)
    dr = np.random.default_rng(5).uniform(0.5, 2.0, rows)
    for s in (A, B):
        if idx is not None:
            s.lowrank_rowmap(idx)
        if resto:
            s.lbfgs_define_resto(rows, dr, max_history=6, type=kkt.LBFGS_SR1)
        else:
            s.lbfgs_define(rows, 6)
    its, yc, yd = iterates(c, 3, seed=21)
    etas = [0.3, 0.3, 0.07]
    outcomes = []
    for k in range(1, 4):
        x0, gf0, jc0, jd0 = its[k - 1]; x1, gf1, jc1, jd1 = its[k]
        if k == 1:
            A.qn_pair_store(x0, None if resto else gf0)
        else:
            A.qn_pair_store()                                                        # roll
        set_j(A, jc1, jd1)
        amax = A.qn_pair_form(x1, None if resto else gf1, yc, yd)
        sv, yv = A.qn_pair_get("s"), A.qn_pair_get("y")
        assert bits(amax) == bits(np.abs(sv if idx is None else sv[idx]).max())
        ds, dy = dev(sv), dev(yv)
        torch.cuda.synchronize()
        oa = A.qn_pair_push(etas[k - 1]) if resto else A.qn_pair_push()
        if resto:
            ob = B.lbfgs_push_resto_device(ds.data_ptr(), dy.data_ptr(), etas[k - 1])
        elif idx is not None:
            ob = B.lbfgs_push_mapped_device(ds.data_ptr(), dy.data_ptr(), nx)
        else:
            ob = B.lbfgs_push_device(ds.data_ptr(), dy.data_ptr())
        assert oa == ob
        outcomes.append(oa)
        Ia, Ib = A.lbfgs_info(), B.lbfgs_info()
        assert Ia["memory"] == Ib["memory"] and bits(Ia["sigma"]) == bits(Ib["sigma"]) and Ia["skipped_in_a_row"] == Ib["skipped_in_a_row"]
        assert A.lowrank_info()["nv"] == B.lowrank_info()["nv"] and A.lowrank_info()["nu"] == B.lowrank_info()["nu"]
        for what in ("S", "Y", "V", "U", "D", "L", "STS"):
            assert np.array_equal(bits(A.lbfgs_get(what)), bits(B.lbfgs_get(what))), (variant, k, what)
        if resto:
            assert bits(A.lbfgs_resto_info()["eta"]) == bits(B.lbfgs_resto_info()["eta"])
    print(f"{variant}: outcomes {outcomes}, memory {A.lbfgs_info()['memory']}")
    assert kkt.LBFGS_STORED in outcomes and A.lbfgs_info()["memory"] >= 2


@pytest.mark.parametrize("resto", [False, True])
def test_device_vectors_give_the_bits_of_host_vectors(resto):
    c = next(x for x in qp.SHAPES() if x["name"] == "nx257")
    s = handle(c)
    s0, y0 = check(s, c, resto)
    set_j(s, c["Jc_last"], c["Jd_last"])
    t = {k: dev(c[k]) for k in ("x_last", "gf_last", "x", "gf", "yc", "yd")}
    torch.cuda.synchronize()
    s.qn_pair_store_device(t["x_last"].data_ptr(), None if resto else t["gf_last"].data_ptr())
    set_j(s, c["Jc_cur"], c["Jd_cur"])
    amax = s.qn_pair_form_device(t["x"].data_ptr(), None if resto else t["gf"].data_ptr(), t["yc"].data_ptr(), t["yd"].data_ptr())
    assert np.array_equal(bits(s.qn_pair_get("s")), bits(s0)) and np.array_equal(bits(s.qn_pair_get("y")), bits(y0)) and bits(amax) == bits(np.abs(s0).max())
    assert s.qn_pair_form_device(t["x"].data_ptr(), None if resto else t["gf"].data_ptr(), t["yc"].data_ptr(), t["yd"].data_ptr(), amax=False) is None
    assert np.array_equal(bits(s.qn_pair_get("y")), bits(y0))                        # run to run: the same bits


def test_state_rules_and_the_validation_through_a_handle_with_a_device():
    c = next(x for x in qp.SHAPES() if x["name"] == "nd0")
    n, irn, jcn, lens = qp.system(c)
    dims = [c["nx"], c["ns"], c["nc"], c["nd"]]
    s = handle(c, define=False)

    def refused(word, call):
        with pytest.raises(ipopt_amd.KKTError, match=word):
            call()

    t = int(np.sum(lens[:qp.SEG_JC])) + 2
    bad = irn.copy(); bad[t] = 1
    refused(f"position {t}.*both indices lie in the x block", lambda: s.qn_pair_define(dims, bad, jcn, qp.SEG_JC, qp.SEG_JD))
    refused("seg_jc = 8 is out of range", lambda: s.qn_pair_define(dims, irn, jcn, 8, qp.SEG_JD))
    refused("J_c triplet at position", lambda: s.qn_pair_define(dims, irn, jcn, 1, qp.SEG_JD))          # the D_x segment is no Jacobian
    refused("qn_pair_define first", lambda: s.qn_pair_store(c["x"], c["gf"]))
    s.qn_pair_define(dims, irn, jcn, qp.SEG_JC, qp.SEG_JD)
    refused("qn_pair_store first", lambda: s.qn_pair_form(c["x"], c["gf"], c["yc"], c["yd"]))
    s.qn_pair_store(c["x_last"], c["gf_last"])
    refused("qn_pair_form first", s.qn_pair_push)
    refused("grad_f is null", lambda: s.qn_pair_form(c["x"], None, c["yc"], c["yd"]))
    assert s.qn_pair_form(c["x"], c["gf"], c["yc"], c["yd"], amax=False) is None
    refused("no history", s.qn_pair_push)
    out = np.zeros(c["nx"])
    assert s.lib.mi355x_kkt_qn_pair_get(s._h, 0, out.ctypes.data, c["nx"] - 1) == kkt.FATAL and "capacity is below" in s.last_error()
    assert s.lib.mi355x_kkt_qn_pair_get(s._h, 0, out.ctypes.data, c["nx"]) == kkt.SUCCESS and np.array_equal(bits(out), bits(c["x"] - c["x_last"]))
    s.lbfgs_define_resto(c["nx"], np.ones(c["nx"]))
    refused("without grad_f", lambda: s.qn_pair_push(0.5))
    s.lbfgs_define(c["nx"], 4)
    assert s.qn_pair_push() in (kkt.LBFGS_STORED, kkt.LBFGS_SKIPPED, kkt.LBFGS_NOT_POSDEF)
    s.qn_pair_store(c["x_last"], None)
    refused("grad_f is given", lambda: s.qn_pair_form(c["x"], c["gf"], c["yc"], c["yd"]))
    s.qn_pair_form(c["x"], None, c["yc"], c["yd"])
    refused("with grad_f", s.qn_pair_push)
    # a new assembly_define ends the definition
    s.assembly_define(lens)
    assert not s.qn_pair_info()["defined"]
    refused("qn_pair_define first", lambda: s.qn_pair_store(c["x"], c["gf"]))


def test_one_chain_as_a_product_would_run_it():
    """qn_bfgs_180's structure: store -> assembly_set with the new J -> form -> push -> factor with the handle's sigma on the x diagonal -> lowrank_update ->
    lowrank_solve, the scaled residual against the dense updated matrix"""
    import scipy.sparse as sp
    c = qp.recorded_case("qn_bfgs_180", 0, 1)
    nx, ns, nc, nd = c["nx"], c["ns"], c["nc"], c["nd"]
    rng = np.random.default_rng(17)
    d = 0.1 * rng.standard_normal(nx)
    c = dict(c, x=c["x_last"] + d, gf=c["gf_last"] + (2.0 + rng.random(nx)) * d, yc=1e-3 * c["yc"], yd=1e-3 * c["yd"])
    s = handle(c)
    s.lbfgs_define(nx, 6)
    sv, yv = check(s, c, False)
    assert s.qn_pair_push() == kkt.LBFGS_STORED
    sigma = s.lbfgs_info()["sigma"]
    s.assembly_set(1, np.full(nx, sigma))
    shift = np.array([0, 0, 0, 0, -DELTA, 0, -1, -DELTA], dtype=float)
    st, neg, _ = s.factor_assembled(SCALE, shift)
    assert st == kkt.SUCCESS and neg == nc + nd
    assert s.lowrank_update() == (kkt.SUCCESS, 0)
    n, irn, jcn, lens = qp.system(c)
    srcs = [np.zeros(lens[0]), np.full(nx, sigma), np.ones(ns), c["Jc_cur"], np.zeros(nc), c["Jd_cur"], np.zeros(ns), np.zeros(nd)]
    vals = np.concatenate([sc * v + sh for sc, sh, v in zip(SCALE, shift, srcs)])
    L = sp.coo_matrix((vals, (irn - 1, jcn - 1)), shape=(n, n)).toarray()
    Kt = L + np.tril(L, -1).T
    V, U = s.lbfgs_get("V"), s.lbfgs_get("U")
    Kt[:nx, :nx] += V @ V.T - U @ U.T
    rhs = rng.standard_normal(n)
    x = rhs.copy()
    s.lowrank_solve(x)
    res = sres(Kt, x, rhs)
    print(f"chain on qn_bfgs_180: sigma {sigma:.3e}, scaled residual {res:.2e}")
    assert res <= RES_TOL
