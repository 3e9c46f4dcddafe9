"""-m 'not gpu': the specification of the quasi-Newton pair formed on the device (tests/support/qn_pair_spec.py) against itself: pair_ld (per-entry
differences, longdouble), pair_ref64 (the float64 transcription of the reference's order, IpLimMemQuasiNewtonUpdater.cpp:282, :297-300 / :304-307) and
bound agree on cases computed by hand; the REFERENCE's order stays within the derived bound on every input of tests/test_gpu_qn_pair.py (INPUTS), so
the bound the device is held to is shown to hold for the reference alone; where the bound is 0 the result is exactly 0; unchanged Jacobians give
y = gf - gf_last bitwise."""
import numpy as np
import pytest

from tests.support import qn_pair_spec as qp

CASES = list(qp.INPUTS())


def hand_case():
    """nx = 3, J_c = [[2, 0, 1]] (one row), J_d = [[0, 3, 0], [0, 4, 0]] with the (0, 1) entry given twice (1 + 2); column 2 changes, column 0 does not"""
    c = dict(name="hand", nx=3, ns=2, nc=1, nd=2, jc=(np.array([0, 0]), np.array([0, 2])), jd=(np.array([0, 1, 0]), np.array([1, 1, 1])), jc_upper=False)
    c["Jc_last"] = np.array([2.0, 1.0]); c["Jc_cur"] = np.array([2.0, 1.5])
    c["Jd_last"] = np.array([1.0, 4.0, 2.0]); c["Jd_cur"] = np.array([1.5, 3.0, 2.0])
    c["x_last"] = np.array([1.0, 2.0, 3.0]); c["x"] = np.array([1.5, 2.0, 2.0])
    c["gf_last"] = np.array([0.5, 0.25, 0.0]); c["gf"] = np.array([1.0, 0.25, -1.0])
    c["yc"] = np.array([4.0]); c["yd"] = np.array([2.0, -1.0])
    return c


def test_the_three_functions_on_a_case_computed_by_hand():
    c = hand_case()
    # y_0 = 0.5 + 0; y_1 = 0 + (0.5 * 2) + (-1 * -1) + 0 = 2; y_2 = -1 + 0.5 * 4 = 1
    for f in (qp.pair_ld, qp.pair_ref64):
        s, y = f(c)
        assert np.array_equal(np.asarray(s, dtype=float), [0.5, 0.0, -1.0]) and np.array_equal(np.asarray(y, dtype=float), [0.5, 2.0, 1.0]), f.__name__
        s, y = f(c, resto=True)
        assert np.array_equal(np.asarray(s, dtype=float), [0.5, 0.0, -1.0]) and np.array_equal(np.asarray(y, dtype=float), [0.0, 2.0, 2.0]), f.__name__
    # bound: k = (1, 3, 1); mag_0 = 1.5 + 4 * 4 = 17.5, mag_1 = 0.5 + 2.5 * 2 + 7 * 1 + 4 * 2 = 20.5, mag_2 = 1 + 2.5 * 4 = 11
    assert np.array_equal(qp.bound(c), np.array([5 * 17.5, 7 * 20.5, 5 * 11.0]) * 2.0 ** -52)
    assert np.array_equal(qp.bound(c, resto=True), np.array([5 * 16.0, 7 * 20.0, 5 * 10.0]) * 2.0 ** -52)
    assert np.array_equal(qp.column_lengths(c), [1, 3, 1]) and qp.expected_lpc(c) == 1


def test_the_inputs_reach_every_instantiation_and_every_edge():
    lens = {c["name"]: qp.column_lengths(c) for c in CASES}
    assert {qp.expected_lpc(c) for c in CASES} == {1, 8, 64}
    assert [c["nx"] for c in CASES[:5]] == [1, 63, 64, 65, 257]
    assert set(lens["columns"][:6]) == {0, 1, 64, 65, 257, 300}
    by = {c["name"]: c for c in CASES}
    assert by["nc0"]["nc"] == 0 and by["nc0"]["nd"] > 0 and by["nd0"]["nd"] == 0 and by["nd0"]["nc"] > 0
    d = by["duplicates"]; pairs = list(zip(*d["jc"]))
    assert len(pairs) - len(set(pairs)) == 25
    assert by["jc_upper"]["jc_upper"]
    assert by["qn_bfgs_517:0->1"]["nc"] == 0 and by["qn_bfgs_517:0->1"]["nd"] > 0                  # a J_d only
    for c in CASES:
        lam = np.concatenate([c["yc"], c["yd"]])
        assert (lam == 0).any() and (lam > 0).any() and (lam < 0).any(), c["name"]
        assert c["ns"] == c["nd"]
    for name in ("qn_bfgs_180:0->1", "qn_bfgs_180:1->2", "qn_sr1_180:0->1", "qn_bfgs_517:0->1"):
        c = by[name]
        assert not (np.array_equal(c["Jc_last"], c["Jc_cur"]) and np.array_equal(c["Jd_last"], c["Jd_cur"])), name     # the recorded Jacobians moved


@pytest.mark.parametrize("resto", [False, True])
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_the_reference_order_stays_within_the_bound(c, resto):
    s_ld, y_ld = qp.pair_ld(c, resto)
    s, y = qp.pair_ref64(c, resto)
    b = qp.bound(c, resto)
    assert np.array_equal(s, c["x"] - c["x_last"]) and np.array_equal(np.asarray(s_ld, dtype=float), s)
    err = np.abs(y.astype(np.longdouble) - y_ld).astype(float)
    ratio = float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    print(f"{c['name']} resto {resto}: reference order / bound {ratio:.3f}")
    assert np.all(err <= b)
    assert np.all(y[b == 0] == 0.0) and np.all(np.asarray(y_ld, dtype=float)[b == 0] == 0.0)
    if resto:
        assert (b == 0).any() or c["name"] != "columns"                                              # the empty column: ypart is exactly 0 there


@pytest.mark.parametrize("c", CASES[:6], ids=[c["name"] for c in CASES[:6]])
def test_unchanged_jacobians_give_the_gradient_difference_bitwise(c):
    u = dict(c, Jc_cur=c["Jc_last"], Jd_cur=c["Jd_last"])
    _, y = qp.pair_ld(u)
    assert np.array_equal(np.asarray(y, dtype=float), c["gf"] - c["gf_last"])
    _, y = qp.pair_ld(u, resto=True)
    assert not np.asarray(y, dtype=float).any()
