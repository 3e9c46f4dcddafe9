"""Host only (no device): MI355X_KKT_DISABLE=trsm_regs selects, inside numeric.hip's run_factor_list, which instantiation of k_big_trsm an FO_TRSM record
launches (trsm_rows_regs with the L11 operands in registers, or trsm_rows_impl with L11 staged in LDS) and with how much LDS.  The plan knows nothing of
it: the exported plan -- `inputs` and both factor schedules included -- is the same under the knob, byte for byte, and the reach of the path is INFERRED
from its structural precondition, an FO_TRSM record in the full single-GPU factor schedule (the form of xcd_affine and norestore in tests/test_reach.py).

Where the precondition holds: NOT in the default plan of these fixtures (grid24, grid48x44, clique_edge: 0 FO_TRSM records -- their levels of a few
big fronts go to k_grp_fused and k_big_diag_trsm; an FO_TRSM record is what levels of many fronts get, synth_1e6: 28 per factorisation), but in the
per-link plan MI355X_KKT_DISABLE=grouped,fuse_dt (tests/support/trsmfix.py BASE), under which both legs of tests/test_gpu_trsm_regs.py run: 6, 12 and 18
records.  Both plans are compared with and without the knob; the precondition is asserted on the per-link one.

Also here, for the fixtures of the device test: the same two facts, plain fp64 LAPACK within 1e-9 of the longdouble-refined reference (the forward-error
cap hides nothing), and on the CPU specification (tests/support/mirror.py) that the hostile grid of that size makes pivot blocks leave the fast path (both
thresholds) and marks columns a posteriori (u = 0.01; at u = 1e-8 no multiplier reaches 1e8 and the specification marks none)."""
import functools

import numpy as np
import pytest

import ipopt_amd
from tests.support import mirror, pathfix, reach as R, trsmfix

PATHFIX_FIXTURES = ["grid24", "grid48x44", "clique_edge"]


def join(*names):
    return ",".join(x for x in names if x) or None


@functools.lru_cache(maxsize=None)
def analysed(name):
    if name in trsmfix.FIXTURES:
        S, tune = trsmfix.system(name), None
    else:
        S = pathfix.system(name); tune = S["tune"]
    with pathfix.knobs(None, tune):
        s = ipopt_amd.KKTSolver(**S["opts"])
        s.initialize_structure(S["n"], S["r"], S["c"], vals=S["v"])
    return s, tune


def plan(name, disable):
    s, tune = analysed(name)
    with pathfix.knobs(disable, tune):
        return R.plan_arrays(s)


def trsm_records(P):
    full = P["factor.single.full"].reshape(-1, R.REC)
    return full[full[:, R.OP] == R.FO_TRSM]


def check_fixture(name):
    for base in (None, trsmfix.BASE):
        on, off = plan(name, base), plan(name, join(base, trsmfix.KNOB))
        assert R.plan_diff(on, off) == [], (name, base)
        for w in R.PLAN_ARRAYS:      # (byte for byte, not only value for value)
            assert on[w].dtype == off[w].dtype and on[w].tobytes() == off[w].tobytes(), (name, base, w)
        t = trsm_records(on)
        print(f"{name} [MI355X_KKT_DISABLE={base}]: FO_TRSM records {len(t)}, widest panels {sorted(set(t[:, R.A0].tolist()))}, row blocks {sorted(set(t[:, R.GX].tolist()))}, "
              f"fronts per launch {sorted(set(t[:, R.GY].tolist()))}")
    assert len(t) >= 1                                            # the precondition, on the plan the device test runs
    assert np.all((t[:, R.A0] >= 1) & (t[:, R.A0] <= 64))      # the record's a[0], the widest panel of the launch: what sizes trsm_regs_lds_bytes
    return t


@pytest.mark.parametrize("fixture", PATHFIX_FIXTURES)
def test_trsm_regs_leaves_the_plan_alone_and_its_launch_is_reached(fixture):
    check_fixture(fixture)


# device-test fixture -> widths (a[0]) its FO_TRSM launches must include: kp16 = 16 / 48 with padded columns / 64
WIDTHS = {"grid24": {15, 30, 45, 55, 60, 64}, "clique331_sn8": {7}, "clique331_sn40": {39}, "clique331_sn64": {63}, "hostile_1e-8": {5, 34, 48, 64}, "hostile_0.01": {5, 34, 48, 64}}


@pytest.mark.parametrize("fixture", sorted(trsmfix.FIXTURES))
def test_device_fixture_reaches_the_launch_and_is_well_conditioned(fixture):
    t = check_fixture(fixture)
    assert WIDTHS[fixture] <= set(t[:, R.A0].tolist())
    assert t[:, R.GX].max() >= 3                                  # several row blocks per front
    if fixture == "clique331_sn8":                                # the chain shrinks by 7 rows a link: every row remainder mod 64 and mod 2
        s, _ = analysed(fixture)
        nsn = s.info().num_sn
        order = np.diff(s.symbolic(2, nsn + 1)); cols = np.diff(s.symbolic(1, nsn + 1)); big = s.symbolic(23, nsn) == R.FC_BIG
        below = (order - cols)[big]
        assert len(below) >= 25 and {0, 1} <= set((below % 2).tolist()) and len(set((below % 64).tolist())) >= 25
    S = trsmfix.system(fixture)
    ref, plain = trsmfix.reference(fixture)
    for k in range(3):
        err = np.abs(plain[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max())
        print(fixture, k, "plain fp64 against the reference: %.2e" % err)
        assert err <= 1e-9
    if S["hostile"] is not None:
        u = S["hostile"]
        s, _ = analysed(fixture)
        nsn = s.info().num_sn
        nbig = int(np.sum((s.symbolic(23, nsn) == R.FC_BIG) & (np.diff(s.symbolic(1, nsn + 1)) <= 64)))
        _, spec = mirror.factor_solve_pivoted(mirror.fetch(s), S["v"], S["B"][0], u=u, u2=max(u, 1e-4))
        print(fixture, "specification: big pivot blocks", nbig, "fast", spec["num_fast"], "2x2", spec["num_two"], "failed a posteriori", spec["num_delay"], "marked", len(spec["marks"]))
        assert spec["num_fast"] < nbig and spec["num_two"] >= 20
        assert (spec["num_delay"] >= 50 and len(spec["marks"]) >= 50) if u >= 0.01 else spec["num_delay"] == 0
