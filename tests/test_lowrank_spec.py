"""-m 'not gpu': the in-place form of the low-rank-updated solve (tests/support/lowrank_spec.py, the statement the device route of
mi355x_kkt_lowrank_* is held to) against the dense K~ = K + V V^T - U U^T, on 4 systems x 6 column counts.  Recipe: V scaled so that
lambda_max(V^T (K^-1)_xx V) = 4, U so that lambda_max(U^T ((K + V V^T)^-1)_xx U) = 0.75  =>  lambda_min(M1) >= 1, lambda_min(M2) = 0.25.
Measured when this was written: scaled residuals <= 1.1e-15 (the reference's right-hand-side form on the same inputs: up to 7.6e-15)."""
import functools

import numpy as np
import pytest

from tests.support import kktgen
from tests.support import lowrank_spec as lr

SYSTEMS = {
    "lukvl_300": lambda: kktgen.lukvl_like(300),
    "lukvl_517_dc": lambda: kktgen.lukvl_like(517, delta_c=1e-8),
    "grid_10x9": lambda: kktgen.grid_kkt(10, 9, dof=2, ncon=1),
    "grid_24x24": lambda: kktgen.grid_kkt(24, 24, dof=3, ncon=2),
}
PAIRS = [(0, 1), (1, 0), (5, 7), (12, 12), (32, 32), (17, 32)]
SPEC_TOL = 5e-14


def sres(K, x, b):      # (tests/test_gpu_parity.py)
    return np.abs(K @ x - b).max() / (abs(K).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max() + 1e-300)


@functools.lru_cache(maxsize=None)
def system(name):
    n, r, c, v, m = SYSTEMS[name]()
    K = kktgen.to_scipy(n, r, c, v).toarray()
    rows = n - m
    return n, rows, m, K, lr.dense_solver(K), lr.num_neg(K)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"nv{p[0]}_nu{p[1]}")
@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_in_place_form_solves_the_dense_updated_system(name, pair):
    n, rows, m, K, ksolve, negK = system(name)
    assert negK == m
    nv, nu = pair
    V, U = lr.scaled_columns(K, rows, nv, nu, seed=11, solve=ksolve)
    upd = lr.update(K, V, U, ksolve)
    assert upd["which"] == 0
    if nv:
        assert np.linalg.eigvalsh(upd["M1"]).min() >= 1.0 - 1e-9
    if nu:
        assert abs(np.linalg.eigvalsh(upd["M2"]).min() - 0.25) <= 1e-9
    Kt = lr.dense_updated(K, V, U)
    rng = np.random.default_rng(5)
    b2 = rng.standard_normal(n)
    b3 = rng.standard_normal(n); b3[rows:] = 0.0
    worst = worst_ref = 0.0
    for b in (Kt @ np.ones(n), b2, b3):
        x = lr.solve(K, V, U, upd, b, ksolve)
        worst = max(worst, sres(Kt, x, b))
        worst_ref = max(worst_ref, sres(Kt, lr.solve_rhs_form(K, V, U, upd, b, ksolve), b))
    print(f"{name} nv={nv} nu={nu}: scaled residual in-place form {worst:.2e}, right-hand-side form {worst_ref:.2e}")
    assert worst <= SPEC_TOL
    assert lr.num_neg(Kt) == negK
    # U doubled: lambda_min(M2) = 1 - 4 * 0.75 = -2, and K~ gains negative eigenvalues
    if nu:
        U2 = 2.0 * U
        upd2 = lr.update(K, V, U2, ksolve)
        assert upd2["which"] == 2
        assert abs(np.linalg.eigvalsh(upd2["M2"]).min() + 2.0) <= 1e-8
        gained = lr.num_neg(lr.dense_updated(K, V, U2)) - negK
        assert 1 <= gained <= nu
