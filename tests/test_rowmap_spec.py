"""-m 'not gpu': the permutation argument of tests/support/rowmap_spec.py.  The mapped update K~ = K + P (V V^T - U U^T) P^T, stated as the update of
tests/support/lowrank_spec.py on the permuted matrix, solves the dense K~ for the six cases of tests/test_gpu_lowrank_rowmap.py; M1 and M2 are positive
definite (which = 0), lambda_min(M2) = 0.25 wherever there is a U, and K~ has K's inertia.
Bound of the solve: scaled residual <= 4 eps cond_2(K).  Sherman-Morrison through K^-1 is only conditionally stable: Z1 = K^-1 P V carries a relative
error of eps cond(K), and it enters M1 = I + sym(V^T Z1) multiplied by lambda_max(V^T (K^-1) V), which the recipe sets to 4.  The single-row case shows it:
V = 101.5 and U = 98.3 on one diagonal entry nearly cancel (V^2 - U^2 = 644) and the specification reaches 1.1e-12 there (cond(K) = 3.4e5; the
unmapped recipe on the first row alone reaches 1.2e-10), where the cases with hundreds of rows reach 1e-15 .. 1e-16."""
import functools

import numpy as np
import pytest

from tests.support import kktgen
from tests.support import lowrank_spec as lr
from tests.support import rowmap_spec as rm

SYSTEMS = {
    180: lambda: kktgen.grid_kkt(10, 9, dof=2, ncon=1),
    517: lambda: kktgen.lukvl_like(517, delta_c=1e-8),
    1728: lambda: kktgen.grid_kkt(24, 24, dof=3, ncon=2),
}


@functools.lru_cache(maxsize=None)
def dense(nx):
    n, r, c, v, m = SYSTEMS[nx]()
    assert n - m == nx
    K = kktgen.to_scipy(n, r, c, v).toarray()
    K.setflags(write=False)
    return K, m


def test_the_maps_are_strictly_ascending_and_hold_both_ends():
    for nx, rows, _ in rm.CASES:
        idx = rm.make_idx(nx, rows)
        assert idx.dtype == np.int32 and idx.size == rows and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < nx
        if rows > 1:
            assert idx[0] == 0 and idx[-1] == nx - 1
        else:
            assert idx[0] == nx // 2
        p = rm.perm_of(idx, nx + 5)
        assert np.array_equal(np.sort(p), np.arange(nx + 5)) and np.array_equal(p[:rows], idx)


@pytest.mark.parametrize("nx,rows,pair", rm.CASES, ids=lambda v: str(v).replace(" ", ""))
def test_the_permuted_specification_solves_the_dense_mapped_system(nx, rows, pair):
    K, m = dense(nx)
    n = K.shape[0]
    M = rm.Mapped(K, rm.make_idx(nx, rows), *pair)
    assert M.upd["which"] == 0
    assert np.linalg.eigvalsh(M.upd["M1"]).min() > 0 if pair[0] else True
    if pair[1]:
        lam = np.linalg.eigvalsh(M.upd["M2"]).min()
        print(f"lambda_min(M2) = {lam!r}")
        assert abs(lam - 0.25) <= 1e-9
    # K~ = K + P (V V^T - U U^T) P^T, written without the helper
    Kt = K + rm.expand(M.V, M.idx, n) @ rm.expand(M.V, M.idx, n).T - rm.expand(M.U, M.idx, n) @ rm.expand(M.U, M.idx, n).T
    assert np.abs(Kt - M.Kt).max() <= 1e-12 * np.abs(Kt).max()
    assert lr.num_neg(M.Kt) == m                                              # the inertia of K
    rng = np.random.default_rng(5)
    b3 = rng.standard_normal(n); keep = np.zeros(n, bool); keep[M.idx] = True; b3[~keep] = 0.0
    B = np.column_stack([M.Kt @ np.ones(n), rng.standard_normal(n), b3])
    X = M.solve(B)
    bound = 4.0 * np.finfo(np.float64).eps * np.linalg.cond(K)
    for k in range(3):
        res = np.abs(M.Kt @ X[:, k] - B[:, k]).max() / (np.abs(M.Kt).sum(axis=1).max() * np.abs(X[:, k]).max() + np.abs(B[:, k]).max())
        print(f"right-hand side {k}: scaled residual {res:.2e} (bound {bound:.2e})")
        assert res <= bound
    assert np.abs(X[:, 0] - 1.0).max() <= 1e-7
