"""CPU: the random stream of the synthetic bench workloads (xoshiro256** seeded by splitmix64(20260923)) -- known answers of the two
published algorithms, and the generator's by-construction inertia on a small sibling of `synth_1e6` checked with the oracle."""
import numpy as np

from oracle import kkt_oracle as ko
from tests.support import kktgen


def test_splitmix64_and_xoshiro256starstar_known_answers():
    x = kktgen.Xoshiro256(0)
    assert int(x.state[0]) == 0xE220A8397B1DCDAF and int(x.state[1]) == 0x6E789E6AA1B965F4      # splitmix64 from seed 0: its first two outputs
    x.state[:] = [1, 2, 3, 4]
    # xoshiro256** from the state (1, 2, 3, 4): 11520, 0, 1509978240, 1215971899390074240 -> the top 53 bits of each
    assert np.array_equal(x.random(4) * 2.0 ** 53, [11520 >> 11, 0, 1509978240 >> 11, 1215971899390074240 >> 11])
    a = kktgen.Xoshiro256(20260923).uniform(-1, 1, (3, 5)); b = kktgen.Xoshiro256(20260923).uniform(-1, 1, 15)
    assert np.array_equal(a.ravel(), b) and np.all(np.abs(a) < 1)                                 # one stream, consumed in C order


def test_synthetic_generator_on_the_xoshiro_stream_has_the_inertia_it_was_built_for():
    n, r, c, v, neg = kktgen.grid_kkt(12, 10, dof=3, ncon=2, seed=20260923, sigma_exp=8.0, rng="xoshiro")
    n2, r2, c2, v2, _ = kktgen.grid_kkt(12, 10, dof=3, ncon=2, seed=20260923, sigma_exp=8.0, rng="xoshiro")
    assert np.array_equal(v, v2) and np.array_equal(r, r2) and neg == 12 * 10 * 2               # deterministic
    K = kktgen.to_scipy(n, r, c, v)
    b = K @ np.ones(n)
    x, oneg, ozero, _ = ko.factor_solve(n, r, c, v, b, u=0.01)
    assert oneg == neg and ozero == 0 and np.abs(x - 1).max() <= 1e-6


def test_clique_generator_has_the_structure_and_the_inertia_it_was_built_for():
    """cliques along a path that share `sep` variables, three-variable constraint rows on disjoint supports: inertia (n_x, m, 0) by LAPACK's eigenvalues,
    with and without shared variables, without constraints, and as a direct sum"""
    for sizes, sep, m in (([40], 0, 6), ([30, 25, 20], 5, 9), ([35, 35], 0, 0)):
        n, r, c, v, neg = kktgen.clique_kkt(sizes, sep, m, seed=5)
        nx = sum(sizes) - sep * (len(sizes) - 1)
        assert n == nx + m and neg == m
        K = kktgen.to_scipy(n, r, c, v).toarray()
        w = np.linalg.eigvalsh(K)
        assert int((w < 0).sum()) == m and np.abs(w).min() > 1e-8
        H = K[:nx, :nx] != 0
        first = 0
        for s in sizes:                                    # every clique is dense, and nothing couples variables of no common clique
            assert H[first:first + s, first:first + s].all()
            first += s - sep
        assert int(np.tril(H, -1).sum()) == sum(s * (s - 1) // 2 for s in sizes) - (len(sizes) - 1) * sep * (sep - 1) // 2
        J = K[nx:, :nx] != 0
        assert np.all(J.sum(axis=1) == 3) and np.all(J.sum(axis=0) <= 1)      # disjoint supports: full row rank whatever the values
    a, b = kktgen.clique_kkt([20], 0, 3, seed=1), kktgen.grid_kkt(4, 3, dof=2, ncon=1, seed=2)
    n, r, c, v, neg = kktgen.block_diag(a, b)
    K = kktgen.to_scipy(n, r, c, v).toarray()
    assert n == a[0] + b[0] and neg == a[4] + b[4] == int((np.linalg.eigvalsh(K) < 0).sum())
    assert not K[:a[0], a[0]:].any() and np.array_equal(K[:a[0], :a[0]], kktgen.to_scipy(*a[:4]).toarray())


def test_with_diagonal_replaces_the_whole_diagonal_entry_and_nothing_else():
    """the H diagonal and Sigma are two triplets of one entry: both go, the value is put once; every other entry, the pattern and the input stay"""
    S = kktgen.block_diag(kktgen.clique_kkt([9, 7], 3, 2, seed=3), kktgen.star_kkt(3, 4, 2, 5, seed=4))
    n, r, c, v, neg = S
    v0 = v.copy()
    K0 = kktgen.to_scipy(n, r, c, v).toarray()
    edit = [0, 5, 13, n - 1]                                # two clique variables, the first constraint row (13 primal variables before it), the last hub variable
    assert [int(np.sum((r == c) & (r == x + 1))) for x in edit] == [2, 2, 1, 2]      # H diagonal + Sigma; the (2,2) block has one triplet
    n2, r2, c2, v2, neg2 = kktgen.with_diagonal(S, edit, 1e-6)
    assert n2 == n and neg2 is None and np.array_equal(r2, r) and np.array_equal(c2, c) and np.array_equal(v, v0) and v2 is not v
    K = kktgen.to_scipy(n2, r2, c2, v2).toarray()
    D = K - K0
    assert np.count_nonzero(D) == len(edit) and all(D[x, x] != 0.0 for x in edit)
    assert all(K[x, x] == 1e-6 for x in edit)
    assert K0[13, 13] == 0.0                                # (a diagonal that was an explicit zero gets the value too)
    off = (r != c)
    assert np.array_equal(v2[off], v[off])
    assert np.array_equal(kktgen.with_diagonal(S, [], 1e-6)[3], v)
    K3 = kktgen.to_scipy(*kktgen.with_diagonal(S, [5, 0], [2.5, -3.0])[:4]).toarray()      # one value per variable
    assert K3[5, 5] == 2.5 and K3[0, 0] == -3.0 and np.count_nonzero(K3 - K0) == 2


def test_star_generator_has_the_structure_and_the_inertia_it_was_built_for():
    """leaf cliques that share the same variables of a hub clique: symmetric pattern, every clique dense, the leaves coupled through the hub only,
    inertia (n, 0, 0) by LAPACK's eigenvalues"""
    leaves, own, sep, hub = 4, 9, 5, 8
    n, r, c, v, neg = kktgen.star_kkt(leaves, own, sep, hub, seed=3)
    assert n == leaves * own + hub and neg == 0 and np.array_equal(v, kktgen.star_kkt(leaves, own, sep, hub, seed=3)[3])
    K = kktgen.to_scipy(n, r, c, v).toarray()
    w = np.linalg.eigvalsh(K)
    assert np.array_equal(K, K.T) and int((w < 0).sum()) == 0 and w.min() > 1e-8
    P = K != 0
    h0 = leaves * own
    assert P[h0:, h0:].all()
    for l in range(leaves):
        mine = np.r_[l * own:(l + 1) * own]
        assert P[np.ix_(mine, mine)].all() and P[np.ix_(mine, np.r_[h0:h0 + sep])].all()
        assert not P[np.ix_(mine, np.r_[h0 + sep:n])].any()
        others = np.setdiff1d(np.r_[0:h0], mine)
        assert not P[np.ix_(mine, others)].any()
    assert int(np.tril(P, -1).sum()) == leaves * (own * (own - 1) // 2 + own * sep) + hub * (hub - 1) // 2
