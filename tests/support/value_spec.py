"""Plain numpy references for the value path of the solver: everything between the caller's numbers and the factorisation.
TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product.

  * the symmetric row view of a triplet pattern and the equilibration variant the solver picks from its density;
  * ruiz_spec(): the Jacobi-style Ruiz sweeps of the in-solver equilibration (k_abs_rowview*, k_ruiz_sweep) in np.longdouble;
  * ruiz_triplet_spec(): the stand-alone routine mi355x_kkt_ruiz_scaling (k_trip_rowmax / k_trip_rescale) in np.longdouble;
  * assemble_spec(): the segment assembly  values = scale * source + shift  in np.longdouble;
  * the 8-block primal-dual operator of IpPDSystemSolver.hpp:24-49 applied straight from triplets (no dense matrix, any size), and
    the reduction / expansion formulas of SolveOnce (IpPDFullSpaceSolver.cpp:418-424, :653-659).

tests/test_value_spec.py checks every function here against dense brute force on the CPU."""
from __future__ import annotations

import numpy as np

LD = np.longdouble
U = 2.0 ** -53          # unit roundoff of fp64


# ------------------------------------------------------------------------------------------------
# pattern, row view, equilibration
# ------------------------------------------------------------------------------------------------
def summed_lower(n, r, c, v, base=1):
    """The de-duplicated pattern of a one-triangle-or-both triplet list: (row >= col, summed values in longdouble), every position once.
    An entry given as (i, j) and one given as (j, i) are the SAME position of the symmetric matrix and are summed, like the gather does."""
    r = np.asarray(r, dtype=np.int64) - base; c = np.asarray(c, dtype=np.int64) - base
    hi, lo = np.maximum(r, c), np.minimum(r, c)
    key = hi * max(n, 1) + lo
    uk, inv = np.unique(key, return_inverse=True)
    a = np.zeros(uk.shape[0], dtype=LD)
    np.add.at(a, inv, np.asarray(v, dtype=LD))
    return uk // max(n, 1), uk % max(n, 1), a


def rslot_len(n, r, c, base=1):
    """entry count of the symmetric row view: 2 x (off-diagonal pattern entries) + (diagonal pattern entries), duplicates counted once"""
    hi, lo, _ = summed_lower(n, r, c, np.zeros(len(r)), base)
    return int(2 * (hi != lo).sum() + (hi == lo).sum())


def ruiz_variant(n, r, c, base=1):
    """which of the three in-solver variants a pattern gets (enqueue_scaling): 0: 2 lanes per row, fused first sweep (rslot_len < 8 n);
    1: 8 lanes per row, fused first sweep (8 n <= rslot_len < 16 n); 2: 8 lanes per row, separate row-view pass (rslot_len >= 16 n)"""
    ln = rslot_len(n, r, c, base)
    return 0 if ln < 8 * n else (1 if ln < 16 * n else 2)


def _rowmax(n, hi, lo, w):
    mx = np.zeros(n, dtype=LD)
    np.maximum.at(mx, hi, w); np.maximum.at(mx, lo, w)
    return mx


def ruiz_spec(n, r, c, v, sweeps=4, base=1):
    """In-solver equilibration, longdouble.  Duplicates are summed FIRST (the solver equilibrates the gathered matrix), then
         sweep 0:        s_i = 1 / sqrt(max_j |a_ij|)
         later sweeps:   s_i <- s_i / sqrt(s_i max_j(|a_ij| s_j))         (Jacobi: every row reads the factors of the sweep before)
    and a row whose maximum is 0 keeps its factor (1 after sweep 0)."""
    hi, lo, a = summed_lower(n, r, c, v, base)
    a = np.abs(a)
    s = np.ones(n, dtype=LD)
    for k in range(sweeps):
        if k == 0:
            mx = _rowmax(n, hi, lo, a)
            s = np.where(mx > 0, 1 / np.sqrt(np.where(mx > 0, mx, 1)), s)
        else:
            mx = np.zeros(n, dtype=LD)
            np.maximum.at(mx, hi, a * s[lo])              # row hi reads s[lo] ...
            np.maximum.at(mx, lo, a * s[hi])              # ... and row lo reads s[hi]
            mx = s * mx
            s = np.where(mx > 0, s / np.sqrt(np.where(mx > 0, mx, 1)), s)
    return s


def ruiz_triplet_spec(n, r, c, v, sweeps=4, base=1):
    """The stand-alone routine, longdouble:  s_i <- s_i / sqrt(max_q |a_q| s_i s_j)  over the TRIPLETS q that touch row i.
    The difference from ruiz_spec(): duplicates of one position are NOT summed, the maximum runs over the triplets as given
    (1e16, 1, -1e16 on one position count as 1e16 here and as 1 in the solver).  Without duplicates the two iterations are the same
    in exact arithmetic."""
    r = np.asarray(r, dtype=np.int64) - base; c = np.asarray(c, dtype=np.int64) - base
    a = np.abs(np.asarray(v, dtype=LD))
    s = np.ones(n, dtype=LD)
    for _ in range(sweeps):
        mx = _rowmax(n, r, c, a * s[r] * s[c])
        s = np.where(mx > 0, s / np.sqrt(np.where(mx > 0, mx, 1)), s)
    return s


# ------------------------------------------------------------------------------------------------
# segment assembly
# ------------------------------------------------------------------------------------------------
def assemble_spec(scales, shifts, sources):
    """values of the segments, longdouble:  scale * source + shift;  a segment with scale 0 is exactly its shift WHATEVER the source
    holds (Ipopt passes no vector at all for such a block)."""
    out = []
    for sc, sh, src in zip(scales, shifts, sources):
        src = np.asarray(src, dtype=LD)
        out.append(np.full(src.shape[0], LD(sh)) if sc == 0.0 else LD(sc) * src + LD(sh))
    return np.concatenate(out) if out else np.zeros(0, dtype=LD)


# ------------------------------------------------------------------------------------------------
# the 8-block primal-dual system.  A problem P is a dict:
#   nx, ns, nc, nd (ns == nd);  wt = (row, col, val) 0-based triplets of W, either triangle, duplicates allowed;  jct, jdt likewise for
#   J_c (nc x nx) and J_d (nd x nx);  ixl, ixu, isl, isu 0-based positions of the bounded entries;  zl, zu, vl, vu multipliers and
#   sxl, sxu, ssl, ssu slacks of the iterate.
# ------------------------------------------------------------------------------------------------
def pd_offsets(P):
    return np.cumsum([0, P["nx"], P["ns"], P["nc"], P["nd"], len(P["ixl"]), len(P["ixu"]), len(P["isl"]), len(P["isu"])])


def pd_split(P, v):
    o = pd_offsets(P)
    return [v[o[i]:o[i + 1]] for i in range(8)]


def k8_triplets(P, deltas):
    """Every term of  K8 v  as a triplet (row, col, coefficient) in longdouble, W's off-diagonal triplets once per triangle, duplicates
    kept as separate terms -- the matrix of IpPDSystemSolver.hpp:24-49 with the perturbations of ComputeResiduals.  A perturbation that
    is exactly 0 contributes no term."""
    dx, ds, dc, dd = (float(d) for d in deltas)
    o = pd_offsets(P)
    X, S, C, D, ZL, ZU, VL, VU = (int(x) for x in o[:8])
    nx, ns, nc, nd = P["nx"], P["ns"], P["nc"], P["nd"]
    R, Cc, Vv = [], [], []

    def put(r, c, v):
        r = np.asarray(r, dtype=np.int64)
        R.append(r); Cc.append(np.asarray(c, dtype=np.int64)); Vv.append(np.broadcast_to(np.asarray(v, dtype=LD), r.shape))

    wr, wc, wv = P["wt"]; off = wr != wc
    put(X + wr, X + wc, wv); put(X + wc[off], X + wr[off], wv[off])
    jr, jc, jv = P["jct"]; put(C + jr, X + jc, jv); put(X + jc, C + jr, jv)
    jr, jc, jv = P["jdt"]; put(D + jr, X + jc, jv); put(X + jc, D + jr, jv)
    ar = np.arange
    if dx != 0.0: put(X + ar(nx), X + ar(nx), dx)
    if ds != 0.0: put(S + ar(ns), S + ar(ns), ds)
    if dc != 0.0: put(C + ar(nc), C + ar(nc), -dc)
    if dd != 0.0: put(D + ar(nd), D + ar(nd), -dd)
    put(S + ar(ns), D + ar(nd), -1.0); put(D + ar(nd), S + ar(ns), -1.0)
    nb = [len(P["ixl"]), len(P["ixu"]), len(P["isl"]), len(P["isu"])]
    put(X + P["ixl"], ZL + ar(nb[0]), -1.0); put(X + P["ixu"], ZU + ar(nb[1]), 1.0)
    put(S + P["isl"], VL + ar(nb[2]), -1.0); put(S + P["isu"], VU + ar(nb[3]), 1.0)
    put(ZL + ar(nb[0]), X + P["ixl"], P["zl"]); put(ZL + ar(nb[0]), ZL + ar(nb[0]), P["sxl"])
    put(ZU + ar(nb[1]), X + P["ixu"], -np.asarray(P["zu"])); put(ZU + ar(nb[1]), ZU + ar(nb[1]), P["sxu"])
    put(VL + ar(nb[2]), S + P["isl"], P["vl"]); put(VL + ar(nb[2]), VL + ar(nb[2]), P["ssl"])
    put(VU + ar(nb[3]), S + P["isu"], -np.asarray(P["vu"])); put(VU + ar(nb[3]), VU + ar(nb[3]), P["ssu"])
    return np.concatenate(R), np.concatenate(Cc), np.concatenate(Vv), int(o[-1])


def _rowsum(n, R, t):
    # (np.add.at is slow on longdouble at 10^6 terms: sort once, reduce by segments)
    order = np.argsort(R, kind="stable")
    Rs = R[order]
    start = np.flatnonzero(np.concatenate([[True], Rs[1:] != Rs[:-1]])) if Rs.size else np.zeros(0, dtype=np.int64)
    out = np.zeros(n, dtype=LD)
    if Rs.size:
        out[Rs[start]] = np.add.reduceat(t[order], start)
    return out


def k8_apply(P, deltas, v, trip=None):
    """(K8 v,  |K8| |v|,  terms per row,  ||K8||_inf)  in longdouble"""
    R, C, V, n8 = trip if trip is not None else k8_triplets(P, deltas)
    v = np.asarray(v, dtype=LD)
    y = _rowsum(n8, R, V * v[C])
    ya = _rowsum(n8, R, np.abs(V) * np.abs(v[C]))
    k = np.bincount(R, minlength=n8)
    nrm = _rowsum(n8, R, np.abs(V)).max(initial=0)
    return y, ya, k, nrm


def sigma(P):
    """Sigma_x, Sigma_s = Z / slack summed onto the x and s diagonal: what the elimination of the bound rows leaves in the augmented system"""
    sx = np.zeros(P["nx"]); np.add.at(sx, P["ixl"], P["zl"] / P["sxl"]); np.add.at(sx, P["ixu"], P["zu"] / P["sxu"])
    ss = np.zeros(P["ns"]); np.add.at(ss, P["isl"], P["vl"] / P["ssl"]); np.add.at(ss, P["isu"], P["vu"] / P["ssu"])
    return sx, ss


def pd_reduce(P, rhs, dtype=LD):
    """right-hand side of the 4-block augmented system (SolveOnce :418-424): aug = rhs[x|s|c|d], += P_L (rhs_zL / slack_L), -= P_U (rhs_zU / slack_U).
    dtype = np.float64 restates the device's arithmetic and order (one division, one addition per bound: nothing to contract)."""
    b = pd_split(P, np.asarray(rhs, dtype=dtype))
    o = pd_offsets(P)
    aug = np.array(np.concatenate(b[:4]), dtype=dtype)
    X, S = 0, P["nx"]
    np.add.at(aug, X + P["ixl"], b[4] / np.asarray(P["sxl"], dtype=dtype)); np.add.at(aug, S + P["isl"], b[6] / np.asarray(P["ssl"], dtype=dtype))
    np.subtract.at(aug, X + P["ixu"], b[5] / np.asarray(P["sxu"], dtype=dtype)); np.subtract.at(aug, S + P["isu"], b[7] / np.asarray(P["ssu"], dtype=dtype))
    assert aug.shape[0] == o[4]
    return aug


def pd_expand(P, rhs, sol4):
    """back to eight blocks (SolveOnce :653-659), longdouble: sol_zL = (rhs_zL - Z_L P^T sol_x) / slack_L, sol_zU = (rhs_zU + Z_U P^T sol_x) / slack_U, same for v / s.
    Returns (sol8, bound8): bound8 is (|rhs_z| + |Z| |sol_x|) / slack on the bound blocks and 0 on the first four -- the scale of the 3 roundings of each entry."""
    b = pd_split(P, np.asarray(rhs, dtype=LD))
    sol4 = np.asarray(sol4, dtype=LD)
    x, s = sol4[:P["nx"]], sol4[P["nx"]:P["nx"] + P["ns"]]
    q = lambda k: np.asarray(P[k], dtype=LD)
    out = [sol4,
           (b[4] - q("zl") * x[P["ixl"]]) / q("sxl"), (b[5] + q("zu") * x[P["ixu"]]) / q("sxu"),
           (b[6] - q("vl") * s[P["isl"]]) / q("ssl"), (b[7] + q("vu") * s[P["isu"]]) / q("ssu")]
    bnd = [np.zeros(sol4.shape[0], dtype=LD),
           (np.abs(b[4]) + np.abs(q("zl") * x[P["ixl"]])) / q("sxl"), (np.abs(b[5]) + np.abs(q("zu") * x[P["ixu"]])) / q("sxu"),
           (np.abs(b[6]) + np.abs(q("vl") * s[P["isl"]])) / q("ssl"), (np.abs(b[7]) + np.abs(q("vu") * s[P["isu"]])) / q("ssu")]
    return np.concatenate(out), np.concatenate(bnd)


def pd_combine(alpha, sol, beta, res):
    """res <- alpha sol + beta res, longdouble; beta == 0 does not read res (it may hold anything, NaN included)"""
    sol = np.asarray(sol, dtype=LD)
    if beta == 0.0:
        return LD(alpha) * sol
    return LD(alpha) * sol + LD(beta) * np.asarray(res, dtype=LD)


def pd_problem(nx, ns, nc, nxl, nxu, nsl, nsu, seed=0):
    """A small-or-large primal-dual test problem: W tridiagonal plus a few random entries, with duplicates and entries in both triangles, strictly
    diagonally dominant with margin >= 1 BEFORE Sigma and delta_x are added; Jacobian rows of 2 to 3 entries; multipliers and slacks in [0.1, 2]."""
    rng = np.random.default_rng(seed)
    nd = ns
    off = rng.uniform(-1, 1, max(nx - 1, 0))
    nextra = 6 if nx > 2 else 0                                      # (a FEW: long-range couplings cost fill, and the factorisation is not what these systems are for)
    ei = rng.integers(0, nx, nextra); ej = rng.integers(0, nx, nextra); ev = rng.uniform(-1, 1, nextra)
    keep = ei != ej; ei, ej, ev = ei[keep], ej[keep], ev[keep]
    ndup = min(5, nx - 1) if nx > 1 else 0                           # duplicates of the first sub-diagonal entries, given in the OTHER triangle
    r_off = np.concatenate([np.arange(1, nx), ei, np.arange(ndup)]); c_off = np.concatenate([np.arange(nx - 1), ej, np.arange(1, ndup + 1)])
    v_off = np.concatenate([off, ev, rng.uniform(-1, 1, ndup)])
    rowsum = np.zeros(nx); np.add.at(rowsum, r_off, np.abs(v_off)); np.add.at(rowsum, c_off, np.abs(v_off))
    diag = rowsum + rng.uniform(1.0, 2.0, nx)
    half = 0.5 * diag[: nx // 3]                                      # duplicate diagonal entries: a third of the diagonal comes in two halves
    wr = np.concatenate([np.arange(nx), np.arange(nx // 3), r_off]); wc = np.concatenate([np.arange(nx), np.arange(nx // 3), c_off])
    wv = np.concatenate([np.concatenate([diag[: nx // 3] - half, diag[nx // 3:]]), half, v_off])

    def jac(m):
        if m == 0:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0)
        rows, cols, vals = [], [], []
        anchor = rng.permutation(nx)[:m] if m <= nx else rng.integers(0, nx, m)
        third = rng.random(m) < 0.5
        for k in range(3):
            sel = np.arange(m) if k < 2 else np.flatnonzero(third)
            rows.append(sel); cols.append((anchor[sel] + k * 7) % nx)
            vals.append(1.5 + rng.random(sel.shape[0]) if k == 0 else rng.uniform(-0.5, 0.5, sel.shape[0]))
        return np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)

    pick = lambda n, k: np.sort(rng.permutation(n)[:k]).astype(np.int32)
    ixl, ixu, isl, isu = pick(nx, nxl), pick(nx, nxu), pick(ns, nsl), pick(ns, nsu)
    pos = lambda k: rng.uniform(0.1, 2.0, k)
    return dict(nx=nx, ns=ns, nc=nc, nd=nd, wt=(wr.astype(np.int64), wc.astype(np.int64), wv), jct=jac(nc), jdt=jac(nd), ixl=ixl, ixu=ixu, isl=isl, isu=isu,
                zl=pos(nxl), zu=pos(nxu), vl=pos(nsl), vu=pos(nsu), sxl=pos(nxl), sxu=pos(nxu), ssl=pos(nsl), ssu=pos(nsu))


def pd_dominance_margin(P, dx):
    """min over the rows of the (1,1) block  W + Sigma_x + delta_x I  of  diagonal - sum |off-diagonal|:  > 0 means strictly diagonally dominant with a
    positive diagonal, hence positive definite -- the augmented system is then quasi-definite as soon as the (s,s) block is positive and delta_c, delta_d are."""
    hi, lo, a = summed_lower(P["nx"], P["wt"][0], P["wt"][1], P["wt"][2], base=0)
    nx = P["nx"]
    d = np.zeros(nx, dtype=LD); offs = np.zeros(nx, dtype=LD)
    dg = hi == lo
    d[hi[dg]] = a[dg]
    np.add.at(offs, hi[~dg], np.abs(a[~dg])); np.add.at(offs, lo[~dg], np.abs(a[~dg]))
    sx, _ = sigma(P)
    return float((d + sx + dx - offs).min(initial=np.inf))


def pd_kkt_triplets(P):
    """1-based triplets of the augmented system in Ipopt's segment order  W | D_x | D_s | J_c | D_c | J_d | -I | D_d  (IpStdAugSystemSolver.cpp:263-298),
    the segment lengths, and the sources of the device-side assembly (W_factor 1; D_c, -I, D_d have no source)."""
    nx, ns, nc, nd = P["nx"], P["ns"], P["nc"], P["nd"]
    wr, wc, wv = P["wt"]; jcr, jcc, jcv = P["jct"]; jdr, jdc, jdv = P["jdt"]
    ar = lambda n, o: np.arange(n) + o
    irn = np.concatenate([wr, ar(nx, 0), ar(ns, nx), jcr + nx + ns, ar(nc, nx + ns), jdr + nx + ns + nc, ar(nd, nx + ns + nc), ar(nd, nx + ns + nc)]) + 1
    jcn = np.concatenate([wc, ar(nx, 0), ar(ns, nx), jcc, ar(nc, nx + ns), jdc, ar(ns, nx), ar(nd, nx + ns + nc)]) + 1
    lens = [len(wv), nx, ns, len(jcv), nc, len(jdv), ns, nd]
    sx, ss = sigma(P)
    srcs = [wv, sx, ss, jcv, np.zeros(nc), jdv, np.zeros(ns), np.zeros(nd)]
    return irn.astype(np.int32), jcn.astype(np.int32), lens, srcs


PD_SCALE = np.array([1, 1, 1, 1, 0, 1, 0, 0], dtype=float)


def pd_shift(deltas):
    dx, ds, dc, dd = deltas
    return np.array([0, dx, ds, 0, -dc, 0, -1, -dd], dtype=float)


# ------------------------------------------------------------------------------------------------
# the systems and shapes the CPU and the GPU tests share (tests/test_value_spec.py pins their properties without a device)
# ------------------------------------------------------------------------------------------------
def with_isolated_row(n, r, c, v, value=3.0):
    """the system with one more row that holds a diagonal entry only: the generators give even orders (n + n - 2, N (dof + ncon) with dof = ncon),
    and the lanes-per-row kernels must also meet an order that is no multiple of their lane count"""
    return n + 1, np.append(r, n + 1).astype(np.int32), np.append(c, n + 1).astype(np.int32), np.append(v, value)


def ruiz_systems():
    """name -> (n, r, c, v, variant the solver must pick).  Orders: 2004 (% 8 = 4), 2005 (odd, % 8 = 5), 799 (odd, % 8 = 7), 1197 (odd, % 8 = 5)."""
    from tests.support import kktgen
    out = {}
    out["lukvl_2lanes_fused"] = kktgen.lukvl_like(1003, seed=3)[:4] + (0,)
    out["lukvl_2lanes_fused_odd"] = with_isolated_row(*kktgen.lukvl_like(1003, seed=3)[:4]) + (0,)
    out["grid_8lanes_fused_odd"] = with_isolated_row(*kktgen.grid_kkt(21, 19, dof=1, ncon=1, seed=1)[:4]) + (1,)
    out["grid_8lanes_rowview_odd"] = kktgen.grid_kkt(21, 19, dof=2, ncon=1, seed=1)[:4] + (2,)
    return out


# name -> (nx, ns, nc, nxl, nxu, nsl, nsu, deltas, segs): the shapes of the primal-dual kernel tests (n4 = nx + 2 ns + nc, len8 = n4 + the bound counts)
PD_DELTAS = (1.0, 0.5, 1e-3, 2e-3)
PD_SHAPES = {
    "lukvle_no_s_no_bounds": (70, 0, 50, 0, 0, 0, 0, PD_DELTAS, [0, 3, 5]),
    "no_equalities":         (50, 6, 0, 20, 15, 4, 3, PD_DELTAS, [0, 3, 5]),
    "x_upper_only":          (50, 6, 10, 0, 21, 0, 0, PD_DELTAS, [0, 3, 5]),
    "x_all_two_sided":       (50, 6, 10, 50, 50, 3, 2, PD_DELTAS, [0, 3, 5]),
    "s_bounds_only":         (50, 6, 10, 0, 0, 6, 5, PD_DELTAS, [0, 3, 5]),
    "n4_63_len8_127":        (40, 5, 13, 30, 25, 5, 4, PD_DELTAS, [0, 3, 5]),
    "n4_64_len8_128":        (40, 5, 14, 30, 25, 5, 4, PD_DELTAS, [0, 3, 5]),
    "n4_65_len8_129":        (40, 5, 15, 30, 25, 5, 4, PD_DELTAS, [0, 3, 5]),
    "segs_5_0_3":            (45, 7, 9, 20, 10, 4, 4, PD_DELTAS, [5, 0, 3]),
    "delta_s_zero":          (45, 7, 9, 20, 10, 7, 7, (1.0, 0.0, 1e-3, 2e-3), [0, 3, 5]),
    "delta_d_zero":          (45, 7, 9, 20, 10, 7, 7, (1.0, 0.5, 1e-3, 0.0), [0, 3, 5]),
    "delta_s_and_d_zero":    (45, 7, 9, 20, 10, 7, 7, (1.0, 0.0, 1e-3, 0.0), [0, 3, 5]),
}
# the grid-stride case: grid1d caps a launch at 2048 x 256 = 524 288 threads; nxl and n4 are both beyond that
PD_LARGE = (560000, 8000, 20000, 560000, 0, 8000, 0, PD_DELTAS, [0, 3, 5])
PD_COEFFS = [(1.0, 0.0), (0.5, 0.0), (1.0, 1.0), (-1.0, 1.0), (0.3, 1.0), (0.5, 2.0)]


def pd_shape(name_or_tuple, seed=11):
    t = PD_SHAPES[name_or_tuple] if isinstance(name_or_tuple, str) else name_or_tuple
    return pd_problem(*t[:7], seed=seed), t[7], t[8]


def keep_fixture():
    """The fixture of test_device_side_assembly_equals_host_assembly_bitwise (tests/test_gpu_parity.py): nx = 300, m = 120,
    K = [[H + Sigma + dx I, J^T], [J, -dc I]] in the segment order  W | D_x | J_c | D_c."""
    rng = np.random.default_rng(5)
    nx, m = 300, 120
    hi = np.concatenate([np.arange(nx), np.arange(nx - 1)]); hj = np.concatenate([np.arange(nx), np.arange(1, nx)])
    hv = np.concatenate([4.0 + rng.random(nx), rng.uniform(-1, 1, nx - 1)])
    Sigma = 10.0 ** rng.uniform(-3, 3, nx)
    ji = np.repeat(np.arange(m), 3); jj = (2 * np.arange(m)[:, None] + np.arange(3)[None, :]).ravel(); jv = rng.uniform(-1, 1, 3 * m); jv[1::3] += 2.0
    r = np.concatenate([np.minimum(hi, hj), np.arange(nx), ji + nx, np.arange(m) + nx]).astype(np.int32) + 1
    c = np.concatenate([np.maximum(hi, hj), np.arange(nx), jj, np.arange(m) + nx]).astype(np.int32) + 1
    b = rng.standard_normal(nx + m)
    return dict(nx=nx, m=m, n=nx + m, r=r, c=c, hv=hv, Sigma=Sigma, jv=jv, b=b, lens=[len(hv), nx, len(jv), m], scale=[1.0, 1.0, 1.0, 0.0])


def keep_host_vals(F, dx, dc, srcs=None):
    hv, Sigma, jv = srcs if srcs is not None else (F["hv"], F["Sigma"], F["jv"])
    return np.concatenate([1.0 * hv, 1.0 * Sigma + dx, 1.0 * jv, np.full(F["m"], -dc)])


def keep_other_matrix(F, seed=17):
    """host values B: matrix A (dx = dc = 0 plus the given deltas) with the rows and columns of a random half scaled by 1e4"""
    rng = np.random.default_rng(seed)
    d = np.where(rng.random(F["n"]) < 0.5, 1e4, 1.0)
    return keep_host_vals(F, 1e-4, 1e-8) * d[F["r"] - 1] * d[F["c"] - 1]


# Ipopt's inertia-correction ladder (IpPDPerturbationHandler.cpp: delta_x from 1e-4 by factors of 100, delta_c = 1e-8 once the Jacobian is suspected)
KEEP_LADDER = [(1e-4 * 100.0 ** k, 1e-8 if k >= 2 else 0.0) for k in range(7)]


def gather_fixture():
    """A pattern whose positions carry 1, 2, 7 and 1000 duplicates (the last one the cancelling triple 1e16, 1, -1e16 repeated, then one 2^40: a multiple of every ulp met on the way, so no order of summation loses it and the block stays regular), each
    on a 1 x 1 diagonal block decoupled from everything else -- x = b / a reads the gathered sum off -- next to a small coupled block, given in a
    shuffled triplet order.  Returns (n, r, c, v, {row (0-based): the list of its duplicates in triplet order})."""
    rng = np.random.default_rng(23)
    groups = {0: [2.5], 1: [0.1, 0.2], 2: list(rng.uniform(-1, 1, 7) + 0.5), 3: [1e16, 1.0, -1e16] * 333 + [2.0 ** 40]}
    n = 8
    r, c, v = [], [], []
    for row, vals in groups.items():
        r += [row] * len(vals); c += [row] * len(vals); v += list(vals)
    for (i, j, a) in ((4, 4, 4.0), (5, 5, 5.0), (6, 6, -3.0), (7, 7, 6.0), (5, 4, 1.0), (4, 5, 0.5), (7, 6, 1.0), (6, 4, 0.25)):      # coupled block, both triangles, one duplicate position
        r.append(i); c.append(j); v.append(a)
    order = rng.permutation(len(v))
    r = np.array(r)[order]; c = np.array(c)[order]; v = np.array(v)[order]
    dup = {row: [float(x) for x in v[(r == row) & (c == row)]] for row in groups}
    return n, (r + 1).astype(np.int32), (c + 1).astype(np.int32), v.astype(np.float64), dup
