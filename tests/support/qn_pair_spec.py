"""Specification of the quasi-Newton pair (s, y) the device forms from the resident Jacobians (mi355x_kkt_qn_pair_*; reference
IpLimMemQuasiNewtonUpdater.cpp:276-308), in plain numpy:

    s = x - x_last
    y = (gf - gf_last) + J_c^T y_c + J_d^T y_d - J_c,last^T y_c - J_d,last^T y_d          (the restoration variant drops the gf term: ypart)

pair_ld     s and y in np.longdouble from the float64 inputs, with the difference taken PER ENTRY, (J_cur[t] - J_last[t]) * lam[i]: what the device
            computes, in higher precision
pair_ref64  the float64 transcription of the REFERENCE's order: s by :282; y by :297-300 (restoration: four TransMultVector calls accumulating into y in
            triplet order, alpha = 1, 1, -1, -1) or :304-307 (y = gf - gf_last; += the two current products, each formed on its own from zero; then the
            two old ones subtracted entry by entry)
bound       (k_j + 4) 2^-52 (|gf_j| + |gf_last_j| + sum_t (|J_cur[t]| + |J_last[t]|) |lam[i_t]|), k_j the entries of column j.  Derived, not measured: one
            rounding per difference, one per product, k_j additions and the gradient difference with unit roundoff 2^-53 give (k_j + 3) 2^-53 mag to
            first order; 2^-52 in its place leaves a factor 2.  The reference's order has at most 2 k_j + 2 additions and satisfies it as well.

A case is a dict: nx, ns, nc, nd; jc, jd = (rows, cols) 0-based inside their block (duplicates allowed); jc_upper (the J_c triplets are handed over as
(x index, c index)); Jc_last, Jc_cur, Jd_last, Jd_cur; x_last, x, gf_last, gf; yc, yd.  INPUTS() yields every case the GPU tests use, so that
tests/test_qn_pair_spec.py holds pair_ref64 to the bound on exactly those."""
import os

import numpy as np

LD = np.longdouble
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")


def _blocks(c):
    """[(rows, cols, J_cur, J_last, lam)] for J_c, J_d"""
    return [(c["jc"][0], c["jc"][1], c["Jc_cur"], c["Jc_last"], c["yc"]), (c["jd"][0], c["jd"][1], c["Jd_cur"], c["Jd_last"], c["yd"])]


def pair_ld(c, resto=False):
    s = c["x"].astype(LD) - c["x_last"].astype(LD)
    y = np.zeros(c["nx"], dtype=LD) if resto else c["gf"].astype(LD) - c["gf_last"].astype(LD)
    for r, col, cur, last, lam in _blocks(c):
        np.add.at(y, col, (cur.astype(LD) - last.astype(LD)) * lam.astype(LD)[r])
    return s, y


def _tmult(y, alpha, r, col, val, lam):
    """GenTMatrix::TransMultVector(alpha, lam, 1, y): y[col] += alpha * val * lam[row], triplet by triplet (np.add.at accumulates in index order)"""
    np.add.at(y, col, (alpha * val) * lam[r])


def pair_ref64(c, resto=False):
    nx = c["nx"]
    s = c["x"] - c["x_last"]                                                         # :282
    (rc, cc, Jc, Jcl, yc), (rd, cd, Jd, Jdl, yd) = _blocks(c)
    if resto:                                                                        # :297-300
        y = np.zeros(nx)
        _tmult(y, 1.0, rc, cc, Jc, yc); _tmult(y, 1.0, rd, cd, Jd, yd)
    else:                                                                            # :304-305
        y = c["gf"] - c["gf_last"]
        a, b = np.zeros(nx), np.zeros(nx)
        _tmult(a, 1.0, rc, cc, Jc, yc); _tmult(b, 1.0, rd, cd, Jd, yd)
        y = (y + a) + b
    _tmult(y, -1.0, rc, cc, Jcl, yc); _tmult(y, -1.0, rd, cd, Jdl, yd)               # :299-300 / :306-307
    return s, y


def bound(c, resto=False):
    nx = c["nx"]
    mag = np.zeros(nx) if resto else np.abs(c["gf"]) + np.abs(c["gf_last"])
    k = np.zeros(nx)
    for r, col, cur, last, lam in _blocks(c):
        np.add.at(mag, col, (np.abs(cur) + np.abs(last)) * np.abs(lam)[r])
        np.add.at(k, col, 1.0)
    return (k + 4.0) * 2.0 ** -52 * mag


def column_lengths(c):
    return np.bincount(np.concatenate([c["jc"][1], c["jd"][1]]).astype(np.int64), minlength=c["nx"])


def expected_lpc(c):
    """the rule of qn_pair_host.h qp_pick_lpc, restated: which instantiation a case must reach"""
    k = column_lengths(c)
    return 64 if k.size and k.max() > 256 else 1 if k.sum() < 4 * c["nx"] else 8


def fill(c, seed, decades=0.0, unchanged=0.3):
    """seeded values for a structure: Jacobians of which a share did not change, multipliers with zeros and both signs, magnitudes over `decades` decades"""
    rng = np.random.default_rng(seed)
    mag = lambda k: 10.0 ** rng.uniform(-decades / 2, decades / 2, k) if decades else np.ones(k)
    for b in ("jc", "jd"):
        k = len(c[b][0])
        last = rng.standard_normal(k) * mag(k)
        cur = np.where(rng.random(k) < unchanged, last, last + rng.standard_normal(k) * mag(k) * 0.1)
        c["J" + b[1] + "_last"], c["J" + b[1] + "_cur"] = last, cur
    nx = c["nx"]
    c["x_last"] = rng.standard_normal(nx) * mag(nx); c["x"] = c["x_last"] + 1e-2 * rng.standard_normal(nx)
    c["gf_last"] = rng.standard_normal(nx) * mag(nx); c["gf"] = c["gf_last"] + 1e-1 * rng.standard_normal(nx) * mag(nx)
    for name, k in (("yc", c["nc"]), ("yd", c["nd"])):
        lam = rng.standard_normal(k) * mag(k)
        lam[rng.random(k) < 0.2] = 0.0
        if k >= 3:                                                                   # (a zero and both signs in every block, whatever the draw)
            lam[0], lam[k // 2], lam[k - 1] = abs(lam[0]) + 0.5, 0.0, -abs(lam[k - 1]) - 0.5
        c[name] = lam
    return c


def _structure(name, nx, nc, nd, jc, jd, jc_upper=False):
    as_idx = lambda rc: (np.asarray(rc[0], dtype=np.int64), np.asarray(rc[1], dtype=np.int64))
    return dict(name=name, nx=nx, ns=nd, nc=nc, nd=nd, jc=as_idx(jc), jd=as_idx(jd), jc_upper=jc_upper)


def random_case(name, nx, nc, nd, per_row, seed, dup=0, jc_upper=False):
    """every row of J_c and J_d holds min(nx, per_row) distinct columns; dup: that many J_c triplets repeated at the end of the segment"""
    rng = np.random.default_rng(1000 + seed)
    def rect(m):
        r, c = [], []
        for i in range(m):
            for j in rng.choice(nx, size=min(nx, per_row), replace=False):
                r.append(i); c.append(int(j))
        return r, c
    jc, jd = rect(nc), rect(nd)
    for q in range(min(dup, len(jc[0]))):
        jc[0].append(jc[0][3 * q % len(jc[0])]); jc[1].append(jc[1][3 * q % len(jc[1])])
    return fill(_structure(name, nx, nc, nd, jc, jd, jc_upper), seed)


def columns_case(seed=7):
    """columns of 0, 1, 64, 65, 257 and 300 entries (and two short ones): J_c has 200 rows, J_d 100; a column of k entries takes the first min(k, 200)
    rows of J_c and the first k - 200 of J_d.  Magnitudes over six decades."""
    lens = [0, 1, 64, 65, 257, 300, 3, 2]
    nc, nd = 200, 100
    jc, jd = ([], []), ([], [])
    for i in range(nc):                                                              # (row by row: the entries of a column are NOT contiguous in the segment)
        for j, k in enumerate(lens):
            if i < min(k, nc):
                jc[0].append(i); jc[1].append(j)
    for i in range(nd):
        for j, k in enumerate(lens):
            if i < k - nc:
                jd[0].append(i); jd[1].append(j)
    return fill(_structure("columns", len(lens), nc, nd, jc, jd), seed, decades=6.0)


RECORDED = [("qn_bfgs_180", 0, 1), ("qn_bfgs_180", 1, 2), ("qn_sr1_180", 0, 1), ("qn_bfgs_517", 0, 1)]


def recorded_solves(name):
    """the first solve record of every iteration of a fixture, by iteration"""
    from oracle import qn_oracle as qn
    by_iter = {}
    for rec in qn.read_qnrec(os.path.join(GOLDEN, name + ".qnrec"))[2]:
        by_iter.setdefault(rec["iter"], rec)
    return by_iter


def recorded_case(name, it0, it1, seed=11):
    """J_c / J_d of the solve records of two consecutive iterations as J_last and J_cur.  The recordings hold neither grad_f nor the multipliers (the recorded
    y cannot be re-formed from them): x, grad_f and the multipliers are seeded random"""
    recs = recorded_solves(name)
    a, b = recs[it0], recs[it1]
    for blk in ("Jc", "Jd"):
        assert np.array_equal(a[blk][0], b[blk][0]) and np.array_equal(a[blk][1], b[blk][1]), "the structure of the Jacobians changed between the iterations"
    c = _structure(f"{name}:{it0}->{it1}", a["nx"], a["nc"], a["nd"], (a["Jc"][0] - 1, a["Jc"][1] - 1), (a["Jd"][0] - 1, a["Jd"][1] - 1))
    fill(c, seed)
    c["Jc_last"], c["Jc_cur"], c["Jd_last"], c["Jd_cur"] = a["Jc"][2].copy(), b["Jc"][2].copy(), a["Jd"][2].copy(), b["Jd"][2].copy()
    c["ns"] = a["ns"]
    return c


def SHAPES():
    """the synthetic cases of the GPU tests: every nx at which the kernel can go wrong, every instantiation, absent blocks, duplicates, the upper orientation"""
    yield random_case("nx1", 1, 5, 3, 7, seed=1)
    yield random_case("nx63", 63, 5, 3, 7, seed=2)
    yield random_case("nx64", 64, 5, 3, 40, seed=3)
    yield random_case("nx65", 65, 5, 3, 7, seed=4)
    yield random_case("nx257", 257, 6, 2, 200, seed=5)
    yield columns_case()
    yield random_case("nc0", 40, 0, 6, 30, seed=6)
    yield random_case("nd0", 40, 6, 0, 5, seed=7)
    yield random_case("duplicates", 33, 7, 4, 20, seed=8, dup=25)
    yield random_case("jc_upper", 50, 9, 5, 12, seed=9, jc_upper=True)


def INPUTS():
    yield from SHAPES()
    for name, it0, it1 in RECORDED:
        yield recorded_case(name, it0, it1)


def system(c):
    """the 4-block KKT triplets of a case, as tests/test_gpu_pd_system.py builds them: segments W | D_x | D_s | J_c | D_c | J_d | -I | D_d (W: the diagonal
    alone) -> (n, irn, jcn (1-based), segment lengths, vals of an unperturbed positive-definite-on-x system)"""
    nx, ns, nc, nd = c["nx"], c["ns"], c["nc"], c["nd"]
    ar = lambda n, o: np.arange(n, dtype=np.int64) + o
    jr, jc_ = c["jc"][0] + nx + ns, c["jc"][1]
    if c["jc_upper"]:
        jr, jc_ = jc_, jr
    irn = np.concatenate([ar(nx, 0), ar(nx, 0), ar(ns, nx), jr, ar(nc, nx + ns), c["jd"][0] + nx + ns + nc, ar(nd, nx + ns + nc), ar(nd, nx + ns + nc)]) + 1
    jcn = np.concatenate([ar(nx, 0), ar(nx, 0), ar(ns, nx), jc_, ar(nc, nx + ns), c["jd"][1], ar(ns, nx), ar(nd, nx + ns + nc)]) + 1
    lens = [nx, nx, ns, len(jr), nc, len(c["jd"][0]), ns, nd]
    return nx + ns + nc + nd, irn.astype(np.int32), jcn.astype(np.int32), lens


SEG_JC, SEG_JD = 3, 5
