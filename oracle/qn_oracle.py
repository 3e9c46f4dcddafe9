"""Reader of the quasi-Newton recordings -- TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product.  Plain numpy / scipy.

  * read_qnrec(): the recordings `oracle/ref_driver --record-qn` makes of the UNMODIFIED reference run with `hessian_approximation
    limited-memory`: per UpdateHessian call the pair (s, y) the updater formed and the W = diag + V V^T - U U^T it left in IpData().W();
    per Solve of the low-rank augmented-system solver everything it was given and what it returned.  Fixtures in tests/golden/*.qnrec;
    the layout is stated above the recording classes of oracle/ref_driver.cpp.
  * aug_matrix(): the symmetric 4-block matrix of a solve record WITHOUT the low-rank term, signs of IpAugSystemSolver.hpp:20-31:
        [ W_factor diag + D_x + delta_x I        0               J_c^T            J_d^T      ]
        [             0                  D_s + delta_s I          0                -I        ]
        [            J_c                         0         D_c - delta_c I          0        ]
        [            J_d                        -I                0          D_d - delta_d I ]
  * dense_updated(): aug_matrix() + W_factor (V V^T - U U^T) on the x block, dense: the matrix the recorded solve answered.
"""
from __future__ import annotations

import numpy as np

UPDATE_TYPE = ("bfgs", "sr1")
INIT = ("scalar1", "scalar2", "scalar3", "scalar4", "constant")
SUCCESS = 0                                         # ESymSolverStatus SYMSOLVER_SUCCESS


def read_qnrec(path):
    """-> (header dict, update records, solve records)"""
    raw = open(path, "rb").read()
    assert raw[:7] == b"QNREC1\n", "not a QNREC1 file"
    off = 7

    def take(fmt, count):
        nonlocal off
        dt = np.dtype(fmt)
        a = np.frombuffer(raw, dtype=dt, count=count, offset=off).copy()
        off += count * dt.itemsize
        return a

    h = take("<i4", 8)
    v = take("<f8", 3)
    header = dict(update_type=UPDATE_TYPE[int(h[0])], max_history=int(h[1]), initialization=INIT[int(h[2])], max_skipping=int(h[3]),
                  nx=int(h[4]), p_lowrank_null=bool(h[5]), init_val=float(v[0]), sigma_min=float(v[1]), sigma_max=float(v[2]))
    if not header["p_lowrank_null"]:
        raise ValueError(f"{path}: recorded with a P_LowRank: the update lives in a subspace of x, which this reader does not restate")
    nx = header["nx"]
    cols = lambda k: take("<f8", k * nx).reshape(k, nx).T.copy()      # (nx, k), one recorded vector per column
    updates, solves = [], []
    while off < len(raw):
        tag = int(np.frombuffer(raw, dtype="<i4", count=1, offset=off)[0])
        if tag == 1:
            h = take("<i4", 8)
            assert int(h[1]) == nx
            sc = take("<f8", 2)
            r = dict(has_pair=bool(h[2]), nv=int(h[3]), nu=int(h[4]), w_changed=bool(h[5]), iter=int(h[7]), amax_s=float(sc[0]), regu_x=float(sc[1]))
            r["s"], r["y"] = (take("<f8", nx), take("<f8", nx)) if r["has_pair"] else (None, None)
            r["diag"], r["V"], r["U"] = take("<f8", nx), cols(r["nv"]), cols(r["nu"])
            r["info"] = raw[off:off + int(h[6])].decode("ascii"); off += int(h[6])
            updates.append(r)
        elif tag == 2:
            h = [int(x) for x in take("<i4", 20)]
            assert h[1] == nx
            sc = take("<f8", 5)
            r = dict(nx=nx, ns=h[2], nc=h[3], nd=h[4], nv=h[5], nu=h[6], check_neg=bool(h[13]), num_neg=h[14], status=h[15], neg_after=h[16], iter=h[17],
                     W_factor=float(sc[0]), delta_x=float(sc[1]), delta_s=float(sc[2]), delta_c=float(sc[3]), delta_d=float(sc[4]))
            r["diag"], r["V"], r["U"] = take("<f8", nx), cols(h[5]), cols(h[6])
            for name, n in (("D_x", h[7]), ("D_s", h[8]), ("D_c", h[9]), ("D_d", h[10])):
                r[name] = take("<f8", n)                                                             # length 0: absent
            for name, n in (("Jc", h[11]), ("Jd", h[12])):
                r[name] = (take("<i4", n), take("<i4", n), take("<f8", n))                           # 1-based (row, col, value)
            n4 = nx + r["ns"] + r["nc"] + r["nd"]
            r["rhs"], r["sol"] = take("<f8", n4), take("<f8", n4)
            solves.append(r)
        else:
            raise ValueError(f"{path}: unknown record tag {tag} at byte {off}")
    return header, updates, solves


def aug_matrix(rec):
    """-> (n, irow, jcol, vals, K): the 4-block matrix as 1-based lower triplets (every diagonal entry present) and as a scipy csc matrix"""
    import scipy.sparse as sp
    nx, ns, nc, nd = rec["nx"], rec["ns"], rec["nc"], rec["nd"]
    n = nx + ns + nc + nd
    ox, os_, oc, od = 0, nx, nx + ns, nx + ns + nc

    def diag(base, D, shift, m):
        d = np.array(base, dtype=np.float64, copy=True) if base is not None else np.zeros(m)
        if len(D):
            d = d + D
        return d + shift

    d = np.concatenate([diag(rec["W_factor"] * rec["diag"], rec["D_x"], rec["delta_x"], nx), diag(None, rec["D_s"], rec["delta_s"], ns),
                        diag(None, rec["D_c"], -rec["delta_c"], nc), diag(None, rec["D_d"], -rec["delta_d"], nd)])
    ar = np.arange(1, n + 1)
    rows, colsx, vals = [ar], [ar], [d]
    for (r_, c_, v_), o in ((rec["Jc"], oc), (rec["Jd"], od)):
        rows.append(r_.astype(np.int64) + o); colsx.append(c_.astype(np.int64) + ox); vals.append(v_)
    rows.append(od + np.arange(1, nd + 1)); colsx.append(os_ + np.arange(1, ns + 1)); vals.append(-np.ones(nd))      # (nd = ns)
    irow, jcol, v = np.concatenate(rows).astype(np.int32), np.concatenate(colsx).astype(np.int32), np.concatenate(vals)
    L = sp.coo_matrix((v, (irow - 1, jcol - 1)), shape=(n, n)).tocsc()
    K = L + sp.tril(L, -1).T
    return n, irow, jcol, v, K.tocsc()


def dense_updated(rec):
    """the dense matrix of the recorded solve: aug_matrix + W_factor (V V^T - U U^T) on the x block"""
    K = aug_matrix(rec)[4].toarray()
    nx = rec["nx"]
    K[:nx, :nx] += rec["W_factor"] * (rec["V"] @ rec["V"].T - rec["U"] @ rec["U"].T)
    return K
