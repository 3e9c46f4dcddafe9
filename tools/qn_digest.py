"""Quasi-Newton histories (mi355x_kkt_lbfgs_*): a fixed script of pushes, one SHA-256 per step over every bit the history shows -- lbfgs_get S, Y, V, U,
D, L, STS (a restoration-phase history: and G, R, eta_col, dv), sigma, nneg, E, eta, the outcome, and one lowrank_solve of a fixed right-hand side
after factor + lowrank_update.  Two builds compute the same thing exactly when their outputs are the same file: the yardstick of a change that must
not move a bit, which the tests' bounds against the specifications would not notice.
  kinds        BFGS; SR1 with one undo in the middle; restoration BFGS and SR1, special 0 and 1; BFGS driven to a Cholesky failure (NOT_POSDEF)
  max_history  1, 8, 9, 16, 17, 32: both sides of the unroll bounds 8 / 16 / 32; max_history + 2 stored pushes, so the ring has wrapped
  rows         1 (one thread), 255, 257 (the partial last workgroup of the form kernels), 1025, 2500 (a partial last slab, several slabs of the dots)
  ways         host vectors; device vectors; a non-identity row map with mapped pushes (host and device x-block vectors in turn)
Every history also gets a skipped push (a NaN entry; BFGS: a pair failing the curvature test as well).  The handles are those of
tests/test_gpu_lbfgs.py: the x diagonal appears a second time, as duplicate triplets that carry B0.
Every step's hash goes to stdout; the file holds, per history, the outcomes and the SHA-256 over its steps' hashes.
usage: python tools/qn_digest.py [out.json]      (default profiles/qn_digest.json)"""
import os, sys, json, hashlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import ipopt_amd
from ipopt_amd import kkt
from tests.support import kktgen, lbfgs_spec as lb, sr1_spec as sr, resto_spec as rs, rowmap_spec as rm

KINDS = [("bfgs", 0, None), ("sr1", 1, None), ("resto_bfgs", 0, False), ("resto_bfgs_special", 0, True), ("resto_sr1", 1, False), ("resto_sr1_special", 1, True)]
HISTORIES, ROWS, WAYS = [1, 8, 9, 16, 17, 32], [1, 255, 257, 1025, 2500], ["host", "device", "mapped"]
BASE = ("S", "Y", "V", "U", "D", "L", "STS")
RESTO = ("G", "R", "eta_col", "dv")


class Handle:
    """an analysed handle whose n_x = rows + 40 x entries all have a duplicate diagonal triplet; the history lives on the first `rows` of them, or on a map"""
    def __init__(self, rows):
        self.rows, self.nx = rows, rows + 40
        n, r, c, v, self.m = kktgen.lukvl_like(self.nx)
        ix = np.arange(1, self.nx + 1).astype(r.dtype)
        self.n, self.v = n, v
        self.s = ipopt_amd.KKTSolver()
        self.s.initialize_structure(n, np.concatenate([r, ix]), np.concatenate([c, ix]), vals=np.concatenate([v, np.ones(self.nx)]))
        self.b = np.random.default_rng(5).standard_normal(n)
        self.idx = rm.make_idx(self.nx, rows)
        self.fill = np.random.default_rng(6).standard_normal((2, self.nx))      # what a mapped push carries outside the map

    def place(self, way):
        self.s.lbfgs_clear(); self.s.lowrank_clear()
        self.s.lowrank_rowmap(self.idx if way == "mapped" else None)
        self.where = self.idx if way == "mapped" else np.arange(self.rows)

    def chain(self, b0):
        """factor K + B0 on the history's rows, lowrank_update, one solve -> what of it there is"""
        s = self.s
        if s.lowrank_info()["rows"] == 0:
            return [b"no update"]
        d = np.zeros(self.nx); d[self.where] = b0
        s.values()[:] = np.concatenate([self.v, d])
        st = s.multi_solve(True, None, True, self.m)
        if st != kkt.SUCCESS:
            return [b"factor %d" % st]
        st, which = s.lowrank_update()
        if st != kkt.SUCCESS or which != 0:
            return [b"update %d %d" % (st, which)]
        x = self.b.copy(); s.lowrank_solve(x)
        return [b"solved", x.tobytes()]


def script(kind, rows, k):
    """-> the steps (s, y, eta) or "undo" of one history, and DR"""
    name, sr1, special = kind
    n = k + 2
    if special is None:
        Sp, Yp = (sr if sr1 else lb).make_pairs(rows, n, seed=40 + rows + k); DR = None
    else:
        Sp, Yp, DR = rs.make_resto(rows, n, seed=40 + rows + k, sr1=bool(sr1))
    steps = [(Sp[:, j], Yp[:, j], rs.ETAS[j % 4]) for j in range(n)]
    ynan = Yp[:, 1].copy(); ynan[rows // 2] = np.nan
    extra = (["undo"] if sr1 else []) + [(Sp[:, 1], ynan, 0.3)] + ([(Sp[:, 1], -Yp[:, 1], 0.3)] if name == "bfgs" else [])      # (a skip would leave nothing to undo)
    at = n // 2 + 1
    return steps[:at] + extra + steps[at:], DR


def not_posdef_script(rows):
    """tests/test_gpu_lbfgs.py: init constant 1e8, s = e_1, y = 1e-9 e_1 twice: the second pivot of M is exactly 0"""
    e1 = np.zeros(rows); e1[0] = 1.0
    return [(e1, 1e-9 * e1, 0.3)] * 2


def run(H, kind, k, way, steps, DR, **define):
    name, sr1, special = kind
    s, rows = H.s, H.rows
    s.lbfgs_clear(); s.lowrank_clear()
    if special is not None:
        s.lbfgs_define_resto(rows, DR, max_history=k, type=sr1, special=special)
    elif sr1:
        s.lbfgs_define_sr1(rows, max_history=k)
    else:
        s.lbfgs_define(rows, max_history=k, **define)
    ident = f"{name}/k{k}/rows{rows}/{way}"
    hashes, outcomes = [], ""
    for j, step in enumerate(steps):
        if isinstance(step, str):
            oc = 10 + s.lbfgs_undo()
        else:
            sv, yv, eta = step
            if way == "mapped":
                sx, yx = H.fill[0].copy(), H.fill[1].copy(); sx[H.idx] = sv; yx[H.idx] = yv
                sv, yv = sx, yx
            args, on_device = [sv, yv], way == "device" or (way == "mapped" and j % 2 == 1)
            if on_device:
                dev = [torch.tensor(a, dtype=torch.float64, device="cuda") for a in args]
                torch.cuda.synchronize()
                args = [d.data_ptr() for d in dev] + ([H.nx] if way == "mapped" else [])
            call = "lbfgs_push" + ("_resto" if special is not None else "") + ("_mapped" if way == "mapped" else "") + ("_device" if on_device else "")
            oc = getattr(s, call)(*args, *([eta] if special is not None else []))
        I, Q, R = s.lbfgs_info(), s.lbfgs_sr1_info(), s.lbfgs_resto_info()
        b0 = R["eta"] * DR if R["special"] else I["sigma"]
        parts = [s.lbfgs_get(w).tobytes(order="F") for w in BASE + (RESTO if special is not None else ())]
        parts += [np.array([I["sigma"], R["eta"]]).tobytes(), np.array([oc, I["memory"], I["skipped_in_a_row"], Q["nneg"], Q["can_undo"]]).tobytes(), Q["E"].tobytes()] + H.chain(b0)
        h = hashlib.sha256()
        for p in parts:
            h.update(len(p).to_bytes(8, "little")); h.update(p)
        hashes.append(h.hexdigest()); outcomes += str(oc) + " "
        print(f"{ident}/{j} {oc} {hashes[-1]}", flush=True)
    return ident, {"outcomes": outcomes.strip(), "sha256": hashlib.sha256("".join(hashes).encode()).hexdigest()}


out = {}
for rows in ROWS:
    H = Handle(rows)
    for way in WAYS:
        H.place(way)
        for kind in KINDS:
            for k in HISTORIES:
                steps, DR = script(kind, rows, k)
                ident, res = run(H, kind, k, way, steps, DR)
                out[ident] = res
        ident, res = run(H, ("bfgs_not_posdef", 0, None), 4, way, not_posdef_script(rows), None, init="constant", init_val=1e8)
        assert res["outcomes"] == f"{kkt.LBFGS_STORED} {kkt.LBFGS_NOT_POSDEF}", res
        out[ident] = res
    H.s.close()
assert sum(r["outcomes"].count("11") for r in out.values()) == len(ROWS) * len(WAYS) * 3 * len(HISTORIES), "every SR1 history takes one push back"
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "qn_digest.json")
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
