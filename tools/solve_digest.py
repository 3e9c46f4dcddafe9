"""Solve sweeps (kernels_solve.hip.inc): one SHA-256 per (fixture, leg) over the bytes of the solutions of the fixture's three right-hand sides, one
factorisation per leg.  Two builds whose sweeps compute the same thing write the same file: the yardstick of a change to the solve kernels that must
not move a bit (the factor kernels being the same, any difference is a solve kernel's).  The fixtures are the tests' own, the legs are chosen so that
every kernel of the file is launched at least once; each leg prints the reach facts (tests/support/reach.py) it stands on and is refused without them:
  bigfix   every fixture x its legs (sweeps / levels / groups): k_fwd_chain / k_bwd_chain, k_fwd_solo64, k_fwd_solo, k_fwd_grp + k_fwd_grp_upd,
           k_bwd_dot64 + k_bwd_fin64, k_bwd_grp_dot + k_bwd_grp
  midfix   every fixture, mid_solve on and off: k_fwd_mid / k_bwd_mid<1, 2>, k_fwd / k_bwd<64, 256>
  pathfix  lukvl1000, lukvl12000: default, MI355X_KKT_DISABLE=leafchain, =pair_solve.  lukvl12000: the leaf chains and k_fwd_pair / k_bwd_pair<16, 16>,
           then <16, 16> on the chains' levels too, then k_fwd / k_bwd<64> on the one-wavefront fronts.  lukvl1000 is small enough for ONE chain
           segment over all its levels: its three legs are the chain sweeps over one-wavefront fronts.
The one-wavefront fronts of the bigfix and midfix legs outside the chain segments go to the pair kernels as well: over all legs, each of
k_fwd_pair / k_bwd_pair<16, 16>, <16>, <32> must have been launched, as every kind of level launch of the big fronts.
usage: python tools/solve_digest.py out.json      (MI355X_KKT_LIBRARY selects the build)"""
import os, sys, json, hashlib
if len(sys.argv) != 2:
    sys.exit(__doc__)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch      # noqa: F401  (torch before the library is loaded: it brings its own HIP runtime)
import ipopt_amd
from ipopt_amd import kkt
from tests.support import bigfix, midfix, pathfix, reach as R

out, seen = {}, {}


def small_kinds(s):
    """what numeric.hip solve_sweep / solve_level launch for the one-wavefront fronts (order <= 32) under the knobs of the moment: the leaf chains, and per
    level outside them and outside the chain segments the instantiation of the pair kernels, or k_fwd / k_bwd<64> without pair_solve"""
    F = R.reach(s)
    nl = s.info().num_levels
    lv, lp = s.launch_plan("levels").reshape(-1, 10), s.symbolic(13, nl * R.FC_COUNT + 1)      # (columns 8, 9: largest order, most pivots of a one-wavefront front of the level)
    in_seg = np.zeros(nl, dtype=bool)
    for lv0, lv1, *_ in s.launch_plan("chain_segs").reshape(-1, 9):
        in_seg[lv0:lv1 + 1] = True
    kinds = {"leafchain": F["leafchain_solve"]}
    for q in range(F["leafchain_solve"], nl):
        if not in_seg[q] and lp[q * R.FC_COUNT + 1] > lp[q * R.FC_COUNT]:
            w = "wave64" if not F["pair_solve"] else "pair<16,16>" if lv[q, 8] <= 16 else "pair<16,32>" if lv[q, 9] <= 16 else "pair<32,32>"
            kinds[w] = kinds.get(w, 0) + 1
    assert F["pair_levels"] == sum(v for w, v in kinds.items() if w.startswith("pair")) and F["pair16_levels"] == kinds.get("pair<16,16>", 0)
    kinds["levels_in_chain_segments"] = int(in_seg.sum())
    return {w: v for w, v in kinds.items() if v}


def digest(ident, s, S, facts):
    """factor once, solve the three right-hand sides -> SHA-256 of the solution bytes"""
    facts = {**facts, **small_kinds(s)}
    for w, v in facts.items():
        seen[w] = seen.get(w, 0) + int(v)
    known = S["neg"] is not None
    s.values()[:] = S["v"]
    x = S["B"].copy()
    st = s.multi_solve(True, x, known, S["neg"] if known else 0)
    assert st == kkt.SUCCESS, (ident, st)
    out[ident] = hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()
    print(f"{ident} n={S['n']} {facts} {out[ident]}", flush=True)
    s.close()


for name, leg in bigfix.CASES:
    with bigfix.leg_knobs(leg):
        s = bigfix.handle(name, leg)
        F = R.solve_reach(s)
        fwd, bwd = F["fwd_solo64_levels"] + F["fwd_solo_levels"] + F["fwd_grp_levels"], F["bwd_dot64_levels"] + F["bwd_grp_levels"]
        # (a fixture need not reach every kernel of its leg; the leg's kind of launch it must)
        assert {"sweeps": F["segments"] >= 1 and F["chain_big_fronts"] > 0,
                "levels": F["segments"] == 0 and F["solve_group"] == 0 and F["unit_max_links"] == 1 and fwd > 0 and bwd > 0,
                "groups": F["segments"] == 0 and F["solve_group"] == 1 and F["unit_max_links"] > 1 and F["fwd_grp_levels"] == F["bwd_grp_levels"] > 0}[leg], (name, leg, F)
        digest(f"bigfix/{name}/{leg}", s, bigfix.system(name), {w: F[w] for w in ("chain_big_fronts", "fwd_solo64_levels", "fwd_solo_levels", "fwd_grp_levels", "bwd_dot64_levels", "bwd_grp_levels") if F[w]})
for name in midfix.FIXTURES:
    S = midfix.system(name)
    for mid_off in (False, True):
        with pathfix.knobs(midfix.disable_list(name, mid_off), S["tune"]):
            s = ipopt_amd.KKTSolver(**S["opts"])
            s.initialize_structure(S["n"], S["r"], S["c"], vals=S["v"])
            level, _, _ = midfix.mid_fronts(s)
            n64, n128 = sum(1 for f in level if f[0] == R.FC_LDS64), sum(1 for f in level if f[0] == R.FC_LDS128)
            assert s.info().maxsupernode <= 64 and n64 > 0 and n128 > 0, (name, n64, n128)      # solve_level's condition for k_fwd_mid / k_bwd_mid; both classes on level launches
            digest(f"midfix/{name}/{'plain' if mid_off else 'mid_solve'}", s, S, {("plain" if mid_off else "mid") + "_lds64_fronts": n64, ("plain" if mid_off else "mid") + "_lds128_fronts": n128})
for name in ("lukvl1000", "lukvl12000"):
    S = pathfix.system(name)
    for leg, disable in (("default", None), ("no_leafchain", "leafchain"), ("no_pair_solve", "pair_solve")):
        with pathfix.knobs(disable, S["tune"]):
            s = ipopt_amd.KKTSolver(**S["opts"])
            s.initialize_structure(S["n"], S["r"], S["c"], vals=S["v"])
            K, nl = small_kinds(s), s.info().num_levels
            if name == "lukvl1000":
                assert K == {"levels_in_chain_segments": nl}, (name, leg, K)
            else:
                assert {"default": K.get("leafchain", 0) > 0 and K.get("pair<16,16>", 0) > 0,
                        "no_leafchain": "leafchain" not in K and K.get("pair<16,16>", 0) > 1,
                        "no_pair_solve": "leafchain" not in K and K.get("wave64", 0) > 1 and not any(w.startswith("pair") for w in K)}[leg], (name, leg, K)
            digest(f"pathfix/{name}/{leg}", s, S, {})
print("over all legs:", seen)
need = ["chain_big_fronts", "fwd_solo64_levels", "fwd_solo_levels", "fwd_grp_levels", "bwd_dot64_levels", "bwd_grp_levels", "mid_lds64_fronts", "mid_lds128_fronts",
        "plain_lds64_fronts", "plain_lds128_fronts", "leafchain", "pair<16,16>", "pair<16,32>", "pair<32,32>", "wave64"]
assert all(seen.get(w, 0) > 0 for w in need), [w for w in need if not seen.get(w, 0)]
path = sys.argv[1]
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
