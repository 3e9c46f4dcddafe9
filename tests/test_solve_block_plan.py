"""Host only (no device): the solve-block schedule "solve.single.block" (launch_plan.cpp build_solve_block_schedule) of every row of the table of
tests/test_gpu_solve_block.py against the restatement of its rules in tests/support/blockfix.py -- L*, the kind and the kernel of every record, grids and
list offsets equal to what numeric.hip solve_level would launch --, and the counts per row pinned as the reach tests pin theirs: a change of the ordering
or of a threshold fails here and does not silently empty a GPU test."""
import numpy as np
import pytest

from tests.support import blockfix as BF, reach as R

# row -> (L*, levels, (blocked launches, launches by column, top launches per column) of one full block, records per kernel: blocked / by column / top)
CHAIN_TOP = {"bump_epoch": 1, "fwd_chain": 1, "bwd_chain": 1}
PINNED = {
    "leaf_edges.levels": (33, 62, (36, 0, 3), {"fwd_leafchain": 1, "fwd_pair16x16": 11, "fwd_pair16": 6, "bwd_pair16x16": 11, "bwd_pair16": 6, "bwd_leafchain": 1}, {}, CHAIN_TOP),
    "leaf_edges_w8.levels": (13, 22, (16, 0, 3), {"fwd_leafchain": 1, "fwd_pair16": 3, "fwd_pair16x16": 4, "bwd_pair16x16": 4, "bwd_pair16": 3, "bwd_leafchain": 1}, {}, CHAIN_TOP),
    "wave_edges.levels": (3, 3, (6, 0, 0), {"fwd_pair32": 3, "bwd_pair32": 3}, {}, {}),
    "leaf_edges.default": (0, 62, (0, 0, 3), {}, {}, CHAIN_TOP),
    "leaf_edges.nopair": (33, 62, (0, 264, 3), {}, {"fwd_wave": 33, "bwd_wave": 33}, CHAIN_TOP),
    "mid_edges": (4, 4, (14, 0, 0), {"fwd_mid1": 2, "fwd_mid2": 3, "fwd_pair32": 1, "fwd_pair16x16": 1, "bwd_pair16x16": 1, "bwd_pair32": 1, "bwd_mid2": 3, "bwd_mid1": 2}, {}, {}),
    "mid_edges.nomid": (4, 4, (4, 40, 0), {"fwd_pair32": 1, "fwd_pair16x16": 1, "bwd_pair16x16": 1, "bwd_pair32": 1},
                        {"fwd_lds64": 2, "fwd_lds128": 3, "bwd_lds128": 3, "bwd_lds64": 2}, {}),
    "grid48x44": (2, 16, (8, 16, 3), {"fwd_mid1": 2, "fwd_mid2": 2, "bwd_mid1": 2, "bwd_mid2": 2}, {"fwd_grp": 1, "fwd_grp_upd": 1, "bwd_dot64": 1, "bwd_fin64": 1}, CHAIN_TOP),
    "hostile16": (14, 14, (20, 148, 0), {"fwd_pair16": 1, "fwd_mid1": 2, "fwd_mid2": 6, "fwd_pair32": 1, "bwd_pair32": 1, "bwd_mid2": 6, "bwd_mid1": 2, "bwd_pair16": 1},
                  {"fwd_grp": 7, "fwd_grp_upd": 7, "fwd_solo64": 3, "bwd_dot64": 10, "bwd_fin64": 10}, {}),
    "tails.levels": (8, 8, (10, 76, 0), {"fwd_mid2": 3, "fwd_pair16x16": 2, "bwd_pair16x16": 2, "bwd_mid2": 3},
                     {"fwd_solo64": 5, "fwd_grp": 1, "fwd_grp_upd": 1, "bwd_dot64": 6, "bwd_fin64": 6}, {}),
    "star6.groups": (7, 7, (4, 32, 0), {"fwd_mid2": 1, "fwd_pair16x16": 1, "bwd_pair16x16": 1, "bwd_mid2": 1}, {"fwd_grp": 2, "fwd_grp_upd": 2, "bwd_grp_dot": 2, "bwd_grp": 2}, {}),
    "chain_delayed.levels": (12, 12, (6, 108, 0), {"fwd_mid2": 1, "fwd_mid1": 2, "bwd_mid1": 2, "bwd_mid2": 1}, {"fwd_solo64": 9, "bwd_dot64": 9, "bwd_fin64": 9}, {}),
}


@pytest.mark.parametrize("row", sorted(BF.ROWS))
def test_the_schedule_is_the_restated_rules_and_the_pinned_counts(row):
    assert sorted(PINNED) == sorted(BF.ROWS)
    with BF.knobs(row):
        s = BF.handle(row)
        rec, ls, counts = BF.expected(s)
        got = [tuple(int(x) for x in r) for r in BF.schedule(s)]
        F = BF.facts(s)
        s.close()
    assert len(got) == len(rec)
    for q, (g, e) in enumerate(zip(got, rec)):
        assert g == e, f"record {q}: {BF.OP_NAMES[g[R.OP]]} {g} against {BF.OP_NAMES[e[R.OP]]} {e}"
    assert (F["first_top_level"], F["counts"]) == (ls, counts)
    assert (F["first_top_level"], F["num_levels"], F["counts"], F["blocked"], F["bycol"], F["top"]) == PINNED[row]


def test_the_order_of_a_block_bulk_forward_top_bulk_backward():
    """grid48x44: blocked and by-column levels below live chain sweeps -- the records of the top part stand together, between the forward and the backward
    records of the bulk, and the bulk's backward half mirrors its forward half level by level"""
    with BF.knobs("grid48x44"):
        s = BF.handle("grid48x44")
        recs = BF.schedule(s)
        s.close()
    kind = recs[:, R.STREAM]
    top = np.nonzero(kind == BF.SB_TOP)[0]
    assert len(top) == 3 and np.array_equal(top, np.arange(top[0], top[0] + 3)) and recs[top[0], R.OP] == BF.SO_BUMP_EPOCH
    fwd, bwd = recs[:top[0]], recs[top[-1] + 1:]
    assert len(fwd) == len(bwd) > 0 and list(fwd[:, R.LV]) == sorted(fwd[:, R.LV]) and list(bwd[:, R.LV]) == sorted(bwd[:, R.LV], reverse=True)
    assert fwd[:, R.LV].max() < recs[top[0], R.LV] == 2
