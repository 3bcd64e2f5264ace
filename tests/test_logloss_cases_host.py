"""Host-side checks of the workloads in tests/logloss_cases.py, so that tests/test_gpu_logloss_k.py tests what it
says: every class of row (1 slot, 2-16, 17-256, more than 256) is present in every step it replays, the tile counts
are the intended ones, a single dropped gradient slot would be seen, and the stored fp32-vs-fp64 deviations the table
bounds are built from are still what the oracle gives."""
import numpy as np
import pytest

import logloss_cases as LC

NAMES = [c.name for c in LC.CASES]
N_ROWS = 16296


def test_case_table():
    assert [(c.name, c.B, c.K, c.d, LC.units(c), c.tiles) for c in LC.CASES] == [
        ("one_tile_full", 16, 255, 50, 4096, 1), ("tile_plus_one", 17, 240, 50, 4097, 2),
        ("tile_plus_k1024", 4, 1024, 64, 4100, 2), ("two_tiles_exact", 32, 255, 200, 8192, 2),
        ("config5_small", 64, 256, 50, 16448, 5), ("k16_edge", 241, 16, 50, 4097, 2)]
    assert LC.type_arrays()[0].entity_count == N_ROWS


@pytest.mark.parametrize("name", NAMES)
def test_every_row_class_in_every_step(name):
    c = LC.BY_NAME[name]
    M = LC.units(c)
    assert -(-M // LC.SUB) == c.tiles
    # units of the last tile: 1 for tile_plus_one and k16_edge, 4 for tile_plus_k1024, a full tile where M is a multiple
    assert (M - 1) % LC.SUB + 1 == {"tile_plus_one": 1, "k16_edge": 1, "tile_plus_k1024": 4, "config5_small": 64}.get(name, 4096)
    bats = LC.case_batches(name)
    assert len(bats) == LC.STEPS
    for s, (pos, negs) in enumerate(bats):
        assert negs.shape == (c.K, c.B, 3)
        tri = LC.step_triples(pos, negs)
        assert tri.shape == (M, 3) and tri.min() >= 0 and tri.max() < N_ROWS       # every triple of a case is valid
        counts = LC.slot_counts(tri, N_ROWS)
        assert counts.sum() == 3 * M
        one, small, mid, big = LC.row_classes(counts)
        assert one > 0 and small > 0 and mid > 0, (s, one, small, mid, big)
        if name == "k16_edge":
            assert (counts == 17).any(), s                       # one full item of 16 slots + an item of one slot
        else:
            assert big > 0, s
        if name == "one_tile_full":
            assert ((counts == 256) | (counts == 257)).any(), s  # 16 full items (+ an item of one slot)
    # the 40-step run of one_tile_full crosses the 32-step prepare chunk and wraps the triple array
    if name == "one_tile_full":
        assert len(LC.case_batches(name, LC.LONG_STEPS)) == LC.LONG_STEPS > 32


@pytest.mark.parametrize("name", NAMES)
def test_a_dropped_slot_is_ten_bounds_away(name):
    """One fp64 step with and without one gradient slot of the row with the most slots -- the slot that moves the row
    most -- differ by more than 10 x the table bound of the case.  Which slot: a slot's share of its row is lr *
    |coef| * |product of the two other rows' elements|, and only the rows the workload lengthens nine times (every
    fifth) are near the unit norm.  A slot whose two other rows are both long (1 in 25) moves its row by 2e-4 to
    1.6e-3; the median slot, between two short rows, by 1.2e-5 to 9e-5 (measured per case, below the 2e-5 floor of
    the bound in four of six cases).  So the bound sees the loss of any of the heavy slots of a hot row, and a kernel that
    drops slots by position (one per item of 16, a whole item) drops heavy ones among them; it does not see the
    loss of a single light slot, and no absolute bound at the fp32 error of the reference could."""
    c = LC.BY_NAME[name]
    _, table = LC.workload(c.B, c.d, c.tri_seed)
    pos, negs = LC.case_batches(name)[0]
    row, n, full, cut, median = LC.drop_one_slot(table.astype(np.float64), pos, negs, float(LC.learning_rate(LC.GS0)), c.l2)
    moved = float(np.abs(full - cut).max())
    print(f"{name}: row {row} with {n} slots: heaviest slot moves it by {moved:.3g}, median slot by {median:.3g}, "
          f"bound {LC.table_tol(c.d32):.3g}")
    assert n > 16 * LC.ITEM_CAP or name == "k16_edge"
    assert moved > 10.0 * LC.table_tol(c.d32)
    assert moved > 10.0 * LC.table_tol(LC.D32_LONG) or name != "one_tile_full"


@pytest.mark.parametrize("name", NAMES)
def test_stored_d32_is_fresh(name):
    c = LC.BY_NAME[name]
    fresh = LC.measure_d32(name)
    assert fresh / 2 <= c.d32 <= fresh * 2, fresh
    _, l64 = LC.case_replay(name)
    _, l32 = LC.case_replay(name, LC.STEPS, True)
    # the oracle's own fp32 losses sit an order inside the loss bound
    assert max(float(np.abs(a - b).max()) / LC.loss_tol(b) for a, b in zip(l32, l64)) < 0.1


def test_stored_d32_of_the_long_and_invalid_runs_is_fresh():
    fresh = LC.measure_d32("one_tile_full", LC.LONG_STEPS)
    assert fresh / 2 <= LC.D32_LONG <= fresh * 2, fresh
    fresh = LC.measure_invalid_d32()
    assert fresh / 2 <= LC.INVALID.d32 <= fresh * 2, fresh


def test_invalid_id_workload():
    iv = LC.INVALID
    id_to_type, tri, table, bats = LC.invalid_workload()
    fb = LC.type_arrays()[0]
    ent = np.arange(fb.relation_count, fb.entity_count)
    assert abs((id_to_type[ent] < 0).mean() - iv.share) < 0.001 and (LC.type_arrays()[1][ent] >= 0).all()
    t64, losses, bad = LC.invalid_replay()
    assert np.isfinite(t64).all()
    M = (1 + iv.K) * iv.B
    for (pos, negs), loss, b in zip(bats, losses, bad):
        t3 = LC.step_triples(pos, negs)
        assert b.sum() >= 20 and b.mean() <= 0.25
        assert np.array_equal(b, (t3 == -1).any(1)) and not b[:iv.B].any() and t3.max() < N_ROWS
        assert np.array_equal(np.isnan(loss), b) and loss.shape == (M,)
    # with nothing invalid the masked step IS the oracle's step
    c = LC.BY_NAME["k16_edge"]
    _, tab = LC.workload(c.B, c.d, c.tri_seed)
    pos, negs = LC.case_batches(c.name)[0]
    a, la = LC.O.logloss_step(tab.astype(np.float64), pos, negs, 0.04, c.l2)
    b_, lb, bad0 = LC.masked_step(tab.astype(np.float64), LC.step_triples(pos, negs), len(pos), 0.04, c.l2)
    assert not bad0.any() and np.array_equal(la, lb) and np.abs(a - b_).max() < 1e-15


def test_scalar_crossings_and_zero_factor():
    assert LC.scalar_crossings(0.1, 0.1, 1024, 27) == [12, 25]
    assert LC.scalar_crossings(0.1, 0.00947265625, 1024, 12) == [7]
    assert LC.scalar_crossings(0.1, 0.1, 1024, 6) == []           # the six steps of the default-l2 test never cross
    assert LC.scalar_crossings(0.125, 2.0 ** -7, 1024, 2) == [0, 1]
