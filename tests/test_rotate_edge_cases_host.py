"""Host-side checks of the fixtures in tests/rotate_edge_cases.py, so that tests/test_gpu_rotate_edges.py tests what it
says: the mirrored constants and thresholds are the sources', the variant dims reach all eight (VEC, LPT) pairs and both
sides of every boundary, each wrap case lies past the threshold it is named for with a ragged last trip, each rank_trip
case makes the sweep's candidate loop go round unevenly and the filter wrap, the sparse tiles are sparse, every exact
case is exact, every layout condition occurs in the sorted list, no float case has a pair near z = 0, and no float case's loss is
one on which the fp32 restatement's errors cancel by chance.  These are
conditions on the inputs, not measurements."""
import numpy as np
import pytest

from tests import rotate_edge_cases as EC
from tests import rotate_ref as RR


def test_mirrored_constants_are_the_sources():
    c = EC.source_constants()
    assert (c["kWave"], c["kBlock"], c["kMaxBlocks"], c["kWin"], c["kRows"], c["kKnownTile"], c["kRotMaxDim"]) \
        == (EC.kWave, EC.kBlock, EC.kMaxBlocks, EC.kWin, EC.kRows, EC.kKnownTile, EC.kRotMaxDim) \
        == (64, 256, 2048, 32, 16, 128, 1024)
    assert EC.source_dispatch() == (EC.LPT_THRESHOLDS, EC.LPT_LAST, EC.FILTER_BLOCKS)
    assert EC.filter_wrap_cells == 262144
    assert [EC.score_wrap_B(lpt) for lpt in (8, 16, 32, 64)] == [65536, 32768, 16384, 8192]
    assert [EC.sort_key_bits(n) for n in EC.KEY_WIDTH_TOTALS] == [8, 9, 9]


def test_mirrored_dispatch():
    assert [EC.lpt_for(n) for n in (1, 8, 9, 16, 17, 32, 33, 64, 65, 512)] == [8, 8, 16, 16, 32, 32, 64, 64, 64, 64]
    assert EC.variant(200) == (4, 32) and EC.variant(200, aligned=False) == (1, 64) and EC.variant(6) == (1, 8)
    assert EC.rank_grid_y(40, 600) == 3 and EC.rank_grid_y(32753, 513) == 2 and EC.rank_grid_y(32752, 513) == 3 and EC.rank_grid_y(10 ** 6, 600) == 1
    # every shape of tests/test_gpu_rotate.py walks each candidate block from a workgroup of its own
    assert all(EC.rank_grid_y(B, E) == -(-E // 256) for B in (1, 40, 130) for E in (1, 255, 256, 257, 600))


def test_variant_coverage():
    """The variant dims reach all eight (VEC, LPT) pairs, and nvec 8|9, 16|17, 32|33 and 64|65 on each path: a changed
    threshold in lpt_for (mirrored in LPT_THRESHOLDS, compared with the source above) leaves a pair unreached."""
    dims = EC.variant_dims()
    assert {EC.variant(d, shift == 0) for d, shift in dims} == EC.ALL_VARIANTS
    v4 = {EC.nvec(d) for d, shift in dims if shift == 0 and d % 8 == 0}
    v1 = {EC.nvec(d, shift == 0) for d, shift in dims if shift or d % 8}
    edges = {8, 9, 16, 17, 32, 33, 64, 65}
    assert edges <= v4 and edges <= v1
    # the same on lpt_for's chain as ge_rotate.hip states it, so that a threshold changed there fails here too; the two
    # sides of each of its thresholds take different lane counts on each path
    chain, last, _ = EC.source_dispatch()
    src_lpt = lambda n: next((lanes for limit, lanes in chain if n <= limit), last)
    for path in (v4, v1):
        assert {src_lpt(n) for n in path} == {EC.lpt_for(n) for n in path} == {8, 16, 32, 64}
        for lo in (8, 16, 32):
            assert {lo, lo + 1} <= path and src_lpt(lo) == EC.lpt_for(lo) == lo and src_lpt(lo + 1) == EC.lpt_for(lo + 1) == 2 * lo
    assert all(EC.variant(d)[0] == 4 for d in EC.DIMS_V4 + EC.DIMS_SHIFTED) and all(EC.variant(d)[0] == 1 for d in EC.DIMS_V1)
    assert max(d for d, _ in dims) == EC.kRotMaxDim and {s for _, s in dims} == {0, 4, 8, 12}
    assert EC.variant(EC.ONE_OFF_D) == (4, 16) and EC.variant(EC.ONE_OFF_D, aligned=False) == (1, 64)


def test_wrap_cases_lie_past_their_thresholds():
    assert {EC.variant(*EC.WRAP[lpt]) for lpt in EC.WRAP} == {(4, 8), (1, 16), (4, 32), (1, 64)}
    for lpt in EC.names("wrap"):
        d, aligned = EC.WRAP[lpt]
        assert EC.variant(d, aligned)[1] == lpt
        W, per_wave = EC.score_wrap_B(lpt), EC.kWave // lpt
        for case in (EC.wrap_exact_case(lpt), EC.wrap_float_case(lpt)):
            B = len(case["pos"])
            assert W < B < 2 * W                                   # a second trip, and one that does not fill the grid
            # the last wave is ragged; at 64 lanes a wave holds one triple and cannot be, so the last workgroup is
            assert B % per_wave != 0 or lpt == EC.kWave
            assert B % (per_wave * (EC.kBlock // EC.kWave)) != 0
        assert len(EC.wrap_score_case(lpt)["tri"]) == EC.wrap_B(lpt)
        assert 5 * EC.wrap_B(lpt) * d * 4 <= 46e6                  # the gradient ring
    assert EC.wrap_loop_case()["B"] == EC.wrap_B(EC.LOOP_LPT) and len(EC.wrap_loop_case()["triples"]) > 10000


@pytest.mark.parametrize("lpt", EC.names("wrap"))
def test_wrap_second_trip_rows(lpt):
    """Rows W ... W + 4 fall in the second trip of the lane groups that handled rows 0 ... 4, which are a valid active
    pair, an inactive one, a pair with a bad id, one with a foreign relation in the negative, and an active one."""
    case = EC.wrap_exact_case(lpt)
    tabs, pos, neg = case["tabs"], case["pos"], case["neg"]
    W, rows = EC.score_wrap_B(lpt), case["second_trip_rows"]
    assert np.array_equal(rows, W + np.arange(len(EC.WRAP_PLANTS))) and rows.max() < len(pos)
    ok = RR.valid_mask(pos, neg, EC.WRAP_E, EC.WRAP_R)
    act = np.zeros(len(pos), dtype=bool)
    act[ok] = RR.active_mask(tabs, pos[ok], neg[ok], case["margin"], False)
    first = {"active": (True, True), "inactive": (True, False), "bad_id": (False, False), "foreign_relation": (False, False)}
    for j, kind in enumerate(EC.WRAP_PLANTS):
        assert (bool(ok[j]), bool(act[j])) == first[kind], (j, kind)
    assert pos[2, 0] == EC.WRAP_E and neg[3, 2] != pos[3, 2] and 0 <= neg[3, 2] < EC.WRAP_R
    assert ok[rows].all() and act[rows].tolist() == [True, True, True, True, False]
    assert (~ok).sum() == 2                                        # nothing else was dropped


@pytest.mark.parametrize("side,l1", EC.names("rank_trip"))
def test_rank_trip_cases(side, l1):
    B, E = EC.TRIP_B, EC.TRIP_E
    gy, n_cb = EC.rank_grid_y(B, E), -(-E // EC.kBlock)
    assert gy < n_cb and n_cb % gy != 0 and E % EC.kBlock != 0
    km = EC.rank_trip_mask(side)
    assert km.sum() > EC.filter_wrap_cells
    assert B * E * 4 < 80e6 and B % EC.kRows == 1                  # scores_out; one row in the last chunk
    test, _ = EC.rank_trip_rows()
    enb, enk, etd, esc = EC.rank_reference(EC.rank_trip_tables(l1), test, side, l1, km)
    assert np.array_equal(esc, np.round(esc)) and esc.max() < 2 ** 24            # fp32 holds every distance
    target = test[:, 0] if side == "head" else test[:, 1]
    ties = esc == etd[:, None]
    assert (ties.sum(1) > 1).all()                                 # every row: a candidate other than the target ties
    (f0, f1), (l0, l1_) = EC.same_y_first_block(E, gy)
    assert f1 <= l0                                                # two different blocks of one blockIdx.y
    planted = (target >= l0) & ties[:, f0:f1].any(1)
    assert planted.sum() >= 1
    assert (enk > 0).mean() > 0.5 and (enb > enk).any()


def test_rank_trip_is_the_smallest_shape():
    """One row fewer and gridDim.y is the number of candidate blocks again; one entity fewer and the share is even."""
    assert EC.rank_grid_y(EC.TRIP_B - 1, EC.TRIP_E) == -(-EC.TRIP_E // EC.kBlock) == 3
    assert -(-(EC.TRIP_E - 1) // EC.kBlock) == 2 == EC.rank_grid_y(EC.TRIP_B, EC.TRIP_E)


def test_known_mask_equals_the_double_loop():
    rng = np.random.default_rng(0)
    E, R, B = 37, 3, 50
    rnd = lambda n: np.stack([rng.integers(0, E, n), rng.integers(0, E, n), rng.integers(0, R, n)], 1)
    test, known = rnd(B), np.concatenate([rnd(600), [[E, 2, 1], [3, -1, 0]]], 0)
    have = {tuple(x) for x in known.tolist()}
    for side in ("tail", "head"):
        slow = np.array([[((h, c, r) if side == "tail" else (c, t, r)) in have for c in range(E)] for h, t, r in test.tolist()])
        assert np.array_equal(RR.known_mask(test, known, E, side), slow) and slow.any()


@pytest.mark.parametrize("side", EC.names("rank_sparse"))
def test_rank_sparse_tiles(side):
    case = EC.rank_sparse_case(side)
    km = RR.known_mask(case["test"], case["known"], EC.SPARSE_E, side)
    tiles = EC.populated_tiles(km)
    assert set(tiles) == set(EC.SPARSE_TILES) | {EC.SPARSE_LAST} and tiles[EC.SPARSE_LAST] == 1
    assert km[EC.SPARSE_B - 1, EC.SPARSE_E - 1]
    n_ct = -(-EC.SPARSE_E // EC.kKnownTile)
    assert EC.SPARSE_LAST == ((EC.SPARSE_B - 1) // EC.kKnownTile, n_ct - 1)
    order = sorted(rt * n_ct + ct for rt, ct in tiles)
    assert all(b - a - 1 >= 3 for a, b in zip(order, order[1:]))  # at least three empty tiles between populated ones


@pytest.mark.parametrize("name,case", EC.exact_cases(), ids=[n for n, _ in EC.exact_cases()])
def test_exact_cases_are_exact(name, case):
    assert RR.is_exact_step(case["tabs"], case["pos"], case["neg"], case["lr"], case["margin"])
    tabs, pos, neg = case["tabs"], case["pos"], case["neg"]
    ok = RR.valid_mask(pos, neg, len(tabs["ent"]), len(tabs["rel"]))
    act = RR.active_mask(tabs, pos[ok], neg[ok], case["margin"], False)
    assert act.any()
    if "one_relation_300" not in name:                             # the batch that is one relation run and nothing else
        assert (~act).any()
    new, loss = RR.sgd_step(tabs, pos[ok], neg[ok], case["lr"], case["margin"], False)
    for k in tabs:
        assert np.array_equal(new[k], new[k].astype(np.float32).astype(np.float64)), k     # fp32 holds the expectation
    assert loss == np.round(loss)


def test_is_exact_step_refuses_what_is_not_exact():
    case = EC.layout_case("run33", 8)
    args = (case["pos"], case["neg"])
    assert RR.is_exact_step(case["tabs"], *args, 2.0 ** -6, -1.0)
    assert not RR.is_exact_step(case["tabs"], *args, 0.01, -1.0)                  # lr not a power of two
    assert not RR.is_exact_step(case["tabs"], *args, 2.0 ** -6, 0.5)              # margin not an integer
    assert not RR.is_exact_step(case["tabs"], *args, 2.0 ** -23, -1.0)            # row / lr leaves the exact range
    assert not RR.is_exact_step({"ent": case["tabs"]["ent"] * 2.0 ** 11, "rel": case["tabs"]["rel"]}, *args, 2.0 ** -6, -1.0)
    assert not RR.is_exact_step({"ent": case["tabs"]["ent"], "rel": case["tabs"]["rel"] + 0.5}, *args, 2.0 ** -6, -1.0)


def _rel_runs(case, l1=False):
    keys = EC.sorted_keys(case, l1)
    E = len(case["tabs"]["ent"])
    R = len(case["tabs"]["rel"])
    rr = EC.runs(keys)
    return keys, [(k, s, n) for k, s, n in rr if E <= k < E + R], E, R


LAYOUT_CONDITIONS = {
    "run32_on_edge": lambda keys, rel, E, R: any(n == 32 and s % 32 == 0 for _, s, n in rel),
    "run31": lambda keys, rel, E, R: any(n == 31 for _, s, n in rel),
    "run33": lambda keys, rel, E, R: any(n == 33 for _, s, n in rel),
    "run64_on_edge": lambda keys, rel, E, R: any(n == 64 and s % 32 == 0 for _, s, n in rel),
    "run65": lambda keys, rel, E, R: any(n == 65 for _, s, n in rel),
    "three_windows_after_entities": lambda keys, rel, E, R: any(
        s % 32 != 0 and (s + n - 1) // 32 - s // 32 >= 2 and keys[s - s % 32] < E for _, s, n in rel),
    "entity_run_ends_window": lambda keys, rel, E, R: any(s % 32 == 0 and s > 0 and keys[s - 1] < E for _, s, n in rel),
    "boundary_mid_window": lambda keys, rel, E, R: 0 < rel[0][1] % 32 and keys[rel[0][1] - 1] < E,
    "ragged_sentinel_tail": lambda keys, rel, E, R: len(keys) % 32 != 0 and keys[-1] == E + R,
    "one_active": lambda keys, rel, E, R: (keys < E + R).sum() == 5,
    "one_relation_300": lambda keys, rel, E, R: len(keys) == 1500 and [n for _, _, n in rel] == [300],
}


@pytest.mark.parametrize("l1", [False, True])
@pytest.mark.parametrize("name,d", EC.names("layout"))
def test_layout_conditions_occur(name, d, l1):
    assert set(LAYOUT_CONDITIONS) == set(EC.LAYOUTS)
    case = EC.layout_case(name, d, l1)
    keys, rel, E, R = _rel_runs(case, l1)
    assert LAYOUT_CONDITIONS[name](keys, rel, E, R), (name, rel)
    counts = case["counts"]
    assert [n for _, _, n in rel] == [c for c in counts if c]
    assert (keys == E + R).sum() == 5 * case["inactive"]
    z = RR.dist(case["tabs"], case["pos"], l1) - RR.dist(case["tabs"], case["neg"], l1) + case["margin"]
    assert np.array_equal(z, np.round(z))                          # integer distances: fp32 decides the activity alike
    assert {EC.variant(d, v4) for d, v4 in EC.LAYOUT_DIMS} == {(4, 8), (4, 64), (1, 8), (1, 64)}
    # the apply walks d / VEC chunks with 64 lanes: at d = 264 (66 float4 chunks) and d = 130 they take a second trip, and
    # a relation key's row ends inside the first (chunk 33) or the second (column 65)
    assert 264 // 4 > EC.kWave > 264 // 8 and 130 > 130 // 2 > EC.kWave


@pytest.mark.parametrize("total", EC.names("key_width"))
def test_key_width_cases(total):
    case = EC.key_width_case(total)
    tabs, pos, neg = case["tabs"], case["pos"], case["neg"]
    E, R = len(tabs["ent"]), len(tabs["rel"])
    assert E + R == total
    ok = RR.valid_mask(pos, neg, E, R)
    assert np.array_equal(np.flatnonzero(~ok), case["invalid"]) and (~ok).sum() == int(0.15 * len(pos))
    act = np.zeros(len(pos), dtype=bool)
    act[ok] = RR.active_mask(tabs, pos[ok], neg[ok], case["margin"], False)
    a, b = case["named"]
    assert act[a] and act[b] and pos[a, 2] == R - 1 and pos[b, 0] == E - 1
    named = RR.named_rows(tabs, pos[ok], neg[ok], act[ok])
    assert named["ent"][E - 1] and named["rel"][R - 1] and not named["ent"].all()
    assert (~act[ok]).any()
    assert (pos[~ok] == E).any() and (pos[~ok] == -1).any() and (pos[~ok, 2] == R).any()


def _float_step_cases():
    out = [("variant-%d-%s" % (d, bool(s)), EC.variant_case(d, bool(s))) for d, s in EC.names("variant") if s in (0, 4)]
    out += [("one_pointer_off", EC.variant_case(EC.ONE_OFF_D, True))]
    out += [("wrap-%d" % lpt, EC.wrap_float_case(lpt)) for lpt in EC.names("wrap")]
    return out


@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("name,case", _float_step_cases(), ids=[n for n, _ in _float_step_cases()])
def test_float_cases_are_fair(name, case, l1):
    """The fp32 restatement decides every pair's activity as fp64 does, and between 10 % and 90 % of the pairs are
    active.  The batch loss is one number, so its e32 is a single sample of the restatement's error, and 8 e32 + 1e-7
    bounds an fp32 kernel only if that sample is a typical one.  The restatement's own distance errors e(D) say what
    is typical: summed over the active terms without cancelling they spread by sigma = sqrt(sum e(D)^2), and any fp32
    evaluation of the same distances spreads alike.  A seed whose loss sample is below sigma / 4 (a normal sample is,
    one time in five) has the errors cancel by chance ("Which cases need the ulp term") and is not used.  The
    condition is on the restatement alone."""
    a64, a32 = EC.float_masks(case, l1)
    assert np.array_equal(a64, a32), np.flatnonzero(a64 != a32)
    assert 0.1 <= a64.mean() <= 0.9
    e32, sigma = EC.loss_sample(case, l1)
    assert e32 >= sigma / 4, (e32, sigma)


def test_rank_edge_cases():
    for name in EC.names("rank_edge"):
        case, spec = EC.rank_edge_case(name), EC.RANK_EDGES[name]
        assert case["tabs"]["ent"].shape == (spec["E"], spec["d"]) and len(case["test"]) == spec["B"]
    assert np.abs(EC.rank_edge_case("drifted_phases")["tabs"]["rel"]).max() > 900
    assert EC.RANK_EDGES["one_row_in_last_chunk"]["B"] % EC.kRows == 1
    assert EC.RANK_EDGES["d8_ent_4_bytes_off"]["d"] % 8 == 0 and EC.RANK_EDGES["d8_ent_4_bytes_off"]["shift"] == 4
