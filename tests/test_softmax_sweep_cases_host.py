"""CPU: the launch arithmetic of the softmax sweeps and the cases tests/test_gpu_softmax_sweep_edges.py runs because of it.

1. tests/softmax_sweep_cases.py's restatement equals csrc/ge_softmax_route.h, compiled as plain host C++ under the address
   and undefined-behaviour sanitizers (tests/softmax_route_dump.cpp), on every width and a (B, K) grid across every
   threshold the arithmetic has; and the sampled objective's candidate-side partials fit their rows on all of it.
2. The case lists reach what they claim: every gradient instantiation at an odd and an even block count, the X-resident
   edge, every ragged chunk, the query-side ranges, every word and block of the live bitmap.
3. Each plausible wrong indexing of the live bitmap marks dead the only live candidate tile of some query tile of case E.
   Those rows' true candidate is then never found and their loss is NaN, which the GPU test refuses.  Only this direction
   shows in outputs: a tile wrongly taken for live contributes -inf logits and +0 products, and changes no output bit by
   design, so no test of outputs can see it."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import softmax_sweep_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "graphembeddings_amd", "csrc")
DIMS = list(range(8, C.MAX_DIM + 1, 8))
SIZES = [1, 63, 64, 65, 130, 512, 513, 577, 2048, 2049, 4096, 4097, 4161]
GRID = [(B, K) for B in SIZES for K in SIZES]           # every pair in both argument orders


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("softmax_route") / "softmax_route_dump")
    tried = []
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if not cxx or not shutil.which(cxx):
            continue
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "softmax_route_dump.cpp"), "-o", exe]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode == 0:
            return exe
        tried.append("%s: %s" % (cxx, p.stderr[-500:]))
    pytest.fail("no host C++ compiler built softmax_route_dump.cpp with the sanitizers:\n" + "\n".join(tried))


# ------------------------------------------------------------------------------------------------ 1. the restatement
def test_restatement_equals_the_header_on_the_whole_grid(dump):
    shapes = [(d, B, K) for d in DIMS for B, K in GRID]
    p = subprocess.run([dump], input="".join("%d %d %d\n" % s for s in shapes), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    out = p.stdout.split("\n")[:-1]
    assert len(out) == len(shapes)
    bad = [(s, line, C.dump_line(*s)) for s, line in zip(shapes, out) if [int(x) for x in line.split()] != C.dump_line(*s)]
    assert not bad, "%d of %d shapes differ, first: %r" % (len(bad), len(shapes), bad[:3])
    # the candidate-side partials of the sampled objective, [nq][K][d], fit the rows reserved for them (the header's numbers)
    for (d, B, K), line in zip(shapes, out):
        v = [int(x) for x in line.split()]
        assert v[11] * K <= v[13], (B, K, v[11], v[13])


def test_gc_rows_hold_every_split_and_are_met_exactly():
    for B, K in GRID:
        assert C.split(K, B) * K <= C.gc_rows(B, K), (B, K)
    assert C.split(4096, 513) * 4096 == C.gc_rows(513, 4096) == 32768          # case F, as the guard test calls it
    (B, K, d), _ = C.ABI_EXACT_FIT
    assert (B + 1, K + 1) == (513, 4096) and C.split(K + 1, B + 1) * (K + 1) == C.gc_rows(B + 1, K + 1)
    assert C.split(K + 1, B) * (K + 1) == C.gc_rows(B, K + 1)                  # "B >= 512": 512 rows fill it as well
    for B in (1, 64, 511, 512, 513, 4097):                                     # never shrinks as B or K grow
        for K in (1, 64, 4095, 4096, 4097, 32768, 32769, 40000):
            assert C.gc_rows(B + 1, K) >= C.gc_rows(B, K) and C.gc_rows(B, K + 1) >= C.gc_rows(B, K)


# ------------------------------------------------------------------------------------------------ 2. what the lists reach
def test_widths_reach_every_instantiation_and_path():
    new = [d for d, _ in C.WIDTHS]
    assert new == [72, 128, 136, 192, 256, 264, 272, 280] and all(reason for _, reason in C.WIDTHS)
    assert not set(new) & set(C.TESTED_WIDTHS) and all(d % 8 == 0 and 8 <= d <= C.MAX_DIM for d in new)
    # the table of the widths: (MAXCB, column blocks)
    assert [(C.maxcb(d), C.col_blocks(d)) for d in new] == [(2, 3), (2, 4), (3, 5), (3, 6), (4, 8), (5, 9), (5, 9), (5, 9)]
    # what the four suites ran before: MAXCB 1, 4 and 5 alone, and no even block count above one block
    assert {C.maxcb(d) for d in C.TESTED_WIDTHS} == {1, 4, 5}
    assert not [d for d in C.TESTED_WIDTHS if C.maxcb(d) > 1 and C.col_blocks(d) % 2 == 0]
    both = new + C.TESTED_WIDTHS
    assert {C.maxcb(d) for d in new} == {2, 3, 4, 5} and {C.maxcb(d) for d in both} == {1, 2, 3, 4, 5}
    # an odd and an even block count per MAXCB where the width range has one
    for m in (1, 2, 3, 4, 5):
        exist = {C.col_blocks(d) % 2 for d in range(8, C.MAX_DIM + 1, 8) if C.maxcb(d) == m}
        got = {C.col_blocks(d) % 2 for d in both if C.maxcb(d) == m}
        assert got == exist, (m, got, exist)
        # MAXCB 5 is 9 blocks alone (10 blocks would be d > 288): no even count exists
        assert exist == ({1} if m == 5 else {0, 1})
    # an even count: both wave pairs own a last live block (n = MAXCB - 1 is live for w >> 1 = 0 and 1); an odd one: pair 1
    # has a dead slot in its last round
    for d in new:
        a, b = C.blocks_of_wave_pair(d, 0), C.blocks_of_wave_pair(d, 1)
        assert sorted(a + b) == list(range(C.col_blocks(d))) and len(a) == C.maxcb(d)
        assert len(b) == C.maxcb(d) - C.col_blocks(d) % 2
    # a last column block narrower than 32 (the c >= d guard of the gradient's store)
    assert {C.last_block_width(d) for d in new} >= {8, 16, 24, 32} and C.last_block_width(72) == C.last_block_width(136) == 8
    # both sides of the X-resident limit, the limit itself among them
    assert [C.xres(d) for d in new] == [1, 1, 1, 1, 1, 0, 0, 0] and C.XRES_MAX_DIM in new and C.XRES_MAX_DIM + 8 in new
    # the chunked path: every width it serves, so every kn of a last chunk
    chunked = [d for d in range(8, C.MAX_DIM + 1, 8) if not C.xres(d)]
    assert chunked == [264, 272, 280, 288] and set(chunked) <= set(both)
    assert [C.chunk_kn(d)[-1] for d in chunked] == [8, 16, 24, 32] and all(C.chunk_kn(d)[:-1] == [32] * 8 for d in chunked)
    # the LDS request: every width inside a CU's LDS, the largest at d = 256 with the MASKED extras
    req = {(d, m): C.lds_bytes(d, m) for d in range(8, C.MAX_DIM + 1, 8) for m in (False, True)}
    assert all(req[d, m] <= C.LDS_MAX for d in both for m in (False, True))
    assert max(req.values()) == req[256, True] == 150016 and req[256, False] == 149248
    # (the request follows the column blocks, not d: the other widths of eight blocks ask as much, and none is listed)
    assert [k for k in req if req[k] == 150016] == [(d, True) for d in (232, 240, 248, 256)]
    assert max(req[d, True] for d in C.TESTED_WIDTHS) == req[200, True] == 133632      # the largest request run before
    assert [d for d, _ in C.ONE_LABEL_WIDTHS] == [128, 264]


def test_sampled_list_reaches_two_tile_query_ranges_and_empty_ones():
    (B, K, d), _ = C.SAMPLED_RANGES[0]
    assert (B, K, d) == C.SAMPLED_APPENDED == (577, 130, 64) and C.SAMPLED_RANGES[1][0] == (577, 577, 64)
    assert all(ns in [(1.0, 20.0), (4.0, 200.0)] for ns in C.SAMPLED_NORMS_SCALES) and len(C.SAMPLED_NORMS_SCALES) == 2
    for (B, K, d), reason in C.SAMPLED_RANGES:
        nq = C.split(K, B)                              # sm_sweep<1, false, true>: X = candidates, Y = queries
        assert reason and nq == 8 and C.tiles(B) == 10 and C.tiles_per_range(B, nq) == 2
        assert C.ranges_used(B, nq) == (5, 3, 2) and B % C.TILE == 1        # five used, three empty, the fifth ends inside a tile
        assert nq * K <= C.gc_rows(B, K)
    assert C.ranges_used(577, C.split(577, 577)) == (5, 3, 2)               # the candidates' own ranges at K = 577
    assert C.split(577, 130) == 3 and C.tiles_per_range(130, 3) == 1        # the candidates at K = 130: one tile a range
    # what the suites ran before: one query tile a range
    for B in (1, 63, 64, 65, 130):
        for K in (1, 2, 63, 64, 65, 129, 300, 577):
            assert C.tiles_per_range(B, C.split(K, B)) == 1 and C.ranges_used(B, C.split(K, B))[1] == 0


def test_bitmap_case_reaches_every_word_and_block():
    B, K, d = C.BITMAP_B, C.BITMAP_K, C.BITMAP_D
    assert (B, K, d) == (448, 4161, 8) and C.tiles(B) == 7 and C.tiles(K) == 66 and C.live_words(K) == 4 and K % C.TILE == 1
    cts = [ct for ct, _, _ in C.BITMAP_TILES]
    assert cts == [0, 31, 32, 33, 63, 64, 65] and all(r for _, _, r in C.BITMAP_TILES)
    assert [(ct >> 5, ct & 31) for ct in cts] == [wb for _, wb, _ in C.BITMAP_TILES]
    assert {ct >> 5 for ct in cts} == {0, 1, 2}                              # words 0, 1 and 2
    assert [ct for ct in cts if ct and ct % 32 == 0] == [32, 64]             # multiples of 32
    assert [ct for ct in cts if ct // 64 == 1] == [64, 65] and C.live_words(K) // 2 == 2   # the second block of the live kernel
    # what the suites ran before: one word, one block
    assert C.live_words(577) == 2 and C.tiles(577) - 1 == 9
    assert [o for o, _ in C.BITMAP_ORDERS] == [tuple(range(7)), tuple(range(6, -1, -1))]
    sets = C.bitmap_sets()
    assert sets.sum(1).tolist() == [64] * 6 + [1] and sets[6, 4160] and not sets.any(0)[:K].all()
    assert int((~sets.any(0)).sum()) == K - 385                              # candidates no row admits: exact zero rows
    for order, reason in C.BITMAP_ORDERS:
        rs = C.bitmap_row_sets(order)
        pairs, seen = C.tiles_seen_live(order)
        assert reason and np.array_equal(pairs, seen)                        # the right indexing reads what was voted
        assert pairs.sum(1).tolist() == [1] * 7                              # exactly one live candidate tile a query tile
        assert [int(np.nonzero(pairs[q])[0][0]) for q in range(7)] == [cts[s] for s in order]
        for mn, _ in C.BITMAP_NORMS_SCALES:
            t, hr, true, cand, rs2, sets2 = C.bitmap_case(order, mn)
            assert np.array_equal(rs, rs2) and np.array_equal(sets, sets2) and t.shape == (4 + K + 40, d) and t.dtype == np.float32
            assert len(np.unique(cand)) == K and cand.min() >= 4 and hr.shape == (B, 2) and (hr[:, 1] < 4).all()
            pos = {int(c): j for j, c in enumerate(cand)}
            col = np.array([pos[int(x)] for x in true])
            assert sets[rs, col].all()                                       # every true candidate from its row's set
            for q in range(7):                                               # the first and the last admissible position
                mine = np.nonzero(sets[order[q]])[0]
                assert col[64 * q] == mine[0] and col[64 * q + 63] == mine[-1]
                assert len(mine) == 1 or len(set(col[64 * q:64 * q + 64].tolist())) > 16


# ------------------------------------------------------------------------------------------------ 3. wrong indexings
@pytest.mark.parametrize("name", sorted(C.WRONG_INDEXINGS))
def test_each_wrong_indexing_kills_a_live_tile(name):
    write_kw, read_kw = C.WRONG_INDEXINGS[name]
    for order, _ in C.BITMAP_ORDERS:
        pairs, seen = C.tiles_seen_live(order, write_kw, read_kw)
        killed = [q for q in range(pairs.shape[0]) if (pairs[q] & ~seen[q]).any()]
        # a query tile of case E has ONE live tile, which holds every true candidate of its rows: killed = all 64 rows NaN
        assert killed, (name, order)


def test_the_bitmap_model_is_the_kernels_when_nothing_is_wrong():
    """write_bitmap / read_bitmap on a bitmap with many live tiles a query tile, and with unwritten words poisoned: every
    pair reads what its lane voted."""
    rng = np.random.default_rng(0)
    for K in (577, 4161, 8193):
        pairs = rng.random((5, C.tiles(K))) < 0.4
        words = C.write_bitmap(pairs, K, fill=0xDEADBEEF)
        got = np.array([[bool(C.read_bitmap(words, q, ct, K)) for ct in range(C.tiles(K))] for q in range(5)])
        assert np.array_equal(got, pairs)
    rs = np.array([0] * 64 + [1] * 6, np.int32)
    sets = np.zeros((2, 130), bool)
    sets[0, 63], sets[1, 64:] = True, True
    assert C.live_pairs(rs, sets, 70, 130).tolist() == [[True, False, False], [False, True, True]]
