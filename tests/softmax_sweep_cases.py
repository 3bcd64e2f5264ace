"""The launch arithmetic of the softmax sweeps (csrc/ge_softmax_route.h, and what softmax_sweep_kernel and
softmax_live_kernel derive from it) restated in Python, and the shapes tests/test_gpu_softmax_sweep_edges.py runs because
of it.  NumPy only: tests/test_softmax_sweep_cases_host.py checks the restatement against the header compiled as host C++
and checks that the case lists reach what they claim, without a GPU.

Every case list is a named constant with one reason per entry."""
import numpy as np

I32, F32 = np.int32, np.float32

# ------------------------------------------------------------------------------------------------ csrc/ge_softmax_route.h
TILE, CHUNK, LDX, LDW, MAX_SPLIT, XRES_MAX_DIM, MAX_COL_BLOCKS = 64, 32, 33, 65, 8, 256, 5
LDS_MAX = 160 * 1024                                    # the LDS of a CU: what lds_opt_in can grant
MAX_DIM = 288                                           # kRankMaxDim: the widest table the softmax launchers take


def col_blocks(d):
    return (d + 31) // 32


def ldy(d):
    return 32 * col_blocks(d) + 1


def tiles(n):
    return (n + TILE - 1) // TILE


def split(NX, NY):
    return int(min(max(512 // tiles(NX), 1), MAX_SPLIT, tiles(NY)))


def live_words(K):
    return 2 * ((tiles(K) + 63) // 64)


def gc_rows(B, K):
    return min(min(tiles(B), MAX_SPLIT) * K, TILE * max(tiles(K), 512))


def maxcb(d):
    return min((col_blocks(d) + 1) // 2, MAX_COL_BLOCKS)


def xres(d):
    return int(d <= XRES_MAX_DIM)


def tiles_per_range(NY, n_ranges):
    return (tiles(NY) + n_ranges - 1) // n_ranges


def lds_bytes(d, masked):
    return 4 * (TILE * ldy(d) + TILE * (ldy(d) if xres(d) else LDX) + TILE * LDW + 4 * TILE + (3 * TILE if masked else 0))


def dump_line(d, B, K):
    """What tests/softmax_route_dump.cpp prints for `d B K`."""
    ns, nq = split(B, K), split(K, B)
    return [col_blocks(d), ldy(d), maxcb(d), xres(d), lds_bytes(d, False), lds_bytes(d, True), tiles(B), tiles(K), live_words(K),
            ns, tiles_per_range(K, ns), nq, tiles_per_range(B, nq), gc_rows(B, K)]


# ---- what the kernel derives from d (softmax_sweep_kernel)
def last_block_width(d):
    """Columns of the last 32-column block of G."""
    return d - 32 * (col_blocks(d) - 1)


def chunk_kn(d):
    """The chunked path's `kn` per staged chunk (empty for an X-resident width, which has no chunks)."""
    return [] if xres(d) else [min(CHUNK, d - kc) for kc in range(0, d, CHUNK)]


def blocks_of_wave_pair(d, pair):
    """The live column blocks of G that the waves with w >> 1 == pair own: pair + 2 n, n < MAXCB."""
    return [pair + 2 * n for n in range(maxcb(d)) if pair + 2 * n < col_blocks(d)]


def ranges_used(NY, n_ranges):
    """(ranges that hold a tile, empty trailing ranges, tiles of the last used range)."""
    tpr, ty = tiles_per_range(NY, n_ranges), tiles(NY)
    used = (ty + tpr - 1) // tpr
    return used, n_ranges - used, ty - (used - 1) * tpr


# ------------------------------------------------------------------------------------------------ C: widths
WIDTH_B, WIDTH_K = 130, 300                             # the shape of every file's test_widths
TESTED_WIDTHS = [8, 56, 64, 200, 288]                   # what the four parity suites run (test_shapes: 64; test_widths)
WIDTHS = [
    (72, "MAXCB 2, 3 column blocks (odd), the last block 8 wide"),
    (128, "MAXCB 2, 4 column blocks (even): both wave pairs own a last live block; the most common width"),
    (136, "MAXCB 3, 5 column blocks (odd), the last block 8 wide"),
    (192, "MAXCB 3, 6 column blocks (even)"),
    (256, "MAXCB 4, 8 column blocks (even): the X-resident edge, the largest dynamic-LDS request"),
    (264, "MAXCB 5, 9 column blocks: chunked, the last chunk ragged with kn = 8 (the c < d zero-fill, one MFMA round)"),
    (272, "MAXCB 5, 9 column blocks: chunked, kn = 16"),
    (280, "MAXCB 5, 9 column blocks: chunked, kn = 24"),
]
ONE_LABEL_WIDTHS = [
    (128, "one label against the 1-vs-all call at an even block count, MAXCB 2"),
    (264, "one label against the 1-vs-all call on the chunked path with a ragged last chunk"),
]

# ------------------------------------------------------------------------------------------------ D: sampled, query-side ranges
SAMPLED_RANGES = [
    ((577, 130, 64), "the candidate-side sweep over ten query tiles in nq = 8 ranges of two: five used, the fifth ends "
                     "inside a tile, three empty ones that the finish kernel sums from gc"),
    ((577, 577, 64), "the same query ranges with the candidates' own split: ten candidate tiles in eight ranges of two"),
]
SAMPLED_NORMS_SCALES = [(1.0, 20.0), (4.0, 200.0)]
SAMPLED_APPENDED = (577, 130, 64)                       # where the invalid-rows-appended bit equality also runs

# ------------------------------------------------------------------------------------------------ E: the live bitmap
BITMAP_B, BITMAP_K, BITMAP_D = 448, 4161, 8             # seven query tiles; 66 candidate tiles, the last one position
BITMAP_TILES = [
    (0, (0, 0), "the first bit of the first word"),
    (31, (0, 31), "the last bit of word 0"),
    (32, (1, 0), "a multiple of 32: the first bit of a word that is not word 0 (the ballot's upper half)"),
    (33, (1, 1), "inside word 1"),
    (63, (1, 31), "the last tile of softmax_live_kernel's first block"),
    (64, (2, 0), "the first tile of its second block, a multiple of 32: word 2"),
    (65, (2, 1), "the last candidate tile, one position (4160): the loss is 0"),
]
BITMAP_ORDERS = [
    (tuple(range(7)), "query tile q uses set q"),
    (tuple(range(6, -1, -1)), "the sets reversed across the query tiles: row stride and tile index cannot cancel"),
]
BITMAP_NORMS_SCALES = [(1.0, 20.0), (4.0, 200.0)]       # tests/test_gpu_softmax_masked.py's

# ------------------------------------------------------------------------------------------------ F: the workspace's exact fit
ABI_EXACT_FIT = ((512, 4095, 8), "with the guard's appended row and candidate B1 = 513, K1 = 4096: nq * K1 = sm_gc_rows = "
                                 "32,768, the candidate-side partials end on the workspace's last row")


def bitmap_sets():
    """bool [7, K]: set s admits every position below K of candidate tile BITMAP_TILES[s]."""
    s = np.zeros((len(BITMAP_TILES), BITMAP_K), bool)
    for n, (ct, _, _) in enumerate(BITMAP_TILES):
        s[n, TILE * ct:TILE * (ct + 1)] = True
    return s


def bitmap_row_sets(order):
    """int32 [B]: the rows of query tile q use set order[q]."""
    return np.repeat(np.asarray(order, I32), TILE)[:BITMAP_B].copy()


def bitmap_case(order, max_norm, seed=0):
    """(table [N, d] f32, hr [B, 2], true [B], cand [K], row_set [B], sets bool [7, K]) of case E, drawn directly with the
    norm recipe of tests/test_gpu_softmax_masked.py's build (which walks B x K in Python): rows 0..3 are the relations, then
    K + 40 entities of which K (shuffled) are the candidates; row norms are log-normal around max_norm, none within 1 % of
    it.  Each row's true candidate is drawn from its set; the first row of a query tile takes the set's first position, the
    last row its last."""
    B, K, d = BITMAP_B, BITMAP_K, BITMAP_D
    rng = np.random.default_rng(1000 * B + 7 * K + d + seed)
    n_rel, n_ent = 4, K + 40
    N = n_rel + n_ent
    t = rng.standard_normal((N, d))
    norms = max_norm * np.exp(rng.normal(0.0, 0.5, N))
    norms = np.where(np.abs(norms / max_norm - 1) < 0.01, 1.05 * max_norm, norms)
    norms[:n_rel] = max_norm * np.array([0.6, 1.7, 0.8, 2.5])
    t = (t * (norms / np.linalg.norm(t, axis=1))[:, None]).astype(F32)
    cand = (n_rel + rng.permutation(n_ent))[:K].astype(I32)
    hr = np.stack([rng.integers(n_rel, N, B), rng.integers(0, n_rel, B)], 1).astype(I32)
    sets, rs = bitmap_sets(), bitmap_row_sets(order)
    col = np.empty(B, np.int64)
    for q in range(tiles(B)):
        mine = np.nonzero(sets[order[q]])[0]
        rows = np.arange(TILE * q, min(TILE * (q + 1), B))
        col[rows] = rng.choice(mine, len(rows))
        col[rows[0]], col[rows[-1]] = mine[0], mine[-1]
    nrm = np.linalg.norm(t.astype(np.float64), axis=1)
    assert (np.abs(nrm / max_norm - 1) > 0.005).all() and (nrm > 0).all() and sets[rs, col].all()
    return t, hr, cand[col].astype(I32), cand, rs, sets


# ------------------------------------------------------------------------------------------------ the live bitmap's index arithmetic
def live_pairs(row_set, sets, B, K):
    """bool [query tiles, candidate tiles]: some row of the query tile admits some position below K of the candidate tile
    (every row valid, every set id in range: what softmax_live_kernel's lanes vote)."""
    qt, ct = tiles(B), tiles(K)
    adm = np.zeros((B, TILE * ct), bool)
    adm[:, :K] = np.asarray(sets, bool)[np.asarray(row_set)]
    return np.stack([adm[TILE * q:TILE * (q + 1)].reshape(-1, ct, TILE).any((0, 2)) for q in range(qt)])


def write_bitmap(pairs, K, block_word=lambda b: 2 * b, block_order=None, fill=0):
    """softmax_live_kernel's stores as uint32 [query tiles * live_words]: block b of query tile qt votes on candidate tiles
    64 b ... 64 b + 63 and stores the ballot's two words at qt * live_words + block_word(b) (+ 1).  block_order: the order in
    which a query tile's blocks store (it matters only when a wrong block_word makes them overlap); fill: the words no
    block stores."""
    qt_n, ct_n = pairs.shape
    lw = live_words(K)
    out = np.full(qt_n * lw + 2, fill, np.uint64)       # (+ 2: room for a wrong store past the end; never read)
    for qt in range(qt_n):
        for b in (block_order or range(lw // 2)):
            ballot = 0
            for lane in range(64):
                if 64 * b + lane < ct_n and pairs[qt, 64 * b + lane]:
                    ballot |= 1 << lane
            at = qt * lw + block_word(b)
            out[at], out[at + 1] = ballot & 0xFFFFFFFF, ballot >> 32
    return out


def read_bitmap(words, qt, ct, K, word=lambda ct: ct >> 5, bit=lambda ct: ct & 31, stride=None):
    """The MASKED sweep's test of pair (qt, ct): bit `bit(ct)` of the 32-bit word live[qt * stride + word(ct)] (stride:
    live_words).  A bit number of 32 and more is past the word: the arithmetic value of (w >> n) & 1 is 0."""
    w = int(words[qt * (live_words(K) if stride is None else stride) + word(ct)])
    return (w >> bit(ct)) & 1 if bit(ct) < 32 else 0


# The plausible wrong indexings of B.3: name -> (what write_bitmap takes, what read_bitmap takes)
WRONG_INDEXINGS = {
    "the sweep reads word ct >> 6": ({}, dict(word=lambda ct: ct >> 6)),
    "the sweep reads bit ct & 63": ({}, dict(bit=lambda ct: ct & 63)),
    "the sweep strides query tiles by live_words / 2": ({}, dict(stride="half")),
    "a block stores at blockIdx.x, the first block last": (dict(block_word=lambda b: b, block_order=(1, 0)), {}),
    "a block stores at blockIdx.x, the second block last": (dict(block_word=lambda b: b, block_order=(0, 1)), {}),
}


def tiles_seen_live(order, write_kw=None, read_kw=None):
    """bool [7, 66] of case E's arrangement `order`: what the sweep takes for live under the given indexing."""
    B, K = BITMAP_B, BITMAP_K
    pairs = live_pairs(bitmap_row_sets(order), bitmap_sets(), B, K)
    words = write_bitmap(pairs, K, **(write_kw or {}))
    rk = dict(read_kw or {})
    if rk.get("stride") == "half":
        rk["stride"] = live_words(K) // 2
    return pairs, np.array([[bool(read_bitmap(words, qt, ct, K, **rk)) for ct in range(tiles(K))] for qt in range(tiles(B))])
