"""Fixtures for the edges of RotatE's hinge path (graphembeddings_amd/csrc/ge_rotate.hip: score, hinge step, AdaGrad
step, the native loops and the rank sweep, with the shared apply stage of ge_transx_apply.h told dr = k < d) and a
restatement of the dispatch that decides which kernel instantiation, which grid-stride trip and which candidate block
a fixture reaches.

tests/test_rotate_edge_cases_host.py proves on the CPU that every fixture is what it claims (exact, covering, past
its threshold, free of pairs near z = 0); tests/test_gpu_rotate_edges.py runs them on the MI355X.  A fixture is built
once per process and must not be modified by its users.

Exact cases stand on rotate_ref.exact_tables_l2 (theta = 0, small integers, the squared norm) with lr a power of two and
an integer margin for which rotate_ref.is_exact_step holds: fp32 must give the fp64 loss and tables bitwise.  The
modulus norm has no exact gradients (u / |u| = 3/5, 4/5): the same layouts run with l1 on collinear_tables by bound.
"""
from __future__ import annotations

import functools
import os
import re

import numpy as np

from tests import rotate_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphembeddings_amd", "csrc")
F32 = np.float32

# ------------------------------------------------------------------------------------ the dispatch, restated
# ge_common.h: kWave, kBlock, kMaxBlocks (grid_for's cap); ge_transx_apply.h: kWin; ge_rotate.hip: kRows, kKnownTile;
# ge_rotate_dev.h: kRotMaxDim.
kWave, kBlock, kMaxBlocks = 64, 256, 2048
kWin, kRows, kKnownTile, kRotMaxDim = 32, 16, 128, 1024
# ge_rotate.hip's lpt_for: nvec <= 8 ? 8 : nvec <= 16 ? 16 : nvec <= 32 ? 32 : 64
LPT_THRESHOLDS = ((8, 8), (16, 16), (32, 32))
LPT_LAST = 64
# run_rank launches rotate_rank_filter_kernel on dim3(1024) x kBlock threads: its loop goes round above this many cells
FILTER_BLOCKS = 1024
filter_wrap_cells = FILTER_BLOCKS * kBlock


def source_constants():
    """{name: value} of the `constexpr int` constants above, read out of the four sources as text."""
    out = {}
    for fn in ("ge_common.h", "ge_rotate.hip", "ge_rotate_dev.h", "ge_transx_apply.h"):
        with open(os.path.join(CSRC, fn)) as f:
            for name, expr in re.findall(r"constexpr\s+int\s+(k\w+)\s*=\s*([0-9][0-9 *]*);", f.read()):
                out[name] = int(np.prod([int(x) for x in expr.split("*")]))
    return out


def source_dispatch():
    """(thresholds, last, filter blocks) of ge_rotate.hip as text: lpt_for's `nvec <= a ? b` chain with its final
    value, and the filter kernel's grid."""
    with open(os.path.join(CSRC, "ge_rotate.hip")) as f:
        src = f.read()
    body = re.search(r"inline int lpt_for\(int nvec\)\s*\{\s*return ([^;]*);", src).group(1)
    pairs = tuple((int(a), int(b)) for a, b in re.findall(r"nvec <= (\d+) \? (\d+)", body))
    last = int(re.search(r":\s*(\d+)\s*$", body).group(1))
    blocks = int(re.search(r"rotate_rank_filter_kernel<L1>\), dim3\((\d+)\)", src).group(1))
    return pairs, last, blocks


def lpt_for(nvec):
    for limit, lanes in LPT_THRESHOLDS:
        if nvec <= limit:
            return lanes
    return LPT_LAST


def nvec(d, aligned=True):
    """Chunks per triple: k / VEC."""
    return (d // 2) // (4 if d % 8 == 0 and aligned else 1)


def variant(d, aligned=True):
    """(VEC, LPT) of rotate_score_kernel / rotate_grad_kernel: float4 iff d % 8 == 0 and every pointer of the call is
    16-byte aligned."""
    return (4 if d % 8 == 0 and aligned else 1), lpt_for(nvec(d, aligned))


ALL_VARIANTS = {(vec, lpt) for vec in (1, 4) for lpt in (8, 16, 32, 64)}


def score_wrap_B(lpt):
    """grid_for caps at kMaxBlocks workgroups of kBlock / kWave waves, a wave holds kWave / lpt triples: the score and
    gradient kernels' loops take a second trip from this B on, and row i + score_wrap_B(lpt) is handled by the lane
    group that handled row i."""
    return kMaxBlocks * (kBlock // kWave) * (kWave // lpt)


def rank_grid_y(B, E):
    """rank_grid's gridDim.y: candidate blocks of kBlock entities are strided by it."""
    n_chunks, n_cb = -(-B // kRows), -(-E // kBlock)
    return max(1, min(-(-2 * kMaxBlocks // n_chunks), n_cb))


def sort_key_bits(n):
    """ge_common.h: the radix sort's key width for keys 0 ... n (n is the sentinel E + R)."""
    b = 1
    while b < 32 and (1 << b) <= n:
        b += 1
    return b


# ------------------------------------------------------------------------------------ helpers
def float_tables(E, R, d, seed, theta=np.pi, scale=0.5):
    """Entities N(0, scale^2), phases uniform in [-theta, theta), rounded to float32 (what the GPU holds), as fp64."""
    rng = np.random.default_rng(seed)
    ent, rel = rng.normal(size=(E, d)) * scale, rng.uniform(-theta, theta, size=(R, d // 2))
    return {"ent": ent.astype(F32).astype(np.float64), "rel": rel.astype(F32).astype(np.float64)}


def pairs(rng, E, R, B):
    """(pos, neg) int32 [B,3]; each negative replaces the head or the tail."""
    pos = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, R, B)], 1).astype(np.int32)
    neg = pos.copy()
    neg[np.arange(B), rng.integers(0, 2, B)] = rng.integers(0, E, B)
    return pos, neg


def float_masks(case, l1):
    """(fp64 active mask, fp32 active mask) of a float case's valid pairs."""
    tabs, pos, neg = case["tabs"], case["pos"], case["neg"]
    ok = RR.valid_mask(pos, neg, len(tabs["ent"]), len(tabs["rel"]))
    return (RR.active_mask(tabs, pos[ok], neg[ok], case["margin"], l1),
            RR.active_mask(tabs, pos[ok], neg[ok], case["margin"], l1, F32))


def loss_sample(case, l1):
    """(e32 of the batch loss, sigma): |fp32 restatement - fp64| of that one number, and the spread the restatement's own
    distance errors give a sum of the active terms D+ - D- when they do not cancel, sqrt(sum_i (e(D+_i)^2 + e(D-_i)^2)),
    e(D) = the fp32 restatement's D minus fp64's."""
    tabs, pos, neg = case["tabs"], case["pos"], case["neg"]
    ok = RR.valid_mask(pos, neg, len(tabs["ent"]), len(tabs["rel"]))
    p, n = pos[ok], neg[ok]
    l64, _, act = RR.hinge_grads(tabs, p, n, case["margin"], l1)
    l32 = RR.hinge_grads(tabs, p, n, case["margin"], l1, F32)[0]
    ep = RR.dist(tabs, p[act], l1, F32).astype(np.float64) - RR.dist(tabs, p[act], l1)
    en = RR.dist(tabs, n[act], l1, F32).astype(np.float64) - RR.dist(tabs, n[act], l1)
    return abs(l32 - l64), float(np.sqrt((ep * ep + en * en).sum()))


def _frozen(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            _frozen(v)
    return case


# ------------------------------------------------------------------------------------ A: variant, B: one_pointer_off
VARIANT_E, VARIANT_R, SCORE_B, STEP_B = 61, 7, 203, 157
DIMS_V4 = (64, 72, 128, 136, 256, 264, 512, 520, 1024)          # nvec 8, 9, 16, 17, 32, 33, 64, 65, 128
DIMS_V1 = (2, 18, 34, 66, 130, 1022)                            # nvec 1, 9, 17, 33, 65, 511
DIMS_SHIFTED = (16, 32, 64, 128)                                # nvec 8, 16, 32, 64 on tables 4 bytes off
SHIFTS_ONE_DIM = (32, (8, 12))                                  # d = 32 also 8 and 12 bytes off
ONE_OFF_D = 72
# (d, shifted): the seed of the case's tables and pairs where the default (d, + 5000 when shifted) fails a host condition
# of test_float_cases_are_fair: a pair within fp32 rounding of z = 0, or a batch loss on which the fp32 restatement's
# errors cancel to less than a quarter of their own spread.  The next seed in steps of 10,000 that meets them for both norms is taken.
VARIANT_SEEDS = {(72, False): 10072, (512, False): 10512, (1024, False): 11024, (66, False): 10066, (1022, False): 11022,
                 (32, True): 15032, (64, True): 15064, (72, True): 15072}


def variant_dims():
    """[(d, shift in bytes)] of family A."""
    return ([(d, 0) for d in DIMS_V4 + DIMS_V1] + [(d, 4) for d in DIMS_SHIFTED]
            + [(SHIFTS_ONE_DIM[0], s) for s in SHIFTS_ONE_DIM[1]])


@functools.lru_cache(maxsize=None)
def variant_case(d, shifted=False):
    """Float tables (phases in [-pi, pi)), SCORE_B triples to score and STEP_B pairs for one step at margin 0."""
    seed = VARIANT_SEEDS.get((d, shifted), d + (5000 if shifted else 0))
    rng = np.random.default_rng(seed)
    pos, neg = pairs(rng, VARIANT_E, VARIANT_R, STEP_B)
    return _frozen(dict(tabs=float_tables(VARIANT_E, VARIANT_R, d, seed), tri=pairs(rng, VARIANT_E, VARIANT_R, SCORE_B)[0],
                        pos=pos, neg=neg, lr=0.01, margin=0.0))


# ------------------------------------------------------------------------------------ C: wrap
# lpt -> (d, aligned): one shape just past each LPT's threshold, both VECs across the four
WRAP = {8: (8, True), 16: (18, False), 32: (136, True), 64: (66, False)}
WRAP_EXTRA = 5                                                  # keeps the last trip ragged
WRAP_E, WRAP_R = 4001, 7
WRAP_LR = 2.0 ** -8
# what the first-trip row in front of each planted second-trip row is
WRAP_PLANTS = ("active", "inactive", "bad_id", "foreign_relation", "active")
# lpt -> seed where 300 + lpt fails the same conditions (steps of 1,000)
WRAP_FLOAT_SEEDS = {32: 1332}


def wrap_B(lpt):
    return score_wrap_B(lpt) + WRAP_EXTRA


@functools.lru_cache(maxsize=None)
def wrap_score_case(lpt):
    d, _ = WRAP[lpt]
    rng = np.random.default_rng(100 + lpt)
    return _frozen(dict(tabs=float_tables(VARIANT_E, VARIANT_R, d, 100 + lpt), tri=pairs(rng, VARIANT_E, VARIANT_R, wrap_B(lpt))[0]))


@functools.lru_cache(maxsize=None)
def wrap_exact_case(lpt):
    """The exact squared-norm fixture at wrap_B(lpt) pairs over WRAP_E entities.  Rows 0 ... 4 of the first trip are what
    WRAP_PLANTS says; rows W ... W + 4 (W = score_wrap_B(lpt)), handled by the same lane groups on their second trip, are
    valid pairs: active, active, active, active, inactive."""
    d, _ = WRAP[lpt]
    W, B = score_wrap_B(lpt), wrap_B(lpt)
    tabs = RR.exact_tables_l2(WRAP_E, WRAP_R, d, seed=lpt, amp=1)
    rng = np.random.default_rng(200 + lpt)
    pos, neg = pairs(rng, WRAP_E, WRAP_R, B)
    margin = 0.0
    act = RR.active_mask(tabs, pos, neg, margin, False)
    ia, ii = np.flatnonzero(act[10:W]) + 10, np.flatnonzero(~act[10:W]) + 10
    src = {"active": ia, "inactive": ii, "bad_id": ia, "foreign_relation": ia}
    for j, kind in enumerate(WRAP_PLANTS):
        pos[j], neg[j] = pos[src[kind][j]], neg[src[kind][j]]
        second = ii[10] if j == len(WRAP_PLANTS) - 1 else ia[20 + j]
        pos[W + j], neg[W + j] = pos[second], neg[second]
    pos[2, 0] = WRAP_E                                          # bad_id
    neg[3, 2] = (pos[3, 2] + 1) % WRAP_R                        # foreign_relation
    return _frozen(dict(tabs=tabs, pos=pos, neg=neg, lr=WRAP_LR, margin=margin,
                        second_trip_rows=np.arange(W, W + len(WRAP_PLANTS))))


@functools.lru_cache(maxsize=None)
def wrap_float_case(lpt):
    d, _ = WRAP[lpt]
    seed = WRAP_FLOAT_SEEDS.get(lpt, 300 + lpt)
    rng = np.random.default_rng(seed)
    pos, neg = pairs(rng, WRAP_E, WRAP_R, wrap_B(lpt))
    return _frozen(dict(tabs=float_tables(WRAP_E, WRAP_R, d, seed), pos=pos, neg=neg, lr=0.01, margin=0.0))


LOOP_LPT, LOOP_STEPS = 64, 3


@functools.lru_cache(maxsize=None)
def wrap_loop_case():
    """The native loop at the LPT 64 wrap shape: a KG of unique triples on 300 entities and 8 relations."""
    d, _ = WRAP[LOOP_LPT]
    rng = np.random.default_rng(7)
    E, R, T = 300, 8, 20000
    tri = np.unique(np.stack([rng.integers(0, E, T), rng.integers(0, E, T), rng.integers(0, R, T)], 1), axis=0)
    return _frozen(dict(tabs=float_tables(E, R, d, 7), triples=tri.astype(np.int64), B=wrap_B(LOOP_LPT)))


# ------------------------------------------------------------------------------------ D: layout
# The sorted slot list of a step: the 4 A entity slots of the A active pairs (keys < E), then their A relation slots
# in relation order (keys E + r), then the 5 (B - A) sentinels.  Relation run r starts at 4 A + (active pairs with a
# relation < r).  counts[r] = active pairs on relation r; `inactive` pairs have neg == pos under margin -1.
LAYOUTS = {
    "run32_on_edge": dict(counts=(4, 32, 3), inactive=2),                 # relation 1 fills window 5, [160, 192), exactly
    "run31": dict(counts=(4, 31, 4), inactive=2),                         # [160, 191)
    "run33": dict(counts=(4, 33, 2), inactive=2),                         # [160, 193)
    "run64_on_edge": dict(counts=(64,), inactive=2),                      # [256, 320): windows 8 and 9, both full
    "run65": dict(counts=(4, 65, 3), inactive=2),                         # [292, 357)
    "three_windows_after_entities": dict(counts=(83,), inactive=2),       # [332, 415): window 10 begins with 12 entity keys
    "entity_run_ends_window": dict(counts=(8,), inactive=3),    # entity keys fill window 0, relation 0 starts window 1
    "boundary_mid_window": dict(counts=(5, 7), inactive=2),               # entity keys end at 48, inside window 1
    "ragged_sentinel_tail": dict(counts=(3, 20), inactive=10),  # n = 165: window 5 is 5 slots, all sentinels
    "one_active": dict(counts=(0, 1), inactive=20),
    "one_relation_300": dict(counts=(0, 300, 0)),
}
LAYOUT_E = 50
LAYOUT_DIMS = ((8, True), (264, True), (6, False), (130, False))   # (d, float4 path)
LAYOUT_LR = 2.0 ** -6


def _ordered(tabs, rng, rel, E, l1):
    """(pos, neg) on the relation column rel with D(pos) - D(neg) >= 1 (the fixtures' distances are integers)."""
    A = len(rel)
    ents = rng.integers(0, E, (A, 4))
    while True:
        pos, neg = np.stack([ents[:, 0], ents[:, 1], rel], 1), np.stack([ents[:, 2], ents[:, 3], rel], 1)
        dp, dn = RR.dist(tabs, pos, l1), RR.dist(tabs, neg, l1)
        tie = np.abs(dp - dn) < 1
        if not tie.any():
            break
        ents[tie] = rng.integers(0, E, (int(tie.sum()), 4))
    swap = dp < dn
    pos[swap], neg[swap] = neg[swap].copy(), pos[swap].copy()
    return pos, neg


@functools.lru_cache(maxsize=None)
def layout_case(name, d, l1=False):
    """One of LAYOUTS at dimension d: exact_tables_l2 (or collinear_tables with l1), margin -1: the counted pairs are
    active (z >= 0), the `inactive` ones have neg == pos (z = -1)."""
    spec = LAYOUTS[name]
    counts, inactive = spec["counts"], spec.get("inactive", 0)
    E, R = LAYOUT_E, len(counts)
    rng = np.random.default_rng(sorted(LAYOUTS).index(name) * 1000 + d)
    tabs = (RR.collinear_tables if l1 else RR.exact_tables_l2)(E, R, d, seed=d + 1, amp=2)
    pos, neg = _ordered(tabs, rng, np.repeat(np.arange(R), counts), E, l1)
    idle = np.stack([rng.integers(0, E, inactive), rng.integers(0, E, inactive), rng.integers(0, R, inactive)], 1)
    pos, neg = np.concatenate([pos, idle]), np.concatenate([neg, idle])
    order = rng.permutation(len(pos))                           # interleave relations and inactive pairs in slot order
    return _frozen(dict(tabs=tabs, pos=pos[order].astype(np.int32), neg=neg[order].astype(np.int32), lr=LAYOUT_LR,
                        margin=-1.0, counts=counts, inactive=inactive))


def sorted_keys(case, l1=False):
    """The key column of the step's sorted (key, slot) list, rebuilt on the host: slots 4i ... 4i+3 = pos h, pos t,
    neg h, neg t, slot 4B + i = E + r, the sentinel E + R for inactive or invalid pairs; stable sort by key."""
    tabs, pos, neg = case["tabs"], np.asarray(case["pos"], dtype=np.int64), np.asarray(case["neg"], dtype=np.int64)
    E, R, B = len(tabs["ent"]), len(tabs["rel"]), len(pos)
    ok = RR.valid_mask(pos, neg, E, R)
    act = np.zeros(B, dtype=bool)
    act[ok] = RR.active_mask(tabs, pos[ok], neg[ok], case["margin"], l1)
    keys = np.full(5 * B, E + R, dtype=np.int64)
    i = np.flatnonzero(act)
    for s, col in enumerate((pos[:, 0], pos[:, 1], neg[:, 0], neg[:, 1])):
        keys[4 * i + s] = col[i]
    keys[4 * B + i] = E + pos[i, 2]
    return np.sort(keys, kind="stable")


def runs(keys):
    """[(key, start, length)] of the runs of equal keys."""
    cut = np.flatnonzero(np.diff(keys)) + 1
    start = np.concatenate([[0], cut])
    return list(zip(keys[start].tolist(), start.tolist(), np.diff(np.concatenate([start, [len(keys)]])).tolist()))


# ------------------------------------------------------------------------------------ E: key_width
KEY_WIDTH_TOTALS = (255, 256, 257)                              # E + R, the sentinel: 8, 9 and 9 key bits
KEY_WIDTH_R, KEY_WIDTH_D, KEY_WIDTH_B = 5, 8, 200


@functools.lru_cache(maxsize=None)
def key_width_case(total):
    """The exact fixture with E + R = total; 15 % of the pairs invalid; entity E - 1 and relation R - 1 named by active
    pairs."""
    R, d, B = KEY_WIDTH_R, KEY_WIDTH_D, KEY_WIDTH_B
    E = total - R
    tabs = RR.exact_tables_l2(E, R, d, seed=total, amp=2)
    rng = np.random.default_rng(total)
    pos, neg = pairs(rng, E, R, B)
    margin = 0.0
    act = np.flatnonzero(RR.active_mask(tabs, pos, neg, margin, False))
    a, b = act[0], act[1]                                       # copies of two active pairs, renamed to the last rows
    pos[a, 2] = neg[a, 2] = R - 1                               # theta = 0 everywhere: the distances do not change
    hot = tabs["ent"][pos[b, 0]]
    tabs["ent"][E - 1] = hot                                    # entity E - 1 a twin of pair b's head, then its head
    same = neg[b, 0] == pos[b, 0]
    pos[b, 0] = E - 1
    if same:
        neg[b, 0] = E - 1
    bad = rng.choice(np.setdiff1d(np.arange(B), [a, b]), int(0.15 * B), replace=False)
    kinds = rng.integers(0, 4, len(bad))
    pos[bad[kinds == 0], 0] = E                                 # the first id past the table: E (a relation key, were it sorted)
    pos[bad[kinds == 1], 1] = -1
    for i in bad[kinds == 2]:
        pos[i, 2] = neg[i, 2] = R
    neg[bad[kinds == 3], 2] = (pos[bad[kinds == 3], 2] + 1) % R
    return _frozen(dict(tabs=tabs, pos=pos, neg=neg, lr=LAYOUT_LR, margin=margin, named=(int(a), int(b)), invalid=np.sort(bad)))


# ------------------------------------------------------------------------------------ F: rank_trip
# The smallest B x E with gridDim.y below the number of candidate blocks, an uneven share and a ragged last block:
# 2,048 chunks of 16 rows (one row in the last) give gridDim.y = ceil(4096 / 2048) = 2, 513 entities give 3 blocks, the
# last of one candidate.  blockIdx.y = 0 walks blocks 0 and 2, blockIdx.y = 1 block 1.
TRIP_B, TRIP_E, TRIP_R, TRIP_D = 32753, 513, 5, 6
TRIP_KNOWN = 30000                                              # about 10 known tails (heads) per (entity, relation)


@functools.lru_cache(maxsize=None)
def rank_trip_rows():
    """(test [B,3], known [T,3]): random rows; the known triples are random too, so every row meets about ten of them,
    plus the first half of the test rows themselves."""
    rng = np.random.default_rng(17)
    rnd = lambda n: np.stack([rng.integers(0, TRIP_E, n), rng.integers(0, TRIP_E, n), rng.integers(0, TRIP_R, n)], 1)
    test = rnd(TRIP_B)
    known = np.concatenate([rnd(TRIP_KNOWN), test[:TRIP_B // 2]], 0)
    test.setflags(write=False)
    known.setflags(write=False)
    return test, known


@functools.lru_cache(maxsize=None)
def rank_trip_mask(side):
    km = RR.known_mask(*rank_trip_rows(), TRIP_E, side)
    km.setflags(write=False)
    return km


@functools.lru_cache(maxsize=None)
def rank_trip_tables(l1, exact=True):
    if not exact:
        return _frozen(float_tables(TRIP_E, TRIP_R, TRIP_D, 23))
    tabs = (RR.collinear_tables if l1 else RR.exact_tables_l2)(TRIP_E, TRIP_R, TRIP_D, seed=19, amp=1)
    # every entity gets a twin in another candidate block, so every row's target ties with at least its twin: entity
    # 257 + i is entity i (the one entity of the last block, 512, is entity 255 of the first), and 256 is entity 0
    tabs["ent"][TRIP_E - kBlock:] = tabs["ent"][:kBlock]
    tabs["ent"][kBlock] = tabs["ent"][0]
    return _frozen(tabs)


def rank_reference(tabs, test, side, l1, km, dtype=np.float64):
    """(n_before, n_known_before, true_dist, scores [B,E]) like rotate_ref.ranks, the distance matrix built in row
    blocks."""
    test = np.asarray(test, dtype=np.int64)
    sc = RR.all_dists_blocked(tabs, test, side, l1, dtype)
    target = test[:, 0] if side == "head" else test[:, 1]
    td = sc[np.arange(len(test)), target]
    nb, nk = RR.counts_from(sc, td, target, km)
    return nb, nk, td, sc


def same_y_first_block(E, gy):
    """(first, last): the candidate-id ranges of the first and the last block walked by the blockIdx.y that walks the last
    block."""
    n_cb = -(-E // kBlock)
    y = (n_cb - 1) % gy
    return (y * kBlock, (y + 1) * kBlock), ((n_cb - 1) * kBlock, E)


# ------------------------------------------------------------------------------------ G: rank_sparse
SPARSE_B, SPARSE_E, SPARSE_R, SPARSE_D = 300, 1000, 4, 6
SPARSE_TILES = ((0, 0), (0, 7), (2, 3))                         # (row tile, column tile) of 128 x 128 cells, ~200 cells each
SPARSE_LAST = (2, 7)                                            # one cell: the last row, the last entity


@functools.lru_cache(maxsize=None)
def rank_sparse_case(side):
    """Row i has fixed entity i (so a known triple lands in one row only); known cells lie in SPARSE_TILES and in one
    cell of the very last tile."""
    rng = np.random.default_rng(29)
    B, E = SPARSE_B, SPARSE_E
    test = np.stack([np.arange(B), rng.integers(0, E, B), rng.integers(0, SPARSE_R, B)], 1)
    cells = []
    for rt, ct in SPARSE_TILES:
        r0, c0 = rt * kKnownTile, ct * kKnownTile
        rows = rng.integers(r0, min(r0 + kKnownTile, B), 200)
        cells.append(np.stack([rows, rng.integers(c0, min(c0 + kKnownTile, E), 200)], 1))
    cells.append(np.array([[B - 1, E - 1]]))
    cells = np.concatenate(cells, 0)
    known = np.stack([cells[:, 0], cells[:, 1], test[cells[:, 0], 2]], 1)
    if side == "head":
        test, known = test[:, [1, 0, 2]], known[:, [1, 0, 2]]
    return _frozen(dict(tabs=float_tables(E, SPARSE_R, SPARSE_D, 31), test=np.ascontiguousarray(test),
                        known=np.ascontiguousarray(known)))


def populated_tiles(km):
    """{(row tile, column tile): cells} of a known mask."""
    out = {}
    for i, c in zip(*np.nonzero(km)):
        key = (int(i) // kKnownTile, int(c) // kKnownTile)
        out[key] = out.get(key, 0) + 1
    return out


# ------------------------------------------------------------------------------------ H: rank_edge
# name -> E, R, d, B, theta (phases uniform in [-theta, theta)), shift of ent in bytes
RANK_EDGES = {
    "d8_ent_4_bytes_off": dict(E=300, R=4, d=8, B=40, theta=np.pi, shift=4),      # the scalar sweep at d % 8 == 0
    "d2": dict(E=300, R=4, d=2, B=40, theta=np.pi, shift=0),                      # k = 1
    "d1024": dict(E=300, R=4, d=kRotMaxDim, B=17, theta=np.pi, shift=0),
    "drifted_phases": dict(E=300, R=4, d=64, B=40, theta=1e3, shift=0),           # the row kernel's s = -s on the head side
    "one_row_in_last_chunk": dict(E=300, R=4, d=16, B=2 * kRows + 1, theta=np.pi, shift=0),
}


@functools.lru_cache(maxsize=None)
def rank_edge_case(name):
    s = RANK_EDGES[name]
    E, R, B = s["E"], s["R"], s["B"]
    seed = 41 + sorted(RANK_EDGES).index(name)
    rng = np.random.default_rng(seed)
    test = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, R, B)], 1)
    known = {}
    for side in ("tail", "head"):
        kn = test[rng.integers(0, B, 40 * B)]
        kn[:, 1 if side == "tail" else 0] = rng.integers(0, E, 40 * B)
        known[side] = np.concatenate([kn, test[:(B + 1) // 2]], 0)
    return _frozen(dict(tabs=float_tables(E, R, s["d"], seed, theta=s["theta"]), test=test, known=known, shift=s["shift"]))


# ------------------------------------------------------------------------------------ the families
def names(family):
    """The parameters of one family's cases."""
    return {
        "variant": variant_dims(),
        "one_pointer_off": ["rel", "ent", "acc_ent", "acc_rel"],
        "wrap": sorted(WRAP),
        "layout": [(n, d) for d, _ in LAYOUT_DIMS for n in LAYOUTS],
        "key_width": list(KEY_WIDTH_TOTALS),
        "rank_trip": [(side, l1) for side in ("tail", "head") for l1 in (True, False)],
        "rank_sparse": ["tail", "head"],
        "rank_edge": sorted(RANK_EDGES),
    }[family]


def exact_cases():
    """[(id, case)] of every exact (squared-norm, bitwise) step case."""
    out = [("wrap-%d" % lpt, wrap_exact_case(lpt)) for lpt in names("wrap")]
    out += [("layout-%s-%d" % nd, layout_case(*nd)) for nd in names("layout")]
    out += [("key_width-%d" % t, key_width_case(t)) for t in names("key_width")]
    return out
