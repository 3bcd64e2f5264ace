"""Fixtures for the edges of one TransR training step (graphembeddings_amd/csrc/ge_transr.hip) and a restatement of
the dispatch that decides which kernel instantiation and which grid-stride wrap a fixture reaches.

tests/test_transr_edge_cases_host.py proves on the CPU that every fixture is what it claims (exact, covering, past
its threshold); tests/test_gpu_transr_edges.py runs them on the MI355X.  A fixture is built once per process and
must not be modified by its users.

Exact cases are `(tabs, pos, neg, margin, l1)` with small-integer tables and an integer margin for which
`transr_ref.is_exact_step` holds: every partial sum of the step stays below 2^24 in any order, so the fp32 kernels
must give the fp64 loss and gradient bitwise.
"""
from __future__ import annotations

import functools
import os
import re

import numpy as np

from tests import transr_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphembeddings_amd", "csrc")
F32_EPS = 2.0 ** -23

# ------------------------------------------------------------------------------------ the dispatch, restated
# ge_common.h: kWave, kBlock, kMaxBlocks (grid_for's cap); ge_transr.hip: kTrMaxDim, kChunk, kAdamMaxBlocks.
K_WAVE, K_BLOCK, K_MAX_BLOCKS = 64, 256, 2048
K_TR_MAX_DIM, K_CHUNK, K_ADAM_MAX_BLOCKS = 256, 16, 4096
# transr_score_launch: grid_for(B, kBlock / kWave), one wave per triple: the loop goes round above this B
SCORE_WRAP = K_MAX_BLOCKS * (K_BLOCK // K_WAVE)
SCORE_B = 20_000                                  # the score-wrap test's batch
# tr_step_core: transr_prep_kernel on grid_for(max(B, E, R), kBlock), transr_emap_kernel on grid_for(4 B, kBlock)
PREP_WRAP = EMAP_WRAP = K_MAX_BLOCKS * K_BLOCK
# tr_step_core / transr_adam_kernel: at most kAdamMaxBlocks blocks of kBlock units (VEC floats each) per table
ADAM_UNIT_CAP = K_ADAM_MAX_BLOCKS * K_BLOCK
PLAN_BLOCK = 1024                                 # kPlanBlock: pairs per pass of transr_plan_kernel


def source_constants():
    """{name: value} of the `constexpr int` constants above, read out of ge_transr.hip and ge_common.h as text."""
    out = {}
    for fn in ("ge_common.h", "ge_transr.hip"):
        with open(os.path.join(CSRC, fn)) as f:
            for name, expr in re.findall(r"constexpr\s+int\s+(k\w+)\s*=\s*([0-9][0-9 *]*);", f.read()):
                out[name] = int(np.prod([int(x) for x in expr.split("*")]))
    return out


def nc_for(n):
    """transr_chunk_kernel's branch on nc = 2n: the column count chunk_body is instantiated with."""
    nc = 2 * n
    return 2 if nc <= 2 else 4 if nc <= 4 else 8 if nc <= 8 else 16 if nc <= 16 else 2 * K_CHUNK


def vec_for(dim_e, dim_r, aligned=True):
    """tr_step_core's `v4`: float4 loads iff both dims are multiples of 4 and ent, rel, rel_matrix, m, v (and the
    workspace's gent and part) are all 16-byte aligned."""
    return 4 if dim_e % 4 == 0 and dim_r % 4 == 0 and aligned else 1


def chunk_sizes(segment_lengths):
    """transr_plan_kernel: every relation segment cut into full chunks of kChunk pairs plus the tail."""
    out = []
    for n in segment_lengths:
        out += [K_CHUNK] * (n // K_CHUNK) + ([n % K_CHUNK] if n % K_CHUNK else [])
    return out


def valid_mask(pos, neg, E, R):
    """transr_prep_kernel's `ok`."""
    pos, neg = np.asarray(pos, np.int64), np.asarray(neg, np.int64)
    ok = (pos[:, 2] >= 0) & (pos[:, 2] < R) & (neg[:, 2] == pos[:, 2])
    for a in (pos[:, 0], pos[:, 1], neg[:, 0], neg[:, 1]):
        ok &= (a >= 0) & (a < E)
    return ok


def triples_reached(case, aligned=True):
    """The (l1, VEC, NC) instantiations of chunk_body one step on `case` runs."""
    tabs, pos, neg, _, l1 = case
    dim_e, dim_r = RR.dims(tabs)
    ok = valid_mask(pos, neg, len(tabs["ent"]), len(tabs["rel"]))
    seg = np.bincount(np.asarray(pos)[ok, 2])
    return {(bool(l1), vec_for(dim_e, dim_r, aligned), nc_for(n)) for n in chunk_sizes(seg[seg > 0])}


ALL_TRIPLES = {(l1, vec, nc) for l1 in (True, False) for vec in (1, 4) for nc in (2, 4, 8, 16, 32)}


def adam_units(tabs, vec):
    """{table: units of the Adam pass}: elements / VEC."""
    return {k: int(np.size(x)) // vec for k, x in tabs.items()}


def sort_key_bits(n):
    """ge_common.h: the radix sorts' key width for keys 0 ... n (n is the sentinel)."""
    b = 1
    while b < 32 and (1 << b) <= n:
        b += 1
    return b


# ------------------------------------------------------------------------------------ fixtures: helpers
def _pairs(rng, E, r):
    """(pos, neg) int32 [len(r), 3] on the relation column r; each negative replaces the head or the tail."""
    B = len(r)
    pos = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), r], 1).astype(np.int32)
    neg = pos.copy()
    neg[np.arange(B), rng.integers(0, 2, B)] = rng.integers(0, E, B)
    return pos, neg


def score_diff(tabs, pos, neg, l1):
    return RR.score(tabs, pos, l1) - RR.score(tabs, neg, l1)


# ------------------------------------------------------------------------------------ dims
SEGMENTS = (1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32, 33, 48)      # 224 pairs; their chunks take every NC
DIMS = ((100, 100), (256, 256), (7, 256), (256, 7), (64, 64), (128, 128), (200, 200), (1, 1), (4, 4), (3, 5),
        (100, 50))
DIMS_E = 50
DIMS_MARGIN = 2.0
# Entries are integers in [-1, 1], each kept with the given probability.  Dense tables leave the exact range for
# L2 at the three largest products of dims (bound / 2^24 = 1.013 at 256 x 256); the density was halved from 1 until
# is_exact_step held.  Every other (dims, norm) is dense.
DIMS_DENSITY = {((256, 256), False): 0.25, ((7, 256), False): 0.5, ((200, 200), False): 0.5}


def segment_batch(E=DIMS_E, seed=11):
    rng = np.random.default_rng(seed)
    r = rng.permutation(np.repeat(np.arange(len(SEGMENTS)), SEGMENTS))
    return _pairs(rng, E, r)


def _dims_case(dims, l1):
    dim_e, dim_r = dims
    tabs = RR.integer_tables(DIMS_E, len(SEGMENTS), dim_e, dim_r, seed=dim_e * 1000 + dim_r, amp=1,
                             density=DIMS_DENSITY.get((dims, l1)))
    pos, neg = segment_batch()
    return tabs, pos, neg, DIMS_MARGIN, l1


# ------------------------------------------------------------------------------------ tie_and_sign
TIE_DIMS = ((4, 4), (3, 5))
TIE_POS_EQ_NEG, TIE_H_EQ_T = 0, 1                 # the pairs made so by hand


def tie_conditions(case):
    """Counts the tie_and_sign fixtures promise to be >= 1: pairs at z == 0 whose two sides differ in u (a pair
    with pos == neg, or with the same h - t on both sides, ties at margin 0 but its two gradients cancel, so the
    mask's choice would not show), pairs at z == -1, components u == 0 of active pairs, pairs with pos == neg,
    positives with h == t."""
    tabs, pos, neg, margin, l1 = case
    z = score_diff(tabs, pos, neg, l1) + margin
    on = z >= 0
    up, un = RR.residual(tabs, pos), RR.residual(tabs, neg)
    u = np.concatenate([up[on], un[on]])
    return {"z_zero": int(((z == 0) & (up != un).any(1)).sum()), "z_minus_one": int((z == -1).sum()),
            "u_zero_active": int((u == 0).sum()), "pos_eq_neg": int(np.all(pos == neg, 1).sum()),
            "h_eq_t": int((pos[:, 0] == pos[:, 1]).sum())}


def _tie_case(dims, l1):
    """Integer tables in [-2, 2], 64 pairs; the margin is the smallest integer >= 0 that puts one pair at z == 0
    and another at z == -1 (the first seed that has one, and a zero component of u on an active pair)."""
    E, R, B = 12, 3, 64
    for seed in range(200):
        rng = np.random.default_rng(seed)
        tabs = RR.integer_tables(E, R, *dims, seed=seed, amp=2)
        pos, neg = _pairs(rng, E, rng.integers(0, R, B))
        neg[TIE_POS_EQ_NEG] = pos[TIE_POS_EQ_NEG]
        pos[TIE_H_EQ_T, 1] = pos[TIE_H_EQ_T, 0]
        neg[TIE_H_EQ_T] = pos[TIE_H_EQ_T]
        neg[TIE_H_EQ_T, 1] = (pos[TIE_H_EQ_T, 1] + 1) % E
        d = score_diff(tabs, pos, neg, l1)
        have = set(d.tolist())
        for margin in range(0, 40):
            case = (tabs, pos, neg, float(margin), l1)
            if -margin in have and -margin - 1 in have and min(tie_conditions(case).values()) >= 1:
                return case
    raise AssertionError("no tie_and_sign fixture found")


# ------------------------------------------------------------------------------------ hot_entity, one pair per relation
def _hot_entity_case(l1):
    """E = 3, so each entity's run of gradient slots holds about 4 B / 3 of them.  The margin (an integer taken
    from the fixture) leaves a tenth of the pairs inactive."""
    E, R, B = 3, 2, 2000
    rng = np.random.default_rng(21)
    tabs = RR.integer_tables(E, R, 8, 8, seed=21, amp=1)
    pos, neg = _pairs(rng, E, rng.integers(0, R, B))
    margin = float(np.ceil(-np.quantile(score_diff(tabs, pos, neg, l1), 0.1)))
    return tabs, pos, neg, margin, l1


def entity_runs(case):
    """Active gradient slots per entity (the length of its run in the sorted slot array)."""
    tabs, pos, neg, margin, l1 = case
    on = score_diff(tabs, pos, neg, l1) + margin >= 0
    ids = np.concatenate([pos[on, 0], pos[on, 1], neg[on, 0], neg[on, 1]])
    return np.bincount(ids, minlength=len(tabs["ent"]))


def _one_pair_per_relation_case(l1):
    E, R = 40, 1500
    rng = np.random.default_rng(31)
    tabs = RR.integer_tables(E, R, 4, 4, seed=31, amp=1)
    pos, neg = _pairs(rng, E, rng.permutation(R))
    return tabs, pos, neg, 2.0, l1


# ------------------------------------------------------------------------------------ key_width
KEY_WIDTH_ER = ((2, 1), (64, 4), (128, 2), (1024, 1024))


def _key_width_case(er, l1):
    """About 15 % of the 300 pairs are invalid, a third each with an id >= E, a negative id, neg_r != pos_r; the
    highest entity and relation occur among the valid ones, and margin 2 leaves some valid pairs inactive, so both
    sentinels (R among the relation keys, E among the entity keys) are sorted."""
    E, R = er
    B, nbad = 300, 45
    rng = np.random.default_rng(41 + E)
    tabs = RR.integer_tables(E, R, 4, 4, seed=E + R, amp=1)
    pos, neg = _pairs(rng, E, rng.integers(0, R, B))
    pos[0], neg[0] = (E - 1, 0, R - 1), (E - 1, E - 1, R - 1)
    bad = 1 + rng.choice(B - 1, nbad, replace=False)
    pos[bad[:15], 0] = np.where(np.arange(15) % 2 == 0, E, 2 ** 31 - 1)
    neg[bad[15:30], 1] = np.where(np.arange(15) % 2 == 0, -1, -3)
    neg[bad[30:], 2] = (neg[bad[30:], 2] + 1) % R if R > 1 else R
    return tabs, pos, neg, 2.0, l1


def valid_only(case):
    tabs, pos, neg, margin, l1 = case
    ok = valid_mask(pos, neg, len(tabs["ent"]), len(tabs["rel"]))
    return tabs, pos[ok], neg[ok], margin, l1


# ------------------------------------------------------------------------------------ emap_wrap
def _emap_wrap_case(l1):
    E, R, B = 1000, 5, 140_000
    rng = np.random.default_rng(51)
    tabs = RR.integer_tables(E, R, 1, 1, seed=51, amp=1)
    pos, neg = _pairs(rng, E, rng.integers(0, R, B))
    return tabs, pos, neg, 1.0, l1


# ------------------------------------------------------------------------------------ the exact cases, by name
def _norm(l1):
    return "l1" if l1 else "l2"


_BUILDERS = {}
for _l1 in (True, False):
    for _d in DIMS:
        _BUILDERS[f"dims-{_d[0]}x{_d[1]}-{_norm(_l1)}"] = functools.partial(_dims_case, _d, _l1)
    for _d in ((100, 100), (8, 12)):
        _BUILDERS[f"misaligned-{_d[0]}x{_d[1]}-{_norm(_l1)}"] = functools.partial(_dims_case, _d, _l1)
    for _d in TIE_DIMS:
        _BUILDERS[f"tie_and_sign-{_d[0]}x{_d[1]}-{_norm(_l1)}"] = functools.partial(_tie_case, _d, _l1)
    _BUILDERS[f"hot_entity-{_norm(_l1)}"] = functools.partial(_hot_entity_case, _l1)
    _BUILDERS[f"one_pair_per_relation-{_norm(_l1)}"] = functools.partial(_one_pair_per_relation_case, _l1)
    for _er in KEY_WIDTH_ER:
        _BUILDERS[f"key_width-{_er[0]}x{_er[1]}-{_norm(_l1)}"] = functools.partial(_key_width_case, _er, _l1)
    _BUILDERS[f"emap_wrap-{_norm(_l1)}"] = functools.partial(_emap_wrap_case, _l1)
EXACT_NAMES = tuple(_BUILDERS)


def names(prefix):
    return [n for n in EXACT_NAMES if n.startswith(prefix + "-")]


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """(tabs, pos, neg, margin, l1) of one exact case.  A key_width case holds its invalid pairs; the step it must
    equal is the one on `valid_only(case)`, which is the exact fixture."""
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def exact_reference(name):
    """(loss, {table: fp64 gradient}) of one exact case, on its valid pairs."""
    tabs, pos, neg, margin, l1 = valid_only(exact_case(name))
    return RR.hinge_grads(tabs, pos, neg, margin, l1)


# ------------------------------------------------------------------------------------ adam_wrap
ADAM_WRAP = {"vec1": dict(E=1_100_003, R=1_100_003, dims=(1, 1)), "vec4": dict(E=1_050_000, R=270_000, dims=(4, 4))}
ADAM_T, ADAM_LR = 7, 2.0 ** -6
_MOMENT_PATTERN = np.array([1, -2, 3, -1, 2, -3, 4]) / 8.0


def cap_rows(rows, cols, vec):
    """The rows on both sides of the table element where the Adam loop starts its second round (element
    ADAM_UNIT_CAP * vec), or () if the table ends before it."""
    row = ADAM_UNIT_CAP * vec // cols
    return (row - 1, row) if row < rows else ()


@functools.lru_cache(maxsize=None)
def adam_wrap_case(which):
    """(tabs, pos, neg, margin, l1): integer tables in [-1, 1] and 64 valid pairs, all active at margin 1000, whose
    heads, tails and relations go through row 0, the last row and the rows on both sides of the cap."""
    spec = ADAM_WRAP[which]
    E, R, (dim_e, dim_r) = spec["E"], spec["R"], spec["dims"]
    vec = vec_for(dim_e, dim_r)
    rng = np.random.default_rng(61)
    tabs = RR.integer_tables(E, R, dim_e, dim_r, seed=61, amp=1)
    ent_rows = (0, E - 1) + cap_rows(E, dim_e, vec)
    rel_rows = (0, R - 1) + cap_rows(R, dim_r, vec) + cap_rows(R, dim_e * dim_r, vec)
    B = 64
    r = rng.integers(0, R, B)
    r[:len(rel_rows)] = rel_rows
    pos, neg = _pairs(rng, E, r)
    for q, e in enumerate(ent_rows):
        pos[q, 0] = neg[q, 0] = e                  # as a head, on both sides
        pos[8 + q, 1] = e                          # as a positive's tail
        neg[8 + q] = pos[8 + q]
        neg[8 + q, 1] = (e + 7) % E
    return tabs, pos, neg, 1000.0, True


def adam_wrap_rows(which):
    spec = ADAM_WRAP[which]
    E, R, (dim_e, dim_r) = spec["E"], spec["R"], spec["dims"]
    vec = vec_for(dim_e, dim_r)
    return ((0, E - 1) + cap_rows(E, dim_e, vec),
            (0, R - 1) + cap_rows(R, dim_r, vec) + cap_rows(R, dim_e * dim_r, vec))


def preset_moments(tabs):
    """({table: m}, {table: v}): non-zero on every element, m a small multiple of 1/8 and v its square."""
    m = {}
    for q, (k, x) in enumerate(tabs.items()):
        n = int(np.size(x))
        m[k] = _MOMENT_PATTERN[(np.arange(n) + q) % len(_MOMENT_PATTERN)].reshape(np.shape(x))
    return m, {k: x * x for k, x in m.items()}


# ------------------------------------------------------------------------------------ steps from non-integer tables
FLOAT_DIMS = ((100, 100), (100, 50), (33, 100), (256, 256))
FLOAT_E, FLOAT_R, FLOAT_B = 200, 10, 300


def xavier_tables(E, R, dim_e, dim_r, rng):
    """transr_ref.random_tables with each table at its Xavier-normal deviation sqrt(2 / (rows + cols)), rounded
    to fp32 so the GPU holds exactly these values."""
    tabs = RR.random_tables(E, R, dim_e, dim_r, rng)
    return {k: (x * np.sqrt(2.0 / sum(x.shape))).astype(np.float32).astype(np.float64) for k, x in tabs.items()}


def ambiguous_count(tabs, pos, neg, margin, l1):
    """fuzz_transr.py's rule: pairs whose z lies within its rounding bound of 0, plus (L1) components of u within
    theirs.  A fixture with a non-zero count could pass or fail on the mask alone."""
    dim_e, dim_r = RR.dims(tabs)
    z = score_diff(tabs, pos, neg, l1) + margin
    zmag = RR.score_magnitude(tabs, pos, l1) + RR.score_magnitude(tabs, neg, l1) + abs(margin)
    n = int((np.abs(z) <= (dim_e + dim_r + 8) * 4 * F32_EPS * zmag).sum())
    if l1:
        u = np.concatenate([RR.residual(tabs, pos), RR.residual(tabs, neg)])
        umag = np.concatenate([RR.residual_magnitude(tabs, t) for t in (pos, neg)])
        n += int((np.abs(u) <= (dim_e + 8) * 2 * F32_EPS * (umag + 1e-30)).sum())
    return n


def _gap_margin(d):
    """An fp32 margin in the middle of the widest gap between neighbouring values of -d that leaves at least a
    tenth of the pairs on either side (at most 1 above the gap's lower end)."""
    s = np.sort(-d)
    lo, hi = int(0.1 * len(s)), int(0.9 * len(s))
    q = lo + int(np.argmax(np.diff(s[lo:hi + 1])))
    return float(np.float32(s[q] + min(0.5 * (s[q + 1] - s[q]), 1.0)))


FAR, FAR_SCALE = 4, 64.0


def _float_batch(rng, E, R, B):
    """The Zipf batch, with the tail of its first fifth of negatives on one of the last FAR entities, whose rows
    are FAR_SCALE times Xavier's size.  With Xavier-sized rows M_r (h - t) is small against r, so D+ - D- of random
    pairs spreads over little more than the rounding bound of z, and no margin keeps every pair clear of the mask's
    edge.  A negative that ends on a far entity lies far behind its positive: these pairs are the inactive ones, and
    the gap they open holds the margin.  No other pair touches a far entity: it would carry large terms on both
    sides, and with them a rounding bound of z as wide as the margin."""
    pos, neg = RR.skewed_batch(rng, E - FAR, R, B)
    n = B // 5
    neg[:n] = pos[:n]
    neg[:n, 1] = E - FAR + np.arange(n) % FAR
    return pos, neg


def _clear_of_zero(tabs, pos, neg):
    """Moves entries of `rel` by 1/64 until no component of u of the batch lies within fuzz_transr.py's rounding
    bound of 0.  A batch of 300 pairs at dim_r = 100 has 60,000 components and the bound is about 1e-3 of their
    deviation, so no seed is free of them; u_k depends on rel[r][k] additively, so the move is exact to follow."""
    dim_e, _ = RR.dims(tabs)
    rel = tabs["rel"].copy()
    r = np.concatenate([pos[:, 2], neg[:, 2]]).astype(np.int64)
    u = np.concatenate([RR.residual(tabs, pos), RR.residual(tabs, neg)]) - rel[r]
    umag = np.concatenate([RR.residual_magnitude(tabs, t) for t in (pos, neg)]) - np.abs(rel[r])
    for _ in range(100):
        uu = u + rel[r]
        b, k = np.nonzero(np.abs(uu) <= 2 * (dim_e + 8) * 2 * F32_EPS * (umag + np.abs(rel[r])))    # twice the bound
        if len(b) == 0:
            return {**tabs, "rel": rel}
        cells = np.unique(np.stack([r[b], k], 1), axis=0)
        rel[cells[:, 0], cells[:, 1]] += 1.0 / 64
        rel = rel.astype(np.float32).astype(np.float64)
    raise AssertionError("could not clear u of zero")


@functools.lru_cache(maxsize=None)
def float_case(dims, l1, E=FLOAT_E, R=FLOAT_R, B=FLOAT_B):
    """(tabs, pos, neg, margin, l1) with Xavier-scaled tables and a Zipf batch: the first seed at which no pair is
    ambiguous (for L1, after `_clear_of_zero`)."""
    for seed in range(50):
        rng = np.random.default_rng(1000 * dims[0] + dims[1] + 7919 * seed)
        tabs = xavier_tables(E, R, *dims, rng)
        tabs["ent"][E - FAR:] *= FAR_SCALE
        pos, neg = _float_batch(rng, E, R, B)
        if l1:
            tabs = _clear_of_zero(tabs, pos, neg)
        margin = _gap_margin(score_diff(tabs, pos, neg, l1))
        if ambiguous_count(tabs, pos, neg, margin, l1) == 0:
            return tabs, pos, neg, margin, l1
    raise AssertionError("no unambiguous fixture found")


def adam_bounds(tabs, m0, v0, g, mag, n_pairs, b1, b2):
    """test_gpu_transr.py::test_twenty_dependent_adam_steps's element-wise bounds on m and v after one step from
    (m0, v0) with the fp64 gradient g, whose terms sum to mag in absolute value: {table: (mref, mtol, vref, vtol)}."""
    dim_e, dim_r = RR.dims(tabs)
    b1, b2 = np.float32(b1), np.float32(b2)
    out = {}
    for k in tabs:
        tol_g = (dim_e + dim_r + 2 * n_pairs) * 2 * F32_EPS * mag[k]
        mref = b1 * m0[k] + (1 - b1) * g[k]
        vref = b2 * v0[k] + (1 - b2) * g[k] ** 2
        mtol = 0.1 * tol_g + 4 * F32_EPS * (np.abs(m0[k]) + np.abs(g[k]))
        vtol = 0.001 * (2 * np.abs(g[k]) + tol_g) * tol_g + 4 * F32_EPS * (np.abs(v0[k]) + g[k] ** 2)
        out[k] = (mref, mtol, vref, vtol)
    return out
