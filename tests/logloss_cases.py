"""The workloads of tests/test_gpu_logloss_k.py and tests/test_logloss_cases_host.py: the --log_loss native loop
(ge_train_steps_logloss) at negative ratios of 16 to 1024, and the oracle replays it is held against.  Test
infrastructure only; nothing here needs a GPU.

A case is (B, K, d): M = (1 + K) B triples per step, sorted by table row in tiles of 4096 units and cut into work
items of <= 16 gradient slots of one row.  With K >= 16 every positive's relation row and its uncorrupted entity row
collect more than 16 slots, so most slots of a step sit in "multi" items that meet through float atomics.

Tolerances.  The loss keeps the project's bound 3e-5 * max(1, |loss|max).  The table bound of a case is
max(2e-5, 4 * D32): D32 is the largest difference between the oracle replayed with a float32 table and float32
scalars and the same oracle in float64 -- the reference arithmetic's own fp32 error over the case's steps -- and 4
is the margin for the kernels' different summation order (atomics, items of 16) and their expf / log1pf.  D32 is
measured on the host and stored beside each case; test_logloss_cases_host.py recomputes it."""
import functools
from collections import namedtuple

import numpy as np

from oracle import c_oracle as CO
from oracle import hole_oracle as O

SUB = 4096            # units per sort tile (kSub)
ITEM_CAP = 16         # gradient slots per work item (kItemCap)
LR0, DECAY_STEPS, DECAY_RATE, SEED, GS0 = 0.05, 40.0, 0.5, 77, 5
CALLS = (7, 13)       # every case runs 20 steps in two run() calls
STEPS = sum(CALLS)
LONG_STEPS = 40       # one_tile_full again, over a chunk boundary of 32 steps

# d32: max |fp32 replay - fp64 replay| over the final table after STEPS steps (measured value in the comment)
Case = namedtuple("Case", "name B K d l2 tiles tri_seed d32")
CASES = (
    Case("one_tile_full", 16, 255, 50, 2e-6, 1, 19, 2.3e-6),       # measured 2.30e-6,
    Case("tile_plus_one", 17, 240, 50, 2e-6, 2, 19, 3.3e-6),       # measured 3.34e-6,
    Case("tile_plus_k1024", 4, 1024, 64, 2e-6, 2, 20, 3.9e-6),     # measured 3.86e-6,
    Case("two_tiles_exact", 32, 255, 200, 2e-6, 2, 19, 3.4e-6),    # measured 3.43e-6,
    Case("config5_small", 64, 256, 50, 2e-6, 5, 19, 1.2e-5),       # measured 1.21e-5: bound 4.8e-5,
    Case("k16_edge", 241, 16, 50, 1e-5, 2, 19, 8.0e-7),            # measured 7.95e-7,
)
BY_NAME = {c.name: c for c in CASES}
D32_LONG = 9.6e-6     # one_tile_full over LONG_STEPS steps (measured 9.59e-6: bound 3.8e-5)


def units(c):
    return (1 + c.K) * c.B


def table_tol(d32):
    return max(2e-5, 4.0 * d32)


def loss_tol(oloss):
    return 3e-5 * max(1.0, float(np.abs(oloss).max()))


@functools.lru_cache(maxsize=None)
def type_arrays():
    from graphembeddings_amd import data as D
    fb = D.fb15k_shape()
    names, id_to_type, offsets, ids = fb.type_arrays()
    return fb, id_to_type, offsets, ids


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def workload(B, d, tri_seed=19):
    """(triples [6B+31, 3] int32, table [N, d] float32 with every fifth row nine times as long)."""
    from graphembeddings_amd import data as D
    fb = type_arrays()[0]
    tri = D.synthetic_fb15k_triples(fb, n_triples=6 * B + 31, seed=tri_seed)
    table = O.init_table(fb.entity_count, d, seed=9)
    table[::5] *= 9.0
    return _frozen(tri), _frozen(table)


def learning_rate(gs, lr0=LR0, decay_steps=DECAY_STEPS, decay_rate=DECAY_RATE):
    """inverse-time decay formed in float32, as the native loop forms it"""
    if decay_steps <= 0:
        return np.float32(lr0)
    return np.float32(lr0) / (np.float32(1.0) + np.float32(decay_rate) * (np.float32(gs) / np.float32(decay_steps)))


def batches(tri, B, K, steps, seed, gs0, id_to_type=None):
    """[(pos [B,3], negs [K,B,3])] of `steps` consecutive steps: batches wrap to row 0 where one would run past the
    array, the k-th corrupted batch of global step gs is drawn with Philox step key gs * K + k."""
    _, itt, offsets, ids = type_arrays()
    if id_to_type is not None:
        itt = id_to_type
    out, row, T = [], 0, len(tri)
    for s in range(steps):
        if row + B > T:
            row = 0
        pos = tri[row:row + B]
        gs = gs0 + s
        negs = np.stack([CO.corrupt_batch(pos, itt, offsets, ids, seed, gs * K + k, 1024, 0) for k in range(K)])
        out.append((pos, _frozen(negs)))
        row += B
    return out


@functools.lru_cache(maxsize=None)
def case_batches(name, steps=STEPS):
    c = BY_NAME[name]
    tri, _ = workload(c.B, c.d, c.tri_seed)
    return tuple(batches(tri, c.B, c.K, steps, SEED, GS0))


def replay(table, bats, l2, dtype=np.float64, gs0=GS0, lr0=LR0, decay_steps=DECAY_STEPS, decay_rate=DECAY_RATE):
    """`len(bats)` dependent steps of oracle.hole_oracle.logloss_step in `dtype` (float32: table, lr and l2 all
    float32 -- the reference arithmetic's own rounding).  Returns (final table, [loss vector per step])."""
    t = np.array(table, dtype=dtype)
    losses = []
    for s, (pos, negs) in enumerate(bats):
        lr = learning_rate(gs0 + s, lr0, decay_steps, decay_rate)
        if dtype == np.float32:
            t, loss = O.logloss_step(t, pos, negs, np.float32(lr), np.float32(l2))
            assert t.dtype == np.float32
        else:
            t, loss = O.logloss_step(t, pos, negs, float(lr), l2)
        losses.append(_frozen(loss))
    return _frozen(t), losses


@functools.lru_cache(maxsize=None)
def case_replay(name, steps=STEPS, fp32=False):
    """The fp64 (or fp32) replay of a case: (final table, losses).  Computed once per process and read-only."""
    c = BY_NAME[name]
    _, table = workload(c.B, c.d, c.tri_seed)
    return replay(table, case_batches(name, steps), c.l2, np.float32 if fp32 else np.float64)


def measure_d32(name, steps=STEPS):
    t64, _ = case_replay(name, steps)
    t32, _ = case_replay(name, steps, True)
    return float(np.abs(t32.astype(np.float64) - t64).max())


def step_triples(pos, negs):
    """[M,3] in the loss vector's order: the positives, then the K corrupted batches"""
    return np.concatenate([pos, np.asarray(negs).reshape(-1, 3)], 0)


def slot_counts(triples, n_rows):
    """gradient slots per table row of one step (three per triple with all ids inside [0, n_rows))"""
    ok = ((triples >= 0) & (triples < n_rows)).all(1)
    return np.bincount(triples[ok].reshape(-1), minlength=n_rows)


def row_classes(counts):
    """rows of a step with exactly 1 slot, 2-16, 17-256, more than 256"""
    return (int((counts == 1).sum()), int(((counts >= 2) & (counts <= ITEM_CAP)).sum()),
            int(((counts > ITEM_CAP) & (counts <= 256)).sum()), int((counts > 256).sum()))


def class_of_rows(counts, rows):
    """for a failure report: how many of `rows` fall in each slot class (0 slots first)"""
    c = counts[rows]
    return {"untouched": int((c == 0).sum()), "1": int((c == 1).sum()), "2-16": int(((c >= 2) & (c <= 16)).sum()),
            "17-256": int(((c > 16) & (c <= 256)).sum()), ">256": int((c > 256).sum())}


def drop_one_slot(table64, pos, negs, lr, l2):
    """One fp64 oracle step, and the same step without ONE gradient slot of the row that collects the most slots: the
    slot that moves the row most.  Returns (row, slots of the row, full row, row without the slot, the median over the
    row's slots of what one slot moves)."""
    tri = step_triples(pos, negs)
    new, _ = O.logloss_step(table64, pos, negs, lr, l2)
    counts = slot_counts(tri, table64.shape[0])
    row = int(counts.argmax())
    labels = np.concatenate([np.ones(len(pos)), -np.ones(len(tri) - len(pos))])
    ii, cols = np.nonzero(tri == row)
    sub = tri[ii]
    s = O.complex_score(sub, table64, 1.0)
    coef = -labels[ii] * O.sigmoid(-labels[ii] * s)
    g3 = O._side_grads(sub, table64, coef, 1.0, "complex")
    g = np.stack([g3[c][n] for n, c in enumerate(cols)])           # [slots, d]: each slot's gradient row
    moves = np.abs(lr * g).max(1)
    k = int(moves.argmax())
    return row, len(ii), new[row], new[row] + lr * g[k], float(np.median(moves))


def scalar_crossings(lr, l2, M, steps):
    """The step indices at which train_logloss_run's carried scalar g (actual table = g * stored table) would leave
    [9.1e-13, 1.1e12] or become 0 -- there the table is materialised and g starts again at 1.  Same arithmetic as the
    host loop: lr and l2 are float32 values, their product with M is formed in double."""
    f = 1.0 - float(np.float32(lr)) * float(M) * float(np.float32(l2))
    g, out = 1.0, []
    for s in range(steps):
        g_new = g * f
        if g_new == 0.0 or abs(g_new) < 9.1e-13 or abs(g_new) > 1.1e12:
            out.append(s)
            g_new = 1.0
        g = g_new
    return out


# non-zero table rows after step 1 and step 2 of test_dense_factor_exactly_zero (B 512, K 1: the rows the step names)
ZERO_FACTOR_ROWS = (1194, 569)

# ------------------------------------------------------------------ triples with an id outside [0, N)
Invalid = namedtuple("Invalid", "B K d l2 steps share type_seed d32")
INVALID = Invalid(64, 32, 50, 2e-6, 3, 0.05, 9, 3.1e-7)     # d32 measured 3.14e-7; 82, 106, 98 invalid triples per step


@functools.lru_cache(maxsize=None)
def invalid_workload():
    """one_tile-sized loop (M = 2112) over type tables in which `share` of the entity ids have type -1: corrupting
    such an entity gives the id -1 (oracle.hole_oracle.corrupt_batch).  Returns (id_to_type, triples, table, batches)."""
    iv = INVALID
    fb, id_to_type, _, _ = type_arrays()
    itt = np.array(id_to_type)
    ent = np.arange(fb.relation_count, fb.entity_count)
    rng = np.random.default_rng(iv.type_seed)
    itt[rng.choice(ent, size=int(round(iv.share * len(ent))), replace=False)] = -1
    tri, table = workload(iv.B, iv.d)
    return _frozen(itt), tri, table, tuple(batches(tri, iv.B, iv.K, iv.steps, SEED, GS0, id_to_type=itt))


def masked_step(t, tri, n_pos, lr, l2):
    """One --log_loss step in which the triples with an id outside [0, N) have a NaN loss and no gradient, while
    the dense factor 1 - lr M l2 still counts all M triples.  Only valid ids reach the oracle's functions.
    Returns (new table, loss [M], invalid [M] bool)."""
    N, M = t.shape[0], len(tri)
    bad = ~((tri >= 0) & (tri < N)).all(1)
    y = np.concatenate([np.ones(n_pos), -np.ones(M - n_pos)]).astype(t.dtype)[~bad]
    v = tri[~bad]
    loss = np.full(M, np.nan, t.dtype)
    loss[~bad] = O.logloss_values(v, y, t, l2)
    coef = -y * O.sigmoid(-y * O.complex_score(v, t, 1.0))
    gh, gt, gr = O._side_grads(v, t, coef, 1.0, "complex")
    new = t * (1.0 - lr * M * l2)
    for col, g in enumerate((gh, gt, gr)):
        np.subtract.at(new, v[:, col], lr * g)
    return new, loss, bad


@functools.lru_cache(maxsize=None)
def invalid_replay(fp32=False):
    """(final table, [loss per step], [invalid mask per step]) of the invalid-id loop, float64 or float32"""
    iv = INVALID
    _, _, table, bats = invalid_workload()
    t = np.array(table, dtype=np.float32 if fp32 else np.float64)
    losses, bads = [], []
    for s, (pos, negs) in enumerate(bats):
        lr = learning_rate(GS0 + s)
        lr, l2 = (np.float32(lr), np.float32(iv.l2)) if fp32 else (float(lr), iv.l2)
        t, loss, bad = masked_step(t, step_triples(pos, negs), len(pos), lr, l2)
        assert t.dtype == (np.float32 if fp32 else np.float64)
        losses.append(_frozen(loss))
        bads.append(_frozen(bad))
    return _frozen(t), losses, bads


def measure_invalid_d32():
    return float(np.abs(invalid_replay(True)[0].astype(np.float64) - invalid_replay()[0]).max())
