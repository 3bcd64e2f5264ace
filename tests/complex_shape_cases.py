"""The cases of tests/test_gpu_complex_shapes.py and tests/test_complex_shape_cases_host.py: one ComplEx / HolE training
step at every instantiation the 12-way shape switch of graphembeddings_amd/csrc/ge_complex.hip can reach, and a
restatement of the dispatch that decides which instantiation -- of the gradient kernels and of the update kernels of
ge_train.hip -- a case runs.  Test infrastructure only; nothing here needs a GPU.

The dispatch, restated: `pick_shape` (embedding_dim, table alignment) -> (VEC, LPT, NITER), GE_DISPATCH_SHAPE's key ->
instantiation map, `apply_items_launch`'s (VW, NJ, RW) and hot_rows_kernel's NJ, and `prep_layout`'s tile count.

The workloads (seeded, built once per process, read-only): `small` (one tile, `same` pairs, sole-slot rows, hot
relation rows), `two_tiles` (4100 pairs: relation order, run sums, LDS merge), `untyped` (`small` with entities of
type -1: invalid pairs) and the 67-pair batch of the single-step API.

Tolerances.  The project's bars (tests/test_gpu_parity.py): losses 1e-5, the table 5e-6 after one step without hot
rows and 2e-5 with them.  Whether a bar holds at d = 1024, over three dependent steps with every relation row hot, is
decided on the CPU from references alone: GAP is the largest difference between an independent fp32 implementation
of the case (the C port oracle/ge_oracle.c for ComplEx and direct-correlation HolE, a float32 torch.fft restatement of
README.md:42 for HolE in the frequency domain) and the fp64 oracle; the bound is max(bar, 4 * GAP) -- two fp32
roundings of one quantity differ by up to twice one's own error, and another summation order (lane slices, tree
reductions, float atomics on hot rows) gets the same again.  GAPS holds the measured values;
test_complex_shape_cases_host.py recomputes them.  The log-loss cases keep logloss_cases.table_tol's rule (the
oracle's own fp32 replay), the AdaGrad cases the derived bounds of test_gpu_adagrad.py."""
import functools
import os
import re
from collections import namedtuple

import numpy as np

from oracle import c_oracle as CO
from oracle import hole_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphembeddings_amd", "csrc")
F32 = np.float32

# ------------------------------------------------------------------------------------ the dispatch, restated
# ge_common.h: kWave, kBlock, kMaxBlocks; ge_prep.h: kSub, kItemCap; ge_train.hip: kOneTileRowRegs
K_WAVE, K_BLOCK, K_MAX_BLOCKS, K_SUB, K_ITEM_CAP, K_ONE_TILE_ROW_REGS = 64, 256, 2048, 4096, 16, 64
MAX_DIM = 1024                  # complex_max_dim(), what ge_max_dim() advertises
HOLE_DIRECT_MAX_DIM = 512       # hole_max_dim(): the direct-correlation kernels of ge_hole.hip
ORD_FROM_B = K_SUB + 1          # the first batch size whose steps carry order[B]


def source_constants():
    """{name: value} of the `constexpr int` constants above, read out of the sources as text."""
    out = {}
    for fn in ("ge_common.h", "ge_prep.h", "ge_train.hip"):
        with open(os.path.join(CSRC, fn)) as f:
            for name, expr in re.findall(r"constexpr\s+(?:int|int64_t)\s+(k\w+)\s*=\s*([0-9][0-9 *]*);", f.read()):
                out[name] = int(np.prod([int(x) for x in expr.split("*")]))
    return out


def pick_shape(d, alignment_bytes=16, ld=0, max_niter=2):
    """ge_complex.hip's pick_shape: (VEC, LPT, NITER) of an embedding_dim on a table whose first byte lies on an
    `alignment_bytes` boundary and no wider one (4, 8 or 16), rows `ld` floats apart (0: dense); None where it refuses."""
    if d <= 0 or d & 1:
        return None
    k = d // 2
    vec = 4 if k % 4 == 0 else 2 if k % 2 == 0 else 1
    while vec > 1 and (alignment_bytes % (vec * 4) != 0 or ld % vec != 0):
        vec >>= 1
    nvec = k // vec
    lpt = 16
    while lpt < 64 and lpt < nvec:
        lpt <<= 1
    niter = -(-nvec // lpt)
    if niter > 2:
        niter = 4
    if niter > max_niter:
        return None
    return vec, lpt, niter


def shape_key(d, alignment_bytes=16):
    """GE_DISPATCH_SHAPE's key of pick_shape's answer, None where pick_shape refuses (GE_ENOTSUP)."""
    s = pick_shape(d, alignment_bytes)
    return None if s is None else s[0] * 1000 + s[1] * 10 + s[2]


# GE_DISPATCH_SHAPE: key -> the (VEC, LPT, NITER) its CALL is instantiated with
DISPATCH = {1161: (1, 16, 1), 1321: (1, 32, 1), 1641: (1, 64, 1), 1642: (1, 64, 2),
            2161: (2, 16, 1), 2321: (2, 32, 1), 2641: (2, 64, 1), 2642: (2, 64, 2),
            4161: (4, 16, 1), 4162: (4, 16, 2), 4322: (4, 32, 2), 4321: (4, 32, 1), 4641: (4, 64, 1), 4642: (4, 64, 2)}
UNREACHABLE_KEYS = (4162, 4322)     # listed in the switch, produced by no embedding_dim
REACHABLE_KEYS = tuple(sorted(set(DISPATCH) - set(UNREACHABLE_KEYS)))


def source_dispatch():
    """The same map read out of the GE_DISPATCH_SHAPE macro as text."""
    with open(os.path.join(CSRC, "ge_complex.hip")) as f:
        text = f.read()
    body = text[text.index("#define GE_DISPATCH_SHAPE"):text.index("#define GE_DISPATCH_SPEC")]
    return {int(k): (int(v), int(l), int(n)) for k, v, l, n in
            re.findall(r"case (\d+): \{ CALL\((\d+), (\d+), (\d+)\); \}", body)}


def one_tile_rows(regs_per_row):
    """ge_train.hip's one_tile_rows: gradient rows a wave of the one-tile update kernel holds in flight."""
    r = K_ONE_TILE_ROW_REGS // regs_per_row
    return K_ITEM_CAP if r > K_ITEM_CAP else 2 if r < 2 else r


def _bucket(n, buckets):
    for b in buckets:
        if n <= b:
            return b
    return None


def apply_items_choice(d, alignment_bytes, n_sub, det=False):
    """What apply_items_launch launches for a training loop's step (gidx given, no second output; the gradient rows lie
    on a 256-byte boundary of the workspace, so the table's alignment decides): dict(kernel, vw, nj, rw, hot_nj) --
    apply_rows_kernel<VW, NJ, DET, RW> (RW = 0: the multi-tile form) and, with det, hot_rows_kernel<hot_nj> -- or None
    where it answers GE_ENOTSUP."""
    nj = -(-d // K_WAVE)
    if det and nj > 16:
        return None
    hot = _bucket(nj, (1, 2, 4, 8, 16)) if det else None
    vw = 4 if d % 4 == 0 and alignment_bytes % 16 == 0 else 2 if d % 2 == 0 and alignment_bytes % 8 == 0 else 1
    njr = -(-(d // vw) // K_WAVE)
    NJ = _bucket(njr, {4: (1, 2, 4), 2: (1, 2, 4, 8), 1: (1, 2, 4, 8, 16)}[vw])
    if NJ is not None:
        return dict(kernel="apply_rows", vw=vw, nj=NJ, rw=one_tile_rows(vw * NJ) if n_sub == 1 else 0, hot_nj=hot)
    NJ = _bucket(nj, (1, 2, 4, 8, 16))
    return None if NJ is None else dict(kernel="apply_sorted", vw=1, nj=NJ, rw=0, hot_nj=hot)


def prep_layout(B, negs=0):
    """ge_prep.h's prep_layout, the part the dispatch depends on: (tiles of a step, whether it carries order[B])."""
    units = (1 + negs) * B if negs > 0 else B
    n_sub = -(-units // K_SUB)
    return n_sub, negs == 0 and n_sub > 1


def route(model, d, alignment_bytes=16):
    """The kernels Trainer.run's hinge loop takes a (model, embedding_dim, table alignment) to: "complex" / "spectral"
    (the ComplEx-shaped kernels, SPEC on the transformed table), "direct" (ge_hole.hip on the real table) or None
    (GE_ENOTSUP, nothing launched)."""
    ok = pick_shape(d, alignment_bytes) is not None
    if model == "complex":
        return "complex" if ok else None
    if model == "hole_spectral":
        return "spectral" if ok else None
    assert model == "hole"
    if ok:
        return "spectral"
    return "direct" if d <= HOLE_DIRECT_MAX_DIM else None


# ------------------------------------------------------------------------------------ the cases
# both ends of every key: the fewest and the most vectors a row of that key has (aligned table)
DIMS = {1161: (2, 30), 1321: (34, 62), 1641: (66, 126), 1642: (130, 254),
        2161: (4, 60), 2321: (68, 124), 2641: (132, 252), 2642: (260, 508),
        4161: (8, 128), 4321: (136, 256), 4641: (264, 512), 4642: (520, 1024)}
LOW = tuple(DIMS[k][0] for k in REACHABLE_KEYS)
HIGH = tuple(DIMS[k][1] for k in REACHABLE_KEYS)
ONE_LIVE_LANE = (130, 260, 520)               # NITER = 2 with one live lane in the second iteration
# (embedding_dim, byte offset of the table from a 16-byte boundary): refused by every ComplEx-shaped kernel
REFUSED = ((258, 0), (1022, 0), (512, 4), (520, 8))
# (embedding_dim, offset, key): tables off the boundary; d = 100 adds apply_rows_kernel<1, 2> and 264 at +8 <2, 4>
MISALIGNED = ((64, 4, 1321), (200, 4, 1642), (256, 4, 1642), (64, 8, 2161), (200, 8, 2641), (256, 8, 2641),
              (100, 4, 1641), (100, 8, 2321), (264, 8, 2642))
UNTYPED_DIMS = (130, 200)
HOLE_TWO_TILES = ONE_LIVE_LANE
HOLE_DIRECT = ((258, 0), (512, 4))            # REFUSED cases model = hole still trains, on the direct kernels


def alignment_of(offset):
    return 16 if offset % 16 == 0 else 8 if offset % 8 == 0 else 4


MARGIN, LR0, DECAY_STEPS, DECAY_RATE, SEED, PADDED = 0.1, 0.1, 50.0, 0.5, 21, 1024
STEP_LR = 0.1                                 # the single-step tests'
LOGLOSS_B, LOGLOSS_K, LOGLOSS_L2 = 100, 2, 2e-6
A0 = 0.1                                      # AdaGrad's initial accumulator value (test_gpu_adagrad.py's)

# name, table rows, relation rows, pairs a step, triples, steps, first row, first global step
Workload = namedtuple("Workload", "name N n_rel B T steps row0 gs0 untyped")
WORKLOADS = {
    # rows 900, 1200, then the batch at 1500 would pass T = 1577: row 0
    "small": Workload("small", 2048, 8, 300, 5 * 300 + 77, 3, 3 * 300, 3, 0.0),
    # row 4100, then 8200 + 4100 > T: row 0
    "two_tiles": Workload("two_tiles", 20000, 8, 4100, 2 * 4100 + 77, 2, 4100, 3, 0.0),
    "untyped": Workload("untyped", 2048, 8, 300, 5 * 300 + 77, 3, 3 * 300, 3, 0.09),
    # the log-loss loop on `small`'s triples: rows 1327, 1427, then row 0
    "logloss": Workload("logloss", 2048, 8, LOGLOSS_B, 5 * 300 + 77, 3, 5 * 300 + 77 - 250, 3, 0.0),
}
SINGLE_ENTITY_SHARE = 0.06                    # of the heads and of the tails: the one entity of type 0


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def graph(name):
    """(id_to_type [N], type_offsets, type_ids, triples [T,3]) of a workload.  Rows [0, n_rel) are relations (type -1),
    row n_rel is the only entity of type 0 -- corrupting it gives itself -- and the others alternate between types 1
    and 2; `untyped` sets a share of the entities' types to -1, whose corruption is the id -1."""
    w = WORKLOADS[name]
    rng = np.random.default_rng({"small": 5, "two_tiles": 6, "untyped": 5, "logloss": 5}[name])
    ent = np.arange(w.n_rel, w.N)
    id_to_type = np.full(w.N, -1, np.int32)
    id_to_type[ent] = 1 + (ent % 2)
    id_to_type[w.n_rel] = 0
    lists = [ent[id_to_type[ent] == t] for t in range(3)]
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    ids = np.concatenate(lists).astype(np.int32)
    tri = np.stack([rng.integers(w.n_rel + 1, w.N, w.T), rng.integers(w.n_rel + 1, w.N, w.T),
                    rng.integers(0, w.n_rel, w.T)], 1).astype(np.int32)
    for col in (0, 1):
        tri[rng.random(w.T) < SINGLE_ENTITY_SHARE, col] = w.n_rel
    if w.untyped:
        lost = np.random.default_rng(9).choice(ent[1:], size=int(round(w.untyped * len(ent))), replace=False)
        id_to_type[lost] = -1
    return _frozen(id_to_type), _frozen(offsets), _frozen(ids), _frozen(tri)


HEAVY = 0.8                                   # share of a ComplEx row's norm on its last complex element


def heavy_share(how, d):
    """With random rows the scores shrink like 1 / sqrt(d), every pair ends up hinge-active and the loss no longer
    depends on any single lane.  So every row carries this share of its norm, at a random phase, on its LAST complex
    element -- the one the tail lane of the low ends holds alone -- and the rest as noise.  Three aligned unit rows
    then score HEAVY^3 whatever d is; a sinusoid's HolE score grows like sqrt(d / 2), which HolE's share takes out."""
    return HEAVY if how == "complex" else HEAVY * min(1.0, (2.0 / d) ** (1.0 / 6.0))


def packed_to_real(S):
    """Rows of packed half spectra [Re X_0 .. Re X_{k-1} | Re X_k, Im X_1 .. Im X_{k-1}] (ge_hole_to_spectral's
    layout) -> the real rows they are the DFT of."""
    k = S.shape[1] // 2
    X = np.zeros((S.shape[0], k + 1), np.complex128)
    X[:, :k] = S[:, :k]
    X[:, k] = S[:, k]
    X[:, 1:k] += 1j * S[:, k + 1:]
    return np.fft.irfft(X, n=2 * k, axis=1)


@functools.lru_cache(maxsize=None)
def table_of(n_rows, d, seed, how="complex"):
    """[n_rows, d] float32: a third of the rows past the unit ball (norms 1.1 - 2.0: the clip and its Jacobian are
    live), the others at norms 0.4 - 1.0; heavy_share of each norm on the last complex element (HolE: of the row's
    spectrum), the rest random."""
    rng = np.random.default_rng(1000 * d + seed)
    k = d // 2
    a = heavy_share(how, d)
    noise = rng.standard_normal((n_rows, d))
    if k > 1:
        noise[:, [k - 1, d - 1]] = 0.0
    w = np.ones(d)                            # Parseval weights of the packed layout (HolE): X_0 and X_k count once
    if how != "complex":
        w[:] = 2.0
        w[[0, k]] = 1.0
    theta = rng.uniform(0.0, 2.0 * np.pi, n_rows)
    t = noise * (np.sqrt(1.0 - a * a) / np.sqrt((noise * noise * w).sum(1)))[:, None]
    if k > 1:
        amp = a / np.sqrt(w[k - 1])
        t[:, k - 1], t[:, d - 1] = amp * np.cos(theta), amp * np.sin(theta)
    if how != "complex":
        t = packed_to_real(t)
    big = rng.random(n_rows) < 1.0 / 3.0
    norm = np.where(big, rng.uniform(1.1, 2.0, n_rows), rng.uniform(0.4, 1.0, n_rows))
    t *= (norm / np.linalg.norm(t, axis=1))[:, None]
    return _frozen(t.astype(F32))


def learning_rate(gs):
    """inverse-time decay formed in float32, as the native loops form it"""
    return float(F32(LR0) / (F32(1.0) + F32(DECAY_RATE) * (F32(gs) / F32(DECAY_STEPS))))


@functools.lru_cache(maxsize=None)
def batches(name):
    """((pos [B,3], neg [B,3], global step, first row), ...) of the workload's steps, and the row the loop ends on:
    batches wrap to row 0 where one would pass the array, negatives from the loop's Philox keys."""
    w = WORKLOADS[name]
    itt, offsets, ids, tri = graph(name)
    out, row = [], w.row0
    for s in range(w.steps):
        if row + w.B > w.T:
            row = 0
        pos = tri[row:row + w.B]
        gs = w.gs0 + s
        if name == "logloss":
            neg = np.stack([CO.corrupt_batch(pos, itt, offsets, ids, SEED, gs * LOGLOSS_K + k, PADDED, 0)
                            for k in range(LOGLOSS_K)])
        else:
            neg = CO.corrupt_batch(pos, itt, offsets, ids, SEED, gs, PADDED, 0)
            assert np.array_equal(neg, O.corrupt_batch(pos, itt, offsets, ids, SEED, gs, PADDED, 0))
        out.append((pos, _frozen(neg), gs, row))
        row += w.B
    return tuple(out), row


def valid_pairs(pos, neg, n_rows):
    """train_prepare_kernel's unit_keys / the gradient kernels' `bad`, negated: every id of the pair inside the table."""
    both = np.concatenate([pos, neg], 1)
    return ((both >= 0) & (both < n_rows)).all(1)


def pre_activation(t64, pos, neg, omodel):
    """sigma(s+) - sigma(s-) + margin of every pair: the hinge's argument (its kink is at 0)."""
    sfun = O.complex_score if omodel == "complex" else O.hole_score
    return O.sigmoid(sfun(pos, t64)) - O.sigmoid(sfun(neg, t64)) + MARGIN


def slot_counts(pos, neg, n_rows, on=None):
    """gradient slots per table row of one hinge step: the positive's three rows and the negative's differing ones
    (of the pairs `on`, default all)."""
    if on is None:
        on = np.ones(len(pos), bool)
    r = np.concatenate([pos[on].ravel(), neg[on][pos[on] != neg[on]]])
    return np.bincount(r, minlength=n_rows)


# ------------------------------------------------------------------------------------ references of one hinge step
def torch_fft_step32(table32, pos, neg, lr):
    """One HolE step in float32 on the CPU: README.md:42's FFT formula with torch.fft, differentiated by autograd
    (test_gpu_parity.py::test_hole_step_matches_torch_fft_autograd_on_device, off the device).  In place on table32;
    returns the losses."""
    import torch
    d, B = table32.shape[1], len(pos)
    ref = torch.from_numpy(table32)
    idx = torch.from_numpy(np.concatenate([pos, neg], 0).astype(np.int64))
    rows = [ref[idx[:, c]].detach().requires_grad_(True) for c in range(3)]
    h, t, r = [x * torch.clamp(torch.rsqrt((x * x).sum(1, keepdim=True)), max=1.0) for x in rows]
    corr = torch.fft.irfft(torch.conj(torch.fft.rfft(h, dim=1)) * torch.fft.rfft(t, dim=1), n=d, dim=1)
    e = torch.sigmoid((r * corr).sum(1))
    loss = torch.clamp(e[:B] - e[B:] + F32(MARGIN), min=0.0)
    loss.sum().backward()
    with torch.no_grad():
        for c in range(3):
            ref.index_add_(0, idx[:, c], rows[c].grad, alpha=-float(lr))
    return loss.detach().numpy()


def step32(table32, pos, neg, lr, how):
    """One hinge step of an independent fp32 implementation, in place on table32: how = "complex" / "direct" (the C
    port) or "spectral" (torch.fft).  Returns the losses."""
    if how == "spectral":
        return torch_fft_step32(table32, pos, neg, lr)
    return CO.hinge_step(table32, pos, neg, MARGIN, float(lr), hole=(how == "direct"), threads=4)


Replay = namedtuple("Replay", "table losses on kink row_end")


def _replay(table, steps, how, fp32):
    """Dependent hinge steps [(pos, neg, lr)] from `table`: fp64 oracle, or the fp32 implementation of `how`.  A pair
    with an id outside the table has loss NaN and no gradient.  Returns Replay(final table, [loss per step], [the
    hinge-active mask per step], the smallest |pre-activation| over all steps (fp64 only), None)."""
    omodel = "complex" if how == "complex" else "hole"
    t = np.array(table, dtype=F32 if fp32 else np.float64)
    losses, ons, kink = [], [], np.inf
    for pos, neg, lr in steps:
        ok = valid_pairs(pos, neg, len(t))
        loss = np.full(len(pos), np.nan, t.dtype)
        p, n = np.ascontiguousarray(pos[ok]), np.ascontiguousarray(neg[ok])
        if fp32:
            loss[ok] = step32(t, p, n, lr, how)
        else:
            pre = pre_activation(t, p, n, omodel)
            kink = min(kink, float(np.abs(pre).min()))
            on = np.zeros(len(pos), bool)
            on[ok] = pre >= 0
            ons.append(_frozen(on))
            t, loss[ok] = O.sgd_step(t, p, n, lr=lr, margin=MARGIN, model=omodel)
        losses.append(_frozen(loss))
    return Replay(_frozen(t), losses, ons, kink, None)


# ------------------------------------------------------------------------------------ loop cases
LoopCase = namedtuple("LoopCase", "workload model d offset how")


def loop_case(workload, model, d, offset=0):
    how = route(model, d, alignment_of(offset))
    assert how is not None, (model, d, offset)
    return LoopCase(workload, model, d, offset, how)


def loop_table(c):
    w = WORKLOADS[c.workload]
    return table_of(w.N, c.d, TABLE_SEEDS.get((c.workload, c.how, c.d), 0), c.how)


@functools.lru_cache(maxsize=None)
def loop_replay(workload, how, d, fp32=False):
    """The replay of a loop case (its values do not depend on where the table lies)."""
    w = WORKLOADS[workload]
    bats, row_end = batches(workload)
    table = table_of(w.N, d, TABLE_SEEDS.get((workload, how, d), 0), how)
    r = _replay(table, [(p, n, learning_rate(gs)) for p, n, gs, _ in bats], how, fp32)
    return r._replace(row_end=row_end)


def gap_of(r32, r64):
    """(loss gap, table gap) between an fp32 replay and the fp64 one; the NaN losses must coincide."""
    gl = 0.0
    for a, b in zip(r32.losses, r64.losses):
        assert np.array_equal(np.isnan(a), np.isnan(b))
        live = ~np.isnan(b)
        gl = max(gl, float(np.abs(a[live].astype(np.float64) - b[live]).max()))
    return gl, float(np.abs(r32.table.astype(np.float64) - r64.table).max())


def measure_loop_gap(workload, how, d):
    return gap_of(loop_replay(workload, how, d, True), loop_replay(workload, how, d))


# The hinge-loop runs of test_gpu_complex_shapes.py, by test: (test, workload, model, d, table offset, deterministic)
LOOP_RUNS = (
    [("b", "small", m, d, 0, False) for m in ("complex", "hole") for d in LOW]
    + [("b", "small", "complex", d, 0, False) for d in HIGH]
    + [("c", "two_tiles", "complex", d, 0, False) for d in LOW]
    + [("c", "two_tiles", "hole", d, 0, False) for d in HOLE_TWO_TILES]
    # (the tables off the boundary again, for the multi-tile update kernel's VW = 1 and <2, 4>)
    + [("c", "two_tiles", "complex", d, off, False) for d, off, _ in MISALIGNED]
    + [("d", "small", "complex", d, 0, True) for d in LOW]
    + [("g", "small", m, d, off, False) for m in ("complex", "hole") for d, off, _ in MISALIGNED]
    + [("h", "untyped", "complex", d, 0, False) for d in UNTYPED_DIMS]
    + [("i", "small", "hole", d, off, False) for d, off in HOLE_DIRECT])


def runs_of(test):
    return [r[1:] for r in LOOP_RUNS if r[0] == test]


def loop_cases():
    """Every (workload, how, d) the hinge-loop tests replay."""
    return sorted({(w, route(m, d, alignment_of(off)), d) for _, w, m, d, off, _ in LOOP_RUNS})


def walk_geometry(B, lpt):
    """complex_hinge_grad_launch + the ORD walk of complex_hinge_grad_plan_kernel: (waves of the grid, pairs of the
    relation order each wave walks)."""
    gpw = K_WAVE // lpt
    per_block = (K_BLOCK // K_WAVE) * gpw
    nwaves = min(K_MAX_BLOCKS, max(1, -(-B // per_block))) * (K_BLOCK // K_WAVE)
    return nwaves, -(-(-(-B // nwaves)) // gpw) * gpw


# ------------------------------------------------------------------------------------ the single-step batch
STEP_N, STEP_REL, STEP_B = 40, 8, 67          # 67: no multiple of the 4, 2 or 1 lane groups of a wave
STEP_SHARES = {"all": 3, "r_only": 5, "h_only": 7, "t_only": 11, "hr": 13, "tr": 17}      # pair index of each sharing


@functools.lru_cache(maxsize=None)
def step_batch():
    """(pos, neg) [67,3] on 40 rows (8 relations): negatives that replace the head or the tail, and by hand one that
    is its positive, one with head and tail both replaced, negatives that keep only the head / only the tail / head and
    relation / tail and relation, and one pair five times."""
    rng = np.random.default_rng(STEP_BATCH_SEED)
    B, E0 = STEP_B, STEP_REL
    pos = np.stack([rng.integers(E0, STEP_N, B), rng.integers(E0, STEP_N, B), rng.integers(0, E0, B)], 1).astype(np.int32)
    neg = pos.copy()
    side = rng.integers(0, 2, B)
    neg[np.arange(B), side] = (pos[np.arange(B), side] - E0 + rng.integers(1, STEP_N - E0, B)) % (STEP_N - E0) + E0
    other = lambda col, i: (pos[i, col] - E0 + 1 + i) % (STEP_N - E0) + E0
    other_rel = lambda i: (pos[i, 2] + 1 + i % (E0 - 1)) % E0
    s = STEP_SHARES
    neg[s["all"]] = pos[s["all"]]
    neg[s["r_only"]] = (other(0, s["r_only"]), other(1, s["r_only"]), pos[s["r_only"], 2])
    neg[s["h_only"]] = (pos[s["h_only"], 0], other(1, s["h_only"]), other_rel(s["h_only"]))
    neg[s["t_only"]] = (other(0, s["t_only"]), pos[s["t_only"], 1], other_rel(s["t_only"]))
    neg[s["hr"]] = (pos[s["hr"], 0], other(1, s["hr"]), pos[s["hr"], 2])
    neg[s["tr"]] = (other(0, s["tr"]), pos[s["tr"], 1], pos[s["tr"], 2])
    pos[21:25], neg[21:25] = pos[20], neg[20]
    return _frozen(pos), _frozen(neg)


def step_how(model):
    return "complex" if model == "complex" else "spectral"


@functools.lru_cache(maxsize=None)
def step_replay(how, d, fp32=False):
    pos, neg = step_batch()
    table = table_of(STEP_N, d, TABLE_SEEDS.get(("step", how, d), 0), how)
    return _replay(table, [(pos, neg, STEP_LR)], how, fp32)


def measure_step_gap(how, d):
    return gap_of(step_replay(how, d, True), step_replay(how, d))


def step_cases():
    return [("step", how, d) for how in ("complex", "spectral") for d in sorted(LOW + HIGH)]


# ------------------------------------------------------------------------------------ the log-loss loop
@functools.lru_cache(maxsize=None)
def logloss_replay(d, fp32=False):
    """logloss_cases.replay on `small`'s graph at B = 100, K = 2: (final table, [loss vector per step])."""
    import logloss_cases as LC
    w = WORKLOADS["logloss"]
    bats, _ = batches("logloss")
    return LC.replay(table_of(w.N, d, 0), [(p, n) for p, n, _, _ in bats], LOGLOSS_L2, F32 if fp32 else np.float64,
                     gs0=w.gs0, lr0=LR0, decay_steps=DECAY_STEPS, decay_rate=DECAY_RATE)


def measure_logloss_d32(d):
    return float(np.abs(logloss_replay(d, True)[0].astype(np.float64) - logloss_replay(d)[0]).max())


# ------------------------------------------------------------------------------------ bounds
SCORE_TOL, TABLE_TOL, HOT_TABLE_TOL = 1e-5, 5e-6, 2e-5       # tests/test_gpu_parity.py
HEADROOM = 4.0


def table_bar(case_key):
    """The project's bar on the table: every loop step has relation rows of more than 16 slots; the single-step batch
    (seeded so) has none."""
    return TABLE_TOL if case_key[0] == "step" else HOT_TABLE_TOL


def bounds(case_key):
    """(loss bound, table bound) of a (workload or "step", how, d): max(bar, 4 x the recorded gap)."""
    gl, gt = GAPS[case_key]
    return max(SCORE_TOL, HEADROOM * gl), max(table_bar(case_key), HEADROOM * gt)


# Table seeds other than 0: the first seed at which no pair of the case lies within 4 x its loss bound of the hinge's
# kink (test_complex_shape_cases_host.py::test_no_pair_near_the_kink)
STEP_BATCH_SEED = 0
TABLE_SEEDS = {('small', 'direct', 258): 1, ('small', 'spectral', 64): 1, ('two_tiles', 'complex', 8): 3,
               ('two_tiles', 'complex', 34): 3, ('two_tiles', 'complex', 66): 1, ('two_tiles', 'complex', 68): 2,
               ('two_tiles', 'complex', 100): 1, ('two_tiles', 'complex', 130): 2, ('two_tiles', 'complex', 132): 2,
               ('two_tiles', 'complex', 264): 1, ('two_tiles', 'spectral', 130): 1, ('two_tiles', 'spectral', 260):
               1}

# (loss gap, table gap): the fp32 implementation against the fp64 oracle, measured on the host (recorded rounded up)
GAPS = {
    ('small', 'complex', 2): (1.1e-07, 2.9e-07),   # measured 1.01e-07, 2.88e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 4): (1.0e-07, 3.5e-07),   # measured 9.99e-08, 3.43e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 8): (1.1e-07, 6.2e-07),   # measured 1.09e-07, 6.15e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 30): (1.1e-07, 6.0e-07),   # measured 1.08e-07, 5.91e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 34): (9.7e-08, 6.1e-07),   # measured 9.67e-08, 6.09e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 60): (1.2e-07, 3.4e-07),   # measured 1.14e-07, 3.30e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 62): (1.1e-07, 3.0e-07),   # measured 1.01e-07, 2.90e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 64): (1.3e-07, 6.3e-07),   # measured 1.23e-07, 6.29e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 66): (1.2e-07, 9.3e-07),   # measured 1.12e-07, 9.27e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 68): (1.2e-07, 4.3e-07),   # measured 1.18e-07, 4.29e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 100): (1.3e-07, 6.8e-07),   # measured 1.26e-07, 6.78e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 124): (1.4e-07, 9.7e-07),   # measured 1.37e-07, 9.69e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 126): (1.3e-07, 4.2e-07),   # measured 1.21e-07, 4.16e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 128): (1.1e-07, 3.2e-07),   # measured 1.04e-07, 3.16e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 130): (1.1e-07, 3.2e-07),   # measured 1.07e-07, 3.16e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 132): (1.3e-07, 2.4e-07),   # measured 1.27e-07, 2.36e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 136): (1.2e-07, 2.9e-07),   # measured 1.18e-07, 2.84e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 200): (1.5e-07, 5.2e-07),   # measured 1.44e-07, 5.19e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 252): (1.9e-07, 6.8e-07),   # measured 1.82e-07, 6.74e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 254): (1.1e-07, 2.6e-07),   # measured 1.07e-07, 2.56e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 256): (1.2e-07, 2.4e-07),   # measured 1.14e-07, 2.38e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 260): (1.3e-07, 2.8e-07),   # measured 1.22e-07, 2.73e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 264): (1.2e-07, 2.9e-07),   # measured 1.11e-07, 2.85e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 508): (1.2e-07, 3.7e-07),   # measured 1.13e-07, 3.61e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 512): (1.3e-07, 4.0e-07),   # measured 1.28e-07, 3.95e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 520): (1.3e-07, 5.2e-07),   # measured 1.22e-07, 5.20e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'complex', 1024): (1.2e-07, 6.5e-07),   # measured 1.14e-07, 6.41e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'direct', 258): (1.5e-07, 2.1e-07),   # measured 1.46e-07, 2.02e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'direct', 512): (2.4e-07, 1.8e-07),   # measured 2.39e-07, 1.73e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'spectral', 2): (1.8e-07, 9.7e-07),   # measured 1.76e-07, 9.61e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'spectral', 4): (1.5e-07, 5.1e-07),   # measured 1.43e-07, 5.00e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'spectral', 8): (1.2e-07, 4.9e-07),   # measured 1.20e-07, 4.88e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'spectral', 34): (1.4e-07, 3.2e-07),   # measured 1.37e-07, 3.19e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'spectral', 64): (1.1e-07, 3.9e-07),   # measured 1.04e-07, 3.87e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'spectral', 66): (1.2e-07, 5.5e-07),   # measured 1.16e-07, 5.42e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'spectral', 68): (1.0e-07, 3.1e-07),   # measured 9.97e-08, 3.01e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'spectral', 100): (9.4e-08, 2.9e-07),   # measured 9.37e-08, 2.87e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'spectral', 130): (8.9e-08, 1.6e-07),   # measured 8.83e-08, 1.58e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'spectral', 132): (1.1e-07, 3.6e-07),   # measured 1.02e-07, 3.52e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'spectral', 136): (9.6e-08, 2.3e-07),   # measured 9.56e-08, 2.28e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'spectral', 200): (8.8e-08, 2.8e-07),   # measured 8.80e-08, 2.74e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'spectral', 256): (1.2e-07, 1.7e-07),   # measured 1.17e-07, 1.60e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'spectral', 260): (9.8e-08, 2.3e-07),   # measured 9.80e-08, 2.23e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'spectral', 264): (1.1e-07, 1.8e-07),   # measured 1.03e-07, 1.78e-07: bounds 1.0e-05, 2.0e-05
    ('small', 'spectral', 520): (1.2e-07, 1.5e-07),   # measured 1.12e-07, 1.46e-07: bounds 1.0e-05, 2.0e-05
    ('step', 'complex', 2): (5.6e-08, 2.2e-07),   # measured 5.50e-08, 2.13e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 4): (6.7e-08, 4.8e-07),   # measured 6.62e-08, 4.71e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 8): (9.0e-08, 2.4e-07),   # measured 8.92e-08, 2.31e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 30): (6.8e-08, 2.5e-07),   # measured 6.76e-08, 2.46e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 34): (7.6e-08, 2.2e-07),   # measured 7.56e-08, 2.17e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 60): (7.0e-08, 3.1e-07),   # measured 6.95e-08, 3.02e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 62): (6.8e-08, 1.5e-07),   # measured 6.78e-08, 1.50e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 66): (6.6e-08, 2.2e-07),   # measured 6.50e-08, 2.15e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 68): (8.4e-08, 1.4e-07),   # measured 8.31e-08, 1.33e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 124): (6.3e-08, 1.7e-07),   # measured 6.27e-08, 1.63e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 126): (6.0e-08, 4.8e-07),   # measured 5.94e-08, 4.75e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 128): (7.0e-08, 1.8e-07),   # measured 6.94e-08, 1.76e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 130): (6.6e-08, 1.8e-07),   # measured 6.55e-08, 1.75e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 132): (8.3e-08, 3.1e-07),   # measured 8.23e-08, 3.00e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 136): (8.2e-08, 1.9e-07),   # measured 8.15e-08, 1.85e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 252): (7.7e-08, 1.4e-07),   # measured 7.65e-08, 1.31e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 254): (8.7e-08, 3.9e-07),   # measured 8.69e-08, 3.83e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 256): (6.7e-08, 2.0e-07),   # measured 6.69e-08, 1.98e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 260): (8.2e-08, 3.0e-07),   # measured 8.18e-08, 3.00e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 264): (8.4e-08, 3.4e-07),   # measured 8.37e-08, 3.37e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 508): (7.8e-08, 2.3e-07),   # measured 7.78e-08, 2.25e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 512): (1.1e-07, 1.6e-07),   # measured 1.08e-07, 1.59e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 520): (8.0e-08, 3.1e-07),   # measured 7.97e-08, 3.07e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'complex', 1024): (9.8e-08, 1.5e-07),   # measured 9.75e-08, 1.42e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 2): (7.2e-08, 1.9e-07),   # measured 7.16e-08, 1.83e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 4): (6.7e-08, 2.7e-07),   # measured 6.64e-08, 2.65e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 8): (9.7e-08, 1.8e-07),   # measured 9.62e-08, 1.78e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 30): (7.7e-08, 1.4e-07),   # measured 7.66e-08, 1.32e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 34): (7.5e-08, 1.9e-07),   # measured 7.46e-08, 1.85e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 60): (7.5e-08, 1.9e-07),   # measured 7.48e-08, 1.88e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 62): (1.0e-07, 1.2e-07),   # measured 9.91e-08, 1.14e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 66): (8.5e-08, 1.2e-07),   # measured 8.45e-08, 1.18e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 68): (7.0e-08, 1.2e-07),   # measured 6.91e-08, 1.20e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 124): (7.9e-08, 6.4e-08),   # measured 7.82e-08, 6.37e-08: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 126): (9.6e-08, 1.4e-07),   # measured 9.50e-08, 1.36e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 128): (7.1e-08, 8.1e-08),   # measured 7.01e-08, 8.00e-08: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 130): (9.6e-08, 6.5e-08),   # measured 9.52e-08, 6.49e-08: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 132): (9.6e-08, 1.8e-07),   # measured 9.50e-08, 1.72e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 136): (7.2e-08, 6.6e-08),   # measured 7.13e-08, 6.51e-08: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 252): (7.5e-08, 1.2e-07),   # measured 7.50e-08, 1.19e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 254): (8.6e-08, 1.2e-07),   # measured 8.53e-08, 1.10e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 256): (8.3e-08, 1.2e-07),   # measured 8.22e-08, 1.18e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 260): (6.5e-08, 8.0e-08),   # measured 6.45e-08, 7.95e-08: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 264): (8.0e-08, 8.6e-08),   # measured 7.93e-08, 8.53e-08: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 508): (9.3e-08, 7.6e-08),   # measured 9.24e-08, 7.56e-08: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 512): (8.2e-08, 6.3e-08),   # measured 8.15e-08, 6.24e-08: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 520): (8.1e-08, 1.1e-07),   # measured 8.02e-08, 1.01e-07: bounds 1.0e-05, 5.0e-06
    ('step', 'spectral', 1024): (5.9e-08, 6.1e-08),   # measured 5.80e-08, 6.08e-08: bounds 1.0e-05, 5.0e-06
    ('two_tiles', 'complex', 2): (7.7e-07, 4.2e-06),   # measured 7.69e-07, 4.19e-06: bounds 1.0e-05, 2.0e-05
    ('two_tiles', 'complex', 4): (1.8e-07, 5.1e-07),   # measured 1.71e-07, 5.05e-07: bounds 1.0e-05, 2.0e-05
    ('two_tiles', 'complex', 8): (1.8e-07, 1.8e-06),   # measured 1.79e-07, 1.76e-06: bounds 1.0e-05, 2.0e-05
    ('two_tiles', 'complex', 34): (2.3e-07, 3.0e-06),   # measured 2.30e-07, 2.91e-06: bounds 1.0e-05, 2.0e-05
    ('two_tiles', 'complex', 64): (2.3e-07, 1.8e-06),   # measured 2.27e-07, 1.78e-06: bounds 1.0e-05, 2.0e-05
    ('two_tiles', 'complex', 66): (2.1e-07, 9.0e-07),   # measured 2.02e-07, 8.94e-07: bounds 1.0e-05, 2.0e-05
    ('two_tiles', 'complex', 68): (2.4e-07, 1.2e-06),   # measured 2.34e-07, 1.15e-06: bounds 1.0e-05, 2.0e-05
    ('two_tiles', 'complex', 100): (2.0e-07, 1.7e-06),   # measured 1.98e-07, 1.70e-06: bounds 1.0e-05, 2.0e-05
    ('two_tiles', 'complex', 130): (2.5e-07, 1.2e-06),   # measured 2.43e-07, 1.12e-06: bounds 1.0e-05, 2.0e-05
    ('two_tiles', 'complex', 132): (2.5e-07, 9.8e-07),   # measured 2.44e-07, 9.79e-07: bounds 1.0e-05, 2.0e-05
    ('two_tiles', 'complex', 136): (2.9e-07, 3.3e-06),   # measured 2.88e-07, 3.27e-06: bounds 1.0e-05, 2.0e-05
    ('two_tiles', 'complex', 200): (1.9e-07, 1.9e-06),   # measured 1.87e-07, 1.90e-06: bounds 1.0e-05, 2.0e-05
    ('two_tiles', 'complex', 256): (2.9e-07, 1.1e-06),   # measured 2.88e-07, 1.02e-06: bounds 1.0e-05, 2.0e-05
    ('two_tiles', 'complex', 260): (2.1e-07, 1.5e-06),   # measured 2.05e-07, 1.43e-06: bounds 1.0e-05, 2.0e-05
    ('two_tiles', 'complex', 264): (2.6e-07, 1.2e-06),   # measured 2.52e-07, 1.12e-06: bounds 1.0e-05, 2.0e-05
    ('two_tiles', 'complex', 520): (2.3e-07, 1.4e-06),   # measured 2.30e-07, 1.34e-06: bounds 1.0e-05, 2.0e-05
    ('two_tiles', 'spectral', 130): (1.7e-07, 9.4e-07),   # measured 1.70e-07, 9.35e-07: bounds 1.0e-05, 2.0e-05
    ('two_tiles', 'spectral', 260): (2.2e-07, 1.1e-06),   # measured 2.18e-07, 1.08e-06: bounds 1.0e-05, 2.0e-05
    ('two_tiles', 'spectral', 520): (2.2e-07, 6.5e-07),   # measured 2.16e-07, 6.45e-07: bounds 1.0e-05, 2.0e-05
    ('untyped', 'complex', 130): (9.8e-08, 3.7e-07),   # measured 9.78e-08, 3.62e-07: bounds 1.0e-05, 2.0e-05
    ('untyped', 'complex', 200): (1.1e-07, 4.9e-07),   # measured 1.03e-07, 4.88e-07: bounds 1.0e-05, 2.0e-05
}

# the log-loss cases: d -> D32 of logloss_cases.table_tol
LOGLOSS_D32 = {
    2: 4.2e-07,   # measured 4.11e-07: bound 2.0e-05
    34: 6.5e-07,   # measured 6.46e-07: bound 2.0e-05
    66: 6.5e-07,   # measured 6.43e-07: bound 2.0e-05
    130: 2.4e-07,   # measured 2.39e-07: bound 2.0e-05
    4: 5.1e-07,   # measured 5.08e-07: bound 2.0e-05
    68: 2.4e-07,   # measured 2.31e-07: bound 2.0e-05
    132: 7.4e-07,   # measured 7.30e-07: bound 2.0e-05
    260: 8.0e-07,   # measured 7.97e-07: bound 2.0e-05
    8: 3.9e-07,   # measured 3.87e-07: bound 2.0e-05
    136: 3.4e-07,   # measured 3.32e-07: bound 2.0e-05
    264: 2.0e-07,   # measured 1.94e-07: bound 2.0e-05
    520: 1.6e-06,   # measured 1.53e-06: bound 2.0e-05
}
