"""GPU: the multi-label (K-vs-all) softmax objective of ComplEx (ge_softmax_labels_loss / ge_softmax_labels_grad,
hole.QueryLabels / LabelSoftmaxAdaGrad / SoftmaxTrainer(labels="all")) against tests/softmax_labels_ref.py.

Shapes are the tile neighbours of tests/test_gpu_softmax.py (64 x 64 tiles; K = 577 is five ranges of two tiles, the last
ending inside a tile), tables and queries its build().  Two label layouts a case:
    "one"    every row one label (the true column of build(): 0, K - 1 and both sides of every 64 boundary among them);
    "mixed"  n_i = 1 ... min(K, 9) by row; the positions 0, K - 1 and both sides of every 64 boundary each a label of some
             row; row 1 names its first position twice; the middle row (the only row at B = 1, none at B = 2) labels ALL K
             positions, in a shuffled order -- there p - y / n nearly cancels in the candidates' summed gradient.

Bounds.  Per case e32 = the largest absolute deviation of softmax_labels_ref's float32 evaluation from its fp64 evaluation,
separately for the loss and for the gradient rows; the GPU must be within 8 * e32 + 1e-7 of the fp64 oracle (the rule of
DESIGN.md section 22).  Every case prints its four figures (`-s`); DESIGN.md section 25 has the measured ranges."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_softmax as G
from graphembeddings_amd import hole as H
from tests import softmax_labels_ref as LR

pytestmark = pytest.mark.gpu

I32, F32 = np.int32, np.float32
A0 = G.A0
dev, bits = G.dev, G.bits


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")


@functools.lru_cache(maxsize=None)
def labels(B, K, layout, seed=0):
    """(label_off [B + 1], label_pos [L]) int32 of the mixed layout for the queries of G.build(B, K, ...)."""
    assert layout == "mixed"                              # "one" is build()'s true column: see case()
    rng = np.random.default_rng(77 * B + K + seed)
    rows = [list(rng.permutation(K)[:1 + i % min(K, 9)]) for i in range(B)]
    if B != 2:
        rows[B // 2] = list(rng.permutation(K))
    special = sorted({0, K - 1} | {c for b in range(64, K, 64) for c in (b - 1, b)})
    for n, c in enumerate(special):
        r = rows[(3 * n) % B]
        if c not in r:
            r.insert(int(rng.integers(0, len(r) + 1)), c)
    dup = rows[1] if B > 1 else rows[0]
    dup.append(dup[0])
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(I32)
    return off, np.concatenate(rows).astype(I32)


@functools.lru_cache(maxsize=None)
def case(B, K, d, max_norm, head, layout, seed=0):
    """(table, hr, label_off, label_pos, cand)"""
    t, hr, true, cand = G.build(B, K, d, max_norm, head, seed)
    if layout == "one":
        where = {int(c): j for j, c in enumerate(cand)}
        return t, hr, np.arange(B + 1, dtype=I32), np.array([where[int(x)] for x in true], I32), cand
    off, pos = labels(B, K, layout, seed)
    return t, hr, off, pos, cand


@functools.lru_cache(maxsize=None)
def reference(B, K, d, max_norm, scale, head, layout, seed=0):
    """(fp64 loss, idx, val at lr = 1; e32 of the loss; e32 of the gradient rows)."""
    t, hr, off, pos, cand = case(B, K, d, max_norm, head, layout, seed)
    l64, idx, v64 = LR.evaluate(t, hr, off, pos, cand, max_norm, scale, head)
    l32, i32_, v32 = LR.evaluate(t, hr, off, pos, cand, max_norm, scale, head, dtype=np.float32)
    assert np.array_equal(idx, i32_)
    return l64, idx, v64, float(np.nanmax(np.abs(l32 - l64))), float(np.abs(v32 - v64).max())


def gpu_grad(t, hr, off, pos, cand, max_norm, scale, head, lr=1.0):
    loss, gi, gv = H.softmax_labels_grad(dev(t), dev(hr), dev(off), dev(pos), dev(cand), lr, scale=scale, max_norm=max_norm,
                                         side="head" if head else "tail")
    torch.cuda.synchronize()
    return loss.cpu().numpy(), gi.cpu().numpy(), gv.cpu().numpy()


def check_case(B, K, d, max_norm, scale, head, layout):
    c = case(B, K, d, max_norm, head, layout)
    l64, idx, v64, e_l, e_g = reference(B, K, d, max_norm, scale, head, layout)
    loss, gi, gv = gpu_grad(*c, max_norm, scale, head)
    assert np.isfinite(l64).all() and np.array_equal(gi, idx) and (idx >= 0).all()
    dl, dg = float(np.abs(loss - l64).max()), float(np.abs(gv - v64).max())
    print("SOFTMAX-LABELS B=%d K=%d d=%d max_norm=%g scale=%g side=%s %s L=%d: loss e32 %.3g gpu %.3g | grad e32 %.3g gpu %.3g"
          % (B, K, d, max_norm, scale, "head" if head else "tail", layout, len(c[3]), e_l, dl, e_g, dg))
    assert np.isfinite(loss).all() and np.isfinite(gv).all()
    assert dl <= 8 * e_l + 1e-7, ("loss", dl, e_l)
    assert dg <= 8 * e_g + 1e-7, ("grad", dg, e_g)


LAYOUTS = ["one", "mixed"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("max_norm,scale", G.NORMS_SCALES)
@pytest.mark.parametrize("K", [1, 2, 64, 65, 300, 577])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_shapes(B, K, max_norm, scale, head, layout):
    check_case(B, K, 64, max_norm, scale, head, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("max_norm,scale", G.NORMS_SCALES)
@pytest.mark.parametrize("d", [8, 56, 200, 288])
def test_widths(d, max_norm, scale, head, layout):
    check_case(130, 300, d, max_norm, scale, head, layout)


def test_layouts_hold_what_they_claim():
    off, pos = labels(130, 300, "mixed")
    n = np.diff(off)
    assert set(range(1, 10)) <= set(n.tolist()) and n.max() == 300 and sorted(pos[off[65]:off[66]].tolist()) == list(range(300))
    assert {0, 63, 64, 127, 128, 191, 192, 255, 256, 299} <= set(np.delete(pos, np.arange(off[65], off[66])).tolist())
    assert pos[off[2] - 1] == pos[off[1]] and len(set(pos[off[1]:off[2]].tolist())) == n[1] - 1
    off1, pos1 = labels(1, 65, "mixed")
    assert off1.tolist() == [0, 66] and sorted(pos1[:65].tolist()) == list(range(65)) and pos1[65] == pos1[0]


@pytest.mark.parametrize("head", [False, True])
def test_invalid_rows_and_a_bad_candidate(head):
    """Invalid rows of each kind (a fixed or relation id outside [0, N); no labels; a label position outside [0, K); a label
    on a candidate outside the table; an offset past L; a decreasing offset) and one candidate id outside [0, N): NaN / -1 /
    zero rows, and every valid row's loss and slots and every candidate row are bit for bit what they are without them
    (they are appended: the valid rows and candidates keep their tiles)."""
    B, K, d, mn, scale = 65, 129, 64, 1.0, 20.0
    t, hr, off, pos, cand = case(B, K, d, mn, head, "mixed")
    N, L = t.shape[0], len(pos)
    base = gpu_grad(t, hr, off, pos, cand, mn, scale, head)
    c1 = int(cand[1])
    hr2 = np.concatenate([hr, [[N, 0], [c1, -1], [c1, N + 9], [-5, 1], [c1, 1], [c1, 1], [c1, 1], [c1, 1], [c1, 1], [c1, 1]]]).astype(I32)
    # the appended rows' entries: four good ones for the rows with bad ids, none, -1, K + 1, the bad candidate's position K,
    # then a row that ends past the array and one whose offsets decrease
    pos2 = np.concatenate([pos, [0, 1, 2, 3], [-1], [K + 1], [K], [4, 5]]).astype(I32)
    off2 = np.concatenate([off, [L + 1, L + 2, L + 3, L + 4, L + 4, L + 5, L + 6, L + 7, L + 12, L + 8]]).astype(I32)
    cand2 = np.concatenate([cand, [N + 3]]).astype(I32)
    B2, L2 = len(hr2), len(pos2)
    assert off2[-1] < L2 < off2[-2]
    loss, gi, gv = gpu_grad(t, hr2, off2, pos2, cand2, mn, scale, head)
    l64, idx, v64 = LR.evaluate(t, hr2, off2, pos2, cand2, mn, scale, head)
    assert np.isnan(loss[B:]).all() and np.isnan(l64[B:]).all() and np.array_equal(gi, idx)
    K2 = K + 1
    assert gi[K] == -1 and not gv[K].any()
    assert (gi[K2 + 2 * B:K2 + 2 * B2] == -1).all() and not gv[K2 + 2 * B:K2 + 2 * B2].any()
    assert (gi[K2 + 2 * B2 + L:] == -1).all() and not gv[K2 + 2 * B2 + L:].any()
    assert np.array_equal(bits(loss[:B]), bits(base[0]))
    assert np.array_equal(gi[:K], base[1][:K]) and np.array_equal(bits(gv[:K]), bits(base[2][:K]))
    assert np.array_equal(gi[K2:K2 + 2 * B], base[1][K:K + 2 * B])
    assert np.array_equal(bits(gv[K2:K2 + 2 * B]), bits(base[2][K:K + 2 * B]))
    assert np.array_equal(gi[K2 + 2 * B2:K2 + 2 * B2 + L], base[1][K + 2 * B:])
    assert np.array_equal(bits(gv[K2 + 2 * B2:K2 + 2 * B2 + L]), bits(base[2][K + 2 * B:]))
    _, _, _, e_l, e_g = reference(B, K, d, mn, scale, head, "mixed")
    assert np.abs(loss[:B] - l64[:B]).max() <= 8 * e_l + 1e-7 and np.abs(gv - v64).max() <= 8 * e_g + 1e-7
    # no labels at all: every row is invalid, every slot empty but the candidates', whose rows are zero
    lo, gi0, gv0 = gpu_grad(t, hr, np.zeros(B + 1, I32), np.zeros(0, I32), cand, mn, scale, head)
    assert np.isnan(lo).all() and np.array_equal(gi0[:K], cand) and (gi0[K:] == -1).all() and not gv0.any()


@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("B,K,d", [(130, 300, 64), (65, 577, 200), (1, 1, 8)])
def test_exact_properties(B, K, d, head):
    mn, scale = 1.0, 20.0
    t, hr, off, pos, cand = case(B, K, d, mn, head, "mixed")
    a, b = gpu_grad(t, hr, off, pos, cand, mn, scale, head), gpu_grad(t, hr, off, pos, cand, mn, scale, head)
    for x, y in zip(a, b):                             # two identical calls
        assert np.array_equal(bits(x), bits(y))
    lo = H.softmax_labels_loss(dev(t), dev(hr), dev(off), dev(pos), dev(cand), scale=scale, max_norm=mn,
                               side="head" if head else "tail")
    assert np.array_equal(bits(lo), bits(a[0]))
    half = gpu_grad(t, hr, off, pos, cand, mn, scale, head, lr=0.5)
    assert np.array_equal(half[1], a[1]) and np.array_equal(bits(half[2]), bits((F32(0.5) * a[2]).astype(F32)))
    # the rows permuted together with their label lists: the losses and the query slots permuted, the label slots moved
    perm = np.random.default_rng(B).permutation(B)
    lists = [pos[off[i]:off[i + 1]] for i in perm]
    poff = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(I32)
    p = gpu_grad(t, hr[perm], poff, np.concatenate(lists).astype(I32), cand, mn, scale, head)
    assert np.array_equal(bits(p[0]), bits(a[0][perm]))
    q = lambda g: g[K:K + 2 * B].reshape(B, 2, -1)
    assert np.array_equal(q(p[1])[:, :, 0], q(a[1])[perm][:, :, 0]) and np.array_equal(bits(q(p[2])), bits(q(a[2])[perm]))
    src = np.concatenate([np.arange(off[i], off[i + 1]) for i in perm]) + K + 2 * B
    assert np.array_equal(p[1][K + 2 * B:], a[1][src]) and np.array_equal(bits(p[2][K + 2 * B:]), bits(a[2][src]))


@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("B,K,d,mn,scale", [(130, 300, 64, 1.0, 20.0), (65, 577, 200, 4.0, 200.0), (1, 2, 8, 1.0, 1.0)])
def test_one_label_is_the_one_vs_all_call(B, K, d, mn, scale, head):
    """One label a row: the loss and the gradient summed per table row are within the bound of ge_softmax_grad's (not
    bitwise: the label term is a slice of its own and reaches the query's gradient as one more partial)."""
    t, hr, true, cand = G.build(B, K, d, mn, head)
    _, _, off, pos, _ = case(B, K, d, mn, head, "one")
    _, _, _, e_l, e_g = reference(B, K, d, mn, scale, head, "one")
    loss, gi, gv = gpu_grad(t, hr, off, pos, cand, mn, scale, head)
    l1, i1, v1 = G.gpu_grad(t, hr, true, cand, mn, scale, head)
    assert np.array_equal(gi[:K + 2 * B], i1) and np.array_equal(gi[K + 2 * B:], true)
    sums = lambda i, v: np.stack([np.bincount(i, v[:, c].astype(np.float64), t.shape[0]) for c in range(d)], 1)
    dl, dg = float(np.abs(loss - l1).max()), float(np.abs(sums(gi, gv) - sums(i1, v1)).max())
    print("SOFTMAX-LABELS one label vs 1-vs-all B=%d K=%d d=%d: loss %.3g (bound %.3g) grad %.3g (bound %.3g)"
          % (B, K, d, dl, 8 * e_l + 1e-7, dg, 8 * e_g + 1e-7))
    assert dl <= 8 * e_l + 1e-7 and dg <= 8 * e_g + 1e-7


def test_host_checks():
    t, hr, off, pos, cand = case(63, 64, 64, 1.0, False, "mixed")
    T, h, o, p, c = dev(t), dev(hr), dev(off), dev(pos), dev(cand)
    for kw in (dict(scale=0.0), dict(scale=float("inf")), dict(scale=20.0, max_norm=0.0), dict(scale=20.0, side="both")):
        with pytest.raises(ValueError):
            H.softmax_labels_loss(T, h, o, p, c, **kw)
    with pytest.raises(ValueError):
        H.softmax_labels_loss(T, h[:, :1], o, p, c, scale=20.0)
    with pytest.raises(ValueError):
        H.softmax_labels_loss(T, h, o[:-1], p, c, scale=20.0)
    with pytest.raises(ValueError):
        H.softmax_labels_loss(T[:, :60].contiguous(), h, o, p, c, scale=20.0)
    with pytest.raises(ValueError):
        H.softmax_labels_grad(T, h, o, p, c, 1.0, scale=20.0, out=(torch.empty(5, dtype=torch.int32, device="cuda"),
                                                                   torch.empty(5, 64, device="cuda")))


# ------------------------------------------------------------------------------------------------ QueryLabels
def test_query_labels():
    train, _, _ = G.planted()
    cand = np.arange(G.N_REL_KG, G.N_REL_KG + G.N_ENT_KG, dtype=I32)[::-1].copy()       # positions are not ids
    where = {int(c): j for j, c in enumerate(cand)}
    for side, (fx, an) in (("tail", (0, 1)), ("head", (1, 0))):
        ql = H.QueryLabels.from_triples(dev(train), dev(cand), side)
        want = {}
        for row in np.concatenate([train, train[:50]]):                                # repeated triples count once
            want.setdefault((int(row[fx]), int(row[2])), set()).add(where[int(row[an])])
        keys = sorted(want)
        assert len(ql) == len(keys) and np.array_equal(ql.queries.cpu().numpy(), np.array(keys, I32))
        off, pos = ql.label_off.cpu().numpy(), ql.label_pos.cpu().numpy()
        assert off[0] == 0 and off[-1] == len(pos) == sum(len(v) for v in want.values())
        assert all(pos[off[i]:off[i + 1]].tolist() == sorted(want[k]) for i, k in enumerate(keys))
        rows = np.random.default_rng(1).permutation(len(keys))[:97]
        hr, o, p = ql.take(dev(rows))
        assert hr.dtype == o.dtype == p.dtype == torch.int32 and np.array_equal(hr.cpu().numpy(), np.array(keys, I32)[rows])
        o, p = o.cpu().numpy(), p.cpu().numpy()
        assert all(p[o[n]:o[n + 1]].tolist() == sorted(want[keys[r]]) for n, r in enumerate(rows)) and o[-1] == len(p)
    assert len(ql) < len(train)
    with pytest.raises(ValueError):
        H.QueryLabels.from_triples(dev(train), dev(cand[1:]), "tail")                  # an answer that is no candidate
    with pytest.raises(ValueError):
        H.QueryLabels.from_triples(dev(train), dev(cand), "both")


# ------------------------------------------------------------------------------------------------ the step
def step_case():
    """(table, tail batch, head batch, cand) at (130, 300, 64): the queries of build(130, 300, 64) -- all of relation 1, rows
    0..2 with candidate 0 as their fixed entity -- with the mixed labels on the tail side; the first 65 of them with other
    labels as (tail, relation) queries on the head side."""
    t, hr, off, pos, cand = case(130, 300, 64, 1.0, False, "mixed")
    off2, pos2 = labels(65, 300, "mixed", seed=5)
    return t, (hr, off, pos), (hr[:65].copy(), off2, pos2), cand


def test_step():
    t, tail, head, cand = step_case()
    N, d = t.shape
    lr, scale = 0.1, 20.0
    ref_t, ref_a = t.astype(np.float64), np.full((N, d), A0, np.float64)
    ref_loss, s, named = LR.step(ref_t, ref_a, tail, head, cand, 1.0, scale, lr)
    e, slots = [], []
    for batch, hd in ((tail, False), (head, True)):
        g64 = LR.evaluate(t, *batch, cand, 1.0, scale, hd)
        g32 = LR.evaluate(t, *batch, cand, 1.0, scale, hd, dtype=np.float32)
        e.append((np.abs(g32[0] - g64[0]).max(), np.abs(g32[2] - g64[2]).max()))
        slots.append(g64[1])
    gb = 8 * max(x[1] for x in e) + 1e-7
    counts = np.bincount(np.concatenate(slots), minlength=N)
    assert counts[cand[0]] >= 5 and counts[tail[0][0, 1]] > 16 and not named.all()
    emb = dev(t)
    L = max(len(tail[2]), len(head[2]))
    opt = H.LabelSoftmaxAdaGrad(emb, dev(cand), 130, L, scale=scale, initial_accumulator_value=A0)
    assert float(opt.accumulator.min()) == float(opt.accumulator.max()) == F32(A0)
    to_dev = lambda b: tuple(dev(x) for x in b)
    lt, lh = opt.step(to_dev(tail), to_dev(head), lr)
    torch.cuda.synchronize()
    assert lt.shape == (130,) and lh.shape == (65,)
    loss = np.concatenate([lt.cpu().numpy(), lh.cpu().numpy()])
    assert np.abs(loss - ref_loss).max() <= 8 * max(x[0] for x in e) + 1e-7
    got_t, got_a = emb.cpu().numpy(), opt.accumulator.cpu().numpy()
    G.check_step(got_t, got_a, ref_t, ref_a, s, counts, lr, gb)
    # rows that are neither candidates nor named by the batch: bit-identical in both arrays
    assert np.array_equal(bits(got_t[~named]), bits(t[~named])) and (got_a[~named] == F32(A0)).all()
    assert (got_a[named] > F32(A0)).any()
    # one side alone; more rows or labels than reserved
    only = opt.step(to_dev(tail), None, lr)
    assert only[1] is None and only[0].shape == (130,)
    with pytest.raises(ValueError):
        opt.step(None, None, lr)
    small = H.LabelSoftmaxAdaGrad(dev(t), dev(cand), 64, L, scale=scale)
    with pytest.raises(ValueError):
        small.step(to_dev(tail), None, lr)


def test_step_is_reproducible():
    t, tail, head, cand = step_case()
    to_dev = lambda b: tuple(dev(x) for x in b)
    runs = []
    for _ in range(2):
        emb = dev(t)
        opt = H.LabelSoftmaxAdaGrad(emb, dev(cand), 130, len(tail[2]), scale=20.0, initial_accumulator_value=A0)
        for k in range(5):
            opt.step(to_dev(tail) if k != 3 else None, to_dev(head) if k != 1 else None, 0.1)
        torch.cuda.synchronize()
        runs.append((emb.cpu().numpy(), opt.accumulator.cpu().numpy()))
    assert np.array_equal(bits(runs[0][0]), bits(runs[1][0])) and np.array_equal(bits(runs[0][1]), bits(runs[1][1]))
    assert not np.array_equal(bits(runs[0][0]), bits(t))


# ------------------------------------------------------------------------------------------------ learning
def test_learning():
    """300 steps of SoftmaxTrainer(labels="all") on the planted workload of tests/test_gpu_softmax.py reach the MRR of the
    same batches run through softmax_labels_ref in fp64 (>= 0.40; within 0.03).  The 1-vs-all trainer's figure from the same
    start is printed beside them."""
    train, test, all_tri = G.planted()
    N = G.N_REL_KG + G.N_ENT_KG
    cand = np.arange(G.N_REL_KG, N, dtype=I32)
    t0 = (np.random.default_rng(0).standard_normal((N, G.D_KG)) * np.sqrt(2.6 / (N + G.D_KG))).astype(F32)
    kw = dict(scale=G.SCALE_KG, learning_rate=G.LR_KG, seed=3, initial_accumulator_value=A0)
    emb = dev(t0)
    tr = H.SoftmaxTrainer(emb, dev(train), dev(cand), G.B_KG, labels="all", **kw)
    twin = H.SoftmaxTrainer(dev(t0), dev(train), dev(cand), G.B_KG, labels="all", **kw)
    q_tail, q_head = len(tr.queries["tail"]), len(tr.queries["head"])
    assert q_tail < len(train) and q_head < len(train) and tr.Q == q_tail + q_head
    host = lambda b: None if b is None else tuple(x.cpu().numpy() for x in b)
    batches = [tuple(host(b) for b in twin.next_queries()) for _ in range(G.STEPS_KG)]
    assert all(sum(len(b[0]) for b in pair if b is not None) == G.B_KG for pair in batches)
    epoch = np.concatenate([np.concatenate([b[0], np.full((len(b[0]), 1), s)], 1) for pair in batches[:tr.Q // G.B_KG]
                            for s, b in enumerate(pair) if b is not None])
    assert len(np.unique(epoch, axis=0)) == tr.Q // G.B_KG * G.B_KG                     # no query twice in an epoch
    loss = tr.run(G.STEPS_KG, keep_losses=True)
    torch.cuda.synchronize()
    assert loss.shape == (G.STEPS_KG, G.B_KG) and tr.global_step == G.STEPS_KG and torch.isfinite(loss).all()
    ref_t, ref_a = t0.astype(np.float64), np.full((N, G.D_KG), A0, np.float64)
    for tail, head in batches:
        LR.step(ref_t, ref_a, tail, head, cand, 1.0, G.SCALE_KG, G.LR_KG)
    ref_mrr, gpu_mrr = G.mrr_host(ref_t, test, all_tri, cand), G.mrr_gpu(emb, test, all_tri, cand)
    one = dev(t0)
    H.SoftmaxTrainer(one, dev(train), dev(cand), G.B_KG, **kw).run(G.STEPS_KG)
    torch.cuda.synchronize()
    print("SOFTMAX-LABELS learning: %d + %d queries of %d triples; reference MRR %.4f, GPU MRR %.4f, 1-vs-all GPU MRR %.4f"
          % (q_tail, q_head, len(train), ref_mrr, gpu_mrr, G.mrr_gpu(one, test, all_tri, cand)))
    assert ref_mrr >= 0.40
    assert abs(gpu_mrr - ref_mrr) <= 0.03


def test_trainer_refusals_and_default():
    train, _, _ = G.planted()
    cand = np.arange(G.N_REL_KG, G.N_REL_KG + G.N_ENT_KG, dtype=I32)
    t0 = (np.random.default_rng(0).standard_normal((G.N_REL_KG + G.N_ENT_KG, 8)) * 0.1).astype(F32)
    mk = lambda **kw: H.SoftmaxTrainer(dev(t0), dev(train), dev(cand), 64, scale=20.0, **kw)
    for kw in (dict(labels="all", n_samples=16), dict(labels="all", candidate_sets={}), dict(labels="some")):
        with pytest.raises(ValueError):
            mk(**kw)
    with pytest.raises(ValueError):
        mk().next_queries()
    a, b = mk(), mk(labels="one")
    a.run(3), b.run(3)
    torch.cuda.synchronize()
    assert np.array_equal(bits(a.embeddings), bits(b.embeddings))


# ------------------------------------------------------------------------------------------------ the driver
def test_driver_softmax_labels(tmp_path):
    """train.py --objective softmax --softmax_labels all on the toy KG of tests/test_gpu_train_eval.py: it trains (one log
    line gives the query counts), writes the checkpoint with the accumulator, resumes, and --infer ranks far above chance
    (0.04 over 120 candidates).  --softmax_labels one writes the files the default writes."""
    from test_gpu_train_eval import _toy_kg
    from graphembeddings_amd import data as D
    from graphembeddings_amd import train as T
    dd = tmp_path / "data"
    dd.mkdir()
    data_dir, out = _toy_kg(dd), str(tmp_path / "run")
    base = ["--data_dir", data_dir, "--batch_size", "64", "--embedding_dim", "32", "--learning_rate", "0.1", "--seed", "1",
            "--objective", "softmax", "--optimizer", "adagrad"]
    argv = base + ["--output_dir", out, "--num_epochs", "30", "--softmax_labels", "all"]
    FLAGS = T.build_parser().parse_args(argv)
    T.check_objective_flags(FLAGS)
    data = D.init_data(data_dir)
    logs = []
    res = T.run_training(data, FLAGS, log=lambda *a: logs.append(" ".join(str(x) for x in a)))
    batch_count = data.triple_count // 64
    assert res["steps"] == 30 * (batch_count - 1) and np.isfinite(res["final_mean_softmax_loss"])
    assert any("no validation ticks" in l for l in logs)
    line = [l for l in logs if l.startswith("Softmax labels: all")]
    assert len(line) == 1 and "tail queries" in line[0] and "head queries" in line[0] and str(data.triple_count) in line[0]
    emb, step, acc = T.load_checkpoint(out, with_accumulator=True)
    assert step == res["global_step"] and acc is not None and acc.shape == emb.shape and float(acc.min()) >= F32(0.1)
    assert float(acc[:data.relation_count].max()) > 0.1 and float(acc.max()) > 0.1
    res2 = T.run_training(data, T.build_parser().parse_args(argv + ["--resume_checkpoint", "--num_epochs", "1"]),
                          log=lambda *a: None)
    assert res2["steps"] == batch_count - 1 and res2["global_step"] == res["global_step"] + res2["steps"]
    _, _, acc2 = T.load_checkpoint(out, with_accumulator=True)
    assert bool((acc2 >= acc).all()) and bool((acc2 > acc).any())
    m = T.infer_triples(T.build_parser().parse_args(argv + ["--infer", "--infer_threshold", "1.0"]), log=lambda *a: None)
    print("SOFTMAX-LABELS driver: filtered MRR %.4f after %d steps" % (m["filtered_mrr"], res["steps"] + res2["steps"]))
    assert m["recorded"] == m["sweeps"] == 80 and m["filtered_mrr"] > 0.15
    # the default and --softmax_labels one: the same files
    kept = []
    for n, extra in enumerate(([], ["--softmax_labels", "one"])):
        o = str(tmp_path / ("one%d" % n))
        lg = []
        T.run_training(data, T.build_parser().parse_args(base + ["--output_dir", o, "--num_epochs", "2", *extra]),
                       log=lambda *a: lg.append(" ".join(str(x) for x in a)))
        e, s, a = T.load_checkpoint(o, with_accumulator=True)
        kept.append((bits(e), s, bits(a), [l for l in lg if "seconds" not in l]))
        assert not any("Softmax labels" in l for l in lg)
    assert np.array_equal(kept[0][0], kept[1][0]) and kept[0][1] == kept[1][1] and np.array_equal(kept[0][2], kept[1][2])
