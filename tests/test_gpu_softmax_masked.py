"""GPU: the type-constrained 1-vs-all softmax objective of ComplEx (ge_softmax_masked_loss / ge_softmax_masked_grad,
hole.softmax_loss / softmax_grad / SoftmaxAdaGrad / SoftmaxTrainer with candidate_sets, train.py
--softmax_candidate_sets) against tests/softmax_masked_ref.py.

Shapes and bound are those of tests/test_gpu_softmax.py: tiles of 64 query rows x 64 candidates, at most 8 candidate
ranges (K = 577: 5 ranges of 2 tiles), 32-column blocks of the gradient GEMM; per case e32 = the largest absolute
deviation of the reference's float32 evaluation from its fp64 evaluation, and the GPU must be within 8 * e32 + 1e-7 of the
fp64 oracle.  Every case prints its four figures (`-s`).

The five sets of a case: all positions; a random half in which positions 31 and 63 are in and 32 and 64 out (both sides
of a mask word and of a tile); the block [40, 40 + K/3), which is not tile-aligned; position 0 plus the last tile; the
empty set.  Bits at positions >= K are ones.  Rows cycle through the sets -1, 0, 1, 2, 3 (-1 where the set is empty at
this K) and draw their true candidate from their set.

DESIGN.md section 24 has the table of the figures measured on MI355X."""
import functools
import types

import numpy as np
import pytest
import torch

from graphembeddings_amd import _lib
from graphembeddings_amd import evaluate as EV
from graphembeddings_amd import hole as H
from tests import softmax_masked_ref as MR
from tests import softmax_ref as SR

pytestmark = pytest.mark.gpu

I32, F32 = np.int32, np.float32
N_REL, EXTRA = 4, 40
A0, DELTA = 0.1, 5e-5                                   # tests/test_gpu_adagrad.py


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(I32) if a.dtype == F32 else a


def five_sets(K, seed):
    rng = np.random.default_rng(seed)
    s = np.zeros((5, K), bool)
    s[0] = True
    s[1] = rng.random(K) < 0.5
    for p, on in ((31, True), (32, False), (63, True), (64, False)):
        if p < K:
            s[1, p] = on
    s[2, 40:40 + K // 3] = True
    s[3, 0] = True
    s[3, 64 * ((K - 1) // 64):] = True
    return s


@functools.lru_cache(maxsize=None)
def build(B, K, d, max_norm, head, seed=0):
    """(table, hr, true, cand, row_set [B], sets bool [5, K]): the case of tests/test_gpu_softmax.py's build -- log-normal
    row norms around max_norm, rows 0..2 sharing a fixed entity that is candidate 0, one relation for B in (63, 130),
    every fourth row behind the first ones with the largest logit its row can have on its true candidate -- with the
    true candidate of every row drawn from the row's set: the first rows take the set's first and last position and
    its positions next to a 64-column boundary."""
    rng = np.random.default_rng(1000 * B + 7 * K + d + seed)
    n_ent = K + EXTRA
    N = N_REL + n_ent
    t = rng.standard_normal((N, d))
    norms = max_norm * np.exp(rng.normal(0.0, 0.5, N))
    norms = np.where(np.abs(norms / max_norm - 1) < 0.01, 1.05 * max_norm, norms)
    norms[:N_REL] = max_norm * np.array([0.6, 1.7, 0.8, 2.5])
    t = (t * (norms / np.linalg.norm(t, axis=1))[:, None]).astype(F32)
    ents = N_REL + rng.permutation(n_ent)
    cand, extra = ents[:K].astype(I32), ents[K:]
    hr = np.stack([rng.integers(N_REL, N, B), rng.integers(0, N_REL, B)], 1).astype(I32)
    if B in (63, 130):
        hr[:, 1] = 1
    hr[:3, 0] = cand[0]
    sets = five_sets(K, 31 * K + seed)
    rs = (np.arange(B) % 5) - 1
    rs = np.where((rs >= 0) & ~sets[np.maximum(rs, 0)].any(1), -1, rs).astype(I32)
    adm, _ = MR.admissible(rs, sets)
    edge = {0, K - 1} | {c for b in range(64, K, 64) for c in (b - 1, b)}
    col, used = np.zeros(B, np.int64), set()
    for i in range(B):
        mine = np.nonzero(adm[i])[0]
        first = [c for c in mine if (c in edge or c in (mine[0], mine[-1])) and c not in used]
        col[i] = first[0] if first and i < 40 else rng.choice(mine)
        used.add(int(col[i]))
    # every fourth row: a true column of its own (where its set has one left) and a fixed entity that is no candidate
    taken = set(col.tolist())
    for n, i in enumerate(range(11, B, 4)):
        free = [c for c in np.nonzero(adm[i])[0] if c not in taken]
        if not free:
            continue
        col[i] = free[rng.integers(len(free))]
        taken.add(int(col[i]))
        hr[i, 0] = extra[n % EXTRA]
        f, r = t[hr[i, 0]].astype(np.float64)[None], t[hr[i, 1]].astype(np.float64)[None]
        q = SR.query(SR._clip(f, max_norm)[0], SR._clip(r, max_norm)[0], head)[0]
        t[cand[col[i]]] = (-1.5 * max_norm * q / np.linalg.norm(q)).astype(F32)
    nrm = np.linalg.norm(t.astype(np.float64), axis=1)
    assert (np.abs(nrm / max_norm - 1) > 0.005).all() and (nrm > 0).all() and adm[np.arange(B), col].all()
    return t, hr, cand[col].astype(I32), cand, rs, sets


def e32_of(t, hr, true, cand, mn, scale, head, rs, sets):
    """(fp64 loss, idx, val at lr = 1; e32 of the loss; e32 of the gradient rows)."""
    l64, idx, v64 = MR.evaluate(t, hr, true, cand, mn, scale, head, rs, sets)
    l32, i32_, v32 = MR.evaluate(t, hr, true, cand, mn, scale, head, rs, sets, dtype=np.float32)
    assert np.array_equal(idx, i32_)
    ok = ~np.isnan(l64)
    return l64, idx, v64, float(np.abs(l32 - l64)[ok].max()) if ok.any() else 0.0, float(np.abs(v32 - v64).max())


@functools.lru_cache(maxsize=None)
def reference(B, K, d, max_norm, scale, head, seed=0):
    t, hr, true, cand, rs, sets = build(B, K, d, max_norm, head, seed)
    return e32_of(t, hr, true, cand, max_norm, scale, head, rs, sets)


def gpu_masked(t, hr, true, cand, mn, scale, head, rs, mask, lr=1.0, grad=True):
    """The entry points themselves (row sets of any value reach them): (loss, grad_idx, grad_val), or the loss alone."""
    T, h, tr, c, r, m = dev(t), dev(hr.astype(I32)), dev(true.astype(I32)), dev(cand.astype(I32)), dev(np.asarray(rs, I32)), \
        dev(np.asarray(mask).view(I32))
    B, K, d = len(hr), len(cand), t.shape[1]
    assert m.shape[1] == H.candidate_mask_words(K)
    ws = H.softmax_masked_workspace(T, B, K)
    loss = torch.empty(B, dtype=torch.float32, device="cuda")
    if not grad:
        _lib.call("ge_softmax_masked_loss", T.data_ptr(), T.shape[0], d, h.data_ptr(), B, tr.data_ptr(), c.data_ptr(), K,
                  float(mn), float(scale), H.MODEL_COMPLEX, int(head), loss.data_ptr(), ws.data_ptr(), ws.numel(),
                  r.data_ptr(), m.data_ptr(), m.shape[0], H._stream())
        torch.cuda.synchronize()
        return loss.cpu().numpy()
    gi = torch.empty(K + 2 * B, dtype=torch.int32, device="cuda")
    gv = torch.empty(K + 2 * B, d, dtype=torch.float32, device="cuda")
    _lib.call("ge_softmax_masked_grad", T.data_ptr(), T.shape[0], d, h.data_ptr(), B, tr.data_ptr(), c.data_ptr(), K,
              float(mn), float(scale), float(lr), H.MODEL_COMPLEX, int(head), loss.data_ptr(), gi.data_ptr(), gv.data_ptr(),
              ws.data_ptr(), ws.numel(), r.data_ptr(), m.data_ptr(), m.shape[0], H._stream())
    torch.cuda.synchronize()
    return loss.cpu().numpy(), gi.cpu().numpy(), gv.cpu().numpy()


def gpu_plain(t, hr, true, cand, mn, scale, head, lr=1.0):
    loss, gi, gv = H.softmax_grad(dev(t), dev(hr), dev(true), dev(cand), lr, scale=scale, max_norm=mn,
                                  side="head" if head else "tail")
    torch.cuda.synchronize()
    return loss.cpu().numpy(), gi.cpu().numpy(), gv.cpu().numpy()


def sets_object(cand, sets):
    """What hole.softmax_loss / softmax_grad take as candidate_sets (evaluate.CandidateSets' three attributes)."""
    return types.SimpleNamespace(mask=dev(MR.pack(sets, True).view(I32)), n_sets=len(sets), cand=dev(np.asarray(cand, I32)))


def check_case(B, K, d, max_norm, scale, head):
    t, hr, true, cand, rs, sets = build(B, K, d, max_norm, head)
    l64, idx, v64, e_l, e_g = reference(B, K, d, max_norm, scale, head)
    loss, gi, gv = gpu_masked(t, hr, true, cand, max_norm, scale, head, rs, MR.pack(sets, True))
    assert np.isfinite(l64).all() and np.array_equal(gi, idx)
    dl, dg = float(np.abs(loss - l64).max()), float(np.abs(gv - v64).max())
    print("SOFTMAX-MASKED B=%d K=%d d=%d max_norm=%g scale=%g side=%s: loss e32 %.3g gpu %.3g | grad e32 %.3g gpu %.3g"
          % (B, K, d, max_norm, scale, "head" if head else "tail", e_l, dl, e_g, dg))
    assert np.isfinite(loss).all() and np.isfinite(gv).all()
    assert dl <= 8 * e_l + 1e-7, ("loss", dl, e_l)
    assert dg <= 8 * e_g + 1e-7, ("grad", dg, e_g)
    # w_ij = 0 exactly: a candidate no row admits has its id and an exact zero row
    adm, _ = MR.admissible(rs, sets)
    nobody = ~adm.any(0)
    assert np.array_equal(gi[:K], cand) and not gv[:K][nobody].any()


NORMS_SCALES = [(1.0, 20.0), (4.0, 200.0)]


@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("max_norm,scale", NORMS_SCALES)
@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 129, 300, 577])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_shapes(B, K, max_norm, scale, head):
    check_case(B, K, 64, max_norm, scale, head)


@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("max_norm,scale", NORMS_SCALES)
@pytest.mark.parametrize("d", [8, 56, 200, 288])
def test_widths(d, max_norm, scale, head):
    check_case(130, 300, d, max_norm, scale, head)


def test_the_sets_are_what_the_docstring_says():
    s = five_sets(300, 1)
    assert s[0].all() and s[1, 31] and not s[1, 32] and s[1, 63] and not s[1, 64] and 100 < s[1].sum() < 200
    assert np.array_equal(np.nonzero(s[2])[0], np.arange(40, 140)) and np.array_equal(np.nonzero(s[3])[0], [0] + list(range(256, 300)))
    assert not s[4].any()
    w = MR.pack(s, True)
    assert w.shape == (5, 12) and w[4, 9] == 0xFFFFF000 and (w[4, :9] == 0).all() and (w[:, 10:] == 0xFFFFFFFF).all()
    t, hr, true, cand, rs, sets = build(130, 300, 64, 1.0, False)
    assert sorted(set(rs.tolist())) == [-1, 0, 1, 2, 3]
    assert (build(65, 2, 64, 1.0, False)[4][3::5] == -1).all()        # the block [40, 40) is empty at K = 2


@pytest.mark.parametrize("head", [False, True])
def test_dead_tiles(head):
    """Three row tiles whose sets are [0, 64), [64, 200) and [250, 320): of the 15 tile pairs 6 are live.  Against the
    oracle, and against three unmasked calls on the compacted candidate lists within the sum of the two bounds."""
    B, K, d, mn, scale = 192, 320, 64, 1.0, 20.0
    t, hr, _, cand, _, _ = build(B, K, d, mn, head)
    sets = np.zeros((3, K), bool)
    sets[0, :64], sets[1, 64:200], sets[2, 250:] = True, True, True
    rs = (np.arange(B) // 64).astype(I32)
    rng = np.random.default_rng(5)
    col = np.array([rng.choice(np.nonzero(sets[s])[0]) for s in rs])
    col[[0, 63, 64, 127, 128, 191]] = [0, 63, 64, 199, 250, 319]
    true = cand[col]
    l64, idx, v64, e_l, e_g = e32_of(t, hr, true, cand, mn, scale, head, rs, sets)
    loss, gi, gv = gpu_masked(t, hr, true, cand, mn, scale, head, rs, MR.pack(sets, True))
    dl, dg = float(np.abs(loss - l64).max()), float(np.abs(gv - v64).max())
    print("SOFTMAX-MASKED dead tiles side=%s: loss e32 %.3g gpu %.3g | grad e32 %.3g gpu %.3g"
          % ("head" if head else "tail", e_l, dl, e_g, dg))
    assert np.array_equal(gi, idx) and dl <= 8 * e_l + 1e-7 and dg <= 8 * e_g + 1e-7
    assert not gv[200:250].any() and gv[:200].any(1).all() and gv[250:K].any(1).all()
    for s in range(3):
        rows, cols = np.nonzero(rs == s)[0], np.nonzero(sets[s])[0]
        pl, pi, pv = gpu_plain(t, hr[rows], true[rows], cand[cols], mn, scale, head)
        r64 = SR.evaluate(t, hr[rows], true[rows], cand[cols], mn, scale, head)
        r32 = SR.evaluate(t, hr[rows], true[rows], cand[cols], mn, scale, head, dtype=np.float32)
        bl = 8 * e_l + 1e-7 + 8 * float(np.abs(r32[0] - r64[0]).max()) + 1e-7
        bg = 8 * e_g + 1e-7 + 8 * float(np.abs(r32[2] - r64[2]).max()) + 1e-7
        assert np.abs(loss[rows] - pl).max() <= bl
        assert np.array_equal(gi[cols], pi[:len(cols)]) and np.abs(gv[cols] - pv[:len(cols)]).max() <= bg
        q = K + 2 * rows
        assert np.array_equal(gi[q], pi[len(cols)::2]) and np.array_equal(gi[q + 1], pi[len(cols) + 1::2])
        assert np.abs(gv[q] - pv[len(cols)::2]).max() <= bg and np.abs(gv[q + 1] - pv[len(cols) + 1::2]).max() <= bg


@pytest.mark.parametrize("head", [False, True])
def test_empty_ranges(head):
    """(130, 577): five ranges of two candidate tiles.  The rows of the first row tile admit the last candidate tile only
    (one position), so four of that tile's five ranges are empty; the other rows are unrestricted."""
    B, K, d, mn, scale = 130, 577, 64, 1.0, 20.0
    t, hr, true, cand, _, _ = build(B, K, d, mn, head)
    sets = np.zeros((1, K), bool)
    sets[0, 576] = True
    rs = np.where(np.arange(B) < 64, 0, -1).astype(I32)
    true = true.copy()
    true[:64] = cand[576]
    l64, idx, v64, e_l, e_g = e32_of(t, hr, true, cand, mn, scale, head, rs, sets)
    loss, gi, gv = gpu_masked(t, hr, true, cand, mn, scale, head, rs, MR.pack(sets, True))
    assert np.array_equal(gi, idx) and not loss[:64].any() and not l64[:64].any()     # one admissible candidate: loss 0
    assert np.abs(loss - l64).max() <= 8 * e_l + 1e-7 and np.abs(gv - v64).max() <= 8 * e_g + 1e-7
    assert not gv[K:K + 128].any()                      # p = 1 on the only candidate: exact zero gradients


@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("B,K,d", [(130, 300, 64), (65, 577, 200), (1, 1, 8)])
def test_exact_properties(B, K, d, head):
    mn, scale = 1.0, 20.0
    t, hr, true, cand, rs, sets = build(B, K, d, mn, head)
    mask = MR.pack(sets, True)
    same = lambda x, y: all(np.array_equal(bits(u), bits(v)) for u, v in zip(x, y))
    # all bits set, or row_set = -1: the unmasked entry points, bit for bit (the true ids are candidates either way)
    plain = gpu_plain(t, hr, true, cand, mn, scale, head)
    ones = np.full_like(mask, 0xFFFFFFFF)
    assert same(gpu_masked(t, hr, true, cand, mn, scale, head, np.maximum(rs, 0), ones), plain)
    assert same(gpu_masked(t, hr, true, cand, mn, scale, head, np.full(B, -1), mask), plain)
    a, b = (gpu_masked(t, hr, true, cand, mn, scale, head, rs, mask) for _ in range(2))
    assert same(a, b)                                   # two identical calls
    if K > 2:
        assert not same(a, plain)
    lo = gpu_masked(t, hr, true, cand, mn, scale, head, rs, mask, grad=False)
    assert np.array_equal(bits(lo), bits(a[0]))
    lp = H.softmax_loss(dev(t), dev(hr), dev(true), dev(cand), scale=scale, max_norm=mn, side="head" if head else "tail",
                        candidate_sets=sets_object(cand, sets), row_sets=dev(rs))
    assert np.array_equal(bits(lp), bits(a[0]))
    half = gpu_masked(t, hr, true, cand, mn, scale, head, rs, mask, lr=0.5)
    assert np.array_equal(half[1], a[1]) and np.array_equal(bits(half[2]), bits((F32(0.5) * a[2]).astype(F32)))
    perm = np.random.default_rng(B).permutation(B)
    p = gpu_masked(t, hr[perm], true[perm], cand, mn, scale, head, rs[perm], mask)
    assert np.array_equal(bits(p[0]), bits(a[0][perm]))
    q = lambda g: g[K:].reshape(B, 2, -1)
    assert np.array_equal(q(p[1])[:, :, 0], q(a[1])[perm][:, :, 0]) and np.array_equal(bits(q(p[2])), bits(q(a[2])[perm]))
    # a set no row uses (4, the empty one, and a sixth), and the bits at positions >= K, change nothing
    other = np.concatenate([mask, mask[1:2]])
    other[4] = 0x55555555
    assert same(gpu_masked(t, hr, true, cand, mn, scale, head, rs, other), a)
    assert same(gpu_masked(t, hr, true, cand, mn, scale, head, rs, MR.pack(sets, False)), a)
    # a candidate no row admits: its id and an exact zero row
    adm, _ = MR.admissible(rs, sets)
    assert np.array_equal(a[1][:K], cand) and not a[2][:K][~adm.any(0)].any()


@pytest.mark.parametrize("head", [False, True])
def test_invalid_rows(head):
    """Appended to (65, 129): a true id its set does not admit, row_set = n_sets, row_set = -2, the empty set.  NaN / -1 /
    zero rows, and everything else is bit for bit what it is without them."""
    B, K, d, mn, scale = 65, 129, 64, 1.0, 20.0
    t, hr, true, cand, rs, sets = build(B, K, d, mn, head)
    mask = MR.pack(sets, True)
    base = gpu_masked(t, hr, true, cand, mn, scale, head, rs, mask)
    out_of_2 = int(np.nonzero(~sets[2])[0][0])
    hr2 = np.concatenate([hr, hr[:4]]).astype(I32)
    true2 = np.concatenate([true, [cand[out_of_2], true[1], true[2], cand[0]]]).astype(I32)
    rs2 = np.concatenate([rs, [2, 5, -2, 4]]).astype(I32)
    loss, gi, gv = gpu_masked(t, hr2, true2, cand, mn, scale, head, rs2, mask)
    l64, idx, v64 = MR.evaluate(t, hr2, true2, cand, mn, scale, head, rs2, sets)
    assert np.isnan(loss[B:]).all() and np.isnan(l64[B:]).all() and np.array_equal(gi, idx)
    assert (gi[K + 2 * B:] == -1).all() and not gv[K + 2 * B:].any()
    assert np.array_equal(bits(loss[:B]), bits(base[0]))
    assert np.array_equal(gi[:K + 2 * B], base[1]) and np.array_equal(bits(gv[:K + 2 * B]), bits(base[2]))


def test_host_checks():
    t, hr, true, cand, rs, sets = build(63, 64, 64, 1.0, False)
    T, h, tr, c = dev(t), dev(hr), dev(true), dev(cand)
    cs = sets_object(cand, sets)
    H.softmax_loss(T, h, tr, c, scale=20.0, candidate_sets=cs, row_sets=dev(rs))
    with pytest.raises(ValueError):
        H.softmax_loss(T, h, tr, c, scale=20.0, row_sets=dev(rs))                       # row_sets without the sets
    with pytest.raises(ValueError):
        H.softmax_loss(T, h, tr, c.flip(0), scale=20.0, candidate_sets=cs, row_sets=dev(rs))    # another candidate list
    with pytest.raises(ValueError):
        H.softmax_grad(T, h, tr, c, 1.0, scale=20.0, candidate_sets=cs, row_sets=dev(rs[:-1]))
    with pytest.raises(ValueError):
        H.softmax_grad(T, h, tr, c, 1.0, scale=20.0, candidate_sets=cs, row_sets=dev(np.full(63, 5)))
    with pytest.raises(ValueError):
        H.softmax_grad(T, h, tr, c[:-1], 1.0, scale=20.0, candidate_sets=cs, row_sets=dev(rs))
    with pytest.raises(ValueError):
        H.SoftmaxAdaGrad(T, c, 63, scale=20.0, candidate_sets=cs)                        # a dict with both sides
    with pytest.raises(ValueError):
        H.SoftmaxTrainer(T, dev(np.zeros((64, 3), I32)), c, 63, scale=20.0, n_samples=8, candidate_sets={"tail": cs, "head": cs})
    with pytest.raises(ValueError):
        H.SoftmaxAdaGrad(T, c, 63, scale=20.0).step(dev(np.zeros((63, 3), I32)), 0.1, row_sets=dev(rs))


# ------------------------------------------------------------------------------------------------ the step
@functools.lru_cache(maxsize=None)
def step_case():
    """(table, triples [B,3], cand, row_set, sets): the tail-side case of build(130, 300, 64) as triples; heads that are
    no candidates, or that the row's set does not admit, are replaced by a candidate from the set.  Both sides use the
    same sets; candidates [200, 220) are admitted by set 0 only and no row uses set 0 or -1 here."""
    t, hr, true, cand, rs, sets = build(130, 300, 64, 1.0, False)
    sets = sets.copy()
    sets[1:, 200:220] = False
    rs = np.where(rs <= 0, 1 + np.arange(130) % 3, rs).astype(I32)
    adm, _ = MR.admissible(rs, sets)
    rng = np.random.default_rng(9)
    pick = lambda i: cand[rng.choice(np.nonzero(adm[i])[0])]
    tri = np.stack([hr[:, 0], true, hr[:, 1]], 1).astype(I32)
    pos = {int(c): j for j, c in enumerate(cand)}
    for i in range(130):
        for c in (0, 1):
            j = pos.get(int(tri[i, c]), -1)
            if j < 0 or not adm[i, j]:
                tri[i, c] = pick(i)
    return t, tri, cand, rs, sets


def check_step(got_t, got_a, ref_t, ref_a, s, counts, lr, gb, steps=1):
    """tests/test_gpu_softmax.py's check_step: the per-step bounds of tests/test_gpu_adagrad.py with the gradient bound
    gb = 8 e32 + 1e-7 added to DELTA."""
    smax = np.abs(s).max(1, keepdims=True)
    delta = steps * (DELTA * np.where(counts[:, None] > 16, np.maximum(1.0, smax), 1.0) + gb)
    et, ea = np.abs(got_t - ref_t), np.abs(got_a - ref_a)
    bt = np.broadcast_to(lr * delta / np.sqrt(A0), ref_t.shape)
    ba = 2.0 * smax * delta + 4.0 * steps * np.spacing(ref_a.astype(F32)).astype(np.float64)
    print("SOFTMAX-MASKED step: table err/bound %.3g (|err| %.3g), accumulator err/bound %.3g (|err| %.3g)"
          % ((et / bt).max(), et.max(), (ea / ba).max(), ea.max()))
    assert np.all(et < bt) and np.all(ea < ba)


def test_step():
    t, tri, cand, rs, sets = step_case()
    N, d = t.shape
    B, K, lr, scale = len(tri), len(cand), 0.1, 20.0
    ref_t, ref_a = t.astype(np.float64), np.full((N, d), A0, np.float64)
    ref_loss, s, named = MR.step(ref_t, ref_a, tri, cand, 1.0, scale, lr, sets, sets, rs)
    assert np.isfinite(ref_loss).all()
    e = []
    for head, (fx, tr) in ((False, (0, 1)), (True, (1, 0))):
        e.append(e32_of(t, tri[:, [fx, 2]], tri[:, tr], cand, 1.0, scale, head, rs, sets)[3:])
    gb = 8 * max(x[1] for x in e) + 1e-7
    counts = np.bincount(np.concatenate([cand, cand, tri[:, 0], tri[:, 1], tri[:, 2], tri[:, 2]]), minlength=N)
    cs = sets_object(cand, sets)
    emb = dev(t)
    opt = H.SoftmaxAdaGrad(emb, dev(cand), B, scale=scale, initial_accumulator_value=A0, candidate_sets={"tail": cs, "head": cs})
    loss = opt.step(dev(tri), lr, row_sets=dev(rs))
    torch.cuda.synchronize()
    assert loss.shape == (B, 2)
    # the losses in the caller's order (the step sorts the rows by set id)
    assert np.abs(loss.cpu().numpy() - ref_loss).max() <= 8 * max(x[0] for x in e) + 1e-7
    got_t, got_a = emb.cpu().numpy(), opt.accumulator.cpu().numpy()
    check_step(got_t, got_a, ref_t, ref_a, s, counts, lr, gb)
    # rows named by nothing, and candidates no row admits: bit-identical in both arrays
    nobody = cand[200:220]
    assert not named[nobody].any() and not np.isin(nobody, tri[:, :2]).any() and not named.all()
    assert np.array_equal(bits(got_t[~named]), bits(t[~named])) and (got_a[~named] == F32(A0)).all()
    assert (got_a[named] > F32(A0)).any()
    with pytest.raises(ValueError):
        opt.step(dev(tri[:-1]), lr)


def test_step_is_reproducible():
    t, tri, cand, rs, sets = step_case()
    cs = sets_object(cand, sets)
    runs = []
    for _ in range(2):
        emb = dev(t)
        opt = H.SoftmaxAdaGrad(emb, dev(cand), len(tri), scale=20.0, initial_accumulator_value=A0,
                               candidate_sets={"tail": cs, "head": cs})
        for k in range(5):
            opt.step(dev(np.roll(tri, 7 * k, axis=0)), 0.1, row_sets=dev(np.roll(rs, 7 * k)))
        torch.cuda.synchronize()
        runs.append((emb.cpu().numpy(), opt.accumulator.cpu().numpy()))
    assert np.array_equal(bits(runs[0][0]), bits(runs[1][0])) and np.array_equal(bits(runs[0][1]), bits(runs[1][1]))
    assert not np.array_equal(bits(runs[0][0]), bits(t))


# ------------------------------------------------------------------------------------------------ learning
N_REL_KG, D_KG, B_KG, STEPS_KG, SCALE_KG, LR_KG = 8, 64, 512, 300, 20.0, 0.1


def test_learning():
    """300 steps of SoftmaxAdaGrad with the type sets on the typed planted KG (tests/softmax_masked_ref.py) reach the
    filtered MRR against the sets of the same batches run through the fp64 reference: the replay >= 0.20 (measured in
    fp64 with torch autograd: 0.2386; batch seeds 4 and 5: 0.218 and 0.253; unmasked training evaluated the same way:
    0.2202; chance about 0.016), the GPU within 0.03 of the replay."""
    train, test, all_tri, cand, sets, typ = MR.typed_setup(N_REL_KG)
    N = N_REL_KG + len(typ)
    id_to_type = np.concatenate([np.full(N_REL_KG, -1), typ]).astype(I32)
    cs = {side: EV.CandidateSets.from_types(cand, id_to_type, train.astype(np.int64), N_REL_KG, side) for side in ("tail", "head")}
    p = np.arange(len(cand))
    for side in cs:                                     # from_types builds the sets the reference is given
        words = cs[side].mask.cpu().numpy().view(np.uint32)
        assert np.array_equal(((words[:, p >> 5] >> (p & 31).astype(np.uint32)) & 1).astype(bool), sets[side])
    t0 = (np.random.default_rng(0).standard_normal((N, D_KG)) * np.sqrt(2.6 / (N + D_KG))).astype(F32)
    emb = dev(t0)
    opt = H.SoftmaxAdaGrad(emb, dev(cand), B_KG, scale=SCALE_KG, initial_accumulator_value=A0, candidate_sets=cs)
    rows = MR.batches(len(train), B_KG, STEPS_KG, seed=3)
    dtrain = dev(train)
    last = None
    for r in rows:
        last = opt.step(dtrain[dev(r)].contiguous(), LR_KG)
    torch.cuda.synchronize()
    assert torch.isfinite(last).all()
    ref_t, ref_a = t0.astype(np.float64), np.full((N, D_KG), A0, np.float64)
    for r in rows:
        MR.step(ref_t, ref_a, train[r], cand, 1.0, SCALE_KG, LR_KG, sets["tail"], sets["head"])
    ref_mrr = MR.mrr_masked(ref_t, test, all_tri, cand, sets)
    fil = []
    for side in ("tail", "head"):
        _, f, a = EV.link_prediction_ranks(emb, test.astype(np.int64), cand.astype(np.int64), known_triples=all_tri.astype(np.int64),
                                           side=side, candidate_sets=cs[side], return_admissible=True)
        assert a.all()
        fil.append(f)
    gpu_mrr = float(np.mean(1.0 / np.concatenate(fil).astype(np.float64)))
    print("SOFTMAX-MASKED learning: reference MRR %.4f, GPU MRR %.4f" % (ref_mrr, gpu_mrr))
    assert ref_mrr >= 0.20
    assert abs(gpu_mrr - ref_mrr) <= 0.03


# ------------------------------------------------------------------------------------------------ the driver
def test_driver_softmax_candidate_sets(tmp_path):
    """train.py --objective softmax --softmax_candidate_sets observed on the toy KG of tests/test_gpu_train_eval.py, next to
    an unmasked run with the same flags: finite losses, the log line, a checkpoint that resumes, and a `constrained` MRR
    of --infer --candidate_sets observed of at least half the unmasked run's."""
    from test_gpu_train_eval import _toy_kg
    from graphembeddings_amd import data as D
    from graphembeddings_amd import train as T
    dd = tmp_path / "data"
    dd.mkdir()
    data_dir = _toy_kg(dd)
    data = D.init_data(data_dir)
    batch_count = data.triple_count // 64
    mrr = {}
    for kind in ("observed", "none"):
        out = str(tmp_path / ("run_" + kind))
        argv = ["--data_dir", data_dir, "--output_dir", out, "--batch_size", "64", "--embedding_dim", "32", "--num_epochs", "30",
                "--learning_rate", "0.1", "--seed", "1", "--objective", "softmax", "--optimizer", "adagrad",
                "--softmax_candidate_sets", kind]
        logs = []
        res = T.run_training(data, T.build_parser().parse_args(argv), log=lambda *a: logs.append(" ".join(str(x) for x in a)))
        assert res["steps"] == 30 * (batch_count - 1) and np.isfinite(res["final_mean_softmax_loss"])
        line = [l for l in logs if "Softmax candidate sets" in l]
        if kind == "observed":
            assert len(line) == 1 and "observed" in line[0] and "mean set size" in line[0]
            emb, step, acc = T.load_checkpoint(out, with_accumulator=True)
            res2 = T.run_training(data, T.build_parser().parse_args(argv + ["--resume_checkpoint", "--num_epochs", "1"]),
                                  log=lambda *a: None)
            assert res2["steps"] == batch_count - 1 and res2["global_step"] == res["global_step"] + res2["steps"]
            assert np.isfinite(res2["final_mean_softmax_loss"])
            _, _, acc2 = T.load_checkpoint(out, with_accumulator=True)
            assert bool((acc2 >= acc).all()) and bool((acc2 > acc).any())
        else:
            assert not line
        m = T.infer_triples(T.build_parser().parse_args(argv + ["--infer", "--infer_threshold", "1.0", "--candidate_sets",
                                                                "observed"]), log=lambda *a: None)
        mrr[kind] = m["constrained"]["mrr_and_hits"]["filtered_mrr"]
    print("SOFTMAX-MASKED driver: constrained filtered MRR %.4f with the sets, %.4f without" % (mrr["observed"], mrr["none"]))
    assert mrr["observed"] >= 0.5 * mrr["none"]
    # the type sets (the toy KG has two types; the candidates are then ordered by type): two epochs, finite losses
    logs = []
    argv = ["--data_dir", data_dir, "--output_dir", str(tmp_path / "run_types"), "--batch_size", "64", "--embedding_dim", "32",
            "--num_epochs", "2", "--learning_rate", "0.1", "--seed", "1", "--objective", "softmax", "--optimizer", "adagrad",
            "--softmax_candidate_sets", "types"]
    res = T.run_training(data, T.build_parser().parse_args(argv), log=lambda *a: logs.append(" ".join(str(x) for x in a)))
    assert res["steps"] == 2 * (batch_count - 1) and np.isfinite(res["final_mean_softmax_loss"])
    assert sum("Softmax candidate sets: types" in l for l in logs) == 1
