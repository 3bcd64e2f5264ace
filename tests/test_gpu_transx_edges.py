"""TransE / TransH / TransD kernels at the edges test_gpu_transx.py's random shapes never reach: every (VEC, LPT)
variant of the score and gradient kernels, misaligned tables, a grid-stride loop that wraps, the windowed apply's
run layouts, and the semantic edges (exact ties, sign(0), the l2_normalize clamp, invalid pairs, the sort's key
width).  On the exact fixtures of tests/transx_ref.py (small integer tables, lr = 2^-6, integer margin) fp32
computes every intermediate exactly in any order, so TransE / TransD losses and tables must equal the fp64
restatement bitwise: one slot dropped or added twice moves a table by at least lr.  TransH goes through rsqrtf and
is held to a bound scaled by each element's sum of |terms|."""
import numpy as np
import pytest
import torch

from tests import transx_ref as TR

pytestmark = pytest.mark.gpu
MODELS = ("transe", "transh", "transd")
EXACT_MODELS = ("transe", "transd")

# ------------------------------------------------------------------ the dispatch, mirrored from ge_transx.hip
MAX_WAVES = 2048 * 4                               # grid_for's kMaxBlocks x waves per 256-thread block


def _lpt_for(nvec):
    return 8 if nvec <= 8 else 16 if nvec <= 16 else 32 if nvec <= 32 else 64


def _variant(d, aligned=True):
    """(VEC, LPT) that vec4_ok / lpt_for pick for dimension d."""
    vec = 4 if d % 4 == 0 and aligned else 1
    return vec, _lpt_for(d // vec)


def _waves(B, d, aligned=True):
    return -(-B // (64 // _variant(d, aligned)[1]))


SWEEP_D = (1, 3, 8, 9, 31, 32, 36, 64, 65, 100, 128, 132, 200, 1023, 1024)


def test_sweep_covers_every_variant():
    """The sweep reaches all 8 kernel variants; a change of the dispatch thresholds that empties one fails here."""
    assert {_variant(d) for d in SWEEP_D} == {(v, lpt) for v in (1, 4) for lpt in (8, 16, 32, 64)}
    assert _variant(100, aligned=False) == (1, 64)
    assert _waves(20000, 200) > MAX_WAVES and _waves(40000, 100) > MAX_WAVES


# ------------------------------------------------------------------ helpers
def _model(model, E, R, d, l1, tabs=None, seed=0):
    from graphembeddings_amd import transx as X
    m = X.TransX(model, E, R, d, l1=l1, seed=seed)
    if tabs is not None:
        for k, v in tabs.items():
            m.tables[k].copy_(torch.as_tensor(np.asarray(v, dtype=np.float32)))
    return m


def _host(m):
    return {k: v.cpu().numpy().astype(np.float64) for k, v in m.tables.items()}


def _dev(a):
    return torch.as_tensor(np.asarray(a, dtype=np.int32)).cuda()


def _pairs(rng, E, R, B):
    pos = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, R, B)], 1).astype(np.int32)
    neg = pos.copy()
    neg[np.arange(B), rng.integers(0, 2, B)] = rng.integers(0, E, B)
    return pos, neg


def _run_step(m, pos, neg, lr, margin):
    before = _host(m)
    loss = float(m.step(_dev(pos), _dev(neg), lr, margin))
    return before, loss, _host(m)


def _assert_close(model, l1, before, loss, after, pos, neg, lr, margin, rtol=2.0 ** -20, atol=5e-6):
    """Loss to 5e-6 relative; each table element to atol + rtol * lr * (sum of |terms| reaching it)."""
    new, rloss = TR.sgd_step(model, before, pos, neg, lr, margin, l1)
    _, mag = TR.hinge_grads(model, before, pos, neg, margin, l1, magnitude=True)
    assert abs(loss - rloss) <= 5e-6 * max(1.0, abs(rloss)), (loss, rloss)
    for k in new:
        err = np.abs(after[k] - new[k])
        bound = atol + rtol * lr * mag[k]
        assert np.all(err <= bound), (k, float(err.max()), float((err / bound).max()))


def _assert_exact(model, l1, before, loss, after, pos, neg, lr, margin):
    assert TR.is_exact_step(model, before, pos, neg, lr, margin, l1)
    new, rloss = TR.sgd_step(model, before, pos, neg, lr, margin, l1)
    assert loss == rloss, (loss, rloss)
    for k in new:
        diff = np.flatnonzero(after[k] != new[k])
        assert len(diff) == 0, (k, len(diff), float(np.abs(after[k] - new[k]).max()))


def _check(model, l1, tabs, pos, neg, lr, margin, E, R, d):
    """One step from `tabs`: bitwise for TransE / TransD (the fixture must be exact), by bound for TransH."""
    m = _model(model, E, R, d, l1, tabs)
    before, loss, after = _run_step(m, pos, neg, lr, margin)
    if model in EXACT_MODELS:
        _assert_exact(model, l1, before, loss, after, pos, neg, lr, margin)
    else:
        _assert_close(model, l1, before, loss, after, pos, neg, lr, margin, rtol=1e-4, atol=1e-6)
    return before, loss, after


def _all_active_margin(model, tabs, pos, neg, l1):
    """The least integer margin with D+ - D- + margin >= 1 for every pair."""
    return float(np.ceil(TR.score(model, tabs, neg, l1).max() - TR.score(model, tabs, pos, l1).min()) + 1)


# ------------------------------------------------------------------ every kernel variant
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("d", SWEEP_D)
def test_variant_sweep_score_and_step(model, l1, d):
    E, R = 61, 7
    m = _model(model, E, R, d, l1, seed=d)
    rng = np.random.default_rng(100 + d)
    tri = _pairs(rng, E, R, 203)[0]                          # ragged B: no multiple of any lane-group count
    got = m.score(_dev(tri)).cpu().numpy().astype(np.float64)
    ref = TR.score(model, _host(m), tri, l1)
    assert np.all(np.abs(got - ref) <= 1e-5 * np.abs(ref) + 1e-7)
    pos, neg = _pairs(rng, E, R, 157)
    before, loss, after = _run_step(m, pos, neg, 0.01, 1.0)
    assert 0 < TR.active_mask(model, before, pos, neg, 1.0, l1).sum()
    _assert_close(model, l1, before, loss, after, pos, neg, 0.01, 1.0)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("l1", [True, False])
def test_misaligned_tables_take_vec1(model, l1):
    """d = 100 tables offset by one float (4- but not 16-byte aligned): the VEC1 / LPT64 fallback."""
    E, R, d = 80, 6, 100
    m = _model(model, E, R, d, l1, seed=4)
    for k, t in list(m.tables.items()):
        buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device=t.device)
        view = buf[1:1 + t.numel()].view_as(t)
        view.copy_(t)
        m.tables[k] = view
        assert view.data_ptr() % 16 == 4
    rng = np.random.default_rng(8)
    tri = _pairs(rng, E, R, 301)[0]
    got = m.score(_dev(tri)).cpu().numpy().astype(np.float64)
    ref = TR.score(model, _host(m), tri, l1)
    assert np.all(np.abs(got - ref) <= 1e-5 * np.abs(ref) + 1e-7)
    pos, neg = _pairs(rng, E, R, 250)
    before, loss, after = _run_step(m, pos, neg, 0.01, 1.0)
    _assert_close(model, l1, before, loss, after, pos, neg, 0.01, 1.0)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("B,d", [(20000, 200), (40000, 100)])
def test_grid_stride_wraps(model, B, d):
    """More lane groups than the capped grid holds: the score and gradient loops go round more than once."""
    assert _waves(B, d) > MAX_WAVES
    E, R, l1 = 3000, 40, False
    m = _model(model, E, R, d, l1, seed=6)
    start = {k: v.clone() for k, v in m.tables.items()}
    rng = np.random.default_rng(B)
    tri = _pairs(rng, E, R, B)[0]
    got = m.score(_dev(tri)).cpu().numpy().astype(np.float64)
    ref = TR.score(model, _host(m), tri, l1)
    assert np.all(np.abs(got - ref) <= 1e-5 * np.abs(ref) + 1e-7)
    pos, neg = _pairs(rng, E, R, B)
    before, loss, after = _run_step(m, pos, neg, 0.001, 1.0)
    _assert_close(model, l1, before, loss, after, pos, neg, 0.001, 1.0)
    for k, v in start.items():                               # the same step again from the same tables
        m.tables[k].copy_(v)
    loss2 = float(m.step(_dev(pos), _dev(neg), 0.001, 1.0))
    assert loss2 == loss
    for k, v in _host(m).items():
        assert np.array_equal(v, after[k]), k


# ------------------------------------------------------------------ the windowed apply's run layouts
def _layout(model, name, d, l1):
    f = TR.layout_batch(model, name, d, l1)
    act = TR.active_mask(model, f["tabs"], f["pos"], f["neg"], f["margin"], l1)
    _, srt = TR.slot_keys(f["pos"], f["neg"], f["E"], f["R"], act)
    for key, start, length in f["expect"]:                  # the batch has the layout it was built for
        assert TR.run_of(srt, key) == (start, length)
    return f


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", sorted(TR.LAYOUTS))
@pytest.mark.parametrize("d", [7, 8])                      # the VEC1 and VEC4 apply kernels
@pytest.mark.parametrize("l1", [True, False])
def test_reduction_layouts(model, name, d, l1):
    f = _layout(model, name, d, l1)
    _check(model, l1, f["tabs"], f["pos"], f["neg"], f["lr"], f["margin"], f["E"], f["R"], d)


# ------------------------------------------------------------------ semantic edges
@pytest.mark.parametrize("model", EXACT_MODELS)
@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("offset", [0, -1])
def test_exact_tie_is_active(model, l1, offset):
    """D+ - D- + margin == 0 takes its gradient (MaximumGrad ties to x); one less, z = -1, leaves the tables."""
    E, R, d = 12, 3, 8
    tabs = TR.exact_tables(model, E, R, d, seed=5)
    pos, neg = np.array([[0, 1, 0]]), np.array([[2, 1, 0]])
    margin = float(TR.score(model, tabs, neg, l1)[0] - TR.score(model, tabs, pos, l1)[0] + offset)
    assert TR.score(model, tabs, pos, l1)[0] - TR.score(model, tabs, neg, l1)[0] + margin == offset
    before, loss, after = _check(model, l1, tabs, pos, neg, 2.0 ** -6, margin, E, R, d)
    moved = any(not np.array_equal(after[k], before[k]) for k in after)
    assert moved == (offset == 0) and loss == 0.0


@pytest.mark.parametrize("model", EXACT_MODELS)
def test_l1_sign_of_zero_on_self_loop(model):
    """h == t under a zero relation row: u+ = 0 in every component, so sign(0) = 0 leaves no positive gradient."""
    E, R, d = 20, 3, 8
    tabs = TR.exact_tables(model, E, R, d, seed=7)
    tabs["rel"][1] = 0.0
    pos = np.array([[4, 4, 1], [9, 9, 1], [2, 6, 0]])
    neg = np.array([[5, 4, 1], [9, 3, 1], [2, 7, 0]])
    assert TR.score(model, tabs, pos[:2], True).tolist() == [0.0, 0.0]
    margin = _all_active_margin(model, tabs, pos, neg, True)
    _check(model, True, tabs, pos, neg, 2.0 ** -6, margin, E, R, d)


@pytest.mark.parametrize("l1", [True, False])
def test_transh_normal_clamp(l1):
    """TransH normals exactly zero, of scale 1e-8 and 1e-7 (n.n below l2_normalize's 1e-12: n^ = n * 1e6 and the
    clamp's branch drops out of the gradient) and of order 1, against fp64 by a bound relative to each element's
    sum of |terms|."""
    E, R, d = 30, 4, 16
    rng = np.random.default_rng(12)
    tabs = {"ent": rng.normal(size=(E, d)), "rel": rng.normal(size=(R, d)), "normal_vector": rng.normal(size=(R, d))}
    tabs["normal_vector"] *= np.array([0.0, 1e-8, 1e-7, 1.0])[:, None]
    tabs = {k: v.astype(np.float32).astype(np.float64) for k, v in tabs.items()}
    nn = (tabs["normal_vector"] ** 2).sum(1)
    # Within fp32 rounding of n.n = 1e-12 the kernel and fp64 may take different branches of max(); no row of
    # this fixture lies there (n.n is 0, ~1e-15, ~1e-13 or ~16), and this keeps it so.
    assert np.all(np.abs(nn - TR.EPS) > 1e-3 * TR.EPS)
    pos, neg = _pairs(rng, E, R, 96)
    pos[:, 2] = neg[:, 2] = np.arange(96) % R
    margin = _all_active_margin("transh", tabs, pos, neg, l1)
    _check("transh", l1, tabs, pos, neg, 0.01, margin, E, R, d)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("B", [1, 7])                     # 5 slots; 35 slots, just over one window
@pytest.mark.parametrize("l1", [True, False])
def test_small_batches(model, B, l1):
    E, R, d = 9, 2, 8
    tabs = TR.fixture_tables(model, E, R, d, seed=B)
    rng = np.random.default_rng(B)
    pos, neg = _pairs(rng, E, R, B)
    margin = _all_active_margin(model, tabs, pos, neg, l1)
    _check(model, l1, tabs, pos, neg, 2.0 ** -6, margin, E, R, d)


@pytest.mark.parametrize("model", MODELS)
def test_all_inactive_batch(model):
    """neg == pos under margin -1: every slot is a sentinel, the loss is exactly 0 and no table moves."""
    E, R, d = 50, 5, 36
    m = _model(model, E, R, d, True, seed=1)
    pos = _pairs(np.random.default_rng(1), E, R, 300)[0]
    before, loss, after = _run_step(m, pos, pos, 0.5, -1.0)
    assert loss == 0.0
    for k in before:
        assert np.array_equal(after[k], before[k]), k


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [7, 8])
def test_single_active_pair_among_inactive(model, d):
    E, R, B, i = 30, 4, 80, 37
    tabs = TR.fixture_tables(model, E, R, d, seed=3)
    rng = np.random.default_rng(3)
    pos = _pairs(rng, E, R, B)[0]
    neg = pos.copy()
    pos[i], neg[i] = TR._ordered_pair(model, tabs, rng, 2, E, 0, True)
    assert TR.active_mask(model, tabs, pos, neg, -1.0).tolist() == [k == i for k in range(B)]
    _check(model, True, tabs, pos, neg, 2.0 ** -6, -1.0, E, R, d)


@pytest.mark.parametrize("model", MODELS)
def test_invalid_pairs_are_skipped(model):
    """A pair with an id out of range (-1 or E on either side, -1 or R for the relation) or neg_r != pos_r takes
    no gradient and adds nothing to the loss: the step equals sgd_step on the valid pairs alone."""
    E, R, d = 40, 5, 8
    tabs = TR.fixture_tables(model, E, R, d, seed=9)
    rng = np.random.default_rng(9)
    pos, neg = _pairs(rng, E, R, 60)
    bad = [(0, 0, -1), (1, 1, E), (2, 0, E), (3, 1, -1)]           # (pair, column, id) of pos ...
    bad_neg = [(4, 0, -1), (5, 1, E), (6, 0, E), (7, 1, -1)]       # ... and of neg
    for i, c, v in bad:
        pos[i, c] = v
    for i, c, v in bad_neg:
        neg[i, c] = v
    pos[8, 2] = neg[8, 2] = -1
    pos[9, 2] = neg[9, 2] = R
    neg[10, 2] = (pos[10, 2] + 1) % R
    valid = np.ones(len(pos), dtype=bool)
    valid[:11] = False
    margin = _all_active_margin(model, tabs, pos[valid], neg[valid], True)
    m = _model(model, E, R, d, True, tabs)
    before, loss, after = _run_step(m, pos, neg, 2.0 ** -6, margin)
    if model in EXACT_MODELS:
        _assert_exact(model, True, before, loss, after, pos[valid], neg[valid], 2.0 ** -6, margin)
    else:
        _assert_close(model, True, before, loss, after, pos[valid], neg[valid], 2.0 ** -6, margin, rtol=1e-4,
                      atol=1e-6)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("k", [10, 16])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_key_width_at_power_of_two(model, k, delta):
    """E + R = 2^k + delta sets the sort's key width and the sentinel E + R: hot entity E - 1 and hot relation
    R - 1 sit right below it, and inactive pairs put sentinel slots right after relation R - 1's run."""
    R, d = 5, 8
    E = 2 ** k + delta - R
    tabs = TR.fixture_tables(model, E, R, d, seed=k)
    rng = np.random.default_rng(k + delta)
    ps, ns = [], []
    for _ in range(40):                                      # pairs through entity E - 1 under relation R - 1
        p = np.array([[E - 1, rng.integers(0, E), R - 1]])
        q = np.array([[rng.integers(0, E), E - 1 if rng.random() < 0.5 else rng.integers(0, E), R - 1]])
        dp, dq = TR.score(model, tabs, p)[0], TR.score(model, tabs, q)[0]
        if abs(dp - dq) >= (1.01 if model == "transh" else 1.0):
            ps.append((p if dp > dq else q)[0])
            ns.append((q if dp > dq else p)[0])
    idle = _pairs(rng, E, R, 25)[0]
    pos = np.concatenate([np.array(ps), idle]).astype(np.int32)
    neg = np.concatenate([np.array(ns), idle]).astype(np.int32)
    order = rng.permutation(len(pos))
    pos, neg = pos[order], neg[order]
    act = TR.active_mask(model, tabs, pos, neg, -1.0)
    _, srt = TR.slot_keys(pos, neg, E, R, act)
    start, length = TR.run_of(srt, E + R - 1)
    assert length == act.sum() >= 20 and srt[start + length] == E + R and TR.run_of(srt, E - 1)[1] >= 20
    _check(model, True, tabs, pos, neg, 2.0 ** -6, -1.0, E, R, d)


# ------------------------------------------------------------------ the native loop
@pytest.mark.parametrize("model", MODELS)
def test_run_continues_across_calls(model):
    """run(3) then run(4) is a fresh run(7), bitwise: the second call starts at step 3."""
    rng = np.random.default_rng(2)
    E, R = 200, 6
    tri = np.unique(np.stack([rng.integers(0, E, 1500), rng.integers(0, E, 1500), rng.integers(0, R, 1500)], 1), axis=0)
    a, b = _model(model, E, R, 24, True, seed=3), _model(model, E, R, 24, True, seed=3)
    ta = a.trainer(tri, 300, margin=1.0, learning_rate=0.01, seed=5)
    la = torch.cat([ta.run(3), ta.run(4)]).cpu().numpy()
    lb = b.trainer(tri, 300, margin=1.0, learning_rate=0.01, seed=5).run(7).cpu().numpy()
    assert ta.step_count == 7 and np.array_equal(la, lb)
    for k in a.tables:
        assert torch.equal(a.tables[k], b.tables[k]), k


@pytest.mark.parametrize("model", MODELS)
def test_trainer_batch_of_one(model):
    """B = 1 through the native loop: each step equals its drawn batch through the single step, and fp64."""
    rng = np.random.default_rng(4)
    E, R, d, lr = 30, 3, 12, 0.05
    tri = np.unique(np.stack([rng.integers(0, E, 120), rng.integers(0, E, 120), rng.integers(0, R, 120)], 1), axis=0)
    a, b = _model(model, E, R, d, True, seed=8), _model(model, E, R, d, True, seed=8)
    ref = _host(a)
    tr = a.trainer(tri, 1, margin=4.0, learning_rate=lr, seed=1)
    la = tr.run(5).cpu().numpy()
    for s in range(5):
        pos, neg = tr.draw(s)
        assert float(b.step(pos, neg, lr, 4.0)) == la[s], s
        ref, rloss = TR.sgd_step(model, ref, pos.cpu().numpy(), neg.cpu().numpy(), lr, 4.0, True)
        assert abs(la[s] - rloss) <= 5e-6 * max(1.0, abs(rloss)), s
    assert la.max() > 0
    for k in a.tables:
        assert torch.equal(a.tables[k], b.tables[k]), k
        assert np.abs(a.tables[k].cpu().numpy() - ref[k]).max() <= 5e-6, k
