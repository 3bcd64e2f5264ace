"""TransR on the MI355X through the C ABI (graphembeddings_amd.transr) against the fp64 restatement
tests/transr_ref.py and the Bernoulli oracle."""
import numpy as np
import pytest
import torch

from oracle import transx_oracle as TO
from tests import transr_ref as RR
from tests import transx_ref as TR

pytestmark = pytest.mark.gpu
F32_EPS = 2.0 ** -23


def _model(E, R, dim_e, dim_r, l1=True, seed=0, tabs=None):
    from graphembeddings_amd import transr as XR
    m = XR.TransR(E, R, dim_e, dim_r, l1=l1, seed=seed)
    if tabs is not None:
        for k, x in tabs.items():
            m.tables[k].copy_(torch.as_tensor(np.asarray(x, dtype=np.float32)))
    return m


def _host(m):
    return {k: v.cpu().numpy().astype(np.float64) for k, v in m.tables.items()}


def _moments(m):
    out = {}
    for k in m.tables:
        a, b = m.moments(k)
        out[k] = (a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64))
    return out


def _cuda(*xs):
    return [torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32)).cuda() for x in xs]


# ------------------------------------------------------------------------------------------- score
@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("dims", [(1, 1), (7, 33), (33, 7), (64, 64), (100, 100), (50, 100), (100, 50), (128, 128),
                                  (256, 256)])
def test_score_matches_fp64(l1, dims):
    dim_e, dim_r = dims
    E, R, B = 61, 7, 203
    m = _model(E, R, dim_e, dim_r, l1=l1, seed=dim_e + dim_r)
    rng = np.random.default_rng(dim_e * 1000 + dim_r)
    tri = RR.skewed_batch(rng, E, R, B)[0]
    got = m.score(*_cuda(tri)).cpu().numpy().astype(np.float64)
    tabs = _host(m)
    ref = RR.score(tabs, tri, l1)
    mag = RR.score_magnitude(tabs, tri, l1)
    tol = (2.0 if l1 else 4.0) * (dim_e + dim_r + 8) * F32_EPS * mag + 1e-30
    assert np.all(np.abs(got - ref) <= tol)


def test_score_bad_ids_are_nan():
    m = _model(10, 2, 8, 4)
    out = m.score(torch.tensor([[0, 1, 0], [0, 10, 0], [0, 1, 2], [-1, 1, 0]], dtype=torch.int32).cuda()).cpu().numpy()
    assert np.isfinite(out[0]) and np.isnan(out[1:]).all()


# ------------------------------------------------------------------------------------------- exact gradient
def _exact_case(name):
    """(tabs, pos, neg, margin, l1): integer fixtures whose every partial sum stays below 2^24."""
    rng = np.random.default_rng(len(name))
    if name == "skewed_l1":
        tabs = RR.integer_tables(300, 20, 33, 7, seed=1)
        pos, neg = RR.skewed_batch(rng, 300, 20, 3000)
        return tabs, pos, neg, 2.0, True
    if name == "skewed_l2_vec4":
        tabs = RR.integer_tables(300, 20, 8, 12, seed=2, amp=1)
        pos, neg = RR.skewed_batch(rng, 300, 20, 1000)
        return tabs, pos, neg, 3.0, False
    if name == "chunk_edges":
        # relation segments of 16, 17, 1, 32, 33, 15 pairs: whole chunks, one over, a lone pair, exact multiples
        counts = (16, 17, 1, 32, 33, 15)
        tabs = RR.integer_tables(40, len(counts), 12, 20, seed=3)
        r = rng.permutation(np.repeat(np.arange(len(counts)), counts))
        pos = np.stack([rng.integers(0, 40, len(r)), rng.integers(0, 40, len(r)), r], 1).astype(np.int32)
        neg = pos.copy()
        neg[:, 1] = rng.integers(0, 40, len(r))
        return tabs, pos, neg, 2.0, True
    if name == "one_relation_20000":
        tabs = RR.integer_tables(400, 3, 5, 6, seed=4, amp=1)
        pos, neg = RR.skewed_batch(rng, 400, 3, 20000, hot=1)
        return tabs, pos, neg, 1.0, True
    raise KeyError(name)


@pytest.mark.parametrize("name", ["skewed_l1", "skewed_l2_vec4", "chunk_edges", "one_relation_20000"])
def test_exact_gradient_bitwise(name):
    """b1 = 1/2, b2 = 3/4 at t = 1: m = g / 2 and (where |g| < 2^12) v = g^2 / 4 exactly, so the kernels' gradient
    must equal the fp64 one bitwise: dM sums over many chunks, entity runs of many slots, ties to the mask."""
    tabs, pos, neg, margin, l1 = _exact_case(name)
    assert RR.is_exact_step(tabs, pos, neg, margin, l1), "fixture leaves the exact range"
    E, R = len(tabs["ent"]), len(tabs["rel"])
    dim_e, dim_r = RR.dims(tabs)
    m = _model(E, R, dim_e, dim_r, l1=l1, tabs=tabs)
    loss = float(m.step(*_cuda(pos, neg), margin, lr=2.0 ** -6, b1=0.5, b2=0.75))
    rloss, g = RR.hinge_grads(tabs, pos, neg, margin, l1)
    assert loss == rloss
    mom = _moments(m)
    for k in tabs:
        mk, vk = mom[k]
        assert np.array_equal(mk, 0.5 * g[k]), k
        small = np.abs(g[k]) < 2.0 ** 12
        assert np.array_equal(vk[small], 0.25 * g[k][small] ** 2), k
        assert np.abs(g[k]).max() > 0, k


# ------------------------------------------------------------------------------------------- Adam at TF defaults
def test_twenty_dependent_adam_steps():
    """m, v against fp64 from the GPU's own previous state within a bound derived from each gradient's terms, and
    x recomputed from the GPU's m and v, on each of 20 dependent steps (t > 1, m, v != 0)."""
    rng = np.random.default_rng(7)
    E, R, dim_e, dim_r = 200, 10, 12, 8
    b1, b2, eps, lr = 0.9, 0.999, 1e-8, 0.01
    m = _model(E, R, dim_e, dim_r, l1=False, seed=3)
    for t in range(1, 21):
        tabs, mom = _host(m), _moments(m)
        pos, neg = RR.skewed_batch(rng, E, R, 300)
        m.step(*_cuda(pos, neg), 1.0, lr=lr)
        assert m.t == t
        _, g = RR.hinge_grads(tabs, pos, neg, 1.0, False)
        _, mag = RR.hinge_grads(tabs, pos, neg, 1.0, False, magnitude=True)
        new, nmom = _host(m), _moments(m)
        a = RR.lr_t(*(float(np.float32(x)) for x in (lr, b1, b2)), t)          # the fp32 arguments, in fp64
        for k in tabs:
            m0, v0 = mom[k]
            m1, v1 = nmom[k]
            tol_g = (dim_e + dim_r + 2 * len(pos)) * 2 * F32_EPS * mag[k]
            mref = np.float32(b1) * m0 + (1 - np.float32(b1)) * g[k]
            vref = np.float32(b2) * v0 + (1 - np.float32(b2)) * g[k] ** 2
            assert np.all(np.abs(m1 - mref) <= 0.1 * tol_g + 4 * F32_EPS * (np.abs(m0) + np.abs(g[k]))), (t, k)
            assert np.all(np.abs(v1 - vref) <= 0.001 * (2 * np.abs(g[k]) + tol_g) * tol_g
                          + 4 * F32_EPS * (np.abs(v0) + g[k] ** 2)), (t, k)
            xref = tabs[k] - a * m1 / (np.sqrt(v1) + eps)
            upd = a * np.abs(m1) / (np.sqrt(v1) + eps)
            assert np.all(np.abs(new[k] - xref) <= 4 * F32_EPS * (np.abs(xref) + upd)), (t, k)


def test_dense_decay():
    """A row touched at step 1 and not at step 2 still moves at step 2; a batch with no active pair still moves
    rows, decays m and advances t."""
    E, R = 20, 3
    m = _model(E, R, 8, 4, seed=1)
    x0 = _host(m)
    m.step(*_cuda([[0, 1, 0]], [[2, 1, 0]]), 100.0)
    x1, (m1, _) = _host(m), _moments(m)["ent"]
    assert not np.array_equal(x1["ent"][0], x0["ent"][0])
    assert np.array_equal(x1["ent"][5], x0["ent"][5])                          # m = 0 there: no move yet
    m.step(*_cuda([[5, 6, 1]], [[7, 6, 1]]), 100.0)
    x2, (m2, _) = _host(m), _moments(m)["ent"]
    assert not np.array_equal(x2["ent"][0], x1["ent"][0])
    assert np.array_equal(m2[0], (np.float32(0.9) * m1[0].astype(np.float32)).astype(np.float64))
    loss = float(m.step(*_cuda([[3, 4, 2]], [[3, 4, 2]]), -1e6))               # z = -1e6: inactive
    x3, (m3, _) = _host(m), _moments(m)["ent"]
    assert loss == 0.0 and m.t == 3
    assert not np.array_equal(x3["ent"][0], x2["ent"][0]) and not np.array_equal(x3["ent"][5], x2["ent"][5])
    assert np.array_equal(m3, (np.float32(0.9) * m2.astype(np.float32)).astype(np.float64))


def test_duplicates_are_summed_before_v():
    tabs = RR.integer_tables(6, 1, 4, 4, seed=1)
    pos, neg = np.array([[0, 1, 0], [0, 2, 0]]), np.array([[3, 1, 0], [0, 4, 0]])
    z = RR.zeros_like(tabs)
    _, _, vd, _ = RR.adam_step(tabs, z, z, pos, neg, 1000.0, 1, b1=0.5, b2=0.75, dedup=True)
    _, _, vs, _ = RR.adam_step(tabs, z, z, pos, neg, 1000.0, 1, b1=0.5, b2=0.75, dedup=False)
    m = _model(6, 1, 4, 4, tabs=tabs)
    m.step(*_cuda(pos, neg), 1000.0, b1=0.5, b2=0.75)
    mom = _moments(m)
    for k in tabs:
        assert np.array_equal(mom[k][1], vd[k]), k
        assert not np.array_equal(mom[k][1], vs[k]), k


def test_invalid_pairs_are_skipped():
    """Pairs with an id out of range or neg_r != pos_r change nothing: the step equals the one on the valid pairs
    alone, bitwise (their order, hence every sum's order, is kept)."""
    rng = np.random.default_rng(5)
    E, R = 100, 6
    pos, neg = RR.skewed_batch(rng, E, R, 400)
    bad = rng.choice(400, 60, replace=False)
    P, N = pos.copy(), neg.copy()
    P[bad[:20], 0] = E
    N[bad[20:40], 1] = -3
    N[bad[40:], 2] = (N[bad[40:], 2] + 1) % R
    keep = np.setdiff1d(np.arange(400), bad)
    a, b = _model(E, R, 16, 12, seed=2), _model(E, R, 16, 12, seed=2)
    la = float(a.step(*_cuda(P, N), 1.0))
    lb = float(b.step(*_cuda(pos[keep], neg[keep]), 1.0))
    assert abs(la - lb) <= 1e-6 * abs(lb)
    for k in a.tables:
        assert torch.equal(a.tables[k], b.tables[k]), k
    assert torch.equal(a.m, b.m) and torch.equal(a.v, b.v)


# ------------------------------------------------------------------------------------------- loop
def _kg(seed=0, E=300, R=12, T=3000):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, R + 1) ** 1.1
    tri = np.stack([rng.integers(0, E, T), rng.integers(0, E, T), rng.choice(R, T, p=w / w.sum())], 1)
    return np.unique(tri, axis=0).astype(np.int64), E, R


def test_reproducible_bitwise():
    tri, E, R = _kg()
    outs = []
    for _ in range(2):
        m = _model(E, R, 20, 24, seed=5)
        losses = m.trainer(tri, 900, margin=1.0, learning_rate=0.01, seed=9).run(5).cpu().numpy()
        outs.append((losses, _host(m), m.m.cpu().numpy(), m.v.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0])
    for k in outs[0][1]:
        assert np.array_equal(outs[0][1][k], outs[1][1][k]), k
    assert np.array_equal(outs[0][2], outs[1][2]) and np.array_equal(outs[0][3], outs[1][3])


def test_loop_equals_single_steps_and_draws_match():
    tri, E, R = _kg(1)
    B, n, seed = 700, 6, 21
    a, b = _model(E, R, 16, 12, seed=2), _model(E, R, 16, 12, seed=2)
    tr = a.trainer(tri, B, margin=1.0, learning_rate=0.01, seed=seed)
    la = tr.run(n).cpu().numpy()
    assert a.t == n
    idx = TO.BernoulliIndex(tri, 0, E, R)
    for s in range(n):
        pos, neg = tr.draw(s)
        p_, n_ = pos.cpu().numpy(), neg.cpu().numpy()
        assert np.array_equal(p_, tri[TR.draw_positive_rows(len(tri), B, seed, s)].astype(np.int32)), s
        assert np.array_equal(n_, TO.bernoulli_corrupt_batch(p_, idx, seed, s)), s
        lb = float(b.step(pos, neg, 1.0, lr=0.01))
        assert lb == la[s], s
    for k in a.tables:
        assert torch.equal(a.tables[k], b.tables[k]), k
    assert torch.equal(a.m, b.m) and torch.equal(a.v, b.v)


def test_state_dict_round_trip_resumes_bitwise():
    tri, E, R = _kg(2)
    a = _model(E, R, 12, 8, seed=1)
    tra = a.trainer(tri, 500, learning_rate=0.01, seed=4)
    tra.run(3)
    state = a.state_dict()
    tra.run(3)
    b = _model(E, R, 12, 8, seed=99)
    b.load_state_dict(state)
    assert b.t == 3
    trb = b.trainer(tri, 500, learning_rate=0.01, seed=4)
    trb.step_count = 3
    trb.run(3)
    for k in a.tables:
        assert torch.equal(a.tables[k], b.tables[k]), k
    assert torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and a.t == b.t == 6


def test_planted_kg_learns():
    """TransR at dim_e = dim_r = 32 with Adam on a planted translational KG (t = nearest entity to h + r in 16
    dims): held-out pairwise accuracy D(true) < D(corrupted) after training, against the untrained tables."""
    tri = TR.planted_kg(seed=0)
    E = 2000
    cut = int(0.9 * len(tri))
    train, held = tri[:cut], tri[cut:]
    rng = np.random.default_rng(1)
    corr = held.copy()
    side = rng.integers(0, 2, len(held))
    corr[np.arange(len(held)), side] = rng.integers(0, E, len(held))
    keep = ~np.all(corr == held, 1)
    held, corr = _cuda(held[keep], corr[keep])
    m = _model(E, 20, 32, 32, seed=0)
    acc = lambda: float((m.score(held) < m.score(corr)).float().mean())
    acc0 = acc()
    m.trainer(train, len(train) // 20, margin=1.0, learning_rate=0.01, seed=3).run(1500)
    acc1 = acc()
    print(f"planted KG held-out pairwise accuracy: untrained {acc0:.4f}, trained {acc1:.4f}")
    assert acc1 >= 0.85 and acc1 - acc0 >= 0.25
