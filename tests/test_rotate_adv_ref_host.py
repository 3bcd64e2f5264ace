"""Host: tests/rotate_adv_ref.py, the restatement the GPU tests of RotatE's self-adversarial loss are held to, against
torch.autograd and against its own definition's special cases.  No GPU, no library call."""
import numpy as np
import torch

from oracle import transx_oracle as TO
from tests import rotate_adv_ref as AR

F32 = np.float32


def _tabs(E, R, d, seed=0, scale=0.5):
    rng = np.random.default_rng(seed)
    return {"ent": rng.normal(size=(E, d)) * scale, "rel": rng.uniform(-np.pi, np.pi, size=(R, d // 2))}


def _batch(rng, E, R, B, K):
    pos = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, R, B)], 1).astype(np.int32)
    side = rng.integers(0, 2, B).astype(np.int32)
    return pos, side, rng.integers(0, E, (B, K)).astype(np.int32)


def _torch_loss(ent, rel, pos, side, neg_ent, margin, alpha, l1):
    """sum_i loss_i with p detached, written independently of the restatement (complex tensors)."""
    k = ent.shape[1] // 2
    z = torch.complex(ent[:, :k], ent[:, k:])

    def dist(h, t, r):
        m = (z[h] * torch.polar(torch.ones_like(rel[r]), rel[r]) - z[t]).abs()
        return (m if l1 else m * m).sum(-1)
    pos, side, neg_ent = (torch.as_tensor(np.asarray(x, dtype=np.int64)) for x in (pos, side, neg_ent))
    h, t, r = pos[:, 0:1], pos[:, 1:2], pos[:, 2:3]
    nh = torch.where(side[:, None] == 0, h.expand_as(neg_ent), neg_ent)
    nt = torch.where(side[:, None] == 0, neg_ent, t.expand_as(neg_ent))
    Dp, Dn = dist(h[:, 0], t[:, 0], r[:, 0]), dist(nh, nt, r.expand_as(neg_ent))
    p = torch.softmax(-alpha * Dn, 1).detach()
    sp = torch.nn.functional.softplus
    return (sp(Dp - margin) + (p * sp(margin - Dn)).sum(1)).sum()


def test_gradients_match_autograd_with_detached_weights():
    E, R, d, B, K = 23, 4, 10, 9, 7
    rng = np.random.default_rng(1)
    for l1 in (True, False):
        for alpha in (0.0, 1.0, 5.0):
            tabs = _tabs(E, R, d, seed=int(alpha) + l1)
            pos, side, neg_ent = _batch(rng, E, R, B, K)
            neg_ent[0, 0] = pos[0, 1 if side[0] == 0 else 0]       # a slot that holds the true entity: an ordinary negative
            ent = torch.tensor(tabs["ent"], requires_grad=True)
            rel = torch.tensor(tabs["rel"], requires_grad=True)
            loss = _torch_loss(ent, rel, pos, side, neg_ent, 3.0, alpha, l1)
            loss.backward()
            want = float(loss.detach())
            for form in ("tail", "head"):
                got, g, named = AR.grads(tabs, pos, side, neg_ent, 3.0, alpha, l1, form=form)
                assert abs(got - want) < 1e-10 * max(1.0, abs(want))
                assert np.abs(g["ent"] - ent.grad.numpy()).max() < 1e-10
                assert np.abs(g["rel"] - rel.grad.numpy()).max() < 1e-10
            assert named["rel"][pos[:, 2]].all() and named["ent"][neg_ent].all()


def test_alpha_zero_is_uniform_and_one_negative_is_two_softplus():
    E, R, d = 17, 3, 8
    tabs = _tabs(E, R, d, 2)
    rng = np.random.default_rng(3)
    pos, side, neg_ent = _batch(rng, E, R, 11, 6)
    neg_ent[2, 1:4] = -1
    P = AR.parts(tabs, pos, side, neg_ent, 2.0, 0.0)
    n = P["live"].sum(1)
    assert n[2] == 3 and np.allclose(P["p"][P["live"]], (1.0 / n)[:, None].repeat(6, 1)[P["live"]], rtol=0, atol=1e-15)
    pos, side, neg_ent = _batch(rng, E, R, 11, 1)
    for alpha in (0.0, 1.0, 5.0):
        P = AR.parts(tabs, pos, side, neg_ent, 2.0, alpha)
        want = AR.softplus(P["Dp"] - 2.0) + AR.softplus(2.0 - P["Dn"][:, 0])
        assert np.abs(P["loss"] - want).max() < 1e-14
    # softplus and sigma as the contract writes them
    x = np.linspace(-30, 30, 241)
    assert np.abs(AR.softplus(x) - np.log1p(np.exp(x))).max() < 1e-12 and np.abs(AR.sigmoid(x) - 1 / (1 + np.exp(-x))).max() < 1e-15


def test_empty_slots_all_empty_rows_and_invalid_rows():
    E, R, d, B, K = 12, 3, 6, 6, 5
    tabs = _tabs(E, R, d, 4)
    rng = np.random.default_rng(5)
    pos, side, neg_ent = _batch(rng, E, R, B, K)
    neg_ent[0, [1, 3]] = (-1, E)                         # two empty slots
    neg_ent[1, :] = (-1, E, -7, E + 5, -1)               # every slot empty: the positive term alone
    side[2] = 2                                          # invalid rows
    pos[3, 0] = E
    pos[4, 2] = -1
    P = AR.parts(tabs, pos, side, neg_ent, 1.5, 1.0)
    assert np.array_equal(P["valid"], [True, True, False, False, False, True])
    assert np.array_equal(np.isnan(P["loss"]), ~P["valid"])
    assert P["loss"][1] == AR.softplus(P["Dp"][1] - 1.5)
    # the row with two empty slots equals the row with those slots removed
    keep = [0, 2, 4]
    Q = AR.parts(tabs, pos[:1], side[:1], neg_ent[:1, keep], 1.5, 1.0)
    assert abs(P["loss"][0] - Q["loss"][0]) < 1e-14
    loss, g, named = AR.grads(tabs, pos, side, neg_ent, 1.5, 1.0)
    assert abs(loss - P["loss"][P["valid"]].sum()) < 1e-12
    ok = [0, 1, 5]
    loss2, g2, named2 = AR.grads(tabs, pos[ok], side[ok], neg_ent[ok], 1.5, 1.0)
    assert loss == loss2 and all(np.array_equal(g[k], g2[k]) and np.array_equal(named[k], named2[k]) for k in g)
    nr = AR.named_rows(tabs, pos, side, neg_ent)
    assert all(np.array_equal(nr[k], named[k]) for k in nr)
    # an invalid row names nothing; an all-empty row names its positive and relation
    only = AR.named_rows(tabs, pos[1:3], side[1:3], neg_ent[1:3])
    assert only["ent"].sum() == len({pos[1, 0], pos[1, 1]}) and only["rel"].sum() == 1


def test_no_inf_or_nan_far_from_the_margin():
    """|D - gamma| up to 1e3 in both directions, in fp32 as well as fp64: losses, weights and gradients stay finite."""
    E, R, d, B, K = 9, 2, 4, 8, 6
    rng = np.random.default_rng(6)
    pos, side, neg_ent = _batch(rng, E, R, B, K)
    for dtype in (np.float64, F32):
        for scale, margin in ((200.0, 0.0), (0.01, 1e3), (200.0, 1e3), (100.0, -1e3)):
            tabs = _tabs(E, R, d, 7, scale=scale)
            for l1 in (True, False):
                for alpha in (0.0, 1.0, 5.0):
                    P = AR.parts(tabs, pos, side, neg_ent, margin, alpha, l1, dtype)
                    assert np.isfinite(P["loss"]).all() and np.isfinite(P["p"]).all()
                    assert np.abs(P["p"].sum(1) - 1).max() < 1e-5
                    loss, g, _ = AR.grads(tabs, pos, side, neg_ent, margin, alpha, l1, dtype)
                    assert np.isfinite(loss) and all(np.isfinite(v).all() for v in g.values())
    tabs = _tabs(E, R, d, 7, scale=200.0)
    assert np.abs(AR.parts(tabs, pos, side, neg_ent, 0.0, 1.0)["Dn"]).max() > 1e3


def test_steps_move_only_named_rows():
    E, R, d, B, K = 40, 5, 8, 6, 3
    tabs = _tabs(E, R, d, 8)
    pos, side, neg_ent = _batch(np.random.default_rng(9), E, R, B, K)
    named = AR.named_rows(tabs, pos, side, neg_ent)
    new, loss = AR.sgd_step(tabs, pos, side, neg_ent, 0.1, 2.0, 1.0)
    accs = {k: np.full(v.shape, 0.1) for k, v in tabs.items()}
    new_a, acc_a, loss_a = AR.adagrad_step(tabs, accs, pos, side, neg_ent, 0.1, 2.0, 1.0)
    assert loss == loss_a > 0
    for k in tabs:
        assert np.array_equal(new[k][~named[k]], tabs[k][~named[k]]) and (new[k][named[k]] != tabs[k][named[k]]).any()
        assert np.array_equal(new_a[k][~named[k]], tabs[k][~named[k]]) and np.array_equal(acc_a[k][~named[k]], accs[k][~named[k]])
        assert (acc_a[k][named[k]] >= 0.1).all()


def _kg(seed, E, R, T):
    rng = np.random.default_rng(seed)
    return np.unique(np.stack([rng.integers(0, E, T), rng.integers(0, E, T), rng.integers(0, R, T)], 1), axis=0)


def test_draw_never_returns_a_known_completion_and_keeps_the_hinge_loops_rows():
    from tests import transx_ref as XR
    E, R = 30, 3
    tri = _kg(0, E, R, 900)                              # dense: about ten known completions per key
    idx = TO.BernoulliIndex(tri, 0, E, R)
    have = {tuple(x) for x in tri.tolist()}
    sides = set()
    for step in (0, 5):
        pos, side, neg_ent = AR.draw(tri, idx, 11, step, 64, 9)
        assert np.array_equal(pos, tri[XR.draw_positive_rows(len(tri), 64, 11, step)])
        hinge_neg = TO.bernoulli_corrupt_batch(pos, idx, 11, step)
        assert np.array_equal(side, (hinge_neg[:, 0] != pos[:, 0]).astype(np.int32))      # the replaced column
        assert neg_ent.min() >= 0 and neg_ent.max() < E
        for i in range(64):
            h, t, r = pos[i].tolist()
            for c in neg_ent[i].tolist():
                assert ((h, c, r) if side[i] == 0 else (c, t, r)) not in have
        sides |= set(side.tolist())
        assert len({tuple(x) for x in neg_ent.tolist()}) > 32          # the K picks of a row are their own draws
    assert sides == {0, 1}
    again = AR.draw(tri, idx, 11, 5, 64, 9)
    assert all(np.array_equal(a, b) for a, b in zip((pos, side, neg_ent), again))


def test_draw_gives_minus_one_where_no_entity_is_free():
    """Three entities; (0, r=0) has every entity as a known tail and (., 2, r=0)... every head: no free entity on either
    side of (0, 2, 0)."""
    E, R = 3, 2
    tri = np.array([[0, 0, 0], [0, 1, 0], [0, 2, 0], [1, 2, 0], [2, 2, 0], [1, 0, 1]])
    idx = TO.BernoulliIndex(tri, 0, E, R)
    pos, side, neg_ent = AR.draw(tri, idx, 3, 0, 200, 4)
    full = (pos[:, 0] == 0) & (pos[:, 1] == 2) & (pos[:, 2] == 0)
    tails_full = (pos[:, 0] == 0) & (pos[:, 2] == 0) & (side == 0)
    heads_full = (pos[:, 1] == 2) & (pos[:, 2] == 0) & (side == 1)
    none_free = tails_full | heads_full
    assert full.any() and none_free[full].all() and (~none_free).any()
    assert (neg_ent[none_free] == -1).all() and (neg_ent[~none_free] >= 0).all()
