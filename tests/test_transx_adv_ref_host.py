"""Host: the restatement tests/transx_adv_ref.py against torch.autograd, the special cases of the loss's definition, and
the L1 sign-stability condition of every L1 case the GPU files build."""
import numpy as np
import pytest
import torch

from tests import transx_adv_ref as AR
from tests import transx_ref as XR

MODELS = AR.MODELS


def _torch_loss(model, tabs, pos, side, neg_ent, margin, alpha, l1):
    """sum_i softplus(D+ - gamma) + sum_j p_ij.detach() softplus(gamma - D-_ij) on torch fp64 leaves (all rows valid, all
    slots live)."""
    T = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in tabs.items()}

    def proj(e_id, r_id):
        e = T["ent"][e_id]
        if model == "transe":
            return e
        if model == "transh":
            n = T["normal_vector"][r_id]
            nh = n / torch.sqrt(torch.clamp((n * n).sum(-1, keepdim=True), min=XR.EPS))
            return e - (e * nh).sum(-1, keepdim=True) * nh
        return e + (e * T["ent_transfer"][e_id]).sum(-1, keepdim=True) * T["rel_transfer"][r_id]

    def dist(h, t, r):
        u = proj(h, r) + T["rel"][r] - proj(t, r)
        return u.abs().sum(-1) if l1 else (u * u).sum(-1)

    pos, side, neg_ent = (torch.as_tensor(np.asarray(x, dtype=np.int64)) for x in (pos, side, neg_ent))
    B, K = neg_ent.shape
    h, t, r = pos[:, 0], pos[:, 1], pos[:, 2]
    tails = (side == 0)[:, None]
    nh = torch.where(tails, h[:, None].expand(B, K), neg_ent)
    nt = torch.where(tails, neg_ent, t[:, None].expand(B, K))
    Dp, Dn = dist(h, t, r), dist(nh, nt, r[:, None].expand(B, K))
    p = torch.softmax(-alpha * Dn, 1).detach()
    sp = torch.nn.functional.softplus
    loss = (sp(Dp - margin) + (p * sp(margin - Dn)).sum(1)).sum()
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in T.items()}


def _dup_batch(rng, E, R, B, K):
    """Duplicate entities and relations, both sides: few ids, so that rows share them."""
    pos, side, neg_ent = AR.batch(rng, E, R, B, K)
    pos[1] = pos[0]                                      # the same positive twice, on different sides
    neg_ent[2, :2] = pos[2, :2]                          # a slot holding the true entity, one holding the fixed one
    return pos, side, neg_ent


@pytest.mark.parametrize("alpha", [0.0, 1.0, 5.0])
@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("model", MODELS)
def test_gradients_match_autograd(model, l1, alpha):
    E, R, d, B, K = 9, 2, 6, 12, 7
    tabs = AR.tables(model, E, R, d, seed=3)
    pos, side, neg_ent = _dup_batch(np.random.default_rng(5), E, R, B, K)
    assert set(side.tolist()) == {0, 1} and len(np.unique(pos[:, 2])) < B
    loss, g, named = AR.grads(model, tabs, pos, side, neg_ent, 2.0, alpha, l1)
    tl, tg = _torch_loss(model, tabs, pos, side, neg_ent, 2.0, alpha, l1)
    assert abs(loss - tl) <= 1e-10 * max(1.0, abs(tl))
    assert set(g) == set(tabs)
    for k in tabs:
        assert np.abs(g[k] - tg[k]).max() <= 1e-10, (k, float(np.abs(g[k] - tg[k]).max()))
        assert np.all(tg[k][~named[k]] == 0), k
    # the kernel's order of evaluation is the same function
    loss_f, g_f, _ = AR.grads(model, tabs, pos, side, neg_ent, 2.0, alpha, l1, form="fixed")
    assert abs(loss_f - loss) <= 1e-10 and all(np.abs(g_f[k] - g[k]).max() <= 1e-10 for k in g)


@pytest.mark.parametrize("model", MODELS)
def test_steps_apply_the_gradients(model):
    E, R, d = 9, 2, 5
    tabs = AR.tables(model, E, R, d, seed=1)
    pos, side, neg_ent = AR.batch(np.random.default_rng(2), E - 2, R, 4, 3)
    loss, g, named = AR.grads(model, tabs, pos, side, neg_ent, 1.5, 1.0)
    new, l2 = AR.sgd_step(model, tabs, pos, side, neg_ent, 0.1, 1.5, 1.0)
    accs = {k: np.full(v.shape, 0.1) for k, v in tabs.items()}
    nt, na, l3 = AR.adagrad_step(model, tabs, accs, pos, side, neg_ent, 0.1, 1.5, 1.0)
    assert loss == l2 == l3
    also = AR.named_rows(model, tabs, pos, side, neg_ent)
    assert set(named) == set(also) == set(tabs) and all(np.array_equal(named[k], also[k]) for k in named)
    for k in tabs:
        assert np.allclose(new[k], tabs[k] - 0.1 * g[k], rtol=0, atol=1e-15)
        rows = named[k]
        assert rows.any() and (len(rows) != E or not rows[-2:].any())       # the batch names entities below E - 2
        assert np.array_equal(nt[k][~rows], tabs[k][~rows]) and np.array_equal(na[k][~rows], accs[k][~rows])
        assert np.allclose(na[k][rows], 0.1 + g[k][rows] ** 2, rtol=0, atol=1e-15)
        assert np.allclose(nt[k][rows], tabs[k][rows] - 0.1 * g[k][rows] / np.sqrt(0.1 + g[k][rows] ** 2), rtol=0, atol=1e-15)


@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("model", MODELS)
def test_special_cases_of_the_definition(model, l1):
    E, R, d = 12, 3, 6
    tabs = AR.tables(model, E, R, d, seed=2)
    pos, side, neg_ent = AR.batch(np.random.default_rng(3), E, R, 5, 6)
    f = lambda ne, alpha, **kw: AR.row_losses(model, tabs, pos, side, ne, 2.0, alpha, l1, **kw)
    # K = 1: alpha does not matter
    assert np.array_equal(f(neg_ent[:, :1], 0.0), f(neg_ent[:, :1], 5.0))
    # alpha = 0: the uniform mean of the negatives' terms
    P = AR.parts(model, tabs, pos, side, neg_ent, 2.0, 0.0, l1)
    assert np.allclose(P["p"], 1 / 6) and np.allclose(P["loss"], AR.softplus(P["Dp"] - 2.0) + AR.softplus(2.0 - P["Dn"]).mean(1))
    # an empty slot equals the row without it, -1 and E alike
    holed = neg_ent.copy()
    holed[:, 2], holed[:, 4] = -1, E
    assert np.allclose(f(holed, 1.0), f(neg_ent[:, [0, 1, 3, 5]], 1.0), rtol=0, atol=1e-14)
    g_h = AR.grads(model, tabs, pos, side, holed, 2.0, 1.0, l1)[1]
    g_w = AR.grads(model, tabs, pos, side, neg_ent[:, [0, 1, 3, 5]], 2.0, 1.0, l1)[1]
    assert all(np.allclose(g_h[k], g_w[k], rtol=0, atol=1e-13) for k in g_h)
    # every slot empty: the positive term alone
    none = np.full_like(neg_ent, -1)
    assert np.allclose(f(none, 1.0), AR.softplus(P["Dp"] - 2.0), rtol=0, atol=1e-14)
    # 64 equal negatives equal the K = 1 row
    for alpha in (0.0, 1.0, 5.0):
        assert np.allclose(f(np.repeat(neg_ent[:, :1], 64, 1), alpha), f(neg_ent[:, :1], alpha), rtol=0, atol=1e-13)
    # invalid rows: NaN, no gradient, 0 in the sum
    bad_pos, bad_side = pos.copy(), side.copy()
    bad_pos[0, 0], bad_pos[1, 2], bad_side[2] = E, -1, 2
    L = AR.row_losses(model, tabs, bad_pos, bad_side, neg_ent, 2.0, 1.0, l1)
    assert np.array_equal(np.isnan(L), [True, True, True, False, False])
    loss, g, named = AR.grads(model, tabs, bad_pos, bad_side, neg_ent, 2.0, 1.0, l1)
    l34, g34, _ = AR.grads(model, tabs, pos[3:], side[3:], neg_ent[3:], 2.0, 1.0, l1)
    assert abs(loss - l34) <= 1e-14 and all(np.allclose(g[k], g34[k], rtol=0, atol=1e-14) for k in g)
    # fp32 runs the same statements in float32
    assert f(neg_ent, 1.0, dtype=np.float32).dtype == np.float32
    assert np.abs(f(neg_ent, 1.0, dtype=np.float32, form="fixed") - f(neg_ent, 1.0)).max() < 1e-4


def test_sign_margin_sees_a_residual_at_zero():
    tabs = AR.tables("transe", 6, 2, 4, seed=0)
    pos, side, neg_ent = AR.batch(np.random.default_rng(0), 6, 2, 2, 3)
    assert AR.sign_stable("transe", tabs, pos, side, neg_ent)
    h, t, r = pos[0]
    tabs["rel"][r, 1] = tabs["ent"][t, 1] - tabs["ent"][h, 1]           # u = 0 at one coordinate of the first positive
    assert not AR.sign_stable("transe", tabs, pos, side, neg_ent)


# ------------------------------------------------------------------------------------------ the GPU files' L1 cases
@pytest.mark.parametrize("d,shift", AR.SHAPES)
@pytest.mark.parametrize("model", MODELS)
def test_l1_step_cases_are_sign_stable(model, d, shift):
    """Every L1 case of test_loss_rows_and_one_step_match_the_restatement: build_case finds a seed among SEEDS at which
    every residual coordinate of every live triple has |u_fp64| > 32 |u_fp32 - u_fp64| (it raises otherwise), with the
    shape's own B, d and K.  SGD and AdaGrad share their cases' batches."""
    seen = set()
    for opt in ("sgd", "adagrad"):
        for K, B, alpha, seed0 in AR.step_cases(model, True, opt, d, shift):
            if (K, B, seed0) in seen:
                continue
            seen.add((K, B, seed0))
            c = AR.step_case(model, True, d, K, B, seed0)
            assert seed0 <= c["seed"] < seed0 + AR.SEEDS
            assert AR.sign_margin(model, c["tabs"], c["pos"], c["side"], c["neg_ent"]) > 0
            assert c["pos"].shape == (B, 3) and c["neg_ent"].shape == (B, K)
            if B >= 2:
                assert set(c["side"][:2].tolist()) == {0, 1}
    assert {K for K, _, _ in seen} == set(AR.ks(d, shift))


def test_the_k_lists_cross_every_team_count_and_edge():
    assert {AR.n_teams(d, s) for d, s in AR.SHAPES} == {32, 16, 8, 4}
    assert [AR.n_teams(d, s) for d, s in AR.SHAPES] == [32, 32, 32, 8, 32, 16, 8, 8, 4, 4, 4, 4]
    for d, s in AR.SHAPES:
        nt, K = AR.n_teams(d, s), AR.ks(d, s)
        assert {1, 2, nt, nt + 1, nt // 4 + 1, 64, 65} <= set(K) and (nt - 1 in K)
        if d < AR.LARGE_D:
            assert {63, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1024} <= set(K)


@pytest.mark.parametrize("model", MODELS)
def test_other_l1_cases_are_sign_stable(model):
    """The remaining L1 cases of the GPU files, through the same builders."""
    for name, c in AR.other_cases(model, True).items():
        assert AR.sign_margin(model, c["tabs"], c["pos"], c["side"], c["neg_ent"]) > 0, name
    norms = set()
    for name, (l1, c) in AR.guard_cases(model).items():     # the guard file's
        norms.add((name.split()[0], l1))
        if l1:
            assert AR.sign_margin(model, c["tabs"], c["pos"], c["side"], c["neg_ent"]) > 0, name
    assert norms == {("loss", True), ("loss", False), ("step", True), ("step", False)}
