"""Host: the NumPy restatement of RotatE (tests/rotate_ref.py) against torch.autograd in fp64, its rule at u = 0, its
rank rule, its optimizer steps against torch.optim, and its generator."""
import numpy as np
import pytest
import torch

from tests import rotate_ref as RR


def _tabs(rng, E, R, d):
    return {"ent": rng.normal(size=(E, d)) * 0.7, "rel": rng.uniform(-np.pi, np.pi, size=(R, d // 2))}


def _batch(rng, E, R, B):
    """Few entities and relations for B pairs: every row is named many times, heads and tails coincide in places."""
    pos = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, R, B)], 1)
    neg = pos.copy()
    neg[np.arange(B), rng.integers(0, 2, B)] = rng.integers(0, E, B)
    return pos, neg


def _torch_loss(P, pos, neg, margin, l1):
    """sum max(D(pos) - D(neg) + margin, 0) written with torch's complex numbers (not with rotate_ref's formulas)."""
    k = P["ent"].shape[1] // 2
    ent = torch.complex(P["ent"][:, :k], P["ent"][:, k:])

    def dist(tri):
        h, t, r = (torch.as_tensor(tri[:, c], dtype=torch.long) for c in range(3))
        u = ent[h] * torch.polar(torch.ones_like(P["rel"][r]), P["rel"][r]) - ent[t]
        m2 = u.real ** 2 + u.imag ** 2
        return torch.sqrt(m2).sum(1) if l1 else m2.sum(1)
    return torch.clamp(dist(pos) - dist(neg) + margin, min=0).sum()


@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_closed_form_gradients_equal_autograd(l1, seed):
    rng = np.random.default_rng(seed)
    E, R, d, B, margin = 12, 3, 10, 96, 0.5
    tabs = _tabs(rng, E, R, d)
    pos, neg = _batch(rng, E, R, B)
    assert len(np.unique(pos[:, :2])) < 2 * B and (pos[:, 0] == pos[:, 1]).any()       # duplicates; h == t somewhere
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in tabs.items()}
    loss = _torch_loss(P, pos, neg, margin, l1)
    loss.backward()
    rloss, grads, active = RR.hinge_grads(tabs, pos, neg, margin, l1)
    assert 0 < active.sum() < B                             # both branches of the hinge
    assert abs(float(loss.detach()) - rloss) <= 1e-10 * max(1.0, abs(rloss))
    for k in tabs:
        assert np.abs(P[k].grad.numpy() - grads[k]).max() <= 1e-10, k


@pytest.mark.parametrize("l1", [True, False])
def test_gradient_is_zero_where_u_is_zero(l1):
    """t = h o r in coordinate 0 (theta = 0 there, equal entries): m_0 = 0 and that coordinate's gradient is 0, not NaN."""
    rng = np.random.default_rng(5)
    tabs = _tabs(rng, 4, 2, 6)
    tabs["rel"][0, 0] = 0.0
    tabs["ent"][1, [0, 3]] = tabs["ent"][0, [0, 3]]
    tri = np.array([[0, 1, 0]])
    gh, gt, gr = RR.triple_grads(tabs, tri, l1)
    assert np.isfinite(gh).all() and np.isfinite(gt).all() and np.isfinite(gr).all()
    assert gh[0, 0] == 0 and gh[0, 3] == 0 and gt[0, 0] == 0 and gt[0, 3] == 0 and gr[0, 0] == 0
    assert (gh[0, [1, 2, 4, 5]] != 0).all()


@pytest.mark.parametrize("l1", [True, False])
def test_steps_equal_torch_optimizers(l1):
    rng = np.random.default_rng(9)
    E, R, d, B, lr, a0, margin = 30, 4, 8, 64, 0.05, 0.1, 0.3
    for opt_name in ("sgd", "adagrad"):
        tabs = _tabs(rng, E, R, d)
        accs = {k: np.full_like(v, a0) for k, v in tabs.items()}
        P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in tabs.items()}
        opt = (torch.optim.SGD(list(P.values()), lr=lr) if opt_name == "sgd"
               else torch.optim.Adagrad(list(P.values()), lr=lr, initial_accumulator_value=a0, eps=0))
        for step in range(3):
            pos, neg = _batch(rng, E, R, B)
            opt.zero_grad()
            _torch_loss(P, pos, neg, margin, l1).backward()
            opt.step()
            if opt_name == "sgd":
                tabs, _ = RR.sgd_step(tabs, pos, neg, lr, margin, l1)
            else:
                tabs, accs, _ = RR.adagrad_step(tabs, accs, pos, neg, lr, margin, l1)
            for k, p in P.items():
                assert np.abs(p.detach().numpy() - tabs[k]).max() <= 1e-10, (opt_name, step, k)
                if opt_name == "adagrad":
                    assert np.abs(opt.state[p]["sum"].numpy() - accs[k]).max() <= 1e-10, (step, k)


def test_rows_no_active_pair_names_keep_both_arrays():
    tabs = RR.exact_tables_l2(12, 3, 4, seed=1)
    tabs["ent"][4], tabs["ent"][1] = tabs["ent"][0], tabs["ent"][0] + 1.0      # pair 0: D- = 0 < D+ = 4, active
    accs = {k: np.full_like(v, 0.1) for k, v in tabs.items()}
    pos = np.array([[0, 1, 0], [2, 3, 1]])
    neg = np.array([[0, 4, 0], [2, 3, 1]])                  # pair 1: neg == pos, z = margin < 0: inactive
    new_t, new_a, _ = RR.adagrad_step(tabs, accs, pos, neg, 0.05, -0.5, False)
    act = RR.active_mask(tabs, pos, neg, -0.5, False)
    assert act[0] and not act[1]
    named = RR.named_rows(tabs, pos, neg, act)
    assert not named["ent"][[2, 3]].any() and not named["rel"][1] and named["ent"][[0, 1, 4]].all()
    for k in tabs:
        assert np.array_equal(new_t[k][~named[k]], tabs[k][~named[k]]) and np.array_equal(new_a[k][~named[k]], accs[k][~named[k]])


def test_head_side_query_gives_the_same_distance():
    rng = np.random.default_rng(2)
    tabs = _tabs(rng, 20, 3, 12)
    tri = _batch(rng, 20, 3, 40)[0]
    for l1 in (True, False):
        d = RR.dist(tabs, tri, l1)
        assert np.abs(RR.dist_head_form(tabs, tri, l1) - d).max() <= 1e-12 * max(1.0, d.max())
        for side in ("tail", "head"):
            nb, nk, td, sc = RR.ranks(tabs, tri, side, l1)
            assert np.abs(td - d).max() <= 1e-12 * max(1.0, d.max())
            assert (nk == 0).all() and sc.shape == (40, 20)


def test_rank_rule_on_ties():
    """The collinear fixture is full of exact ties: ascending (D, id), the target never before itself, known cells
    counted only where they rank before."""
    tabs = RR.collinear_tables(30, 2, 4, seed=0, amp=1)
    rng = np.random.default_rng(0)
    tri = _batch(rng, 30, 2, 50)[0]
    known = rng.random((50, 30)) < 0.3
    nb, nk, td, sc = RR.ranks(tabs, tri, "tail", True, known)
    assert np.array_equal(sc, np.round(sc)) and (sc % 5 == 0).all()
    ties = 0
    for i in range(50):
        order = sorted(range(30), key=lambda c: (sc[i, c], c))
        pos = order.index(tri[i, 1])
        assert nb[i] == pos and nk[i] == sum(known[i, c] for c in order[:pos])
        ties += int((sc[i] == td[i]).sum() > 1)
    assert ties >= 10


def test_generator_returns_unique_in_range_rows():
    tri = RR.planted_rotation_kg(n_ent=120, n_rel=10, k=4, n_triples=3000, seed=1, sym=3)
    assert tri.dtype == np.int64 and tri.ndim == 2 and tri.shape[1] == 3
    assert len(np.unique(tri, axis=0)) == len(tri) > 1000          # (at most a few rows per (h, r): 1,200 pairs)
    assert tri[:, :2].min() >= 0 and tri[:, :2].max() < 120 and tri[:, 2].min() >= 0 and tri[:, 2].max() < 10
    assert (tri[:, 0] != tri[:, 1]).all()                   # never h
    assert not np.array_equal(tri, np.unique(tri, axis=0))  # shuffled
    assert np.array_equal(tri, RR.planted_rotation_kg(n_ent=120, n_rel=10, k=4, n_triples=3000, seed=1, sym=3))
    # the first `sym` relations are symmetric: (h, t, r) mostly comes with (t, h, r) among those planted both ways
    rows = {tuple(x) for x in tri}
    sym = [x for x in tri if x[2] < 3]
    asym = [x for x in tri if x[2] >= 3]
    back = lambda xs: np.mean([(x[1], x[0], x[2]) in rows for x in xs])
    assert back(sym) > back(asym) + 0.05
