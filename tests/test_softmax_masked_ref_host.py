"""Host: the closed form of tests/softmax_masked_ref.py -- against torch.autograd in fp64 on the torch statement of the
type-constrained objective, against tests/softmax_ref.py with every bit set and on each set's compacted candidate list --
and the typed planted KG the GPU learning test trains on."""
import numpy as np
import pytest
import torch

from tests import softmax_masked_ref as MR
from tests import softmax_ref as SR
from tests.test_softmax_ref_host import case


def sets_for(K, B, seed):
    """(bool [4, K]: all / a random half / a block / position 0 and the tail end; row_set [B] cycling -1, 0, 1, 2, 3)."""
    rng = np.random.default_rng(seed)
    s = np.zeros((4, K), bool)
    s[0] = True
    s[1] = rng.random(K) < 0.5
    s[2, K // 4:K // 4 + max(1, K // 3)] = True
    s[3, 0] = s[3, K - max(1, K // 5):] = True
    return s, (np.arange(B) % 5) - 1


def draw_true(cand, sets, row_set, seed):
    rng = np.random.default_rng(seed)
    adm, _ = MR.admissible(row_set, sets)
    return np.array([cand[rng.choice(np.nonzero(a)[0])] for a in adm])


def torch_objective(table, hr, true, cand, max_norm, scale, head, adm):
    T = torch.tensor(table, dtype=torch.float64, requires_grad=True)

    def look(ids):
        x = T[torch.as_tensor(ids)]
        return x * torch.clamp(max_norm / x.norm(dim=1, keepdim=True), max=1.0)
    k = table.shape[1] // 2
    f, r, c = look(hr[:, 0]), look(hr[:, 1]), look(cand)
    cplx = lambda x: torch.complex(x[:, :k], x[:, k:])
    fc, rc, cc = cplx(f), cplx(r), cplx(c)
    if not head:
        s = ((fc * rc)[:, None, :] * cc.conj()[None, :, :]).real.sum(-1)
    else:
        s = (cc[None, :, :] * (rc * fc.conj())[:, None, :]).real.sum(-1)
    z = (-scale * s).masked_fill(~torch.as_tensor(adm), -float("inf"))
    col = torch.as_tensor([list(cand).index(t) for t in true])
    loss = torch.logsumexp(z, 1) - z[torch.arange(len(true)), col]
    loss.sum().backward()
    return loss.detach().numpy(), T.grad.numpy()


@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("B,K,d", [(5, 9, 8), (17, 40, 56)])
@pytest.mark.parametrize("max_norm,scale", [(1.0, 20.0), (4.0, 1.0)])
def test_closed_form_equals_autograd(B, K, d, head, max_norm, scale):
    table, hr, _, cand = case(B, K, d, 11 * B + d, max_norm)
    sets, rs = sets_for(K, B, B)
    true = draw_true(cand, sets, rs, K)
    loss, idx, val = MR.evaluate(table, hr, true, cand, max_norm, scale, head, rs, sets)
    adm, _ = MR.admissible(rs, sets)
    tl, tg = torch_objective(table, hr, true, cand, max_norm, scale, head, adm)
    assert np.isfinite(loss).all() and np.abs(loss - tl).max() <= 1e-10
    dense = np.zeros_like(table)
    np.add.at(dense, idx, -val)
    assert (idx >= 0).all() and len(idx) == K + 2 * B
    assert np.abs(dense - tg).max() <= 1e-10


@pytest.mark.parametrize("head", [False, True])
def test_all_bits_set_is_the_unmasked_objective(head):
    table, hr, true, cand = case(17, 40, 56, 7, 1.0)
    ref = SR.evaluate(table, hr, true, cand, 1.0, 20.0, head)
    for rs, sets in ((np.zeros(17, int), np.ones((1, 40), bool)), (np.full(17, -1), np.zeros((2, 40), bool))):
        got = MR.evaluate(table, hr, true, cand, 1.0, 20.0, head, rs, sets)
        assert np.array_equal(got[1], ref[1])
        assert np.abs(got[0] - ref[0]).max() <= 1e-12 and np.abs(got[2] - ref[2]).max() <= 1e-12
    g32 = MR.evaluate(table.astype(np.float32), hr, true, cand, 1.0, 20.0, head, np.full(17, -1), np.zeros((1, 40), bool),
                      dtype=np.float32)
    r32 = SR.evaluate(table.astype(np.float32), hr, true, cand, 1.0, 20.0, head, dtype=np.float32)
    assert g32[0].dtype == np.float32 and np.array_equal(g32[0], r32[0]) and np.array_equal(g32[2], r32[2])


@pytest.mark.parametrize("head", [False, True])
def test_each_set_is_the_unmasked_objective_on_its_compacted_list(head):
    B, K, d = 20, 40, 56
    table, hr, _, cand = case(B, K, d, 13, 1.0)
    sets, rs = sets_for(K, B, 3)
    rs = np.where(rs < 0, 0, rs)
    true = draw_true(cand, sets, rs, 5)
    loss, idx, val = MR.evaluate(table, hr, true, cand, 1.0, 20.0, head, rs, sets)
    dense = np.zeros_like(table)
    np.add.at(dense, idx, val)
    want = np.zeros_like(table)
    for s in range(len(sets)):
        rows = np.nonzero(rs == s)[0]
        l, i, v = SR.evaluate(table, hr[rows], true[rows], cand[sets[s]], 1.0, 20.0, head)
        assert np.abs(loss[rows] - l).max() <= 1e-12
        np.add.at(want, i, v)
    assert np.abs(dense - want).max() <= 1e-12


def test_invalid_rows():
    """An inadmissible true candidate, a set id outside [-1, n_sets), an empty set: NaN, -1 slots, zero rows, nothing in
    the candidates' gradients; a candidate no valid row admits keeps its id and has a zero row."""
    B, K, d = 6, 9, 8
    table, hr, _, cand = case(B, K, d, 3, 1.0)
    sets = np.zeros((3, K), bool)
    sets[0, :4], sets[1, 2:6] = True, True                 # set 2 is empty; positions 6.. are admitted by set -1 only
    rs = np.array([0, 1, 0, 3, -2, 2])
    true = cand[[0, 3, 5, 0, 0, 0]]                        # row 2: position 5 is not in set 0
    loss, idx, val = MR.evaluate(table, hr, true, cand, 1.0, 20.0, False, rs, sets)
    good = MR.evaluate(table, hr[:2], true[:2], cand, 1.0, 20.0, False, rs[:2], sets)
    assert np.isnan(loss[2:]).all() and np.array_equal(loss[:2], good[0])
    assert (idx[K + 4:] == -1).all() and not val[K + 4:].any()
    assert np.array_equal(idx[:K], cand) and np.array_equal(val[:K + 4], good[2])
    assert not val[6:K].any() and val[:6].any(1).all()


def test_step_leaves_unadmitted_candidates_alone():
    table, hr, _, cand = case(8, 12, 8, 9, 1.0)
    sets = np.zeros((3, 12), bool)
    sets[:, :8] = True
    tri = np.stack([cand[np.arange(8) % 8], cand[(np.arange(8) + 3) % 8], hr[:, 1]], 1)
    t, a = table.copy(), np.full_like(table, 0.1)
    loss, s, named = MR.step(t, a, tri, cand, 1.0, 20.0, 0.1, sets, sets)
    assert loss.shape == (8, 2) and np.isfinite(loss).all() and named[cand[:8]].all() and not named[cand[8:]].any()
    assert np.array_equal(t[~named], table[~named]) and np.allclose(a[named], 0.1 + s[named] ** 2)


def test_typed_planted_kg():
    train, test, tri, cand, sets, typ = MR.typed_setup()
    assert len(tri) == 3046 and len(train) == 2746 and len(test) == 300
    for side, col in (("tail", 1), ("head", 0)):
        assert sets[side].sum(1).mean() == 400
        assert sets[side][test[:, 2], test[:, col] - 8].all()          # every held-out row is admissible
        assert sets[side][train[:, 2], train[:, col] - 8].all()
    b = MR.batches(len(train), 512, 12)
    assert all(len(x) == 512 for x in b) and len(np.unique(np.concatenate(b[:5]))) == 5 * 512
    assert not np.array_equal(np.sort(b[5]), np.sort(b[0]))
