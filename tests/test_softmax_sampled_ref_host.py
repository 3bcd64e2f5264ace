"""Host: the closed form of tests/softmax_sampled_ref.py against torch.autograd in fp64 on the torch statement of the
sampled objective (clip on lookup, ComplEx score, z = -scale * s, the true entity's own logit, slots that hold the true
entity masked out, log of the sum minus the true logit, summed over the rows), and against tests/softmax_ref.py where the
two objectives coincide."""
import numpy as np
import pytest
import torch

from tests import softmax_ref as SR
from tests import softmax_sampled_ref as SS


def case(B, K, d, seed, max_norm):
    """Rows on both sides of the clip (odd table rows clipped), on each of the four operands.  Candidates are drawn with
    replacement from fewer ids than slots (duplicates); rows 0..2 have a true id that is a candidate (row 0: a duplicated
    one), the last rows a true id that is none."""
    rng = np.random.default_rng(seed)
    n_rel, n_ent = 3, K + 6
    N = n_rel + n_ent
    t = rng.standard_normal((N, d))
    norms = max_norm * np.exp(rng.normal(0.0, 0.3, N)) * np.where(np.arange(N) % 2, 1.8, 0.5)
    assert (np.abs(norms / max_norm - 1) > 0.01).all()
    t *= (norms / np.linalg.norm(t, axis=1))[:, None]
    cand = n_rel + rng.integers(0, K, K)                  # ids in [n_rel, n_rel + K): the last 6 entities are never drawn
    cand[:2] = cand[2]                                    # a triple for certain
    hr = np.stack([rng.integers(n_rel, N, B), rng.integers(0, n_rel, B)], 1)
    hr[:2, 1], hr[:2, 0] = [0, 1], [n_rel, n_rel + 1]
    true = n_rel + rng.integers(0, n_ent, B)
    true[0], true[1], true[2] = cand[2], cand[-1], cand[K // 2]
    true[-2:] = [N - 1, N - 2]
    return t, hr, true, cand.astype(np.int64)


def torch_objective(table, hr, true, cand, max_norm, scale, head):
    T = torch.tensor(table, dtype=torch.float64, requires_grad=True)

    def look(ids):
        x = T[torch.as_tensor(ids)]
        return x * torch.clamp(max_norm / x.norm(dim=1, keepdim=True), max=1.0)
    k = table.shape[1] // 2
    f, r, c, t = look(hr[:, 0]), look(hr[:, 1]), look(cand), look(true)
    cplx = lambda x: torch.complex(x[:, :k], x[:, k:])
    fc, rc, cc, tc = cplx(f), cplx(r), cplx(c), cplx(t)
    if not head:     # Re< h, r, conj(t) >, t the candidates
        s = ((fc * rc)[:, None, :] * cc.conj()[None, :, :]).real.sum(-1)
        st = (fc * rc * tc.conj()).real.sum(-1)
    else:            # h the candidates, t fixed
        s = (cc[None, :, :] * (rc * fc.conj())[:, None, :]).real.sum(-1)
        st = (tc * rc * fc.conj()).real.sum(-1)
    hit = torch.as_tensor(np.asarray(cand)[None, :] == np.asarray(true)[:, None])
    z = (-scale * s).masked_fill(hit, -float("inf"))
    zt = -scale * st
    loss = torch.logsumexp(torch.cat([z, zt[:, None]], 1), 1) - zt
    loss.sum().backward()
    return loss.detach().numpy(), T.grad.numpy()


@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("B,K,d", [(5, 9, 8), (17, 40, 56)])
@pytest.mark.parametrize("max_norm,scale", [(1.0, 20.0), (4.0, 1.0)])
def test_closed_form_equals_autograd(B, K, d, head, max_norm, scale):
    table, hr, true, cand = case(B, K, d, 11 * B + d, max_norm)
    assert len(np.unique(cand)) < K and np.isin(true, cand).any() and not np.isin(true, cand).all()
    nrm = np.linalg.norm(table, axis=1)
    for ids in (hr[:, 0], hr[:, 1], cand, true):
        assert (nrm[ids] > max_norm).any() and (nrm[ids] < max_norm).any()
    loss, idx, val = SS.evaluate(table, hr, true, cand, max_norm, scale, head)
    tl, tg = torch_objective(table, hr, true, cand, max_norm, scale, head)
    assert (loss >= 0).all() and np.all(np.abs(loss - tl) <= 1e-10 * np.maximum(1.0, np.abs(tl)))
    assert (idx >= 0).all() and len(idx) == K + 3 * B
    dense = -SS.merged(idx, val, table.shape[0])          # val = -1 * gradient, duplicates summed
    assert np.all(np.abs(dense - tg) <= 1e-10 * np.maximum(1.0, np.abs(tg).max()))


@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("max_norm,scale", [(1.0, 20.0), (4.0, 1.0)])
def test_distinct_candidates_holding_every_true_id_give_the_full_softmax(head, max_norm, scale):
    """Where `cand` is distinct and holds every true id the objective IS the 1-vs-all one: loss and per-row gradients
    equal tests/softmax_ref.evaluate's to 1e-12."""
    B, K, d = 17, 40, 56
    table, hr, _, _ = case(B, K, d, 7, max_norm)
    rng = np.random.default_rng(1)
    cand = 3 + rng.permutation(K)
    true = cand[rng.integers(0, K, B)]
    N = table.shape[0]
    l1, i1, v1 = SS.evaluate(table, hr, true, cand, max_norm, scale, head)
    l0, i0, v0 = SR.evaluate(table, hr, true, cand, max_norm, scale, head)
    assert np.abs(l1 - l0).max() <= 1e-12 * max(1.0, np.abs(l0).max())
    g1, g0 = SS.merged(i1, v1, N), SS.merged(i0, v0, N)
    assert np.abs(g1 - g0).max() <= 1e-12 * max(1.0, np.abs(g0).max())


def test_a_row_with_every_slot_excluded_has_loss_zero_exactly():
    table, hr, true, cand = case(6, 9, 8, 3, 1.0)
    N = table.shape[0]
    cand2 = np.where(np.arange(9) % 2 == 0, true[3], N + 5)          # row 3: its true id or an empty slot everywhere
    for dtype in (np.float64, np.float32):
        loss, idx, val = SS.evaluate(table, hr, true, cand2, 1.0, 20.0, False, dtype=dtype)
        assert loss[3] == 0.0 and not val[9 + 9:9 + 12].any() and (idx[9 + 9:9 + 12] >= 0).all()
        assert (np.delete(loss, np.nonzero(true == true[3])[0]) > 0).all()
        assert (idx[1:9:2] == -1).all() and not val[1:9:2].any()


def test_invalid_rows_and_float32():
    table, hr, true, cand = case(17, 40, 56, 5, 1.0)
    N = table.shape[0]
    hr2, true2 = hr.copy(), true.copy()
    hr2[4, 0], hr2[5, 1], true2[6] = N, -1, N + 3
    t32 = table.astype(np.float32)
    l64, i64_, v64 = SS.evaluate(t32, hr2, true2, cand, 1.0, 20.0, True)
    l32, i32_, v32 = SS.evaluate(t32, hr2, true2, cand, 1.0, 20.0, True, dtype=np.float32)
    assert l32.dtype == np.float32 and v32.dtype == np.float32 and np.array_equal(i64_, i32_)
    bad = np.array([4, 5, 6])
    assert np.isnan(l64[bad]).all() and np.isfinite(np.delete(l64, bad)).all()
    for i in bad:
        assert (i64_[40 + 3 * i:40 + 3 * i + 3] == -1).all() and not v64[40 + 3 * i:40 + 3 * i + 3].any()
    assert 0 < np.nanmax(np.abs(l32 - l64)) < 1e-4 and 0 < np.abs(v32 - v64).max() < 1e-3


def test_step_sums_both_sides_before_the_update():
    table, hr, true, cand = case(8, 12, 8, 9, 1.0)
    tri = np.stack([hr[:, 0], true, hr[:, 1]], 1)
    t, a = table.copy(), np.full_like(table, 0.1)
    loss, s, named = SS.step(t, a, tri, cand, 1.0, 20.0, 0.1)
    assert loss.shape == (8, 2) and named[cand].all() and named[tri.ravel()].all() and not named.all()
    assert np.array_equal(t[~named], table[~named]) and np.allclose(a[named], 0.1 + s[named] ** 2)
