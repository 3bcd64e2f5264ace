"""Host: the closed form of tests/softmax_ref.py against torch.autograd in fp64 on the torch statement of the 1-vs-all
objective (clip on lookup, ComplEx score, z = -scale * s, logsumexp minus the true logit, summed over the rows)."""
import numpy as np
import pytest
import torch

from tests import softmax_ref as SR


def case(B, K, d, seed, max_norm):
    """Rows on both sides of the clip (norms log-normal around max_norm, none within 1 % of it, none zero); every row's
    true id is a candidate; one relation shared, one entity fixed in several rows and a candidate."""
    rng = np.random.default_rng(seed)
    n_rel, N = 3, 3 + K + 4
    t = rng.standard_normal((N, d))
    norms = max_norm * np.exp(rng.normal(0.0, 0.3, N)) * np.where(np.arange(N) % 2, 1.8, 0.5)    # odd rows clipped
    assert (np.abs(norms / max_norm - 1) > 0.01).all()
    t *= (norms / np.linalg.norm(t, axis=1))[:, None]
    cand = (n_rel + rng.permutation(K)).astype(np.int64)
    hr = np.stack([rng.integers(n_rel, N, B), rng.integers(0, n_rel, B)], 1)
    hr[:3, 0], hr[3, 0] = cand[0], cand[0] ^ 1            # fixed rows on both sides of the clip, relations too
    hr[:2, 1] = [0, 1]
    true = cand[rng.integers(0, K, B)]
    true[0], true[-1] = cand[0], cand[K - 1]
    return t, hr, true, cand


def torch_objective(table, hr, true, cand, max_norm, scale, head):
    T = torch.tensor(table, dtype=torch.float64, requires_grad=True)

    def look(ids):
        x = T[torch.as_tensor(ids)]
        return x * torch.clamp(max_norm / x.norm(dim=1, keepdim=True), max=1.0)
    k = table.shape[1] // 2
    f, r, c = look(hr[:, 0]), look(hr[:, 1]), look(cand)
    cplx = lambda x: torch.complex(x[:, :k], x[:, k:])
    fc, rc, cc = cplx(f), cplx(r), cplx(c)
    if not head:     # Re< h, r, conj(t) >, t the candidates
        s = ((fc * rc)[:, None, :] * cc.conj()[None, :, :]).real.sum(-1)
    else:            # h the candidates, t fixed
        s = (cc[None, :, :] * (rc * fc.conj())[:, None, :]).real.sum(-1)
    z = -scale * s
    col = torch.as_tensor([list(cand).index(t) for t in true])
    loss = torch.logsumexp(z, 1) - z[torch.arange(len(true)), col]
    loss.sum().backward()
    return loss.detach().numpy(), T.grad.numpy()


@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("B,K,d", [(5, 9, 8), (17, 40, 56)])
@pytest.mark.parametrize("max_norm,scale", [(1.0, 20.0), (4.0, 1.0)])
def test_closed_form_equals_autograd(B, K, d, head, max_norm, scale):
    table, hr, true, cand = case(B, K, d, 11 * B + d, max_norm)
    loss, idx, val = SR.evaluate(table, hr, true, cand, max_norm, scale, head)
    # clips of both kinds on each of the three operands
    nrm = np.linalg.norm(table, axis=1)
    for ids in (hr[:, 0], hr[:, 1], cand):
        assert (nrm[ids] > max_norm).any() and (nrm[ids] < max_norm).any()
    tl, tg = torch_objective(table, hr, true, cand, max_norm, scale, head)
    assert np.all(np.abs(loss - tl) <= 1e-11 * np.maximum(1.0, np.abs(tl)))
    dense = np.zeros_like(table)
    np.add.at(dense, idx, -val)                       # val = -1 * gradient, duplicates summed
    assert (idx >= 0).all() and len(idx) == K + 2 * B
    assert np.all(np.abs(dense - tg) <= 1e-11 * np.maximum(1.0, np.abs(tg).max()))


def test_invalid_rows_and_bad_candidates():
    """A row with an id outside the table or a true id that is no candidate: NaN, -1 slots, zero rows, and nothing in the
    candidates' gradients; a candidate outside [0, N): an empty slot left out of every softmax."""
    B, K, d = 6, 9, 8
    table, hr, true, cand = case(B, K, d, 3, 1.0)
    N = table.shape[0]
    hr2, true2, cand2 = hr.copy(), true.copy(), cand.copy()
    hr2[2, 0], hr2[3, 1], true2[4], true2[5] = N, -1, N + 3, 1       # row 1 of the table is a relation: no candidate
    cand2[-1] = N + 7
    true2[:2] = np.where(true2[:2] == cand[-1], cand[0], true2[:2])
    good = SR.evaluate(table, hr2[:2], true2[:2], cand[:-1], 1.0, 20.0, False)
    loss, idx, val = SR.evaluate(table, hr2, true2, cand2, 1.0, 20.0, False)
    assert np.isnan(loss[2:]).all() and np.array_equal(loss[:2], good[0])
    assert (idx[K + 4:] == -1).all() and not val[K + 4:].any() and idx[K - 1] == -1 and not val[K - 1].any()
    assert np.array_equal(idx[:K - 1], good[1][:K - 1]) and np.array_equal(val[:K - 1], good[2][:K - 1])
    assert np.array_equal(val[K:K + 4], good[2][K - 1:])


def test_float32_evaluation_is_close_to_the_oracle():
    table, hr, true, cand = case(17, 40, 56, 5, 1.0)
    t32 = table.astype(np.float32)
    l64, i64_, v64 = SR.evaluate(t32, hr, true, cand, 1.0, 20.0, True)
    l32, i32_, v32 = SR.evaluate(t32, hr, true, cand, 1.0, 20.0, True, dtype=np.float32)
    assert l32.dtype == np.float32 and v32.dtype == np.float32 and np.array_equal(i64_, i32_)
    assert 0 < np.abs(l32 - l64).max() < 1e-4 and 0 < np.abs(v32 - v64).max() < 1e-3


def test_step_sums_both_sides_before_the_update():
    table, hr, true, cand = case(8, 12, 8, 9, 1.0)
    tri = np.stack([hr[:, 0], true, hr[:, 1]], 1)
    tri[:, 0] = cand[np.arange(8) % 12]               # heads are candidates too
    t, a = table.copy(), np.full_like(table, 0.1)
    loss, s, named = SR.step(t, a, tri, cand, 1.0, 20.0, 0.1)
    assert loss.shape == (8, 2) and named[cand].all() and named[tri[:, 2]].all()
    assert np.array_equal(t[~named], table[~named]) and np.allclose(a[named], 0.1 + s[named] ** 2)
