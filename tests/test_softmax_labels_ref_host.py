"""Host: the closed form of tests/softmax_labels_ref.py against torch.autograd in fp64 on the torch statement of the
multi-label objective (clip on lookup, ComplEx score, z = -scale * s, logsumexp minus the mean of the label logits, summed
over the rows), and against tests/softmax_ref.py where every row has exactly one label."""
import numpy as np
import pytest
import torch

from tests import softmax_labels_ref as LR
from tests import softmax_ref as SR
from tests.test_softmax_ref_host import case


def label_case(B, K, seed, one=False):
    """CSR labels: n_i from 1 up to min(K, 5) (`one`: 1 each), distinct positions per row except row 1, which names its
    first position twice; row 0 holds position 0, the last row position K - 1."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(B):
        n = 1 if one else 1 + i % min(K, 5)
        rows.append(list(rng.permutation(K)[:n]))
    rows[0][0], rows[-1][-1] = 0, K - 1
    if not one and B > 1:
        rows[1] = rows[1] + [rows[1][0]]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return off, np.concatenate(rows).astype(np.int64)


def torch_objective(table, hr, off, pos, cand, max_norm, scale, head):
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
    # the target distribution: y_ij / n_i
    y = torch.zeros(z.shape, dtype=torch.float64)
    for i in range(len(hr)):
        for p in pos[off[i]:off[i + 1]]:
            y[i, int(p)] += 1.0 / (off[i + 1] - off[i])
    loss = torch.logsumexp(z, 1) - (y * z).sum(1)
    loss.sum().backward()
    return loss.detach().numpy(), T.grad.numpy()


@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("B,K,d", [(5, 9, 8), (17, 40, 56)])
@pytest.mark.parametrize("max_norm,scale", [(1.0, 20.0), (4.0, 1.0)])
def test_closed_form_equals_autograd(B, K, d, head, max_norm, scale):
    table, hr, _, cand = case(B, K, d, 11 * B + d, max_norm)
    off, pos = label_case(B, K, B + K)
    L = len(pos)
    loss, idx, val = LR.evaluate(table, hr, off, pos, cand, max_norm, scale, head)
    tl, tg = torch_objective(table, hr, off, pos, cand, max_norm, scale, head)
    assert np.all(np.abs(loss - tl) <= 1e-11 * np.maximum(1.0, np.abs(tl)))
    dense = np.zeros_like(table)
    np.add.at(dense, idx, -val)                       # val = -1 * gradient, the slots of a row summed
    assert (idx >= 0).all() and len(idx) == K + 2 * B + L and np.array_equal(idx[K + 2 * B:], cand[pos])
    assert np.all(np.abs(dense - tg) <= 1e-11 * np.maximum(1.0, np.abs(tg).max()))
    # lr scales the values and nothing else
    half = LR.evaluate(table, hr, off, pos, cand, max_norm, scale, head, lr=0.5)
    assert np.array_equal(half[0], loss) and np.array_equal(half[2], 0.5 * val)


@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("B,K,d", [(5, 9, 8), (17, 40, 56)])
def test_one_label_is_the_one_vs_all_objective(B, K, d, head):
    """One label a row: the loss is softmax_ref.evaluate's bit for bit (the mean of one logit is the logit), the slots'
    ids are its ids, the query slots and the candidate slots with the label slots added are its gradients.  The
    gradients are the same numbers summed in another order -- there the label term goes through the matrix products with
    the softmax term, here it is added to their results -- so they agree to a few roundings of fp64 at the size of the
    largest entry (64 eps), not bitwise."""
    table, hr, _, cand = case(B, K, d, 11 * B + d, 1.0)
    off, pos = label_case(B, K, B + K, one=True)
    loss, idx, val = LR.evaluate(table, hr, off, pos, cand, 1.0, 20.0, head)
    l1, i1, v1 = SR.evaluate(table, hr, cand[pos], cand, 1.0, 20.0, head)
    assert np.array_equal(loss, l1)
    assert np.array_equal(idx[:K + 2 * B], i1) and np.array_equal(idx[K + 2 * B:], cand[pos])
    summed = val[:K + 2 * B].copy()
    np.add.at(summed, pos, val[K + 2 * B:])
    tol = 64 * np.finfo(np.float64).eps * np.abs(v1).max()
    assert 0 < tol < 1e-11 and np.abs(summed - v1).max() <= tol


def test_invalid_rows_and_bad_candidates():
    """Invalid rows of every kind -- a fixed or relation id outside the table, no labels, a label position outside [0, K),
    a label on an empty candidate slot, offsets that decrease or point past L -- are NaN with -1 slots and zero rows and
    leave the valid rows' figures bit for bit what they are without them; a candidate outside the table is an empty slot."""
    B, K, d = 4, 9, 8
    table, hr, _, cand = case(B, K, d, 3, 1.0)
    N = table.shape[0]
    off, pos = label_case(B, K, 5)
    pos = np.where(pos == K - 1, 0, pos)
    L = len(pos)
    good = LR.evaluate(table, hr, off, pos, cand[:-1], 1.0, 20.0, False)
    hr2 = np.concatenate([hr, [[N, 0], [cand[0], -1], [cand[0], 1], [cand[0], 1], [cand[0], 1], [cand[0], 1], [cand[0], 1]]])
    # rows B..: bad fixed, bad relation, no labels, position K, the empty slot K - 1, an offset past L, a decreasing offset
    pos2 = np.concatenate([pos, [1], [2], [K], [K - 1], [3, 4]])
    off2 = np.concatenate([off, [L + 1, L + 2, L + 2, L + 3, L + 4, L + 9, L + 6]])
    cand2 = cand.copy()
    cand2[-1] = N + 7
    loss, idx, val = LR.evaluate(table, hr2, off2, pos2, cand2, 1.0, 20.0, False)
    B2, L2 = len(hr2), len(pos2)
    assert np.isnan(loss[B:]).all() and np.array_equal(loss[:B], good[0])
    assert idx[K - 1] == -1 and not val[K - 1].any()
    assert np.array_equal(idx[:K - 1], good[1][:K - 1]) and np.array_equal(val[:K - 1], good[2][:K - 1])
    assert np.array_equal(val[K:K + 2 * B], good[2][K - 1:K - 1 + 2 * B])
    assert (idx[K + 2 * B:K + 2 * B2] == -1).all() and not val[K + 2 * B:K + 2 * B2].any()
    assert np.array_equal(val[K + 2 * B2:K + 2 * B2 + L], good[2][K - 1 + 2 * B:])
    assert (idx[K + 2 * B2 + L:] == -1).all() and not val[K + 2 * B2 + L:].any() and len(idx) == K + 2 * B2 + L2


def test_float32_evaluation_is_close_to_the_oracle():
    table, hr, _, cand = case(17, 40, 56, 5, 1.0)
    off, pos = label_case(17, 40, 1)
    t32 = table.astype(np.float32)
    l64, i64_, v64 = LR.evaluate(t32, hr, off, pos, cand, 1.0, 20.0, True)
    l32, i32_, v32 = LR.evaluate(t32, hr, off, pos, cand, 1.0, 20.0, True, dtype=np.float32)
    assert l32.dtype == np.float32 and v32.dtype == np.float32 and np.array_equal(i64_, i32_)
    assert 0 < np.abs(l32 - l64).max() < 1e-4 and 0 < np.abs(v32 - v64).max() < 1e-3


def test_step_sums_both_sides_before_the_update():
    table, hr, _, cand = case(8, 12, 8, 9, 1.0)
    hr[:, 0] = cand[np.arange(8) % 12]                # the fixed entities are candidates too
    off, pos = label_case(8, 12, 2)
    t, a = table.copy(), np.full_like(table, 0.1)
    loss, s, named = LR.step(t, a, (hr, off, pos), (hr[:3], off[:4], pos[:off[3]]), cand, 1.0, 20.0, 0.1)
    assert loss.shape == (11,) and named[cand].all() and named[hr[:, 1]].all()
    assert np.array_equal(t[~named], table[~named]) and np.allclose(a[named], 0.1 + s[named] ** 2)
    only_tail = LR.step(table.copy(), np.full_like(table, 0.1), (hr, off, pos), None, cand, 1.0, 20.0, 0.1)
    assert only_tail[0].shape == (8,) and np.array_equal(only_tail[0], loss[:8])
