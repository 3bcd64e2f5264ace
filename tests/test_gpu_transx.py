"""TransE / TransH / TransD on the MI355X through the C ABI (graphembeddings_amd.transx) against the fp64
restatement tests/transx_ref.py and the Bernoulli oracle."""
import numpy as np
import pytest
import torch

from oracle import transx_oracle as TO
from tests import transx_ref as TR

pytestmark = pytest.mark.gpu
MODELS = ("transe", "transh", "transd")


def _model(model, E, R, d, l1=True, seed=0):
    from graphembeddings_amd import transx as X
    return X.TransX(model, E, R, d, l1=l1, seed=seed)


def _host(m):
    return {k: v.cpu().numpy().astype(np.float64) for k, v in m.tables.items()}


def _pairs(rng, E, R, B):
    pos = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, R, B)], 1).astype(np.int32)
    neg = pos.copy()
    side = rng.integers(0, 2, B)
    neg[np.arange(B), side] = rng.integers(0, E, B)
    return pos, neg


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("d", [1, 37, 100, 128, 200, 1024])
def test_score_matches_fp64(model, l1, d):
    E, R, B = 61, 7, 203                                     # ragged B: not a multiple of any group count
    m = _model(model, E, R, d, l1=l1, seed=d)
    rng = np.random.default_rng(d)
    tri = _pairs(rng, E, R, B)[0]
    got = m.score(torch.as_tensor(tri).cuda()).cpu().numpy().astype(np.float64)
    ref = TR.score(model, _host(m), tri, l1)
    assert np.all(np.abs(got - ref) <= 1e-5 * np.abs(ref) + 1e-7)


def test_score_bad_ids_are_nan():
    m = _model("transe", 10, 2, 8)
    out = m.score(torch.tensor([[0, 1, 0], [0, 10, 0], [0, 1, 2]], dtype=torch.int32).cuda()).cpu().numpy()
    assert np.isfinite(out[0]) and np.isnan(out[1]) and np.isnan(out[2])


def _check_step(model, l1, E, R, d, pos, neg, lr, margin, tol=5e-6, seed=0):
    m = _model(model, E, R, d, l1=l1, seed=seed)
    before = _host(m)
    loss = float(m.step(torch.as_tensor(pos).cuda(), torch.as_tensor(neg).cuda(), lr, margin))
    new, rloss = TR.sgd_step(model, before, pos, neg, lr, margin, l1)
    assert abs(loss - rloss) <= tol * max(1.0, abs(rloss))
    after = _host(m)
    for k in new:
        assert np.abs(after[k] - new[k]).max() <= tol, k


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("d", [37, 100])
def test_one_step_matches_fp64(model, l1, d):
    rng = np.random.default_rng(11)
    pos, neg = _pairs(rng, 300, 9, 500)
    _check_step(model, l1, 300, 9, d, pos, neg, lr=0.01, margin=1.0)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("hot", ["relation", "head"])
def test_hot_rows(model, hot):
    """>= 1,000 slots on one row: the windowed two-level sum."""
    rng = np.random.default_rng(2)
    B = 1500
    pos, neg = _pairs(rng, 2000, 30, B)
    if hot == "relation":
        pos[:, 2] = neg[:, 2] = 4
    else:                                                    # every pair shares head 17; negatives corrupt the tail
        pos[:, 0] = neg[:, 0] = 17
        neg[:, 1] = rng.integers(0, 2000, B)
    _check_step(model, True, 2000, 30, 100, pos, neg, lr=0.001, margin=1.0)


@pytest.mark.parametrize("model", MODELS)
def test_twenty_dependent_steps(model):
    rng = np.random.default_rng(7)
    E, R, d = 400, 6, 64
    m = _model(model, E, R, d, l1=False, seed=3)
    ref = _host(m)
    for s in range(20):
        pos, neg = _pairs(rng, E, R, 256)
        loss = float(m.step(torch.as_tensor(pos).cuda(), torch.as_tensor(neg).cuda(), 0.01, 1.0))
        ref, rloss = TR.sgd_step(model, ref, pos, neg, 0.01, 1.0, False)
        assert abs(loss - rloss) <= 5e-6 * max(1.0, abs(rloss)), s
    got = _host(m)
    for k in ref:
        assert np.abs(got[k] - ref[k]).max() <= 5e-6, k


def _kg(seed=0, E=300, R=8, T=3000):
    rng = np.random.default_rng(seed)
    tri = np.stack([rng.integers(0, E, T), rng.integers(0, E, T), rng.integers(0, R, T)], 1)
    tri[:400, 2] = 0                                          # one busy relation
    return np.unique(tri, axis=0).astype(np.int64), E, R


@pytest.mark.parametrize("model", MODELS)
def test_reproducible_bitwise(model):
    tri, E, R = _kg()
    outs = []
    for _ in range(2):
        m = _model(model, E, R, 100, seed=5)
        losses = m.trainer(tri, 1200, margin=1.0, learning_rate=0.01, seed=9).run(5).cpu().numpy()
        outs.append((losses, _host(m)))
    assert np.array_equal(outs[0][0], outs[1][0])
    for k in outs[0][1]:
        assert np.array_equal(outs[0][1][k], outs[1][1][k]), k


@pytest.mark.parametrize("model", MODELS)
def test_loop_equals_single_steps_and_draws_match(model):
    tri, E, R = _kg(1)
    B, n, seed = 700, 6, 21
    a, b = _model(model, E, R, 48, seed=2), _model(model, E, R, 48, seed=2)
    tr = a.trainer(tri, B, margin=1.0, learning_rate=0.01, seed=seed)
    la = tr.run(n).cpu().numpy()
    idx = TO.BernoulliIndex(tri, 0, E, R)
    for s in range(n):
        pos, neg = tr.draw(s)
        p_, n_ = pos.cpu().numpy(), neg.cpu().numpy()
        assert np.array_equal(p_, tri[TR.draw_positive_rows(len(tri), B, seed, s)].astype(np.int32)), s
        assert np.array_equal(n_, TO.bernoulli_corrupt_batch(p_, idx, seed, s)), s
        assert np.array_equal(n_[:, 2], p_[:, 2])
        lb = float(b.step(pos, neg, 0.01, 1.0))
        assert lb == la[s], s
    for k in a.tables:
        assert torch.equal(a.tables[k], b.tables[k]), k


def test_state_dict_round_trip():
    m = _model("transd", 20, 3, 8, seed=1)
    m2 = _model("transd", 20, 3, 8, seed=2)
    m2.load_state_dict(m.state_dict())
    for k in m.tables:
        assert torch.equal(m.tables[k], m2.tables[k])


def test_planted_kg_learns():
    """TransE at d=32 on a planted translational KG (t = nearest entity to h + r in 16 dims): held-out pairwise
    accuracy D(true) < D(corrupted) after training, against the untrained table."""
    tri = TR.planted_kg(seed=0)
    E = 2000
    cut = int(0.9 * len(tri))
    train, held = tri[:cut], tri[cut:]
    rng = np.random.default_rng(1)
    corr = held.copy()
    side = rng.integers(0, 2, len(held))
    corr[np.arange(len(held)), side] = rng.integers(0, E, len(held))
    keep = ~np.all(corr == held, 1)
    held = torch.as_tensor(held[keep].astype(np.int32)).cuda()
    corr = torch.as_tensor(corr[keep].astype(np.int32)).cuda()
    m = _model("transe", E, 20, 32, seed=0)
    acc = lambda: float((m.score(held) < m.score(corr)).float().mean())
    acc0 = acc()
    m.trainer(train, len(train) // 20, margin=1.0, learning_rate=0.01, seed=3).run(3000)
    acc1 = acc()
    print(f"planted KG held-out pairwise accuracy: untrained {acc0:.4f}, trained {acc1:.4f}")
    assert acc1 >= 0.8 and acc1 - acc0 >= 0.25
