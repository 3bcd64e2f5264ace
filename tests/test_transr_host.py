"""CPU checks of the TransR layer: the fp64 restatement against torch autograd and torch.optim.Adam, the dedup
choice, the driver's flags, and argument errors raised before any GPU call."""
import numpy as np
import pytest
import torch

from graphembeddings_amd import transr as XR
from graphembeddings_amd import transr_train as XRT
from tests import transr_ref as RR


def _autograd(tabs, pos, neg, margin, l1):
    """The reference's graph in torch fp64: batch matmul of M_r on h and on t, TF's tie rules as torch.where."""
    T = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in tabs.items()}
    dim_e, dim_r = T["ent"].shape[1], T["rel"].shape[1]
    pos, neg = torch.as_tensor(pos), torch.as_tensor(neg)
    Mt = T["rel_matrix"][neg[:, 2]].reshape(-1, dim_r, dim_e)              # transR.py:55 looks up neg_r

    def D(tr):
        h = torch.bmm(Mt, T["ent"][tr[:, 0]].unsqueeze(2)).squeeze(2)
        t = torch.bmm(Mt, T["ent"][tr[:, 1]].unsqueeze(2)).squeeze(2)
        u = h + T["rel"][tr[:, 2]] - t
        return u.abs().sum(1) if l1 else (u * u).sum(1)

    z = D(pos) - D(neg) + margin
    loss = torch.where(z >= 0, z, torch.zeros_like(z)).sum()
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in T.items()}


@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("dims", [(7, 5), (4, 9), (6, 6)])
def test_ref_gradients_match_autograd(l1, dims):
    dim_e, dim_r = dims
    rng = np.random.default_rng(3)
    E, R, B = 12, 3, 40
    tabs = RR.random_tables(E, R, dim_e, dim_r, rng)
    pos, neg = RR.skewed_batch(rng, E, R, B)
    neg[5] = pos[5]                                             # identical pair: z = margin
    loss, g = RR.hinge_grads(tabs, pos, neg, 1.0, l1)
    aloss, ag = _autograd(tabs, pos, neg, 1.0, l1)
    assert abs(loss - aloss) <= 1e-12 * max(1.0, abs(aloss))
    for k in tabs:
        assert np.abs(g[k] - ag[k]).max() <= 1e-12 * max(1.0, np.abs(ag[k]).max()), k


def test_ref_tie_is_active_and_sign_of_zero():
    """z == 0 exactly takes a gradient; a zero component of u takes sign 0 (integer tables make both exact)."""
    tabs = RR.integer_tables(6, 1, 3, 2, seed=4)
    pos, neg = np.array([[0, 1, 0]]), np.array([[2, 3, 0]])
    margin = float(RR.score(tabs, neg)[0] - RR.score(tabs, pos)[0])
    loss, g = RR.hinge_grads(tabs, pos, neg, margin, True)
    assert loss == 0.0 and np.abs(g["rel"]).max() > 0
    aloss, ag = _autograd(tabs, pos, neg, margin, True)
    assert all(np.array_equal(g[k], ag[k]) for k in tabs)
    self_loop = np.array([[0, 0, 0]])                           # u = r: set r's first component to 0
    tabs["rel"][0, 0] = 0.0
    _, sl = RR.slices(tabs, self_loop, np.array([[1, 2, 0]]), 100.0, True)
    assert sl["rel"][1][0][0] == 0.0


def test_adam_restatement_matches_torch_adam_at_eps0():
    """With eps = 0 TF1's lr_t form and torch's bias-corrected form are the same update; every element has a
    gradient at every step, so this pins where the bias correction goes."""
    rng = np.random.default_rng(8)
    tabs = RR.random_tables(5, 2, 3, 4, rng)
    m, v = RR.zeros_like(tabs), RR.zeros_like(tabs)
    P = {k: torch.tensor(x, dtype=torch.float64, requires_grad=True) for k, x in tabs.items()}
    opt = torch.optim.Adam(list(P.values()), lr=0.01, betas=(0.9, 0.999), eps=0.0)
    for t in range(1, 8):
        g = {k: rng.normal(size=x.shape) + 0.1 for k, x in tabs.items()}
        tabs, m, v = RR.adam_apply(tabs, m, v, g, {k: x * x for k, x in g.items()}, t, 0.01, 0.9, 0.999, 0.0)
        for k, p in P.items():
            p.grad = torch.tensor(g[k])
        opt.step()
    for k in tabs:
        assert np.abs(tabs[k] - P[k].detach().numpy()).max() <= 1e-12, k


def test_dedup_choice_changes_v():
    """Entity 0 is the head of two pairs: dedup=True gives v = (1-b2)(g1 + g2)^2, False (1-b2)(g1^2 + g2^2)."""
    tabs = RR.integer_tables(6, 1, 4, 4, seed=1)
    pos = np.array([[0, 1, 0], [0, 2, 0]])
    neg = np.array([[3, 1, 0], [0, 4, 0]])
    margin = 1000.0
    z = RR.zeros_like(tabs)
    a = RR.adam_step(tabs, z, z, pos, neg, margin, 1, b1=0.5, b2=0.75, dedup=True)
    b = RR.adam_step(tabs, z, z, pos, neg, margin, 1, b1=0.5, b2=0.75, dedup=False)
    assert np.array_equal(a[1]["ent"], b[1]["ent"])             # m is linear: the same either way
    assert not np.array_equal(a[2]["ent"][0], b[2]["ent"][0])
    _, sl = RR.slices(tabs, pos, neg, margin)
    rows, vals = sl["ent"]
    g0 = vals[rows == 0]
    assert np.allclose(a[2]["ent"][0], 0.25 * g0.sum(0) ** 2) and np.allclose(b[2]["ent"][0], 0.25 * (g0 ** 2).sum(0))
    for k in ("rel", "rel_matrix"):                             # the one relation carries both pairs
        assert not np.array_equal(a[2][k], b[2][k]), k


def test_untouched_rows_still_move():
    rng = np.random.default_rng(2)
    tabs = RR.random_tables(8, 3, 4, 4, rng)
    z = RR.zeros_like(tabs)
    pos, neg = np.array([[0, 1, 0]]), np.array([[2, 1, 0]])
    t1, m1, v1, _ = RR.adam_step(tabs, z, z, pos, neg, 100.0, 1)
    assert np.abs(m1["ent"][0]).max() > 0 and np.array_equal(t1["ent"][5], tabs["ent"][5])
    pos2, neg2 = np.array([[5, 6, 1]]), np.array([[7, 6, 1]])
    t2, m2, _, _ = RR.adam_step(t1, m1, v1, pos2, neg2, 100.0, 2)
    assert not np.array_equal(t2["ent"][0], t1["ent"][0])      # decayed m still moves row 0
    assert np.abs(m2["ent"][0]).max() < np.abs(m1["ent"][0]).max()


def test_exact_bound_accepts_small_fixtures_and_rejects_floats():
    rng = np.random.default_rng(0)
    tabs = RR.integer_tables(50, 3, 8, 5, seed=0)
    pos, neg = RR.skewed_batch(rng, 50, 3, 200)
    assert RR.is_exact_step(tabs, pos, neg, 1.0)
    assert not RR.is_exact_step(RR.random_tables(50, 3, 8, 5, rng), pos, neg, 1.0)
    bad = neg.copy()
    bad[0, 2] = (bad[0, 2] + 1) % 3
    assert not RR.is_exact_step(tabs, pos, bad, 1.0)


def test_cli_reference_defaults():
    a = XRT.build_parser().parse_args([])
    assert (a.l1, a.hidden_size_e, a.hidden_size_r, a.nbatches, a.train_times, a.margin, a.learning_rate, a.seed) == \
        (True, 100, 100, 100, 3000, 1.0, 0.001, 0)
    a = XRT.build_parser().parse_args(["--l2", "--hidden_size_e", "50", "--hidden_size_r", "20"])
    assert (a.l1, a.hidden_size_e, a.hidden_size_r) == (False, 50, 20)
    with pytest.raises(SystemExit):
        XRT.build_parser().parse_args(["--l1", "--l2"])
    assert XRT.MAX_DIM == XR.MAX_DIM


def _write_kg(d, rows=((0, 1, 0), (1, 2, 1), (2, 0, 0))):
    (d / "relation2id.txt").write_text("2\n")
    (d / "entity2id.txt").write_text("3\n")
    (d / "triple2id.txt").write_text(f"{len(rows)}\n" + "".join(f"{h} {t} {r}\n" for h, t, r in rows))


def test_malformed_input_raises_before_gpu(tmp_path, monkeypatch):
    calls = []
    monkeypatch.setattr(XR._lib, "call", lambda *a: calls.append(a))
    monkeypatch.setattr(XR._lib, "load", lambda: calls.append("load"))
    for kw in ({"dim_e": 0}, {"dim_e": 257}, {"dim_r": 300}):
        with pytest.raises(ValueError):
            XR.TransR(10, 2, **kw)
    with pytest.raises(ValueError):
        XR.TransR(0, 2)
    for lr, b1, b2, eps in ((0.0, 0.9, 0.999, 1e-8), (0.001, 1.0, 0.999, 1e-8), (0.001, 0.9, -0.1, 1e-8),
                            (0.001, 0.9, 0.999, -1.0)):
        with pytest.raises(ValueError):
            XR.check_adam(lr, b1, b2, eps)
    for flags in (["--hidden_size_e", "0"], ["--hidden_size_r", "257"], ["--nbatches", "0"], ["--learning_rate", "0"],
                  ["--margin", "nan"], ["--seed", "-1"]):
        with pytest.raises(ValueError):
            XRT.main(flags + ["--data_dir", str(tmp_path)])
    _write_kg(tmp_path, rows=((0, 9, 0),))
    with pytest.raises(ValueError):
        XRT.main(["--data_dir", str(tmp_path), "--nbatches", "1"])
    _write_kg(tmp_path)
    with pytest.raises(ValueError):                             # 3 triples cannot fill 100 batches
        XRT.main(["--data_dir", str(tmp_path)])
    assert calls == []


def test_load_state_dict_that_raises_leaves_the_model_untouched():
    """Every shape (and t) is checked before anything is copied: a wrong-shaped later tensor raises with the tables,
    m, v and t intact."""
    m = XR.TransR(10, 3, 8, 4, device="cpu")
    m.m.fill_(0.5); m.v.fill_(0.25); m.t = 3
    before = {k: v.clone() for k, v in list(m.tables.items()) + [("m", m.m), ("v", m.v)]}
    good = XR.TransR(10, 3, 8, 4, seed=7, device="cpu").state_dict()
    for key, bad in (("rel_matrix", torch.zeros(3, 31)), ("v", torch.zeros(5)), ("t", -1)):
        state = dict(good, l1=False, **{key: bad})
        with pytest.raises(ValueError):
            m.load_state_dict(state)
        assert m.l1 is True and m.t == 3
        for k, v in list(m.tables.items()) + [("m", m.m), ("v", m.v)]:
            assert torch.equal(v, before[k]), (key, k)
