"""CPU checks of the TransX layer: the fp64 restatement against torch autograd, the *2id.txt reader, the driver's
flags, and argument errors raised before any GPU call."""
import numpy as np
import pytest
import torch

from graphembeddings_amd import transx as X
from graphembeddings_amd import transx_train as XT
from tests import transx_ref as TR

MODELS = ("transe", "transh", "transd")


def _tables(model, E, R, d, rng):
    t = {"ent": rng.normal(size=(E, d)), "rel": rng.normal(size=(R, d))}
    for name in TR.EXTRA[model]:
        t[name] = rng.normal(size=((E if name == "ent_transfer" else R), d))
    return t


def _autograd(model, tabs, pos, neg, margin, l1):
    """The same formulas, differentiated by torch in fp64 with TF's tie rules spelled as torch.where."""
    T = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in tabs.items()}
    pos, neg = torch.as_tensor(pos), torch.as_tensor(neg)

    def proj(e_id, r_id):
        e = T["ent"][e_id]
        if model == "transh":
            n = T["normal_vector"][r_id]
            nn = (n * n).sum(1, keepdim=True)
            nh = n * torch.rsqrt(torch.where(nn >= TR.EPS, nn, torch.full_like(nn, TR.EPS)))
            return e - (e * nh).sum(1, keepdim=True) * nh
        if model == "transd":
            return e + (e * T["ent_transfer"][e_id]).sum(1, keepdim=True) * T["rel_transfer"][r_id]
        return e

    def D(tr):
        u = proj(tr[:, 0], tr[:, 2]) + T["rel"][tr[:, 2]] - proj(tr[:, 1], tr[:, 2])
        return u.abs().sum(1) if l1 else (u * u).sum(1)

    z = D(pos) - D(neg) + margin
    loss = torch.where(z >= 0, z, torch.zeros_like(z)).sum()
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in T.items()}


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("l1", [True, False])
def test_ref_gradients_match_autograd(model, l1):
    rng = np.random.default_rng(3)
    E, R, d, B = 12, 3, 7, 40
    tabs = _tables(model, E, R, d, rng)
    pos = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, R, B)], 1)
    neg = pos.copy()
    neg[:, 1] = rng.integers(0, E, B)
    neg[::3, 0], neg[::3, 1] = rng.integers(0, E, len(neg[::3])), pos[::3, 1]
    neg[5] = pos[5]                                            # identical pair: D+ - D- + margin = margin
    if model == "transh":
        tabs["normal_vector"][1] = 0.0                         # a zero normal: the l2_normalize clamp
    # a zero L1 component: h + r - t = 0 in column 0 of pair 0 (TransE only: projections move it)
    if model == "transe":
        tabs["rel"][pos[0, 2], 0] = tabs["ent"][pos[0, 1], 0] - tabs["ent"][pos[0, 0], 0]
    loss, g = TR.hinge_grads(model, tabs, pos, neg, 1.0, l1)
    aloss, ag = _autograd(model, tabs, pos, neg, 1.0, l1)
    assert abs(loss - aloss) <= 1e-12 * max(1.0, abs(aloss))
    for k in tabs:
        assert np.abs(g[k] - ag[k]).max() <= 1e-12 * max(1.0, np.abs(ag[k]).max()), k


@pytest.mark.parametrize("model", MODELS)
def test_ref_exact_tie_is_active(model):
    """D+ - D- + margin == 0 exactly: MaximumGrad sends the tie to x, so the pair takes a gradient."""
    rng = np.random.default_rng(5)
    tabs = _tables(model, 6, 2, 4, rng)
    pos, neg = np.array([[0, 1, 0]]), np.array([[2, 1, 0]])
    margin = float(TR.score(model, tabs, neg)[0] - TR.score(model, tabs, pos)[0])
    loss, g = TR.hinge_grads(model, tabs, pos, neg, margin, True)
    assert loss == pytest.approx(0.0, abs=1e-12)
    assert np.abs(g["rel"]).max() > 0 or np.abs(g["ent"]).max() > 0
    aloss, ag = _autograd(model, tabs, pos, neg, margin, True)
    for k in tabs:
        assert np.abs(g[k] - ag[k]).max() <= 1e-12, k


def test_ref_sgd_sums_duplicates():
    rng = np.random.default_rng(1)
    tabs = _tables("transe", 5, 1, 3, rng)
    pos = np.array([[0, 1, 0], [0, 1, 0]])
    neg = np.array([[0, 2, 0], [0, 3, 0]])
    new, loss = TR.sgd_step("transe", tabs, pos, neg, 0.1, 5.0, True)
    _, g = TR.hinge_grads("transe", tabs, pos, neg, 5.0, True)
    assert np.allclose(new["ent"], tabs["ent"] - 0.1 * g["ent"])
    g0, g1 = (TR.hinge_grads("transe", tabs, pos[k:k + 1], neg[k:k + 1], 5.0, True)[1] for k in (0, 1))
    for k in tabs:                                             # row 0 and relation 0 take both pairs' terms
        assert np.allclose(g[k], g0[k] + g1[k])
    assert loss > 0


def test_draw_rows_uniform():
    rows = TR.draw_positive_rows(37, 20000, seed=4, step=9)
    assert rows.min() >= 0 and rows.max() < 37
    counts = np.bincount(rows, minlength=37)
    assert counts.min() > 400 and counts.max() < 700


def _write_kg(tmp_path, E=5, R=2, rows=((0, 1, 0), (2, 3, 1), (4, 0, 1)), declared=None, extra=""):
    (tmp_path / "relation2id.txt").write_text(f"{R}\nrel0\t0\nrel1\t1\n")
    (tmp_path / "entity2id.txt").write_text(f"{E}\n" + "".join(f"e{i}\t{i}\n" for i in range(E)))
    body = "".join(f"{h} {t} {r}\n" for h, t, r in rows)
    (tmp_path / "triple2id.txt").write_text(f"{len(rows) if declared is None else declared}\n{body}{extra}")


def test_reader_like_init_cpp(tmp_path):
    _write_kg(tmp_path, declared=10)                          # fewer rows than declared: init.cpp reads what is there
    E, R, tri = X.read_kg(str(tmp_path))
    assert (E, R) == (5, 2)
    assert tri.dtype == np.int32 and tri.tolist() == [[0, 1, 0], [2, 3, 1], [4, 0, 1]]   # h t r order


@pytest.mark.parametrize("bad", ["partial", "too_many", "ent_range", "rel_range", "token"])
def test_reader_rejects_malformed(tmp_path, bad):
    if bad == "partial":
        _write_kg(tmp_path, extra="1 2\n")
    elif bad == "too_many":
        _write_kg(tmp_path, declared=2)
    elif bad == "ent_range":
        _write_kg(tmp_path, rows=((0, 5, 0),))
    elif bad == "rel_range":
        _write_kg(tmp_path, rows=((0, 1, 2),))
    else:
        _write_kg(tmp_path, extra="1 x 0\n")
    with pytest.raises(ValueError):
        X.read_kg(str(tmp_path))


def test_cli_reference_defaults():
    a = XT.build_parser().parse_args([])
    assert (a.model, a.l1, a.hidden_size, a.nbatches, a.train_times, a.margin, a.learning_rate) == \
        ("transe", True, 100, 100, 3000, 1.0, 0.001)
    a = XT.build_parser().parse_args(["--model", "transd", "--l2", "--hidden_size", "50"])
    assert (a.model, a.l1, a.hidden_size) == ("transd", False, 50)
    with pytest.raises(SystemExit):
        XT.build_parser().parse_args(["--model", "transr"])


def test_malformed_input_raises_before_gpu(tmp_path, monkeypatch):
    calls = []
    monkeypatch.setattr(X._lib, "call", lambda *a: calls.append(a))
    monkeypatch.setattr(X._lib, "load", lambda: calls.append("load"))
    with pytest.raises(ValueError):
        X.TransX("transr", 10, 2, 8)
    with pytest.raises(ValueError):
        X.TransX("transe", 10, 2, 2048)
    with pytest.raises(ValueError):
        XT.main(["--hidden_size", "0", "--data_dir", str(tmp_path)])
    _write_kg(tmp_path, rows=((0, 9, 0),))
    with pytest.raises(ValueError):
        XT.main(["--data_dir", str(tmp_path), "--nbatches", "1"])
    _write_kg(tmp_path)
    with pytest.raises(ValueError):                           # 3 triples cannot fill 100 batches
        XT.main(["--data_dir", str(tmp_path)])
    assert calls == []
