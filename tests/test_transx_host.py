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


def test_slot_keys_scheme():
    """Slots 4i..4i+3 = pos h, pos t, neg h, neg t; slot 4B+i = E + r; an inactive pair's slots = E + R."""
    E, R = 10, 3
    pos, neg = np.array([[1, 2, 0], [3, 1, 2], [7, 7, 1]]), np.array([[1, 5, 0], [3, 1, 2], [4, 7, 1]])
    keys, srt = TR.slot_keys(pos, neg, E, R, [True, False, True])
    assert keys.tolist() == [1, 2, 1, 5, 13, 13, 13, 13, 7, 7, 4, 7, 10, 13, 11]
    assert srt.tolist() == sorted(keys.tolist())
    assert TR.run_of(srt, 7) == (5, 3) and TR.run_of(srt, 13) == (10, 5)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", sorted(TR.LAYOUTS))
@pytest.mark.parametrize("d", [7, 8])
@pytest.mark.parametrize("l1", [True, False])
def test_layout_batches_have_their_layout(model, name, d, l1):
    """Each layout the GPU tests use puts its runs where it says, with the activity it says, and (TransE / TransD)
    is exact: every value of the step is an integer, or a multiple of lr, below 2^24, so fp32 holds it."""
    f = TR.layout_batch(model, name, d, l1)
    spec = TR.LAYOUTS[name]
    act = TR.active_mask(model, f["tabs"], f["pos"], f["neg"], f["margin"], l1)
    assert act.sum() == sum(spec["counts"]) and len(act) == sum(spec["counts"]) + spec.get("inactive", 0)
    z = TR.score(model, f["tabs"], f["pos"], l1) - TR.score(model, f["tabs"], f["neg"], l1) + f["margin"]
    assert np.all(z[~act] == -1.0) and np.all(z[act] >= (1.0 if f["margin"] > 0 else 0.0))
    _, srt = TR.slot_keys(f["pos"], f["neg"], f["E"], f["R"], act)
    for key, start, length in f["expect"]:
        assert TR.run_of(srt, key) == (start, length)
    if model != "transh":
        assert TR.exact_step_bound(model, f["tabs"], f["pos"], f["neg"], f["lr"], f["margin"], l1) < TR.FP32_EXACT
        new, loss = TR.sgd_step(model, f["tabs"], f["pos"], f["neg"], f["lr"], f["margin"], l1)
        assert np.float32(loss) == loss
        for k in new:
            assert np.array_equal(new[k].astype(np.float32), new[k]) and not np.array_equal(new[k], f["tabs"][k])


def test_layouts_cut_where_they_say():
    """The windows of the runs: whole, cut in two, straddling, four windows, meeting, ending at the last slot."""
    win = lambda s, n: (s // TR.KWIN, (s + n - 1) // TR.KWIN)
    spans = {name: [win(s, n) for _, s, n in spec["expect"]] for name, spec in TR.LAYOUTS.items()}
    assert spans["run32_on_boundary"] == [(5, 5)] and spans["run33"] == [(5, 6)] and spans["straddle2"] == [(1, 2)]
    assert spans["four_windows"] == [(13, 16)] and spans["two_cuts_meet"] == [(10, 11), (11, 12)]
    assert spans["cut_before_sentinel"] == [(2, 3)] and spans["hot_entities"] == [(0, 1), (1, 2)]
    f = TR.layout_batch("transe", "two_cuts_meet", 8)
    assert 5 * len(f["pos"]) == 410                                        # relation 2 ends at the last slot
    f = TR.layout_batch("transe", "cut_before_sentinel", 8)
    assert 5 * sum(TR.LAYOUTS["cut_before_sentinel"]["counts"]) == 115    # relation 1 ends right before sentinels


def test_exact_bound_rejects_what_fp32_cannot_hold():
    f = TR.layout_batch("transd", "four_windows", 100, l1=False)          # a 100-slot hot row at d = 100, L2
    args = (f["pos"], f["neg"], f["lr"], f["margin"], False)
    assert TR.exact_step_bound("transd", f["tabs"], *args) > TR.FP32_EXACT
    assert not TR.is_exact_step("transd", f["tabs"], *args)
    g = TR.layout_batch("transd", "four_windows", 8, l1=False)
    assert TR.is_exact_step("transd", g["tabs"], g["pos"], g["neg"], g["lr"], g["margin"], False)
    half = {k: v + 0.5 for k, v in g["tabs"].items()}
    for bad in ((half, g["lr"], g["margin"]), (g["tabs"], 0.01, g["margin"]), (g["tabs"], g["lr"], g["margin"] + 0.5)):
        assert not TR.is_exact_step("transd", bad[0], g["pos"], g["neg"], bad[1], bad[2], False)
    with pytest.raises(ValueError):
        TR.exact_step_bound("transh", TR.exact_tables("transh", 5, 2, 4), g["pos"][:1] % 2, g["neg"][:1] % 2,
                            1 / 64, 1.0)


@pytest.mark.parametrize("model", MODELS)
def test_magnitude_bounds_the_gradient(model):
    rng = np.random.default_rng(6)
    tabs = _tables(model, 12, 3, 5, rng)
    pos = np.stack([rng.integers(0, 12, 30), rng.integers(0, 12, 30), rng.integers(0, 3, 30)], 1)
    neg = pos.copy()
    neg[:, 1] = rng.integers(0, 12, 30)
    _, g = TR.hinge_grads(model, tabs, pos, neg, 2.0, True)
    _, mag = TR.hinge_grads(model, tabs, pos, neg, 2.0, True, magnitude=True)
    _, g1 = TR.hinge_grads(model, tabs, pos[:1], neg[:1], 2.0, True)
    _, mag1 = TR.hinge_grads(model, tabs, pos[:1], neg[:1], 2.0, True, magnitude=True)
    for k in g:
        assert np.all(np.abs(g[k]) <= mag[k] + 1e-12) and mag[k].max() > np.abs(g[k]).max()
        assert np.all(np.abs(g1[k]) <= mag1[k] + 1e-12)


def test_load_state_dict_that_raises_leaves_the_model_untouched():
    """Every shape is checked before anything is copied: a wrong-shaped later table raises with `ent` still intact."""
    m = X.TransX("transd", 10, 3, 8, device="cpu")
    before = {k: v.clone() for k, v in m.tables.items()}
    state = X.TransX("transd", 10, 3, 8, seed=7, device="cpu").state_dict()
    state["l1"] = False
    state["rel_transfer"] = torch.zeros(3, 9)
    with pytest.raises(ValueError, match="rel_transfer"):
        m.load_state_dict(state)
    assert m.l1 is True
    for k, v in m.tables.items():
        assert torch.equal(v, before[k]), k
