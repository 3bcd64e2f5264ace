"""AdaGrad training of TransE / TransH / TransD on the MI355X (ge_transx_adagrad_step, ge_transx_train_steps_adagrad
through graphembeddings_amd.transx) against the fp64 restatement tests/transx_adagrad_ref.py.

Bounds (tests/transx_adagrad_ref.bounds; derived, not tuned): with g the fp64 summed gradient, mag =
hinge_grads(magnitude=True) and delta = 2^-18 mag,
    table        lr delta / sqrt(a_before) + 2^-22 (|t| + lr)
    accumulator  2 |g| delta + delta^2 + 2^-22 a_new
    loss         5e-6 max(1, |loss|)                       (test_gpu_transx.py)
The reference takes lr as the fp32 value the ABI passes.  Every check prints its family's largest error and largest
error / bound when it grows (`pytest -s` records them)."""
import numpy as np
import pytest
import torch

from tests import transx_adagrad_ref as AR
from tests import transx_ref as TR

pytestmark = pytest.mark.gpu
MODELS = ("transe", "transh", "transd")
A0 = 0.1
LR = float(np.float32(0.05))
F32, I32 = np.float32, np.int32

WORST = {}


def near(family, what, err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    ratio = float(np.max(err / bound))
    w = WORST.setdefault((family, what), [0.0, 0.0])
    if ratio > w[0] or float(err.max()) > w[1]:
        w[0], w[1] = max(w[0], ratio), max(w[1], float(err.max()))
        print("DEV %s %s: largest err/bound %.4g, largest |err| %.4g" % (family, what, w[0], w[1]))
    assert np.all(err <= bound), (family, what, float(err.max()), ratio)


def _model(model, E, R, d, l1=True, seed=0, tabs=None, a0=A0):
    from graphembeddings_amd import transx as X
    m = X.TransX(model, E, R, d, l1=l1, seed=seed)
    if tabs is not None:
        for k, v in tabs.items():
            m.tables[k].copy_(torch.as_tensor(np.asarray(v, dtype=F32)))
    if a0 is not None:
        m.enable_adagrad(a0)
    return m


def _f32(tensors):
    return {k: v.cpu().numpy().copy() for k, v in tensors.items()}


def _f64(arrays):
    return {k: v.astype(np.float64) for k, v in arrays.items()}


def _dev(a):
    return torch.as_tensor(np.asarray(a, dtype=I32)).cuda()


def _pairs(rng, E, R, B):
    pos = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, R, B)], 1).astype(I32)
    neg = pos.copy()
    neg[np.arange(B), rng.integers(0, 2, B)] = rng.integers(0, E, B)
    return pos, neg


def _bits_equal(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k].view(I32), b[k].view(I32)) for k in a)


def _step_check(family, m, pos, neg, lr, margin):
    """One adagrad_step of m from its current state, held to the restatement seeded with that fp32 state; rows no active
    pair names bitwise unchanged in tables and accumulators.  Returns (loss, named)."""
    t0, a0 = _f32(m.tables), _f32(m.accumulators)
    loss = float(m.adagrad_step(_dev(pos), _dev(neg), lr, margin))
    t1, a1 = _f32(m.tables), _f32(m.accumulators)
    rt, ra, rloss, _ = AR.adagrad_step(m.model, _f64(t0), _f64(a0), pos, neg, lr, margin, m.l1)
    bt, ba = AR.bounds(m.model, _f64(t0), _f64(a0), pos, neg, lr, margin, m.l1)
    near(family, "loss", abs(loss - rloss), 5e-6 * max(1.0, abs(rloss)))
    named = AR.named_rows(t0, pos, neg, TR.active_mask(m.model, _f64(t0), pos, neg, margin, m.l1))
    for k in t0:
        near(family, "table", np.abs(t1[k] - rt[k]), bt[k])
        near(family, "accumulator", np.abs(a1[k] - ra[k]), ba[k])
        idle = ~named[k]
        assert np.array_equal(t1[k][idle].view(I32), t0[k][idle].view(I32)), (k, "a table row no active pair names changed")
        assert np.array_equal(a1[k][idle].view(I32), a0[k][idle].view(I32)), (k, "an accumulator row no active pair names changed")
    return loss, named


# ------------------------------------------------------------------ 1. one step against the restatement
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("d", [37, 100])                   # the scalar and the float4 apply
def test_one_step_matches_fp64(model, l1, d):
    pos, neg = _pairs(np.random.default_rng(11), 300, 9, 500)
    m = _model(model, 300, 9, d, l1=l1)
    _, named = _step_check("one_step", m, pos, neg, LR, 1.0)
    assert all(v.any() for v in named.values())


# ------------------------------------------------------------------ 2. the windowed apply's run layouts
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", sorted(TR.LAYOUTS))
@pytest.mark.parametrize("d", [7, 12])                     # the scalar and the float4 apply
def test_window_layouts(model, name, d):
    f = TR.layout_batch(model, name, d, True)
    act = TR.active_mask(model, f["tabs"], f["pos"], f["neg"], f["margin"], True)
    _, srt = TR.slot_keys(f["pos"], f["neg"], f["E"], f["R"], act)
    for key, start, length in f["expect"]:                 # the batch has the layout it was built for
        assert TR.run_of(srt, key) == (start, length)
    m = _model(model, f["E"], f["R"], d, tabs=f["tabs"])
    _, named = _step_check("layouts", m, f["pos"], f["neg"], LR, f["margin"])
    if name == "cut_before_sentinel":                      # the inactive pairs' own rows stayed out (checked bitwise above)
        idle_pairs = f["pos"][~act]
        assert len(idle_pairs) == 10
        assert (~named["ent"][idle_pairs[:, :2]]).any()
    for key, _, _ in f["expect"]:                          # ... and the runs meant were applied
        assert named["ent"][key] if key < f["E"] else named["rel"][key - f["E"]]


# ------------------------------------------------------------------ 3. hot rows
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("hot", ["relation", "head"])
def test_hot_rows(model, hot):
    """>= 1,000 slots on one row: AdaGrad squares the sum of all of them."""
    rng = np.random.default_rng(2)
    B = 1500
    pos, neg = _pairs(rng, 2000, 30, B)
    if hot == "relation":
        pos[:, 2] = neg[:, 2] = 4
    else:                                                  # every pair shares head 17; negatives corrupt the tail
        pos[:, 0] = neg[:, 0] = 17
        neg[:, 1] = rng.integers(0, 2000, B)
    m = _model(model, 2000, 30, 100)
    act = TR.active_mask(model, _f64(_f32(m.tables)), pos, neg, 1.0, True)
    assert act.sum() >= 1000 // (1 if hot == "relation" else 2)
    _step_check("hot_rows", m, pos, neg, LR, 1.0)


# ------------------------------------------------------------------ 4. twenty dependent steps
@pytest.mark.parametrize("model", MODELS)
def test_twenty_dependent_steps(model):
    """Each step is held to the restatement re-seeded from the device's fp32 tables and accumulators."""
    rng = np.random.default_rng(7)
    E, R, d = 400, 6, 64
    m = _model(model, E, R, d, l1=False, seed=3)
    for _ in range(20):
        pos, neg = _pairs(rng, E, R, 256)
        _step_check("twenty_steps", m, pos, neg, LR, 1.0)
    assert all(float(a.max()) > A0 for a in m.accumulators.values())


# ------------------------------------------------------------------ 5. / 6. nothing active, lr = 0
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [37, 100])
def test_nothing_active(model, d):
    pos, neg = _pairs(np.random.default_rng(5), 300, 9, 500)
    m = _model(model, 300, 9, d)
    t0, a0 = _f32(m.tables), _f32(m.accumulators)
    assert float(m.adagrad_step(_dev(pos), _dev(neg), LR, -1e30)) == 0.0
    assert _bits_equal(t0, _f32(m.tables)) and _bits_equal(a0, _f32(m.accumulators))


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [37, 100])
def test_lr_zero(model, d):
    pos, neg = _pairs(np.random.default_rng(6), 300, 9, 500)
    m = _model(model, 300, 9, d)
    t0, a0 = _f32(m.tables), _f32(m.accumulators)
    m.adagrad_step(_dev(pos), _dev(neg), 0.0, 1.0)
    assert _bits_equal(t0, _f32(m.tables))
    _, ra, _, g = AR.adagrad_step(model, _f64(t0), _f64(a0), pos, neg, 0.0, 1.0, True)
    _, ba = AR.bounds(model, _f64(t0), _f64(a0), pos, neg, 0.0, 1.0, True)
    a1 = _f32(m.accumulators)
    for k in ra:
        near("lr_zero", "accumulator", np.abs(a1[k] - ra[k]), ba[k])
        assert np.abs(g[k]).max() > 0 and a1[k].max() > A0


# ------------------------------------------------------------------ 7. the native loop
def _kg(seed=0, E=300, R=8, T=3000):
    rng = np.random.default_rng(seed)
    tri = np.stack([rng.integers(0, E, T), rng.integers(0, E, T), rng.integers(0, R, T)], 1)
    tri[:400, 2] = 0                                       # one busy relation
    return np.unique(tri, axis=0).astype(np.int64), E, R


def _state(m):
    return _f32(m.tables), _f32(m.accumulators)


@pytest.mark.parametrize("model", MODELS)
def test_loop(model):
    tri, E, R = _kg(1)
    B, seed, d = 700, 21, 48
    kw = dict(margin=1.0, learning_rate=LR, seed=seed, optimizer="adagrad", initial_accumulator_value=A0)
    a = _model(model, E, R, d, seed=2, a0=None)
    assert a.accumulators is None
    tr = a.trainer(tri, B, **kw)                            # enables AdaGrad
    assert set(a.accumulators) == set(a.tables) and all(bool((v == F32(A0)).all()) for v in a.accumulators.values())
    la = tr.run(7).cpu().numpy()
    # seven draw(s) + adagrad_step calls: the loop's Philox draws are the SGD loop's
    b = _model(model, E, R, d, seed=2)
    sgd_tr = _model(model, E, R, d, seed=2, a0=None).trainer(tri, B, margin=1.0, learning_rate=LR, seed=seed)
    for s in range(7):
        pos, neg = tr.draw(s)
        ps, ns = sgd_tr.draw(s)
        assert torch.equal(pos, ps) and torch.equal(neg, ns)
        assert float(b.adagrad_step(pos, neg, LR, 1.0)) == la[s], s
    assert all(_bits_equal(x, y) for x, y in zip(_state(a), _state(b)))
    # run(3); run(4)
    c = _model(model, E, R, d, seed=2, a0=None)
    trc = c.trainer(tri, B, **kw)
    lc = np.concatenate([trc.run(3).cpu().numpy(), trc.run(4).cpu().numpy()])
    assert np.array_equal(lc.view(I32), la.view(I32)) and trc.step_count == 7
    assert all(_bits_equal(x, y) for x, y in zip(_state(a), _state(c)))
    # a second fresh run
    e = _model(model, E, R, d, seed=2, a0=None)
    le = e.trainer(tri, B, **kw).run(7).cpu().numpy()
    assert np.array_equal(le.view(I32), la.view(I32))
    assert all(_bits_equal(x, y) for x, y in zip(_state(a), _state(e)))
    assert e.trainer(tri, B, **kw).run(0).numel() == 0
    assert float(max(v.max() for v in a.accumulators.values())) > A0


# ------------------------------------------------------------------ 8. SGD untouched
@pytest.mark.parametrize("model", MODELS)
def test_sgd_step_untouched(model):
    pos, neg = _pairs(np.random.default_rng(11), 300, 9, 500)
    m = _model(model, 300, 9, 100)
    before, a0 = _f64(_f32(m.tables)), _f32(m.accumulators)
    loss = float(m.step(_dev(pos), _dev(neg), 0.01, 1.0))
    new, rloss = TR.sgd_step(model, before, pos, neg, 0.01, 1.0, True)
    assert abs(loss - rloss) <= 5e-6 * max(1.0, abs(rloss))
    after = _f32(m.tables)
    for k in new:
        assert np.abs(after[k] - new[k]).max() <= 5e-6, k
    assert _bits_equal(a0, _f32(m.accumulators))
    # ... and the SGD loop of a model with accumulators leaves them alone as well
    tri, E, R = _kg()
    m = _model(model, E, R, 48)
    a0 = _f32(m.accumulators)
    m.trainer(tri, 200, learning_rate=0.01).run(2)
    assert _bits_equal(a0, _f32(m.accumulators))


# ------------------------------------------------------------------ 9. state
def test_state_dict_round_trip_and_refusal():
    tri, E, R = _kg(2)
    kw = dict(margin=1.0, learning_rate=LR, seed=4, optimizer="adagrad")
    m = _model("transd", E, R, 16, seed=1, a0=None)
    plain = m.state_dict()
    assert set(plain) == {"model", "l1", "n_ent", "n_rel", "d", "ent", "rel", "ent_transfer", "rel_transfer"}
    tr = m.trainer(tri, 300, initial_accumulator_value=0.25, **kw)
    tr.run(3)
    sd = m.state_dict()
    assert set(sd) == set(plain) | {"adagrad_init"} | {"adagrad_" + k for k in m.tables} and sd["adagrad_init"] == 0.25
    m2 = _model("transd", E, R, 16, seed=2, a0=None)
    m2.load_state_dict(sd)                                  # a state with accumulators enables AdaGrad and restores them
    assert m2.adagrad_init == 0.25 and all(_bits_equal(x, y) for x, y in zip(_state(m), _state(m2)))
    tr2 = m2.trainer(tri, 300, **kw)
    tr2.step_count = tr.step_count
    l1_, l2_ = tr.run(3).cpu().numpy(), tr2.run(3).cpu().numpy()
    assert np.array_equal(l1_.view(I32), l2_.view(I32))
    assert all(_bits_equal(x, y) for x, y in zip(_state(m), _state(m2)))
    # a wrong-shape accumulator raises and changes nothing, the tables included
    m3 = _model("transd", E, R, 16, seed=3, a0=0.5)
    m3.adagrad_step(*tr.draw(0), LR, 1.0)
    t3, a3 = _state(m3)
    for bad in (dict(sd, adagrad_rel_transfer=torch.zeros(R + 1, 16)), dict(sd, adagrad_ent=torch.zeros(E, 15)),
                {k: v for k, v in sd.items() if k != "adagrad_ent_transfer"}, dict(sd, adagrad_init=0.0),
                dict(sd, rel=torch.zeros(R, 15))):
        with pytest.raises(ValueError):
            m3.load_state_dict(bad)
        assert all(_bits_equal(x, y) for x, y in zip((t3, a3), _state(m3))) and m3.adagrad_init == 0.5
    # a state without accumulators refills those of a model that has them
    m3.load_state_dict(plain)
    assert _bits_equal(_f32(m3.tables), {k: plain[k].numpy() for k in m3.tables})
    assert all(bool((v == 0.5).all()) for v in m3.accumulators.values())
    # ... and leaves a model without them as it was
    m4 = _model("transd", E, R, 16, seed=5, a0=None)
    m4.load_state_dict(plain)
    assert m4.accumulators is None and set(m4.state_dict()) == set(plain)


def test_python_refusals():
    from graphembeddings_amd import transr
    m = _model("transe", 20, 3, 8, a0=None)
    pos, neg = _pairs(np.random.default_rng(0), 20, 3, 4)
    with pytest.raises(RuntimeError, match="enable_adagrad"):
        m.adagrad_step(_dev(pos), _dev(neg), LR, 1.0)
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError):
            m.enable_adagrad(bad)
    assert m.accumulators is None
    m.enable_adagrad()
    assert m.adagrad_init == 0.1
    tri = np.array([[0, 1, 0], [2, 3, 1]])
    with pytest.raises(ValueError, match="Adam"):
        transr.TransR(20, 3, 8, 8).trainer(tri, 2, optimizer="adagrad")
    with pytest.raises(ValueError, match="optimizer"):
        m.trainer(tri, 2, optimizer="adam")


# ------------------------------------------------------------------ 10. learning
def test_planted_kg_learns_with_adagrad():
    """test_gpu_transx.py's test_planted_kg_learns with optimizer="adagrad": lr 0.05, a0 0.1, 600 steps against the SGD
    test's 3,000 (the fp64 restatement with uniform corruption reaches 0.879 at these settings)."""
    tri = TR.planted_kg(seed=0)
    E = 2000
    cut = int(0.9 * len(tri))
    train, held = tri[:cut], tri[cut:]
    rng = np.random.default_rng(1)
    corr = held.copy()
    side = rng.integers(0, 2, len(held))
    corr[np.arange(len(held)), side] = rng.integers(0, E, len(held))
    keep = ~np.all(corr == held, 1)
    held = torch.as_tensor(held[keep].astype(I32)).cuda()
    corr = torch.as_tensor(corr[keep].astype(I32)).cuda()
    m = _model("transe", E, 20, 32, seed=0, a0=None)
    acc = lambda: float((m.score(held) < m.score(corr)).float().mean())
    acc0 = acc()
    m.trainer(train, len(train) // 20, margin=1.0, learning_rate=0.05, seed=3, optimizer="adagrad",
              initial_accumulator_value=0.1).run(600)
    acc1 = acc()
    print(f"planted KG held-out pairwise accuracy with AdaGrad: untrained {acc0:.4f}, trained {acc1:.4f} (600 steps)")
    assert acc1 >= 0.8 and acc1 - acc0 >= 0.25


# ------------------------------------------------------------------ 11. the driver
def _write(path, rows, count=None):
    with open(path, "w") as f:
        f.write(f"{len(rows) if count is None else count}\n")
        for r in rows:
            f.write(" ".join(str(int(x)) for x in r) + "\n")


def test_driver_trains_saves_and_reloads(tmp_path, capsys):
    from graphembeddings_amd import transx_train as D
    tri = TR.planted_kg(n_ent=120, n_rel=4, n_triples=900, seed=1)
    dd = tmp_path / "data"
    dd.mkdir()
    _write(str(dd / "entity2id.txt"), [], 120)
    _write(str(dd / "relation2id.txt"), [], 4)
    _write(str(dd / "triple2id.txt"), tri)
    base = ["--data_dir", str(dd), "--model", "transh", "--hidden_size", "12", "--nbatches", "4", "--learning_rate", "0.05"]
    ada = ["--optimizer", "adagrad", "--adagrad_init", "0.2"]

    def run(out, more):
        assert D.main(base + ["--output_dir", str(tmp_path / out)] + more) == 0
        text = capsys.readouterr().out
        losses = [float(x) for x in text.split("\n")[1::2] if x and not x.startswith(("saved", "wrote"))]
        return torch.load(str(tmp_path / out / "transh.pt"), map_location="cpu"), text, losses

    sa, _, la = run("a", ada + ["--train_times", "3"])
    names = ("ent", "rel", "normal_vector")
    assert sa["adagrad_init"] == 0.2 and all(float(sa["adagrad_" + k].min()) >= F32(0.2) for k in names)
    assert all(float(sa["adagrad_" + k].max()) > 0.2 and sa["adagrad_" + k].shape == sa[k].shape for k in names)
    assert len(la) == 3 and la[2] < la[0]
    # --load restores the accumulators and training continues from them
    sb, text, lb = run("b", ada + ["--train_times", "2", "--load", str(tmp_path / "a" / "transh.pt")])
    assert "holds no AdaGrad accumulators" not in text and sb["adagrad_init"] == 0.2
    assert all(bool((sb["adagrad_" + k] >= sa["adagrad_" + k]).all()) and float((sb["adagrad_" + k] - sa["adagrad_" + k]).max()) > 0
               for k in names)
    assert not torch.equal(sb["ent"], sa["ent"]) and len(lb) == 2
    # --train_times 0: the file is handed on as it is
    sc, _, _ = run("c", ada + ["--train_times", "0", "--load", str(tmp_path / "a" / "transh.pt")])
    assert all(torch.equal(sc[k], sa[k]) for k in sa if k.startswith("adagrad_") and k != "adagrad_init")
    # a file without accumulators: they start at --adagrad_init, and the driver says so
    ss, _, _ = run("s", ["--train_times", "1"])
    assert not any(k.startswith("adagrad") for k in ss)
    sd_, text, _ = run("d", ada + ["--train_times", "1", "--load", str(tmp_path / "s" / "transh.pt")])
    assert "holds no AdaGrad accumulators: they start at --adagrad_init 0.2" in text
    assert sd_["adagrad_init"] == 0.2 and float(sd_["adagrad_ent"].min()) >= F32(0.2)
    with pytest.raises(ValueError, match="adagrad_init"):
        D.main(base + ada[:2] + ["--adagrad_init", "0"])
