"""GPU: evaluate.TranslationPocket -- filtered-MRR validation ticks and a pocket for TransE / TransH / TransD, TransR and
RotatE.

Shapes: E = 300 entities (one full and one partial 256-candidate block of the rank sweeps), R = 7 relations, V = 37
validation rows (no multiple of the sweeps' 16-row chunk); transe / transh / transd at d = 20, TransR at dim_e = 12,
dim_r = 8, RotatE at d = 16; both norms for TransE and RotatE.  known = train + valid.

The reference of every metric is mrr_and_hits over the integer ranks of evaluate.translation_ranks on the same rows (the
evaluator the drivers print), compared through tests/rank_tick_ref.check_metrics: entries 2-7 bitwise, the two MRRs within
2^-23.  Pocket contents are compared bitwise, as int32."""
import functools

import numpy as np
import pytest
import torch

from graphembeddings_amd import _lib
from graphembeddings_amd import evaluate as EV
from graphembeddings_amd import rotate, transr, transx
from tests import rank_tick_ref as RT
from tests import rotate_ref as RR
from tests import transx_ref as XR

pytestmark = pytest.mark.gpu

I32, F32 = np.int32, np.float32
E, R, V = 300, 7, 37
KINDS = ["transe-l1", "transe-l2", "transh", "transd", "transr", "rotate-l1", "rotate-l2"]
POCKET_KINDS = ["transe-l1", "transh", "transd", "transr", "rotate-l1"]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")


def make(kind, seed=0):
    if kind.startswith("transe"):
        return transx.TransX("transe", E, R, 20, l1=kind.endswith("l1"), seed=seed)
    if kind in ("transh", "transd"):
        return transx.TransX(kind, E, R, 20, l1=True, seed=seed)
    if kind == "transr":
        return transr.TransR(E, R, 12, 8, l1=True, seed=seed)
    return rotate.RotatE(E, R, 16, l1=kind.endswith("l1"), seed=seed)


@functools.lru_cache(maxsize=None)
def graph(rotational: bool):
    """(train, valid, known = train + valid) of a planted KG, computed once per family."""
    if rotational:
        tri = RR.planted_rotation_kg(n_ent=E, n_rel=R, k=4, n_triples=4000, seed=3, sym=2)
    else:
        tri = XR.planted_kg(n_ent=E, n_rel=R, dim=8, n_triples=4000, seed=3)
    train, valid = tri[:-V], tri[-V:]
    assert len(valid) == V and len(set(valid[:, 2])) > 1
    return train, valid, tri


def graph_of(kind):
    return graph(kind.startswith("rotate"))


def reference(m, rows, known, sets=None):
    """The eight numbers of a tick in float64, from the integer ranks of translation_ranks on `rows`, both sides."""
    raws, fils = [], []
    for side in ("tail", "head"):
        r, f = EV.translation_ranks(m, rows, known, side=side, candidate_sets=None if sets is None else sets[side])
        raws.append(r)
        fils.append(f)
    raw, fil = np.concatenate(raws), np.concatenate(fils)
    mh = EV.mrr_and_hits(raw, fil)
    return np.array([mh[k] for k in RT.KEYS[:7]] + [float(raw.size)])


def got8(metrics: dict) -> np.ndarray:
    return np.array([metrics[k] for k in RT.KEYS], dtype=F32)


def bits(a):
    return np.ascontiguousarray(a).view(I32)


def state_of(m):
    torch.cuda.synchronize()
    return {k: t.detach().cpu().numpy().copy() for k, t in m._pocket_tensors().items()}


def set_state(m, state):
    for k, t in m._pocket_tensors().items():
        t.copy_(torch.as_tensor(state[k]).cuda())


def same(a: dict, b: dict) -> bool:
    return a.keys() == b.keys() and all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)


# ------------------------------------------------------------------------------------------------ metrics
@pytest.mark.parametrize("kind", KINDS)
def test_metrics_parity(kind):
    train, valid, known = graph_of(kind)
    m = make(kind, seed=1)
    ref = reference(m, valid, known)
    vp = EV.TranslationPocket(m, valid, known)
    before = state_of(m)
    vp.tick(3)
    vp.tick(4)
    (s1, a), (s2, b) = vp.read()
    assert (s1, s2) == (3, 4) and vp.read() == []
    RT.check_metrics(got8(a), ref, "pocket %s" % kind)
    assert a["counted"] == 2 * V == ref[7]
    assert np.array_equal(bits(got8(a)), bits(got8(b)))                  # two ticks on one state agree bitwise
    assert a["improved"] and not b["improved"]                          # ... and a tie keeps the first
    assert float(vp.best) == a["filtered_mrr"]
    assert same(before, state_of(m)) and same(before, {k: t.cpu().numpy() for k, t in vp.pocket.items()})
    assert sorted(vp.row_index.tolist()) == list(range(V)) and np.all(np.diff(valid[vp.row_index, 2]) >= 0)


@pytest.mark.parametrize("kind", ["transe-l1", "transr", "rotate-l1"])
def test_unfiltered_and_batches(kind):
    """known=None: filtered == raw.  batch=16 and batch=5: several native calls a side, the last one partial, give the
    numbers of one call."""
    train, valid, known = graph_of(kind)
    m = make(kind, seed=2)
    vp = EV.TranslationPocket(m, valid, None, keep_state=False)
    vp.tick(0)
    (_, a), = vp.read()
    RT.check_metrics(got8(a), reference(m, valid, None), "pocket unfiltered %s" % kind)
    assert a["filtered_mrr"] == a["raw_mrr"] and a["mean_filtered_pos"] == a["mean_raw_pos"]
    assert vp.pocket is None and vp.restore() is None
    whole = EV.TranslationPocket(m, valid, known, keep_state=False)
    whole.tick(0)
    (_, w), = whole.read()
    for batch in (16, 5):
        vp = EV.TranslationPocket(m, valid, known, keep_state=False, batch=batch)
        vp.tick(0)
        (_, b), = vp.read()
        assert np.array_equal(bits(got8(b)), bits(got8(w))), batch


@pytest.mark.parametrize("kind", ["transh", "rotate-l2"])
def test_rows(kind):
    train, valid, known = graph_of(kind)
    m = make(kind, seed=3)
    n, seed = 10, 4
    want = np.random.default_rng(seed).permutation(V)[:n]
    vp = EV.TranslationPocket(m, valid, known, rows=n, seed=seed)
    assert vp.V == n and sorted(vp.row_index.tolist()) == sorted(want.tolist())
    assert np.array_equal(vp.triples.cpu().numpy(), valid[vp.row_index])
    vp.tick(1)
    (_, a), = vp.read()
    RT.check_metrics(got8(a), reference(m, valid[want], known), "pocket rows %s" % kind)
    assert a["counted"] == 2 * n
    other = EV.TranslationPocket(m, valid, known, rows=n, seed=seed + 1)
    assert sorted(other.row_index.tolist()) != sorted(want.tolist())
    assert EV.TranslationPocket(m, valid, known, rows=V + 100, seed=seed).V == V


# ------------------------------------------------------------------------------------------------ the pocket
def trained(kind):
    """A model after a few hundred steps of its native loop on the planted KG (B of the pocket sequence)."""
    train = graph_of(kind)[0]
    m = make(kind, seed=5)
    if kind == "transr":
        tr = m.trainer(train, 128, margin=1.0, learning_rate=0.01, seed=1)
    else:
        tr = m.trainer(train, 128, loss="self_adversarial", negatives=8, adversarial_temperature=1.0, margin=2.0,
                       learning_rate=0.5 if kind.startswith("rotate") else 0.05, optimizer="adagrad", seed=1)
    tr.run(300)
    return m


def noisy(m, base, scale, seed):
    """base's tables plus Gaussian noise of `scale` standard deviations of each table; fresh optimiser state."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, v in base.items():
        if k in m.tables:
            out[k] = (v + rng.standard_normal(v.shape) * scale * v.std()).astype(F32) if scale else v.copy()
        else:
            out[k] = (0.1 + rng.random(v.shape)).astype(F32)
    return out


# State A of the pocket sequence: B plus noise of this many standard deviations of each table -- enough to rank clearly
# worse than B and clearly better than C (3 standard deviations, next to random).  The order is asserted before any tick.
A_NOISE = {"transe-l1": 1.0, "transh": 1.0, "transd": 1.0, "transr": 0.25, "rotate-l1": 0.25}


@pytest.mark.parametrize("kind", POCKET_KINDS)
def test_pocket_sequence(kind):
    train, valid, known = graph_of(kind)
    m = trained(kind)
    sB = state_of(m)
    sA, sC = noisy(m, sB, A_NOISE[kind], 1), noisy(m, sB, 3.0, 2)
    sD = noisy(m, sB, 0.0, 3)                                           # B's tables, other accumulators / moments
    assert all(np.array_equal(bits(sD[k]), bits(sB[k])) for k in m.tables) and not same(sD, sB)
    mrr = {}
    for name, s in (("A", sA), ("B", sB), ("C", sC)):
        set_state(m, s)
        mrr[name] = EV.evaluate_translation(m, valid, known)["filtered_mrr"]
    print("TRANSLATION POCKET %s: MRR A %.4f, B %.4f, C %.4f" % (kind, mrr["A"], mrr["B"], mrr["C"]))
    assert mrr["B"] > mrr["A"] + 1e-4 and mrr["A"] > mrr["C"] + 1e-4     # the order the test is about, checked first
    vp = EV.TranslationPocket(m, valid, known)
    assert list(vp.pocket) == list(sB)
    for t in vp.pocket.values():
        t.fill_(float("nan"))
    seen = []
    for i, s in enumerate((sA, sB, sC, sD), 1):
        set_state(m, s)
        if kind == "transr":
            m.t = 1000 + i
        vp.tick(10 * i)
        torch.cuda.synchronize()
        seen.append(({k: t.cpu().numpy().copy() for k, t in vp.pocket.items()}, float(vp.best)))
    assert same(state_of(m), sD)                                          # the model's own tensors are only read
    hist = vp.read()
    assert [s for s, _ in hist] == [10, 20, 30, 40]
    got = [h["filtered_mrr"] for _, h in hist]
    for name, g in zip("ABC", got):
        assert abs(g - float(F32(mrr[name]))) <= RT.MRR_TOL
    assert got[3] == got[1]
    assert [h["improved"] for _, h in hist] == [True, True, False, False] == RT.pocket(got)[1]
    assert same(seen[0][0], sA) and seen[0][1] == got[0]
    for i in (1, 2, 3):     # after B, after C (untouched), after B again with other optimiser state (a tie: untouched)
        assert same(seen[i][0], sB), i
        assert seen[i][1] == got[1]
    assert vp.restore() == 20
    assert same(state_of(m), sB)
    if kind == "transr":
        assert m.t == 1002                                                # the step count recorded at B's tick
    assert vp.restore() == 20                                             # idempotent


def test_all_bad_rows_leave_a_poisoned_pocket():
    """Rows whose ids are all out of range, through the raw calls of a tick: counts -1 and NaN distances, so nothing is
    counted, best stays 0, the flag 0, and ge_copy_if leaves a poisoned pocket untouched."""
    m = make("transd", seed=7)
    bad = torch.full((V, 3), E + 5, dtype=torch.int32, device="cuda")
    nb = torch.zeros(2 * V, dtype=torch.int32, device="cuda")
    nk = torch.zeros(2 * V, dtype=torch.int32, device="cuda")
    td = torch.zeros(2 * V, dtype=torch.float32, device="cuda")
    ws = torch.empty(m._ws_bytes("rank", V), dtype=torch.uint8, device="cuda")
    for k in (0, 1):
        out = m.rank_counts(bad, cand_is_head=bool(k), out=(nb[k * V:(k + 1) * V], nk[k * V:(k + 1) * V], td[k * V:(k + 1) * V]),
                            workspace=ws)
        assert out[0].data_ptr() == nb.data_ptr() + 4 * k * V            # the views themselves come back
    hist = torch.zeros(8, dtype=torch.float32, device="cuda")
    best = torch.zeros((), dtype=torch.float32, device="cuda")
    flag = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    S = torch.cuda.current_stream().cuda_stream
    _lib.call("ge_rank_metrics", nb.data_ptr(), nk.data_ptr(), td.data_ptr(), 2 * V, hist.data_ptr(), best.data_ptr(),
              flag.data_ptr(), S)
    state = m._pocket_tensors()
    pocket = {k: torch.full_like(t, float("nan")) for k, t in state.items()}
    _lib.call("ge_copy_if", flag.data_ptr(), *_lib.copy_if_args([t.data_ptr() for t in state.values()],
                                                               [pocket[k].data_ptr() for k in state],
                                                               [t.numel() for t in state.values()]), S)
    torch.cuda.synchronize()
    assert (nb == -1).all() and (nk == -1).all() and bool(torch.isnan(td).all())
    got = hist.cpu().numpy()
    assert np.isnan(got[:7]).all() and got[7] == 0
    assert float(best) == 0.0 and int(flag[0]) == 0
    assert all(bool(torch.isnan(p).all()) for p in pocket.values())


@pytest.mark.parametrize("kind,loss,optimizer", [("transe-l1", "hinge", "sgd"), ("transh", "self_adversarial", "adagrad"),
                                                 ("rotate-l1", "self_adversarial", "sgd"), ("transr", "hinge", "sgd")])
def test_ticks_do_not_train(kind, loss, optimizer):
    """run(5); tick; run(5) leaves every table, accumulator and loss bitwise what run(5); run(5) leaves."""
    train, valid, known = graph_of(kind)
    kw = dict(loss=loss, negatives=4, adversarial_temperature=0.5) if loss == "self_adversarial" else {}
    runs = []
    for ticking in (False, True):
        m = make(kind, seed=9)
        tr = m.trainer(train, 64, margin=1.5, learning_rate=0.02, seed=3, optimizer=optimizer, **kw)
        vp = EV.TranslationPocket(m, valid, known) if ticking else None
        a = tr.run(5)
        if ticking:
            vp.tick(tr.step_count)
        b = tr.run(5)
        runs.append((state_of(m), torch.cat([a, b]).cpu().numpy(), getattr(m, "t", None)))
        if ticking:
            (step, h), = vp.read()
            assert step == 5 and h["counted"] == 2 * V and h["improved"]
    assert same(runs[0][0], runs[1][0])
    assert np.array_equal(bits(runs[0][1]), bits(runs[1][1])) and np.isfinite(runs[0][1]).all()
    assert runs[0][2] == runs[1][2]
    assert len(runs[0][0]) == {"transe-l1": 2, "transh": 6, "rotate-l1": 2, "transr": 5}[kind]


def test_candidate_sets():
    train, valid, known = graph_of("transe-l1")
    m = make("transe-l2", seed=11)
    sets = {side: EV.CandidateSets.from_observed(np.arange(E), known, R, side) for side in ("tail", "head")}
    con = EV.evaluate_translation(m, valid, known, candidate_sets=sets)["constrained"]
    vp = EV.TranslationPocket(m, valid, known, candidate_sets=sets)
    vp.tick(1)
    (_, a), = vp.read()
    RT.check_metrics(got8(a), np.array([con[k] for k in RT.KEYS[:7]] + [2.0 * V]), "pocket candidate sets")
    free = EV.TranslationPocket(m, valid, known)
    free.tick(1)
    assert free.read()[0][1]["mean_raw_pos"] > a["mean_raw_pos"]         # the sets really restrict the candidates
    with pytest.raises(ValueError, match="candidate_sets"):
        EV.TranslationPocket(m, valid, known, candidate_sets={"tail": sets["tail"]})
    with pytest.raises(ValueError, match="CandidateSets"):
        EV.TranslationPocket(m, valid, known, candidate_sets={"tail": sets["tail"], "head": object()})
    q = make("rotate-l1")
    with pytest.raises(NotImplementedError, match="candidate sets"):
        EV.TranslationPocket(q, graph_of("rotate-l1")[1], None, candidate_sets=sets)


def test_host_errors_and_capacity():
    train, valid, known = graph_of("transe-l1")
    m = make("transe-l1")
    with pytest.raises(ValueError, match="empty"):
        EV.TranslationPocket(m, valid[:0], known)
    for col, bad in ((0, E), (1, -1), (2, R)):
        rows = valid.copy()
        rows[3, col] = bad
        with pytest.raises(ValueError, match="outside"):
            EV.TranslationPocket(m, rows, known)
    for rows in (0, -2):
        with pytest.raises(ValueError, match="rows"):
            EV.TranslationPocket(m, valid, known, rows=rows)
    wrong = {side: EV.KnownIndex(known, max(E, R) + 1, side, "cuda") for side in ("tail", "head")}
    with pytest.raises(ValueError, match="n_rows"):
        EV.TranslationPocket(m, valid, wrong)
    right = {side: EV.KnownIndex(known, max(E, R), side, "cuda") for side in ("tail", "head")}
    a, b = EV.TranslationPocket(m, valid, right, keep_state=False), EV.TranslationPocket(m, valid, known, keep_state=False)
    a.tick(0)
    b.tick(0)
    assert a.read()[0][1] == b.read()[0][1]                              # ready-made indices serve as the triples do
    vp = EV.TranslationPocket(m, valid, known, capacity=2)
    vp.tick(1)
    vp.tick(2)
    with pytest.raises(RuntimeError, match="read"):
        vp.tick(3)
    assert [s for s, _ in vp.read()] == [1, 2]
    vp.tick(3)
    assert [s for s, _ in vp.read()] == [3]


@pytest.mark.parametrize("kind", ["transe-l1", "rotate-l1"])
def test_enable_adagrad_after_construction_is_refused(kind):
    train, valid, known = graph_of(kind)
    m = make(kind)
    vp = EV.TranslationPocket(m, valid, known)
    vp.tick(1)
    m.enable_adagrad(0.1)
    with pytest.raises(RuntimeError, match="state tensors"):
        vp.tick(2)
    assert [s for s, _ in vp.read()] == [1]
    with pytest.raises(RuntimeError, match="state tensors"):
        vp.restore()
    vp = EV.TranslationPocket(m, valid, known)                           # built after it: the accumulators are pocketed
    assert list(vp.pocket) == ["ent", "rel", "adagrad_ent", "adagrad_rel"]
    m.enable_adagrad(0.3)                                                # refilled, same shapes: still the same set
    vp.tick(1)
    assert vp.read()[0][1]["improved"] and float(vp.pocket["adagrad_rel"].min()) == float(F32(0.3))
