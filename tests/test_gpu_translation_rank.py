"""Link-prediction ranks of TransE / TransH / TransD / TransR (ge_transx_rank / ge_transr_rank) on the MI355X against
the fp64 oracle tests/translation_rank_ref.py, the stored distances of the same sweep, and each other."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import translation_rank_ref as RK
from tests import transx_ref as XR

pytestmark = pytest.mark.gpu
MODELS = ("transe", "transh", "transd", "transr")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(model, E, R, d, l1=True, seed=0, d_r=None):
    if model == "transr":
        from graphembeddings_amd import transr as TR
        return TR.TransR(E, R, d, d if d_r is None else d_r, l1=l1, seed=seed)
    from graphembeddings_amd import transx as X
    return X.TransX(model, E, R, d, l1=l1, seed=seed)


def _load(m, tabs):
    for k, v in tabs.items():
        m.tables[k].copy_(torch.as_tensor(v, dtype=torch.float32))


def _host(m):
    return {k: v.cpu().numpy().astype(np.float64) for k, v in m.tables.items()}


def _fixture_model(model, l1, seed=0, **kw):
    tabs, test, known = RK.tie_fixture(model, seed=seed, **kw)
    E, R = tabs["ent"].shape[0], tabs["rel"].shape[0]
    if model == "transr":
        m = _model(model, E, R, tabs["ent"].shape[1], l1, d_r=tabs["rel"].shape[1])
    else:
        m = _model(model, E, R, tabs["ent"].shape[1], l1)
    _load(m, tabs)
    return m, tabs, test, known


def _cells(m, test, known, side):
    from graphembeddings_amd import evaluate as EV
    n_rows = max(m.n_ent, m.n_rel)
    idx = EV.KnownIndex(known, n_rows, side, "cuda")
    pos_of = torch.arange(n_rows, dtype=torch.int64, device="cuda")
    pos_of[m.n_ent:] = -1
    t = torch.as_tensor(test).cuda()
    return idx.cells(t[:, 0 if side == "tail" else 1], t[:, 2], pos_of, m.n_ent)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("side", ["tail", "head"])
def test_exact_fixture_counts_and_self_consistency(model, l1, side):
    """Integer tables: counts equal the fp64 oracle exactly (ties on both sides of the target, a known candidate tied
    with it, the target itself known, duplicate known triples); the sweep's stored distances give the same counts and
    hold true_dist bitwise."""
    m, tabs, test, known = _fixture_model(model, l1)
    off, rc = _cells(m, test, known, side)
    nb, nk, td, sc = m.rank_counts(torch.as_tensor(test).cuda(), cand_is_head=side == "head", known_off=off,
                                   known_rc=rc, return_scores=True)
    nb, nk, td, sc = nb.cpu().numpy(), nk.cpu().numpy(), td.cpu().numpy(), sc.cpu().numpy()
    D = RK.distances(model, tabs, test, side, l1)
    tid = RK.true_ids(test, side)
    km = RK.known_mask(test, known, m.n_ent, side)
    enb, enk = RK.counts(D, tid, km)
    assert np.array_equal(nb, enb) and np.array_equal(nk, enk)
    assert (nk > 0).any() and (enb > enk).any()
    assert np.array_equal(sc.astype(np.float64), D)
    # self-consistency with the stored row
    i = np.arange(len(test))
    assert np.array_equal(td.view(np.int32), sc[i, tid].view(np.int32))
    snb, snk = RK.counts(sc.astype(np.float64), tid, km)
    assert np.array_equal(nb, snb) and np.array_equal(nk, snk)
    raw, fil = m.ranks(test, known, side=side)
    assert np.array_equal(raw, enb + 1) and np.array_equal(fil, enb + 1 - enk)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("side", ["tail", "head"])
def test_random_tables_within_bound_and_self_consistent(model, l1, side):
    E, R, d, n = 300, 6, 16, 200
    m = _model(model, E, R, d, l1, seed=11)
    rng = np.random.default_rng(5)
    test = np.stack([rng.integers(0, E, n), rng.integers(0, E, n), rng.integers(0, R, n)], 1)
    known = np.stack([rng.integers(0, E, 3000), rng.integers(0, E, 3000), rng.integers(0, R, 3000)], 1)
    known = np.concatenate([known, test[:50]], 0)
    off, rc = _cells(m, test, known, side)
    nb, nk, td, sc = [x.cpu().numpy() for x in m.rank_counts(torch.as_tensor(test).cuda(), cand_is_head=side == "head",
                                                             known_off=off, known_rc=rc, return_scores=True)]
    tabs = _host(m)
    D = RK.distances(model, tabs, test, side, l1)
    M = RK.distances(model, tabs, test, side, l1, magnitude=True)
    tid = RK.true_ids(test, side)
    tol = (2 * d + 8) * RK.U * (1 if l1 else 2)           # gamma_n of the dE-long projection and d-long sum
    lo, hi = RK.count_bounds(D, M, tid, tol)
    assert np.all(lo <= nb) and np.all(nb <= hi)
    assert np.mean(lo == hi) >= 0.9
    assert np.all(np.abs(sc - D) <= tol * M)
    i = np.arange(n)
    assert np.array_equal(td.view(np.int32), sc[i, tid].view(np.int32))
    km = RK.known_mask(test, known, E, side)
    snb, snk = RK.counts(sc.astype(np.float64), tid, km)
    assert np.array_equal(nb, snb) and np.array_equal(nk, snk)
    # the sweep's D of the true triple against the score kernel's
    score = m.score(torch.as_tensor(test.astype(np.int32)).cuda()).cpu().numpy()
    assert np.all(np.abs(td.astype(np.float64) - score) <= 2 * tol * M[i, tid])


@pytest.mark.parametrize("model", MODELS)
def test_ranks_do_not_depend_on_grouping(model):
    E, R, n = 257, 9, 2100
    m = _model(model, E, R, 12, seed=2)
    rng = np.random.default_rng(9)
    test = np.stack([rng.integers(0, E, n), rng.integers(0, E, n), rng.integers(0, R, n)], 1)
    known = test[rng.random(n) < 0.5]
    for side in ("tail", "head"):
        raw, fil = m.ranks(test, known, side=side)
        perm = rng.permutation(n)
        r2, f2 = m.ranks(test[perm], known, side=side)
        assert np.array_equal(r2, raw[perm]) and np.array_equal(f2, fil[perm])
        for b in (1, 7, 1000):
            sub = test[:300] if b == 1 else test
            rb, fb = m.ranks(sub, known, side=side, batch=b)
            assert np.array_equal(rb, raw[:len(sub)]) and np.array_equal(fb, fil[:len(sub)])
        r3, f3 = m.ranks(test, known, side=side)
        assert np.array_equal(r3, raw) and np.array_equal(f3, fil)
        # one call with the rows in the caller's order (no grouping) gives the same counts
        nb, nk, _ = m.rank_counts(torch.as_tensor(test[perm]).cuda(), cand_is_head=side == "head",
                                  known_off=None, known_rc=None)
        assert np.array_equal(nb.cpu().numpy() + 1, raw[perm])


def _variant(ent, d_e, d_q):
    """Mirror of rank_vec4 in ge_transx_rank.hip: 4-wide entity loads iff both widths are multiples of 4 and ent is
    16-byte aligned."""
    return 4 if d_e % 4 == 0 and d_q % 4 == 0 and ent.data_ptr() % 16 == 0 else 1


def _misalign(m):
    """Every table replaced by a copy that starts 4 bytes past a 16-byte boundary."""
    for k, t in m.tables.items():
        buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=t.device)
        v = buf[1:1 + t.numel()].view_as(t)
        v.copy_(t)
        m.tables[k] = v


def _check_against_oracle(m, model, test, side="tail", known=None):
    tabs = _host(m)
    l1 = m.l1
    D = RK.distances(model, tabs, test, side, l1)
    M = RK.distances(model, tabs, test, side, l1, magnitude=True)
    tid = RK.true_ids(test, side)
    d = tabs["ent"].shape[1] + tabs["rel"].shape[1]
    lo, hi = RK.count_bounds(D, M, tid, 4.0 * (2 * d + 8) * RK.U * 2)
    raw, fil = m.ranks(test, known, side=side)
    assert np.all(lo + 1 <= raw) and np.all(raw <= hi + 1)
    assert np.all(fil >= 1) and np.all(fil <= raw)
    return lo, hi


@pytest.mark.parametrize("model,d", [(m, d) for m in MODELS for d in (1, 3, 4, 100, 128, 200, 1024)
                                     if not (m == "transr" and d > 256)])      # TransR tables are at most 256 wide
def test_widths_and_variants(model, d):
    E, R, n = 70, 3, 40
    d_r = {1: 3, 3: 4, 4: 8, 100: 36, 128: 128, 200: 256}.get(d, d) if model == "transr" else d
    m = _model(model, E, R, d, l1=d % 2 == 0, seed=d, d_r=d_r if model == "transr" else None)
    rng = np.random.default_rng(d)
    test = np.stack([rng.integers(0, E, n), rng.integers(0, E, n), rng.integers(0, R, n)], 1)
    seen = set()
    for misaligned in (False, True):
        if misaligned:
            _misalign(m)
        seen.add(_variant(m.tables["ent"], d, d_r))
        for side in ("tail", "head"):
            _check_against_oracle(m, model, test, side)
    want = {1} if (d % 4 or d_r % 4) else {1, 4}
    assert seen == want


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("E", [1, 2, 255, 257])
def test_entity_counts_and_single_rows(model, E):
    R = 4
    m = _model(model, E, R, 8, seed=E)
    rng = np.random.default_rng(E)
    test = np.stack([rng.integers(0, E, 30), rng.integers(0, E, 30), rng.integers(0, R, 30)], 1)
    _check_against_oracle(m, model, test)
    _check_against_oracle(m, model, test[:1], "head")
    raw, fil = m.ranks(test, test, side="tail")
    assert np.all(raw <= E) and np.all(fil >= 1)


@pytest.mark.parametrize("model", MODELS)
def test_one_relation_and_every_row_its_own(model):
    E, n = 130, 64
    rng = np.random.default_rng(3)
    m = _model(model, E, n, 8, seed=3)
    one = np.stack([rng.integers(0, E, n), rng.integers(0, E, n), np.full(n, 5)], 1)
    own = np.stack([rng.integers(0, E, n), rng.integers(0, E, n), rng.permutation(n)], 1)
    for test in (one, own):
        for side in ("tail", "head"):
            _check_against_oracle(m, model, test, side, known=test[::3])


@pytest.mark.parametrize("model", MODELS)
def test_out_of_range_ids(model):
    m = _model(model, 20, 3, 8)
    for bad in ([[0, 20, 0]], [[-1, 1, 0]], [[0, 1, 3]]):
        with pytest.raises(ValueError):
            m.ranks(np.array(bad), side="tail")
    # the native call marks the row, and the rows beside it are unaffected
    t = torch.tensor([[0, 1, 0], [0, 25, 1], [2, 3, 2]], dtype=torch.int32).cuda()
    nb, nk, td = m.rank_counts(t)
    assert nb[1].item() == -1 and nk[1].item() == -1 and bool(torch.isnan(td[1]))
    nb2, _, _ = m.rank_counts(t[[0, 2]])
    assert torch.equal(nb[[0, 2]], nb2)
    with pytest.raises(ValueError):
        m.ranks(np.array([[0, 1]]))
    with pytest.raises(ValueError):
        m.ranks(np.array([[0, 1, 0]]), side="both")


def test_planted_kg_learns_by_filtered_rank():
    """TransE d=32 on the planted KG of test_gpu_transx.test_planted_kg_learns, measured by filtered rank over all
    entities (both sides): the mean rank falls below 0.1 E and Hits@10 grows tenfold."""
    from graphembeddings_amd import evaluate as EV
    tri = XR.planted_kg(seed=0)
    E = 2000
    cut = int(0.9 * len(tri))
    train, held = tri[:cut], tri[cut:]
    m = _model("transe", E, 20, 32, seed=0)
    before = EV.evaluate_translation(m, held, tri)
    m.trainer(train, len(train) // 20, margin=1.0, learning_rate=0.01, seed=3).run(3000)
    after = EV.evaluate_translation(m, held, tri)
    print(f"planted KG filtered mean rank {before['mean_filtered_pos']:.1f} -> {after['mean_filtered_pos']:.1f}, "
          f"hits@10 {before['hits10']:.2f} -> {after['hits10']:.2f} %")
    assert after["sweeps"] == 2 * len(held)
    assert before["mean_filtered_pos"] > 0.3 * E
    assert after["mean_filtered_pos"] < 0.1 * E
    assert after["hits10"] >= 10 * max(before["hits10"], 0.1)


def _write(path, rows, count=None):
    with open(path, "w") as f:
        f.write(f"{len(rows) if count is None else count}\n")
        for r in rows:
            f.write(" ".join(str(int(x)) for x in r) + "\n")


@pytest.mark.parametrize("mod,model,extra", [("transx_train", "transe", ["--model", "transe", "--hidden_size", "16"]),
                                             ("transr_train", "transr", ["--hidden_size_e", "16", "--hidden_size_r", "8"])])
def test_driver_evaluates_and_reloads(tmp_path, mod, model, extra):
    tri = XR.planted_kg(n_ent=300, n_rel=5, n_triples=3000, seed=1)
    cut = int(0.9 * len(tri))
    d = tmp_path / "data"
    d.mkdir()
    _write(str(d / "entity2id.txt"), [], 300)
    _write(str(d / "relation2id.txt"), [], 5)
    _write(str(d / "triple2id.txt"), tri[:cut])
    _write(str(d / "test2id.txt"), tri[cut:])
    _write(str(d / "valid2id.txt"), tri[cut:cut + 20])
    run = lambda out, more: subprocess.run(
        [sys.executable, "-m", f"graphembeddings_amd.{mod}", "--data_dir", str(d), "--nbatches", "5", "--output_dir",
         str(out), "--test_file", str(d / "test2id.txt"), "--filter_file", str(d / "valid2id.txt"), *extra, *more],
        cwd=ROOT, capture_output=True, text=True, timeout=300)
    p = run(tmp_path / "a", ["--train_times", "2"])
    assert p.returncode == 0, p.stderr
    for side in ("tail:", "head:", "both:"):
        assert any(line.startswith(side) and "filtered MRR" in line for line in p.stdout.splitlines()), p.stdout
    j1 = json.load(open(tmp_path / "a" / f"{model}_test.json"))
    assert j1["sweeps"] == 2 * (len(tri) - cut)
    p2 = run(tmp_path / "b", ["--train_times", "0", "--load", str(tmp_path / "a" / f"{model}.pt")])
    assert p2.returncode == 0, p2.stderr
    j2 = json.load(open(tmp_path / "b" / f"{model}_test.json"))
    assert j1 == j2
