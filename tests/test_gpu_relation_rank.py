"""Relation prediction (h, ?, t) on the MI355X: ge_transx_relation_rank / ge_transr_relation_rank against the fp64
oracle tests/relation_rank_ref.py and their own stored distances, the host layers over them (relation_ranks,
predict_relations, the drivers' flags) and the ComplEx / HolE route through the head-side sweep."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import relation_rank_ref as RL
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


def _host(m):
    return {k: v.cpu().numpy().astype(np.float64) for k, v in m.tables.items()}


def _cells(m, test, known):
    from graphembeddings_amd import evaluate as EV
    n_rows = max(m.n_ent, m.n_rel)
    idx = EV.KnownIndex(known, n_rows, "relation", "cuda")
    pos_of = torch.arange(n_rows, dtype=torch.int64, device="cuda")
    pos_of[m.n_rel:] = -1
    t = torch.as_tensor(test).cuda()
    return idx.cells(t[:, 0], t[:, 1], pos_of, m.n_rel)


def _run(m, test, known=None):
    """(n_before, n_known_before, true_dist, scores) of one native call, as numpy arrays."""
    off, rc = _cells(m, test, known) if known is not None else (None, None)
    out = m.relation_rank_counts(torch.as_tensor(test).cuda(), known_off=off, known_rc=rc, return_scores=True)
    return [x.cpu().numpy() for x in out]


def _tol(d_e, d_q, l1):
    """The issue's (2 d + 8) 2^-24 (x 2 for the squares) with 2 d = dim_e + dim_r: one rounding of w, a dot as long as
    the entity width, the fmaf, and a sum as long as the distance's width."""
    return (d_e + d_q + 8) * RL.U * (1 if l1 else 2)


def _chunk_rows(R):
    """Mirror of chunk_rows in ge_transx_relrank.hip: rows of one internal chunk of a call."""
    c = 65536
    while c > 1024 and c * R > 1 << 22:
        c >>= 1
    return c


def _wide_tile(R):
    """Mirror of the tile choice in ge_transx_relrank.hip (TransE / TransH / TransD): the tile with fewer padded
    relation slots, 64 x 64 when 8-relation tiles (512 rows x 8 relations) need as many."""
    wide, narrow = (R + 63) // 64 * 64, (R + 7) // 8 * 8
    return wide <= narrow


# ---------------------------------------------------------------- 1. exact fixture
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("l1", [True, False])
def test_exact_fixture_counts_and_self_consistency(model, l1):
    """Integer tables: counts equal the fp64 oracle exactly (ties on both sides of the target, known candidates tied
    with it, the target itself known, duplicate known triples); the stored distances are the fp64 ones, give the same
    counts and hold true_dist bitwise."""
    tabs, test, known = RL.tie_fixture(model)
    E, R = tabs["ent"].shape[0], tabs["rel"].shape[0]
    m = _model(model, E, R, tabs["ent"].shape[1], l1, d_r=tabs["rel"].shape[1])
    for k, v in tabs.items():
        m.tables[k].copy_(torch.as_tensor(v, dtype=torch.float32))
    nb, nk, td, sc = _run(m, test, known)
    D = RL.distances(model, tabs, test, l1)
    km = RL.known_mask(test, known, R)
    enb, enk = RL.counts(D, test[:, 2], km)
    assert np.array_equal(nb, enb) and np.array_equal(nk, enk)
    assert (nk > 0).any()
    assert np.array_equal(sc.astype(np.float64), D)
    i = np.arange(len(test))
    assert np.array_equal(td.view(np.int32), sc[i, test[:, 2]].view(np.int32))
    snb, snk = RL.counts(sc.astype(np.float64), test[:, 2], km)
    assert np.array_equal(nb, snb) and np.array_equal(nk, snk)
    raw, fil = m.relation_ranks(test, known)
    assert raw.dtype == np.int64 and fil.dtype == np.int64
    assert np.array_equal(raw, enb + 1) and np.array_equal(fil, enb + 1 - enk)


# ---------------------------------------------------------------- 2. random tables
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("l1", [True, False])
def test_random_tables_within_bound(model, l1):
    E, R, d, n = 60, 300, 16, 200
    m = _model(model, E, R, d, l1, seed=11)
    rng = np.random.default_rng(5)
    test = np.stack([rng.integers(0, E, n), rng.integers(0, E, n), rng.integers(0, R, n)], 1)
    known = np.stack([rng.integers(0, E, 3000), rng.integers(0, E, 3000), rng.integers(0, R, 3000)], 1)
    known = np.concatenate([known, test[:50]], 0)
    nb, nk, td, sc = _run(m, test, known)
    tabs = _host(m)
    D = RL.distances(model, tabs, test, l1)
    M = RL.distances(model, tabs, test, l1, magnitude=True)
    tol = (2 * d + 8) * RL.U * (1 if l1 else 2)
    err = np.abs(sc - D) / (tol * M)
    lo, hi = RL.count_bounds(D, M, test[:, 2], tol)
    i = np.arange(n)
    score = m.score(torch.as_tensor(test.astype(np.int32)).cuda()).cpu().numpy()
    gap = np.abs(td.astype(np.float64) - score) / (2 * tol * M[i, test[:, 2]])
    print(f"{model} l1={l1}: max |scores - D| / (tol M) = {err.max():.4f}, mean(lo == hi) = {np.mean(lo == hi):.4f}, "
          f"max |true_dist - score| / (2 tol M) = {gap.max():.4f}")
    assert np.all(np.abs(sc - D) <= tol * M)
    assert np.all(lo <= nb) and np.all(nb <= hi)
    assert np.mean(lo == hi) >= 0.9
    assert np.all(np.abs(td.astype(np.float64) - score) <= 2 * tol * M[i, test[:, 2]])
    # the counters are those of the stored distances
    assert np.array_equal(td.view(np.int32), sc[i, test[:, 2]].view(np.int32))
    snb, snk = RL.counts(sc.astype(np.float64), test[:, 2], RL.known_mask(test, known, R))
    assert np.array_equal(nb, snb) and np.array_equal(nk, snk) and (nk > 0).any()


# ---------------------------------------------------------------- 3. independence
@pytest.mark.parametrize("model", MODELS)
def test_ranks_do_not_depend_on_the_rows_beside(model):
    E, R, n = 90, 37, 2100
    m = _model(model, E, R, 12, seed=2)
    rng = np.random.default_rng(9)
    test = np.stack([rng.integers(0, E, n), rng.integers(0, E, n), rng.integers(0, R, n)], 1)
    known = test[rng.random(n) < 0.5]
    raw, fil = m.relation_ranks(test, known)
    assert (fil < raw).any()
    perm = rng.permutation(n)
    r2, f2 = m.relation_ranks(test[perm], known)
    assert np.array_equal(r2, raw[perm]) and np.array_equal(f2, fil[perm])
    for b in (1, 7, 1000):
        sub = test[:200] if b == 1 else test
        rb, fb = m.relation_ranks(sub, known, batch=b)
        assert np.array_equal(rb, raw[:len(sub)]) and np.array_equal(fb, fil[:len(sub)])
    r3, f3 = m.relation_ranks(test, known)
    assert np.array_equal(r3, raw) and np.array_equal(f3, fil)
    a = [x.cpu() for x in m.relation_rank_counts(torch.as_tensor(test).cuda(), return_scores=True)]
    b = [x.cpu() for x in m.relation_rank_counts(torch.as_tensor(test).cuda(), return_scores=True)]
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("model,R", [(m, R) for m in MODELS for R in (3, 64, 4100)])
def test_row_chunk_boundary(model, R):
    """One call of a few rows more than the launcher's internal chunk equals calls that end before the boundary, on
    the 64 x 64 tile (R = 64) and the narrow one (R = 3 with 65,536-row chunks, R = 4100 with 1,024-row ones)."""
    assert _wide_tile(R) == (R == 64)
    E, d = 50, 4
    n = _chunk_rows(R) + 37
    m = _model(model, E, R, d, seed=4)
    rng = np.random.default_rng(R)
    test = np.stack([rng.integers(0, E, n), rng.integers(0, E, n), rng.integers(0, R, n)], 1)
    last = np.repeat(test[-37:], 20, axis=0)                     # known relations of the rows past the boundary
    last[:, 2] = rng.integers(0, R, len(last))
    known = np.concatenate([test[rng.random(n) < 0.3], test[-37:], last], 0)
    raw, fil = m.relation_ranks(test, known)                     # (the default batch holds all rows: one call)
    half = _chunk_rows(R) // 2 + 5
    rb, fb = m.relation_ranks(test, known, batch=half)
    assert np.array_equal(raw, rb) and np.array_equal(fil, fb)
    tail = slice(n - 60, n)                                      # rows on both sides of the boundary, as a call of their own
    nb, nk, td, sc = _run(m, test[tail], known)
    assert np.array_equal(raw[tail], nb + 1) and np.array_equal(fil[tail], nb + 1 - nk)
    assert (fil[tail] < raw[tail]).any()
    tabs = _host(m)
    D = RL.distances(model, tabs, test[tail], True)
    M = RL.distances(model, tabs, test[tail], True, magnitude=True)
    assert np.all(np.abs(sc - D) <= _tol(d, d, True) * M)


# ---------------------------------------------------------------- 4. widths and edges
def _misalign(m):
    """Every table replaced by a copy that starts 4 bytes past a 16-byte boundary."""
    for k, t in m.tables.items():
        buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=t.device)
        v = buf[1:1 + t.numel()].view_as(t)
        v.copy_(t)
        m.tables[k] = v


def _check_against_oracle(m, model, test, known=None):
    tabs = _host(m)
    D = RL.distances(model, tabs, test, m.l1)
    M = RL.distances(model, tabs, test, m.l1, magnitude=True)
    tol = _tol(tabs["ent"].shape[1], tabs["rel"].shape[1], m.l1)
    nb, nk, td, sc = _run(m, test, known)
    assert np.all(np.abs(sc - D) <= tol * M)
    lo, hi = RL.count_bounds(D, M, test[:, 2], tol)
    assert np.all(lo <= nb) and np.all(nb <= hi)
    assert np.all(nk >= 0) and np.all(nk <= nb)
    i = np.arange(len(test))
    assert np.array_equal(td.view(np.int32), sc[i, test[:, 2]].view(np.int32))
    km = RL.known_mask(test, known, m.n_rel) if known is not None else None
    snb, snk = RL.counts(sc.astype(np.float64), test[:, 2], km)
    assert np.array_equal(nb, snb) and np.array_equal(nk, snk)
    return sc


@pytest.mark.parametrize("R", [9, 60])
@pytest.mark.parametrize("model,d", [(m, d) for m in MODELS for d in (1, 3, 4, 100, 128, 200, 1024)
                                     if not (m == "transr" and d > 256)] + [("transr", 256)])
def test_widths_and_variants(model, d, R):
    """Every width on both tiles (R = 9: 512 x 8; R = 60: 64 x 64 with idle relation lanes), TransR with
    dim_e != dim_r up to its largest, and the scalar path of a misaligned rel table: the aligned and the misaligned
    tables hold the same values, so the 4-wide and the scalar staging must agree bitwise."""
    E, n = 70, 40
    assert _wide_tile(R) == (R == 60)
    d_r = {1: 3, 3: 4, 4: 8, 100: 36, 128: 128, 200: 256, 256: 256}[d] if model == "transr" else d
    m = _model(model, E, R, d, l1=d % 2 == 0, seed=d, d_r=d_r if model == "transr" else None)
    rng = np.random.default_rng(d)
    test = np.stack([rng.integers(0, E, n), rng.integers(0, E, n), rng.integers(0, R, n)], 1)
    sc = _check_against_oracle(m, model, test, known=test[::3])
    assert m.tables["rel"].data_ptr() % 16 == 0
    _misalign(m)
    assert m.tables["rel"].data_ptr() % 16 == 4 and m.tables["ent"].data_ptr() % 16 == 4
    sc2 = _check_against_oracle(m, model, test, known=test[::3])
    assert np.array_equal(sc.view(np.int32), sc2.view(np.int32))


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("R", [1, 2, 18, 255, 257])
def test_relation_counts(model, R):
    E = 40
    m = _model(model, E, R, 8, seed=R)
    rng = np.random.default_rng(R)
    test = np.stack([rng.integers(0, E, 150), rng.integers(0, E, 150), rng.integers(0, R, 150)], 1)
    _check_against_oracle(m, model, test, known=test[::2])
    _check_against_oracle(m, model, test[:1])
    raw, fil = m.relation_ranks(test, test)
    assert np.all(raw <= R) and np.all(fil >= 1) and np.all(fil <= raw)


@pytest.mark.parametrize("model", MODELS)
def test_one_entity(model):
    """E = 1: h == t, w = 0."""
    R = 11
    m = _model(model, 1, R, 8, seed=1)
    test = np.stack([np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64), np.arange(R)], 1)
    _check_against_oracle(m, model, test, known=test[:4])
    raw, _ = m.relation_ranks(test)
    assert sorted(raw.tolist()) == list(range(1, R + 1))     # D_c depends on c alone: the R targets take the R ranks


# ---------------------------------------------------------------- 5. out-of-range ids
@pytest.mark.parametrize("model", MODELS)
def test_out_of_range_ids(model):
    m = _model(model, 20, 3, 8)
    for bad in ([[0, 20, 0]], [[-1, 1, 0]], [[0, 1, 3]], [[0, 1, -1]]):
        with pytest.raises(ValueError):
            m.relation_ranks(np.array(bad))
    t = torch.tensor([[0, 1, 0], [0, 25, 1], [2, 3, 2], [1, 2, 3]], dtype=torch.int32).cuda()
    nb, nk, td, sc = m.relation_rank_counts(t, return_scores=True)
    for row in (1, 3):
        assert nb[row].item() == -1 and nk[row].item() == -1 and bool(torch.isnan(td[row]))
        assert bool(torch.isnan(sc[row]).all())
    nb2, _, td2 = m.relation_rank_counts(t[[0, 2]])
    assert torch.equal(nb[[0, 2]], nb2) and torch.equal(td[[0, 2]], td2)
    with pytest.raises(ValueError):
        m.predict_relations(np.array([[0, 20]]), 2)
    with pytest.raises(ValueError):
        m.predict_relations(np.array([[0, 1]]), 0)
    with pytest.raises(ValueError):
        m.predict_relations(np.array([[0, 1, 2]]), 2)


# ---------------------------------------------------------------- 6. predict_relations
def _first_k(D, k, mask=None):
    """The first k relations of every row in ascending (D, id), masked cells skipped; padding -1 / +inf."""
    n, R = D.shape
    ids = np.full((n, k), -1, dtype=np.int64)
    dist = np.full((n, k), np.inf, dtype=np.float32)
    for i in range(n):
        cs = [c for c in sorted(range(R), key=lambda c: (D[i, c], c)) if mask is None or not mask[i, c]][:k]
        ids[i, :len(cs)] = cs
        dist[i, :len(cs)] = D[i, cs]
    return ids, dist


@pytest.mark.parametrize("model", MODELS)
def test_predict_relations_is_the_sort_of_the_stored_distances(model):
    E, R, n = 30, 23, 1100                                   # (more rows than one sorted chunk of 1024)
    m = _model(model, E, R, 8, seed=6)
    m.tables["rel"][5] = m.tables["rel"][2]                  # exact ties between relations
    for k in m.tables:
        if k != "rel" and m.tables[k].shape[0] == R:
            m.tables[k][5] = m.tables[k][2]
    rng = np.random.default_rng(2)
    pairs = np.stack([rng.integers(0, E, n), rng.integers(0, E, n)], 1)
    known = np.stack([pairs[:, 0], pairs[:, 1], rng.integers(0, R, n)], 1)[: n // 2]
    known = np.concatenate([known, np.stack([pairs[:40, 0], pairs[:40, 1], np.full(40, 2)], 1)], 0)
    tri = np.concatenate([pairs, np.zeros((n, 1), dtype=np.int64)], 1)
    sc = _run(m, tri)[3]
    assert np.array_equal(sc[:, 2].view(np.int32), sc[:, 5].view(np.int32))
    for k in (1, 5, R, R + 4):
        ids, dist = m.predict_relations(pairs, k)
        assert ids.dtype == np.int64 and dist.dtype == np.float32 and ids.shape == (n, k)
        eid, ed = _first_k(sc, k)
        assert np.array_equal(ids, eid) and np.array_equal(dist.view(np.int32), ed.view(np.int32))
        fid, fd = m.predict_relations(pairs, k, known=known, batch=300)
        eid, ed = _first_k(sc, k, RL.known_mask(tri, known, R))
        assert np.array_equal(fid, eid) and np.array_equal(fd.view(np.int32), ed.view(np.int32))
    assert np.all(ids[:, R:] == -1) and np.all(np.isinf(dist[:, R:])) and np.all(ids[:, :R] >= 0)
    assert np.all(fid[:40, -5:] == -1)                       # a known relation leaves one more slot of padding
    # with the same known set, entry j has filtered rank j + 1
    fid, _ = m.predict_relations(pairs, 6, known=known)
    for j in (0, 3, 5):
        _, fil = m.relation_ranks(np.stack([pairs[:, 0], pairs[:, 1], fid[:, j]], 1), known)
        assert np.array_equal(fil, np.full(n, j + 1))


# ---------------------------------------------------------------- 7. ComplEx and HolE
@pytest.mark.parametrize("model", ["complex", "hole"])
def test_complex_and_hole_relations_through_the_head_sweep(model):
    from graphembeddings_amd import evaluate as EV
    from graphembeddings_amd import hole as H
    from tests import topk_ref as TK
    d, N, R, n = 64, 300, 12, 150
    rng = np.random.default_rng(7)
    table = (rng.standard_normal((N, d)) * 0.2).astype(np.float32)
    table[3] = table[7]                                      # two relations tie exactly
    emb = torch.as_tensor(table).cuda()
    test = np.stack([rng.integers(R, N, n), rng.integers(R, N, n), rng.integers(0, R, n)], 1)
    test[:10, 2] = 7
    known = np.concatenate([np.stack([test[:, 0], test[:, 1], rng.integers(0, R, n)], 1), test[:20]], 0)
    raw, fil = EV.relation_ranks(emb, test, R, known, model=model)
    # the sweep's own losses of (c, t, h), c over the relation rows
    sweep_emb, sweep_model = (H.hole_to_spectral(emb.clone()), "hole_spectral") if model == "hole" else (emb, "complex")
    cand = torch.arange(R, dtype=torch.int32, device="cuda")
    hr = torch.as_tensor(test[:, [1, 0]].astype(np.int32)).cuda()
    L = H.rank_candidates(sweep_emb, hr, cand[:1].expand(n).contiguous(), cand, cand_is_head=True, return_scores=True,
                          model=sweep_model)[-1].cpu().numpy()
    # the swept loss of cell (row, c) is the model's loss of the triple (h, t, c), by the fp64 oracle on the real table
    # and at the tolerance the sweep's own tests use: the h <-> r exchange is the right one
    from oracle import hole_oracle as O
    score = O.hole_evaluate_triples if model == "hole" else O.evaluate_triples
    t64 = table.astype(np.float64)
    for c in range(R):
        tri_c = np.stack([test[:, 0], test[:, 1], np.full(n, c)], 1)
        assert np.abs(L[:, c] - score(tri_c, t64)[:, 0]).max() < 1e-5
    km = RL.known_mask(test, known, R)
    enb, enk = RL.counts(L.astype(np.float64), test[:, 2], km)
    assert np.array_equal(raw, enb + 1) and np.array_equal(fil, enb + 1 - enk)
    assert (enk > 0).any() and np.all(raw <= R)
    pairs = test[:, :2]
    for k in (3, R + 2):
        ids, ls = EV.predict_relations(emb, pairs, R, k, model=model)
        eid, el = TK.first_k_rows(L, np.arange(R), k)
        assert np.array_equal(ids, eid) and np.array_equal(ls, el)
        assert ids.max() < R and np.all((ids >= 0) | np.isinf(ls))
        fid, fl = EV.predict_relations(emb, pairs, R, k, known, model=model)
        eid, el = TK.first_k_rows(L, np.arange(R), k, km)
        assert np.array_equal(fid, eid) and np.array_equal(fl, el) and fid.max() < R


# ---------------------------------------------------------------- 8. drivers
def _write(path, rows, count=None):
    with open(path, "w") as f:
        f.write(f"{len(rows) if count is None else count}\n")
        for r in rows:
            f.write(" ".join(str(int(x)) for x in r) + "\n")


@pytest.mark.parametrize("mod,model,extra", [("transx_train", "transh", ["--model", "transh", "--hidden_size", "16"]),
                                             ("transr_train", "transr", ["--hidden_size_e", "16", "--hidden_size_r", "8"])])
def test_driver_relation_flags(tmp_path, mod, model, extra):
    E, R = 60, 7
    tri = XR.planted_kg(n_ent=E, n_rel=R, n_triples=600, seed=1)
    cut = int(0.9 * len(tri))
    d = tmp_path / "data"
    d.mkdir()
    _write(str(d / "entity2id.txt"), [], E)
    _write(str(d / "relation2id.txt"), [], R)
    _write(str(d / "triple2id.txt"), tri[:cut])
    _write(str(d / "test2id.txt"), tri[cut:])
    out = tmp_path / "out"
    p = subprocess.run(
        [sys.executable, "-m", f"graphembeddings_amd.{mod}", "--data_dir", str(d), "--nbatches", "5", "--train_times", "1",
         "--output_dir", str(out), "--test_file", str(d / "test2id.txt"), "--relation_ranks", "--predict_relations_k", "3",
         *extra], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert any(line.startswith("relation:") and "filtered MRR" in line for line in p.stdout.splitlines()), p.stdout
    j = json.load(open(out / f"{model}_test.json"))
    assert set(j["relation"]) == set(j["tail"]) and 0 < j["relation"]["filtered_mrr"] <= 1
    assert j["sweeps"] == 2 * (len(tri) - cut)               # the entity block is what it was
    lines = open(out / f"{model}_predict_relations.tsv").read().splitlines()
    pairs = {(int(h), int(t)) for h, t, _ in tri[cut:]}
    assert len(lines) == 3 * len(pairs)
    held = {tuple(int(x) for x in r) for r in tri[cut:]}
    seen_in_test = 0
    for i, line in enumerate(lines):
        h, t, pos, c, dist, in_test = line.split("\t")
        assert (int(h), int(t)) in pairs and int(pos) == i % 3 + 1 and 0 <= int(c) < R and float(dist) >= 0
        assert int(in_test) == ((int(h), int(t), int(c)) in held)
        seen_in_test += int(in_test)
    assert seen_in_test > 0                                  # the test file is not part of the prediction filter


# ---------------------------------------------------------------- 9. planted KG
def test_planted_kg_relation_mrr_improves():
    """The short TransE training of test_planted_kg_learns_by_filtered_rank: the filtered relation MRR of the held-out
    rows is higher after it than before."""
    from graphembeddings_amd import evaluate as EV
    tri = XR.planted_kg(seed=0)
    cut = int(0.9 * len(tri))
    train, held = tri[:cut], tri[cut:]
    m = _model("transe", 2000, 20, 32, seed=0)
    before = EV.evaluate_translation(m, held, tri, both_sides=False, relations=True)
    m.trainer(train, len(train) // 20, margin=1.0, learning_rate=0.01, seed=3).run(3000)
    after = EV.evaluate_translation(m, held, tri, both_sides=False, relations=True)
    print(f"planted KG filtered relation MRR {before['relation']['filtered_mrr']:.4f} -> "
          f"{after['relation']['filtered_mrr']:.4f}")
    assert "relation" not in EV.evaluate_translation(m, held[:50], tri, both_sides=False)
    assert after["relation"]["filtered_mrr"] > before["relation"]["filtered_mrr"]
