"""Top-k tail / head prediction of TransE / TransH / TransD / TransR (ge_transx_topk / ge_transr_topk, predict) on the
MI355X against the fp64 oracle tests/translation_rank_ref.py, the rank sweep's stored distances and its ranks."""
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


def _queries(test, side):
    test = np.asarray(test, dtype=np.int64)
    return np.stack([test[:, 0] if side == "tail" else test[:, 1], test[:, 2]], 1)


def _walk(D, queries, side, k, known=()):
    """fp64 reference: per row sorted(range(E), key=(D, c)), known cells skipped, first k, padded -1 / +inf."""
    ks = {tuple(int(x) for x in t) for t in np.asarray(known, dtype=np.int64).reshape(-1, 3)}
    E = D.shape[1]
    ids = np.full((len(queries), k), -1, dtype=np.int64)
    dist = np.full((len(queries), k), np.inf)
    for i, (f, r) in enumerate(queries):
        out = [c for c in sorted(range(E), key=lambda c: (D[i, c], c))
               if ((int(f), c, int(r)) if side == "tail" else (c, int(f), int(r))) not in ks][:k]
        ids[i, :len(out)] = out
        dist[i, :len(out)] = D[i, out]
    return ids, dist


def _stored(m, queries, side, known=None):
    """(ids, dist) of the stable (D, id) sort of rank_counts(return_scores=True) with known cells removed."""
    from graphembeddings_amd import evaluate as EV
    q = torch.as_tensor(np.asarray(queries, dtype=np.int64)).cuda()
    zero = torch.zeros_like(q[:, 0])
    tri = torch.stack([zero, q[:, 0], q[:, 1]] if side == "head" else [q[:, 0], zero, q[:, 1]], 1)
    D = m.rank_counts(tri, cand_is_head=(side == "head"), return_scores=True)[-1]
    cells = None
    if known is not None:
        idx = EV.KnownIndex(known, max(m.n_ent, m.n_rel), side, "cuda")
        pos_of = torch.arange(max(m.n_ent, m.n_rel), dtype=torch.int64, device="cuda")
        pos_of[m.n_ent:] = -1
        off, rc = idx.cells(q[:, 0], q[:, 1], pos_of, m.n_ent)
        cells = EV._known_cells_rc(off, rc, m.n_ent)
    ids, dist = EV._topk_of_losses(D, torch.arange(m.n_ent, device="cuda"), m.n_ent, cells)
    return ids.cpu().numpy(), dist.cpu().numpy()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("side", ["tail", "head"])
def test_exact_ties_against_the_fp64_walk(model, l1, side):
    tabs, test, known = RK.tie_fixture(model)
    E, R = tabs["ent"].shape[0], tabs["rel"].shape[0]
    m = _model(model, E, R, tabs["ent"].shape[1], l1, d_r=tabs["rel"].shape[1] if model == "transr" else None)
    _load(m, tabs)
    q = _queries(test, side)
    D = RK.distances(model, _host(m), test, side, l1)
    for kn in (None, known):
        for k in (1, 3, E - 1, E, E + 5):
            ids, dist = m.predict(q, k, known=kn, side=side)
            rid, rdist = _walk(D, q, side, k, () if kn is None else kn)
            np.testing.assert_array_equal(ids, rid, err_msg=f"k={k} known={kn is not None}")
            np.testing.assert_array_equal(dist, rdist.astype(np.float32))


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("side", ["tail", "head"])
def test_random_tables_bitwise_and_filtered_rank(model, l1, side):
    E, R, n = 3001, 7, 300
    m = _model(model, E, R, 24, l1, seed=3, d_r=16 if model == "transr" else None)
    rng = np.random.default_rng(5)
    test = np.stack([rng.integers(0, E, n), rng.integers(0, E, n), rng.integers(0, R, n)], 1)
    known = np.concatenate([test, np.stack([rng.integers(0, E, 4 * n), rng.integers(0, E, 4 * n),
                                            rng.integers(0, R, 4 * n)], 1)])
    q = _queries(test, side)
    for k in (1, 10, 128):
        ids, dist = m.predict(q, k, known=known, side=side)
        sid, sdist = _stored(m, q, side, known)
        np.testing.assert_array_equal(ids, sid[:, :k])
        assert dist.tobytes() == sdist[:, :k].astype(np.float32).tobytes()
    # the j-th returned candidate has filtered rank j + 1 under the same known set
    ids, dist = m.predict(q[:40], 10, known=known, side=side)
    j = np.arange(10)
    rows = np.repeat(np.arange(40), 10)
    f, r, c = q[rows, 0], q[rows, 1], ids.reshape(-1)
    tri = np.stack([f, c, r] if side == "tail" else [c, f, r], 1)
    _, fil = m.ranks(tri, known, side=side)
    np.testing.assert_array_equal(fil, np.tile(j + 1, 40))
    # distances within the fp64 bound
    D = RK.distances(model, _host(m), tri, side, l1)
    M = RK.distances(model, _host(m), tri, side, l1, magnitude=True)
    ii = np.arange(len(tri))
    want = D[ii, tri[:, 1] if side == "tail" else tri[:, 0]]
    tol = 1e-5 * M[ii, tri[:, 1] if side == "tail" else tri[:, 0]] + 1e-30
    assert np.all(np.abs(dist.reshape(-1) - want) <= tol)


@pytest.mark.parametrize("model", MODELS)
def test_grouping_independence(model):
    E, R = 1500, 6
    m = _model(model, E, R, 20, seed=1)
    rng = np.random.default_rng(2)
    q = np.stack([rng.integers(0, E, 100), rng.integers(0, R, 100)], 1)
    ids, dist = m.predict(q, 16)
    ids2, dist2 = m.predict(q, 16)
    assert ids.tobytes() == ids2.tobytes() and dist.tobytes() == dist2.tobytes()
    perm = rng.permutation(len(q))
    ids3, dist3 = m.predict(q[perm], 16)
    np.testing.assert_array_equal(ids3, ids[perm])
    assert dist3.tobytes() == dist[perm].tobytes()
    # rows passed unsorted to the kernel (interleaved relations), and row by row
    i4, d4 = m.topk_candidates(torch.as_tensor(q).cuda(), 16)
    np.testing.assert_array_equal(i4.cpu().numpy(), ids)
    for i in (0, 17, 99):
        i5, d5 = m.topk_candidates(torch.as_tensor(q[i:i + 1]).cuda(), 16)
        np.testing.assert_array_equal(i5.cpu().numpy()[0], ids[i])
        assert d5.cpu().numpy()[0].tobytes() == dist[i].tobytes()


@pytest.mark.parametrize("model,d", [(m, d) for m in MODELS for d in (1, 3, 4, 100, 1024 if m != "transr" else 256)])
def test_widths_and_variants(model, d):
    E = 700
    m = _model(model, E, 3, d, seed=4, d_r=max(1, d // 2) if model == "transr" else None)
    q = np.stack([np.arange(0, E, 37), np.arange(0, E, 37) % 3], 1)
    ids, dist = m.predict(q, 12, side="head")
    sid, sdist = _stored(m, q, "head")
    np.testing.assert_array_equal(ids, sid[:, :12])
    assert dist.tobytes() == sdist[:, :12].tobytes()
    if d % 4 == 0:                                        # a misaligned ent: the VEC 1 path
        big = torch.empty(E * d + 1, device="cuda")
        view = big[1:].view(E, d)
        view.copy_(m.tables["ent"])
        m.tables["ent"] = view
        i2, d2 = m.predict(q, 12, side="head")
        np.testing.assert_array_equal(i2, ids)
        assert d2.tobytes() == dist.tobytes()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("E", [1, 2, 255, 257])
def test_entity_counts(model, E):
    m = _model(model, E, 2, 8, seed=6)
    q = np.stack([np.arange(E) % E, np.arange(E) % 2], 1)
    for k in (1, E, E + 3):
        ids, dist = m.predict(q, k)
        sid, sdist = _stored(m, q, "tail")
        kk = min(k, E)
        np.testing.assert_array_equal(ids[:, :kk], sid[:, :kk])
        assert (ids[:, kk:] == -1).all() and np.isinf(dist[:, kk:]).all()


@pytest.mark.parametrize("B", [1, 64])
def test_many_candidates_ranges_and_merge(B):
    E = 200_000
    m = _model("transe", E, 4, 16, seed=7)
    rng = np.random.default_rng(8)
    q = np.stack([rng.integers(0, E, B), rng.integers(0, 4, B)], 1)
    sid, sdist = _stored(m, q, "tail")
    for k in (1, 10, 128):
        ids, dist = m.predict(q, k)
        np.testing.assert_array_equal(ids, sid[:, :k])
        assert dist.tobytes() == sdist[:, :k].tobytes()


def test_rows_whose_every_candidate_is_known_and_bad_ids():
    from graphembeddings_amd import _lib
    E = 300
    m = _model("transh", E, 3, 8, seed=9)
    known = np.array([[5, c, 1] for c in range(E)])
    ids, dist = m.predict([[5, 1], [6, 1]], 4, known=known)
    assert (ids[0] == -1).all() and np.isinf(dist[0]).all()
    assert (ids[1] >= 0).all()
    with pytest.raises(ValueError):
        m.predict([[E, 0]], 4)
    with pytest.raises(ValueError):
        m.predict([[0, 3]], 4)
    ids, dist = m.topk_candidates(torch.tensor([[E, 0], [1, 1], [0, -1]], device="cuda"), 4)
    ids, dist = ids.cpu().numpy(), dist.cpu().numpy()
    assert (ids[[0, 2]] == -1).all() and np.isnan(dist[[0, 2]]).all()
    assert (ids[1] >= 0).all()
    for k in (0, _lib.load().ge_transx_topk_max_k() + 1):
        with pytest.raises(ValueError):
            m.topk_candidates(torch.zeros(1, 2, dtype=torch.int32, device="cuda"), k)


@pytest.mark.parametrize("model", MODELS)
def test_nan_rows_and_the_fallback_agree(model):
    E = 400
    m = _model(model, E, 3, 8, seed=10)
    m.tables["ent"][17, 0] = float("nan")
    q = np.array([[3, 0], [17, 1], [4, 2]])
    known = np.array([[4, 17, 2], [17, 4, 2]])             # row 2's NaN candidate is known on both sides: skipped
    for side in ("tail", "head"):
        a = m.predict(q, 9, known=known, side=side)
        b = m.predict(q, 9, known=known, side=side, fused=False)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        assert (a[0][:2] == -1).all() and np.isnan(a[1][:2]).all()
        assert (a[0][2] >= 0).all() and 17 not in a[0][2]


@pytest.mark.parametrize("model", MODELS)
def test_large_k_and_unfused_agree_with_the_kernel(model):
    from graphembeddings_amd import transx as X
    kmax = X.topk_max_k()
    E = 1200
    m = _model(model, E, 4, 12, seed=11)
    rng = np.random.default_rng(12)
    q = np.stack([rng.integers(0, E, 50), rng.integers(0, 4, 50)], 1)
    known = np.stack([rng.integers(0, E, 300), rng.integers(0, E, 300), rng.integers(0, 4, 300)], 1)
    ids, dist = m.predict(q, kmax, known=known, side="head")
    big_i, big_d = m.predict(q, kmax + 70, known=known, side="head")
    un_i, un_d = m.predict(q, kmax, known=known, side="head", fused=False)
    np.testing.assert_array_equal(big_i[:, :kmax], ids)
    assert big_d[:, :kmax].tobytes() == dist.tobytes()
    np.testing.assert_array_equal(un_i, ids)
    assert un_d.tobytes() == dist.tobytes()


def test_no_score_matrix_at_fb15k_shape():
    E, R, B, k = 14951, 1345, 59071, 128
    m = _model("transe", E, R, 100, seed=13)
    rng = np.random.default_rng(14)
    q = np.stack([rng.integers(0, E, B), rng.integers(0, R, B)], 1)
    known = np.stack([np.repeat(q[:, 0], 4), rng.integers(0, E, 4 * B), np.repeat(q[:, 1], 4)], 1)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ids, _ = m.predict(q, k, known=known)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"predict peak growth {grown / 1e6:.0f} MB against B*E*4/8 = {B * E * 4 / 8 / 1e6:.0f} MB")
    assert grown < B * E * 4 / 8
    assert ids.shape == (B, k) and (ids[:, 0] >= 0).all()


def _write(path, rows, count=None):
    with open(path, "w") as f:
        f.write(f"{len(rows) if count is None else count}\n")
        for r in rows:
            f.write(" ".join(str(int(x)) for x in r) + "\n")


@pytest.mark.parametrize("mod,model,extra", [("transx_train", "transe", ["--model", "transe", "--hidden_size", "16"]),
                                             ("transr_train", "transr", ["--hidden_size_e", "16", "--hidden_size_r", "8"])])
def test_driver_writes_the_prediction_file(tmp_path, mod, model, extra):
    from graphembeddings_amd import evaluate as EV
    tri = XR.planted_kg(n_ent=300, n_rel=5, n_triples=3000, seed=1)
    cut = int(0.9 * len(tri))
    d = tmp_path / "data"
    d.mkdir()
    _write(str(d / "entity2id.txt"), [], 300)
    _write(str(d / "relation2id.txt"), [], 5)
    _write(str(d / "triple2id.txt"), tri[:cut])
    _write(str(d / "test2id.txt"), tri[cut:])
    _write(str(d / "valid2id.txt"), tri[cut:cut + 20])
    K = 5
    p = subprocess.run(
        [sys.executable, "-m", f"graphembeddings_amd.{mod}", "--data_dir", str(d), "--nbatches", "5", "--output_dir",
         str(tmp_path / "a"), "--test_file", str(d / "test2id.txt"), "--filter_file", str(d / "valid2id.txt"),
         "--train_times", "2", "--predict_k", str(K), *extra], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    lines = open(tmp_path / "a" / f"{model}_predict.tsv").read().splitlines(keepends=True)
    # the same lines from predict() on the saved model, under the driver's filter
    if model == "transr":
        from graphembeddings_amd import transr as TR
        m = TR.TransR(300, 5, 16, 8)
    else:
        from graphembeddings_amd import transx as X
        m = X.TransX("transe", 300, 5, 16)
    m.load_state_dict(torch.load(tmp_path / "a" / f"{model}.pt", map_location="cpu"))
    test, flt = tri[cut:], np.concatenate([tri[:cut], tri[cut:cut + 20]])
    want = []
    for side, cols in (("tail", [0, 2]), ("head", [1, 2])):
        qs = EV.distinct_pairs(test[:, cols])
        ids, dist = m.predict(qs, K, known=flt, side=side)
        want += EV.translation_predict_lines(side, qs, ids, dist, test)
        # every test triple outside the filter with filtered rank <= K sits at exactly that position, in_test = 1
        fset = {tuple(t) for t in flt.tolist()}
        free = np.array([t for t in test.tolist() if tuple(t) not in fset])
        _, fil = m.ranks(free, flt, side=side)
        pos = {(int(q[0]), int(q[1])): i for i, q in enumerate(qs)}
        for t, rk in zip(free, fil):
            if rk <= K:
                f, c = (t[0], t[1]) if side == "tail" else (t[1], t[0])
                row = pos[(int(f), int(t[2]))]
                assert ids[row, rk - 1] == c
                line = EV.translation_predict_lines(side, qs[row:row + 1], ids[row:row + 1], dist[row:row + 1], test)
                assert line[rk - 1].endswith("\t1\n")
    assert lines == want


def test_planted_kg_top10_finds_held_out_tails():
    from graphembeddings_amd import evaluate as EV
    tri = XR.planted_kg(seed=0)
    cut = int(0.9 * len(tri))
    train, held = tri[:cut], tri[cut:]
    m = _model("transe", 2000, 20, 32, seed=0)

    def found():
        qs = held[:, [0, 2]]
        ids, _ = m.predict(qs, 10, known=train)
        return float(np.mean([(ids[i] == held[i, 1]).any() for i in range(len(held))]))
    before = found()
    m.trainer(train, len(train) // 20, margin=1.0, learning_rate=0.01, seed=3).run(3000)
    after = found()
    print(f"planted KG: held-out tail in the top 10 {100 * before:.2f} % -> {100 * after:.2f} %")
    assert after >= 10 * max(before, 0.002)
