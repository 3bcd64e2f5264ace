"""Nearest-neighbour entity search (ge_neighbor_*, neighbors.nearest) on the MI355X against the fp64 contract
tests/neighbors_ref.py: stored distances within the per-cell bound, fused lists bit-equal to a (D, id) sort of the stored
distances, ties, planted clusters, bad inputs, the stored and torch routes, memory, reproducibility and the drivers."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import neighbors_ref as NR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ("cosine", "euclidean")


def _table(N, d, seed=0, spread=0.0):
    """float32 [N, d] rows; spread > 0: row norms from 10^-spread to 10^spread."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, d)).astype(np.float32)
    if spread:
        X *= (10.0 ** rng.uniform(-spread, spread, N)).astype(np.float32)[:, None] / np.sqrt(d).astype(np.float32)
    return X


def _dev(a, dtype=torch.int32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def _stored(T, q, planes, metric):
    """ge_neighbor_dists: [B, K] float32 (any query ids, out-of-range ones included)."""
    from graphembeddings_amd import _lib
    qd = _dev(q)
    out = torch.empty((len(q), planes.cand.numel()), dtype=torch.float32, device="cuda")
    _lib.call("ge_neighbor_dists", T.data_ptr(), T.shape[0], T.shape[1], qd.data_ptr(), len(q), planes.cand.data_ptr(),
              planes.cand.numel(), NB_METRIC[metric], planes.buffer.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out.cpu().numpy()


def _fused(T, q, planes, k, metric, exclude_self):
    """ge_neighbor_topk straight through the C ABI (any query ids)."""
    from graphembeddings_amd import _lib
    qd = _dev(q)
    B, K = len(q), planes.cand.numel()
    ws = torch.empty(int(_lib.load().ge_neighbor_workspace_bytes(B, K, k)), dtype=torch.uint8, device="cuda")
    oid = torch.empty((B, k), dtype=torch.int32, device="cuda")
    od = torch.empty((B, k), dtype=torch.float32, device="cuda")
    _lib.call("ge_neighbor_topk", T.data_ptr(), T.shape[0], T.shape[1], qd.data_ptr(), B, planes.cand.data_ptr(), K, k,
              NB_METRIC[metric], int(exclude_self), planes.buffer.data_ptr(), oid.data_ptr(), od.data_ptr(), ws.data_ptr(),
              ws.numel(), torch.cuda.current_stream().cuda_stream)
    return oid.cpu().numpy().astype(np.int64), od.cpu().numpy()


NB_METRIC = {"cosine": 0, "euclidean": 1}


def _sorted_lists(D, q, cand, k, exclude_self):
    """The contract's lists from stored distances, vectorised: excluded cells +inf, a stable lexsort by (D, id)."""
    D = D.copy()
    q, cand = np.asarray(q, dtype=np.int64), np.asarray(cand, dtype=np.int64)
    if exclude_self:
        D[cand[None, :] == q[:, None]] = np.inf
    C = np.broadcast_to(cand, D.shape)
    order = np.lexsort((C, D), axis=-1)[:, :k]
    ids, dist = np.take_along_axis(C, order, 1).copy(), np.take_along_axis(D, order, 1).copy()
    if ids.shape[1] < k:
        pad = k - ids.shape[1]
        ids = np.concatenate([ids, np.full((len(q), pad), -1, dtype=np.int64)], 1)
        dist = np.concatenate([dist, np.full((len(q), pad), np.inf, dtype=np.float32)], 1)
    ids[np.isinf(dist)] = -1
    bad = np.isnan(D).any(1)
    ids[bad], dist[bad] = -1, np.nan
    return ids, dist


def _same(a, b):
    """Bitwise equality of float arrays (NaN == NaN)."""
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


# ---- 1. stored distances against fp64, within the per-cell bound
@pytest.mark.parametrize("d", [1, 3, 8, 33, 56, 100, 128, 200, 257, 288])
@pytest.mark.parametrize("metric", METRICS)
def test_stored_distances_within_the_per_cell_bound(d, metric):
    from graphembeddings_amd import neighbors as NB
    X = _table(400, d, seed=d, spread=3.0)                 # row norms 1e-3 ... 1e3
    X[:5] = 0.0                                            # zero rows
    X[5:10] = X[10:15] * np.float32(2.5)                   # scaled copies
    X[15:20] = X[10:15] * np.float32(1e-3)
    rng = np.random.default_rng(d + 1)
    cand = rng.permutation(400)[:350]
    q = np.concatenate([np.arange(20), rng.integers(0, 400, 60)])
    T = torch.as_tensor(X).cuda()
    planes = NB.NeighborPlanes(T, cand)
    D = _stored(T, q, planes, metric)
    ref = NR.distances(X, q, cand, metric)
    bound = NR.dist_bound(X, q, cand, metric)
    err = np.abs(D.astype(np.float64) - ref)
    assert np.isfinite(D).all() and (D >= 0).all() and not np.signbit(D).any()
    assert (err <= bound).all(), f"worst excess {(err - bound).max():.3g} at {np.unravel_index((err - bound).argmax(), err.shape)}"
    zq = np.nonzero(q < 5)[0]                              # a zero row: cosine 1 to everything, Euclidean the other's norm
    if metric == "cosine":
        assert (D[zq] == 1.0).all()
    else:
        assert np.allclose(D[zq], np.sqrt((X[cand].astype(np.float64) ** 2).sum(1))[None, :], rtol=1e-6, atol=0)
    ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)    # (0 / 0 between two zero rows)
    print(f"d={d} {metric}: max err {err.max():.3g}, max err / bound {ratio.max():.3g}")


# ---- 2. fused top-k bit-equal to a stable (D, id) sort of the stored distances
CASES = [(1, 1, 1), (1, 6, 7), (1, 14951, 128), (1, 14951, 10), (127, 129, 100), (128, 6, 10), (129, 129, 128),
         (300, 14951, 7), (300, 14951, 128), (129, 14951, 1), (20000, 129, 10), (20000, 6, 7), (20000, 1, 1),
         (20000, 129, 128)]


@pytest.mark.parametrize("B,K,k", CASES)
@pytest.mark.parametrize("metric", METRICS)
def test_fused_topk_equals_the_sorted_stored_distances(B, K, k, metric):
    from graphembeddings_amd import neighbors as NB
    i = CASES.index((B, K, k))
    d = (33, 100, 200)[i % 3]
    N = K + 500
    X = _table(N, d, seed=i, spread=1.0)
    X[N - 3:] = X[:3]                                       # some exact ties
    rng = np.random.default_rng(i)
    cand = rng.permutation(N)[:K]                           # permuted order
    q = np.concatenate([cand[: min(K, B // 2 + 1)], rng.integers(0, N, B)])[:B]   # inside and outside the list
    T = torch.as_tensor(X).cuda()
    planes = NB.NeighborPlanes(T, cand)
    D = _stored(T, q, planes, metric)
    for excl in ((True, False) if B <= 300 else (i % 2 == 0,)):
        ids, dist = _fused(T, q, planes, k, metric, excl)
        want_ids, want_d = _sorted_lists(D, q, cand, k, excl)
        assert np.array_equal(ids, want_ids), (excl, np.argwhere(ids != want_ids)[:5])
        assert _same(dist, want_d), excl


# ---- 3. exact ties
@pytest.mark.parametrize("metric", METRICS)
def test_duplicates_come_out_in_id_order(metric):
    from graphembeddings_amd import neighbors as NB
    X = _table(500, 100, seed=3)
    for r in (40, 77, 301, 499):
        X[r] = X[5]                                         # row 5 and its four duplicates
    X[200] = X[100] = X[150]
    T = torch.as_tensor(X).cuda()
    ids, dist = NB.nearest(T, [5, 40, 150], 6, metric=metric, exclude_self=True)
    assert ids[0, :4].tolist() == [40, 77, 301, 499]        # the query's duplicates first, in id order
    assert ids[1, :4].tolist() == [5, 77, 301, 499]
    assert ids[2, :2].tolist() == [100, 200]
    assert dist[0, 0] == dist[0, 3] and dist[1, 0] == dist[1, 3]
    ids, _ = NB.nearest(T, [5], 6, metric=metric, exclude_self=False)
    assert ids[0, :5].tolist() == [5, 40, 77, 301, 499]
    ids, dist = NB.nearest(T, np.arange(500), 20, metric=metric)
    tie = dist[:, 1:] == dist[:, :-1]
    assert (ids[:, 1:][tie] > ids[:, :-1][tie]).all()


# ---- 4. planted clusters
@pytest.mark.parametrize("d", [100, 200])
@pytest.mark.parametrize("metric", METRICS)
def test_planted_clusters_are_found(d, metric):
    from graphembeddings_amd import neighbors as NB
    rng = np.random.default_rng(d)
    centres = rng.standard_normal((64, d))
    X = (np.repeat(centres, 32, 0) + 0.01 * rng.standard_normal((64 * 32, d))).astype(np.float32)
    perm = rng.permutation(64 * 32)                         # members scattered over the table
    X = X[perm]
    cluster = (np.arange(64 * 32) // 32)[perm]
    T = torch.as_tensor(X).cuda()
    ids, dist = NB.nearest(T, np.arange(64 * 32), 31, metric=metric)
    for r in range(64 * 32):
        mates = np.nonzero(cluster == cluster[r])[0]
        assert sorted(ids[r].tolist()) == sorted(set(mates.tolist()) - {r})
    assert (np.diff(dist, axis=1) >= 0).all()


# ---- 5. bad inputs
@pytest.mark.parametrize("metric", METRICS)
def test_bad_query_ids_and_nan_rows_through_the_abi(metric):
    from graphembeddings_amd import neighbors as NB
    X = _table(300, 64, seed=5)
    T = torch.as_tensor(X).cuda()
    planes = NB.NeighborPlanes(T, np.arange(300))
    q = np.array([3, -1, 300, 7, 1 << 30], dtype=np.int64)
    ids, dist = _fused(T, q, planes, 10, metric, True)
    assert (ids[[1, 2, 4]] == -1).all() and np.isnan(dist[[1, 2, 4]]).all()
    assert (ids[[0, 3]] >= 0).all() and np.isfinite(dist[[0, 3]]).all()
    D = _stored(T, q, planes, metric)
    assert np.isnan(D[[1, 2, 4]]).all() and np.isfinite(D[[0, 3]]).all()
    # a NaN candidate row: every query for which it is eligible gets -1 / NaN; exclude_self keeps the NaN row's own query
    # from being poisoned by itself only -- its own distances are NaN everywhere
    X[11, 4] = np.nan
    T2 = torch.as_tensor(X).cuda()
    planes2 = NB.NeighborPlanes(T2, np.arange(300))
    ids, dist = _fused(T2, np.array([3, 11, 200]), planes2, 5, metric, True)
    assert (ids == -1).all() and np.isnan(dist).all()
    planes3 = NB.NeighborPlanes(T2, np.delete(np.arange(300), 11))
    ids, dist = _fused(T2, np.array([3, 200]), planes3, 5, metric, True)       # not a candidate: no effect
    assert (ids >= 0).all() and np.isfinite(dist).all()


def test_bad_inputs_raise_on_the_host_through_nearest():
    from graphembeddings_amd import neighbors as NB
    T = torch.as_tensor(_table(100, 32)).cuda()
    for q in ([0, 100], [-1], [[1]]):
        with pytest.raises(ValueError):
            NB.nearest(T, q, 5)
    with pytest.raises(ValueError):
        NB.nearest(T, [0], 5, candidates=[1, 2, 2])
    with pytest.raises(ValueError):
        NB.nearest(T, [0], 5, candidates=[1, 200])
    with pytest.raises(ValueError):
        NB.nearest(T.double(), [0], 5)
    planes = NB.NeighborPlanes(T, np.arange(50))
    with pytest.raises(ValueError, match="another candidate list"):
        NB.nearest(T, [0], 5, candidates=np.arange(60), planes=planes)
    with pytest.raises(ValueError, match="another table"):
        NB.nearest(T.clone(), [0], 5, planes=planes)


# ---- 6. the stored and torch routes
@pytest.mark.parametrize("metric", METRICS)
def test_stored_route_extends_the_fused_lists(metric):
    from graphembeddings_amd import neighbors as NB
    X = _table(3000, 100, seed=6, spread=1.0)
    T = torch.as_tensor(X).cuda()
    rng = np.random.default_rng(6)
    cand = rng.permutation(3000)[:2500]
    q = rng.integers(0, 3000, 1500)                         # two stored chunks
    planes = NB.NeighborPlanes(T, cand)
    a_ids, a_d = NB.nearest(T, q, 128, candidates=cand, metric=metric, planes=planes)
    b_ids, b_d = NB.nearest(T, q, 200, candidates=cand, metric=metric, planes=planes)
    assert np.array_equal(a_ids, b_ids[:, :128]) and _same(a_d, b_d[:, :128])
    ids, dist = _sorted_lists(_stored(T, q, planes, metric), q, cand, 200, True)
    assert np.array_equal(ids, b_ids) and _same(dist, b_d)


@pytest.mark.parametrize("metric", METRICS)
def test_torch_route_is_bounded_against_fp64(metric):
    from graphembeddings_amd import neighbors as NB
    X = _table(1024, 300, seed=7, spread=1.0)
    X[:3] = 0.0
    T = torch.as_tensor(X).cuda()
    q, cand = np.arange(0, 1024, 3), np.arange(1024)
    ids, dist = NB.nearest(T, q, 10, metric=metric)
    ref = NR.distances(X, q, cand, metric)
    bound = NR.dist_bound(X, q, cand, metric, norm_adds=300)          # (torch's reductions: any order)
    rows = np.arange(len(q))[:, None]
    assert (ids >= 0).all()
    assert (np.abs(dist - ref[rows, ids]) <= bound[rows, ids]).all()
    ref_ids, ref_d = NR.topk_of(ref, q, cand, 10, True)
    assert (ref[rows, ids] <= ref_d[:, -1:] + 2 * bound.max()).all()    # the list is the true top 10, up to the bound
    assert np.mean(ids == ref_ids) > 0.99


# ---- 7. memory at 1.2 M candidates
def test_memory_stays_far_below_the_distance_matrix():
    from graphembeddings_amd import evaluate as EV
    from graphembeddings_amd import neighbors as NB
    N, d, B, k = 1_200_000, 200, 4096, 10
    g = torch.Generator(device="cuda").manual_seed(0)
    T = torch.randn((N, d), generator=g, device="cuda", dtype=torch.float32)
    q = np.random.default_rng(0).integers(0, N, B)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ids, dist = NB.nearest(T, q, k)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"nearest peak growth {grown / 1e6:.0f} MB against B*K*4 = {B * N * 4 / 1e6:.0f} MB")
    assert grown < B * N * 4 / 8
    assert (ids >= 0).all() and np.isfinite(dist).all()
    planes = NB.NeighborPlanes(T)
    sub = q[:64]
    D = torch.as_tensor(_stored(T, sub, planes, "cosine")).cuda()
    cells = (torch.arange(64).cuda(), torch.as_tensor(sub).cuda())     # candidates = every row: column = row id
    s_ids, s_d = EV._topk_of_losses(D, planes.cand64, k, cells)
    assert np.array_equal(s_ids.cpu().numpy(), ids[:64]) and _same(s_d.cpu().numpy(), dist[:64])


# ---- 8. reproducibility
@pytest.mark.parametrize("metric", METRICS)
def test_two_identical_calls_agree_bitwise(metric):
    from graphembeddings_amd import neighbors as NB
    X = _table(14951, 200, seed=8, spread=1.0)
    T = torch.as_tensor(X).cuda()
    q = np.random.default_rng(8).integers(0, 14951, 300)
    planes = NB.NeighborPlanes(T)
    a = _fused(T, q, planes, 100, metric, True)
    b = _fused(T, q, planes, 100, metric, True)
    assert np.array_equal(a[0], b[0]) and _same(a[1], b[1])
    assert _same(_stored(T, q[:50], planes, metric), _stored(T, q[:50], planes, metric))
    c = NB.nearest(T, q, 100, metric=metric)
    assert np.array_equal(a[0], c[0]) and _same(a[1], c[1])


# ---- 9. drivers
def test_train_driver_writes_neighbors_tsv(tmp_path):
    from graphembeddings_amd import data as D
    from graphembeddings_amd import neighbors as NB
    from graphembeddings_amd import train as T
    from tests.test_gpu_train_eval import _toy_kg
    dd = tmp_path / "data"
    dd.mkdir()
    data_dir = _toy_kg(dd)
    out = tmp_path / "run"
    out.mkdir()
    emb = torch.as_tensor(_table(122, 32, seed=9)).cuda()
    T.save_checkpoint(str(out), emb, 0)
    argv = ["--data_dir", data_dir, "--output_dir", str(out), "--embedding_dim", "32"]
    T.main(argv + ["--neighbors", "5"])
    lines = open(out / "neighbors.tsv").read().splitlines()
    data = D.init_inference_data(data_dir, min_mentions=None)
    R, E = data.relation_count, data.entity_count
    assert len(lines) == (E - R) * 5
    first = lines[0].split("\t")
    assert first[0] == str(R) and first[1] == data.id_to_metadata[R] and first[2] == "1"
    ids, dist = NB.nearest(emb, np.arange(R, E), 5, candidates=np.arange(R, E))
    want = NB.neighbor_lines(np.arange(R, E), ids, dist, data.id_to_metadata)
    assert [l + "\n" for l in lines] == want
    assert all(int(l.split("\t")[3]) >= R for l in lines)          # candidates are entity rows
    (tmp_path / "ids.txt").write_text(f"{R + 4}\n{R + 7}\n")
    T.main(argv + ["--neighbors", "3", "--neighbors_of", str(tmp_path / "ids.txt"), "--neighbors_metric", "euclidean"])
    lines = open(out / "neighbors.tsv").read().splitlines()
    assert len(lines) == 6 and lines[0].startswith(f"{R + 4}\t") and lines[3].startswith(f"{R + 7}\t")
    for extra in (["--gpus", "2"], ["--infer"]):
        with pytest.raises(SystemExit):
            T.main(argv + ["--neighbors", "5"] + extra)


def _write(path, rows, count=None):
    with open(path, "w") as f:
        f.write(f"{len(rows) if count is None else count}\n")
        for r in rows:
            f.write(" ".join(str(int(x)) for x in r) + "\n")


def test_transx_driver_writes_neighbors_tsv(tmp_path):
    from graphembeddings_amd import neighbors as NB
    from graphembeddings_amd import transx as X
    from tests import transx_ref as XR
    tri = XR.planted_kg(n_ent=300, n_rel=5, n_triples=3000, seed=1)
    d = tmp_path / "data"
    d.mkdir()
    _write(str(d / "entity2id.txt"), [], 300)
    _write(str(d / "relation2id.txt"), [], 5)
    _write(str(d / "triple2id.txt"), tri)
    p = subprocess.run(
        [sys.executable, "-m", "graphembeddings_amd.transx_train", "--data_dir", str(d), "--nbatches", "5", "--output_dir",
         str(tmp_path / "a"), "--train_times", "1", "--neighbors_k", "3", "--model", "transe", "--hidden_size", "16"],
        cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    lines = open(tmp_path / "a" / "transe_neighbors.tsv").read().splitlines(keepends=True)
    assert len(lines) == 300 * 3
    m = X.TransX("transe", 300, 5, 16)
    m.load_state_dict(torch.load(tmp_path / "a" / "transe.pt", map_location="cpu"))
    ids, dist = NB.nearest(m.tables["ent"].contiguous(), np.arange(300), 3)
    assert lines == NB.neighbor_lines(np.arange(300), ids, dist)
