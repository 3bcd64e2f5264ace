"""Top-k prediction, host side: the heap restatement's write set on hand-built cases, the TSV line format, and the
workspace contract of ge_topk_1vK_planes (host-only calls; no GPU)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_ref as T  # noqa: E402


def _lines(pops, h, r, true_set):
    from graphembeddings_amd import evaluate as E
    return E.inference_lines(h, r, [i for _, i in pops], [l for l, _ in pops], true_set)


def _driver_lines(losses, ids, h, r, K, true_set, thr):
    """What the driver writes for one query: the raw pops up to the K-th filtered one, if the lowest loss is below thr."""
    pops = T.heap_pops(losses, ids)
    if not pops[0][0] < thr:
        return []
    n_fil = m = 0
    for l, i in pops:
        m += 1
        if i not in true_set:
            n_fil += 1
            if n_fil == K:
                break
    return _lines(pops[:m], h, r, true_set)


def test_write_set_exact_ties_break_by_id():
    losses = np.float32([0.3, 0.1, 0.3, 0.1, 0.2])
    ids = [9, 7, 4, 8, 5]
    got = T.write_set(losses, ids, 1, 2, 4, set(), 0.5)
    assert [int(l.split("\t")[2]) for l in got] == [7, 8, 5, 4]
    assert got == _driver_lines(losses, ids, 1, 2, 4, set(), 0.5)


def test_write_set_known_pops_before_between_and_after_the_kth():
    losses = np.float32([0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07])
    ids = [10, 11, 12, 13, 14, 15, 16]
    known = {10, 12, 14}                     # before the first, between, and right after the K-th filtered pop
    got = T.write_set(losses, ids, 3, 0, 2, known, 0.5)
    assert [l.split("\t")[2] for l in got] == ["10", "11", "12", "13"]
    assert [l.rstrip("\n").split("\t")[4] for l in got] == ["True", "False", "True", "False"]
    assert got == _driver_lines(losses, ids, 3, 0, 2, known, 0.5)
    # K beyond the known ones: every pop up to the K-th filtered one
    assert T.write_set(losses, ids, 3, 0, 3, known, 0.5) == _driver_lines(losses, ids, 3, 0, 3, known, 0.5)


def test_write_set_fewer_candidates_than_k_and_non_confident():
    losses = np.float32([0.2, 0.1])
    ids = [5, 6]
    assert T.write_set(losses, ids, 0, 1, 10, {5}, 0.5) == _driver_lines(losses, ids, 0, 1, 10, {5}, 0.5)
    assert len(T.write_set(losses, ids, 0, 1, 10, {5}, 0.5)) == 2
    assert T.write_set(losses, ids, 0, 1, 10, set(), 0.1) == []            # lowest loss 0.1 is not below 0.1
    assert _driver_lines(losses, ids, 0, 1, 10, set(), 0.1) == []


def test_tsv_line_format_character_for_character():
    pops = [(np.float32(0.0123456789), 17), (np.float32(0.5), 3)]
    got = "".join(_lines(pops, 4, 1, {3}))
    assert got == "0.012346\t4\t17\t1\tFalse\n0.500000\t4\t3\t1\tTrue\n"
    assert got == "".join(T.write_set(np.float32([0.0123456789, 0.5]), [17, 3], 4, 1, 5, {3}, 0.9))


def test_first_k_rows_equals_heap():
    """Test scaffolding only: the vectorised restatement the GPU tests compare against equals the literal heap."""
    rng = np.random.default_rng(0)
    losses = rng.choice(np.float32([0.1, 0.2, 0.3, 0.25]), size=(6, 40)).astype(np.float32)
    ids = rng.permutation(100)[:40]
    mask = rng.random((6, 40)) < 0.2
    for k in (1, 5, 40, 45):
        oid, ol = T.first_k_rows(losses, ids, k, mask)
        for b in range(6):
            hid, hl = T.first_k(losses[b], ids, k, set(ids[mask[b]].tolist()))
            assert np.array_equal(oid[b], hid) and np.array_equal(ol[b], hl)


def test_topk_workspace_contract_host_only():
    from graphembeddings_amd import _lib, build
    build.build()
    lib = _lib.load()
    assert lib.ge_version() >= 360
    assert lib.ge_topk_max_k() >= 128
    ws = lambda B, K, k: int(lib.ge_topk_workspace_bytes(B, K, k))
    B, K = 59071, 14951
    assert 0 < ws(B, K, 128) < B * K * 4 / 8
    prev = 0
    for b in (1, 64, 127, 128, 129, 300, 1024, 20000, 32639, 32640, 32769, 40000, B, 2 * B):
        assert ws(b, K, 10) >= prev
        prev = ws(b, K, 10)
    for kk in range(1, 129):
        assert ws(1000, K, kk) >= ws(1000, K, max(1, kk - 1))
    for kc in (1, 10, 128, 129, 14951, 1_200_000):
        assert ws(64, kc, 10) >= ws(64, max(1, kc // 2), 10)
    assert ws(64, K, 129) == 0 and ws(64, K, 0) == 0


def test_predict_k_refuses_several_gpus():
    import pytest
    from graphembeddings_amd import train as TT
    with pytest.raises(SystemExit, match="predict_k"):
        TT.main(["--data_dir", "x", "--output_dir", "y", "--infer", "--predict_k", "3", "--gpus", "2"])


def test_driver_write_set_with_long_raw_lists(tmp_path, monkeypatch):
    """evaluate.predict_inference_results' bookkeeping -- the K-th filtered pop, its raw position m, the raw top-m in
    chunks of like m, the lines -- against the heap restatement, with the sweeps replaced by a fixed loss matrix.  Raw
    lists longer than hole.topk_max_k() (the chunked fallback): K > 128, and K = 3 behind 150 known pops."""
    import types
    from collections import defaultdict

    import torch

    from graphembeddings_amd import evaluate as E
    from graphembeddings_amd import hole as H
    rng = np.random.default_rng(4)
    R, N = 2, 302
    cand = np.arange(R, N)
    heads = rng.choice(cand, 40, replace=False)
    test = np.stack([np.repeat(heads, 2), rng.choice(cand, 80), np.tile([0, 1], 40)], 1)
    queries = test[:, [0, 2]]                                   # (already distinct, in order)
    losses = rng.choice(np.linspace(0.01, 0.99, 200).astype(np.float32), size=(len(queries), len(cand)))
    row_of = {(int(h), int(r)): i for i, (h, r) in enumerate(queries)}
    known = []
    for i, (h, r) in enumerate(queries):
        if i % 2 == 0:                                          # 150 known tails among the lowest losses
            best = cand[np.lexsort((cand, losses[i]))[:150]]
            known += [[h, t, r] for t in best]
        else:
            known += [[h, t, r] for t in rng.choice(cand, 5, replace=False)]
    known = np.array(known, dtype=np.int64)
    true = {}
    for h, t, r in known:
        true.setdefault(int(h), {}).setdefault(int(r), set()).add(int(t))

    def fake_predict(emb, q, c, k, known_triples=None, **kw):
        rows = [row_of[(int(h), int(r))] for h, r in q]
        mask = None
        if known_triples is not None:
            mask = np.array([[int(t) in true.get(int(h), {}).get(int(r), set()) for t in c] for h, r in q])
        return TR_first_k_rows(losses[rows], c, k, mask)

    def fake_scores(emb, hr, c, **kw):
        return torch.as_tensor(losses[[row_of[(int(h), int(r))] for h, r in hr.tolist()]])

    TR_first_k_rows = T.first_k_rows
    monkeypatch.setattr(E, "predict_links", fake_predict)
    monkeypatch.setattr(E, "KnownIndex", lambda *a, **kw: "train + valid")
    monkeypatch.setattr(H, "score_candidates", fake_scores)
    monkeypatch.setattr(H, "topk_max_k", lambda: 128)
    true_dd = defaultdict(lambda: defaultdict(set), {h: defaultdict(set, v) for h, v in true.items()})
    data = types.SimpleNamespace(relation_count=R, entity_count=N, test_array=test, triples=known, validation_triples=None,
                                 true_triples=true_dd)
    emb = torch.zeros(N, 40)                                    # (d = 40: the unfused bookkeeping, on the host)
    for K, thr in ((3, 0.5), (130, 0.9), (200, 1.0)):
        path = str(tmp_path / f"out{K}.tsv")
        res = E.predict_inference_results(emb, data, K, thr, path, log=lambda *a: None)
        expect = []
        for i, (h, r) in enumerate(queries):
            expect += T.write_set(losses[i], cand, h, r, K, true.get(int(h), {}).get(int(r), set()), thr)
        assert open(path).read() == "".join(expect)
        assert res["lines"] == len(expect) and len(expect) > 0
    # the K = 3 lists run past 128 pops for the rows with 150 known tails ahead
    assert len(T.write_set(losses[0], cand, queries[0][0], queries[0][1], 3, true[int(queries[0][0])][0], 1.0)) > 128
