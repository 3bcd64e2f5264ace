"""GPU: top-k prediction (ge_topk_1vK_planes, hole.topk_candidates, evaluate.predict_links, train.py --predict_k)
against the reference's heap (tests/topk_ref.py) fed with the rank sweep's own losses."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu


def _table(N, d, seed=1):
    """test_gpu_ranks_equal_reference_heap_semantics' construction: exact duplicates and near-duplicates a few ulps
    apart (inside the raw-score bracket)."""
    rng = np.random.default_rng(seed)
    table = (rng.standard_normal((N, d)) * 0.2).astype(np.float32)
    table[50] = table[51]
    table[60] = table[61]
    for j in range(70, 90):
        table[j] = table[52] * np.float32(1.0 + 2e-7 * (j - 79.5))
    return table


def _sweep_losses(emb, hr, cand, side, model="complex"):
    from graphembeddings_amd import hole as H
    tid = cand[:1].expand(hr.shape[0]).contiguous()
    return H.rank_candidates(emb, hr, tid, cand, cand_is_head=(side == "head"), return_scores=True, model=model)[-1]


def _known(emb_n, hr_np, cand_np, rng, per_row=5):
    rows = np.repeat(np.arange(len(hr_np)), per_row)
    other = rng.choice(cand_np, size=rows.size)
    return np.stack([hr_np[rows, 0], other, hr_np[rows, 1]], 1)


def _known_mask(kn, hr_np, cand_np, side):
    """[B, K] known-true cells straight from the known triples (h, t, r): the candidate completes a known triple."""
    ks = set(map(tuple, np.asarray(kn).tolist()))
    if side == "tail":
        return np.array([[(int(f), int(c), int(r)) in ks for c in cand_np] for f, r in hr_np], dtype=bool)
    return np.array([[(int(c), int(f), int(r)) in ks for c in cand_np] for f, r in hr_np], dtype=bool)


CASES = [  # (d, k, B, K)
    (56, 1, 1, 1), (56, 7, 300, 129), (64, 10, 129, 9), (64, 100, 128, 100), (104, 128, 127, 14951),
    (104, 7, 1, 6), (200, 10, 300, 14951), (200, 128, 129, 129), (200, 1, 128, 14951), (232, 100, 1, 14951),
    (232, 128, 300, 127), (256, 7, 127, 14951), (256, 10, 129, 10), (288, 128, 300, 14951), (288, 100, 128, 99),
]


@pytest.mark.parametrize("d,k,B,K", CASES)
@pytest.mark.parametrize("side", ["tail", "head"])
def test_gpu_topk_equals_heap_over_sweep_losses(d, k, B, K, side):
    from graphembeddings_amd import evaluate as E
    from graphembeddings_amd import hole as H
    rng = np.random.default_rng(d + k + B + K)
    R, N = 5, max(K, 200) + 100
    table = _table(N, d)
    emb = torch.as_tensor(table).cuda()
    special = np.array([50, 51, 60, 61] + list(range(52, 53)) + list(range(70, 90)))    # ties and near-ties first
    rest = rng.permutation(np.setdiff1d(np.arange(R, N), special))
    cand_np = rng.permutation(np.concatenate([special, rest])[:K])
    cand = torch.as_tensor(cand_np.astype(np.int32)).cuda()
    hr_np = np.stack([rng.integers(R, N, B), rng.integers(0, R, B)], 1)
    hr_np[0] = [52, 1]
    hr = torch.as_tensor(hr_np.astype(np.int32)).cuda()
    losses = _sweep_losses(emb, hr, cand, side).cpu().numpy()
    # raw
    ids, ls = H.topk_candidates(emb, hr, cand, k, cand_is_head=(side == "head"))
    eid, el = TR.first_k_rows(losses, cand_np, k)
    assert np.array_equal(ids.cpu().numpy(), eid) and np.array_equal(ls.cpu().numpy(), el)
    # filtered: known cells from a KnownIndex, as the rank sweep takes them
    kn = _known(N, hr_np, cand_np, rng)
    if side == "head":
        kn = kn[:, [1, 0, 2]]
    index = E.KnownIndex(kn, N, side, emb.device)
    pos_of = torch.full((N,), -1, dtype=torch.int64, device="cuda")
    pos_of[cand.to(torch.int64)] = torch.arange(K, device="cuda")
    fixed, rel = hr[:, 0].to(torch.int64), hr[:, 1].to(torch.int64)
    off, rc = index.cells(fixed, rel, pos_of, K)
    fid, fl = H.topk_candidates(emb, hr, cand, k, known_off=off, known_rc=rc, cand_is_head=(side == "head"))
    mask = _known_mask(kn, hr_np, cand_np, side)
    eid, el = TR.first_k_rows(losses, cand_np, k, mask)
    assert np.array_equal(fid.cpu().numpy(), eid) and np.array_equal(fl.cpu().numpy(), el)
    # agreement with the rank sweep: the j-th filtered pop has filtered rank j + 1
    fid_np = fid.cpu().numpy()
    for j in sorted({0, k // 2, k - 1}):
        ok = fid_np[:, j] >= 0
        if not ok.any():
            continue
        sel = torch.as_tensor(np.nonzero(ok)[0]).cuda()
        # (the known-cell lists are per call: rebuilt for the selected rows)
        o2, r2 = index.cells(fixed[sel], rel[sel], pos_of, K)
        nb, nk = H.rank_candidates(emb, hr[sel], torch.as_tensor(fid_np[ok, j]).cuda(), cand, known_off=o2, known_rc=r2,
                                   cand_is_head=(side == "head"))
        raw = nb.cpu().numpy() + 1
        assert np.array_equal(raw - nk.cpu().numpy(), np.full(ok.sum(), j + 1))
        m_rows = mask[ok]
        key_l, key_i = losses[ok], cand_np[None, :]
        ref_l, ref_i = fl.cpu().numpy()[ok, j][:, None], fid_np[ok, j][:, None]
        before = (key_l < ref_l) | ((key_l == ref_l) & (key_i < ref_i))
        assert np.array_equal(raw, j + 1 + (before & m_rows).sum(1))     # raw = filtered + the known pops before it


def test_gpu_topk_hole_real_table_equals_spectral_sweep_heap():
    from graphembeddings_amd import evaluate as E
    from graphembeddings_amd import hole as H
    rng = np.random.default_rng(3)
    R, N, d, k = 4, 700, 64, 10
    emb = torch.as_tensor(_table(N, d, seed=3)).cuda()
    cand_np = np.arange(R, N)
    q = np.stack([rng.integers(R, N, 150), rng.integers(0, R, 150)], 1)
    for side in ("tail", "head"):
        ids, ls = E.predict_links(emb, q, cand_np, k, side=side, model="hole")
        spec = H.hole_to_spectral(emb.clone())
        losses = _sweep_losses(spec, torch.as_tensor(q.astype(np.int32)).cuda(), torch.as_tensor(cand_np.astype(np.int32)).cuda(),
                               side, model="hole_spectral").cpu().numpy()
        eid, el = TR.first_k_rows(losses, cand_np, k)
        assert np.array_equal(ids, eid) and np.array_equal(ls, el)


def test_gpu_topk_edges_padding_bad_rows_fallbacks_planes_determinism():
    from graphembeddings_amd import _lib
    from graphembeddings_amd import evaluate as E
    from graphembeddings_amd import hole as H
    rng = np.random.default_rng(5)
    R, N, d = 3, 400, 64
    emb = torch.as_tensor(_table(N, d, seed=5)).cuda()
    cand_np = np.arange(R, 20)
    q = np.stack([rng.integers(R, N, 130), rng.integers(0, R, 130)], 1)
    # fewer eligible than k: padding; every candidate known: all padding
    kn = np.stack([np.repeat(q[:, 0], 5), rng.choice(cand_np, 5 * len(q)), np.repeat(q[:, 1], 5)], 1)
    ids, ls = E.predict_links(emb, q, cand_np, 30, known_triples=kn)
    n_el = len(cand_np) - np.array([len(set(kn[(kn[:, 0] == h) & (kn[:, 2] == r), 1])) for h, r in q])
    for i in range(len(q)):
        assert (ids[i, :n_el[i]] >= 0).all() and (ids[i, n_el[i]:] == -1).all() and np.isinf(ls[i, n_el[i]:]).all()
    # ids out of range raise in Python, and give -1 / NaN rows through the raw ABI
    cand = torch.as_tensor(cand_np.astype(np.int32)).cuda()
    with pytest.raises(ValueError):
        H.topk_candidates(emb, torch.tensor([[N, 0]], dtype=torch.int32).cuda(), cand, 5)
    with pytest.raises(ValueError):
        H.topk_candidates(emb, torch.tensor([[5, 0]], dtype=torch.int32).cuda(), torch.tensor([5, 5], dtype=torch.int32).cuda(), 1)
    hr = torch.tensor([[5, 0], [N + 3, 0], [6, -1], [7, 1]], dtype=torch.int32).cuda()
    k = 4
    oid = torch.empty(4, k, dtype=torch.int32, device="cuda")
    ol = torch.empty(4, k, dtype=torch.float32, device="cuda")
    nb = int(_lib.load().ge_topk_workspace_bytes(4, cand.numel(), k))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    _lib.call("ge_topk_1vK_planes", emb.data_ptr(), N, d, hr.data_ptr(), 4, cand.data_ptr(), cand.numel(), 1.0, 0, 0, None,
              None, k, oid.data_ptr(), ol.data_ptr(), None, ws.data_ptr(), nb, H._stream())
    oid, ol = oid.cpu().numpy(), ol.cpu().numpy()
    assert (oid[1:3] == -1).all() and np.isnan(ol[1:3]).all()
    good = H.topk_candidates(emb, hr[[0, 3]], cand, k)
    assert np.array_equal(oid[[0, 3]], good[0].cpu().numpy()) and np.array_equal(ol[[0, 3]], good[1].cpu().numpy())
    oid2 = torch.empty(4, k, dtype=torch.int32, device="cuda")
    ol2 = torch.empty(4, k, dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.GeError):       # short workspace: GE_ENOMEM
        _lib.call("ge_topk_1vK_planes", emb.data_ptr(), N, d, hr.data_ptr(), 4, cand.data_ptr(), cand.numel(), 1.0, 0, 0,
                  None, None, k, oid2.data_ptr(), ol2.data_ptr(), None, ws.data_ptr(), nb - 1, H._stream())
    # k > ge_topk_max_k() and d = 40 / 48: the fallbacks, against their own losses' heap
    big = np.arange(R, N)
    kbig = H.topk_max_k() + 5
    ids, ls = E.predict_links(emb, q, big, kbig)
    losses = _sweep_losses(emb, torch.as_tensor(q.astype(np.int32)).cuda(), torch.as_tensor(big.astype(np.int32)).cuda(), "tail")
    eid, el = TR.first_k_rows(losses.cpu().numpy(), big, kbig)
    assert np.array_equal(ids, eid) and np.array_equal(ls, el)
    for dd in (40, 48):
        e2 = torch.as_tensor(_table(N, dd, seed=dd)).cuda()
        ids, ls = E.predict_links(e2, q, big, 10, side="head")
        sc = H.score_candidates(e2, torch.as_tensor(q.astype(np.int32)).cuda(), torch.as_tensor(big.astype(np.int32)).cuda(),
                                cand_is_head=True).cpu().numpy()
        eid, el = TR.first_k_rows(sc, big, 10)
        assert np.array_equal(ids, eid) and np.array_equal(ls, el)
    # planes built once == per call; two identical calls are bitwise equal
    bc = torch.as_tensor(big.astype(np.int32)).cuda()
    hq = torch.as_tensor(q.astype(np.int32)).cuda()
    pl = H.RankPlanes(emb, bc)
    a = H.topk_candidates(emb, hq, bc, 50, planes=pl)
    b = H.topk_candidates(emb, hq, bc, 50)
    c = H.topk_candidates(emb, hq, bc, 50, planes=pl)
    for x, y in ((a, b), (a, c)):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])


def test_gpu_topk_small_batch_many_candidates_uses_ranges():
    """One query and 64 queries against many candidates: the candidate ranges and their merge."""
    from graphembeddings_amd import hole as H
    rng = np.random.default_rng(11)
    N, d = 200_000, 64
    emb = (torch.randn(N, d, device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 0.2).contiguous()
    cand = torch.arange(2, N, dtype=torch.int32, device="cuda")
    for B, k in ((1, 128), (64, 10), (3, 1)):
        hr = torch.as_tensor(np.stack([rng.integers(2, N, B), rng.integers(0, 2, B)], 1).astype(np.int32)).cuda()
        ids, ls = H.topk_candidates(emb, hr, cand, k)
        losses = _sweep_losses(emb, hr, cand, "tail")
        for b in range(B):
            v, o = torch.sort(losses[b], stable=True)      # (candidates in id order: a stable sort is (loss, id))
            assert torch.equal(ids[b].to(torch.int64), cand[o[:k]].to(torch.int64)) and torch.equal(ls[b], v[:k])


def test_gpu_predict_links_holds_no_score_matrix_at_fb15k_shape():
    from graphembeddings_amd import evaluate as E
    R, N, d, B, k = 1345, 1345 + 14951, 200, 59071, 128
    rng = np.random.default_rng(7)
    emb = (torch.randn(N, d, device="cuda", generator=torch.Generator("cuda").manual_seed(1)) * 0.1).contiguous()
    cand = np.arange(R, N)
    q = np.stack([rng.integers(R, N, B), rng.integers(0, R, B)], 1)
    known = np.stack([rng.integers(R, N, 4 * B), rng.integers(R, N, 4 * B), rng.integers(0, R, 4 * B)], 1)
    index = E.KnownIndex(known, N, "tail", emb.device)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ids, ls = E.predict_links(emb, q, cand, k, known_triples=index)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    assert grown < B * len(cand) * 4 / 8, grown
    assert ids.shape == (B, k) and (ids >= 0).all() and (np.diff(ls, axis=1) >= 0).all()


def _toy_kg(tmp_path, n_ent=120, gsz=6, seed=0):
    """tests/test_gpu_train_eval.py's learnable toy KG."""
    rng = np.random.default_rng(seed)
    R, N = 2, 2 + n_ent
    rows = [(i, f"r{i}", f"r{i}", "RELATION") for i in range(R)]
    rows += [(R + e, f"e{e}", f"e{e}", "A" if e % 3 else "B") for e in range(n_ent)]
    with open(tmp_path / "entity_metadata.tsv", "w") as f:
        f.write("Index\tId\tName\tType\n")
        for r in rows:
            f.write("\t".join(str(x) for x in r) + "\n")
    (tmp_path / "relation_ids.txt").write_text("".join(f"r{i}\t{i}\n" for i in range(R)))
    r0, r1 = [], []
    ng = n_ent // gsz
    for g in range(ng):
        mem = [R + g * gsz + i for i in range(gsz)]
        r0 += [[a, b, 0] for a in mem for b in mem if a != b]
        r1 += [[R + g * gsz + i, R + ((g + 1) % ng) * gsz + i, 1] for i in range(gsz)]
    r0 = np.array(r0, dtype=np.int64)
    rng.shuffle(r0)
    n_test, n_valid = 40, 64
    train = np.concatenate([r0[n_test + n_valid:], np.array(r1, dtype=np.int64)])
    rng.shuffle(train)
    np.savetxt(tmp_path / "test_positive_triples.txt", r0[:n_test], fmt="%d", delimiter="\t")
    np.savetxt(tmp_path / "triples-valid.txt", r0[n_test:n_test + n_valid], fmt="%d", delimiter="\t")
    np.savetxt(tmp_path / "triples.txt", train, fmt="%d", delimiter="\t")
    return str(tmp_path)


def test_gpu_driver_predict_k_writes_the_reference_lines(tmp_path):
    from graphembeddings_amd import data as D
    from graphembeddings_amd import hole as H
    from graphembeddings_amd import train as T
    dd = tmp_path / "data"
    dd.mkdir()
    data_dir = _toy_kg(dd)
    out = str(tmp_path / "run")
    argv = ["--data_dir", data_dir, "--output_dir", out, "--batch_size", "64", "--embedding_dim", "64",
            "--num_epochs", "150", "--learning_rate", "0.5", "--margin", "0.5", "--padded_size", "64", "--seed", "1"]
    T.run_training(D.init_data(data_dir), T.build_parser().parse_args(argv), log=lambda *a: None)
    plain_log, pred_log = [], []
    m0 = T.infer_triples(T.build_parser().parse_args(argv + ["--infer", "--infer_threshold", "0.3"]),
                         log=lambda *a: plain_log.append(a))
    assert not os.path.exists(os.path.join(out, "inference_results.tsv"))
    m1 = T.infer_triples(T.build_parser().parse_args(argv + ["--infer", "--infer_threshold", "0.3", "--predict_k", "3"]),
                         log=lambda *a: pred_log.append(a))
    assert m0 == m1
    assert len(pred_log) == len(plain_log) + 1 and "lines written" in str(pred_log[-1][0])
    text = open(os.path.join(out, "inference_results.tsv")).read()
    # the reference's write set over the sweep's own losses
    data = D.init_inference_data(data_dir)
    emb, _ = T.load_checkpoint(out)
    cand = np.arange(data.relation_count, data.entity_count)
    hr_all = data.test_array[:, [0, 2]]
    _, first = np.unique(hr_all, axis=0, return_index=True)
    queries = hr_all[np.sort(first)]
    losses = _sweep_losses(emb, torch.as_tensor(queries.astype(np.int32)).cuda(),
                           torch.as_tensor(cand.astype(np.int32)).cuda(), "tail").cpu().numpy()
    expect = []
    for i, (h, r) in enumerate(queries):
        expect += TR.write_set(losses[i], cand, h, r, 3, data.true_triples[int(h)][int(r)], 0.3)
    assert text == "".join(expect)
    assert len(expect) > 0
    # learning: the top filtered prediction hits a held-out tail far above chance
    from graphembeddings_amd import evaluate as E
    known = np.concatenate([data.triples, data.validation_triples])
    ids, _ = E.predict_links(emb, queries, cand, 1, known_triples=known)
    hits = np.mean([ids[i, 0] in data.test_triples[int(h)][int(r)] for i, (h, r) in enumerate(queries)])
    chance = np.mean([len(data.test_triples[int(h)][int(r)]) / len(cand) for h, r in queries])
    assert hits > 5 * chance, (hits, chance)


@pytest.mark.parametrize("d,k,fused", [(48, 10, False), (64, 10, False), (64, 150, True), (200, 130, True)])
@pytest.mark.parametrize("side", ["tail", "head"])
def test_gpu_predict_links_filtered_fallbacks_equal_heap(d, k, fused, side):
    """The fallbacks with a filter: fused=False (score_candidates' losses; d = 48 has no fused sweep) and k above
    hole.topk_max_k() (the rank sweep's losses), against the heap over the same losses, known cells from the triples."""
    from graphembeddings_amd import evaluate as E
    from graphembeddings_amd import hole as H
    rng = np.random.default_rng(d + k)
    R, N, B = 4, 500, 140
    emb = torch.as_tensor(_table(N, d, seed=d)).cuda()
    cand_np = rng.permutation(np.arange(R, N))[:300]
    q = np.stack([rng.integers(R, N, B), rng.integers(0, R, B)], 1)
    q[0] = [52, 1]
    kn = _known(N, q, cand_np, rng, per_row=40)
    if side == "head":
        kn = kn[:, [1, 0, 2]]
    ids, ls = E.predict_links(emb, q, cand_np, k, known_triples=kn, side=side, fused=fused)
    hq = torch.as_tensor(q.astype(np.int32)).cuda()
    cq = torch.as_tensor(cand_np.astype(np.int32)).cuda()
    if fused:
        losses = _sweep_losses(emb, hq, cq, side)
    else:
        losses = H.score_candidates(emb, hq, cq, cand_is_head=(side == "head"))
    eid, el = TR.first_k_rows(losses.cpu().numpy(), cand_np, k, _known_mask(kn, q, cand_np, side))
    assert np.array_equal(ids, eid) and np.array_equal(ls, el)


def test_gpu_driver_lines_with_raw_lists_past_the_kernel_k():
    """predict_inference_results on the GPU sweeps where the raw lists run past hole.topk_max_k(): K = 130, and K = 3
    behind 150 known tails -- against the heap restatement over the sweep's losses."""
    import types
    from collections import defaultdict

    from graphembeddings_amd import evaluate as E
    R, N, d = 2, 302, 64
    rng = np.random.default_rng(9)
    emb = torch.as_tensor(_table(N, d, seed=9)).cuda()
    cand = np.arange(R, N)
    heads = rng.choice(cand, 30, replace=False)
    test = np.stack([np.repeat(heads, 2), rng.choice(cand, 60), np.tile([0, 1], 30)], 1)
    queries = test[:, [0, 2]]
    losses = _sweep_losses(emb, torch.as_tensor(queries.astype(np.int32)).cuda(),
                           torch.as_tensor(cand.astype(np.int32)).cuda(), "tail").cpu().numpy()
    true = defaultdict(lambda: defaultdict(set))
    known = []
    for i, (h, r) in enumerate(queries):
        tails = cand[np.lexsort((cand, losses[i]))[:150]] if i % 2 == 0 else rng.choice(cand, 5, replace=False)
        for t in tails:
            if t != test[i, 1]:
                known.append([h, t, r])
                true[int(h)][int(r)].add(int(t))
    data = types.SimpleNamespace(relation_count=R, entity_count=N, test_array=test, triples=np.array(known),
                                 validation_triples=None, true_triples=true)
    for K in (3, 130):
        path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"topk_driver_{os.getpid()}_{K}.tsv")
        try:
            E.predict_inference_results(emb, data, K, 1.0, path, log=lambda *a: None)
            text = open(path).read()
        finally:
            if os.path.exists(path):
                os.remove(path)
        expect = []
        for i, (h, r) in enumerate(queries):
            expect += TR.write_set(losses[i], cand, h, r, K, true[int(h)][int(r)], 1.0)
        assert text == "".join(expect)
        assert max(len(TR.write_set(losses[i], cand, h, r, K, true[int(h)][int(r)], 1.0))
                   for i, (h, r) in enumerate(queries)) > 128


def test_gpu_predict_links_hole_refuses_planes():
    from graphembeddings_amd import evaluate as E
    from graphembeddings_amd import hole as H
    emb = torch.as_tensor(_table(300, 64, seed=2)).cuda()
    cand = np.arange(4, 300)
    spec = H.hole_to_spectral(emb.clone())
    pl = H.RankPlanes(spec, torch.as_tensor(cand.astype(np.int32)).cuda(), model="hole_spectral")
    q = np.array([[10, 1], [20, 2]])
    with pytest.raises(ValueError, match="hole_spectral"):
        E.predict_links(emb, q, cand, 5, model="hole", planes=pl)
    a = E.predict_links(spec, q, cand, 5, model="hole_spectral", planes=pl)
    b = E.predict_links(emb, q, cand, 5, model="hole")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
