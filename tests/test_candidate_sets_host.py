"""Candidate sets without a GPU: the numpy part of evaluate.CandidateSets' builders (cell lists, allow bitmaps) against
brute force -- from_types' on the packaged FB15k id files --, the host-side ValueErrors, ge_candidate_mask_words and the
driver's flag checks."""
import numpy as np
import pytest
import torch

import test_abi_workspace_host as W

# The mask's size function joins the table test_abi_workspace_host.py checks (its test_every_size_function_is_listed reads
# CASES when it runs, after every module is collected): 0 for K <= 0, non-decreasing in K across the 128-candidate tile.
W.CASES["ge_candidate_mask_words"] = ([sorted(W.SIZES + [14951, 2 ** 31 - 1])], [(0,), (-1,), (-2 ** 40,)], False)


def E():
    from graphembeddings_amd import evaluate
    return evaluate


def test_mask_words_is_four_per_tile():
    from graphembeddings_amd import _lib
    from graphembeddings_amd import hole as H
    fn = _lib.load().ge_candidate_mask_words
    for K in (1, 32, 127, 128, 129, 130, 417, 14951, 2 ** 31 - 1):
        assert int(fn(K)) == 4 * ((K + 127) // 128) == H.candidate_mask_words(K)
    assert int(fn(0)) == 0 == H.candidate_mask_words(0) and int(fn(-5)) == 0
    W.test_size_function("ge_candidate_mask_words")


def test_cells_from_lists_and_observed_against_brute_force():
    CS = E().CandidateSets
    rng = np.random.default_rng(0)
    R, N = 7, 300
    cand = rng.permutation(np.arange(R, N))[:200]
    pos = {int(c): i for i, c in enumerate(cand)}
    assert np.array_equal(CS.positions_of(cand, np.array([cand[3], N + 5, 0, cand[199], cand[0]])), [3, -1, -1, 199, 0])
    lists = {2: [int(cand[5]), int(cand[5]), int(cand[0])], 0: cand[50:60], 6: []}
    cells, n_sets = CS.cells_from_lists(cand, lists)
    assert n_sets == 7
    want = sorted({(2, 5), (2, 0)} | {(0, i) for i in range(50, 60)})
    assert cells.dtype == np.int32 and [tuple(c) for c in cells.tolist()] == want
    assert CS.cells_from_lists(cand, {}, n_sets=3)[0].shape == (0, 2)
    triples = np.stack([rng.integers(R, N, 500), rng.integers(R, N, 500), rng.integers(0, R, 500)], 1)
    for side, col in (("tail", 1), ("head", 0)):
        want = sorted({(int(t[2]), pos[int(t[col])]) for t in triples if int(t[col]) in pos})
        got = CS.cells_from_observed(cand, triples, R, side)
        assert got.dtype == np.int32 and [tuple(c) for c in got.tolist()] == want
    assert CS.cells_from_observed(cand, np.zeros((0, 3), np.int64), R, "tail").shape == (0, 2)


def _bits(allow, n_class):
    c = np.arange(n_class)
    return ((allow[:, c >> 5] >> (c & 31).astype(np.uint32)) & 1).astype(bool)


def test_allow_from_types_against_brute_force():
    CS = E().CandidateSets
    rng = np.random.default_rng(1)
    R, N, T = 5, 400, 70                                   # 70 types: three words of the bitmap
    codes = rng.integers(-1, T, N).astype(np.int32)
    triples = np.stack([rng.integers(R, N, 300), rng.integers(R, N, 300), rng.integers(0, R - 1, 300)], 1)
    for side, col in (("tail", 1), ("head", 0)):
        got_codes, allow, n_class = CS.allow_from_types(codes, triples, R, side)
        assert np.array_equal(got_codes, codes) and n_class == int(codes.max()) + 1
        assert allow.dtype == np.uint32 and allow.shape == (R, (n_class + 31) // 32)
        want = np.zeros((R, n_class), bool)
        for t in triples:
            if codes[t[col]] >= 0:
                want[t[2], codes[t[col]]] = True
        assert np.array_equal(_bits(allow, n_class), want) and not want[R - 1].any()
    # a dict of type names gives the same sets as its codes
    names = {i: "T%d" % c for i, c in enumerate(codes) if c >= 0}
    dc, dallow, dn = CS.allow_from_types(names, np.concatenate([triples, [[N - 1, N - 1, 0]]]), R, "tail")
    assert dc.shape[0] == max(names) + 1
    by_name = {}
    for i, c in enumerate(dc):
        if c >= 0:
            by_name.setdefault(int(c), set()).add(names[i])
    assert all(len(v) == 1 for v in by_name.values())


def test_from_types_sets_on_the_packaged_fb15k_ids():
    """The reference's TODO (holE.py:533) on the packaged FB15k files: per relation, the candidates whose type was seen
    as a tail (head) of the relation in the packaged valid + test triples, against a dict of sets."""
    from graphembeddings_amd import data as D
    CS = E().CandidateSets
    data = D.init_inference_data(D.PACKAGE_FB15K_DIR)
    R, N = data.relation_count, data.entity_count
    assert (R, N) == (1345, 1345 + 14951)
    triples = np.concatenate([a for a in (data.validation_triples, data.test_array) if a is not None])
    codes = data.type_arrays()[1]
    cand = np.arange(R, N)
    for side, col in (("tail", 1), ("head", 0)):
        got_codes, allow, n_class = CS.allow_from_types(codes, triples, R, side)
        seen = {}
        for t in triples:
            seen.setdefault(int(t[2]), set()).add(data.id_to_type[int(t[col])])
        names = data.type_arrays()[0]
        adm = _bits(allow, n_class)[:, got_codes[cand]]                  # [R, K]: what the device builder expands
        rng = np.random.default_rng(2)
        for r in list(rng.integers(0, R, 40)) + [int(triples[0, 2])]:
            want = np.array([data.id_to_type[int(c)] in seen.get(int(r), ()) for c in cand])
            assert np.array_equal(adm[r], want), (side, r)
        sizes = adm.sum(1)
        assert sizes.max() <= len(cand) and (sizes[sorted(seen)] > 0).all() and len(names) >= n_class - 1


def test_host_value_errors():
    ev = E()
    CS = ev.CandidateSets
    from graphembeddings_amd import hole as H
    cand = np.arange(5, 50)
    with pytest.raises(ValueError):
        CS.cells_from_lists(cand, {0: [4]})                              # not a candidate
    with pytest.raises(ValueError):
        CS.cells_from_lists(cand, {3: [5]}, n_sets=3)                    # set index out of range
    with pytest.raises(ValueError):
        CS.cells_from_lists(cand, {-1: [5]})
    with pytest.raises(ValueError):
        CS.cells_from_lists(np.array([5, 5, 6]), {0: [5]})               # candidates not distinct
    with pytest.raises(ValueError):
        CS.cells_from_observed(cand, np.array([[5, 6, 9]]), 3, "tail")   # relation outside [0, relation_count)
    with pytest.raises(ValueError):
        CS.cells_from_observed(cand, np.array([[5, 6, 1]]), 3, "left")
    with pytest.raises(ValueError):
        CS.allow_from_types(np.zeros(10, np.int32), np.array([[5, 60, 1]]), 3, "tail")    # entity without a type entry
    with pytest.raises(ValueError):
        CS.allow_from_types(np.zeros((2, 2)), np.array([[0, 1, 1]]), 3, "tail")
    # the sweeps' host checks come before any launch: CPU tensors are enough to reach them
    emb = torch.zeros(60, 64)
    test = np.array([[6, 7, 1]])
    with pytest.raises(ValueError):
        ev.link_prediction_ranks(emb, test, cand, side="tail", row_sets=[0])
    with pytest.raises(ValueError):
        ev.link_prediction_ranks(emb, test, cand, side="tail", return_admissible=True)
    with pytest.raises(ValueError):
        ev.predict_links(emb, [[6, 1]], cand, 3, row_sets=[0])
    with pytest.raises(ValueError):
        H._sets_args(None, [0], torch.zeros(1, 2, dtype=torch.int32), torch.arange(45, dtype=torch.int32), "x")
    fake = CS(torch.arange(45, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32), np.zeros(2))
    with pytest.raises(ValueError):                                      # not a device mask
        H._sets_args(fake, None, torch.zeros(1, 2, dtype=torch.int32), torch.arange(45, dtype=torch.int32), "x")
    with pytest.raises(ValueError):
        ev.evaluate_constrained(emb, None, "relations")


def test_driver_flag_checks():
    from graphembeddings_amd import train as T
    base = ["--data_dir", "x", "--output_dir", "y"]
    p = T.build_parser()
    assert p.parse_args(base).candidate_sets is None
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--candidate_sets", "everything"])
    with pytest.raises(SystemExit, match="needs --infer"):
        T.check_candidate_set_flags(p.parse_args(base + ["--candidate_sets", "types"]))
    with pytest.raises(SystemExit, match="one GPU"):
        T.check_candidate_set_flags(p.parse_args(base + ["--infer", "--candidate_sets", "observed", "--gpus", "2"]))
    with pytest.raises(SystemExit, match="one GPU"):
        T.check_candidate_set_flags(p.parse_args(base + ["--infer", "--candidate_sets", "observed"]), world=2)
    T.check_candidate_set_flags(p.parse_args(base + ["--infer", "--candidate_sets", "types"]))
    T.check_candidate_set_flags(p.parse_args(base))
    with pytest.raises(SystemExit, match="needs --infer"):
        T.main(base + ["--candidate_sets", "types"])
