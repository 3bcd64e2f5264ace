"""Host side of relation prediction (h, ?, t): the fp64 oracle tests/relation_rank_ref.py against the score oracles,
the known-relation index, the argument checks, the drivers' flags and the workspace contract of
ge_transx_relation_rank / ge_transr_relation_rank through the built library (no GPU needed)."""
import argparse
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import relation_rank_ref as RL
from tests import transr_ref as RR
from tests import transx_ref as XR

MODELS = ("transe", "transh", "transd", "transr")


def _random_tables(model, E, R, d, seed):
    rng = np.random.default_rng(seed)
    if model == "transr":
        return RR.random_tables(E, R, d, d + 3, rng)
    rows = {"ent": E, "rel": R, "normal_vector": R, "ent_transfer": E, "rel_transfer": R}
    return {k: rng.normal(size=(rows[k], d)) for k in ("ent", "rel") + XR.EXTRA[model]}


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("l1", [True, False])
def test_oracle_columns_are_the_score_of_each_relation(model, l1):
    E, R, d, n = 17, 9, 6, 25
    tabs = _random_tables(model, E, R, d, seed=4)
    rng = np.random.default_rng(1)
    test = np.stack([rng.integers(0, E, n), rng.integers(0, E, n), rng.integers(0, R, n)], 1)
    D = RL.distances(model, tabs, test, l1)
    M = RL.distances(model, tabs, test, l1, magnitude=True)
    assert D.shape == (n, R) and np.all(M >= D - 1e-12)
    for c in range(R):
        tri = np.stack([test[:, 0], test[:, 1], np.full(n, c)], 1)
        ref = RR.score(tabs, tri, l1) if model == "transr" else XR.score(model, tabs, tri, l1)
        np.testing.assert_allclose(D[:, c], ref, rtol=0, atol=1e-12)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("l1", [True, False])
def test_counts_equal_the_brute_force_walk_on_the_tie_fixture(model, l1):
    tabs, test, known = RL.tie_fixture(model)
    R = tabs["rel"].shape[0]
    D = RL.distances(model, tabs, test, l1)
    assert np.array_equal(D, np.round(D)) and D.max() < XR.FP32_EXACT
    nb, nk = RL.counts(D, test[:, 2], RL.known_mask(test, known, R))
    raw, fil = RL.brute_force(model, tabs, test, l1, known)
    assert np.array_equal(nb + 1, raw) and np.array_equal(nb + 1 - nk, fil)
    # exact ties on both sides of some target, and known candidates that count
    i = np.arange(len(test))
    tied = D == D[i, test[:, 2]][:, None]
    c = np.arange(R)[None, :]
    assert (tied & (c < test[:, 2:3])).any() and (tied & (c > test[:, 2:3])).any()
    assert (nk > 0).any() and len(np.unique(known, axis=0)) < len(known)


def test_known_index_of_relations_on_cpu_tensors():
    from graphembeddings_amd import evaluate as EV
    known = np.array([[3, 1, 2], [0, 4, 1], [3, 1, 0], [3, 1, 2], [4, 0, 1], [0, 4, 0]])
    idx = EV.KnownIndex(known, 7, "relation", "cpu")
    # key = h * n_rows + t, sorted by (h, t, r) with duplicates removed; the values are the relations
    assert idx.key.tolist() == [0 * 7 + 4, 0 * 7 + 4, 3 * 7 + 1, 3 * 7 + 1, 4 * 7 + 0]
    assert idx.ent.tolist() == [0, 1, 0, 2, 1]
    empty = EV.KnownIndex(None, 7, "relation", "cpu")
    assert empty.key.numel() == 0 and empty.ent.numel() == 0
    # the entity sides are what they were
    tail = EV.KnownIndex(known, 7, "tail", "cpu")
    assert tail.key.tolist() == [0 * 7 + 0, 0 * 7 + 1, 3 * 7 + 0, 3 * 7 + 2, 4 * 7 + 1] and tail.ent.tolist() == [4, 4, 1, 1, 0]


def _stub(n_ent=20, n_rel=3):
    return types.SimpleNamespace(n_ent=n_ent, n_rel=n_rel, tables={"ent": torch.zeros(1)})


def test_bad_ids_k_and_pair_shapes_raise_before_any_gpu_call():
    from graphembeddings_amd import evaluate as EV
    m = _stub()
    for bad in ([[0, 20, 0]], [[-1, 1, 0]], [[0, 1, 3]]):
        with pytest.raises(ValueError):
            EV.translation_relation_ranks(m, np.array(bad))
    with pytest.raises(ValueError):
        EV.translation_relation_ranks(m, np.array([[0, 1]]))
    with pytest.raises(ValueError, match="k must be >= 1"):
        EV.predict_translation_relations(m, np.array([[0, 1]]), 0)
    for bad in (np.array([[0, 1, 2]]), np.array([0, 1]), np.array([[0, 20]]), np.array([[-1, 0]]), np.array([[0.5, 1.0]])):
        with pytest.raises(ValueError):
            EV.predict_translation_relations(m, bad, 2)
    with pytest.raises(ValueError, match="n_rows"):
        EV.predict_translation_relations(m, np.array([[0, 1]]), 2, known=EV.KnownIndex(None, 5, "relation", "cpu"))
    with pytest.raises(ValueError):
        EV.predict_relations(torch.zeros(30, 8), np.array([[0, 30]]), 4, 2)
    with pytest.raises(ValueError):
        EV.predict_relations(torch.zeros(30, 8), np.array([[0, 1, 2]]), 4, 2)


def test_relation_lines_character_for_character():
    from graphembeddings_amd import evaluate as EV
    test = np.array([[1, 2, 0], [4, 1, 3]])
    pairs = np.array([[1, 2], [4, 1]])
    ids = np.array([[0, 5, -1], [2, 3, 1]])
    dist = np.array([[0.5, np.float32(1.0 / 3.0), np.inf], [1.0, 2.0, 3.0]], dtype=np.float32)
    assert EV.translation_relation_lines(pairs, ids, dist, test) == [
        "1\t2\t1\t0\t0.5\t1\n", "1\t2\t2\t5\t0.333333343\t0\n",
        "4\t1\t1\t2\t1\t0\n", "4\t1\t2\t3\t2\t1\n", "4\t1\t3\t1\t3\t0\n"]


def test_library_exports_the_relation_rank_symbols_and_workspace_contract():
    from graphembeddings_amd import _lib, build
    lib_path = build.build()
    raw = ctypes.CDLL(lib_path)
    for name in ("ge_transx_relation_rank_workspace_bytes", "ge_transx_relation_rank",
                 "ge_transr_relation_rank_workspace_bytes", "ge_transr_relation_rank"):
        assert hasattr(raw, name) and name in _lib.SYMBOLS
    lib = _lib.load()
    assert lib.ge_version() >= 390
    xs = lambda model, E, R, d, B: int(lib.ge_transx_relation_rank_workspace_bytes(model, E, R, d, B))
    rs = lambda E, R, de, dr, B: int(lib.ge_transr_relation_rank_workspace_bytes(E, R, de, dr, B))
    E, B = 14951, 59071
    for R in (18, 1345):
        for model in (0, 1, 2):
            assert 0 < xs(model, E, R, 100, B) < 64 << 20       # a fixed row chunk, not [B, R]
            assert xs(model, E, R, 100, 2 * B) == xs(model, E, R, 100, B) or R == 18
            assert xs(model, E, R, 100, 10) <= xs(model, E, R, 100, 1000) <= xs(model, E, R, 100, B)
        assert 0 < rs(E, R, 100, 100, B) < 64 << 20
    for bad in ((3, E, 5, 8, 10), (-1, E, 5, 8, 10), (0, 0, 5, 8, 10), (0, E, 0, 8, 10), (0, E, 5, 0, 10),
                (0, E, 5, lib.ge_transx_max_dim() + 1, 10), (0, E, 5, 8, 0), (0, E, 5, 8, -3), (0, E, 5, 8, (1 << 28) + 1)):
        assert xs(*bad) == 0
    dm = lib.ge_transr_max_dim()
    for bad in ((0, 5, 8, 8, 10), (E, 0, 8, 8, 10), (E, 5, 0, 8, 10), (E, 5, 8, 0, 10), (E, 5, dm + 1, 8, 10),
                (E, 5, 8, dm + 1, 10), (E, 5, 8, 8, 0), (E, 5, 8, 8, (1 << 28) + 1)):
        assert rs(*bad) == 0
    assert xs(0, E, 5, lib.ge_transx_max_dim(), 10) > 0 and rs(E, 5, dm, dm, 10) > 0


def _args(**kw):
    base = dict(filter_file=[], test_file=None, load=None, predict_k=None, relation_ranks=False, predict_relations_k=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_driver_flags_parse_and_are_checked(tmp_path):
    from graphembeddings_amd import train as T
    from graphembeddings_amd import transr_train as RT
    from graphembeddings_amd import transx_train as TT
    t = tmp_path / "test2id.txt"
    t.write_text("1\n0 1 0\n")
    for mod in (TT, RT):
        a = mod.build_parser().parse_args(["--relation_ranks", "--predict_relations_k", "3"])
        assert a.relation_ranks is True and a.predict_relations_k == 3
        with pytest.raises(ValueError, match="needs --test_file"):
            mod.check_args(a)
        d = mod.build_parser().parse_args([])
        assert d.relation_ranks is False and d.predict_relations_k is None
    with pytest.raises(ValueError, match="--relation_ranks needs --test_file"):
        TT.check_eval_args(_args(relation_ranks=True))
    with pytest.raises(ValueError, match="--predict_relations_k needs --test_file"):
        TT.check_eval_args(_args(predict_relations_k=2))
    with pytest.raises(ValueError, match="--predict_relations_k must be >= 1"):
        TT.check_eval_args(_args(predict_relations_k=0, test_file=str(t)))
    TT.check_eval_args(_args(predict_relations_k=1, relation_ranks=True, test_file=str(t)))
    assert "not the test file" in " ".join(TT.build_parser().format_help().split())
    f = T.build_parser().parse_args(["--data_dir", "x", "--output_dir", "y", "--infer", "--relation_ranks"])
    assert f.relation_ranks is True and T.build_parser().parse_args(["--data_dir", "x", "--output_dir", "y"]).relation_ranks is False
    with pytest.raises(SystemExit, match="--relation_ranks needs --infer"):
        T.main(["--data_dir", "x", "--output_dir", "y", "--relation_ranks"])
    with pytest.raises(SystemExit, match="one GPU"):
        T.main(["--data_dir", "x", "--output_dir", "y", "--infer", "--relation_ranks", "--gpus", "2"])
