"""Host side of the translation models' candidate sets: every ValueError that fires before device work, the drivers'
--candidate_sets flag, the refusals of the four masked entry points through the built library, and the numpy restatement
the GPU tests use as their oracle (tests/translation_sets_ref.py) on a hand-written example.  No GPU needed."""
import argparse
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import translation_sets_ref as REF

F32 = np.float32
INF, NAN = np.inf, np.nan


def _model(n_ent=10, n_rel=3):
    """What the host checks read of a model: its sizes and the device of its tables (CPU tensors reach every check)."""
    return SimpleNamespace(n_ent=n_ent, n_rel=n_rel, tables={"ent": torch.zeros(n_ent, 4)})


def _sets(n_ent=10, n_sets=3, cand=None):
    from graphembeddings_amd.evaluate import CandidateSets
    cand = torch.arange(n_ent, dtype=torch.int32) if cand is None else cand
    return CandidateSets(cand, torch.zeros(n_sets, REF.words(n_ent), dtype=torch.int32), np.zeros(n_sets))


def test_value_errors_before_any_device_work():
    from graphembeddings_amd import evaluate as EV
    m, cs = _model(), _sets()
    test = np.array([[1, 2, 0], [3, 4, 2]])
    queries = test[:, [0, 2]]
    # sets without the arguments that need them
    with pytest.raises(ValueError, match="need candidate_sets"):
        EV.translation_ranks(m, test, row_sets=[0, 0])
    with pytest.raises(ValueError, match="need candidate_sets"):
        EV.translation_ranks(m, test, return_admissible=True)
    with pytest.raises(ValueError, match="need candidate_sets"):
        EV.predict_translation(m, queries, 3, row_sets=[0, 0])
    for call in (lambda **kw: EV.translation_ranks(m, test, **kw), lambda **kw: EV.predict_translation(m, queries, 3, **kw)):
        with pytest.raises(ValueError, match="one entry per row"):           # wrong row_sets length
            call(candidate_sets=cs, row_sets=[0])
        with pytest.raises(ValueError, match="one entry per row"):
            call(candidate_sets=cs, row_sets=[[0, 1]])
        with pytest.raises(ValueError, match=r"outside \[-1, 3\)"):           # a set index out of range
            call(candidate_sets=cs, row_sets=[0, 3])
        with pytest.raises(ValueError, match=r"outside \[-1, 3\)"):
            call(candidate_sets=cs, row_sets=[-2, 0])
        with pytest.raises(ValueError, match="integer"):
            call(candidate_sets=cs, row_sets=[0.5, 1.0])
        with pytest.raises(ValueError, match="another candidate list"):      # sets of another length ...
            call(candidate_sets=_sets(n_ent=9))
        with pytest.raises(ValueError, match="another candidate list"):      # ... or of other ids
            call(candidate_sets=_sets(cand=torch.arange(1, 11, dtype=torch.int32)))
        with pytest.raises(ValueError, match="relation id"):                 # the default row set needs a set per relation
            call(candidate_sets=_sets(n_sets=2))
        with pytest.raises(ValueError, match="CandidateSets"):
            call(candidate_sets={"tail": cs})
        with pytest.raises(ValueError, match="side"):
            call(candidate_sets=cs, side="left")
    with pytest.raises(ValueError, match="per evaluated side"):
        EV.evaluate_translation(m, test, candidate_sets={"tail": cs})
    with pytest.raises(ValueError, match="per evaluated side"):
        EV.evaluate_translation(m, test, candidate_sets=cs)


def test_model_layer_refuses_malformed_sets():
    from graphembeddings_amd.transx import _Model
    m = _Model()
    m.n_ent = 300
    rs, mask = torch.zeros(4, dtype=torch.int32), torch.zeros(2, 12, dtype=torch.int32)
    assert m._sets_args(4, None, None) == ()
    with pytest.raises(ValueError, match="come together"):
        m._sets_args(4, rs, None)
    with pytest.raises(RuntimeError, match="no CPU path"):                   # (CPU tensors: refused before any call)
        m._sets_args(4, rs, mask)


def _args(**kw):
    base = dict(filter_file=[], test_file=None, load=None, predict_k=None, candidate_sets=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_drivers_accept_observed_and_nothing_else(tmp_path):
    from graphembeddings_amd import transr_train as RT
    from graphembeddings_amd import transx_train as TT
    t = tmp_path / "test2id.txt"
    t.write_text("1\n0 1 0\n")
    for mod in (TT, RT):
        p = mod.build_parser()
        assert p.parse_args([]).candidate_sets is None
        a = p.parse_args(["--candidate_sets", "observed", "--test_file", str(t)])
        assert a.candidate_sets == "observed"
        mod.check_args(a)
        for other in ("types", "everything", ""):
            with pytest.raises(SystemExit):
                p.parse_args(["--candidate_sets", other])
        with pytest.raises(ValueError, match="--candidate_sets needs --test_file"):
            mod.check_args(p.parse_args(["--candidate_sets", "observed"]))
        assert "not the test file" in " ".join(p.format_help().split())
    with pytest.raises(ValueError, match="must be 'observed'"):
        TT.check_eval_args(_args(candidate_sets="types", test_file=str(t)))
    TT.check_eval_args(_args(test_file=str(t)))


A = 1 << 12                                   # a fake, 256-byte aligned, never-dereferenced address


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: host-only refusals")
def test_masked_entry_points_refuse_bad_arguments_without_launching():
    from graphembeddings_amd import _lib
    lib = _lib.load()
    EINVAL, ENOMEM = _lib.GE_EINVAL, _lib.GE_ENOMEM
    tx = (0, 0, A, 300, A, 4, A, A, A, 8)
    tr = (0, A, 300, A, A, 4, 8, 12)
    sizes = {("ge_transx", "rank"): lib.ge_transx_rank_workspace_bytes(0, 300, 4, 8, 2),
             ("ge_transr", "rank"): lib.ge_transr_rank_workspace_bytes(300, 4, 8, 12, 2),
             ("ge_transx", "topk"): lib.ge_transx_topk_workspace_bytes(0, 300, 4, 8, 2, 5),
             ("ge_transr", "topk"): lib.ge_transr_topk_workspace_bytes(300, 4, 8, 12, 2, 5)}
    for pre, tabs in (("ge_transx", tx), ("ge_transr", tr)):
        for kind in ("rank", "topk"):
            need = int(sizes[(pre, kind)])
            assert need > 0
            assert len(_lib.SYMBOLS[f"{pre}_{kind}_masked"][1]) == len(_lib.SYMBOLS[f"{pre}_{kind}"][1]) + (2 if kind == "rank" else 3)

            def call(B=2, row_set=A, mask=A, n_sets=3, ws=A, ws_bytes=need, k=5, known=(None, None)):
                outs = (A, A, A) if kind == "rank" else (k, A, A)
                return getattr(lib, f"{pre}_{kind}_masked")(*tabs, A, B, 0, *known, row_set, mask, n_sets, *outs, ws, ws_bytes, None)
            assert call(mask=None) == EINVAL
            assert call(row_set=None) == EINVAL
            assert call(n_sets=0) == EINVAL
            assert call(n_sets=-1) == EINVAL
            assert call(mask=A + 2) == EINVAL and call(row_set=A + 2) == EINVAL
            assert call(B=0, mask=None) == EINVAL                 # the sets come before B == 0
            assert call(B=0) == 0
            assert call(ws_bytes=need - 1) == ENOMEM
            assert call(ws=A + 16) == EINVAL
            assert call(ws=None) == EINVAL
            assert call(known=(A, None)) == EINVAL
            assert call(B=-1) == EINVAL
            if kind == "topk":
                assert call(k=0) == EINVAL and call(k=lib.ge_transx_topk_max_k() + 1) == EINVAL


def test_oracle_on_a_hand_written_example():
    """Three rows over five entities, every number worked out by hand.
    stored distances (row: entity 0 .. 4)        true   set           admissible entities
      row 0:  3  1  1  2  0                        2      0 = {1, 2, 4}  1, 2, 4
      row 1:  5  5  0  NaN 1                       1      1 = {0, 3}     0, 3
      row 2:  2  2  2  2  2                        3      -1             all
    known cells: (0, 4), (1, 3), (2, 0).
    row 0: D_true = 1 at entity 2.  Before it: entity 4 (0 < 1) and entity 1 (1 == 1, id 1 < 2); entity 0, 3 are larger.
           Both are admissible: n_before = 2; of them entity 4 is known: n_known_before = 1.
    row 1: D_true = 5 at entity 1, which is not in its set.  Before it: entity 0 (5 == 5, id 0 < 1), entity 2 (0), entity
           4 (1); NaN compares false.  Admissible among them: entity 0 only: n_before = 1, none known: 0.
    row 2: all equal 2, true 3: entities 0, 1, 2 are before: n_before = 3; entity 0 is known: n_known_before = 1."""
    sc = np.array([[3, 1, 1, 2, 0], [5, 5, 0, NAN, 1], [2, 2, 2, 2, 2]], F32)
    adm = np.array([[0, 1, 1, 0, 1], [1, 0, 0, 1, 0]], bool)
    row_set = np.array([0, 1, -1])
    true_id = np.array([2, 1, 3])
    known = np.zeros((3, 5), bool)
    known[0, 4] = known[1, 3] = known[2, 0] = True
    nb, nk, bad = REF.masked_counts(sc, true_id, adm, row_set, known)
    assert nb.tolist() == [2, 1, 3] and nk.tolist() == [1, 0, 1] and not bad.any()
    nb, nk, _ = REF.masked_counts(sc, true_id, adm, row_set, None)
    assert nb.tolist() == [2, 1, 3] and nk.tolist() == [0, 0, 0]
    # top-3, filtered.  row 0: admissible and not known = {1, 2}: (1, id 1), (1, id 2), then padding.
    # row 1: {0}: the NaN of entity 3 is known, so it does not flag the row: (5, id 0), padding.
    # row 2: {1, 2, 3, 4} all at 2: ids 1, 2, 3.
    ids, dist = REF.masked_topk(sc, 3, adm, row_set, known)
    assert ids.tolist() == [[1, 2, -1], [0, -1, -1], [1, 2, 3]]
    assert np.array_equal(dist, np.array([[1, 1, INF], [5, INF, INF], [2, 2, 2]], F32))
    # unfiltered: row 0 = {1, 2, 4}: (0, 4), (1, 1), (1, 2).  row 1 = {0, 3}: entity 3 is admissible, not known, NaN: flagged.
    ids, dist = REF.masked_topk(sc, 3, adm, row_set, None)
    assert ids.tolist() == [[4, 1, 2], [-1, -1, -1], [0, 1, 2]]
    assert np.array_equal(dist[0], np.array([0, 1, 1], F32)) and np.isnan(dist[1]).all()
    # a bad set index: counters -1 and a flagged top-k row; the rows next to it are unchanged
    nb, nk, bad = REF.masked_counts(sc, true_id, adm, np.array([0, 2, -2]), known)
    assert nb.tolist() == [2, -1, -1] and nk.tolist() == [1, -1, -1] and bad.tolist() == [False, True, True]
    ids, dist = REF.masked_topk(sc, 2, adm, np.array([0, 2, -1]), known)
    assert ids.tolist() == [[1, 2], [-1, -1], [1, 2]] and np.isnan(dist[1]).all()
    # the mask format: bit c & 31 of word c >> 5, four words per 128 entities, pad bits on request
    assert REF.words(1) == 4 and REF.words(128) == 4 and REF.words(129) == 8 and REF.words(300) == 12
    bits = np.zeros((2, 40), bool)
    bits[0, [0, 31, 32]] = True
    bits[1, 39] = True
    m = REF.pack(bits)
    assert m.shape == (2, 4) and m[0].tolist() == [0x80000001, 1, 0, 0] and m[1].tolist() == [0, 0x80, 0, 0]
    assert REF.pack(bits, pad=True)[1].tolist() == [0, 0xFFFFFF80, 0xFFFFFFFF, 0xFFFFFFFF]
    assert REF.admitted(adm, np.array([1, -1, 7])).sum(1).tolist() == [2, 5, 0]
