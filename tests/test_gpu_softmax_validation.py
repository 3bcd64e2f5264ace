"""GPU: train.py --objective softmax with --softmax_validation_ticks / --softmax_validation_rows / --softmax_patience on
the planted KG of tests/test_gpu_softmax.py written to files (408 rows, 2776-ish training triples, the 300 held-out
triples as triples-valid.txt), embedding_dim 64: batch_count = 5, so an epoch is 4 steps and two ticks come after its
steps 2 and 4.

The file's table is checked against evaluate.link_prediction_ranks on the same validation rows with the filter the tick
uses (train + valid): its filtered MRR equals the run's pocket_mrr within 2^-23 (tests/rank_tick_ref.py: the counts are
the rank entry points', only the summary's final rounding to float32 differs)."""
import numpy as np
import pytest
import torch

import test_gpu_softmax as TS
from graphembeddings_amd import data as D
from graphembeddings_amd import evaluate as EV
from graphembeddings_amd import train as T
from tests import rank_tick_ref as RT

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")


@pytest.fixture(scope="module")
def kg(tmp_path_factory):
    """The planted KG as a data directory; returns (directory, data)."""
    dd = tmp_path_factory.mktemp("planted")
    train, held, _ = TS.planted()
    R, N = TS.N_REL_KG, TS.N_REL_KG + TS.N_ENT_KG
    with open(dd / "entity_metadata.tsv", "w") as f:
        f.write("Index\tId\tName\tType\n")
        for i in range(N):
            f.write("%d\t%s%d\t%s%d\t%s\n" % ((i, "r", i, "r", i, "RELATION") if i < R else (i, "e", i, "e", i, "A")))
    (dd / "relation_ids.txt").write_text("".join("r%d\t%d\n" % (i, i) for i in range(R)))
    np.savetxt(dd / "triples.txt", train, fmt="%d", delimiter="\t")
    np.savetxt(dd / "triples-valid.txt", held, fmt="%d", delimiter="\t")
    np.savetxt(dd / "test_positive_triples.txt", held[:40], fmt="%d", delimiter="\t")
    data = D.init_data(str(dd))
    assert data.entity_count == N and data.relation_count == R and len(data.validation_triples) == 300
    return str(dd), data


def argv_of(data_dir, out, *extra):
    return ["--data_dir", data_dir, "--output_dir", str(out), "--batch_size", "512", "--embedding_dim", "64", "--seed", "3",
            "--learning_rate", "0.1", "--learning_decay_steps", "0", "--objective", "softmax", "--optimizer", "adagrad",
            "--softmax_scale", "20", *extra]


def run(data, argv):
    logs = []
    res = T.run_training(data, T.build_parser().parse_args(argv), log=lambda *a: logs.append(" ".join(str(x) for x in a)))
    return res, logs


def file_mrr(out, data, kind=None):
    """The filtered MRR, both sides, of the checkpoint's table over the validation rows, filtered by train + valid."""
    ck = torch.load(T.checkpoint_path(str(out)), weights_only=True)
    emb = ck["embeddings"].cuda().contiguous()
    valid = np.asarray(data.validation_triples, dtype=np.int64)
    known = np.concatenate([np.asarray(data.triples), valid], 0).astype(np.int64)
    cand = np.arange(data.relation_count, data.entity_count, dtype=np.int32)
    sets = EV.constrained_sets(data, kind)[1] if kind else None
    fil = [EV.link_prediction_ranks(emb, valid, cand, known, side, candidate_sets=None if sets is None else sets[side])[1]
           for side in ("tail", "head")]
    return ck, float(np.mean(1.0 / np.concatenate(fil).astype(np.float64)))


@pytest.mark.parametrize("kind", [None, "observed"])
def test_ticks_and_pocket(kg, tmp_path, kind):
    data_dir, data = kg
    out = tmp_path / "run"
    extra = ["--num_epochs", "3", "--softmax_validation_ticks", "2"] + (["--softmax_candidate_sets", kind] if kind else [])
    res, logs = run(data, argv_of(data_dir, out, *extra))
    assert res["steps"] == 12 and not res["stopped_early"]
    ticks = [l for l in logs if "Validation MRR" in l]
    assert len(ticks) == 6 and not any("no validation ticks" in l for l in logs)
    assert [int(l.split("Step")[1].split()[0]) for l in ticks] == [2, 4, 6, 8, 10, 12] == [s for s, _ in res["history"]]
    assert all("hits@10" in l for l in ticks)
    mrrs = [m for _, m in res["history"]]
    print("SOFTMAX validation (%s): history %s" % (kind, res["history"]))
    assert res["pocket_mrr"] == max(mrrs) > 0
    assert res["pocket_step"] == res["history"][mrrs.index(max(mrrs))][0]
    ck, mrr = file_mrr(out, data, kind)
    assert abs(float(F32(mrr)) - res["pocket_mrr"]) <= RT.MRR_TOL, (mrr, res["pocket_mrr"])
    assert ck["global_step"] == res["pocket_step"] and ck["validation_mrr"] == res["pocket_mrr"]
    acc = ck["adagrad_accumulator"]
    assert acc.shape == ck["embeddings"].shape and float(acc.min()) >= F32(0.1) and float(acc.max()) > 0.1
    if kind is None:
        # --resume_checkpoint restores the best: at learning rate 0 every tick ties with it, so nothing is saved again
        before = open(T.checkpoint_path(str(out)), "rb").read()
        res2, logs2 = run(data, argv_of(data_dir, out, "--num_epochs", "1", "--softmax_validation_ticks", "2", "--resume_checkpoint",
                                        "--learning_rate", "0"))
        assert [m for _, m in res2["history"]] == [res["pocket_mrr"]] * 2
        assert res2["pocket_mrr"] == res["pocket_mrr"] and res2["pocket_step"] == res["pocket_step"]
        assert not any("Model saved" in l for l in logs2) and open(T.checkpoint_path(str(out)), "rb").read() == before


def test_validation_rows(kg, tmp_path):
    data_dir, data = kg
    res, logs = run(data, argv_of(data_dir, tmp_path / "run", "--num_epochs", "1", "--softmax_validation_ticks", "1",
                                  "--softmax_validation_rows", "100"))
    ticks = [l for l in logs if "Validation MRR" in l]
    assert len(ticks) == 1 and "200 rows" in ticks[0] and [s for s, _ in res["history"]] == [4]


def test_early_stopping(kg, tmp_path):
    """Learning rate 0: the table cannot change, so every tick after the first returns the same bits -- no improvement --
    and --softmax_patience 2 stops the run after the third tick."""
    data_dir, data = kg
    out = tmp_path / "run"
    res, logs = run(data, argv_of(data_dir, out, "--num_epochs", "5", "--softmax_validation_ticks", "2", "--softmax_patience", "2",
                                  "--learning_rate", "0"))
    assert res["stopped_early"] is True and res["steps"] == 6
    assert [s for s, _ in res["history"]] == [2, 4, 6] and len({m for _, m in res["history"]}) == 1
    assert res["pocket_step"] == 2 and res["pocket_mrr"] == res["history"][0][1]
    assert any("no improvement in 2 validation ticks" in l for l in logs)
    ck, mrr = file_mrr(out, data)
    assert ck["global_step"] == 2 and abs(float(F32(mrr)) - res["pocket_mrr"]) <= RT.MRR_TOL


def test_no_validation_triples(kg, tmp_path):
    data_dir, data = kg
    import copy
    bare = copy.copy(data)
    bare.validation_triples = None
    with pytest.raises(ValueError, match="validation triples"):
        run(bare, argv_of(data_dir, tmp_path / "run", "--softmax_validation_ticks", "2"))


def test_learning(kg, tmp_path):
    """300 steps at the settings of test_gpu_softmax.test_learning (batch 512, scale 20, learning rate 0.1, accumulator
    0.1) with a tick per epoch: the pocket's MRR on the held-out rows is at least the last tick's, and at least 0.40 (the
    floor of test_learning, whose fp64 replay gives 0.457)."""
    data_dir, data = kg
    res, logs = run(data, argv_of(data_dir, tmp_path / "run", "--num_epochs", "1000", "--max_steps", str(TS.STEPS_KG),
                                  "--softmax_validation_ticks", "1", "--adagrad_init", str(TS.A0)))
    assert res["steps"] == TS.STEPS_KG and len(res["history"]) == TS.STEPS_KG // 4
    last = res["history"][-1][1]
    print("SOFTMAX validation learning: pocket MRR %.4f at step %d, last tick %.4f" % (res["pocket_mrr"], res["pocket_step"], last))
    assert res["pocket_mrr"] >= last
    assert res["pocket_mrr"] >= 0.40
