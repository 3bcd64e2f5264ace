"""GPU: transx_train and rotate_train end to end with --validation_file on a tiny planted KG (E = 200) written to tmp_path:
the ticks land in <name>_validation.json, <name>.pt is the best tick's state, --patience stops early, and without
--validation_file the saved file is bitwise what the training loop alone leaves."""
import json

import numpy as np
import pytest
import torch

from graphembeddings_amd import evaluate as EV
from graphembeddings_amd import rotate, rotate_train, transx, transx_train
from tests import rotate_ref as RR
from tests import transx_ref as XR

pytestmark = pytest.mark.gpu

E, R, D = 200, 5, 16
N_VALID = N_TEST = 40


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")


def _write(path, rows, count=None):
    with open(path, "w") as f:
        f.write(f"{len(rows) if count is None else count}\n")
        for r in rows:
            f.write(" ".join(str(int(x)) for x in r) + "\n")


DRIVERS = {
    "transe": (transx_train, ["--model", "transe", "--learning_rate", "0.05", "--margin", "2"],
               lambda: transx.TransX("transe", E, R, D, l1=True, seed=0)),
    "rotate": (rotate_train, ["--learning_rate", "0.5", "--margin", "3"], lambda: rotate.RotatE(E, R, D, l1=True, seed=0)),
}
SHAKE_LR = {"transe": "3.0", "rotate": "0.1"}      # plain SGD on the hinge at this rate undoes a trained state
ADV = ["--optimizer", "adagrad", "--loss", "self_adversarial", "--negatives", "8", "--adversarial_temperature", "0.5"]


def kg(tmp_path, name):
    if name == "rotate":
        tri = RR.planted_rotation_kg(n_ent=E, n_rel=R, k=4, n_triples=2500, seed=4, sym=1)
    else:
        tri = XR.planted_kg(n_ent=E, n_rel=R, dim=8, n_triples=2500, seed=4)
    train, valid, test = tri[:-(N_VALID + N_TEST)], tri[-(N_VALID + N_TEST):-N_TEST], tri[-N_TEST:]
    d = tmp_path / "data"
    d.mkdir()
    _write(str(d / "entity2id.txt"), [], E)
    _write(str(d / "relation2id.txt"), [], R)
    _write(str(d / "triple2id.txt"), train)
    _write(str(d / "valid2id.txt"), valid)
    _write(str(d / "test2id.txt"), test)
    common = ["--data_dir", str(d), "--hidden_size", str(D), "--nbatches", "4", "--seed", "0"]
    return train, valid, test, d, common


def validation_mrr(model, valid, known, **kw):
    """The filtered MRR (a float32 value) of one tick on the model as it is."""
    vp = EV.TranslationPocket(model, valid, known, keep_state=False, **kw)
    vp.tick(0)
    return vp.read()[0][1]["filtered_mrr"]


@pytest.mark.parametrize("name", sorted(DRIVERS))
def test_ticks_pocket_and_saved_state(tmp_path, capsys, name):
    mod, flags, make = DRIVERS[name]
    train, valid, test, d, common = kg(tmp_path, name)
    out = tmp_path / "out"
    args = common + flags + ADV + ["--output_dir", str(out), "--train_times", "6", "--validation_file", str(d / "valid2id.txt"),
                                   "--validation_every", "2", "--test_file", str(d / "test2id.txt")]
    assert mod.main(args) == 0
    printed = capsys.readouterr().out
    res = json.load(open(out / f"{name}_validation.json"))
    hist = res["history"]
    assert [h["epoch"] for h in hist] == [1, 3, 5] and [h["step"] for h in hist] == [8, 16, 24]
    assert printed.count("Validation MRR:") == 3 and "Epoch 5 Step 24 Validation MRR:" in printed
    mrrs = [h["filtered_mrr"] for h in hist]
    print("VALIDATION DRIVER %s: MRR per tick %s" % (name, mrrs))
    best = int(np.argmax(mrrs))                                          # (argmax: the first on a tie)
    assert res["pocket_mrr"] == mrrs[best] and res["pocket_epoch"] == hist[best]["epoch"] and res["pocket_step"] == hist[best]["step"]
    assert hist[best]["improved"] and not any(h["improved"] for h in hist[best + 1:])
    assert res["stopped_early"] is False and res["rows"] == N_VALID and all(h["counted"] == 2 * N_VALID for h in hist)
    # the saved file: the keys of a run without validation, and the best tick's state
    state = torch.load(out / f"{name}.pt", map_location="cpu")
    m = make()
    assert set(state) == set(dict(m.state_dict(), adagrad_init=0.1, **{"adagrad_" + k: 0 for k in m.tables}))
    m.load_state_dict(state)
    known = np.concatenate([train, valid, test], 0)
    assert validation_mrr(m, valid, known) == res["pocket_mrr"]
    # ... which the test evaluation ran on
    test_json = json.load(open(out / f"{name}_test.json"))
    assert test_json["filtered_mrr"] == EV.evaluate_translation(m, test, np.concatenate([train, test], 0))["filtered_mrr"]
    # --validation_rows: a seeded subset, recorded
    args2 = common + flags + ADV + ["--output_dir", str(tmp_path / "rows"), "--train_times", "2", "--validation_file",
                                    str(d / "valid2id.txt"), "--validation_every", "5", "--validation_rows", "9"]
    assert mod.main(args2) == 0
    res2 = json.load(open(tmp_path / "rows" / f"{name}_validation.json"))
    assert res2["rows"] == 9 and [h["epoch"] for h in res2["history"]] == [1] and res2["history"][0]["counted"] == 18
    m2 = make()
    m2.load_state_dict(torch.load(tmp_path / "rows" / f"{name}.pt", map_location="cpu"))
    assert validation_mrr(m2, valid, np.concatenate([train, valid], 0), rows=9, seed=0) == res2["pocket_mrr"]


@pytest.mark.parametrize("name", sorted(DRIVERS))
def test_patience_stops_at_the_first_tick_that_does_not_improve(tmp_path, capsys, name):
    """A trained state (the best tick's of a validated run) is loaded and then trained on with plain SGD on the hinge at
    a learning rate that undoes it: the first tick ranks worse than the loaded state and the second worse again (both
    asserted from a run without --patience).  A run started with --load starts its best at 0, so the first tick improves,
    the second does not, and --patience 1 stops there: two of the six epochs' three ticks."""
    mod, flags, make = DRIVERS[name]
    train, valid, test, d, common = kg(tmp_path, name)
    good = tmp_path / "good"
    assert mod.main(common + flags + ADV + ["--output_dir", str(good), "--train_times", "40", "--validation_file",
                                            str(d / "valid2id.txt"), "--validation_every", "10"]) == 0
    start = json.load(open(good / f"{name}_validation.json"))["pocket_mrr"]
    shake = common + [f if f != flags[flags.index("--learning_rate") + 1] else SHAKE_LR[name] for f in flags]
    shake = shake + ["--load", str(good / f"{name}.pt"), "--train_times", "6", "--validation_file", str(d / "valid2id.txt"),
                     "--validation_every", "2"]
    free = tmp_path / "free"
    assert mod.main(shake + ["--output_dir", str(free)]) == 0
    mrrs = [h["filtered_mrr"] for h in json.load(open(free / f"{name}_validation.json"))["history"]]
    print("VALIDATION DRIVER %s: shaken MRR per tick %s" % (name, mrrs))
    assert len(mrrs) == 3 and mrrs[1] < mrrs[0] < start                   # the precondition: the second tick is worse
    capsys.readouterr()
    out = tmp_path / "patient"
    assert mod.main(shake + ["--output_dir", str(out), "--patience", "1"]) == 0
    printed = capsys.readouterr().out
    res = json.load(open(out / f"{name}_validation.json"))
    assert res["stopped_early"] is True and [h["epoch"] for h in res["history"]] == [1, 3]
    assert [h["filtered_mrr"] for h in res["history"]] == mrrs[:2]        # the same run, cut short
    assert [h["improved"] for h in res["history"]] == [True, False]
    assert res["pocket_epoch"] == 1 and res["pocket_step"] == 8 and res["pocket_mrr"] == mrrs[0]
    assert "stopping after epoch 3" in printed and "\n4\n" not in printed
    m = make()
    m.load_state_dict(torch.load(out / f"{name}.pt", map_location="cpu"))
    assert validation_mrr(m, valid, np.concatenate([train, valid], 0)) == mrrs[0]
    # --patience 2 is not yet used up after one bad tick
    assert mod.main(shake + ["--output_dir", str(tmp_path / "p2"), "--patience", "2", "--train_times", "4"]) == 0
    assert json.load(open(tmp_path / "p2" / f"{name}_validation.json"))["stopped_early"] is False


@pytest.mark.parametrize("name", sorted(DRIVERS))
def test_without_validation_file_nothing_changes(tmp_path, name):
    """The driver without --validation_file against the loop it has always run, written out here: the same seeds, the same
    calls, the saved tensors bitwise equal -- and against a run with validation at the last epoch only, whose one tick
    (which does not train) pockets that same final state."""
    mod, flags, make = DRIVERS[name]
    train, valid, test, d, common = kg(tmp_path, name)
    out = tmp_path / "plain"
    assert mod.main(common + flags + ADV + ["--output_dir", str(out), "--train_times", "3"]) == 0
    assert not (out / f"{name}_validation.json").exists()
    state = torch.load(out / f"{name}.pt", map_location="cpu")
    m = make()
    lr, margin = float(flags[flags.index("--learning_rate") + 1]), float(flags[flags.index("--margin") + 1])
    tr = m.trainer(train, len(train) // 4, margin=margin, learning_rate=lr, seed=0, optimizer="adagrad",
                   initial_accumulator_value=0.1, loss="self_adversarial", negatives=8, adversarial_temperature=0.5)
    for _ in range(3):
        tr.run(4)
    want = m.state_dict()
    assert set(state) == set(want)
    for k, v in want.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(state[k].view(torch.int32), v.view(torch.int32)), k
        else:
            assert state[k] == v, k
    ticked = tmp_path / "ticked"
    assert mod.main(common + flags + ADV + ["--output_dir", str(ticked), "--train_times", "3", "--validation_file",
                                            str(d / "valid2id.txt"), "--validation_every", "100"]) == 0
    res = json.load(open(ticked / f"{name}_validation.json"))
    assert [h["epoch"] for h in res["history"]] == [2] and res["pocket_epoch"] == 2
    again = torch.load(ticked / f"{name}.pt", map_location="cpu")
    for k, v in want.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(again[k].view(torch.int32), v.view(torch.int32)), k
