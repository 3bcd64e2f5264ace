"""`python -m graphembeddings_amd.transx_train`: the driver of transE.py / transH.py / transD.py.

Reads relation2id.txt, entity2id.txt and triple2id.txt from --data_dir, trains for --train_times epochs of
--nbatches batches of triples // nbatches pairs (Config, transE.py:12-21), prints each epoch's summed loss as the
reference does, and saves the tables with torch.save (TF's model.vec checkpoint format is not reproduced).
--loss self_adversarial trains on the self-adversarial negative-sampling loss of Sun et al. 2019 instead of the margin
hinge: --negatives K filtered negatives per positive, weighted by a softmax at --adversarial_temperature, --margin = gamma.
--validation_file adds filtered-MRR validation ticks during training (evaluate.TranslationPocket): the saved state is the
best tick's, --patience stops early, <model>_validation.json records the ticks.
The flags, checks and run() both translation drivers share live here; transr_train adds TransR's own.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

MAX_NEGATIVES = 1024    # graphembeddings_amd.transx.MAX_NEGATIVES, kept here so that checking flags imports no torch

FILTER_HELP = ("filtered evaluation (Bordes et al.): the filter is triple2id.txt + the --test_file + every --filter_file; "
               "unlike the ComplEx evaluator, which filters train + valid as holE.py does")


def add_common_flags(p: argparse.ArgumentParser, dims, out: str) -> None:
    """The flags of transx_train and transr_train, with the model's int size flags `dims` (default 100) after
    --l1 / --l2; `out` names the files written."""
    p.add_argument("--data_dir", default="./data/", help="directory of the three *2id.txt files")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--l1", dest="l1", action="store_true", help="L1 distance (Config.L1_flag = True, the default)")
    g.add_argument("--l2", dest="l1", action="store_false", help="squared L2 distance")
    p.set_defaults(l1=True)
    for flag in dims:
        p.add_argument(f"--{flag}", type=int, default=100)
    p.add_argument("--nbatches", type=int, default=100)
    p.add_argument("--train_times", type=int, default=3000)
    p.add_argument("--margin", type=float, default=1.0)
    p.add_argument("--learning_rate", type=float, default=0.001)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--output_dir", default=".", help=f"where {out}.pt (and {out}_test.json) is written")
    p.add_argument("--test_file", default=None,
                   help="a *2id.txt file of test triples (leading count, then `h t r` rows) ranked after training over "
                        "all entities, heads and tails; " + FILTER_HELP)
    p.add_argument("--filter_file", action="append", default=[],
                   help="a further *2id.txt file of known triples for the filter (repeatable; e.g. valid2id.txt)")
    p.add_argument("--load", default=None, help="a saved state_dict to start from (with --train_times 0: evaluate only)")
    p.add_argument("--predict_k", type=int, default=None,
                   help=f"after the evaluation write {out}_predict.tsv: the top K tails of every distinct (h, r) of the "
                        "--test_file, then the top K heads of every distinct (t, r), over all entities.  Lines: side, "
                        "fixed, relation, position, entity, distance, in_test.  Its filter is triple2id.txt + every "
                        "--filter_file but NOT the test file (unlike the ranking filter), so held-out answers can appear")
    p.add_argument("--candidate_sets", choices=("observed",), default=None,
                   help="with --test_file: also the type-constrained protocol -- each row ranked against the entities seen "
                        "on that side of its relation in triple2id.txt + every --filter_file (not the test file).  Prints "
                        f"a `constrained:` line and adds a `constrained` block to {out}_test.json; with --predict_k the "
                        "tails and heads are predicted from the relation's set only")
    p.add_argument("--relation_ranks", action="store_true",
                   help=f"with --test_file: also rank every test triple's relation among all relations (h, ?, t), same "
                        f"filter; adds a `relation` block to {out}_test.json and prints its line")
    p.add_argument("--predict_relations_k", type=int, default=None,
                   help=f"after the evaluation write {out}_predict_relations.tsv: the top K relations of every distinct "
                        "(h, t) of the --test_file.  Lines: head, tail, position, relation, distance, in_test.  Filter as "
                        "--predict_k: triple2id.txt + every --filter_file, not the test file")
    p.add_argument("--classify", action="store_true",
                   help=f"triple classification after the evaluation: fit one threshold per relation on the --valid_file, "
                        f"classify the --test_file; prints a line, writes {out}_classify.json and {out}_thresholds.tsv.  "
                        "Negatives not given are drawn one per positive by the filtered Bernoulli sampler over "
                        "triple2id.txt + valid + test + every --filter_file")
    p.add_argument("--valid_file", default=None, help="a *2id.txt file of validation triples (for --classify)")
    p.add_argument("--valid_neg_file", default=None, help="false validation triples, same `h t r` id format")
    p.add_argument("--test_neg_file", default=None, help="false test triples, same `h t r` id format")
    p.add_argument("--classify_seed", type=int, default=0, help="seed of the drawn negatives")
    p.add_argument("--neighbors_k", type=int, default=None,
                   help=f"after saving write {out}_neighbors.tsv: the K nearest entities of every entity by the `ent` "
                        "table (lines: query, position, neighbor, distance)")
    p.add_argument("--neighbors_metric", choices=("cosine", "euclidean"), default="cosine",
                   help="the distance of --neighbors_k")
    add_validation_flags(p, out)


def add_validation_flags(p: argparse.ArgumentParser, out: str = "<name>") -> None:
    """--validation_file and the flags that need it (transx_train, transr_train, rotate_train)."""
    p.add_argument("--validation_file", default=None,
                   help="a *2id.txt file of validation triples: every --validation_every epochs (and after the last one) "
                        "they are ranked over all entities, heads and tails, filtered by triple2id.txt + this file + the "
                        f"--test_file + every --filter_file; {out}.pt and everything after training then hold the state "
                        f"of the tick with the best filtered MRR, and {out}_validation.json the ticks")
    p.add_argument("--validation_every", type=int, default=None, help="epochs between validation ticks (default 10)")
    p.add_argument("--validation_rows", type=int, default=None,
                   help="rank only this many validation triples, drawn once with --seed (default: all)")
    p.add_argument("--patience", type=int, default=None,
                   help="stop after this many validation ticks in a row without a better filtered MRR")


def check_validation_args(a) -> None:
    """The four validation flags, read with getattr (a Namespace built without them: no validation); sets the default
    --validation_every."""
    path = getattr(a, "validation_file", None)
    rest = {k: getattr(a, k, None) for k in ("validation_every", "validation_rows", "patience")}
    if path is None:
        given = [k for k, v in rest.items() if v is not None]
        if given:
            raise ValueError("--%s needs --validation_file" % given[0])
        return
    for k, v in rest.items():
        if v is not None and v < 1:
            raise ValueError(f"--{k} must be >= 1, got {v}")
    if not os.path.isfile(path):
        raise ValueError(f"no such file: {path}")
    if rest["validation_every"] is None:
        a.validation_every = 10


def check_training_args(a) -> None:
    if a.nbatches <= 0 or a.train_times < 0:
        raise ValueError("--nbatches must be positive and --train_times non-negative")
    if not a.learning_rate > 0 or a.margin != a.margin:
        raise ValueError("--learning_rate must be positive and --margin a number")


def check_eval_args(a) -> None:
    if a.filter_file and not a.test_file:
        raise ValueError("--filter_file needs --test_file")
    if a.predict_k is not None:
        if not a.test_file:
            raise ValueError("--predict_k needs --test_file")
        if a.predict_k < 1:
            raise ValueError(f"--predict_k must be >= 1, got {a.predict_k}")
    if getattr(a, "candidate_sets", None) is not None:
        if a.candidate_sets != "observed":
            raise ValueError(f"--candidate_sets must be 'observed', got {a.candidate_sets!r}")
        if not a.test_file:
            raise ValueError("--candidate_sets needs --test_file")
    if getattr(a, "relation_ranks", False) and not a.test_file:
        raise ValueError("--relation_ranks needs --test_file")
    rel_k = getattr(a, "predict_relations_k", None)     # (a Namespace built without the flag: none)
    if rel_k is not None:
        if not a.test_file:
            raise ValueError("--predict_relations_k needs --test_file")
        if rel_k < 1:
            raise ValueError(f"--predict_relations_k must be >= 1, got {rel_k}")
    neighbors_k = getattr(a, "neighbors_k", None)       # (a Namespace built without the flag: none)
    if neighbors_k is not None and neighbors_k < 1:
        raise ValueError(f"--neighbors_k must be >= 1, got {neighbors_k}")
    classify_files = [getattr(a, k, None) for k in ("valid_file", "valid_neg_file", "test_neg_file")]
    if getattr(a, "classify", False):
        if not a.test_file or not a.valid_file:
            raise ValueError("--classify needs --test_file and --valid_file")
        if a.classify_seed < 0:
            raise ValueError(f"--classify_seed must be non-negative, got {a.classify_seed}")
    elif any(classify_files):
        raise ValueError("--valid_file, --valid_neg_file and --test_neg_file need --classify")
    for path in ([a.test_file] if a.test_file else []) + list(a.filter_file) + ([a.load] if a.load else []) \
            + [f for f in classify_files if f]:
        if not os.path.isfile(path):
            raise ValueError(f"no such file: {path}")
    check_validation_args(a)


def validation_line(epoch: int, step: int, m: dict) -> str:
    return (f"Epoch {epoch} Step {step} Validation MRR: {m['filtered_mrr']:.6f} (hits@10 {m['hits10']:.2f} %)"
            + (" *" if m["improved"] else ""))


def run(a, driver: str, make_model, name: str, trainer_kw=None) -> int:
    """Everything after the flags are checked: read --data_dir, build make_model(E, R), --load, train (with
    --validation_file: a validation tick every --validation_every epochs, the best tick's state restored after the last,
    <name>_validation.json), save <name>.pt (with --neighbors_k, <name>_neighbors.tsv) and, with --test_file, rank it (heads and tails, printed)
    into <name>_test.json (with --relation_ranks, relations too; with --candidate_sets, the `constrained` block and
    line); with --predict_k, write <name>_predict.tsv (from the relation's set with --candidate_sets); with
    --predict_relations_k, <name>_predict_relations.tsv; with --classify, <name>_classify.json and
    <name>_thresholds.tsv.  trainer_kw: further keywords of the model's trainer() (the loss of transx_train and rotate_train)."""
    import numpy as np
    from .transx import read_kg, read_triples
    E, R, tri = read_kg(a.data_dir)
    B = len(tri) // a.nbatches        # config.batch_size = getTripleTotal() / nbatches
    if B <= 0:
        raise ValueError(f"{len(tri)} triples cannot fill {a.nbatches} batches")
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(f"{driver} needs an MI355X: graphembeddings_amd has no CPU path")
    m = make_model(E, R)
    adagrad = getattr(a, "optimizer", "sgd") == "adagrad"      # (transx_train alone has the flag)
    if a.load:
        state = torch.load(a.load, map_location="cpu")
        m.load_state_dict(state)
        if adagrad and "adagrad_init" not in state:
            print(f"{a.load} holds no AdaGrad accumulators: they start at --adagrad_init {a.adagrad_init}")
    kw = dict(optimizer="adagrad", initial_accumulator_value=getattr(a, "adagrad_init", 0.1)) if adagrad else {}
    tr = m.trainer(tri, B, margin=a.margin, learning_rate=a.learning_rate, seed=a.seed, **kw, **(trainer_kw or {}))
    vp, history, stopped_early, since = None, [], False, 0    # since: ticks in a row without a better MRR
    if getattr(a, "validation_file", None):   # filter: triple2id.txt + validation + test + --filter_file
        from .evaluate import TranslationPocket
        valid = read_triples(a.validation_file, E, R)
        more = [read_triples(f, E, R) for f in ([a.test_file] if a.test_file else []) + list(a.filter_file)]
        vp = TranslationPocket(m, valid, np.concatenate([tri, valid] + more, 0), rows=getattr(a, "validation_rows", None), seed=a.seed)
    for epoch in range(a.train_times):
        res = float(tr.run(a.nbatches).double().sum())
        print(epoch)
        print(res)
        if vp is not None and ((epoch + 1) % a.validation_every == 0 or epoch + 1 == a.train_times):
            vp.tick(tr.step_count)
            (step, mt), = vp.read()           # (the loss above has synchronised this epoch already)
            history.append({"epoch": epoch, "step": step, **mt})
            print(validation_line(epoch, step, mt))
            since = 0 if mt["improved"] else since + 1
            if getattr(a, "patience", None) is not None and since >= a.patience:
                stopped_early = True
                print(f"no better validation MRR in {since} ticks: stopping after epoch {epoch}")
                sys.stdout.flush()
                break
        sys.stdout.flush()
    os.makedirs(a.output_dir, exist_ok=True)
    if vp is not None:                        # the best tick's state: what is saved, evaluated and written from here on
        best_step = vp.restore()
        best = next((h for h in history if h["step"] == best_step and h["improved"]), None)
        json_path = os.path.join(a.output_dir, f"{name}_validation.json")
        with open(json_path, "w") as f:
            json.dump({"history": history, "pocket_mrr": best["filtered_mrr"] if best else None,
                       "pocket_epoch": best["epoch"] if best else None, "pocket_step": best_step,
                       "stopped_early": stopped_early, "rows": vp.V}, f, indent=1, sort_keys=True)
        if best:
            print(f"restored the state of epoch {best['epoch']} (step {best_step}): validation MRR {best['filtered_mrr']:.6f}")
        print(f"wrote {json_path}")
    out = os.path.join(a.output_dir, f"{name}.pt")
    torch.save(m.state_dict(), out)
    print(f"saved {out}")
    if getattr(a, "neighbors_k", None) is not None:
        from .neighbors import write_neighbors
        tsv = os.path.join(a.output_dir, f"{name}_neighbors.tsv")
        n = write_neighbors(tsv, m.tables["ent"].contiguous(), np.arange(E), a.neighbors_k, metric=a.neighbors_metric)
        print(f"wrote {tsv} ({n} lines)")
    if a.test_file:                  # filter: triple2id.txt + test + --filter_file
        from .evaluate import (evaluate_translation, write_translation_predictions,
                               write_translation_relation_predictions)
        test = read_triples(a.test_file, E, R)
        extra = [read_triples(f, E, R) for f in a.filter_file]
        known = np.concatenate([tri, test] + extra, 0)
        sets = None
        if getattr(a, "candidate_sets", None) == "observed":   # from triple2id.txt + --filter_file, not the test file
            from .evaluate import CandidateSets
            seen = np.concatenate([tri] + extra, 0)
            sets = {side: CandidateSets.from_observed(np.arange(E), seen, R, side, device=m.tables["ent"].device)
                    for side in ("tail", "head")}
        res = evaluate_translation(m, test, known, both_sides=True, verbose=True,
                                   relations=bool(getattr(a, "relation_ranks", False)), candidate_sets=sets)
        json_path = os.path.join(a.output_dir, f"{name}_test.json")
        with open(json_path, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
        print(f"wrote {json_path}")
        if a.predict_k is not None:  # filter: triple2id.txt + --filter_file, not the test file
            tsv = os.path.join(a.output_dir, f"{name}_predict.tsv")
            n = write_translation_predictions(m, test, np.concatenate([tri] + extra, 0), a.predict_k, tsv,
                                              candidate_sets=sets)
            print(f"wrote {tsv} ({n} lines)")
        if getattr(a, "predict_relations_k", None) is not None:
            tsv = os.path.join(a.output_dir, f"{name}_predict_relations.tsv")
            n = write_translation_relation_predictions(m, test, np.concatenate([tri] + extra, 0),
                                                       a.predict_relations_k, tsv)
            print(f"wrote {tsv} ({n} lines)")
    if getattr(a, "classify", False):  # negatives drawn against triple2id.txt + valid + test + --filter_file
        from . import classify as C
        test, valid = read_triples(a.test_file, E, R), read_triples(a.valid_file, E, R)
        extra = [read_triples(f, E, R) for f in a.filter_file]
        neg = {k: read_triples(getattr(a, k), E, R) if getattr(a, k) else None for k in ("valid_neg_file", "test_neg_file")}
        res = m.triple_classification(valid, test, neg["valid_neg_file"], neg["test_neg_file"],
                                      known=np.concatenate([tri, valid, test] + extra, 0), seed=a.classify_seed)
        print(C.summary_line(res))
        json_path = os.path.join(a.output_dir, f"{name}_classify.json")
        tsv = os.path.join(a.output_dir, f"{name}_thresholds.tsv")
        C.write_results(res, json_path, tsv)
        print(f"wrote {json_path} and {tsv}")
    return 0


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m graphembeddings_amd.transx_train", description=__doc__.splitlines()[0])
    p.add_argument("--model", choices=("transe", "transh", "transd"), default="transe")
    add_common_flags(p, ("hidden_size",), "<model>")
    p.add_argument("--optimizer", choices=("sgd", "adagrad"), default="sgd",
                   help="sgd: the reference's GradientDescentOptimizer (the default); adagrad: TF1's AdagradOptimizer on "
                        "every table (try --learning_rate 0.05); the saved file then carries the accumulators and --load "
                        "restores them")
    p.add_argument("--adagrad_init", type=float, default=0.1,
                   help="AdagradOptimizer's initial_accumulator_value (with --optimizer adagrad)")
    p.add_argument("--loss", choices=("hinge", "self_adversarial"), default="hinge",
                   help="hinge (the default): the reference's loss, one negative per positive; self_adversarial: the "
                        "negative-sampling loss of Sun et al. 2019 over --negatives negatives per positive (--margin is "
                        "its gamma)")
    p.add_argument("--negatives", type=int, default=None,
                   help=f"negatives per positive, 1 to {MAX_NEGATIVES} (with --loss self_adversarial; default 64)")
    p.add_argument("--adversarial_temperature", type=float, default=None,
                   help="alpha >= 0 of the softmax over a positive's negatives, 0: uniform weights (with --loss "
                        "self_adversarial; default 1.0)")
    return p


def check_loss_args(a) -> None:
    """--loss, --negatives and --adversarial_temperature, with rotate_train's rules and defaults (64 and 1.0)."""
    loss = getattr(a, "loss", "hinge")                   # (a Namespace built without the flags: the hinge)
    negatives, alpha = getattr(a, "negatives", None), getattr(a, "adversarial_temperature", None)
    if loss not in ("hinge", "self_adversarial"):
        raise ValueError(f"--loss must be 'hinge' or 'self_adversarial', got {loss!r}")
    if loss != "self_adversarial":
        if negatives is not None or alpha is not None:
            raise ValueError("--negatives and --adversarial_temperature need --loss self_adversarial")
        return
    a.negatives = 64 if negatives is None else negatives
    a.adversarial_temperature = 1.0 if alpha is None else alpha
    if not 1 <= a.negatives <= MAX_NEGATIVES:
        raise ValueError(f"--negatives must lie in [1, {MAX_NEGATIVES}], got {a.negatives}")
    if not math.isfinite(a.adversarial_temperature) or a.adversarial_temperature < 0:
        raise ValueError(f"--adversarial_temperature must be finite and >= 0, got {a.adversarial_temperature}")
    if not math.isfinite(a.margin):
        raise ValueError(f"--margin must be finite, got {a.margin}")


def check_args(a) -> None:
    """Everything that can be wrong with the flags, before any GPU call."""
    if not 1 <= a.hidden_size <= 1024:
        raise ValueError(f"--hidden_size must lie in [1, 1024], got {a.hidden_size}")
    optimizer, a0 = getattr(a, "optimizer", "sgd"), getattr(a, "adagrad_init", 0.1)   # (a Namespace built without them)
    if optimizer not in ("sgd", "adagrad"):
        raise ValueError(f"--optimizer must be 'sgd' or 'adagrad', got {optimizer!r}")
    if not a0 > 0:
        raise ValueError(f"--adagrad_init must be positive, got {a0}")
    check_loss_args(a)
    check_training_args(a)
    check_eval_args(a)


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    check_args(a)
    from .transx import TransX
    kw = dict(loss=a.loss, negatives=a.negatives, adversarial_temperature=a.adversarial_temperature) \
        if a.loss == "self_adversarial" else {}
    return run(a, "transx_train", lambda E, R: TransX(a.model, E, R, a.hidden_size, l1=a.l1, seed=a.seed), a.model,
               trainer_kw=kw)


if __name__ == "__main__":
    sys.exit(main())
