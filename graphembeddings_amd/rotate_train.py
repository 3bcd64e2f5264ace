"""`python -m graphembeddings_amd.rotate_train`: the driver of RotatE, after transr_train.

Reads relation2id.txt, entity2id.txt and triple2id.txt from --data_dir, trains for --train_times epochs of
--nbatches batches of triples // nbatches pairs with SGD or AdaGrad on the margin hinge (--loss hinge, the default) or on
the paper's self-adversarial negative-sampling loss (--loss self_adversarial: --negatives K filtered negatives per
positive, weighted by a softmax at --adversarial_temperature, --margin = gamma), prints each epoch's summed loss, and saves the tables (and the AdaGrad accumulators) with torch.save as rotate.pt; with --test_file the filtered
ranks over all entities, heads and tails, go to rotate_test.json.  --validation_file adds filtered-MRR validation ticks
during training, as in transx_train: rotate.pt is then the best tick's state.
The flags of operations RotatE does not have (top-k prediction, candidate sets, relation prediction, triple
classification files, nearest neighbours) are not defined.
"""
from __future__ import annotations

import argparse
import math
import sys

from .transx_train import FILTER_HELP, add_validation_flags, check_eval_args, check_training_args, run

MAX_DIM = 1024          # graphembeddings_amd.rotate.MAX_DIM, kept here so that checking flags imports no torch
MAX_NEGATIVES = 1024    # graphembeddings_amd.rotate.MAX_NEGATIVES, likewise


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m graphembeddings_amd.rotate_train", description=__doc__.splitlines()[0])
    p.add_argument("--data_dir", default="./data/", help="directory of the three *2id.txt files")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--l1", dest="l1", action="store_true", help="sum of the complex moduli (the paper's norm, the default)")
    g.add_argument("--l2", dest="l1", action="store_false", help="sum of the squared moduli")
    p.set_defaults(l1=True)
    p.add_argument("--hidden_size", type=int, default=100, help="floats per entity row (even): hidden_size / 2 complex coordinates")
    p.add_argument("--nbatches", type=int, default=100)
    p.add_argument("--train_times", type=int, default=3000)
    p.add_argument("--margin", type=float, default=1.0, help="the hinge's margin; gamma of --loss self_adversarial")
    p.add_argument("--loss", choices=("hinge", "self_adversarial"), default="hinge",
                   help="hinge (the default): one negative per positive; self_adversarial: the paper's negative-sampling "
                        "loss over --negatives negatives per positive")
    p.add_argument("--negatives", type=int, default=None,
                   help=f"negatives per positive, 1 to {MAX_NEGATIVES} (with --loss self_adversarial; default 64)")
    p.add_argument("--adversarial_temperature", type=float, default=None,
                   help="alpha >= 0 of the softmax over a positive's negatives, 0: uniform weights (with --loss "
                        "self_adversarial; default 1.0)")
    p.add_argument("--learning_rate", type=float, default=0.001)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--optimizer", choices=("sgd", "adagrad"), default="sgd",
                   help="sgd (the default) or adagrad: TF1's AdagradOptimizer rule on both tables; the saved file then "
                        "carries the accumulators and --load restores them")
    p.add_argument("--adagrad_init", type=float, default=0.1,
                   help="AdagradOptimizer's initial_accumulator_value (with --optimizer adagrad)")
    p.add_argument("--output_dir", default=".", help="where rotate.pt (and rotate_test.json) is written")
    p.add_argument("--test_file", default=None,
                   help="a *2id.txt file of test triples (leading count, then `h t r` rows) ranked after training over "
                        "all entities, heads and tails; " + FILTER_HELP)
    p.add_argument("--filter_file", action="append", default=[],
                   help="a further *2id.txt file of known triples for the filter (repeatable; e.g. valid2id.txt)")
    p.add_argument("--load", default=None, help="a saved state_dict to start from (with --train_times 0: evaluate only)")
    add_validation_flags(p, "rotate")
    p.set_defaults(predict_k=None)                    # what run() and check_eval_args read of the undefined flags
    return p


def check_args(a) -> None:
    """Everything that can be wrong with the flags, before any GPU call."""
    if not 2 <= a.hidden_size <= MAX_DIM or a.hidden_size % 2:
        raise ValueError(f"--hidden_size must be even and lie in [2, {MAX_DIM}], got {a.hidden_size}")
    if not a.adagrad_init > 0:
        raise ValueError(f"--adagrad_init must be positive, got {a.adagrad_init}")
    if a.loss != "self_adversarial":
        if a.negatives is not None or a.adversarial_temperature is not None:
            raise ValueError("--negatives and --adversarial_temperature need --loss self_adversarial")
    else:
        if a.negatives is None:
            a.negatives = 64
        if a.adversarial_temperature is None:
            a.adversarial_temperature = 1.0
        if not 1 <= a.negatives <= MAX_NEGATIVES:
            raise ValueError(f"--negatives must lie in [1, {MAX_NEGATIVES}], got {a.negatives}")
        if not math.isfinite(a.adversarial_temperature) or a.adversarial_temperature < 0:
            raise ValueError(f"--adversarial_temperature must be finite and >= 0, got {a.adversarial_temperature}")
        if not math.isfinite(a.margin):
            raise ValueError(f"--margin must be finite, got {a.margin}")
    check_training_args(a)
    if a.seed < 0:
        raise ValueError(f"--seed must be non-negative, got {a.seed}")
    check_eval_args(a)


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    check_args(a)
    from .rotate import RotatE
    kw = dict(loss=a.loss, negatives=a.negatives, adversarial_temperature=a.adversarial_temperature) \
        if a.loss == "self_adversarial" else {}
    return run(a, "rotate_train", lambda E, R: RotatE(E, R, a.hidden_size, l1=a.l1, seed=a.seed), "rotate", trainer_kw=kw)


if __name__ == "__main__":
    sys.exit(main())
