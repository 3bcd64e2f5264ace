"""`python -m graphembeddings_amd.transr_train`: the driver of transR.py.

Reads relation2id.txt, entity2id.txt and triple2id.txt from --data_dir, trains for --train_times epochs of
--nbatches batches of triples // nbatches pairs with Adam (Config and AdamOptimizer(0.001), transR.py:12-22, 88),
prints each epoch's summed loss as the reference does, and saves the tables and the Adam state with torch.save
(TF's model.vec checkpoint format is not reproduced).
"""
from __future__ import annotations

import argparse
import sys

from .transx_train import add_common_flags, check_eval_args, check_training_args, run

MAX_DIM = 256           # graphembeddings_amd.transr.MAX_DIM, kept here so that checking flags imports no torch


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m graphembeddings_amd.transr_train", description=__doc__.splitlines()[0])
    add_common_flags(p, ("hidden_size_e", "hidden_size_r"), "transr")
    return p


def check_args(a) -> None:
    """Everything that can be wrong with the flags, before any GPU call."""
    for flag in ("hidden_size_e", "hidden_size_r"):
        if not 1 <= getattr(a, flag) <= MAX_DIM:
            raise ValueError(f"--{flag} must lie in [1, {MAX_DIM}], got {getattr(a, flag)}")
    check_training_args(a)
    if a.seed < 0:
        raise ValueError(f"--seed must be non-negative, got {a.seed}")
    check_eval_args(a)


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    check_args(a)
    from .transr import TransR
    return run(a, "transr_train", lambda E, R: TransR(E, R, a.hidden_size_e, a.hidden_size_r, l1=a.l1, seed=a.seed),
               "transr")


if __name__ == "__main__":
    sys.exit(main())
