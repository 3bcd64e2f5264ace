"""`python -m graphembeddings_amd.transr_train`: the driver of transR.py.

Reads relation2id.txt, entity2id.txt and triple2id.txt from --data_dir, trains for --train_times epochs of
--nbatches batches of triples // nbatches pairs with Adam (Config and AdamOptimizer(0.001), transR.py:12-22, 88),
prints each epoch's summed loss as the reference does, and saves the tables and the Adam state with torch.save
(TF's model.vec checkpoint format is not reproduced).
"""
from __future__ import annotations

import argparse
import os
import sys

from .transx_train import add_eval_flags, check_eval_args, evaluate_to_json

MAX_DIM = 256           # graphembeddings_amd.transr.MAX_DIM, kept here so that checking flags imports no torch


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m graphembeddings_amd.transr_train", description=__doc__.splitlines()[0])
    p.add_argument("--data_dir", default="./data/", help="directory of the three *2id.txt files")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--l1", dest="l1", action="store_true", help="L1 distance (Config.L1_flag = True, the default)")
    g.add_argument("--l2", dest="l1", action="store_false", help="squared L2 distance")
    p.set_defaults(l1=True)
    p.add_argument("--hidden_size_e", type=int, default=100)
    p.add_argument("--hidden_size_r", type=int, default=100)
    p.add_argument("--nbatches", type=int, default=100)
    p.add_argument("--train_times", type=int, default=3000)
    p.add_argument("--margin", type=float, default=1.0)
    p.add_argument("--learning_rate", type=float, default=0.001)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--output_dir", default=".", help="where transr.pt (and transr_test.json) is written")
    add_eval_flags(p)
    return p


def check_args(a) -> None:
    """Everything that can be wrong with the flags, before any GPU call."""
    for flag in ("hidden_size_e", "hidden_size_r"):
        if not 1 <= getattr(a, flag) <= MAX_DIM:
            raise ValueError(f"--{flag} must lie in [1, {MAX_DIM}], got {getattr(a, flag)}")
    if a.nbatches <= 0 or a.train_times < 0:
        raise ValueError("--nbatches must be positive and --train_times non-negative")
    if not a.learning_rate > 0 or a.margin != a.margin:
        raise ValueError("--learning_rate must be positive and --margin a number")
    if a.seed < 0:
        raise ValueError(f"--seed must be non-negative, got {a.seed}")
    check_eval_args(a)


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    check_args(a)
    from . import transr as TR
    E, R, tri = TR.read_kg(a.data_dir)
    B = len(tri) // a.nbatches        # config.batch_size = getTripleTotal() / nbatches
    if B <= 0:
        raise ValueError(f"{len(tri)} triples cannot fill {a.nbatches} batches")
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("transr_train needs an MI355X: graphembeddings_amd has no CPU path")
    m = TR.TransR(E, R, a.hidden_size_e, a.hidden_size_r, l1=a.l1, seed=a.seed)
    if a.load:
        m.load_state_dict(torch.load(a.load, map_location="cpu"))
    tr = m.trainer(tri, B, margin=a.margin, learning_rate=a.learning_rate, seed=a.seed)
    for epoch in range(a.train_times):
        res = float(tr.run(a.nbatches).double().sum())
        print(epoch)
        print(res)
        sys.stdout.flush()
    os.makedirs(a.output_dir, exist_ok=True)
    out = os.path.join(a.output_dir, "transr.pt")
    torch.save(m.state_dict(), out)
    print(f"saved {out}")
    if a.test_file:
        evaluate_to_json(m, a, E, R, tri, os.path.join(a.output_dir, "transr_test.json"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
