"""RotatE's step and two-sided filtered evaluation timed beside TransE's, for information.

    python tools/rotate_bench.py [--steps 200] [--calls 5] [--test 2000] [--out F]

One FB15k-like shape: n_ent 14,951, n_rel 1,345, d 200 for both models (RotatE: 100 complex coordinates), B 4,096 pairs
drawn by the native loop's own sampler from the distinct rows of 483,142 synthetic triples (483,031 with the tool's
seed; the JSON line's `triples`).  One JSON line with, per model:
  step_us   the native loop (trainer.run) over --steps steps, device events around the call, median of --calls calls
            after one warm-up call, the two models alternating
  eval_ms   evaluate_translation (tails and heads, filtered by the training triples + the test rows) of --test rows: a
            host clock around the call, which ends in device-to-host copies; median of --calls, alternating
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphembeddings_amd import evaluate as EV  # noqa: E402
from graphembeddings_amd import rotate, transx  # noqa: E402

E, R, D, B, T = 14951, 1345, 200, 4096, 483142


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--test", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("rotate_bench needs an MI355X: there is no CPU path to time")
    rng = np.random.default_rng(0)
    # relation frequencies fall off as in FB15k (Zipf-like): a few hot relation rows per batch
    rel = np.minimum((rng.pareto(0.8, T)).astype(np.int64), R - 1)
    tri = np.unique(np.stack([rng.integers(0, E, T), rng.integers(0, E, T), rel], 1), axis=0)
    test = tri[rng.permutation(len(tri))[:a.test]]
    models = {"rotate": rotate.RotatE(E, R, D, l1=True, seed=0), "transe": transx.TransX("transe", E, R, D, l1=True, seed=0)}
    trainers = {k: m.trainer(tri, B, margin=1.0, learning_rate=0.001, seed=1) for k, m in models.items()}
    for tr in trainers.values():
        tr.run(a.steps)
    step = {k: [] for k in models}
    for _ in range(a.calls):
        for k, tr in trainers.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.run(a.steps)
            e1.record()
            e1.synchronize()
            step[k].append(e0.elapsed_time(e1) * 1e3 / a.steps)
    ev, res = {k: [] for k in models}, {}
    for k, m in models.items():
        EV.evaluate_translation(m, test[:64], tri)
    for _ in range(a.calls):
        for k, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[k] = EV.evaluate_translation(m, test, tri)
            ev[k].append((time.perf_counter() - t0) * 1e3)
    out = {"shape": {"n_ent": E, "n_rel": R, "d": D, "B": B, "triples": int(len(tri)), "test_rows": int(len(test))},
           "steps_per_call": a.steps, "calls": a.calls, "device": torch.cuda.get_device_name(0)}
    for k in models:
        out[k] = {"step_us": float(np.median(step[k])), "step_us_all": [round(x, 2) for x in step[k]],
                  "eval_ms": float(np.median(ev[k])), "eval_ms_all": [round(x, 1) for x in ev[k]],
                  "filtered_mrr": res[k]["filtered_mrr"]}
    line = json.dumps(out, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
