"""RotatE's self-adversarial training step timed beside its hinge step, for information.

    python tools/rotate_adv_bench.py [--steps 50] [--calls 5] [--out F]

tools/rotate_bench.py's shape and method: n_ent 14,951, n_rel 1,345, d 200, batches drawn by the native loops' own
samplers from the distinct rows of 483,142 synthetic triples; device events around trainer.run over --steps steps, one
warm-up call, the median of --calls calls, the three loops alternating in one visit:
  adv_B1024_K256   the self-adversarial loop, B 1,024 positives with K 256 negatives each
  adv_B4096_K64    the same at B 4,096, K 64
  hinge_B4096      the hinge loop at B 4,096
One JSON line with, per loop, step_us and -- for the two self-adversarial shapes -- grad_row_bytes, the bytes of gradient
rows written by the gradient kernel and read again by the apply stage, (K + 3) B d 4 each way, and hbm_share, the share
of the 8.0 TB/s HBM peak that 2 x grad_row_bytes / step time is.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphembeddings_amd import rotate  # noqa: E402

E, R, D, T = 14951, 1345, 200, 483142
HBM_PEAK = 8.0e12                       # bytes / s, the MI355X's specified peak
SHAPES = {"adv_B1024_K256": (1024, 256), "adv_B4096_K64": (4096, 64), "hinge_B4096": (4096, None)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("rotate_adv_bench needs an MI355X: there is no CPU path to time")
    rng = np.random.default_rng(0)
    rel = np.minimum((rng.pareto(0.8, T)).astype(np.int64), R - 1)
    tri = np.unique(np.stack([rng.integers(0, E, T), rng.integers(0, E, T), rel], 1), axis=0)
    trainers = {}
    for name, (B, K) in SHAPES.items():
        m = rotate.RotatE(E, R, D, l1=True, seed=0)
        kw = dict(loss="self_adversarial", negatives=K, adversarial_temperature=1.0, margin=6.0) if K else dict(margin=1.0)
        trainers[name] = m.trainer(tri, B, learning_rate=0.001, seed=1, **kw)
    for tr in trainers.values():
        tr.run(a.steps)
    step = {k: [] for k in trainers}
    for _ in range(a.calls):
        for k, tr in trainers.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.run(a.steps)
            e1.record()
            e1.synchronize()
            step[k].append(e0.elapsed_time(e1) * 1e3 / a.steps)
    out = {"shape": {"n_ent": E, "n_rel": R, "d": D, "triples": int(len(tri))}, "steps_per_call": a.steps, "calls": a.calls,
           "device": torch.cuda.get_device_name(0)}
    for k, (B, K) in SHAPES.items():
        us = float(np.median(step[k]))
        out[k] = {"B": B, "step_us": us, "step_us_all": [round(x, 2) for x in step[k]]}
        if K:
            nbytes = (K + 3) * B * D * 4
            out[k].update(K=K, grad_row_bytes=nbytes, hbm_share=2 * nbytes / (us * 1e-6) / HBM_PEAK)
    line = json.dumps(out, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
