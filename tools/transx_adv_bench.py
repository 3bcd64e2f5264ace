"""The self-adversarial training step of TransE / TransH / TransD timed beside their hinge step, for information
(DESIGN.md section 29).

    python tools/transx_adv_bench.py [--steps 20] [--calls 5] [--dims 100,200] [--out F]

tools/rotate_adv_bench.py's shape and method: n_ent 14,951, n_rel 1,345, batches drawn by the native loops' own samplers
from the distinct rows of 483,142 synthetic triples; device events around trainer.run over --steps steps, one warm-up
call, the median of --calls calls, every loop of every model alternating in one visit:
  adv_B1024_K256   the self-adversarial loop, B 1,024 positives with K 256 negatives each
  adv_B4096_K64    the same at B 4,096, K 64
  hinge_B4096      the hinge loop at B 4,096
One JSON line with, per d, model and loop, step_us and -- for the two self-adversarial shapes -- grad_row_bytes, the bytes
of gradient rows written by the gradient kernel and read again by the apply stage, (K + 3) B d 4 per plane each way (TransD
has two planes on every slot, TransH a second one on the relation slots alone), and hbm_share, the share of the 8.0 TB/s
HBM peak that 2 x grad_row_bytes / step time is.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphembeddings_amd import transx  # noqa: E402

E, R, T = 14951, 1345, 483142
HBM_PEAK = 8.0e12                       # bytes / s, the MI355X's specified peak
MODELS = ("transe", "transh", "transd")
SHAPES = {"adv_B1024_K256": (1024, 256), "adv_B4096_K64": (4096, 64), "hinge_B4096": (4096, None)}


def grad_row_bytes(model, B, K, d):
    """Bytes of gradient rows the kernel writes: plane 0 on every slot; plane 1 on every slot (TransD) or on the B relation
    slots (TransH)."""
    slots = (K + 3) * B
    return (slots + {"transe": 0, "transh": B, "transd": slots}[model]) * d * 4


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--dims", default="100,200")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("transx_adv_bench needs an MI355X: there is no CPU path to time")
    rng = np.random.default_rng(0)
    rel = np.minimum((rng.pareto(0.8, T)).astype(np.int64), R - 1)
    tri = np.unique(np.stack([rng.integers(0, E, T), rng.integers(0, E, T), rel], 1), axis=0)
    out = {"shape": {"n_ent": E, "n_rel": R, "triples": int(len(tri))}, "steps_per_call": a.steps, "calls": a.calls,
           "device": torch.cuda.get_device_name(0)}
    for d in (int(x) for x in a.dims.split(",")):
        trainers = {}
        for model in MODELS:
            for name, (B, K) in SHAPES.items():
                m = transx.TransX(model, E, R, d, l1=True, seed=0)
                kw = dict(loss="self_adversarial", negatives=K, adversarial_temperature=1.0, margin=6.0) if K else dict(margin=1.0)
                trainers[model, name] = m.trainer(tri, B, learning_rate=0.001, seed=1, **kw)
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
        res = {}
        for (model, name), times in step.items():
            B, K = SHAPES[name]
            us = float(np.median(times))
            r = {"B": B, "step_us": us, "step_us_all": [round(x, 2) for x in times]}
            if K:
                nbytes = grad_row_bytes(model, B, K, d)
                r.update(K=K, grad_row_bytes=nbytes, hbm_share=2 * nbytes / (us * 1e-6) / HBM_PEAK)
            res.setdefault(model, {})[name] = r
        out["d%d" % d] = res
        del trainers
        torch.cuda.empty_cache()
    line = json.dumps(out, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
