"""TransX step timing at FB15k shape (E=14,951, R=1,345, d=100, B=4,831 = 483,142 // 100): the native loop
(`Trainer.run`, 100 steps per call) for each model and norm, and the same step in torch eager fp32 on the host.

    python tools/transx_bench.py [--calls 5] [--steps 100] [--cpu_steps 5] [--threads 16] [--out FILE]
                                 [--optimizer sgd|adagrad|both]

Prints one JSON line per configuration.  --optimizer both times the SGD loop and the AdaGrad loop
(ge_transx_train_steps_adagrad) of one shape alternated call by call in one process, each on its own model, at the same
learning rate, so that the two lines of a shape compare like with like.  Synthetic triples with FB15k's shape; a
relation column drawn with a Zipf-like skew so the busiest relation gets hundreds of slots per step, as FB15k's do."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphembeddings_amd import transx as X  # noqa: E402

E, R, D, T = 14951, 1345, 100, 483142


def fb15k_like(seed=0):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, R + 1) ** 1.1
    r = rng.choice(R, size=T, p=w / w.sum())
    tri = np.stack([rng.integers(0, E, T), rng.integers(0, E, T), r], 1)
    return np.unique(tri, axis=0)


def cpu_step(model, tabs, pos, neg, lr, margin, l1):
    """One eager fp32 step on the host: autograd of the reference's loss, then the sparse SGD update."""
    T_ = {k: v.detach().requires_grad_(True) for k, v in tabs.items()}

    def proj(e, r):
        x = T_["ent"][e]
        if model == "transh":
            n = torch.nn.functional.normalize(T_["normal_vector"][r], dim=1, eps=1e-6)
            return x - (x * n).sum(1, keepdim=True) * n
        if model == "transd":
            return x + (x * T_["ent_transfer"][e]).sum(1, keepdim=True) * T_["rel_transfer"][r]
        return x

    def dist(t):
        u = proj(t[:, 0], t[:, 2]) + T_["rel"][t[:, 2]] - proj(t[:, 1], t[:, 2])
        return u.abs().sum(1) if l1 else (u * u).sum(1)

    loss = torch.clamp(dist(pos) - dist(neg) + margin, min=0).sum()
    loss.backward()
    with torch.no_grad():
        for k, v in tabs.items():
            v.sub_(lr * T_[k].grad)
    return float(loss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--cpu_steps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--optimizer", choices=("sgd", "adagrad", "both"), default="sgd")
    a = ap.parse_args()
    opts = ("sgd", "adagrad") if a.optimizer == "both" else (a.optimizer,)
    tri = fb15k_like()
    B = len(tri) // 100
    lines = []
    torch.set_num_threads(a.threads)
    for model in ("transe", "transh", "transd"):
        for l1 in (True, False):
            ms = {o: X.TransX(model, E, R, D, l1=l1, seed=0) for o in opts}
            trs = {o: ms[o].trainer(tri, B, margin=1.0, learning_rate=0.001, seed=1, optimizer=o) for o in opts}
            for o in opts:
                trs[o].run(a.steps)                           # warm-up call
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            pers, last = {o: [] for o in opts}, {}
            for _ in range(a.calls):
                for o in opts:
                    t0.record()
                    last[o] = trs[o].run(a.steps)
                    t1.record()
                    t1.synchronize()
                    pers[o].append(t0.elapsed_time(t1) * 1e3 / a.steps)
            assert all(torch.isfinite(x).all() for x in last.values())
            m, tr = ms[opts[0]], trs[opts[0]]
            cpu_us = None
            if a.cpu_steps > 0:
                tabs = {k: v.cpu().clone() for k, v in m.tables.items()}
                pos, neg = (t.cpu().long() for t in tr.draw(0))
                cpu_step(model, tabs, pos, neg, 0.001, 1.0, l1)
                t = time.perf_counter()
                for _ in range(a.cpu_steps):
                    cpu_step(model, tabs, pos, neg, 0.001, 1.0, l1)
                cpu_us = (time.perf_counter() - t) * 1e6 / a.cpu_steps
            for o in opts:
                per, losses = pers[o], last[o]
                us = float(np.median(per))
                rec = {"model": model, "norm": "L1" if l1 else "L2", "E": E, "R": R, "d": D, "B": B,
                       "steps_per_call": a.steps, "us_per_step": round(us, 2), "us_per_step_all_calls": [round(x, 2) for x in per],
                       "scored_triples_per_s": round(2 * B / (us * 1e-6)), "cpu_eager_us_per_step": None if cpu_us is None else round(cpu_us, 1),
                       "cpu_threads": a.threads, "last_loss": float(losses[-1])}
                if a.optimizer != "sgd":
                    rec["optimizer"] = o
                print(json.dumps(rec), flush=True)
                lines.append(rec)
            del m, tr, ms, trs
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
