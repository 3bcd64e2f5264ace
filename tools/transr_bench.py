"""TransR step timing at FB15k shape (E=14,951, R=1,345, dim_e = dim_r = 100, B=4,831 = 483,142 // 100): the
native loop (`Trainer.run`, 100 steps per call, median of --calls calls), the same step in torch eager on the GPU
(autograd of the reference's loss, then torch.optim.Adam on the dense gradients: every element decays, as TF1's
Adam does), and the same step in torch eager on the host with --threads threads.

    python tools/transr_bench.py [--calls 5] [--steps 100] [--gpu_eager_steps 20] [--cpu_steps 3] [--threads 16]
                                 [--l2] [--out FILE]
    python tools/transr_bench.py --stats KERNEL_STATS_CSV       (no GPU: per-kernel split of a rocprofv3 run)

Prints one JSON line.  Synthetic triples with FB15k's shape and a Zipf-like relation column (as transx_bench.py).
The Adam pass's algorithmic traffic is 24 bytes per element of the three tables (x, m, v read and written)."""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

E, R, DE, DR, T = 14951, 1345, 100, 100, 483142


def adam_bytes(E=E, R=R, de=DE, dr=DR):
    return 24 * (E * de + R * dr + R * dr * de)


def fb15k_like(seed=0):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, R + 1) ** 1.1
    r = rng.choice(R, size=T, p=w / w.sum())
    tri = np.stack([rng.integers(0, E, T), rng.integers(0, E, T), r], 1)
    return np.unique(tri, axis=0)


def eager_step(P, opt, pos, neg, margin, l1):
    """One eager step: autograd of sum max(D+ - D- + margin, 0), then Adam on every element."""
    import torch
    opt.zero_grad(set_to_none=False)
    M = P["rel_matrix"][pos[:, 2]].view(-1, DR, DE)

    def dist(t):
        u = torch.bmm(M, (P["ent"][t[:, 0]] - P["ent"][t[:, 1]]).unsqueeze(2)).squeeze(2) + P["rel"][t[:, 2]]
        return u.abs().sum(1) if l1 else (u * u).sum(1)

    loss = torch.clamp(dist(pos) - dist(neg) + margin, min=0).sum()
    loss.backward()
    opt.step()
    return loss.detach()


def time_eager(tables, pos, neg, steps, device, l1):
    import torch
    P = {k: v.detach().to(device).clone().requires_grad_(True) for k, v in tables.items()}
    opt = torch.optim.Adam(list(P.values()), lr=0.001, betas=(0.9, 0.999), eps=1e-8)
    pos, neg = pos.to(device).long(), neg.to(device).long()
    eager_step(P, opt, pos, neg, 1.0, l1)                   # warm-up (allocates the moments)
    if device != "cpu":
        torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        eager_step(P, opt, pos, neg, 1.0, l1)
    if device != "cpu":
        torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6 / steps


def summarise_stats(path, steps_total):
    """Per-kernel split of a rocprofv3 --stats CSV: us per step and share, plus the Adam pass's bytes/s."""
    rows = []
    for i, row in enumerate(csv.reader(open(path))):
        if i == 0 or not row or row[0].startswith("#"):
            continue
        name = re.sub(r"\(.*", "", row[0])
        name = "rocprim radix sort" if "rocprim" in name else name.replace("void ge::", "")
        rows.append((name, int(row[1]), float(row[2]) * 1e-3))      # TotalDurationNs -> us
    agg = {}
    for name, calls, total in rows:
        c, t = agg.get(name, (0, 0.0))
        agg[name] = (c + calls, t + total)
    tot = sum(t for _, t in agg.values())
    out = {"kernels": {k: {"calls": c, "us_per_step": round(t / steps_total, 2), "share": round(t / tot, 4)}
                       for k, (c, t) in sorted(agg.items(), key=lambda x: -x[1][1])}}
    adam = [(c, t) for k, (c, t) in agg.items() if "transr_adam_kernel" in k]
    if adam:
        c, t = adam[0]
        us = t / c
        out["adam_us"] = round(us, 2)
        out["adam_algorithmic_TBps"] = round(adam_bytes() / (us * 1e-6) / 1e12, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--gpu_eager_steps", type=int, default=20)
    ap.add_argument("--cpu_steps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--l2", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats", default=None, help="summarise this rocprofv3 kernel_stats.csv and exit")
    ap.add_argument("--stats_steps", type=int, default=None, help="steps the profiled run took (default: calls+1 x steps)")
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(summarise_stats(a.stats, a.stats_steps or (a.calls + 1) * a.steps)))
        return
    import torch
    from graphembeddings_amd import transr as XR
    tri = fb15k_like()
    B = len(tri) // 100
    l1 = not a.l2
    torch.set_num_threads(a.threads)
    m = XR.TransR(E, R, DE, DR, l1=l1, seed=0)
    tr = m.trainer(tri, B, margin=1.0, learning_rate=0.001, seed=1)
    tr.run(a.steps)                                          # warm-up call
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for _ in range(a.calls):
        t0.record()
        losses = tr.run(a.steps)
        t1.record()
        t1.synchronize()
        per.append(t0.elapsed_time(t1) * 1e3 / a.steps)
    assert torch.isfinite(losses).all()
    us = float(np.median(per))
    tabs = {k: v.detach().clone() for k, v in m.tables.items()}
    pos, neg = tr.draw(0)
    gpu_us = time_eager(tabs, pos, neg, a.gpu_eager_steps, "cuda", l1) if a.gpu_eager_steps > 0 else None
    cpu_us = time_eager({k: v.cpu() for k, v in tabs.items()}, pos.cpu(), neg.cpu(), a.cpu_steps, "cpu", l1) \
        if a.cpu_steps > 0 else None
    rec = {"model": "transr", "norm": "L1" if l1 else "L2", "E": E, "R": R, "dim_e": DE, "dim_r": DR, "B": B,
           "steps_per_call": a.steps, "us_per_step": round(us, 2), "us_per_step_all_calls": [round(x, 2) for x in per],
           "scored_triples_per_s": round(2 * B / (us * 1e-6)),
           "torch_eager_gpu_us_per_step": None if gpu_us is None else round(gpu_us, 1),
           "torch_eager_cpu_us_per_step": None if cpu_us is None else round(cpu_us, 1), "cpu_threads": a.threads,
           "adam_algorithmic_bytes_per_step": adam_bytes(), "last_loss": float(losses[-1])}
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
