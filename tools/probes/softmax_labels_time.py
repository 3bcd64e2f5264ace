"""Time per call of the multi-label (K-vs-all) softmax next to the 1-vs-all one, in one process, between device events, at
(B, K, d) = (4096, 14951, 200) on a 16,296-row table (norms on both sides of the clip).  3 warm-up calls, then three
windows of `calls` calls, ge_softmax_grad on the same queries alternated with every figure.  One JSON line per figure:
  1. ge_softmax_labels_grad at a mean of 1, 3 and 10 labels a row (n_i = 1; 1 ... 5; 1 ... 19, distinct random positions)
     against ge_softmax_grad with each row's first label as its true candidate;
  2. LabelSoftmaxAdaGrad.step (4,096 rows a side, mean 3 labels) against SoftmaxAdaGrad.step on 4,096 triples."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from graphembeddings_amd import data as D
from graphembeddings_amd import hole as H

DIM, B = 200, 4096


def windows(fn, calls, n=3):
    for _ in range(3):
        fn()
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(round(e0.elapsed_time(e1) / calls, 4))
    return out


def table(n_rows, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randn(n_rows, DIM, device="cuda", generator=g)
    norms = torch.exp(0.5 * torch.randn(n_rows, 1, device="cuda", generator=g))
    return (t * (norms / t.norm(dim=1, keepdim=True))).contiguous()


def labels(rng, K, most):
    rows = [rng.choice(K, 1 + i % most, replace=False) for i in range(B)]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return off, np.concatenate(rows).astype(np.int32)


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    fb = D.fb15k_shape()
    n_rel, N = fb.relation_count, fb.entity_count
    K = N - n_rel
    rng = np.random.default_rng(0)
    emb = table(N)
    cand = torch.arange(n_rel, N, dtype=torch.int32, device="cuda")
    hr = torch.as_tensor(np.stack([rng.integers(n_rel, N, B), rng.integers(0, n_rel, B)], 1).astype(np.int32)).cuda()
    med = lambda v: sorted(v)[len(v) // 2]
    step_batch = None
    for most in (1, 5, 19):
        off, pos = labels(rng, K, most)
        o, p = torch.as_tensor(off).cuda(), torch.as_tensor(pos).cuda()
        true = cand[p[o[:-1].long()].long()].contiguous()
        L = len(pos)
        ws, ws1 = H.softmax_labels_workspace(emb, B, K, L), H.softmax_workspace(emb, B, K)
        out = (torch.empty(K + 2 * B + L, dtype=torch.int32, device="cuda"), torch.empty(K + 2 * B + L, DIM, device="cuda"))
        out1 = (out[0][:K + 2 * B], out[1][:K + 2 * B])
        lab = windows(lambda: H.softmax_labels_grad(emb, hr, o, p, cand, 1.0, scale=20.0, workspace=ws, out=out), calls)
        one = windows(lambda: H.softmax_grad(emb, hr, true, cand, 1.0, scale=20.0, workspace=ws1, out=out1), calls)
        print(json.dumps({"figure": "grad call", "B": B, "K": K, "d": DIM, "L": L, "mean_labels": round(L / B, 2),
                          "labels_grad_ms": lab, "one_vs_all_grad_ms": one, "ratio_of_medians": round(med(lab) / med(one), 4)}),
              flush=True)
        if most == 5:
            step_batch = (hr, o, p)
    tri = torch.as_tensor(np.stack([rng.integers(n_rel, N, B), rng.integers(n_rel, N, B), rng.integers(0, n_rel, B)], 1)).cuda()
    opt1 = H.SoftmaxAdaGrad(emb.clone(), cand, B, scale=20.0)
    optl = H.LabelSoftmaxAdaGrad(emb.clone(), cand, B, step_batch[2].numel(), scale=20.0)
    s1 = windows(lambda: opt1.step(tri, 0.1), calls)
    sl = windows(lambda: optl.step(step_batch, step_batch, 0.1), calls)
    print(json.dumps({"figure": "step", "rows_a_side": B, "mean_labels": round(step_batch[2].numel() / B, 2),
                      "LabelSoftmaxAdaGrad_step_ms": sl, "SoftmaxAdaGrad_step_ms": s1,
                      "ratio_of_medians": round(med(sl) / med(s1), 4)}), flush=True)


if __name__ == "__main__":
    main()
