"""Time per call of the sampled softmax objective next to the 1-vs-all one, in one process, between device events:
ge_softmax_sampled_grad and SampledSoftmaxAdaGrad.step at (B, K', d) = (4096, K', 200) for K' in 256, 1024, 4096, 14951
on a 16,296-row table (norms on both sides of the clip), each alternated with SoftmaxAdaGrad.step over all 14,951 entity
rows; then one row at K' = 4096 on a 1.2 M-row table.  3 warm-up calls, then three windows of `calls` calls.  One JSON
line per figure."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from graphembeddings_amd import hole as H

D, B, N_REL, N_ENT = 200, 4096, 1345, 14951


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
    t = torch.randn(n_rows, D, device="cuda", generator=g)
    norms = torch.exp(0.5 * torch.randn(n_rows, 1, device="cuda", generator=g))
    return (t * (norms / t.norm(dim=1, keepdim=True))).contiguous()


def batch(n_rows, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ent = lambda: torch.randint(N_REL, n_rows, (B,), device="cuda", generator=g)
    return torch.stack([ent(), ent(), torch.randint(0, N_REL, (B,), device="cuda", generator=g)], 1).to(torch.int32)


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    n_rows = N_REL + N_ENT
    tri = batch(n_rows, 1)
    full = H.SoftmaxAdaGrad(table(n_rows), torch.arange(N_REL, n_rows, dtype=torch.int32, device="cuda"), B, scale=20.0)
    g = torch.Generator(device="cuda").manual_seed(7)
    for K in (256, 1024, 4096, 14951):
        cand = torch.randint(N_REL, n_rows, (K,), device="cuda", generator=g).to(torch.int32)
        emb = table(n_rows)
        ws = H.softmax_sampled_workspace(emb, B, K)
        hr, true = tri[:, [0, 2]].contiguous(), tri[:, 1].contiguous()
        out = (torch.empty(K + 3 * B, dtype=torch.int32, device="cuda"), torch.empty(K + 3 * B, D, device="cuda"))
        grad = windows(lambda: H.softmax_sampled_grad(emb, hr, true, cand, 1.0, scale=20.0, workspace=ws, out=out), calls)
        loss = windows(lambda: H.softmax_sampled_loss(emb, hr, true, cand, scale=20.0, workspace=ws), calls)
        opt = H.SampledSoftmaxAdaGrad(emb, B, K, scale=20.0)
        step = windows(lambda: opt.step(tri, cand, 0.1), calls)
        full_step = windows(lambda: full.step(tri, 0.1), max(calls // 3, 5))
        print(json.dumps({"table_rows": n_rows, "B": B, "K": K, "d": D, "workspace_MiB": round(ws.numel() / 2**20, 1),
                          "sampled_loss_ms": loss, "sampled_grad_ms": grad, "sampled_step_ms": step,
                          "full_softmax_step_ms_same_process": full_step}), flush=True)
    del full
    torch.cuda.empty_cache()
    big = 1_200_000
    emb, tri, K = table(big), batch(big, 2), 4096
    cand = torch.randint(N_REL, big, (K,), device="cuda", generator=g).to(torch.int32)
    opt = H.SampledSoftmaxAdaGrad(emb, B, K, scale=20.0)
    ws = H.softmax_sampled_workspace(emb, B, K)
    hr, true = tri[:, [0, 2]].contiguous(), tri[:, 1].contiguous()
    grad = windows(lambda: H.softmax_sampled_grad(emb, hr, true, cand, 1.0, scale=20.0, workspace=ws), calls)
    step = windows(lambda: opt.step(tri, cand, 0.1), calls)
    print(json.dumps({"table_rows": big, "B": B, "K": K, "d": D, "sampled_grad_ms": grad, "sampled_step_ms": step}), flush=True)


if __name__ == "__main__":
    main()
