"""Nearest-neighbour search timing (ge_neighbor_topk, neighbors.nearest's routes).

    python tools/neighbors_bench.py [--calls 5] [--ks 1,10,100,128] [--metrics cosine,euclidean] [--dims 200,100]
                                    [--big | --big_only] [--no_baselines] [--out F]

FB15k all-pairs: 14,951 queries x 14,951 candidates at d = 200 and d = 100.  --big: 1.2 M candidates at d = 200 with
B = 1, 64, 1024, 16384 queries and k = 10, 128.  Each line gives, in ms (median of --calls after one warm-up, device
events around the device work only, no host copies):
  fused_ms    ge_neighbor_topk over all B rows at once, planes built beforehand (planes_ms: ge_neighbor_planes)
  stored_ms   the stored route: ge_neighbor_dists in chunks of 1024 rows + the stable (D, id) device sort
              (evaluate._topk_of_losses), as nearest() takes it for k > 128
  torch_ms    the torch route: normalised rows, an fp32 matmul, the distance expressions and the same sort
  topk_ms     what a user writes today: the same matmul and distances + torch.topk (no (D, id) tie rule)
and the executed f16-MFMA flops of the fused sweep (3 MFMAs per 16-column k block over whole 128 x 128 tiles) as
PFLOP/s and as a share of the 2.5 PFLOP/s dense f16 peak.  Prints one JSON line per configuration."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphembeddings_amd import _lib  # noqa: E402
from graphembeddings_amd import evaluate as EV  # noqa: E402
from graphembeddings_amd import neighbors as NB  # noqa: E402

PEAK_F16 = 2.5e15
CHUNK = 1024


def timed(fn, calls):
    fn()
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def mfma_flops(B, K, d):
    kkb = max(4, (d + 15) // 16)
    return 3 * 2 * (-(-B // 128) * 128) * (-(-K // 128) * 128) * 16 * kkb


def stream():
    return torch.cuda.current_stream().cuda_stream


@torch.no_grad()
def run(T, q, ks, metrics, calls, shape, baselines, out):
    N, d = T.shape
    B = len(q)
    planes = NB.NeighborPlanes(T)
    K = planes.cand.numel()
    qd = torch.as_tensor(q.astype(np.int32)).cuda()
    planes_ms = timed(lambda: _lib.call("ge_neighbor_planes", T.data_ptr(), N, d, planes.cand.data_ptr(), K,
                                        planes.buffer.data_ptr(), stream()), calls)
    norms = torch.linalg.vector_norm(T, dim=1)
    inv = torch.where(norms == 0, torch.zeros_like(norms), 1.0 / norms)
    U = T * inv[:, None]
    rows = torch.arange(B, device="cuda")
    for metric in metrics:
        m = NB.METRICS[metric]

        def torch_chunks(k, sort):
            for s in range(0, B, CHUNK):
                ql = qd[s:s + CHUNK].long()
                L = NB._distances_torch(U[ql] @ U.t(), norms[ql], norms, m)
                if sort:
                    EV._topk_of_losses(L, planes.cand64, k, (rows[:ql.numel()], ql))
                else:
                    L[rows[:ql.numel()], ql] = float("inf")
                    torch.topk(L, k, dim=1, largest=False)

        def stored(k):
            for s in range(0, B, CHUNK):
                qb = qd[s:s + CHUNK]
                L = torch.empty((qb.numel(), K), dtype=torch.float32, device="cuda")
                _lib.call("ge_neighbor_dists", T.data_ptr(), N, d, qb.data_ptr(), qb.numel(), planes.cand.data_ptr(), K,
                          m, planes.buffer.data_ptr(), L.data_ptr(), stream())
                EV._topk_of_losses(L, planes.cand64, k, (rows[:qb.numel()], qb.long()))

        for k in ks:
            ws = torch.empty(int(_lib.load().ge_neighbor_workspace_bytes(B, K, k)), dtype=torch.uint8, device="cuda")
            oid = torch.empty((B, k), dtype=torch.int32, device="cuda")
            od = torch.empty((B, k), dtype=torch.float32, device="cuda")
            fused = lambda: _lib.call("ge_neighbor_topk", T.data_ptr(), N, d, qd.data_ptr(), B, planes.cand.data_ptr(), K,
                                      k, m, 1, planes.buffer.data_ptr(), oid.data_ptr(), od.data_ptr(), ws.data_ptr(),
                                      ws.numel(), stream())
            ms = timed(fused, calls)
            fl = mfma_flops(B, K, d)
            rec = {"shape": shape, "metric": metric, "B": B, "K": K, "d": d, "k": k, "fused_ms": ms,
                   "planes_ms": planes_ms, "mfma_pflops": fl / ms / 1e12, "f16_peak_share": fl / ms / 1e12 / (PEAK_F16 / 1e15)}
            if baselines.get("stored"):
                rec["stored_ms"] = timed(lambda: stored(k), max(1, calls // 2))
            if baselines.get("torch"):
                rec["torch_ms"] = timed(lambda: torch_chunks(k, True), max(1, calls // 2))
            if baselines.get("topk"):
                rec["topk_ms"] = timed(lambda: torch_chunks(k, False), max(1, calls // 2))
            print(json.dumps(rec), flush=True)
            out.append(rec)
            del ws, oid, od
    del planes, U
    torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--calls", type=int, default=5)
    p.add_argument("--ks", default="1,10,100,128")
    p.add_argument("--metrics", default="cosine,euclidean")
    p.add_argument("--dims", default="200,100")
    p.add_argument("--big", action="store_true")
    p.add_argument("--big_only", action="store_true")
    p.add_argument("--no_baselines", action="store_true", help="the fused route only (e.g. under rocprofv3)")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    ks = [int(x) for x in a.ks.split(",")]
    metrics = a.metrics.split(",")
    out = []
    g = torch.Generator(device="cuda").manual_seed(0)
    if not a.big_only:
        for d in (int(x) for x in a.dims.split(",")):
            T = torch.randn((14951, d), generator=g, device="cuda")
            base = {} if a.no_baselines else {"stored": True, "torch": True, "topk": True}
            run(T, np.arange(14951), ks, metrics, a.calls, "fb15k_allpairs", base, out)
            del T
    if a.big or a.big_only:
        N = 1_200_000
        T = torch.randn((N, 200), generator=g, device="cuda")
        rng = np.random.default_rng(0)
        for B in (1, 64, 1024, 16384):
            q = rng.integers(0, N, B)
            base = {} if a.no_baselines else {"stored": B <= 64, "torch": B <= 64, "topk": B <= 1024}
            run(T, q, [10, 128], metrics, a.calls, f"big_B{B}", base, out)
    if a.out:
        with open(a.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in out)


if __name__ == "__main__":
    main()
