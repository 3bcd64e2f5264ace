"""Top-k prediction (ge_topk_1vK_planes) against the unfused route (score_candidates + torch.topk in row chunks), and
the rank sweep at the same shape.  One JSON line per measurement; median of 5 after 2 warm-up calls, device events.

  python tools/topk_bench.py [--out profiles/r08_topk_bench.jsonl] [--quick]

Shapes: the FB15k test set (59,071 rows x 14,951 candidates, d = 200, filtered by 4 random known cells per row) at
k = 1, 10, 100, 128, tails and heads; B = 1, 64, 1024 against 1.2 M candidates (raw).  The fused share of the f16 MFMA
peak counts the flops the sweep executes (3 f16 MFMAs per 16-wide k block), as bench.py's rank_sweep_mfma_roofline."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphembeddings_amd import evaluate as E  # noqa: E402
from graphembeddings_amd import hole as H  # noqa: E402

PEAK_F16_TFLOPS = 2500.0      # dense f16 MFMA, MI355X


def timed(fn, iters=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def unfused(emb, hr, cand, k, side, chunk):
    """score_candidates + torch.topk per chunk of rows (no filter, no id tie-break: a lower bound on the unfused cost)."""
    for s in range(0, hr.shape[0], chunk):
        sc = H.score_candidates(emb, hr[s:s + chunk], cand, cand_is_head=(side == "head"))
        torch.topk(sc, k, dim=1, largest=False, sorted=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="FB15k shape at k = 10 only")
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    d = 200
    R, N, B = 1345, 1345 + 14951, 59071
    g = torch.Generator(device="cpu").manual_seed(3)
    emb = H.init_embeddings(N, d, seed=3) * 4.0
    cand = torch.arange(R, N, dtype=torch.int32).cuda()
    K = cand.numel()
    hr = torch.stack([torch.randint(R, N, (B,), generator=g), torch.randint(0, R, (B,), generator=g)], 1).int().cuda()
    tid = torch.randint(R, N, (B,), generator=g).int().cuda()
    planes = H.RankPlanes(emb, cand)
    kpad = 16 * ((d + 15) // 16)
    flops = 3 * 2.0 * B * K * kpad
    rng = np.random.default_rng(0)
    hr_np = hr.cpu().numpy().astype(np.int64)
    pos_of = torch.full((N,), -1, dtype=torch.int64, device="cuda")
    pos_of[cand.to(torch.int64)] = torch.arange(K, device="cuda")
    for side in ("tail", "head"):
        known = np.stack([np.repeat(hr_np[:, 0], 4), rng.integers(R, N, 4 * B), np.repeat(hr_np[:, 1], 4)], 1)
        if side == "head":
            known = known[:, [1, 0, 2]]
        off, rc = E.KnownIndex(known, N, side, emb.device).cells(hr[:, 0].long(), hr[:, 1].long(), pos_of, K)
        ms = timed(lambda: H.rank_candidates(emb, hr, tid, cand, known_off=off, known_rc=rc, cand_is_head=(side == "head"),
                                             planes=planes))
        emit({"what": "rank sweep (ranks, filtered)", "side": side, "B": B, "K": K, "d": d, "ms": ms,
              "mfma_share": flops / (ms * 1e-3) / 1e12 / PEAK_F16_TFLOPS})
        for k in ((10,) if args.quick else (1, 10, 100, 128)):
            ms = timed(lambda: H.topk_candidates(emb, hr, cand, k, known_off=off, known_rc=rc, cand_is_head=(side == "head"),
                                                 planes=planes))
            ws = int(H._lib.load().ge_topk_workspace_bytes(B, K, k))
            emit({"what": "top-k fused (filtered)", "side": side, "B": B, "K": K, "d": d, "k": k, "ms": ms,
                  "mfma_share": flops / (ms * 1e-3) / 1e12 / PEAK_F16_TFLOPS, "workspace_MB": ws / 1e6,
                  "score_matrix_MB": B * K * 4 / 1e6})
            ms_u = timed(lambda: unfused(emb, hr, cand, k, side, 4096), iters=3, warm=1)
            emit({"what": "top-k unfused (score_candidates + torch.topk, 4096-row chunks, raw)", "side": side, "B": B,
                  "K": K, "d": d, "k": k, "ms": ms_u, "fused_speedup": ms_u / ms})
    if args.quick:
        return
    Nb = 1_200_000
    big = (torch.randn(Nb, d, device="cuda", generator=torch.Generator("cuda").manual_seed(5)) * 0.1).contiguous()
    cb = torch.arange(8, Nb, dtype=torch.int32, device="cuda")
    pb = H.RankPlanes(big, cb)
    for Bs in (1, 64, 1024):
        hq = torch.stack([torch.randint(8, Nb, (Bs,), generator=g), torch.randint(0, 8, (Bs,), generator=g)], 1).int().cuda()
        for k in (10, 128):
            ms = timed(lambda: H.topk_candidates(big, hq, cb, k, planes=pb))
            ms_u = timed(lambda: unfused(big, hq, cb, k, "tail", 256), iters=3, warm=1)
            emit({"what": "top-k small batch, raw", "B": Bs, "K": int(cb.numel()), "d": d, "k": k, "fused_ms": ms,
                  "unfused_ms": ms_u, "fused_speedup": ms_u / ms,
                  "mfma_share": 3 * 2.0 * 128 * ((Bs + 127) // 128) * cb.numel() * kpad / (ms * 1e-3) / 1e12 / PEAK_F16_TFLOPS})
    if out:
        out.close()


if __name__ == "__main__":
    main()
