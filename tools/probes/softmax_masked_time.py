"""Time per call of the type-constrained 1-vs-all softmax next to the unmasked one, in one process, between device
events, at (B, K, d) = (4096, 14951, 200) on a 16,296-row table (norms on both sides of the clip); the batch is 4,096 rows
of data.synthetic_fb15k_triples.  3 warm-up calls, then three windows of `calls` calls, ge_softmax_grad of the same build
alternated with every figure.  One JSON line per figure:
  1. every bit set (one set): ge_softmax_masked_grad against ge_softmax_grad;
  2. the type sets of FB15k (CandidateSets.from_types, fb15k_shape().type_arrays()), both sides, in four cells:
     candidates in id order / ordered by (type code, id), x rows as drawn / sorted by set id -- ms and the share of live
     (query tile, candidate tile) pairs.  Once with sets and batch from the synthetic triples (heads and tails drawn
     without regard to types: nearly every type is seen with every relation), once from the real valid + test triples
     shipped with the package;
  3. SoftmaxAdaGrad.step with the sets (candidates ordered by type; the step sorts the rows itself) against the step
     without them."""
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from graphembeddings_amd import data as D
from graphembeddings_amd import evaluate as E
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


def live_share(mask, rs, K):
    """Share of (64-row, 64-candidate) tile pairs in which some row admits some candidate."""
    tk = (K + 63) // 64
    m = mask[rs.long()][:, :2 * tk].reshape(B // 64, 64, tk, 2)
    return float((m != 0).any(3).any(1).float().mean())


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    fb = D.fb15k_shape()
    R, N = fb.relation_count, fb.entity_count
    K = N - R
    tri_all = D.synthetic_fb15k_triples(fb)
    codes = np.asarray(fb.type_arrays()[1])
    rows = np.random.default_rng(1).choice(len(tri_all), B, replace=False)
    tri = torch.as_tensor(tri_all[rows].astype(np.int32)).cuda()
    emb = table(N)
    ids = np.arange(R, N, dtype=np.int32)
    by_type = ids[np.lexsort((ids, codes[ids]))]
    gi, gv = torch.empty(K + 2 * B, dtype=torch.int32, device="cuda"), torch.empty(K + 2 * B, DIM, device="cuda")
    ws, wsm = H.softmax_workspace(emb, B, K), H.softmax_masked_workspace(emb, B, K)

    def plain(cand, t, side):
        fx, tr = (0, 1) if side == "tail" else (1, 0)
        hr, true = t[:, [fx, 2]].contiguous(), t[:, tr].contiguous()
        return lambda: H.softmax_grad(emb, hr, true, cand, 1.0, scale=20.0, side=side, workspace=ws, out=(gi, gv))

    def masked(cand, t, side, cs, rs):
        fx, tr = (0, 1) if side == "tail" else (1, 0)
        hr, true = t[:, [fx, 2]].contiguous(), t[:, tr].contiguous()
        # the host checks of hole.softmax_grad synchronise once a call; the entry point is timed through them, as a user's
        # call is
        return lambda: H.softmax_grad(emb, hr, true, cand, 1.0, scale=20.0, side=side, workspace=wsm, out=(gi, gv),
                                      candidate_sets=cs, row_sets=rs)

    cand = torch.as_tensor(ids).cuda()
    ones = types.SimpleNamespace(mask=torch.full((1, H.candidate_mask_words(K)), -1, dtype=torch.int32, device="cuda"),
                                 n_sets=1, cand=cand)
    zero = torch.zeros(B, dtype=torch.int32, device="cuda")
    a = windows(masked(cand, tri, "tail", ones, zero), calls)
    b = windows(plain(cand, tri, "tail"), calls)
    print(json.dumps({"figure": "all bits set", "B": B, "K": K, "d": DIM, "masked_grad_ms": a, "unmasked_grad_ms": b,
                      "ratio_of_medians": round(sorted(a)[1] / sorted(b)[1], 4)}), flush=True)

    inf = D.init_inference_data(D.PACKAGE_FB15K_DIR)
    real_all = np.concatenate([inf.validation_triples, inf.test_array]).astype(np.int64)
    real = torch.as_tensor(real_all[np.random.default_rng(2).choice(len(real_all), B, replace=False)].astype(np.int32)).cuda()
    best = None
    for source, src_all, src in (("synthetic triples", tri_all, tri), ("real valid + test triples", real_all, real)):
        order = torch.argsort(src[:, 2].long(), stable=True)
        for cname, cnp in (("id order", ids), ("by type", by_type)):
            cand = torch.as_tensor(cnp).cuda()
            sets = {s: E.CandidateSets.from_types(cnp, codes, src_all, R, s) for s in ("tail", "head")}
            for rname, t in (("as drawn", src), ("sorted by set", src[order].contiguous())):
                rs = t[:, 2].contiguous()
                line = {"figure": "FB15k type sets", "source": source, "candidates": cname, "rows": rname,
                        "mean_set_size": {s: round(float(sets[s].counts[t[:, 2].cpu().numpy()].mean()), 1) for s in sets}}
                for s in ("tail", "head"):
                    line[s + "_live_share"] = round(live_share(sets[s].mask, rs, K), 4)
                    line[s + "_masked_grad_ms"] = windows(masked(cand, t, s, sets[s], rs), calls)
                    line[s + "_unmasked_grad_ms"] = windows(plain(cand, t, s), calls)
                print(json.dumps(line), flush=True)
                tot = sorted(line["tail_masked_grad_ms"])[1] + sorted(line["head_masked_grad_ms"])[1]
                if best is None or tot < best[0]:
                    best = (tot, cname, cnp, sets, source, src)

    _, cname, cnp, sets, source, tri = best
    cand = torch.as_tensor(cnp).cuda()
    full = H.SoftmaxAdaGrad(table(N), cand, B, scale=20.0)
    typed = H.SoftmaxAdaGrad(table(N), cand, B, scale=20.0, candidate_sets=sets)
    a = windows(lambda: typed.step(tri, 0.1), calls)
    b = windows(lambda: full.step(tri, 0.1), calls)
    print(json.dumps({"figure": "SoftmaxAdaGrad.step", "source": source, "candidates": cname, "rows": "as drawn (the step sorts them)",
                      "masked_step_ms": a, "unmasked_step_ms": b}), flush=True)


if __name__ == "__main__":
    main()
