"""Time per rank validation tick (evaluate.RankPocket.tick = ge_rank_validation_tick) next to SoftmaxAdaGrad.step, in one
process, between device events, on a 16,296-row table (norms on both sides of the clip), d = 200, K = 14,951: V = 50,000
random validation triples filtered by 483,142 random known triples, unmasked and with observed candidate sets; the step at
(B, K, d) = (4096, 14951, 200).  3 warm-up calls, then three windows of `calls` calls.  One JSON line per figure.  Every
tick after the first ties with it (the table does not change), so the pocket copies are timed apart, on a fresh pocket
whose every tick improves (best reset before each)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from graphembeddings_amd import data as D
from graphembeddings_amd import evaluate as EV
from graphembeddings_amd import hole as H

DIM, B, V, KNOWN = 200, 4096, 50000, 483142


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


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    fb = D.fb15k_shape()
    n_rel, N = fb.relation_count, fb.entity_count
    K = N - n_rel
    rng = np.random.default_rng(0)
    tri = lambda n: np.stack([rng.integers(n_rel, N, n), rng.integers(n_rel, N, n), rng.integers(0, n_rel, n)], 1).astype(np.int64)
    known, valid = tri(KNOWN), tri(V)
    known = np.concatenate([known, valid])
    emb = table(N)
    acc = torch.full_like(emb, 0.1)
    cand = np.arange(n_rel, N, dtype=np.int32)
    sets = {side: EV.CandidateSets.from_observed(cand, known, n_rel, side) for side in ("tail", "head")}
    for name, cs in (("unmasked", None), ("observed sets", sets)):
        vp = EV.RankPocket(emb, valid, cand, known, accumulator=acc, candidate_sets=cs, capacity=64)

        def tick():
            vp.tick(0)
            if len(vp._steps) >= 60:
                vp._steps = []                   # (the history rows are overwritten: no read, no synchronisation)

        def improving_tick():
            vp.best.zero_()
            tick()
        tie, imp = windows(tick, calls), windows(improving_tick, calls)
        m = dict(zip(vp.KEYS, vp.hist[0].cpu().tolist()))
        print(json.dumps({"figure": "tick", "form": name, "V": V, "K": K, "d": DIM, "known": len(known),
                          "tick_ms": tie, "tick_with_pocket_copies_ms": imp, "counted": m["counted"],
                          "mean_set_size": None if cs is None else round(float(cs["tail"].counts[valid[:, 2]].mean()), 1)}), flush=True)
    batch = torch.as_tensor(tri(B)).cuda()
    opt = H.SoftmaxAdaGrad(emb.clone(), torch.as_tensor(cand).cuda(), B, scale=20.0)
    print(json.dumps({"figure": "step", "B": B, "K": K, "d": DIM, "SoftmaxAdaGrad_step_ms": windows(lambda: opt.step(batch, 0.1), calls)}),
          flush=True)


if __name__ == "__main__":
    main()
