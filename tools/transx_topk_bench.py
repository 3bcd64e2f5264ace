"""Top-k prediction timing of the translation models (ge_transx_topk / ge_transr_topk through predict_translation).

    python tools/transx_topk_bench.py [--calls 5] [--models transe,transh,transd,transr] [--ks 1,10,100,128] [--big]
                                      [--out F]

FB15k shape: E = 14,951, R = 1,345, d = 100, L1, 59,071 query rows (a Zipf relation column), filtered by about 4
random known cells per row, tails and heads.  --big adds TransE d = 100 against E = 1.2 M with B = 1, 64, 1024 rows,
raw.  Each line gives, in ms (median of --calls after one warm-up, device events around the whole call): `fused_ms`
(the selection inside the sweep), `rank_ms` (the rank sweep on the same rows, ranks()) and `unfused_ms` (the rank
sweep's stored distances + a stable device sort in 1024-row chunks: predict(fused=False)).
Prints one JSON line per configuration."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphembeddings_amd import evaluate as EV  # noqa: E402
from graphembeddings_amd import transr as TRm  # noqa: E402
from graphembeddings_amd import transx as X  # noqa: E402

E, R, D, N = 14951, 1345, 100, 59071


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


def make(name, n_ent, n_rel):
    return TRm.TransR(n_ent, n_rel, D, D) if name == "transr" else X.TransX(name, n_ent, n_rel, D)


@torch.no_grad()
def run_shape(m, name, q, known, ks, calls, out, shape, unfused=True):
    n_rows = max(m.n_ent, m.n_rel)
    for side in ("tail", "head"):
        idx = EV.KnownIndex(known, n_rows, side, "cuda") if known is not None else None
        zero = np.zeros(len(q), dtype=np.int64)
        tri = np.stack([zero, q[:, 0], q[:, 1]] if side == "head" else [q[:, 0], zero, q[:, 1]], 1)
        rank_ms = timed(lambda: m.ranks(tri, idx, side=side), calls)
        for k in ks:
            rec = {"shape": shape, "model": name, "side": side, "rows": int(len(q)), "n_ent": m.n_ent, "k": k,
                   "filtered": known is not None,
                   "fused_ms": timed(lambda: m.predict(q, k, known=idx, side=side), calls), "rank_ms": rank_ms}
            if unfused:
                rec["unfused_ms"] = timed(lambda: m.predict(q, k, known=idx, side=side, fused=False), max(1, calls // 2))
            print(json.dumps(rec), flush=True)
            out.append(rec)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--calls", type=int, default=5)
    p.add_argument("--models", default="transe,transh,transd,transr")
    p.add_argument("--ks", default="1,10,100,128")
    p.add_argument("--big", action="store_true")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    ks = [int(x) for x in a.ks.split(",")]
    rng = np.random.default_rng(0)
    w = 1.0 / np.arange(1, R + 1) ** 1.1
    q = np.stack([rng.integers(0, E, N), rng.choice(R, size=N, p=w / w.sum())], 1)
    known = np.concatenate([np.stack([q[:, 0], rng.integers(0, E, N), q[:, 1]], 1) for _ in range(4)])
    known = np.concatenate([known, known[:, [1, 0, 2]]])       # about 4 known cells per row on either side
    out = []
    for name in a.models.split(","):
        run_shape(make(name, E, R), name, q, known, ks, a.calls, out, "fb15k")
        torch.cuda.empty_cache()
    if a.big:
        m = make("transe", 1_200_000, 16)
        for B in (1, 64, 1024):
            qb = np.stack([rng.integers(0, 1_200_000, B), rng.integers(0, 16, B)], 1)
            run_shape(m, "transe", qb, None, ks, a.calls, out, f"big_B{B}", unfused=B <= 64)
    if a.out:
        with open(a.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in out)


if __name__ == "__main__":
    main()
