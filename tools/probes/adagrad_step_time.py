"""Time per step of the AdaGrad loop (ge_train_steps_adagrad) and of the deterministic SGD loop (ge_train_steps with
GE_STEP_DETERMINISTIC) -- both run the gradient kernel and two update launches a step -- alternated in one process:
FB15k-shaped, d = 200, B = 4096, and B = 65,536 on the 1.2 M-row (960 MB) table.  One JSON line per timed run; the
distinct rows of the last step give the bytes the accumulator adds (one more row read and one more row write each)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from graphembeddings_amd import data as D
from graphembeddings_amd import hole as H


def timed(tr, steps):
    tr.run(steps)                                   # warm: code objects, the look-ahead records
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.run(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def distinct_rows(tr, B):
    row = (tr.row - B) % tr.triples.shape[0]
    pos = tr.triples[row:row + B]
    return int(torch.unique(torch.cat([pos.reshape(-1), tr._neg.reshape(-1)])).numel())


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    d = 200
    fb = D.fb15k_shape()
    _, id_to_type, offsets, ids = fb.type_arrays()
    small = (fb.entity_count, torch.as_tensor(D.synthetic_fb15k_triples(fb, n_triples=400000, seed=2)).cuda(),
             H.TypeTables.from_host(id_to_type, offsets, ids, padded_size=1024), 4096, 400, "fb15k")
    data, tri = D.synthetic_large(n_entities=1_200_000, n_triples=4_000_000, seed=1234, zipf_s=0.8)
    _, id_to_type, offsets, ids = D.synthetic_large_type_arrays(data)
    large = (data.entity_count, torch.as_tensor(tri).cuda(), H.TypeTables.from_host(id_to_type, offsets, ids, padded_size=1024),
             65536, 32, "synthetic 1.2M rows")
    for n_rows, dtri, tt, B, steps, name in (small, large):
        for r in range(rounds):
            for opt in ("sgd_deterministic", "adagrad"):
                emb = H.init_embeddings(n_rows, d, seed=0)
                kw = dict(optimizer="adagrad") if opt == "adagrad" else dict(deterministic=True)
                tr = H.Trainer(emb, dtri, tt, B, margin=0.2, learning_rate=0.1, decay_steps=1e5, seed=0, **kw)
                us = timed(tr, steps)
                rows = distinct_rows(tr, B)
                print(json.dumps({"workload": name, "B": B, "d": d, "loop": opt, "round": r, "us_per_step": round(us, 2),
                                  "distinct_rows_last_step": rows, "accumulator_bytes_per_step": rows * 2 * 4 * d,
                                  "mean_loss": float(tr.last_loss.mean())}), flush=True)
                tr.close()
                del tr, emb
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
