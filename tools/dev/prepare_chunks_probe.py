"""One measurement of tools/dev/ab_prepare_chunks.sh: the headline step (FB15k-shaped ComplEx, d = 200, B = 4096) with the
library GE_LIB names (default: the product one), at GE_MARGIN (0.2), with a pipeline handle unless GE_NO_HANDLE=1.
Prints {"us_per_step": median of 5 x 400 steps after 200 warm-up steps, "reps": the five, ...}."""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from graphembeddings_amd import _lib as L

if os.environ.get("GE_LIB"):
    L.LIB_PATH = os.path.abspath(os.environ["GE_LIB"])
    import torch  # first: the library must bind to the HIP runtime PyTorch brings (see _lib.load)
    have = ctypes.CDLL(L.LIB_PATH)
    for name in [n for n in L.SYMBOLS if not hasattr(have, n)]:
        del L.SYMBOLS[name]          # an older build: everything this probe calls is older still
import numpy as np
import torch
from graphembeddings_amd import data as D, hole as H

margin = float(os.environ.get("GE_MARGIN", "0.2"))
fb = D.fb15k_shape()
names, id_to_type, offsets, ids = fb.type_arrays()
tt = H.TypeTables.from_host(id_to_type, offsets, ids, padded_size=1024)
tri = torch.as_tensor(D.synthetic_fb15k_triples(fb, n_triples=483142, seed=0)).cuda()
emb = H.init_embeddings(fb.entity_count, 200, seed=0)
tr = H.Trainer(emb, tri, tt, 4096, margin=margin, learning_rate=0.1, decay_steps=32.0 * 117, seed=0,
               lookahead=os.environ.get("GE_NO_HANDLE") != "1")
tr.run(200)
torch.cuda.synchronize()
res = []
for rep in range(5):
    t0 = time.perf_counter()
    tr.run(400)
    torch.cuda.synchronize()
    res.append((time.perf_counter() - t0) / 400 * 1e6)
out = {"us_per_step": round(float(np.median(res)), 3), "reps": [round(r, 3) for r in res], "margin": margin,
       "handle": tr._pipe is not None}
for k, name in ((1, "grad_us"), (2, "apply_us")):
    ev = H.Events(2 * 256)
    tr.run(256, events=ev.handles, ev_kernel=k)
    torch.cuda.synchronize()
    t = [1e3 * ev.elapsed_ms(2 * i, 2 * i + 1) for i in range(256)]
    out[name] = {"mean": round(float(np.mean(t)), 2), "median": round(float(np.median(t)), 2), "min": round(min(t), 2)}
    ev.close()
out["loss"] = float(tr.last_loss.mean())
out["table_sum"] = float(tr.embeddings.double().sum())
print(json.dumps(out))
