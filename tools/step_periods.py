"""Each step's kernel times against its position in the prepare chunk, at the headline shape (FB15k-shaped ComplEx, d = 200,
B = 4096): does a step that runs beside a prepare launch take longer than one that runs alone?

One native call of `--chunks` whole chunks with HIP events riding on every step's gradient-kernel dispatch, then a second
call with the events on the update kernel (no profiler attached; the method of profiles/r04_step_periods_b65536.json).
With a pipeline handle the launch for chunk c + 1 is enqueued when chunk c is entered and starts when the last step of
chunk c - 1 has finished, so the steps it runs beside are the first `--prepare-us / step` positions of every chunk.

usage: python tools/step_periods.py [--lib PATH --chunk N] [--margin M] [--no-handle] [--prepare-us US] > out.json
  --lib    another build of the library (one without ge_train_max_chunk_steps needs --chunk, its chunk length)
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphembeddings_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--chunk", type=int, default=None)
ap.add_argument("--chunks", type=int, default=6)
ap.add_argument("--margin", type=float, default=0.2)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--no-handle", action="store_true", help="prepare on the caller's stream (no pipeline handle)")
ap.add_argument("--prepare-us", type=float, default=121.0, help="how long a prepare launch lasts beside training")
args = ap.parse_args()
if args.lib:
    L.LIB_PATH = os.path.abspath(args.lib)
    import torch  # first: the library must bind to the HIP runtime PyTorch brings (see _lib.load)
    have = ctypes.CDLL(L.LIB_PATH)
    for name in [n for n in L.SYMBOLS if not hasattr(have, n)]:
        del L.SYMBOLS[name]          # an older build: everything this tool calls is older still

import torch
from graphembeddings_amd import data as D
from graphembeddings_amd import hole as H

B = args.batch
chunk = args.chunk or int(L.load().ge_train_max_chunk_steps(B, 0))
fb = D.fb15k_shape()
names, id_to_type, offsets, ids = fb.type_arrays()
tt = H.TypeTables.from_host(id_to_type, offsets, ids, padded_size=1024)
tri = torch.as_tensor(D.synthetic_fb15k_triples(fb, n_triples=483142, seed=0)).cuda()
emb = H.init_embeddings(fb.entity_count, 200, seed=0)
tr = H.Trainer(emb, tri, tt, B, margin=args.margin, learning_rate=0.1, decay_steps=32.0 * 117, seed=0,
               lookahead=not args.no_handle)
n = args.chunks * chunk
tr.run(2 * chunk)
torch.cuda.synchronize()
out = {"B": B, "d": 200, "margin": args.margin, "chunk_steps": chunk, "steps_per_call": n, "handle": not args.no_handle,
       "library": os.path.basename(L.LIB_PATH)}
ev = H.Events(2 * n)
for kern, name in ((1, "grad"), (2, "apply")):
    # with a handle the sequence never restarts here: step s of the call is step global_step + s of the sequence;
    # without one every call is a sequence of its own
    first = 0 if args.no_handle else tr.global_step
    tr.run(n, events=ev.handles, ev_kernel=kern)
    torch.cuda.synchronize()
    out[name + "_position_in_chunk"] = [(first + s) % chunk for s in range(n)]
    out[name + "_us"] = [round(1e3 * ev.elapsed_ms(2 * s, 2 * s + 1), 2) for s in range(n)]
    out[name + "_start_to_next_start_us"] = [round(1e3 * ev.elapsed_ms(2 * s, 2 * s + 2), 2) for s in range(n - 1)]
ev.close()
out["final_mean_hinge"] = float(tr.last_loss.mean())

# the stop rule's comparison: positions the prepare launch covers against the rest of the chunk
period = float(np.median(out["grad_start_to_next_start_us"]))
beside = max(1, int(np.ceil(args.prepare_us / period)))
summary = {"step_period_us_median": round(period, 2), "prepare_us_assumed": args.prepare_us, "positions_beside_prepare": beside}
for name in ("grad", "apply"):
    pos = np.array(out[name + "_position_in_chunk"])
    us = np.array(out[name + "_us"])
    a, b = us[pos < beside], us[pos >= beside]
    summary[name] = {"beside_median": round(float(np.median(a)), 2), "beside_mean": round(float(a.mean()), 2),
                     "rest_median": round(float(np.median(b)), 2), "rest_mean": round(float(b.mean()), 2),
                     "rest_p10": round(float(np.percentile(b, 10)), 2), "rest_p90": round(float(np.percentile(b, 90)), 2),
                     "rest_std": round(float(b.std()), 2), "all_mean": round(float(us.mean()), 2)}
    by_pos = [round(float(np.median(us[pos == p])), 2) for p in range(min(chunk, 2 * beside + 8))]
    summary[name]["median_by_position"] = by_pos
out["summary"] = summary
print(json.dumps(out))
