"""Event-timed rank sweep with and without per-relation candidate sets, alternated in one process, at bench.py's
rank_sweep shape and table (59,071 rows x 14,951 candidates, d = 200, planes built once); the sets are
CandidateSets.from_types over the packaged FB15k types and valid + test triples.  One JSON line.
    python tools/probes/masked_rank_time.py [--lib PATH] [--runs N] [--unmasked-only]
--lib: time another build of libge_hip.so (an older one without the masked entry points: the unmasked sweep only).
--unmasked-only: the loop an older build runs, unmasked sweeps back to back: the like-for-like comparison with --lib."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from graphembeddings_amd import _lib
args = sys.argv[1:]
lib_path = args[args.index("--lib") + 1] if "--lib" in args else None
runs = int(args[args.index("--runs") + 1]) if "--runs" in args else 7
masked = "--unmasked-only" not in args
if lib_path:                     # (torch is imported: one HIP runtime in the process, as _lib.load arranges)
    import ctypes
    lib = ctypes.CDLL(os.path.abspath(lib_path))
    masked = masked and hasattr(lib, "ge_rank_1vK_masked")
    for name, (res, a) in _lib.SYMBOLS.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, a
    _lib._lib = lib              # what _lib.load() returns from here on, whatever version it reports
from graphembeddings_amd import data as D, evaluate as E, hole as H
d, n_rows, n_entities, n_relations = 200, 59_071, 16_296, 1_345
g = torch.Generator(device="cpu").manual_seed(3)
emb = H.init_embeddings(n_entities, d, seed=3) * 4.0
cand = torch.arange(n_relations, n_entities, dtype=torch.int32).cuda()
hr = torch.stack([torch.randint(n_relations, n_entities, (n_rows,), generator=g),
                  torch.randint(0, n_relations, (n_rows,), generator=g)], 1).int().cuda()
tid = torch.randint(n_relations, n_entities, (n_rows,), generator=g).int().cuda()
planes = H.RankPlanes(emb, cand)
cs = None
if masked:
    inf = D.init_inference_data(D.PACKAGE_FB15K_DIR)
    tri = np.concatenate([inf.validation_triples, inf.test_array])
    cs = E.CandidateSets.from_types(cand, inf.type_arrays()[1], tri, n_relations, "tail")
def once(sets):
    ev = H.Events(2)
    ev.record(0)
    nb, _ = H.rank_candidates(emb, hr, tid, cand, planes=planes, **({"candidate_sets": sets} if sets is not None else {}))
    ev.record(1)
    torch.cuda.synchronize()
    ms = ev.elapsed_ms(0, 1)
    ev.close()
    return ms, float(nb.float().mean())
for _ in range(2):
    once(None)
    if masked:
        once(cs)
un, ma = [], []
for _ in range(runs):
    un.append(once(None))
    if masked:
        ma.append(once(cs))
out = {"lib": lib_path or "this build", "unmasked_ms": [round(t, 3) for t, _ in un], "unmasked_median_ms": float(np.median([t for t, _ in un])),
       "unmasked_mean_n_before": un[0][1]}
if masked:
    out.update(masked_ms=[round(t, 3) for t, _ in ma], masked_median_ms=float(np.median([t for t, _ in ma])),
               masked_mean_n_before=ma[0][1], mean_set_size=float(cs.counts[hr[:, 1].cpu().numpy()].mean()),
               n_candidates=int(cand.numel()))
print(json.dumps(out))
