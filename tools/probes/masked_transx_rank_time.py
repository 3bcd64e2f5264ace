"""Event-timed entity rank sweep of the translation models with and without per-relation candidate sets, alternated in
one process, at DESIGN.md section 12's shape (the 59,071 FB15k test rows x 14,951 entities, d = 100, both norms, both
sides): the unmasked sweep, the masked sweep with CandidateSets.from_types over the packaged FB15k types (valid + test
triples), and the masked sweep with every bit set (the cost of the scan and the queue alone).  The rows are sorted by
relation, as evaluate.translation_ranks passes them; each timed call is rank_counts without known lists (preparation,
row kernel, sweep).  One JSON line per (model, norm, side).
    python tools/probes/masked_transx_rank_time.py [--lib PATH] [--runs N] [--unmasked-only] [--models a,b] [--topk K]
--lib: time another build of libge_hip.so (an older one without the masked entry points: the unmasked sweep only).
--topk K: time topk_candidates(k = K) on the same rows' (fixed entity, relation) queries in place of rank_counts; the
"mean_n_before" fields then hold the mean number of candidates returned.
--unmasked-only: the loop an older build runs, unmasked sweeps back to back: the like-for-like comparison with --lib."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from graphembeddings_amd import _lib
args = sys.argv[1:]
lib_path = args[args.index("--lib") + 1] if "--lib" in args else None
runs = int(args[args.index("--runs") + 1]) if "--runs" in args else 7
models = args[args.index("--models") + 1].split(",") if "--models" in args else ["transe", "transh", "transd", "transr"]
masked = "--unmasked-only" not in args
topk = int(args[args.index("--topk") + 1]) if "--topk" in args else 0
if lib_path:                     # (torch is imported: one HIP runtime in the process, as _lib.load arranges)
    import ctypes
    lib = ctypes.CDLL(os.path.abspath(lib_path))
    masked = masked and hasattr(lib, "ge_transx_rank_masked")
    for name, (res, a) in _lib.SYMBOLS.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, a
    _lib._lib = lib              # what _lib.load() returns from here on, whatever version it reports
from graphembeddings_amd import data as D, evaluate as E, hole as H
from graphembeddings_amd.transr import TransR
from graphembeddings_amd.transx import TransX
d = 100
inf = D.init_inference_data(D.PACKAGE_FB15K_DIR)
R = inf.relation_count
n_ent = inf.entity_count - R                                   # the ComplEx table numbers its rows relations first
shift = lambda t: np.stack([t[:, 0] - R, t[:, 1] - R, t[:, 2]], 1).astype(np.int64)
test = shift(inf.test_array)
test = test[np.argsort(test[:, 2], kind="stable")]
seen = np.concatenate([shift(inf.validation_triples), test])
types = inf.type_arrays()[1][R:]
tri = torch.as_tensor(test.astype(np.int32)).cuda()
queries = {head: torch.as_tensor(test[:, [1 if head else 0, 2]].astype(np.int32)).cuda() for head in (False, True)}
B = len(test)
sets = {}
if masked:
    for side in ("tail", "head"):
        cs = E.CandidateSets.from_types(np.arange(n_ent), types, seen, R, side)
        rs = torch.as_tensor(test[:, 2].astype(np.int32)).cuda()
        # the union of a 16-row chunk's sets: what the sweep computes a distance for
        bits = cs.mask.cpu().numpy().view(np.uint32)
        union = [int(np.unpackbits(np.bitwise_or.reduce(bits[np.unique(test[i:i + 16, 2])], 0).view(np.uint8)).sum())
                 for i in range(0, B, 16)]
        sets[side] = dict(cs=cs, rs=rs, full=torch.full_like(cs.mask, -1), mean_set=float(cs.counts[test[:, 2]].mean()),
                          mean_union=float(np.mean(union)))
def once(m, head, **kw):
    ev = H.Events(2)
    ev.record(0)
    if topk:
        nb = m.topk_candidates(queries[head], topk, cand_is_head=head, **kw)[0]
    else:
        nb, _, _ = m.rank_counts(tri, cand_is_head=head, **kw)
    ev.record(1)
    torch.cuda.synchronize()
    ms = ev.elapsed_ms(0, 1)
    ev.close()
    if topk:
        nb = (nb >= 0).sum(1)
    return ms, float(nb.float().mean())
for name in models:
    for l1 in (True, False):
        m = TransR(n_ent, R, d, d, l1=l1, seed=3) if name == "transr" else TransX(name, n_ent, R, d, l1=l1, seed=3)
        for side in ("tail", "head"):
            head = side == "head"
            variants = {"unmasked": {}}
            if masked:
                s = sets[side]
                variants["masked"] = dict(row_set=s["rs"], mask=s["cs"].mask)
                variants["masked_all_bits"] = dict(row_set=s["rs"], mask=s["full"])
            got = {v: [] for v in variants}
            for i in range(2 + runs):
                for v, kw in variants.items():                 # alternated sweep by sweep
                    t = once(m, head, **kw)
                    if i >= 2:
                        got[v].append(t)
            out = {"lib": lib_path or "this build", "model": name, "l1": l1, "side": side, "rows": B, "n_ent": n_ent, "d": d}
            if topk:
                out["topk"] = topk
            for v, ts in got.items():
                out[v + "_ms"] = [round(t, 3) for t, _ in ts]
                out[v + "_median_ms"] = round(float(np.median([t for t, _ in ts])), 3)
                out[v + "_mean_n_before"] = ts[0][1]
            if masked:
                out.update(mean_set_size=sets[side]["mean_set"], mean_chunk_union=sets[side]["mean_union"])
            print(json.dumps(out), flush=True)
