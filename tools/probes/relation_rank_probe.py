"""Relation-prediction timing of the translation models at FB15k shape (59,071 rows, E = 14,951, d = 100) against
R = 1,345 relations (FB15k) and R = 18 (WN18): per model and norm the native call (ge_transx_relation_rank /
ge_transr_relation_rank, unfiltered), the whole filtered host path (evaluate.translation_relation_ranks: known-cell
lists + the call) and a chunked torch-eager GPU baseline that computes the same [rows, R] distances.

    python tools/probes/relation_rank_probe.py [--calls 5] [--models transe,transh,transd,transr] [--rels 1345,18]
                                               [--rows 59071] [--baseline_rows 4096] [--transr_rows N]
                                               [--no_baseline] [--no_path] [--out F]

Each native figure is the median of --calls runs timed with device events, after one warm-up run (the filtered path
runs after the call and is not warmed again).  The baseline runs --baseline_rows rows and is scaled to the rows of the
line.  --transr_rows runs TransR on the first N rows only (its work is rows x R x dim_r x dim_e; every line states its
own rows).  `cell_k` is the work the algorithm needs from shapes: rows x R x d
(TransE / TransH / TransD: one difference-and-accumulate per cell and component; TransH twice, its dot first) or
rows x R x dim_r x dim_e fmaf (TransR); `floor_ms` is cell_k over the fp32 vector rate (78.6e12 lane-operations/s =
157.3 TFLOPS of fmaf), times the operations one cell_k costs (TransE 2: add, |.|-accumulate or fmaf; TransD 3;
TransH 2 + 3; TransR 1).  Prints one JSON line per configuration."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from graphembeddings_amd import evaluate as EV  # noqa: E402
from graphembeddings_amd import transr as TRm  # noqa: E402
from graphembeddings_amd import transx as X  # noqa: E402

E, D, T = 14951, 100, 483142
VALU_RATE = 78.6e12                    # fp32 lane-operations per second (256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz)
OPS_PER_CELL_K = {"transe": 2, "transd": 3, "transh": 5, "transr": 1}


def triples(R, n_test, seed=0):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, R + 1) ** 1.1
    n = T + n_test
    tri = np.unique(np.stack([rng.integers(0, E, n), rng.integers(0, E, n), rng.choice(R, size=n, p=w / w.sum())], 1), axis=0)
    rng.shuffle(tri)
    return tri[:-n_test], tri[-n_test:]


def timed(fn, calls, warm=True):
    if warm:
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


@torch.no_grad()
def torch_distances(m, name, t, chunk):
    """The same [rows, R] distances in torch eager on the GPU, per row chunk; returns the last chunk (kept alive)."""
    ent, rel = m.tables["ent"], m.tables["rel"]
    out = None
    for s in range(0, len(t), chunk):
        c = t[s:s + chunk]
        w = ent[c[:, 0]] - ent[c[:, 1]]
        if name == "transr":
            u = (w @ m.tables["rel_matrix"].view(-1, m.dim_e).T).view(len(c), m.n_rel, m.dim_r) + rel[None]
        elif name == "transh":
            n = m.tables["normal_vector"]
            n = n * torch.rsqrt(torch.clamp((n * n).sum(1, keepdim=True), min=1e-12))
            u = w[:, None] - (w @ n.T)[:, :, None] * n[None] + rel[None]
        elif name == "transd":
            s_ = (ent[c[:, 0]] * m.tables["ent_transfer"][c[:, 0]]).sum(1) - (ent[c[:, 1]] * m.tables["ent_transfer"][c[:, 1]]).sum(1)
            u = w[:, None] + s_[:, None, None] * m.tables["rel_transfer"][None] + rel[None]
        else:
            u = w[:, None] + rel[None]
        out = u.abs().sum(-1) if m.l1 else (u * u).sum(-1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--models", default="transe,transh,transd,transr")
    ap.add_argument("--rels", default="1345,18")
    ap.add_argument("--rows", type=int, default=59071)
    ap.add_argument("--baseline_rows", type=int, default=4096)
    ap.add_argument("--transr_rows", type=int, default=None)
    ap.add_argument("--no_baseline", action="store_true")
    ap.add_argument("--no_path", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("relation_rank_probe needs an MI355X: there is no CPU path")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    for R in (int(x) for x in a.rels.split(",")):
        train, test = triples(R, a.rows)
        known = np.concatenate([train, test], 0)
        tg_all = torch.as_tensor(test).cuda()
        test_all = test
        index = EV.KnownIndex(known, max(E, R), "relation", "cuda")
        for name in a.models.split(","):
            for l1 in (True, False):
                m = TRm.TransR(E, R, D, D, l1=l1, seed=0) if name == "transr" else X.TransX(name, E, R, D, l1=l1, seed=0)
                n = a.transr_rows if name == "transr" and a.transr_rows else len(test_all)
                test, tg = test_all[:n], tg_all[:n]
                call_ms, lo, hi = timed(lambda: m.relation_rank_counts(tg), a.calls)
                cell_k = len(test) * R * D * (D if name == "transr" else 1)
                floor = cell_k * OPS_PER_CELL_K[name] / VALU_RATE * 1e3
                line = {"model": name, "l1": l1, "rows": len(test), "E": E, "R": R, "d": D, "calls": a.calls,
                        "native_call_ms": round(call_ms, 3), "native_call_ms_min_max": [round(lo, 3), round(hi, 3)],
                        "cell_k": cell_k, "floor_ms": round(floor, 3), "call_over_floor": round(call_ms / floor, 2)}
                if not a.no_path:
                    path_ms, _, _ = timed(lambda: EV.translation_relation_ranks(m, test, index), a.calls, warm=False)
                    line["filtered_ranks_ms"] = round(path_ms, 3)
                if not a.no_baseline:
                    nb = min(a.baseline_rows, len(test))
                    chunk = 256 if name == "transr" else max(16, min(nb, (1 << 26) // (R * D)))
                    sub = tg[:nb]
                    # the baseline computes the kernel's distances (up to fp32 rounding)
                    ref = m.relation_rank_counts(sub[:chunk], return_scores=True)[-1]
                    got = torch_distances(m, name, sub[:chunk], chunk)
                    line["baseline_max_rel_diff"] = float(((ref - got).abs() / ref.abs().clamp_min(1e-6)).max())
                    bms, _, _ = timed(lambda: torch_distances(m, name, sub, chunk), max(1, a.calls // 2))
                    line["torch_eager_gpu_ms_scaled"] = round(bms * len(test) / nb, 1)
                    line["baseline_rows"] = nb
                    line["speedup_vs_torch"] = round(bms * len(test) / nb / call_ms, 1)
                print(json.dumps(line))
                sys.stdout.flush()
                if a.out:                                  # line by line: a run that is cut short keeps what it has
                    with open(a.out, "a") as f:
                        f.write(json.dumps(line) + "\n")
                del m
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
