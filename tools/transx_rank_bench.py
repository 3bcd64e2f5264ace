"""Filtered link-prediction timing of the translation models at FB15k shape (E=14,951, R=1,345, d=100, a 59,071-row
test set with tools/transx_bench.py's Zipf relation column): the full two-sided filtered evaluation
(evaluate.evaluate_translation: known-cell lists, ge_transx_rank / ge_transr_rank, both sides) per model and norm,
and a chunked torch-eager GPU baseline that computes the same ranks.

    python tools/transx_rank_bench.py [--calls 5] [--models transe,transh,transd,transr] [--baseline_rows 4096] [--out F]

Each native figure is the median of --calls evaluations timed with device events.  The baseline ranks
--baseline_rows rows per side (projected candidate rows, (q - P).abs().sum(-1) or its square, in chunks, then the
(D, id) count and the known-cell count) and is scaled to the full test set.  Prints one JSON line per configuration."""
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

E, R, D, T, N_TEST = 14951, 1345, 100, 483142, 59071


def fb15k_like(seed=0):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, R + 1) ** 1.1
    r = rng.choice(R, size=T + N_TEST, p=w / w.sum())
    tri = np.unique(np.stack([rng.integers(0, E, T + N_TEST), rng.integers(0, E, T + N_TEST), r], 1), axis=0)
    rng.shuffle(tri)
    return tri[:-N_TEST], tri[-N_TEST:]


def timed(fn, calls):
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


@torch.no_grad()
def torch_ranks(m, name, test, known_set, side, chunk=64):
    """The same ranks in torch eager on the GPU: per row chunk, every candidate's projection, D, then the counts."""
    t = torch.as_tensor(test).cuda()
    ent = m.tables["ent"]
    raw = torch.empty(len(test), dtype=torch.int64, device="cuda")
    fil = torch.empty_like(raw)
    ids = torch.arange(m.n_ent, device="cuda")
    for s in range(0, len(test), chunk):
        c = t[s:s + chunk]
        h, tt, r = c[:, 0], c[:, 1], c[:, 2]
        if name == "transr":
            M = m.tables["rel_matrix"][r].view(-1, m.dim_r, m.dim_e)
            P = torch.einsum("bke,ne->bnk", M, ent)
        elif name == "transh":
            n = m.tables["normal_vector"][r]
            n = n * torch.rsqrt(torch.clamp((n * n).sum(1, keepdim=True), min=1e-12))
            P = ent[None] - (ent[None] * n[:, None]).sum(-1, keepdim=True) * n[:, None]
        elif name == "transd":
            a = (ent * m.tables["ent_transfer"]).sum(1)
            P = ent[None] + a[None, :, None] * m.tables["rel_transfer"][r][:, None]
        else:
            P = ent[None].expand(len(c), -1, -1)
        fixed, target = (h, tt) if side == "tail" else (tt, h)
        Pf = P[torch.arange(len(c), device="cuda"), fixed]
        q = Pf + m.tables["rel"][r] if side == "tail" else Pf - m.tables["rel"][r]
        u = q[:, None] - P
        Dc = u.abs().sum(-1) if m.l1 else (u * u).sum(-1)
        dt = Dc.gather(1, target[:, None])
        before = (Dc < dt) | ((Dc == dt) & (ids[None] < target[:, None]))
        key = (fixed * m.n_rel + r)[:, None] * m.n_ent + ids[None]          # (fixed, r, candidate)
        at = torch.searchsorted(known_set, key).clamp_(max=known_set.numel() - 1)
        kn = known_set[at] == key
        raw[s:s + chunk] = before.sum(1) + 1
        fil[s:s + chunk] = raw[s:s + chunk] - (before & kn).sum(1)
    return raw, fil


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--models", default="transe,transh,transd,transr")
    ap.add_argument("--baseline_rows", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    train, test = fb15k_like()
    known = np.concatenate([train, test], 0)
    dev = "cuda"
    n_rows = max(E, R)
    # the baseline's filter: sorted keys (fixed, r, other), looked up with searchsorted
    kt = torch.as_tensor(known).cuda()
    tail_set = torch.unique((kt[:, 0] * R + kt[:, 2]) * E + kt[:, 1])
    head_set = torch.unique((kt[:, 1] * R + kt[:, 2]) * E + kt[:, 0])
    lines = []
    for name in a.models.split(","):
        for l1 in (True, False):
            m = TRm.TransR(E, R, D, D, l1=l1, seed=0) if name == "transr" else X.TransX(name, E, R, D, l1=l1, seed=0)
            idx = {s: EV.KnownIndex(known, n_rows, s, dev) for s in ("tail", "head")}
            ev = lambda: [EV.translation_ranks(m, test, idx[s], side=s) for s in ("tail", "head")]
            ref = ev()
            ms = timed(ev, a.calls)
            nb = a.baseline_rows
            sub = test[np.argsort(test[:, 2], kind="stable")][:: max(1, len(test) // nb)][:nb]
            base = lambda: [torch_ranks(m, name, sub, tail_set if s == "tail" else head_set, s) for s in ("tail", "head")]
            # the baseline must agree with the native ranks on its rows (up to fp32 rounding of near-ties)
            pos = {tuple(x): i for i, x in enumerate(test.tolist())}
            rows = np.array([pos[tuple(x)] for x in sub.tolist()])
            agree = float(np.mean([np.mean(ref[k][1][rows] == b[1].cpu().numpy()) for k, b in enumerate(base())]))
            bms = timed(base, max(1, a.calls // 2)) * len(test) / len(sub)
            line = {"model": name, "l1": l1, "E": E, "R": R, "d": D, "test_rows": len(test),
                    "eval_two_sided_filtered_ms": round(ms, 3), "torch_eager_gpu_ms_scaled": round(bms, 1),
                    "speedup_vs_torch": round(bms / ms, 1), "baseline_rows_per_side": len(sub),
                    "baseline_filtered_agree": round(agree, 5),
                    "differences_two_sided": 2 * len(test) * E * D}
            print(json.dumps(line))
            sys.stdout.flush()
            lines.append(line)
            del m
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
