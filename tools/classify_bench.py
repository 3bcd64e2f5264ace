"""Triple-classification timing (ge_threshold_fit, ge_threshold_classify) beside the same fit written with torch ops.

    python tools/classify_bench.py [--calls 20] [--out F]

Two shapes: `fb15k_valid` (100,000 labelled triples over 1,345 relations, Zipf-distributed) and `hot_relation` (4 M
triples over 16 relations, one relation holding half of them).  Each JSON line gives, in ms (median of --calls after
one warm-up, device events around the device work only, the two versions of a stage timed alternately):
  sort_ms            the host layer's plumbing, shared by both fits: the 64-bit key, torch.sort and three gathers
  fit_ms             ge_threshold_fit on the sorted input (memset + four kernels)
  torch_fit_ms       the same fit with torch ops on the sorted input: two cumsums, the admissible mask, searchsorted for
                     the segment ends, scatter_reduce(amax) of a packed int64 key, gathers -- checked equal to fit_ms's
  classify_ms        ge_threshold_classify with labels and confusion counts
  torch_classify_ms  score <= thr[seg] and a bincount of 4 * seg + class
and the bytes the fit's kernels read per element (9 B in `cuts`, 5 B in `count`) over fit_ms as GB/s."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphembeddings_amd import _lib  # noqa: E402
from graphembeddings_amd import classify as CL  # noqa: E402


def timed_pair(fa, fb, calls):
    """Median ms of fa and fb, called alternately."""
    fa(), fb()
    ta, tb = [], []
    for _ in range(calls):
        for fn, ts in ((fa, ta), (fb, tb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
    return float(np.median(ta)), float(np.median(tb))


def torch_fit(score, seg, label, n_seg):
    """ge_threshold_fit's five outputs with torch ops, on sorted input whose segments are all in range."""
    M = score.numel()
    lab = label.bool()
    G = torch.cumsum(lab.long(), 0) - torch.cumsum((~lab).long(), 0)
    P = torch.cumsum(lab.long(), 0)
    idx = torch.arange(M, device=score.device)
    nxt_same = torch.zeros(M, dtype=torch.bool, device=score.device)
    nxt_same[:-1] = seg[1:] == seg[:-1]
    nxt = torch.cat([score[1:], score.new_full((1,), float("nan"))])
    adm = ~torch.isnan(score) & (~nxt_same | torch.isnan(nxt) | (score < nxt))
    ids = torch.arange(n_seg, device=score.device, dtype=seg.dtype)
    start, end = torch.searchsorted(seg, ids), torch.searchsorted(seg, ids, right=True)
    has = end > start
    at = lambda v, i: torch.where(i > 0, v[(i - 1).clamp(min=0)], torch.zeros_like(v[:1]))
    n_pos = at(P, end) - at(P, start)
    n_neg = (end - start) - n_pos
    base = at(G, start)
    key = torch.where(adm, (G + M) * (2 * M) + (M - 1 - idx), torch.full_like(G, -1))
    best = torch.full((n_seg,), -1, dtype=torch.long, device=score.device).scatter_reduce(0, seg.long(), key, "amax")
    g, i = torch.div(best, 2 * M, rounding_mode="floor") - M, (M - 1 - best % (2 * M)).clamp(0, M - 1)
    win = (best >= 0) & (g > base)
    inf = score.new_full((1,), float("inf"))
    hi_cut = torch.where(nxt_same[i] & ~torch.isnan(nxt[i]), nxt[i], inf)
    first = score[start.clamp(max=M - 1)]
    hi0 = torch.where(has & ~torch.isnan(first), first, inf)
    return {"thr_lo": torch.where(win, score[i], -inf), "thr_hi": torch.where(win, hi_cut, hi0),
            "best_correct": (n_neg + torch.where(win, g - base, torch.zeros_like(g))).int(),
            "n_pos": n_pos.int(), "n_neg": n_neg.int()}


def torch_classify(score, seg, label, thr, n_seg):
    pred = score <= thr[seg.long()]
    lab = label.bool()
    cls = torch.where(pred, torch.where(lab, 0, 1), torch.where(lab, 3, 2))
    return pred, torch.bincount(seg.long() * 4 + cls, minlength=4 * n_seg).view(n_seg, 4).int()


@torch.no_grad()
def run(shape, score, seg, label, n_seg, calls):
    M = score.numel()
    lib = _lib.load()
    st = lambda: torch.cuda.current_stream().cuda_stream
    state = {}

    def sort():
        order = torch.sort(CL._sort_key(score, seg)).indices
        state["s"], state["g"], state["l"] = score[order].contiguous(), seg[order].contiguous(), label[order].contiguous()
    sort_ms, _ = timed_pair(sort, sort, calls)
    s, g, l = state["s"], state["g"], state["l"]
    ws = torch.empty(int(lib.ge_threshold_fit_workspace_bytes(M, n_seg)), dtype=torch.uint8, device="cuda")
    out = {k: torch.empty(n_seg, dtype=torch.float32 if k.startswith("thr") else torch.int32, device="cuda")
           for k in CL._FIELDS}

    def native_fit():
        _lib.call("ge_threshold_fit", s.data_ptr(), g.data_ptr(), l.data_ptr(), M, n_seg,
                  *(out[k].data_ptr() for k in CL._FIELDS), ws.data_ptr(), ws.numel(), st())
    fit_ms, torch_fit_ms = timed_pair(native_fit, lambda: state.__setitem__("t", torch_fit(s, g, l, n_seg)), calls)
    for k in CL._FIELDS:
        assert torch.equal(out[k], state["t"][k]), f"{shape}: the torch fit and ge_threshold_fit differ in {k}"
    thr = CL._resolve_pair(out["thr_lo"], out["thr_hi"], "mid").contiguous()
    pred = torch.empty(M, dtype=torch.uint8, device="cuda")
    conf = torch.empty(n_seg, 4, dtype=torch.int32, device="cuda")

    def native_classify():
        _lib.call("ge_threshold_classify", score.data_ptr(), seg.data_ptr(), label.data_ptr(), M, n_seg, thr.data_ptr(),
                  pred.data_ptr(), conf.data_ptr(), st())
    classify_ms, torch_classify_ms = timed_pair(
        native_classify, lambda: state.__setitem__("c", torch_classify(score, seg, label, thr, n_seg)), calls)
    assert torch.equal(pred.bool(), state["c"][0]) and torch.equal(conf, state["c"][1]), f"{shape}: classify differs"
    rec = {"shape": shape, "M": M, "n_seg": n_seg, "largest_segment": int(torch.bincount(seg.long()).max()),
           "sort_ms": sort_ms, "fit_ms": fit_ms, "torch_fit_ms": torch_fit_ms, "classify_ms": classify_ms,
           "torch_classify_ms": torch_classify_ms, "fit_read_GBps": 14 * M / fit_ms / 1e6,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("classify_bench needs an MI355X: there is nothing to time without one")
    rng = np.random.default_rng(0)
    recs = []
    # FB15k's validation shape: 50,000 positives + 50,000 negatives, relation frequencies ~ 1 / rank
    M, R = 100_000, 1345
    w = 1.0 / np.arange(1, R + 1)
    seg = rng.choice(R, M, p=w / w.sum()).astype(np.int32)
    # 4 M triples over 16 relations, relation 0 holding half
    M2, R2 = 4_000_000, 16
    seg2 = np.where(rng.random(M2) < 0.5, 0, rng.integers(1, R2, M2)).astype(np.int32)
    for shape, sg, n_seg in (("fb15k_valid", seg, R), ("hot_relation", seg2, R2)):
        m = len(sg)
        label = rng.integers(0, 2, m).astype(np.uint8)
        score = (rng.standard_normal(m) + 1.5 * (1 - label)).astype(np.float32)    # positives lower, overlapping
        to = lambda x: torch.as_tensor(x).cuda()
        recs.append(run(shape, to(score), to(sg), to(label), n_seg, a.calls))
    if a.out:
        with open(a.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in recs)


if __name__ == "__main__":
    main()
