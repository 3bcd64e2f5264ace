"""numpy reference of triple classification (include/ge_hip.h: ge_threshold_fit / ge_threshold_classify, and
graphembeddings_amd.classify's resolve).  The fit evaluates every admissible cut of every segment directly in int64: fit_segment
by a plain loop (small inputs), fit() for all segments at once.
"""
import numpy as np

I32, I64, F32, U8 = np.int32, np.int64, np.float32, np.uint8


def sort_order(score, seg):
    """The order ge_threshold_fit expects: (seg ascending, score ascending, NaN last), stable."""
    score = np.asarray(score, F32)
    nan = np.isnan(score)
    return np.lexsort((np.where(nan, F32(0), score), nan, np.asarray(seg, I64)))


def fit_segment(score, label):
    """One segment, ALREADY sorted ascending with NaN last: (thr_lo, thr_hi, best_correct, n_pos, n_neg)."""
    score, label = np.asarray(score, F32), np.asarray(label, I64)
    m = len(score)
    n_pos, n_neg = int((label != 0).sum()), int((label == 0).sum())
    if m == 0:
        return F32(-np.inf), F32(np.inf), 0, 0, 0
    m_v = int((~np.isnan(score)).sum())
    best_p, best = 0, n_neg
    for p in range(1, m_v + 1):
        if not (p == m_v or score[p - 1] < score[p]):
            continue
        correct = int((label[:p] != 0).sum()) + int((label[p:] == 0).sum())
        if correct > best:
            best_p, best = p, correct
    lo = F32(-np.inf) if best_p == 0 else score[best_p - 1]
    hi = F32(np.inf) if best_p == m_v else score[best_p]
    return lo, hi, best, n_pos, n_neg


def fit(score, seg, label, n_seg):
    """ge_threshold_fit on input in ANY order (sorted here): the five [n_seg] outputs as a dict.  Every admissible cut
    of every segment is evaluated at once, in int64: correct = positives at or before the cut + negatives after it."""
    score, seg, label = np.asarray(score, F32), np.asarray(seg, I64), np.asarray(label) != 0
    o = sort_order(score, seg)
    score, seg, label = score[o], seg[o], label[o]
    keep = (seg >= 0) & (seg < n_seg)                   # elements of no segment are ignored
    score, seg, label = score[keep], seg[keep], label[keep]
    m = len(score)
    out = {"thr_lo": np.full(n_seg, -np.inf, F32), "thr_hi": np.full(n_seg, np.inf, F32),
           "best_correct": np.zeros(n_seg, I32), "n_pos": np.zeros(n_seg, I32), "n_neg": np.zeros(n_seg, I32)}
    if m == 0:
        return out
    n_pos = np.bincount(seg[label], minlength=n_seg).astype(I64)
    n_neg = np.bincount(seg[~label], minlength=n_seg).astype(I64)
    out["n_pos"], out["n_neg"] = n_pos.astype(I32), n_neg.astype(I32)
    start = np.searchsorted(seg, np.arange(n_seg), "left")
    pos_to = np.cumsum(label.astype(I64))               # positives / negatives at or before element i, all segments
    neg_to = np.cumsum((~label).astype(I64))
    pos_in = pos_to - (pos_to[start[seg]] - label[start[seg]])          # ... of i's own segment
    neg_in = neg_to - (neg_to[start[seg]] - (~label[start[seg]]))
    correct = pos_in + (n_neg[seg] - neg_in)            # the cut after element i
    nxt_same = np.zeros(m, bool)
    nxt_same[:-1] = seg[1:] == seg[:-1]
    nxt = np.empty(m, F32)
    nxt[:-1], nxt[-1] = score[1:], np.nan
    with np.errstate(invalid="ignore"):
        adm = ~np.isnan(score) & (~nxt_same | np.isnan(nxt) | (score < nxt))
    idx = np.nonzero(adm)[0]
    # per segment the first admissible cut with the largest correct
    first = idx[np.lexsort((idx, -correct[idx], seg[idx]))]
    first = first[np.concatenate([[True], seg[first][1:] != seg[first][:-1]])] if len(first) else first
    out["best_correct"] = n_neg.astype(I32)             # p = 0
    nonempty = np.nonzero(np.bincount(seg, minlength=n_seg))[0]
    s0 = score[start[nonempty]]
    out["thr_hi"][nonempty] = np.where(np.isnan(s0), F32(np.inf), s0)
    win = first[correct[first] > n_neg[seg[first]]]
    ws = seg[win]
    out["best_correct"][ws] = correct[win].astype(I32)
    out["thr_lo"][ws] = score[win]
    hi = np.where(nxt_same[win] & ~np.isnan(nxt[win]), nxt[win], F32(np.inf))
    out["thr_hi"][ws] = hi
    return out


def fit_by_segment(score, seg, label, n_seg):
    """fit() with fit_segment's plain loop over the cuts of each segment: the check of fit() itself (small inputs)."""
    score, seg, label = np.asarray(score, F32), np.asarray(seg, I64), np.asarray(label)
    o = sort_order(score, seg)
    score, seg, label = score[o], seg[o], label[o]
    out = {"thr_lo": np.full(n_seg, -np.inf, F32), "thr_hi": np.full(n_seg, np.inf, F32),
           "best_correct": np.zeros(n_seg, I32), "n_pos": np.zeros(n_seg, I32), "n_neg": np.zeros(n_seg, I32)}
    for s in range(n_seg):
        r = fit_segment(score[seg == s], label[seg == s])
        for k, v in zip(("thr_lo", "thr_hi", "best_correct", "n_pos", "n_neg"), r):
            out[k][s] = v
    return out


def classify(score, seg, thr, n_seg, label=None):
    """ge_threshold_classify: (pred uint8 [M], confusion int32 [n_seg, 4] = tp, fp, tn, fn, or None)."""
    score, seg, thr = np.asarray(score, F32), np.asarray(seg, I64), np.asarray(thr, F32)
    ok = (seg >= 0) & (seg < n_seg)
    pred = np.zeros(len(score), bool)
    with np.errstate(invalid="ignore"):
        pred[ok] = score[ok] <= thr[seg[ok]]
    if label is None:
        return pred.astype(U8), None
    lab = np.asarray(label) != 0
    conf = np.zeros((n_seg, 4), I32)
    for c, m in enumerate((pred & lab, pred & ~lab, ~pred & ~lab, ~pred & lab)):
        np.add.at(conf[:, c], seg[ok & m], 1)
    return pred.astype(U8), conf


def resolve_pair(lo, hi, mode):
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    if mode == "lo":
        return lo.copy()
    with np.errstate(invalid="ignore"):
        mid = (0.5 * (lo.astype(np.float64) + hi.astype(np.float64))).astype(F32)
        mid = np.where(mid >= hi, lo, mid)
    mid = np.where(np.isposinf(hi), hi, mid)
    return np.where(np.isneginf(lo), lo, mid).astype(F32)


def resolve(per_rel, glob, mode="mid", fallback="global"):
    """Thresholds.resolve: per_rel the fit's dict over relations, glob the dict of the one global segment."""
    own = resolve_pair(per_rel["thr_lo"], per_rel["thr_hi"], mode)
    g = resolve_pair(glob["thr_lo"][:1], glob["thr_hi"][:1], mode)[0]
    degenerate = (per_rel["n_pos"] == 0) | (per_rel["n_neg"] == 0)
    return np.where(degenerate & (fallback == "global"), g, own).astype(F32)


def accuracies(conf):
    """(overall accuracy, macro accuracy over the relations that have triples) of a [n_rel, 4] confusion table."""
    conf = np.asarray(conf, I64)
    tot = conf.sum(1)
    right = conf[:, 0] + conf[:, 2]
    have = tot > 0
    return float(right.sum()) / float(max(tot.sum(), 1)), float(np.mean(right[have] / tot[have])) if have.any() else 0.0
