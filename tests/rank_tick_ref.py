"""NumPy fp64 restatement of ge_rank_metrics (include/ge_hip.h) and of the pocket rule over a sequence of ticks.

rank_metrics: row i counts iff true_loss is None or true_loss[i] is not NaN, and 0 <= n_known_before[i] <= n_before[i];
raw = 1 + n_before, fil = raw - n_known_before; the eight outputs as float64 (the kernel rounds each to float32 once).
The rank sums and hit counts are integers (int64 here); the reciprocal sums use math.fsum, so the reference's own error is
one rounding of the sum -- far below the 2^-24 half-ulp of a float32 MRR.

pocket: improved = mrr > best, NaN never, a tie keeps the first best.
"""
import math

import numpy as np

KEYS = ("filtered_mrr", "raw_mrr", "mean_filtered_pos", "mean_raw_pos", "hits1", "hits3", "hits10", "counted")
MRR_TOL = 2.0 ** -23      # entries 0 and 1: MRR <= 1, so the final rounding to float32 moves it by at most one ulp of 1


def counted_rows(n_before, n_known_before, true_loss=None) -> np.ndarray:
    nb, nk = np.asarray(n_before, dtype=np.int64), np.asarray(n_known_before, dtype=np.int64)
    ok = (nk >= 0) & (nk <= nb)
    if true_loss is not None:
        ok &= ~np.isnan(np.asarray(true_loss, dtype=np.float64))
    return ok


def ranks(n_before, n_known_before, true_loss=None):
    """(raw, filtered) int64 ranks of the counted rows."""
    ok = counted_rows(n_before, n_known_before, true_loss)
    raw = 1 + np.asarray(n_before, dtype=np.int64)[ok]
    return raw, raw - np.asarray(n_known_before, dtype=np.int64)[ok]


def rank_metrics(n_before, n_known_before, true_loss=None) -> np.ndarray:
    raw, fil = ranks(n_before, n_known_before, true_loss)
    n = raw.size
    if n == 0:
        return np.array([np.nan] * 7 + [0.0])
    hits = lambda k: (100.0 * int(np.count_nonzero(fil <= k))) / n
    return np.array([math.fsum(1.0 / fil.astype(np.float64)) / n, math.fsum(1.0 / raw.astype(np.float64)) / n,
                     int(fil.sum()) / n, int(raw.sum()) / n, hits(1), hits(3), hits(10), float(n)])


def as_dict(metrics) -> dict:
    return dict(zip(KEYS, (float(x) for x in metrics)))


def pocket(mrrs, best: float = 0.0):
    """The pocket rule over the ticks' MRRs in order: ([best after each tick], [improved at each tick])."""
    bests, improved = [], []
    for m in mrrs:
        imp = bool(m > best)
        if imp:
            best = m
        bests.append(best)
        improved.append(imp)
    return bests, improved


def check_metrics(got, ref, what=""):
    """The bounds of the kernel's eight float32 outputs against rank_metrics' float64 ones: entries 2-7 equal
    float32(reference) exactly (integer sums, one correctly rounded division); entries 0 and 1 within 2^-23 of it."""
    got, ref32 = np.asarray(got, dtype=np.float32), np.asarray(ref, dtype=np.float64).astype(np.float32)
    print("RANK METRICS %s: got %s ref %s |d mrr| %.3g %.3g" % (what, got.tolist(), ref32.tolist(),
                                                                 abs(float(got[0]) - float(ref32[0])),
                                                                 abs(float(got[1]) - float(ref32[1]))))
    if ref[7] == 0:
        assert np.isnan(got[:7]).all() and got[7] == 0, (what, got)
        return
    assert np.array_equal(got[2:].view(np.int32), ref32[2:].view(np.int32)), (what, got, ref32)
    assert abs(float(got[0]) - float(ref32[0])) <= MRR_TOL and abs(float(got[1]) - float(ref32[1])) <= MRR_TOL, (what, got, ref32)
