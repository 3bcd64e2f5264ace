"""Restatement of the reference's prediction heap (holE.py:427-469) for the top-k tests: what it pops, in which order,
and which lines it writes to inference_results.tsv.  Not product code."""
from heapq import heappop, heappush

import numpy as np


def heap_pops(losses, ids):
    """Every (loss, id) in the order holE.py:445-447 pops them: a min-heap of (loss, triple tuple); for one query the
    tuples differ only in the candidate, so ties go to the smaller id."""
    heap = []
    for l, i in zip(losses, ids):
        heappush(heap, (float(l), int(i)))
    out = []
    while heap:
        out.append(heappop(heap))
    return out


def first_k(losses, ids, k, known=frozenset()):
    """The first k pops that are not known-true (the filtered list), padded with (+inf, -1)."""
    out = [(l, i) for l, i in heap_pops(losses, ids) if i not in known][:k]
    out += [(float("inf"), -1)] * (k - len(out))
    return np.array([i for _, i in out], dtype=np.int64), np.array([l for l, _ in out], dtype=np.float32)


def first_k_rows(losses, ids, k, known_mask=None):
    """first_k for every row of a [B, K] loss matrix, by a lexicographic sort (equal to the heap: keys are distinct)."""
    losses = np.asarray(losses, dtype=np.float32)
    ids = np.asarray(ids, dtype=np.int64)
    B, K = losses.shape
    out_id = np.full((B, k), -1, dtype=np.int64)
    out_l = np.full((B, k), np.inf, dtype=np.float32)
    for b in range(B):
        keep = np.ones(K, dtype=bool) if known_mask is None else ~known_mask[b]
        l, i = losses[b][keep], ids[keep]
        o = np.lexsort((i, l))[:k]
        out_id[b, :o.size], out_l[b, :o.size] = i[o], l[o]
    return out_id, out_l


def write_set(losses, ids, head, relation, max_triples, true_set, infer_threshold):
    """The lines eval_link_prediction (holE.py:427-456) writes for one (head, relation, ?) sweep, transcribed."""
    heap = []
    min_loss = 100
    for l, t in zip(losses, ids):
        loss = float(l)
        min_loss = min(min_loss, loss)
        heappush(heap, (loss, (int(head), int(t), int(relation))))
    is_confident = min_loss < infer_threshold
    filtered_rank = 0
    lines = []
    while heap:
        pair = heappop(heap)
        loss = pair[0]
        head_id, tail_id, relation_id = pair[1]
        in_sample = tail_id in true_set
        if is_confident and filtered_rank < max_triples:
            lines.append('{:.6f}\t{}\t{}\t{}\t{}\n'.format(loss, head_id, tail_id, relation_id, in_sample))
        if is_confident and in_sample:
            continue
        filtered_rank += 1
    return lines
