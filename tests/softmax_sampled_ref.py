"""Sampled softmax with shared negatives (include/ge_hip.h: ge_softmax_sampled_loss / ge_softmax_sampled_grad) in closed
form, NumPy -- tests/softmax_ref.py's objective over candidates that need not hold the true entity and may repeat.

    z_ij     = -scale * s_ij,   z_i,true = -scale * (Q'_i . clip(true_i))     (the true entity's own logit, counted once)
    loss_i   = log(exp(z_i,true) + sum_{j: cand_j in [0,N), cand_j != true_i} exp(z_ij)) - z_i,true       NaN if invalid
    dL/ds_ij = -scale * p_ij (0 for a slot left out),   dL/ds_i,true = -scale * (p_i,true - 1)

A row is valid iff its fixed, relation and true ids lie in [0, N).  Slots: j < K the candidates, K + 3i the fixed row,
K + 3i + 1 the relation, K + 3i + 2 the true entity.  `dtype` float64 is the oracle; float32 evaluates the SAME formulas in
float32 with the sums over rows taken in index order -- its distance from the fp64 result is the yardstick of the GPU
tolerance (e32 of tests/test_gpu_softmax_sampled.py)."""
import numpy as np

from tests import adagrad_ref as AR
from tests.softmax_ref import _clip, _clip_back, query


def evaluate(table, hr, true_id, cand, max_norm, scale, head, lr=1.0, dtype=np.float64):
    """(loss [B], grad_idx [K + 3B] int32, grad_val [K + 3B, d] = -lr * gradient of SUM_i loss_i) in `dtype`."""
    dt = np.dtype(dtype).type
    T = np.asarray(table).astype(dtype)
    N, d = T.shape
    k = d // 2
    hr, true_id, cand = np.asarray(hr, np.int64), np.asarray(true_id, np.int64), np.asarray(cand, np.int64)
    B, K = hr.shape[0], cand.shape[0]
    inr = lambda v: (v >= 0) & (v < N)
    cok = inr(cand)
    valid = inr(hr[:, 0]) & inr(hr[:, 1]) & inr(true_id)
    safe = lambda v: np.where(inr(v), v, 0)
    f, r, c, t = T[safe(hr[:, 0])], T[safe(hr[:, 1])], T[safe(cand)], T[safe(true_id)]
    fh, nf = _clip(f, max_norm)
    rh, nr = _clip(r, max_norm)
    ch, nc = _clip(c, max_norm)
    th, nt = _clip(t, max_norm)
    Q = query(fh, rh, head)
    z = (dt(-scale) * (Q @ ch.T)).astype(dtype)
    out = ~cok[None, :] | (cand[None, :] == true_id[:, None])          # no term of the row's softmax
    z[out] = -np.inf
    zt = (dt(-scale) * (Q * th).sum(1, dtype=dtype)).astype(dtype)
    z[~valid], zt[~valid] = -np.inf, 0.0
    m = np.maximum(z.max(1), zt) if K else zt
    with np.errstate(invalid="ignore"):
        lse = m + np.log(np.exp(z - m[:, None]).sum(1, dtype=dtype) + np.exp(zt - m))
        loss = np.where(valid, lse - zt, np.nan).astype(dtype)
        w = (dt(-scale) * np.exp(z - lse[:, None])).astype(dtype)
        wt = (dt(-scale) * (np.exp(zt - lse) - dt(1))).astype(dtype)
    w[out] = 0
    w[~valid], wt[~valid] = 0, 0
    if dtype == np.float64:
        GC, GQ = w.T @ Q, w @ ch
    else:                                   # in index order
        GC, GQ = np.zeros((K, d), dtype), np.zeros((B, d), dtype)
        for i in range(B):
            GC += w[i][:, None] * Q[i][None, :]
        for j in range(K):
            GQ += w[:, j][:, None] * ch[j][None, :]
    GQ = GQ + wt[:, None] * th
    GT = wt[:, None] * Q
    gc, gt = _clip_back(c, nc, GC, max_norm), _clip_back(t, nt, GT, max_norm)
    Gre, Gim = GQ[:, :k], GQ[:, k:]
    a, b, e, h = fh[:, :k], fh[:, k:], rh[:, :k], rh[:, k:]
    if not head:
        gfh = np.concatenate([Gre * e + Gim * h, Gim * e - Gre * h], 1)
        grh = np.concatenate([Gre * a + Gim * b, Gim * a - Gre * b], 1)
    else:
        gfh = np.concatenate([Gre * e - Gim * h, Gre * h + Gim * e], 1)
        grh = np.concatenate([Gre * a + Gim * b, Gre * b - Gim * a], 1)
    gf, gr = _clip_back(f, nf, gfh, max_norm), _clip_back(r, nr, grh, max_norm)
    idx = np.full(K + 3 * B, -1, np.int32)
    val = np.zeros((K + 3 * B, d), dtype)
    idx[:K][cok] = cand[cok]
    val[:K][cok] = gc[cok]
    qi = np.nonzero(valid)[0]
    idx[K + 3 * qi], idx[K + 3 * qi + 1], idx[K + 3 * qi + 2] = hr[qi, 0], hr[qi, 1], true_id[qi]
    val[K + 3 * qi], val[K + 3 * qi + 1], val[K + 3 * qi + 2] = gf[qi], gr[qi], gt[qi]
    return loss, idx, (dt(-lr) * val).astype(dtype)


def merged(idx, val, N):
    """The slices summed by row id: [N, d]."""
    out = np.zeros((N, val.shape[1]), val.dtype)
    ok = idx >= 0
    np.add.at(out, idx[ok], val[ok])
    return out


def step(table, accum, triples, cand, max_norm, scale, lr):
    """One SampledSoftmaxAdaGrad step in place on fp64 `table` / `accum`: both sides against the same candidates and the
    table as it is, one AdaGrad update of every row named from its summed gradient.  Returns (loss [B,2], per-row sums
    [N,d], rows named [N])."""
    tri = np.asarray(triples, np.int64)
    lt, it, vt = evaluate(table, tri[:, [0, 2]], tri[:, 1], cand, max_norm, scale, False)
    lh, ih, vh = evaluate(table, tri[:, [1, 2]], tri[:, 0], cand, max_norm, scale, True)
    s, named = AR.apply_rows(table, accum, np.concatenate([it, ih]), -np.concatenate([vt, vh]), lr)
    return np.stack([lt, lh], 1), s, named
