"""The multi-label (K-vs-all) softmax objective of ComplEx (include/ge_hip.h: ge_softmax_labels_loss / ge_softmax_labels_grad)
in closed form, NumPy, on the helpers of tests/softmax_ref.py.

    row i = the query (fixed_i, rel_i); its labels = the candidate positions label_pos[label_off[i] : label_off[i + 1]], n_i
    loss_i = logsumexp_j(z_ij) - (1 / n_i) sum_l z_i,l                  NaN for an invalid row
    dL/ds_ij = -scale * (softmax_j(z_ij) - y_ij / n_i)                  y_ij = labels of row i at position j

The gradient comes in K + 2B + L slots: the candidates' slots hold the softmax term alone, every label entry has a slot of
its own with the label term of its candidate (the clip derivative is linear in its argument, so the slots of one table
row sum to its gradient), the queries' two slots hold both terms.  `dtype` float64 is the oracle; float32 evaluates the
SAME formulas in float32 with the sums over rows in index order, as softmax_ref.evaluate does."""
import numpy as np

from tests import adagrad_ref as AR
from tests import softmax_ref as SR


def evaluate(table, hr, label_off, label_pos, cand, max_norm, scale, head, lr=1.0, dtype=np.float64):
    """(loss [B], grad_idx [K + 2B + L] int32, grad_val [K + 2B + L, d] = -lr * gradient of SUM_i loss_i) in `dtype`."""
    dt = np.dtype(dtype).type
    T = np.asarray(table).astype(dtype)
    N, d = T.shape
    k = d // 2
    hr, cand = np.asarray(hr, np.int64), np.asarray(cand, np.int64)
    off, lpos = np.asarray(label_off, np.int64), np.asarray(label_pos, np.int64)
    B, K, L = hr.shape[0], cand.shape[0], lpos.shape[0]
    assert off.shape[0] == B + 1
    inr = lambda v: (v >= 0) & (v < N)
    cok = inr(cand)
    valid = inr(hr[:, 0]) & inr(hr[:, 1])
    labels = [None] * B
    for i in range(B):
        lo, hi = off[i], off[i + 1]
        ok = 0 <= lo < hi <= L
        if ok:
            p = lpos[lo:hi]
            ok = bool(((p >= 0) & (p < K)).all()) and bool(cok[p].all())
        valid[i] = valid[i] and ok
        labels[i] = lpos[lo:hi] if valid[i] else None
    safe = lambda v: np.where(inr(v), v, 0)
    f, r, c = T[safe(hr[:, 0])], T[safe(hr[:, 1])], T[safe(cand)]
    fh, nf = SR._clip(f, max_norm)
    rh, nr = SR._clip(r, max_norm)
    ch, nc = SR._clip(c, max_norm)
    Q = SR.query(fh, rh, head)
    z = (dt(-scale) * (Q @ ch.T)).astype(dtype)
    z[:, ~cok] = -np.inf
    z[~valid] = 0.0
    m = z.max(1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(1, dtype=dtype))
    mean = np.zeros(B, dtype)
    lsum = np.zeros((B, d), dtype)                      # (scale / n_i) sum_l C'_l, in label order
    for i in np.nonzero(valid)[0]:
        zs = dt(0)
        for l in labels[i]:
            zs += z[i, l]
            lsum[i] += ch[l]
        mean[i] = zs / dt(len(labels[i]))
        lsum[i] *= dt(scale) / dt(len(labels[i]))
    loss = np.where(valid, lse - mean, np.nan).astype(dtype)
    w = (dt(-scale) * np.exp(z - lse[:, None])).astype(dtype)
    w[~valid] = 0
    w[:, ~cok] = 0
    if dtype == np.float64:
        GC, GQ = w.T @ Q, w @ ch
    else:                                   # in index order
        GC, GQ = np.zeros((K, d), dtype), np.zeros((B, d), dtype)
        for i in range(B):
            GC += w[i][:, None] * Q[i][None, :]
        for j in range(K):
            GQ += w[:, j][:, None] * ch[j][None, :]
    GQ = GQ + lsum
    gc = SR._clip_back(c, nc, GC, max_norm)
    Gre, Gim = GQ[:, :k], GQ[:, k:]
    a, b, e, h = fh[:, :k], fh[:, k:], rh[:, :k], rh[:, k:]
    if not head:
        gfh = np.concatenate([Gre * e + Gim * h, Gim * e - Gre * h], 1)
        grh = np.concatenate([Gre * a + Gim * b, Gim * a - Gre * b], 1)
    else:
        gfh = np.concatenate([Gre * e - Gim * h, Gre * h + Gim * e], 1)
        grh = np.concatenate([Gre * a + Gim * b, Gre * b - Gim * a], 1)
    gf, gr = SR._clip_back(f, nf, gfh, max_norm), SR._clip_back(r, nr, grh, max_norm)
    R = K + 2 * B + L
    idx = np.full(R, -1, np.int32)
    val = np.zeros((R, d), dtype)
    idx[:K][cok] = cand[cok]
    val[:K][cok] = gc[cok]
    qi = np.nonzero(valid)[0]
    idx[K + 2 * qi], idx[K + 2 * qi + 1] = hr[qi, 0], hr[qi, 1]
    val[K + 2 * qi], val[K + 2 * qi + 1] = gf[qi], gr[qi]
    for i in qi:
        p = labels[i]
        g = (dt(scale) / dt(len(p))) * Q[i]            # dL/dC'_l of the label term: -(1 / n_i) dz_il/dC'_l = (scale / n_i) Q'_i
        x = K + 2 * B + off[i] + np.arange(len(p))
        idx[x] = cand[p]
        val[x] = SR._clip_back(c[p], nc[p], np.broadcast_to(g, (len(p), d)).astype(dtype), max_norm)
    return loss, idx, (dt(-lr) * val).astype(dtype)


def step(table, accum, tail_batch, head_batch, cand, max_norm, scale, lr):
    """One LabelSoftmaxAdaGrad step in place on fp64 `table` / `accum`: both sides ((hr, label_off, label_pos) or None)
    against the table as it is, one AdaGrad update of every row named from its summed gradient.  Returns (losses of the
    sides that have rows, concatenated; per-row sums [N,d]; rows named [N])."""
    losses, idx, val = [], [], []
    for batch, head in ((tail_batch, False), (head_batch, True)):
        if batch is None or len(batch[0]) == 0:
            continue
        l, i, v = evaluate(table, batch[0], batch[1], batch[2], cand, max_norm, scale, head)
        losses.append(l), idx.append(i), val.append(v)
    s, named = AR.apply_rows(table, accum, np.concatenate(idx), -np.concatenate(val), lr)
    return np.concatenate(losses), s, named
