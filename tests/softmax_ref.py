"""The 1-vs-all softmax objective of ComplEx (include/ge_hip.h: ge_softmax_loss / ge_softmax_grad) in closed form, NumPy.

    x^     = x * min(1, max_norm / |x|)                      (rows clipped on lookup; the clip is active iff |x| >= max_norm)
    s_ij   = Re< h^, r^, conj(t^) >                          candidate = tail (head=False) or head (head=True)
    z_ij   = -scale * s_ij
    loss_i = logsumexp_j(z_ij) - z_i,true                    NaN for an invalid row
    dL/ds_ij = -scale * (softmax_j(z_ij) - [cand_j == true_i])

chained through the score and the three clips.  `dtype` float64 is the oracle; float32 evaluates the SAME formulas in
float32 with the sums over rows (queries for a candidate's gradient, candidates for a query's) taken in index order --
its distance from the fp64 result is the yardstick of the GPU tolerance (e32 of tests/test_gpu_softmax.py)."""
import numpy as np

from tests import adagrad_ref as AR


def _clip(x, max_norm):
    n = np.sqrt((x * x).sum(1))
    with np.errstate(divide="ignore"):
        sc = np.minimum(x.dtype.type(1), x.dtype.type(max_norm) / n).astype(x.dtype)
    return x * sc[:, None], n


def _clip_back(x, n, g, max_norm):
    """dL/dx from g = dL/d clip(x): alpha g + beta x (row_coef of csrc/ge_complex_dev.h)."""
    dt = x.dtype.type
    xg = (x * g).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        alpha = dt(max_norm) / n
        act = alpha[:, None] * (g - x * (xg / (n * n))[:, None])
    return np.where((n >= dt(max_norm))[:, None], act, g).astype(x.dtype)


def query(fh, rh, head):
    """Q' [B,d] from the clipped fixed and relation rows, in the staging form of score_1vK_kernel."""
    k = fh.shape[1] // 2
    a, b, e, h = fh[:, :k], fh[:, k:], rh[:, :k], rh[:, k:]
    if not head:
        return np.concatenate([a * e - b * h, a * h + b * e], 1)
    return np.concatenate([e * a + h * b, e * b - h * a], 1)


def evaluate(table, hr, true_id, cand, max_norm, scale, head, lr=1.0, dtype=np.float64):
    """(loss [B], grad_idx [K + 2B] int32, grad_val [K + 2B, d] = -lr * gradient of SUM_i loss_i) in `dtype`."""
    dt = np.dtype(dtype).type
    T = np.asarray(table).astype(dtype)
    N, d = T.shape
    k = d // 2
    hr, true_id, cand = np.asarray(hr, np.int64), np.asarray(true_id, np.int64), np.asarray(cand, np.int64)
    B, K = hr.shape[0], cand.shape[0]
    inr = lambda v: (v >= 0) & (v < N)
    cok = inr(cand)
    pos = np.full(B, -1, np.int64)
    where = {int(c): j for j, c in enumerate(cand) if cok[j]}
    for i in range(B):
        pos[i] = where.get(int(true_id[i]), -1)
    valid = inr(hr[:, 0]) & inr(hr[:, 1]) & inr(true_id) & (pos >= 0)
    safe = lambda v: np.where(inr(v), v, 0)
    f, r, c = T[safe(hr[:, 0])], T[safe(hr[:, 1])], T[safe(cand)]
    fh, nf = _clip(f, max_norm)
    rh, nr = _clip(r, max_norm)
    ch, nc = _clip(c, max_norm)
    Q = query(fh, rh, head)
    S = Q @ ch.T
    z = (dt(-scale) * S).astype(dtype)
    z[:, ~cok] = -np.inf
    z[~valid] = 0.0
    m = z.max(1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(1, dtype=dtype))
    rows = np.arange(B)
    loss = np.where(valid, lse - z[rows, np.maximum(pos, 0)], np.nan).astype(dtype)
    p = np.exp(z - lse[:, None])
    y = np.zeros((B, K), dtype)
    y[rows[valid], pos[valid]] = 1
    w = (dt(-scale) * (p - y)).astype(dtype)
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
    gc = _clip_back(c, nc, GC, max_norm)
    Gre, Gim = GQ[:, :k], GQ[:, k:]
    a, b, e, h = fh[:, :k], fh[:, k:], rh[:, :k], rh[:, k:]
    if not head:
        gfh = np.concatenate([Gre * e + Gim * h, Gim * e - Gre * h], 1)
        grh = np.concatenate([Gre * a + Gim * b, Gim * a - Gre * b], 1)
    else:
        gfh = np.concatenate([Gre * e - Gim * h, Gre * h + Gim * e], 1)
        grh = np.concatenate([Gre * a + Gim * b, Gre * b - Gim * a], 1)
    gf, gr = _clip_back(f, nf, gfh, max_norm), _clip_back(r, nr, grh, max_norm)
    idx = np.full(K + 2 * B, -1, np.int32)
    val = np.zeros((K + 2 * B, d), dtype)
    idx[:K][cok] = cand[cok]
    val[:K][cok] = gc[cok]
    qi = np.nonzero(valid)[0]
    idx[K + 2 * qi], idx[K + 2 * qi + 1] = hr[qi, 0], hr[qi, 1]
    val[K + 2 * qi], val[K + 2 * qi + 1] = gf[qi], gr[qi]
    return loss, idx, (dt(-lr) * val).astype(dtype)


def step(table, accum, triples, cand, max_norm, scale, lr):
    """One SoftmaxAdaGrad step in place on fp64 `table` / `accum`: both sides against the table as it is, one AdaGrad
    update of every row named from its summed gradient.  Returns (loss [B,2], per-row sums [N,d], rows named [N])."""
    tri = np.asarray(triples, np.int64)
    lt, it, vt = evaluate(table, tri[:, [0, 2]], tri[:, 1], cand, max_norm, scale, False)
    lh, ih, vh = evaluate(table, tri[:, [1, 2]], tri[:, 0], cand, max_norm, scale, True)
    s, named = AR.apply_rows(table, accum, np.concatenate([it, ih]), -np.concatenate([vt, vh]), lr)
    return np.stack([lt, lh], 1), s, named
