"""fp64 restatement of transR.py for the tests (product code never imports it).

Forward u = M_r (h - t) + r with M_r = rel_matrix[r] read as [dim_r][dim_e], D = sum |u| (L1) or sum u^2, the
hinge loss and its gradient with TF1's rules written out by hand (a pair is active iff D+ - D- + margin >= 0;
d|x|/dx = sign(x) with sign(0) = 0), the gradient's IndexedSlices as TF builds them (one slice per looked-up id:
ent 4 per pair, rel 2 per pair (pos_r, neg_r), rel_matrix 1 per pair), and TF1's Adam on every element of every
table with a `dedup` flag: True sums duplicate slices first, so v takes (1-b2) (sum g)^2 (the TF 1.x sparse path and
the product); False adds the slices' squares, (1-b2) sum g^2 (an optimizer that scatter_adds duplicates).
"""
from __future__ import annotations

import numpy as np

from tests.transx_ref import FP32_EXACT  # noqa: F401  (2^24: below it fp32 sums of integers are exact)

TABLES = ("ent", "rel", "rel_matrix")


def _f64(tabs):
    return {k: np.asarray(v, dtype=np.float64) for k, v in tabs.items()}


def matrices(tabs, r, dim_e, dim_r):
    return tabs["rel_matrix"][r].reshape(-1, dim_r, dim_e)


def dims(tabs):
    dim_e, dim_r = tabs["ent"].shape[1], tabs["rel"].shape[1]
    assert tabs["rel_matrix"].shape[1] == dim_e * dim_r
    return dim_e, dim_r


def residual(tabs, tri):
    """u [B, dim_r] of triples (h, t, r)."""
    tabs = _f64(tabs)
    tri = np.asarray(tri, dtype=np.int64)
    dim_e, dim_r = dims(tabs)
    h, t, r = tri[:, 0], tri[:, 1], tri[:, 2]
    M = matrices(tabs, r, dim_e, dim_r)
    x = tabs["ent"][h] - tabs["ent"][t]
    return np.einsum("bkj,bj->bk", M, x) + tabs["rel"][r]


def residual_magnitude(tabs, tri):
    """|M_r| (|h| + |t|) + |r|: bounds every partial sum of u and the terms it is made of."""
    A = {k: np.abs(np.asarray(v, dtype=np.float64)) for k, v in tabs.items()}
    tri = np.asarray(tri, dtype=np.int64)
    dim_e, dim_r = dims(A)
    M = matrices(A, tri[:, 2], dim_e, dim_r)
    return np.einsum("bkj,bj->bk", M, A["ent"][tri[:, 0]] + A["ent"][tri[:, 1]]) + A["rel"][tri[:, 2]]


def score_magnitude(tabs, tri, l1=True):
    """score with every term in absolute value: bounds each partial sum of D."""
    ua = residual_magnitude(tabs, tri)
    return ua.sum(1) if l1 else (ua * ua).sum(1)


def score(tabs, tri, l1=True):
    u = residual(tabs, tri)
    return np.abs(u).sum(1) if l1 else (u * u).sum(1)


def _fgrad(u, l1):
    return np.sign(u) if l1 else 2.0 * u


def slices(tabs, pos, neg, margin, l1=True, magnitude=False):
    """(loss, {table: (rows [S], grads [S, cols])}): TF's IndexedSlices of d loss / d table, inactive pairs
    included with zero rows.  With magnitude=True every slice instead holds its gradient with each product and sum
    taken in absolute value (g bounded by 1 for L1 and 2 sum |terms of u| for L2): a bound on every partial sum of
    the slice and on the terms it is made of, whatever order a kernel adds them in."""
    tabs = _f64(tabs)
    pos, neg = np.asarray(pos, dtype=np.int64), np.asarray(neg, dtype=np.int64)
    dim_e, dim_r = dims(tabs)
    r = pos[:, 2]
    M = matrices(tabs, r, dim_e, dim_r)
    up, un = residual(tabs, pos), residual(tabs, neg)
    dp = np.abs(up).sum(1) if l1 else (up * up).sum(1)
    dn = np.abs(un).sum(1) if l1 else (un * un).sum(1)
    z = dp - dn + margin
    act = (z >= 0).astype(np.float64)[:, None]
    loss = float(np.where(z >= 0, z, 0.0).sum())
    xp = tabs["ent"][pos[:, 0]] - tabs["ent"][pos[:, 1]]
    xn = tabs["ent"][neg[:, 0]] - tabs["ent"][neg[:, 1]]
    if magnitude:
        A = {k: np.abs(v) for k, v in tabs.items()}
        Ma = np.abs(M)
        xp_a = A["ent"][pos[:, 0]] + A["ent"][pos[:, 1]]
        xn_a = A["ent"][neg[:, 0]] + A["ent"][neg[:, 1]]
        if l1:
            gp = gn = np.ones_like(up)
        else:
            gp = 2.0 * (np.einsum("bkj,bj->bk", Ma, xp_a) + A["rel"][r])
            gn = 2.0 * (np.einsum("bkj,bj->bk", Ma, xn_a) + A["rel"][r])
        gp, gn = act * gp, act * gn
        vp, vn = np.einsum("bkj,bk->bj", Ma, gp), np.einsum("bkj,bk->bj", Ma, gn)
        dM = (gp[:, :, None] * xp_a[:, None, :] + gn[:, :, None] * xn_a[:, None, :]).reshape(len(pos), -1)
        ent = np.concatenate([vp, vp, vn, vn])
        rel = np.concatenate([gp, gn])
    else:
        gp, gn = act * _fgrad(up, l1), act * _fgrad(un, l1)
        vp, vn = np.einsum("bkj,bk->bj", M, gp), np.einsum("bkj,bk->bj", M, gn)
        dM = (gp[:, :, None] * xp[:, None, :] - gn[:, :, None] * xn[:, None, :]).reshape(len(pos), -1)
        ent = np.concatenate([vp, -vp, -vn, vn])
        rel = np.concatenate([gp, -gn])
    out = {"ent": (np.concatenate([pos[:, 0], pos[:, 1], neg[:, 0], neg[:, 1]]), ent),
           "rel": (np.concatenate([r, r]), rel),
           "rel_matrix": (r, dM)}
    return loss, out


def dense(tabs, sl):
    """Sum each table's slices into a dense gradient."""
    g = {}
    for k, (rows, vals) in sl.items():
        g[k] = np.zeros(np.shape(tabs[k]), dtype=np.float64)
        np.add.at(g[k], rows, vals)
    return g


def hinge_grads(tabs, pos, neg, margin, l1=True, magnitude=False):
    """(loss, dense fp64 gradient of every table); magnitude=True: the bound of `slices`, summed per element."""
    loss, sl = slices(tabs, pos, neg, margin, l1, magnitude)
    return loss, dense(tabs, sl)


def lr_t(lr, b1, b2, t):
    """TF1's bias-corrected step size, powers from the 1-based t."""
    return lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def adam_apply(tabs, m, v, g, gsq, t, lr, b1, b2, eps):
    """Adam on every element: m, v decay everywhere; g = 0 (and gsq = 0) on untouched rows."""
    a = lr_t(lr, b1, b2, t)
    nt, nm, nv = {}, {}, {}
    for k in tabs:
        nm[k] = b1 * np.asarray(m[k], np.float64) + (1.0 - b1) * g[k]
        nv[k] = b2 * np.asarray(v[k], np.float64) + (1.0 - b2) * gsq[k]
        nt[k] = np.asarray(tabs[k], np.float64) - a * nm[k] / (np.sqrt(nv[k]) + eps)
    return nt, nm, nv


def adam_step(tabs, m, v, pos, neg, margin, t, lr=0.001, b1=0.9, b2=0.999, eps=1e-8, l1=True, dedup=True):
    """(tables, m, v, loss) after one step t (1-based) of TF1's Adam on the hinge loss."""
    loss, sl = slices(tabs, pos, neg, margin, l1)
    g = dense(tabs, sl)
    if dedup:
        gsq = {k: x * x for k, x in g.items()}
    else:
        gsq = dense(tabs, {k: (rows, vals * vals) for k, (rows, vals) in sl.items()})
    nt, nm, nv = adam_apply(tabs, m, v, g, gsq, t, lr, b1, b2, eps)
    return nt, nm, nv, loss


def zeros_like(tabs):
    return {k: np.zeros(np.shape(x), dtype=np.float64) for k, x in tabs.items()}


# ------------------------------------------------------------------------------------ fixtures
def random_tables(E, R, dim_e, dim_r, rng, scale=1.0):
    return {"ent": rng.normal(size=(E, dim_e)) * scale, "rel": rng.normal(size=(R, dim_r)) * scale,
            "rel_matrix": rng.normal(size=(R, dim_e * dim_r)) * scale}


def integer_tables(E, R, dim_e, dim_r, seed=0, amp=2, density=None):
    """Tables of small integers in [-amp, amp] (fp64 holding integers).  With `density`, each entry is kept with
    that probability and is zero otherwise (the keep draws follow the tables', so None gives the same tables as
    ever): sparser tables keep large dims inside the exact range."""
    rng = np.random.default_rng(seed)
    tabs = {"ent": rng.integers(-amp, amp + 1, size=(E, dim_e)).astype(np.float64),
            "rel": rng.integers(-amp, amp + 1, size=(R, dim_r)).astype(np.float64),
            "rel_matrix": rng.integers(-amp, amp + 1, size=(R, dim_e * dim_r)).astype(np.float64)}
    if density is not None:
        for k, x in tabs.items():
            tabs[k] = np.where(rng.random(x.shape) < density, x, 0.0)
    return tabs


def skewed_batch(rng, E, R, B, s=1.1, hot=None):
    """(pos, neg) int32 [B,3] with a Zipf-like relation column (relation k drawn with weight 1/(k+1)^s; `hot` puts
    every pair on that relation); each negative replaces the head or the tail and keeps the relation."""
    if hot is None:
        w = 1.0 / np.arange(1, R + 1) ** s
        r = rng.choice(R, size=B, p=w / w.sum())
    else:
        r = np.full(B, hot)
    pos = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), r], 1).astype(np.int32)
    neg = pos.copy()
    side = rng.integers(0, 2, B)
    neg[np.arange(B), side] = rng.integers(0, E, B)
    return pos, neg


def exact_step_bound(tabs, pos, neg, margin, l1=True):
    """For integer tables and an integer margin: the largest magnitude any partial sum of one step's forward and
    gradient can reach in any summation order (X = h - t, u, D, z, the loss, g, M^T g, the dM, drel and entity
    row sums).  Below 2^24 fp32 computes all of them exactly, so a kernel's loss and gradient (m = g (1 - b1) with
    b1 = 1/2) must equal the fp64 ones bitwise.  Raises ValueError for a fixture not of this form."""
    tabs = _f64(tabs)
    if not all(np.array_equal(x, np.round(x)) for x in tabs.values()) or margin != round(margin):
        raise ValueError("tables and margin must hold integers")
    pos, neg = np.asarray(pos, dtype=np.int64), np.asarray(neg, dtype=np.int64)
    E, R = len(tabs["ent"]), len(tabs["rel"])
    if (min(pos[:, :2].min(), neg[:, :2].min()) < 0 or max(pos[:, :2].max(), neg[:, :2].max()) >= E
            or pos[:, 2].min() < 0 or pos[:, 2].max() >= R or not np.array_equal(pos[:, 2], neg[:, 2])):
        raise ValueError("every pair must be valid")
    dim_e, dim_r = dims(tabs)
    A = {k: np.abs(x) for k, x in tabs.items()}
    Ma = matrices(A, pos[:, 2], dim_e, dim_r)
    worst, dist = 0.0, []
    for trip in (pos, neg):
        xa = A["ent"][trip[:, 0]] + A["ent"][trip[:, 1]]
        ua = np.einsum("bkj,bj->bk", Ma, xa) + A["rel"][trip[:, 2]]
        worst = max(worst, xa.max(), ua.max())
        D = score(tabs, trip, l1)
        worst = max(worst, (ua.sum(1) if l1 else (ua * ua).sum(1)).max())
        dist.append(D)
    z = dist[0] - dist[1] + margin
    worst = max(worst, (np.abs(dist[0]) + np.abs(dist[1]) + abs(margin)).max(), np.abs(z).sum())
    _, mag = hinge_grads(tabs, pos, neg, margin, l1, magnitude=True)
    _, sl = slices(tabs, pos, neg, margin, l1, magnitude=True)
    worst = max(worst, max(x.max() for x in mag.values()), max(vals.max() for _, vals in sl.values()))
    return float(worst)


def is_exact_step(tabs, pos, neg, margin, l1=True):
    try:
        return exact_step_bound(tabs, pos, neg, margin, l1) < FP32_EXACT
    except ValueError:
        return False
