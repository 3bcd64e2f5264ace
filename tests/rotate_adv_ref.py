"""NumPy restatement of RotatE's self-adversarial negative-sampling loss (include/ge_hip.h's ge_rotate_adv_*) on top of
tests/rotate_ref.py, for the tests (product code never imports it).  fp64 by default; with dtype=np.float32 the same
statements run in fp32, which is how the GPU tests size their tolerances.

A batch: pos [B,3] (h, t, r), side [B] (0: the tail is replaced, 1: the head), neg_ent [B,K].  Negative j of row i is
(h, neg_ent[i,j], r) or (neg_ent[i,j], t, r); a slot outside [0, E) is empty; a row with a positive id out of range or a
side outside {0, 1} is invalid (loss NaN here, 0 in the batch sum, no gradient).
  p_ij   = softmax_j(-alpha D-_ij) over the live slots, not differentiated
  loss_i = softplus(D+_i - gamma) + sum_j p_ij softplus(gamma - D-_ij)
`form`: "tail" evaluates every distance as |h e^{i theta} - t| (rotate_ref.dist), "head" as |h - t e^{-i theta}|
(rotate_ref.dist_head_form, what the kernel evaluates where heads are replaced).  In fp64 the two agree to rounding; in
fp32 the tests take the form that deviates more.
"""
from __future__ import annotations

import numpy as np

from oracle.transx_oracle import TAG_BSIDE, BernoulliIndex, _skip_known, philox4x32_10  # noqa: F401
from tests import rotate_ref as RR
from tests import transx_ref as XR

TAG_ADVPICK = 0x61647670  # 'advp'


def softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def valid_rows(pos, side, E, R):
    pos, side = np.asarray(pos, dtype=np.int64), np.asarray(side, dtype=np.int64)
    return ((pos[:, 0] >= 0) & (pos[:, 0] < E) & (pos[:, 1] >= 0) & (pos[:, 1] < E) & (pos[:, 2] >= 0) & (pos[:, 2] < R)
            & ((side == 0) | (side == 1)))


def _negatives(pos, side, neg_ent, E, R):
    """(valid [B], live [B,K], pos' [B,3], neg triples [B,K,3]) with every id of an invalid row or an empty slot set to 0."""
    pos, side, neg_ent = (np.asarray(x, dtype=np.int64) for x in (pos, side, neg_ent))
    valid = valid_rows(pos, side, E, R)
    live = valid[:, None] & (neg_ent >= 0) & (neg_ent < E)
    p = np.where(valid[:, None], pos, 0)
    c = np.where(live, neg_ent, 0)
    tails = (side == 0)[:, None]
    neg = np.stack([np.where(tails, p[:, :1], c), np.where(tails, c, p[:, 1:2]), np.broadcast_to(p[:, 2:3], c.shape)], 2)
    return valid, live, p, neg


def _dist(tabs, tri, l1, form):
    return (RR.dist_head_form if form == "head" else RR.dist)(tabs, tri, l1, tabs["ent"].dtype)


def parts(tabs, pos, side, neg_ent, margin, alpha, l1=True, dtype=np.float64, form="tail"):
    """Everything the loss is made of: dict(valid [B], live [B,K], Dp [B], Dn [B,K], p [B,K], loss [B] (NaN: invalid),
    pos [B,3], neg [B,K,3]) in `dtype`."""
    tabs = RR._cast(tabs, dtype)
    E, R = len(tabs["ent"]), len(tabs["rel"])
    valid, live, p3, neg = _negatives(pos, side, neg_ent, E, R)
    B, K = live.shape
    gamma, alpha = np.asarray(margin, dtype=dtype), np.asarray(alpha, dtype=dtype)
    Dp = _dist(tabs, p3, l1, form)
    Dn = _dist(tabs, neg.reshape(-1, 3), l1, form).reshape(B, K)
    z = np.where(live, -alpha * Dn, -np.inf).astype(dtype)
    mx = np.where(live.any(1), z.max(1, initial=-np.inf), 0).astype(dtype)
    e = np.where(live, np.exp(np.where(live, z - mx[:, None], 0)), 0).astype(dtype)
    s = e.sum(1)
    p = (e / np.where(s > 0, s, 1)[:, None]).astype(dtype)
    loss = softplus(Dp - gamma) + (p * softplus(gamma - Dn)).sum(1)
    loss = np.where(valid, loss, np.nan).astype(dtype)
    return dict(valid=valid, live=live, Dp=Dp, Dn=Dn, p=p, loss=loss, pos=p3, neg=neg)


def row_losses(tabs, pos, side, neg_ent, margin, alpha, l1=True, dtype=np.float64, form="tail"):
    """loss_i [B]; NaN for an invalid row."""
    return parts(tabs, pos, side, neg_ent, margin, alpha, l1, dtype, form)["loss"]


def _triple_grads(tabs, tri, l1, form):
    """Per-row (d/d ent[h] [n,d], d/d ent[t] [n,d], d/d rel[r] [n,k]) of D in the form's arithmetic."""
    if form != "head":
        return RR.triple_grads(tabs, tri, l1)
    ent, th = tabs["ent"], tabs["rel"][tri[:, 2]]
    k = ent.shape[1] // 2
    c, s = np.cos(th), np.sin(th)
    h, t = tri[:, 0], tri[:, 1]
    qre, qim = ent[t, :k] * c + ent[t, k:] * s, ent[t, k:] * c - ent[t, :k] * s
    gre, gim = RR._dist_grad(ent[h, :k] - qre, ent[h, k:] - qim, l1)          # dD/dv, v = h - q
    gh = np.concatenate([gre, gim], 1)
    gt = np.concatenate([-(gre * c - gim * s), -(gre * s + gim * c)], 1)      # -g e^{i theta}
    return gh, gt, gim * qre - gre * qim


def grads(tabs, pos, side, neg_ent, margin, alpha, l1=True, dtype=np.float64, form="tail"):
    """(batch loss, {"ent": [E,d], "rel": [R,k]} summed gradients, named {"ent": bool [E], "rel": bool [R]})."""
    P = parts(tabs, pos, side, neg_ent, margin, alpha, l1, dtype, form)
    tabs = RR._cast(tabs, dtype)
    gamma = np.asarray(margin, dtype=dtype)
    valid, live = P["valid"], P["live"]
    B, K = live.shape
    a_pos = np.where(valid, sigmoid(P["Dp"] - gamma), 0).astype(dtype)
    a_neg = np.where(live, -P["p"] * sigmoid(gamma - P["Dn"]), 0).astype(dtype)
    out = {k: np.zeros_like(v) for k, v in tabs.items()}
    named = {k: np.zeros(len(v), dtype=bool) for k, v in tabs.items()}
    for tri, a, on in ((P["pos"], a_pos, valid), (P["neg"].reshape(-1, 3), a_neg.reshape(-1), live.reshape(-1))):
        gh, gt, gr = _triple_grads(tabs, tri, l1, form)
        a = a[:, None]
        np.add.at(out["ent"], tri[:, 0], (a * gh).astype(dtype))
        np.add.at(out["ent"], tri[:, 1], (a * gt).astype(dtype))
        np.add.at(out["rel"], tri[:, 2], (a * gr).astype(dtype))
        named["ent"][tri[on, 0]] = True
        named["ent"][tri[on, 1]] = True
        named["rel"][tri[on, 2]] = True
    loss = float(np.where(valid, P["loss"], 0).astype(dtype).sum())
    return loss, out, named


def named_rows(tabs, pos, side, neg_ent):
    """{"ent": bool [E], "rel": bool [R]}: the rows a valid row names (its positive, its live slots, its relation)."""
    E, R = len(tabs["ent"]), len(tabs["rel"])
    valid, live, p3, neg = _negatives(pos, side, neg_ent, E, R)
    out = {"ent": np.zeros(E, dtype=bool), "rel": np.zeros(R, dtype=bool)}
    out["ent"][p3[valid, 0]] = True
    out["ent"][p3[valid, 1]] = True
    out["ent"][np.asarray(neg_ent, dtype=np.int64)[live]] = True
    out["rel"][p3[valid, 2]] = True
    return out


def sgd_step(tabs, pos, side, neg_ent, lr, margin, alpha, l1=True, dtype=np.float64, form="tail"):
    """(new tables, loss): every gradient on the pre-step tables, duplicates summed, row -= lr * sum."""
    loss, g, _ = grads(tabs, pos, side, neg_ent, margin, alpha, l1, dtype, form)
    lr = np.asarray(lr, dtype=dtype)
    return {k: np.asarray(v, dtype=dtype) - lr * g[k] for k, v in tabs.items()}, loss


def adagrad_step(tabs, accs, pos, side, neg_ent, lr, margin, alpha, l1=True, dtype=np.float64, form="tail"):
    """(new tables, new accumulators, loss): per named row acc += s * s, row -= lr * s / sqrt(acc); others as they were."""
    loss, g, named = grads(tabs, pos, side, neg_ent, margin, alpha, l1, dtype, form)
    lr = np.asarray(lr, dtype=dtype)
    new_t, new_a = {}, {}
    for k, v in tabs.items():
        v, a, s = np.asarray(v, dtype=dtype), np.asarray(accs[k], dtype=dtype), g[k]
        acc = a + s * s
        upd = v - lr * s / np.sqrt(acc)
        rows = named[k][:, None]
        new_a[k], new_t[k] = np.where(rows, acc, a), np.where(rows, upd, v)
    return new_t, new_a, loss


def largest_dist(tabs, pos, side, neg_ent, l1=True):
    """The largest distance a row's loss is formed from (rotate_ref.bound's `scale`)."""
    P = parts(tabs, pos, side, neg_ent, 0.0, 0.0, l1)
    vals = np.concatenate([P["Dp"][P["valid"]], P["Dn"][P["live"]]])
    return float(vals.max()) if vals.size else 0.0


def worse32(ref64, a32, b32):
    """Of two float32 evaluations, the one that deviates more from ref64 (the larger e32)."""
    r = np.asarray(ref64, dtype=np.float64)
    ea, eb = np.abs(np.asarray(a32, dtype=np.float64) - r), np.abs(np.asarray(b32, dtype=np.float64) - r)
    return a32 if np.nanmax(ea, initial=0.0) >= np.nanmax(eb, initial=0.0) else b32


# ------------------------------------------------------------------------------------------------ the draw
def draw(triples, index: BernoulliIndex, seed: int, step: int, B: int, K: int):
    """(pos [B,3], side [B], neg_ent [B,K]) int32 of ge_rotate_adv_draw_batch: row i's positive and side are
    ge_transx_draw_batch's of (seed, step, i); negative j is the entity the Philox word at row index i K + j under
    TAG_ADVPICK draws among those that are not known completions of (fixed entity, r); -1 where none is free."""
    tri = np.asarray(triples, dtype=np.int32)
    pos = tri[XR.draw_positive_rows(len(tri), B, seed, step)]
    s_lo, s_hi = step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF
    k_lo, k_hi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    rows = np.arange(B, dtype=np.uint64)
    w_side = philox4x32_10(s_lo, s_hi, rows & 0xFFFFFFFF, rows >> 32, k_lo ^ TAG_BSIDE, k_hi)[0]
    cells = np.arange(B * K, dtype=np.uint64)
    w_pick = philox4x32_10(s_lo, s_hi, cells & 0xFFFFFFFF, cells >> 32, k_lo ^ TAG_ADVPICK, k_hi)[0].reshape(B, K)
    side = np.zeros(B, dtype=np.int32)
    neg_ent = np.full((B, K), -1, dtype=np.int32)
    for i in range(B):
        h, t, r = (int(v) for v in pos[i])
        if not 0 <= r < index.n_rel:
            continue
        tail_side = int(w_side[i]) < int(index.tail_threshold[r])
        side[i] = 0 if tail_side else 1
        key_arr, ent_arr, key = (index.bh_key, index.bh_ent, h * index.n_rel + r) if tail_side else \
            (index.bt_key, index.bt_ent, t * index.n_rel + r)
        ll = int(np.searchsorted(key_arr, key, side="left"))
        rr = int(np.searchsorted(key_arr, key, side="right")) - 1
        cnt = max(rr - ll + 1, 0)
        free = index.n_ent - cnt
        if free <= 0:
            continue
        known = ent_arr.astype(np.int64) - index.ent_lo
        for j in range(K):
            tmp = (int(w_pick[i, j]) * free) >> 32
            neg_ent[i, j] = index.ent_lo + (tmp if cnt == 0 else _skip_known(known, ll, rr, tmp))
    return pos, side, neg_ent
