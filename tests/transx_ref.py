"""fp64 restatement of transE.py / transH.py / transD.py for the tests (product code never imports it).

Forward (projection, distance), the hinge loss, its gradient with TF1's rules written out by hand (a pair is active
iff D+ - D- + margin >= 0, as MaximumGrad sends ties to x; d|x|/dx = sign(x) with sign(0) = 0; l2_normalize's
max(n.n, 1e-12) differentiated on the branch it takes, ties to n.n), the dedup-sum SGD step
(tf.train.GradientDescentOptimizer on IndexedSlices: duplicates summed, row -= lr * sum, every gradient on the
pre-step tables), and the native loop's positive draw.
"""
from __future__ import annotations

import numpy as np

from oracle.hole_oracle import philox4x32_10

EPS = 1e-12
TAG_TXDRAW = 0x74786472
EXTRA = {"transe": (), "transh": ("normal_vector",), "transd": ("ent_transfer", "rel_transfer")}


def _proj(model, tabs, e_id, r_id):
    """(projected rows [B,d], aux) for entity ids e_id under relations r_id."""
    e = tabs["ent"][e_id]
    if model == "transe":
        return e
    if model == "transh":
        n = tabs["normal_vector"][r_id]
        nh = n / np.sqrt(np.maximum((n * n).sum(1, keepdims=True), EPS))
        return e - (e * nh).sum(1, keepdims=True) * nh
    ep, rp = tabs["ent_transfer"][e_id], tabs["rel_transfer"][r_id]
    return e + (e * ep).sum(1, keepdims=True) * rp


def score(model, tabs, tri, l1=True):
    tri = np.asarray(tri, dtype=np.int64)
    tabs = {k: np.asarray(v, dtype=np.float64) for k, v in tabs.items()}
    h, t, r = tri[:, 0], tri[:, 1], tri[:, 2]
    u = _proj(model, tabs, h, r) + tabs["rel"][r] - _proj(model, tabs, t, r)
    return np.abs(u).sum(1) if l1 else (u * u).sum(1)


def _fgrad(u, l1):
    return np.sign(u) if l1 else 2.0 * u


def _triple_grads(model, tabs, h, t, r, g):
    """Backward of D for triples (h, t, r) given dL/du = g [B,d]: per-row gradients of every table."""
    out = {}
    eh, et = tabs["ent"][h], tabs["ent"][t]
    out["rel"] = g
    if model == "transe":
        out["ent_h"], out["ent_t"] = g, -g
        return out
    if model == "transh":
        n = tabs["normal_vector"][r]
        nn = (n * n).sum(1, keepdims=True)
        inv = 1.0 / np.sqrt(np.maximum(nn, EPS))
        nh = n * inv
        c = (g * nh).sum(1, keepdims=True)
        a, b = (eh * nh).sum(1, keepdims=True), (et * nh).sum(1, keepdims=True)
        out["ent_h"], out["ent_t"] = g - c * nh, -(g - c * nh)
        gnh = -c * (eh - et) - (a - b) * g
        # n^ = n * s, s = (max(nn, eps))^-1/2: dn = s gnh + (gnh.n) ds/dnn 2n, ds/dnn = -s^3/2 on the nn branch
        branch = (nn >= EPS).astype(np.float64)
        out["normal_vector"] = inv * gnh - branch * inv ** 3 * (gnh * n).sum(1, keepdims=True) * n
        return out
    hp, tp, rp = tabs["ent_transfer"][h], tabs["ent_transfer"][t], tabs["rel_transfer"][r]
    c = (g * rp).sum(1, keepdims=True)
    a, b = (eh * hp).sum(1, keepdims=True), (et * tp).sum(1, keepdims=True)
    out["ent_h"], out["ent_t"] = g + c * hp, -(g + c * tp)
    out["ent_transfer_h"], out["ent_transfer_t"] = c * eh, -c * et
    out["rel_transfer"] = (a - b) * g
    return out


def hinge_grads(model, tabs, pos, neg, margin, l1=True):
    """(loss, dense fp64 gradient of every table) of sum_i max(D(pos_i) - D(neg_i) + margin, 0)."""
    tabs = {k: np.asarray(v, dtype=np.float64) for k, v in tabs.items()}
    pos, neg = np.asarray(pos, dtype=np.int64), np.asarray(neg, dtype=np.int64)
    grads = {k: np.zeros_like(v) for k, v in tabs.items()}
    loss = 0.0
    for trip, sgn in ((pos, 1.0), (neg, -1.0)):
        h, t, r = trip[:, 0], trip[:, 1], trip[:, 2]
        u = _proj(model, tabs, h, r) + tabs["rel"][r] - _proj(model, tabs, t, r)
        if sgn > 0:
            dp = np.abs(u).sum(1) if l1 else (u * u).sum(1)
            up = u
        else:
            dn = np.abs(u).sum(1) if l1 else (u * u).sum(1)
    z = dp - dn + margin
    active = (z >= 0).astype(np.float64)[:, None]
    loss = float(np.where(z >= 0, z, 0.0).sum())
    for trip, sgn in ((pos, 1.0), (neg, -1.0)):
        h, t, r = trip[:, 0], trip[:, 1], trip[:, 2]
        u = _proj(model, tabs, h, r) + tabs["rel"][r] - _proj(model, tabs, t, r)
        g = sgn * active * _fgrad(u, l1)
        parts = _triple_grads(model, tabs, h, t, r, g)
        np.add.at(grads["ent"], h, parts["ent_h"])
        np.add.at(grads["ent"], t, parts["ent_t"])
        np.add.at(grads["rel"], r, parts["rel"])
        if model == "transh":
            np.add.at(grads["normal_vector"], r, parts["normal_vector"])
        if model == "transd":
            np.add.at(grads["ent_transfer"], h, parts["ent_transfer_h"])
            np.add.at(grads["ent_transfer"], t, parts["ent_transfer_t"])
            np.add.at(grads["rel_transfer"], r, parts["rel_transfer"])
    return loss, grads


def sgd_step(model, tabs, pos, neg, lr, margin, l1=True):
    """(new tables fp64, loss): every gradient on the pre-step tables, duplicates summed, row -= lr * sum."""
    loss, grads = hinge_grads(model, tabs, pos, neg, margin, l1)
    return {k: np.asarray(v, dtype=np.float64) - lr * grads[k] for k, v in tabs.items()}, loss


def draw_positive_rows(T, B, seed, step):
    """Rows of the triple list the native loop draws at (seed, step): (w * T) >> 32 of a Philox word per row."""
    rows = np.arange(B, dtype=np.uint64)
    w = philox4x32_10(step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF, rows & np.uint64(0xFFFFFFFF), rows >> np.uint64(32),
                      (seed & 0xFFFFFFFF) ^ TAG_TXDRAW, (seed >> 32) & 0xFFFFFFFF)[0]
    return ((w.astype(np.uint64) * np.uint64(T)) >> np.uint64(32)).astype(np.int64)


def planted_kg(n_ent=2000, n_rel=20, dim=16, n_triples=20000, noise=0.05, seed=0):
    """A translational KG with no download: entities and relations are random points, and each triple's tail is
    the entity nearest to h + r (+ noise).  Returns (triples [T,3] (h, t, r) int64, unique)."""
    rng = np.random.default_rng(seed)
    ent = rng.normal(size=(n_ent, dim))
    rel = rng.normal(size=(n_rel, dim)) * 0.5
    h = rng.integers(0, n_ent, n_triples)
    r = rng.integers(0, n_rel, n_triples)
    q = ent[h] + rel[r] + noise * rng.normal(size=(n_triples, dim))
    # nearest entity to h + r, blockwise (n_triples x n_ent distances)
    t = np.empty(n_triples, dtype=np.int64)
    sq = (ent * ent).sum(1)
    for s in range(0, n_triples, 2048):
        blk = q[s:s + 2048]
        d2 = sq[None, :] - 2.0 * blk @ ent.T
        d2[np.arange(len(blk)), h[s:s + 2048]] = np.inf    # no self loops
        t[s:s + 2048] = d2.argmin(1)
    tri = np.unique(np.stack([h, t, r], 1), axis=0)
    rng.shuffle(tri)
    return tri
