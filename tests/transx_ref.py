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


def _fgrad_bound(model, tabs, h, t, r, l1):
    """|f(u)| bounded by the terms of u = h_p + r - t_p: 1 for L1, 2 sum |term| for L2."""
    A = {k: np.abs(v) for k, v in tabs.items()}
    if l1:
        return np.ones_like(A["ent"][h])
    terms = A["ent"][h] + A["rel"][r] + A["ent"][t]
    if model != "transe":
        x = A["normal_vector"][r] if model == "transh" else A["rel_transfer"][r]
        if model == "transh":
            x = x / np.sqrt(np.maximum((tabs["normal_vector"][r] ** 2).sum(1, keepdims=True), EPS))
            a, b = (A["ent"][h] * x).sum(1, keepdims=True), (A["ent"][t] * x).sum(1, keepdims=True)
        else:
            a = (A["ent"][h] * A["ent_transfer"][h]).sum(1, keepdims=True)
            b = (A["ent"][t] * A["ent_transfer"][t]).sum(1, keepdims=True)
        terms = terms + (a + b) * x
    return 2.0 * terms


def _triple_grad_bounds(model, tabs, h, t, r, g):
    """_triple_grads with every product and sum taken in absolute value: each slot's gradient is bounded by its
    terms, not by what is left after they cancel."""
    A = {k: np.abs(v) for k, v in tabs.items()}
    g = np.abs(g)
    eh, et = A["ent"][h], A["ent"][t]
    if model == "transe":
        return {"rel": g, "ent_h": g, "ent_t": g}
    if model == "transh":
        n = A["normal_vector"][r]
        nn = (n * n).sum(1, keepdims=True)
        inv = 1.0 / np.sqrt(np.maximum(nn, EPS))
        nh = n * inv
        c = (g * nh).sum(1, keepdims=True)
        a, b = (eh * nh).sum(1, keepdims=True), (et * nh).sum(1, keepdims=True)
        gnh = c * (eh + et) + (a + b) * g
        branch = (nn >= EPS).astype(np.float64)
        return {"rel": g, "ent_h": g + c * nh, "ent_t": g + c * nh,
                "normal_vector": inv * gnh + branch * inv ** 3 * (gnh * n).sum(1, keepdims=True) * n}
    hp, tp, rp = A["ent_transfer"][h], A["ent_transfer"][t], A["rel_transfer"][r]
    c = (g * rp).sum(1, keepdims=True)
    a, b = (eh * hp).sum(1, keepdims=True), (et * tp).sum(1, keepdims=True)
    return {"rel": g, "ent_h": g + c * hp, "ent_t": g + c * tp, "ent_transfer_h": c * eh, "ent_transfer_t": c * et,
            "rel_transfer": (a + b) * g}


def hinge_grads(model, tabs, pos, neg, margin, l1=True, magnitude=False):
    """(loss, dense fp64 gradient of every table) of sum_i max(D(pos_i) - D(neg_i) + margin, 0).  With
    magnitude=True the tables hold instead the sum over the slots that reach each element of the slot's gradient
    with every product and sum in absolute value: a bound on every partial sum of that element's gradient and on
    the terms each slot is made of, whatever order a kernel adds them in."""
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
        g = sgn * active * (_fgrad_bound(model, tabs, h, t, r, l1) if magnitude else _fgrad(u, l1))
        parts = (_triple_grad_bounds if magnitude else _triple_grads)(model, tabs, h, t, r, g)
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


# ------------------------------------------------------------------------------------ the step's slot layout
KWIN = 32                       # sorted slots per wave in the apply's first pass (kWin in ge_transx.hip)


def slot_keys(pos, neg, E, R, active):
    """The step's gradient slots as include/ge_hip.h and ge_transx.hip's header state them: slots 4i..4i+3 take
    pos h, pos t, neg h, neg t (key = entity id), slot 4B+i takes key E + r, and every slot of an inactive pair
    takes the sentinel E + R.  Returns (keys [5B] unsorted, the stably sorted keys)."""
    pos, neg = np.asarray(pos, dtype=np.int64), np.asarray(neg, dtype=np.int64)
    active = np.asarray(active, dtype=bool)
    B = len(pos)
    keys = np.empty(5 * B, dtype=np.int64)
    for s, col in enumerate((pos[:, 0], pos[:, 1], neg[:, 0], neg[:, 1])):
        keys[s:4 * B:4] = col
    keys[4 * B:] = E + pos[:, 2]
    keys[np.concatenate([np.repeat(~active, 4), ~active])] = E + R
    return keys, keys[np.argsort(keys, kind="stable")]


def run_of(sorted_keys, key):
    """(start, length) of the run of `key` in the sorted keys; (start // KWIN, last // KWIN) are its windows."""
    idx = np.flatnonzero(np.asarray(sorted_keys) == key)
    assert len(idx) and idx[-1] - idx[0] + 1 == len(idx), key
    return int(idx[0]), len(idx)


# ------------------------------------------------------------------------------------ exact-arithmetic fixtures
FP32_EXACT = 2.0 ** 24


def exact_tables(model, E, R, d, seed=0, amp=2):
    """Tables of small integers in [-amp, amp] (fp64 holding integers)."""
    rng = np.random.default_rng(seed)
    rows = {"ent": E, "rel": R, "normal_vector": R, "ent_transfer": E, "rel_transfer": R}
    return {k: rng.integers(-amp, amp + 1, size=(rows[k], d)).astype(np.float64) for k in ("ent", "rel") + EXTRA[model]}


def fixture_tables(model, E, R, d, seed=0):
    """exact_tables for TransE / TransD.  TransH has no exact fixture, and on integer tables its projection leaves
    L1 components that are 0 in fp64 but +-1 ulp in fp32, where sign() takes either value: it gets fp32-held normal
    values instead."""
    if model != "transh":
        return exact_tables(model, E, R, d, seed)
    rng = np.random.default_rng(seed)
    rows = {"ent": E, "rel": R, "normal_vector": R}
    return {k: rng.normal(size=(n, d)).astype(np.float32).astype(np.float64) for k, n in rows.items()}


def exact_step_bound(model, tabs, pos, neg, lr, margin, l1=True):
    """For integer tables, an integer margin and lr = 2^-k: the largest magnitude any partial sum of one step can
    reach in any summation order, counted on the value's own grid (1 for distances, dots and gradient rows; lr for
    the updated tables).  Below 2^24 fp32 computes every one of them exactly, so a kernel's loss and tables must
    equal sgd_step's bitwise.  TransE and TransD only: TransH goes through rsqrt.  Raises ValueError for a
    fixture not of this form."""
    if model not in ("transe", "transd"):
        raise ValueError(f"{model}: no exact fixture (l2_normalize takes a square root)")
    tabs = {k: np.asarray(v, dtype=np.float64) for k, v in tabs.items()}
    if not all(np.array_equal(v, np.round(v)) for v in tabs.values()) or margin != round(margin):
        raise ValueError("tables and margin must hold integers")
    if not lr > 0 or np.frexp(lr)[0] != 0.5:
        raise ValueError(f"lr={lr} is not a power of two")
    pos, neg = np.asarray(pos, dtype=np.int64), np.asarray(neg, dtype=np.int64)
    E, R = len(tabs["ent"]), len(tabs["rel"])
    if (pos[:, :2].min() < 0 or neg[:, :2].min() < 0 or max(pos[:, :2].max(), neg[:, :2].max()) >= E
            or pos[:, 2].min() < 0 or pos[:, 2].max() >= R or not np.array_equal(pos[:, 2], neg[:, 2])):
        raise ValueError("every pair must be valid")
    worst, dist = 0.0, []
    for trip in (pos, neg):
        h, t, r = trip[:, 0], trip[:, 1], trip[:, 2]
        eh, et, rr = tabs["ent"][h], tabs["ent"][t], tabs["rel"][r]
        terms = [eh, rr, et]
        if model == "transd":
            hp, tp, rp = tabs["ent_transfer"][h], tabs["ent_transfer"][t], tabs["rel_transfer"][r]
            a, b = (eh * hp).sum(1, keepdims=True), (et * tp).sum(1, keepdims=True)
            worst = max(worst, np.abs(eh * hp).sum(1).max(), np.abs(et * tp).sum(1).max())
            terms += [a * rp, b * rp]
        worst = max(worst, sum(np.abs(x) for x in terms).max())                      # u = h_p + r - t_p
        u = _proj(model, tabs, h, r) + rr - _proj(model, tabs, t, r)
        f = _fgrad(u, l1)
        dist.append(np.abs(u).sum(1) if l1 else (u * u).sum(1))
        worst = max(worst, dist[-1].max())
        if model == "transd":
            c = (f * rp).sum(1, keepdims=True)
            worst = max(worst, np.abs(f * rp).sum(1).max())
            for row in (np.abs(f) + np.abs(c * hp), np.abs(f) + np.abs(c * tp), np.abs(c * eh), np.abs(c * et),
                        (np.abs(a) + np.abs(b)) * np.abs(f)):
                worst = max(worst, row.max())
    z = dist[0] - dist[1] + margin
    worst = max(worst, (dist[0] + dist[1] + abs(margin)).max(), np.abs(z).sum())    # z, and the loss's sum
    _, mag = hinge_grads(model, tabs, pos, neg, margin, l1, magnitude=True)
    for k, v in tabs.items():
        worst = max(worst, mag[k].max(), (np.abs(v) / lr + mag[k]).max())            # row - lr * sum, in units of lr
    return float(worst)


def is_exact_step(model, tabs, pos, neg, lr, margin, l1=True):
    try:
        return exact_step_bound(model, tabs, pos, neg, lr, margin, l1) < FP32_EXACT
    except ValueError:
        return False


# Batches that place a run of the sorted slots where the apply's windows cut it.  Relation run r starts at
# 4 A + (active pairs with relation < r), A = active pairs: every entity key sorts before every relation key.
# counts[r] = active pairs with relation r; `inactive` pairs (neg == pos under margin -1) add sentinel slots;
# `hot` = slots of entities 0, 1, ... .  `expect` = (("rel" | "ent", id), start, length) of the runs meant.
LAYOUTS = {
    # relation 1 fills window 5, [160, 192), exactly
    "run32_on_boundary": dict(counts=(4, 32, 3), expect=((("rel", 1), 160, 32),)),
    # relation 1 is [160, 193): window 5 and one slot of window 6
    "run33": dict(counts=(4, 33, 2), expect=((("rel", 1), 160, 33),)),
    # relation 1 is [63, 65): the last slot of window 1 and the first of window 2
    "straddle2": dict(counts=(3, 2, 10), expect=((("rel", 1), 63, 2),)),
    # relation 1 is [421, 521): windows 13 to 16
    "four_windows": dict(counts=(1, 100, 4), expect=((("rel", 1), 421, 100),)),
    # relations 1 [330, 370) and 2 [370, 410) are both cut and meet inside window 11; relation 2 ends at the last slot
    "two_cuts_meet": dict(counts=(2, 40, 40), expect=((("rel", 1), 330, 40), (("rel", 2), 370, 40))),
    # relation 1 is [95, 115), cut between windows 2 and 3, and the 50 sentinel slots of 10 inactive pairs follow
    "cut_before_sentinel": dict(counts=(3, 20), inactive=10, expect=((("rel", 1), 95, 20),)),
    # entities 0 [0, 45) and 1 [45, 85) are both cut and meet inside window 1 (TransD: the ent_transfer plane)
    "hot_entities": dict(counts=(10, 12, 8), hot=(45, 40), expect=((("ent", 0), 0, 45), (("ent", 1), 45, 40))),
}
LAYOUT_E = 50


def _ordered_pair(model, tabs, rng, r, E, lo, l1):
    """A (pos, neg) pair of relation r with D(pos) - D(neg) >= 1.  Integer tables make the difference an integer
    for TransE / TransD; TransH's is not, so it keeps 0.01 of room for fp32 rounding."""
    need = 1.01 if model == "transh" else 1.0
    while True:
        p = np.array([[rng.integers(lo, E), rng.integers(lo, E), r]])
        n = np.array([[rng.integers(lo, E), rng.integers(lo, E), r]])
        dp, dn = score(model, tabs, p, l1)[0], score(model, tabs, n, l1)[0]
        if abs(dp - dn) >= need:
            return (p[0], n[0]) if dp > dn else (n[0], p[0])


def layout_batch(model, name, d, l1=True, seed=0):
    """One of LAYOUTS on fixture_tables: dict(tabs, pos, neg, lr, margin, E, R, expect=((key, start, length), ...)).
    With no inactive pairs the margin is the least integer that makes every pair active (z >= 1); with inactive
    pairs it is -1, they have neg == pos (z = -1) and the active ones D+ - D- >= 1 (z >= 0)."""
    spec = LAYOUTS[name]
    counts, inactive, hot = spec["counts"], spec.get("inactive", 0), spec.get("hot", ())
    E, R = LAYOUT_E, len(counts)
    rng = np.random.default_rng(seed)
    tabs = fixture_tables(model, E, R, d, seed=seed + 1)
    rel = np.repeat(np.arange(R), counts)
    A = len(rel)
    lo = len(hot)                                  # the hot entities appear only where `hot` puts them
    if inactive:
        pairs = [_ordered_pair(model, tabs, rng, r, E, lo, l1) for r in rel]
        pos, neg = np.array([p for p, _ in pairs]), np.array([n for _, n in pairs])
        idle = np.stack([rng.integers(lo, E, inactive), rng.integers(lo, E, inactive), rng.integers(0, R, inactive)], 1)
        pos, neg = np.concatenate([pos, idle]), np.concatenate([neg, idle])
        margin = -1.0
    else:
        ents = rng.integers(lo, E, 4 * A)
        at = rng.permutation(4 * A)
        k = 0
        for e, c in enumerate(hot):
            ents[at[k:k + c]] = e
            k += c
        ents = ents.reshape(A, 4)
        pos = np.stack([ents[:, 0], ents[:, 1], rel], 1)
        neg = np.stack([ents[:, 2], ents[:, 3], rel], 1)
        margin = float(score(model, tabs, neg, l1).max() - score(model, tabs, pos, l1).min() + 1)
    order = rng.permutation(len(pos))              # interleave relations and inactive pairs in slot order
    pos, neg = pos[order].astype(np.int32), neg[order].astype(np.int32)
    expect = tuple(((key if kind == "ent" else E + key), s, n) for (kind, key), s, n in spec["expect"])
    return dict(tabs=tabs, pos=pos, neg=neg, lr=2.0 ** -6, margin=margin, E=E, R=R, expect=expect)


def active_mask(model, tabs, pos, neg, margin, l1=True):
    return score(model, tabs, pos, l1) - score(model, tabs, neg, l1) + margin >= 0
