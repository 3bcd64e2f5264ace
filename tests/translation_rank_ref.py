"""fp64 restatement of the translation models' link-prediction ranks (ge_transx_rank / ge_transr_rank).

For test row (h, t, r) every entity c replaces the tail (side "tail": D_c = D(h, c, r)) or the head (D_c = D(c, t, r));
the order is ascending by (D, entity id); n_before counts the c ordered before the target, n_known_before those of
them whose completed triple is known.  Distances come from transx_ref._proj / transr_ref.residual."""
import numpy as np

from tests import transr_ref as RR
from tests import transx_ref as XR

U = 2.0 ** -24


def _proj_all(model, tabs, r):
    """Projection of every entity under relation r: [E, d] fp64."""
    E = tabs["ent"].shape[0]
    if model == "transr":
        dim_e, dim_r = RR.dims(tabs)
        return tabs["ent"] @ RR.matrices(tabs, np.array([r]), dim_e, dim_r)[0].T
    return XR._proj(model, tabs, np.arange(E), np.full(E, r))


def _proj_mag_all(model, tabs, r):
    """A bound on every partial sum that makes each entity's projection under r, [E, d]."""
    A = {k: np.abs(np.asarray(v, dtype=np.float64)) for k, v in tabs.items()}
    E = A["ent"].shape[0]
    if model == "transr":
        dim_e, dim_r = RR.dims(A)
        return A["ent"] @ RR.matrices(A, np.array([r]), dim_e, dim_r)[0].T
    if model == "transe":
        return A["ent"]
    if model == "transh":
        n = tabs["normal_vector"][r]
        nh = np.abs(n) / np.sqrt(max((n * n).sum(), XR.EPS))
        return A["ent"] + (A["ent"] @ nh)[:, None] * nh[None, :]
    return A["ent"] + (A["ent"] * A["ent_transfer"]).sum(1, keepdims=True) * A["rel_transfer"][r][None, :]


def distances(model, tabs, test, side="tail", l1=True, magnitude=False):
    """fp64 D [n, E] of every test row against every candidate; magnitude=True: the same with every term in absolute
    value (bounds each partial sum)."""
    tabs = {k: np.asarray(v, dtype=np.float64) for k, v in tabs.items()}
    test = np.asarray(test, dtype=np.int64)
    E = tabs["ent"].shape[0]
    out = np.empty((len(test), E))
    for i, (h, t, r) in enumerate(test):
        P = (_proj_mag_all if magnitude else _proj_all)(model, tabs, r)
        fixed = h if side == "tail" else t
        rel = np.abs(tabs["rel"][r]) if magnitude else tabs["rel"][r]
        if magnitude:
            u = P[fixed][None, :] + rel[None, :] + P
        elif side == "tail":
            u = (P[fixed] + rel)[None, :] - P
        else:
            u = P + rel[None, :] - P[fixed][None, :]
        out[i] = np.abs(u).sum(1) if l1 else (u * u).sum(1)
    return out


def _before(D, true_ids):
    n, E = D.shape
    dt = D[np.arange(n), true_ids][:, None]
    c = np.arange(E)[None, :]
    return (D < dt) | ((D == dt) & (c < np.asarray(true_ids)[:, None]))


def known_mask(test, known, E, side="tail"):
    """[n, E] bool: the completed triple of (row, c) is in `known` (a set of (h, t, r))."""
    ks = {tuple(int(x) for x in k) for k in np.asarray(known, dtype=np.int64).reshape(-1, 3)}
    m = np.zeros((len(test), E), dtype=bool)
    for i, (h, t, r) in enumerate(np.asarray(test, dtype=np.int64)):
        for c in range(E):
            if ((int(h), c, int(r)) if side == "tail" else (c, int(t), int(r))) in ks:
                m[i, c] = True
    return m


def counts(D, true_ids, kmask=None):
    """(n_before, n_known_before) int64 of each row of distances D under (D, id) order."""
    b = _before(D, true_ids)
    nk = (b & kmask).sum(1) if kmask is not None else np.zeros(len(D), dtype=np.int64)
    return b.sum(1).astype(np.int64), nk.astype(np.int64)


def count_bounds(D, M, true_ids, tol_rel):
    """[lo, hi] of n_before when each D_c may be off by tol_rel * M_c (M: distances(..., magnitude=True))."""
    n, E = D.shape
    tol = tol_rel * M
    i = np.arange(n)
    dt, tt = D[i, true_ids][:, None], tol[i, true_ids][:, None]
    c = np.arange(E)[None, :]
    not_true = c != np.asarray(true_ids)[:, None]
    sure = (D + tol < dt - tt) & not_true
    maybe = (D - tol <= dt + tt) & not_true
    return sure.sum(1), maybe.sum(1)


def true_ids(test, side):
    test = np.asarray(test, dtype=np.int64)
    return test[:, 1] if side == "tail" else test[:, 0]


def brute_force(model, tabs, test, side="tail", l1=True, known=()):
    """(raw, filtered) by sorting every row's candidates with sorted(key=(D, id)) and walking the list."""
    D = distances(model, tabs, test, side, l1)
    ks = {tuple(int(x) for x in k) for k in np.asarray(known, dtype=np.int64).reshape(-1, 3)}
    raw, fil = [], []
    for i, (h, t, r) in enumerate(np.asarray(test, dtype=np.int64)):
        target = t if side == "tail" else h
        order = sorted(range(D.shape[1]), key=lambda c: (D[i, c], c))
        pos = order.index(target)
        skipped = sum(1 for c in order[:pos] if (((int(h), c, int(r)) if side == "tail" else (c, int(t), int(r))) in ks))
        raw.append(pos + 1)
        fil.append(pos + 1 - skipped)
    return np.array(raw), np.array(fil)


def tie_fixture(model, E=40, R=5, d=8, n_test=24, seed=0):
    """Integer tables (every intermediate below 2^24) with duplicated entity rows, test rows whose target sits in a
    tie group, and a known set that holds tied candidates before and after the target, the targets themselves and
    duplicate triples.  TransH normals are signed unit axes (n^ = n exactly).  Returns (tabs, test, known)."""
    rng = np.random.default_rng(seed)
    if model == "transr":
        tabs = RR.integer_tables(E, R, d, d + 2 if d < 8 else d, seed=seed)
    else:
        tabs = XR.exact_tables(model, E, R, d, seed=seed)
    if model == "transh":
        n = np.zeros((R, d))
        n[np.arange(R), rng.integers(0, d, R)] = rng.choice([-1.0, 1.0], R)
        tabs["normal_vector"] = n
    groups = [np.sort(rng.choice(E, 3, replace=False)) for _ in range(4)]
    for g in groups:                                     # exact ties: identical rows across a group
        for k in tabs:
            if tabs[k].shape[0] == E:
                tabs[k][g[1:]] = tabs[k][g[0]]
    test = []
    for i in range(n_test):
        g = groups[i % len(groups)]
        target = g[rng.integers(0, 3)]
        other, r = rng.integers(0, E), rng.integers(0, R)
        test.append((other, target, r) if i % 2 == 0 else (target, other, r))
    test = np.array(test, dtype=np.int64)
    known = [test[:6]]                                   # targets themselves
    for h, t, r in test:                                  # tied candidates on both sides of the target, both sides
        for g in groups:
            for c in g[rng.random(3) < 0.5]:
                known.append([[h, c, r], [c, t, r]])
    known = np.concatenate([np.asarray(k, dtype=np.int64).reshape(-1, 3) for k in known], 0)
    known = np.concatenate([known, known[:10]], 0)        # duplicate known triples
    return tabs, test, known
