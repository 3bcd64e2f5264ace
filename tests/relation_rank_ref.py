"""fp64 restatement of the translation models' relation prediction (ge_transx_relation_rank / ge_transr_relation_rank).

For test row (h, t, r) every relation c is a candidate with D_c = D(h, t, c), in the linear form the kernels compute:
w = e_h - e_t, then TransE u = w + r_c; TransH u = w - (n^_c . w) n^_c + r_c; TransD u = w + s rp_c + r_c with
s = e_h . p_h - e_t . p_t; TransR u = M_c w + r_c; D = sum |u| or sum u^2.  The order is ascending by (D, relation
id); n_before counts the c ordered before r, n_known_before those of them with (h, t, c) known."""
import numpy as np

from tests import transr_ref as RR
from tests import transx_ref as XR
from tests.translation_rank_ref import U, count_bounds, counts  # noqa: F401  (the same count rules)

REL_TABLES = ("rel", "normal_vector", "rel_transfer", "rel_matrix")


def distances(model, tabs, test, l1=True, magnitude=False):
    """fp64 D [n, R] of every test row against every relation; magnitude=True: the same with every term in absolute
    value (|e_h| + |e_t|, |n^|, |M|, ...), which bounds each partial sum."""
    tabs = {k: np.asarray(v, dtype=np.float64) for k, v in tabs.items()}
    if magnitude:
        A = {k: np.abs(v) for k, v in tabs.items()}
    else:
        A = tabs
    test = np.asarray(test, dtype=np.int64)
    h, t = test[:, 0], test[:, 1]
    w = A["ent"][h] + A["ent"][t] if magnitude else A["ent"][h] - A["ent"][t]          # [n, dE]
    rel = A["rel"]                                                                     # [R, dq]
    if model == "transe":
        u = w[:, None, :] + rel[None]
    elif model == "transh":
        n = tabs["normal_vector"]
        nh = n / np.sqrt(np.maximum((n * n).sum(1, keepdims=True), XR.EPS))
        if magnitude:
            nh = np.abs(nh)
        a = w @ nh.T                                                                   # [n, R]
        u = w[:, None, :] + (a if magnitude else -a)[:, :, None] * nh[None] + rel[None]
    elif model == "transd":
        sh, st = (A["ent"][h] * A["ent_transfer"][h]).sum(1), (A["ent"][t] * A["ent_transfer"][t]).sum(1)
        s = sh + st if magnitude else sh - st
        u = w[:, None, :] + s[:, None, None] * A["rel_transfer"][None] + rel[None]
    elif model == "transr":
        dim_e, dim_r = RR.dims(tabs)
        M = A["rel_matrix"].reshape(-1, dim_r, dim_e)                                  # [R, dR, dE]
        u = np.einsum("ckj,nj->nck", M, w) + rel[None]
    else:
        raise ValueError(model)
    return np.abs(u).sum(2) if l1 else (u * u).sum(2)


def known_mask(test, known, R):
    """[n, R] bool: (h, t, c) of (row, c) is in `known`."""
    ks = {tuple(int(x) for x in k) for k in np.asarray(known, dtype=np.int64).reshape(-1, 3)}
    m = np.zeros((len(test), R), dtype=bool)
    for i, (h, t, _) in enumerate(np.asarray(test, dtype=np.int64)):
        for c in range(R):
            m[i, c] = (int(h), int(t), c) in ks
    return m


def brute_force(model, tabs, test, l1=True, known=()):
    """(raw, filtered) by sorting every row's relations with sorted(key=(D, id)) and walking the list."""
    D = distances(model, tabs, test, l1)
    ks = {tuple(int(x) for x in k) for k in np.asarray(known, dtype=np.int64).reshape(-1, 3)}
    raw, fil = [], []
    for i, (h, t, r) in enumerate(np.asarray(test, dtype=np.int64)):
        order = sorted(range(D.shape[1]), key=lambda c: (D[i, c], c))
        pos = order.index(r)
        skipped = sum(1 for c in order[:pos] if (int(h), int(t), c) in ks)
        raw.append(pos + 1)
        fil.append(pos + 1 - skipped)
    return np.array(raw), np.array(fil)


def tie_fixture(model, E=12, R=20, d=8, n_test=24, seed=0):
    """Integer tables (every intermediate below 2^24) with groups of relations whose rel / normal_vector /
    rel_transfer / rel_matrix rows are identical, so that exact ties sit on both sides of the target; test rows whose
    relation sits in a tie group; a known set that holds tied candidates, the targets themselves and duplicate
    triples.  TransH normals are signed unit axes (n^ = n exactly); TransR has dim_r = d + 2.
    Returns (tabs, test, known)."""
    rng = np.random.default_rng(seed)
    if model == "transr":
        tabs = RR.integer_tables(E, R, d, d + 2, seed=seed)
    else:
        tabs = XR.exact_tables(model, E, R, d, seed=seed)
    if model == "transh":
        n = np.zeros((R, d))
        n[np.arange(R), rng.integers(0, d, R)] = rng.choice([-1.0, 1.0], R)
        tabs["normal_vector"] = n
    groups = np.sort(rng.permutation(R)[:12].reshape(4, 3), axis=1)
    for g in groups:                                     # exact ties: identical relation-side rows across a group
        for k in REL_TABLES:
            if k in tabs:
                tabs[k][g[1:]] = tabs[k][g[0]]
    test = np.array([(rng.integers(0, E), rng.integers(0, E), groups[i % 4][rng.integers(0, 3)]) for i in range(n_test)],
                    dtype=np.int64)
    known = [test[:6]]                                   # targets themselves
    for h, t, _ in test:                                 # tied candidates on both sides of the target
        for g in groups:
            for c in g[rng.random(3) < 0.5]:
                known.append([[h, t, c]])
    known = np.concatenate([np.asarray(k, dtype=np.int64).reshape(-1, 3) for k in known], 0)
    known = np.concatenate([known, known[:10]], 0)        # duplicate known triples
    return tabs, test, known
