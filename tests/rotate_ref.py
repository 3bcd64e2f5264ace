"""NumPy restatement of RotatE (graphembeddings_amd.rotate, include/ge_hip.h's ge_rotate_*) for the tests (product
code never imports it).  fp64 by default; every function takes `dtype`, and with np.float32 the same statements run in
fp32, which is how the GPU tests size their tolerances (e32: the largest deviation of the fp32 evaluation from fp64).

Tables: ent [E,d], d even, k = d / 2, a row [Re (k) | Im (k)]; rel [R,k] of phases.  u_j = h_j e^{i theta_j} - t_j,
m_j = |u_j|, D = sum m_j (l1) or sum m_j^2.  g_j = dD/du_j = u_j / m_j (0 where m_j == 0) or 2 u_j; dD/dh_j =
g_j conj(e^{i theta_j}); dD/dt_j = -g_j; dD/dtheta_j = Re g_j (-Im w_j) + Im g_j Re w_j with w_j = h_j e^{i theta_j}.
The hinge, the dedup-sum SGD step and the AdaGrad step are the translation family's (tests/transx_ref.py,
tests/transx_adagrad_ref.py); ranks are ascending (D, entity id) with known-cell filtering.
"""
from __future__ import annotations

import numpy as np


def _cast(tabs, dtype):
    return {k: np.asarray(v, dtype=dtype) for k, v in tabs.items()}


def _parts(tabs, h, t, r):
    """(w_re, w_im, u_re, u_im, c, s) [B,k] of the triples, in the tables' dtype."""
    ent, th = tabs["ent"], tabs["rel"][r]
    k = ent.shape[1] // 2
    c, s = np.cos(th), np.sin(th)
    hre, him, tre, tim = ent[h, :k], ent[h, k:], ent[t, :k], ent[t, k:]
    wre, wim = hre * c - him * s, hre * s + him * c
    return wre, wim, wre - tre, wim - tim, c, s


def _norm(ure, uim, l1):
    m2 = ure * ure + uim * uim
    return (np.sqrt(m2) if l1 else m2).sum(1)


def dist(tabs, tri, l1=True, dtype=np.float64):
    """D of every (h, t, r) row."""
    tabs, tri = _cast(tabs, dtype), np.asarray(tri, dtype=np.int64)
    _, _, ure, uim, _, _ = _parts(tabs, tri[:, 0], tri[:, 1], tri[:, 2])
    return _norm(ure, uim, l1)


def dist_head_form(tabs, tri, l1=True, dtype=np.float64):
    """The same D as the head side of the rank sweep writes it: |h - t e^{-i theta}|."""
    tabs, tri = _cast(tabs, dtype), np.asarray(tri, dtype=np.int64)
    ent, th = tabs["ent"], tabs["rel"][tri[:, 2]]
    k = ent.shape[1] // 2
    c, s = np.cos(th), np.sin(th)
    h, t = tri[:, 0], tri[:, 1]
    qre, qim = ent[t, :k] * c + ent[t, k:] * s, ent[t, k:] * c - ent[t, :k] * s
    return _norm(qre - ent[h, :k], qim - ent[h, k:], l1)


def _dist_grad(ure, uim, l1):
    if not l1:
        return 2 * ure, 2 * uim
    m = np.sqrt(ure * ure + uim * uim)
    safe = np.where(m > 0, m, 1)
    return np.where(m > 0, ure / safe, 0), np.where(m > 0, uim / safe, 0)


def _grads_of(parts, l1):
    wre, wim, ure, uim, c, s = parts
    gre, gim = _dist_grad(ure, uim, l1)
    gh = np.concatenate([gre * c + gim * s, gim * c - gre * s], 1)
    gt = np.concatenate([-gre, -gim], 1)
    return gh, gt, gim * wre - gre * wim


def triple_grads(tabs, tri, l1=True):
    """Per-row gradients of D: (d/d ent[h] [B,d], d/d ent[t] [B,d], d/d rel[r] [B,k]) in the tables' dtype."""
    return _grads_of(_parts(tabs, tri[:, 0], tri[:, 1], tri[:, 2]), l1)


def active_mask(tabs, pos, neg, margin, l1=True, dtype=np.float64):
    z = dist(tabs, pos, l1, dtype) - dist(tabs, neg, l1, dtype) + np.asarray(margin, dtype=dtype)
    return z >= 0


def hinge_grads(tabs, pos, neg, margin, l1=True, dtype=np.float64):
    """(loss, {"ent": [E,d], "rel": [R,k]} summed gradients, active [B]) of sum_i max(D(pos_i) - D(neg_i) + margin, 0);
    a pair is active iff that argument is >= 0."""
    tabs = _cast(tabs, dtype)
    pos, neg = np.asarray(pos, dtype=np.int64), np.asarray(neg, dtype=np.int64)
    parts = [_parts(tabs, tri[:, 0], tri[:, 1], tri[:, 2]) for tri in (pos, neg)]
    z = _norm(parts[0][2], parts[0][3], l1) - _norm(parts[1][2], parts[1][3], l1) + np.asarray(margin, dtype=dtype)
    active = z >= 0
    loss = np.where(active, z, 0).astype(dtype).sum()
    grads = {k: np.zeros_like(v) for k, v in tabs.items()}
    a = active.astype(dtype)[:, None]
    for tri, sgn, p in ((pos, 1, parts[0]), (neg, -1, parts[1])):
        gh, gt, gr = _grads_of(p, l1)
        np.add.at(grads["ent"], tri[:, 0], (sgn * a * gh).astype(dtype))
        np.add.at(grads["ent"], tri[:, 1], (sgn * a * gt).astype(dtype))
        np.add.at(grads["rel"], tri[:, 2], (sgn * a * gr).astype(dtype))
    return float(loss), grads, active


def named_rows(tabs, pos, neg, active):
    """{"ent": bool [E], "rel": bool [R]}: the rows an active pair names."""
    pos, neg = np.asarray(pos, dtype=np.int64), np.asarray(neg, dtype=np.int64)
    out = {k: np.zeros(len(v), dtype=bool) for k, v in tabs.items()}
    out["ent"][np.concatenate([pos[active, 0], pos[active, 1], neg[active, 0], neg[active, 1]])] = True
    out["rel"][pos[active, 2]] = True
    return out


def sgd_step(tabs, pos, neg, lr, margin, l1=True, dtype=np.float64):
    """(new tables, loss): every gradient on the pre-step tables, duplicates summed, row -= lr * sum."""
    loss, grads, _ = hinge_grads(tabs, pos, neg, margin, l1, dtype)
    lr = np.asarray(lr, dtype=dtype)
    return {k: np.asarray(v, dtype=dtype) - lr * grads[k] for k, v in tabs.items()}, loss


def adagrad_step(tabs, accs, pos, neg, lr, margin, l1=True, dtype=np.float64):
    """(new tables, new accumulators, loss): per row an active pair names, acc += s * s, row -= lr * s / sqrt(acc) on the
    updated accumulator; every other row of both arrays as it was."""
    loss, grads, active = hinge_grads(tabs, pos, neg, margin, l1, dtype)
    named = named_rows(tabs, pos, neg, active)
    lr = np.asarray(lr, dtype=dtype)
    new_t, new_a = {}, {}
    for k, v in tabs.items():
        v, a, s = np.asarray(v, dtype=dtype), np.asarray(accs[k], dtype=dtype), grads[k]
        acc = a + s * s
        upd = v - lr * s / np.sqrt(acc)
        rows = named[k][:, None]
        new_a[k], new_t[k] = np.where(rows, acc, a), np.where(rows, upd, v)
    return new_t, new_a, loss


def rank_query(tabs, tri, side="tail", dtype=np.float64):
    """(q_re, q_im) [B,k] of the rank sweep: h o e^{i theta} (tail side) or t o e^{-i theta} (head side)."""
    tabs, tri = _cast(tabs, dtype), np.asarray(tri, dtype=np.int64)
    ent, th = tabs["ent"], tabs["rel"][tri[:, 2]]
    k = ent.shape[1] // 2
    c, s = np.cos(th), np.sin(th)
    f = tri[:, 1] if side == "head" else tri[:, 0]
    if side == "head":
        s = -s
    return ent[f, :k] * c - ent[f, k:] * s, ent[f, :k] * s + ent[f, k:] * c


def all_dists(tabs, tri, side="tail", l1=True, dtype=np.float64):
    """[B, E]: D of every entity in the tail's (head's) place."""
    qre, qim = rank_query(tabs, tri, side, dtype)
    ent = np.asarray(tabs["ent"], dtype=dtype)
    k = ent.shape[1] // 2
    out = np.empty((len(qre), len(ent)), dtype=dtype)
    for i in range(len(qre)):
        a, b = qre[i][None, :] - ent[:, :k], qim[i][None, :] - ent[:, k:]
        m2 = a * a + b * b
        out[i] = (np.sqrt(m2) if l1 else m2).sum(1)
    return out


def counts_from(scores, true_dist, target, known_mask=None):
    """(n_before, n_known_before) [B] from a [B,E] distance matrix with the (D, id) rule: c ranks before the target iff
    D_c < D_true, or D_c == D_true and c < target.  known_mask [B,E] bool: the cells counted as known."""
    ids = np.arange(scores.shape[1])[None, :]
    td, tg = np.asarray(true_dist)[:, None], np.asarray(target)[:, None]
    before = (scores < td) | ((scores == td) & (ids < tg))
    nk = (before & known_mask).sum(1) if known_mask is not None else np.zeros(len(scores), dtype=np.int64)
    return before.sum(1), nk


def ranks(tabs, tri, side="tail", l1=True, known_mask=None, dtype=np.float64):
    """(n_before, n_known_before, true_dist, scores) of the rows, ascending (D, entity id)."""
    tri = np.asarray(tri, dtype=np.int64)
    sc = all_dists(tabs, tri, side, l1, dtype)
    target = tri[:, 0] if side == "head" else tri[:, 1]
    td = sc[np.arange(len(tri)), target]
    nb, nk = counts_from(sc, td, target, known_mask)
    return nb, nk, td, sc


def pairwise_accuracy(tabs, held, corr, l1=True):
    """Share of rows with D(held) < D(corr): test_gpu_transx.py's held-out figure."""
    return float((dist(tabs, held, l1) < dist(tabs, corr, l1)).mean())


def planted_rotation_kg(n_ent=500, n_rel=40, k=4, n_triples=30000, noise=0.05, seed=0, sym=4):
    """A rotational KG with no download: entities are complex standard normals in k dims, relations uniform phases --
    except the first `sym`, drawn from {0, pi} and therefore symmetric -- and each triple's tail is the entity nearest to
    h o r + noise in the modulus-L1 norm, never h.  Returns (triples [T,3] (h, t, r) int64, unique rows, shuffled)."""
    rng = np.random.default_rng(seed)
    ent = rng.normal(size=(n_ent, k)) + 1j * rng.normal(size=(n_ent, k))
    phase = rng.uniform(-np.pi, np.pi, size=(n_rel, k))
    phase[:sym] = np.pi * rng.integers(0, 2, size=(sym, k))
    h = rng.integers(0, n_ent, n_triples)
    r = rng.integers(0, n_rel, n_triples)
    q = ent[h] * np.exp(1j * phase[r]) + noise * (rng.normal(size=(n_triples, k)) + 1j * rng.normal(size=(n_triples, k)))
    t = np.empty(n_triples, dtype=np.int64)
    for s in range(0, n_triples, 1024):
        blk = q[s:s + 1024]
        D = np.abs(blk[:, None, :] - ent[None, :, :]).sum(2)
        D[np.arange(len(blk)), h[s:s + 1024]] = np.inf      # no self loops
        t[s:s + 1024] = D.argmin(1)
    tri = np.unique(np.stack([h, t, r], 1), axis=0)
    rng.shuffle(tri)
    return tri


# ------------------------------------------------------------------------------------ the GPU tests' tolerance
ULP = 2.0 ** -23
FLOOR = 1e-7                    # test_gpu_transx.py's absolute term


def bound(ref64, ref32, scale=0.0):
    """(bound, base, e32) of one case: e32 = the largest deviation of the float32 evaluation ref32 from ref64;
    base = 8 e32 + FLOOR is the rule.  Only in a case whose e32 is below one fp32 ulp of its largest value,
    2^-23 max(1, |ref|), bound adds one such ulp per element: there the fp32 restatement happens to land on the fp64 values,
    and a correctly rounded fp32 result may still sit one ulp from them.  Elsewhere bound is base.
    scale: the largest fp32 value the quantity is formed from, where that is larger than the quantity itself -- a batch
    loss is sum_i (D+ - D- + margin) of fp32 distances and cannot be more exact than one ulp of the largest of them,
    however small the difference; the ulp is then taken at max(1, |ref|, scale).  (With one pair the fp32 restatement's
    own error is a single sample, and is often far below that ulp.)"""
    ref64, ref32 = np.asarray(ref64, dtype=np.float64), np.asarray(ref32, dtype=np.float64)
    e32 = float(np.abs(ref32 - ref64).max()) if ref64.size else 0.0
    ulp = ULP * np.maximum(np.maximum(1.0, np.abs(ref64)), float(scale))
    base = 8.0 * e32 + FLOOR + 0.0 * ulp
    return (base + ulp if ref64.size and e32 < float(ulp.max()) else base), base, e32


def largest_dist(tabs, pos, neg, l1=True):
    """The largest distance a batch's loss is formed from (bound's `scale` for a loss)."""
    return float(max(dist(tabs, pos, l1).max(), dist(tabs, neg, l1).max()))


# ------------------------------------------------------------------------------------ exact-arithmetic fixtures
def exact_tables_l2(E, R, d, seed=0, amp=2):
    """theta = 0 everywhere, small integer coordinates: with the squared norm every distance, gradient and sum is an
    integer that fp32 holds."""
    rng = np.random.default_rng(seed)
    return {"ent": rng.integers(-amp, amp + 1, size=(E, d)).astype(np.float64), "rel": np.zeros((R, d // 2))}


def collinear_tables(E, R, d, seed=0, amp=3):
    """theta = 0 and every entity coordinate an integer multiple n (3 + 4i): every difference is a Pythagorean
    (3n, 4n), its modulus the integer 5 |n|, so the modulus norm is exact in fp32 too (and full of ties)."""
    rng = np.random.default_rng(seed)
    n = rng.integers(-amp, amp + 1, size=(E, d // 2)).astype(np.float64)
    return {"ent": np.concatenate([3 * n, 4 * n], 1), "rel": np.zeros((R, d // 2))}


FP32_EXACT = 2.0 ** 24


def valid_mask(pos, neg, E, R):
    """The gradient kernel's `ok`: every id in range and the negative on the positive's relation."""
    pos, neg = np.asarray(pos, dtype=np.int64), np.asarray(neg, dtype=np.int64)
    ok = (pos[:, 2] >= 0) & (pos[:, 2] < R) & (neg[:, 2] == pos[:, 2])
    for a in (pos[:, 0], pos[:, 1], neg[:, 0], neg[:, 1]):
        ok &= (a >= 0) & (a < E)
    return ok


def exact_step_bound(tabs, pos, neg, lr, margin):
    """For exact_tables_l2's form (integer entities, theta = 0), the squared norm, an integer margin and lr = 2^-n: the
    largest sum of |terms| any sum of one SGD step can reach in any order, counted on the value's own grid (1 for the
    distances, the loss and the summed gradient rows; lr for row - lr * sum).  Below 2^24 fp32 computes every one of them
    exactly, so the step's loss and tables must equal sgd_step's bitwise.  Pairs the kernel drops (valid_mask) write
    nothing and are left out.  Raises ValueError for a fixture not of this form."""
    tabs = _cast(tabs, np.float64)
    if not np.array_equal(tabs["ent"], np.round(tabs["ent"])) or np.any(tabs["rel"] != 0) or margin != round(margin):
        raise ValueError("integer entities, zero phases and an integer margin are needed")
    if not lr > 0 or np.frexp(lr)[0] != 0.5:
        raise ValueError(f"lr={lr} is not a power of two")
    pos, neg = np.asarray(pos, dtype=np.int64), np.asarray(neg, dtype=np.int64)
    ok = valid_mask(pos, neg, len(tabs["ent"]), len(tabs["rel"]))
    pos, neg = pos[ok], neg[ok]
    parts = [_parts(tabs, tri[:, 0], tri[:, 1], tri[:, 2]) for tri in (pos, neg)]
    dp, dn = _norm(parts[0][2], parts[0][3], False), _norm(parts[1][2], parts[1][3], False)
    z = dp - dn + margin
    active = z >= 0
    worst = max(float((dp + dn + abs(margin)).max()), float(np.abs(z[active]).sum()))
    mag = {k: np.zeros_like(v) for k, v in tabs.items()}
    for tri, (wre, wim, ure, uim, _, _) in ((pos, parts[0]), (neg, parts[1])):
        g = np.abs(np.concatenate([2 * ure, 2 * uim], 1))[active]          # |dD/dh| = |dD/dt| at theta = 0
        np.add.at(mag["ent"], tri[active, 0], g)
        np.add.at(mag["ent"], tri[active, 1], g)
        np.add.at(mag["rel"], tri[active, 2], (np.abs(2 * uim * wre) + np.abs(2 * ure * wim))[active])
    for k, v in tabs.items():
        worst = max(worst, float((np.abs(v) / lr + mag[k]).max()))
    return worst


def is_exact_step(tabs, pos, neg, lr, margin):
    """True iff every sum of |terms| of the squared-norm step stays below 2^24: fp32 gives the fp64 result bitwise in any
    order (the distances, the loss, every summed gradient row and lr * sum against the row)."""
    try:
        return exact_step_bound(tabs, pos, neg, lr, margin) < FP32_EXACT
    except ValueError:
        return False


def known_mask(test, known, E, side="tail"):
    """[n, E] bool: cell (i, c) is known iff the test row with c in the candidate's place is a known triple.  Every
    triple is encoded as one integer (fixed entity, relation, candidate) and the cells are looked up with np.isin, a block
    of rows at a time."""
    test, known = np.asarray(test, dtype=np.int64), np.asarray(known, dtype=np.int64).reshape(-1, 3)
    fix, cand = (0, 1) if side == "tail" else (1, 0)
    R = int(max(test[:, 2].max(initial=0), known[:, 2].max(initial=0))) + 1
    inside = (known[:, cand] >= 0) & (known[:, cand] < E)
    keys = np.unique((known[inside, fix] * R + known[inside, 2]) * E + known[inside, cand])
    out = np.empty((len(test), E), dtype=bool)
    ids = np.arange(E, dtype=np.int64)[None, :]
    for s in range(0, len(test), 4096):
        rows = test[s:s + 4096]
        out[s:s + 4096] = np.isin(((rows[:, fix] * R + rows[:, 2]) * E)[:, None] + ids, keys)
    return out


def all_dists_blocked(tabs, tri, side="tail", l1=True, dtype=np.float64, block=2048):
    """all_dists for many rows: the same statements, a block of rows at a time instead of one."""
    qre, qim = rank_query(tabs, tri, side, dtype)
    ent = np.asarray(tabs["ent"], dtype=dtype)
    k = ent.shape[1] // 2
    out = np.empty((len(qre), len(ent)), dtype=dtype)
    for s in range(0, len(qre), block):
        a, b = qre[s:s + block, None, :] - ent[None, :, :k], qim[s:s + block, None, :] - ent[None, :, k:]
        m2 = a * a + b * b
        out[s:s + block] = (np.sqrt(m2) if l1 else m2).sum(2)
    return out
