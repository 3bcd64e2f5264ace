"""The type-constrained 1-vs-all softmax objective of ComplEx (include/ge_hip.h: ge_softmax_masked_loss /
ge_softmax_masked_grad) in closed form, NumPy: tests/softmax_ref.py with row i's softmax taken over the candidate
POSITIONS its set admits.

    adm_ij = row_set_i == -1 or sets[row_set_i, j]           sets: bool [n_sets, K] by candidate position
    loss_i = logsumexp_{j: adm_ij} z_ij - z_i,true           NaN for an invalid row
    dL/ds_ij = -scale * (softmax_{j: adm_ij}(z_ij) - [cand_j == true_i]),  0 for an inadmissible pair

A row is valid iff it is valid in softmax_ref AND its row set is -1 or in [0, n_sets) AND the position of its true candidate
is admissible.  `dtype` float64 is the oracle; float32 evaluates the same formulas in float32 with the sums over rows in
index order, as softmax_ref.evaluate does."""
import numpy as np

from tests import adagrad_ref as AR
from tests.softmax_ref import _clip, _clip_back, query


def mask_words(K):
    return 0 if K <= 0 else 4 * ((K + 127) // 128)


def pack(sets, ones_beyond_k=False):
    """uint32 [n_sets, mask_words(K)] of bool [n_sets, K]: bit c & 31 of word c >> 5 = position c."""
    sets = np.asarray(sets, bool)
    n, K = sets.shape
    W = mask_words(K)
    full = np.zeros((n, 32 * W), bool)
    full[:, :K] = sets
    if ones_beyond_k:
        full[:, K:] = True
    w = (full.reshape(n, W, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(2)
    return w.astype(np.uint32)


def admissible(row_set, sets):
    """(bool [B, K], bool [B] the row's set id is usable)."""
    sets = np.asarray(sets, bool)
    rs = np.asarray(row_set, np.int64)
    ok = (rs >= -1) & (rs < sets.shape[0])
    adm = np.where((rs == -1)[:, None], True, sets[np.clip(rs, 0, sets.shape[0] - 1)])
    return adm & ok[:, None], ok


def evaluate(table, hr, true_id, cand, max_norm, scale, head, row_set, sets, lr=1.0, dtype=np.float64):
    """(loss [B], grad_idx [K + 2B] int32, grad_val [K + 2B, d] = -lr * gradient of SUM_i loss_i) in `dtype`."""
    dt = np.dtype(dtype).type
    T = np.asarray(table).astype(dtype)
    N, d = T.shape
    k = d // 2
    hr, true_id, cand = np.asarray(hr, np.int64), np.asarray(true_id, np.int64), np.asarray(cand, np.int64)
    B, K = hr.shape[0], cand.shape[0]
    inr = lambda v: (v >= 0) & (v < N)
    cok = inr(cand)
    adm, set_ok = admissible(row_set, sets)
    pos = np.full(B, -1, np.int64)
    where = {int(c): j for j, c in enumerate(cand) if cok[j]}
    for i in range(B):
        pos[i] = where.get(int(true_id[i]), -1)
    rows = np.arange(B)
    valid = inr(hr[:, 0]) & inr(hr[:, 1]) & inr(true_id) & (pos >= 0) & set_ok & adm[rows, np.maximum(pos, 0)]
    safe = lambda v: np.where(inr(v), v, 0)
    f, r, c = T[safe(hr[:, 0])], T[safe(hr[:, 1])], T[safe(cand)]
    fh, nf = _clip(f, max_norm)
    rh, nr = _clip(r, max_norm)
    ch, nc = _clip(c, max_norm)
    Q = query(fh, rh, head)
    S = Q @ ch.T
    z = (dt(-scale) * S).astype(dtype)
    z[:, ~cok] = -np.inf
    z[~adm] = -np.inf
    z[~valid] = 0.0
    m = z.max(1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(1, dtype=dtype))
    loss = np.where(valid, lse - z[rows, np.maximum(pos, 0)], np.nan).astype(dtype)
    p = np.exp(z - lse[:, None])
    y = np.zeros((B, K), dtype)
    y[rows[valid], pos[valid]] = 1
    w = (dt(-scale) * (p - y)).astype(dtype)
    w[~valid] = 0
    w[:, ~cok] = 0
    w[~adm] = 0
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


def step(table, accum, triples, cand, max_norm, scale, lr, sets_tail, sets_head, row_set=None):
    """One SoftmaxAdaGrad step with candidate sets in place on fp64 `table` / `accum` (row_set default: the relation
    ids).  Returns (loss [B,2], per-row sums [N,d], rows named [N]).  A candidate no valid row admits is a slot with an
    exact zero row: AdaGrad leaves it as it is, and it does not count as named."""
    tri = np.asarray(triples, np.int64)
    rs = tri[:, 2] if row_set is None else np.asarray(row_set, np.int64)
    lt, it, vt = evaluate(table, tri[:, [0, 2]], tri[:, 1], cand, max_norm, scale, False, rs, sets_tail)
    lh, ih, vh = evaluate(table, tri[:, [1, 2]], tri[:, 0], cand, max_norm, scale, True, rs, sets_head)
    idx, val = np.concatenate([it, ih]), np.concatenate([vt, vh])
    idx = np.where(np.any(val != 0, 1), idx, -1).astype(np.int32)
    s, named = AR.apply_rows(table, accum, idx, -val, lr)
    return np.stack([lt, lh], 1), s, named


# ------------------------------------------------------------------------------------------------ the typed planted KG
def typed_kg(n_ent=800, n_rel=8, n_types=4, dim=8, n_triples=6000, noise=0.05, seed=1):
    """A planted KG with types: relation r takes heads of two types (dom) and tails of two types (ran); the tail of
    (h, r) is the admissible entity nearest ent[h] + rel[r].  Returns (triples [n,3] head, tail, relation; type [n_ent])."""
    rng = np.random.default_rng(seed)
    ent = rng.normal(size=(n_ent, dim)); rel = rng.normal(size=(n_rel, dim)) * 0.5
    typ = np.arange(n_ent) % n_types
    dom = np.stack([rng.permutation(n_types)[:2] for _ in range(n_rel)])
    ran = np.stack([rng.permutation(n_types)[:2] for _ in range(n_rel)])
    r = rng.integers(0, n_rel, n_triples)
    h = np.array([rng.choice(np.nonzero(np.isin(typ, dom[x]))[0]) for x in r])
    q = ent[h] + rel[r] + noise * rng.normal(size=(n_triples, dim))
    d2 = (ent * ent).sum(1)[None, :] - 2.0 * q @ ent.T
    d2[~((typ[None, :] == ran[r][:, 0:1]) | (typ[None, :] == ran[r][:, 1:2]))] = np.inf
    d2[np.arange(n_triples), h] = np.inf
    tri = np.unique(np.stack([h, d2.argmin(1), r], 1), axis=0); rng.shuffle(tri)
    return tri, typ


def typed_setup(n_rel=8):
    """(train, held out [300], all triples, cand, {side: bool [n_rel, K]}): entity ids shifted behind the relation rows;
    set r of a side = every entity whose type was seen on that side of r in train (CandidateSets.from_types)."""
    tri, typ = typed_kg(n_rel=n_rel)
    tri = tri.copy()
    tri[:, :2] += n_rel
    test, train = tri[:300], np.unique(tri[300:], axis=0)
    cand = np.arange(n_rel, n_rel + len(typ), dtype=np.int32)
    sets = {}
    for side, col in (("tail", 1), ("head", 0)):
        s = np.zeros((n_rel, len(cand)), bool)
        for r in range(n_rel):
            seen = np.unique(typ[train[train[:, 2] == r, col] - n_rel])
            s[r] = np.isin(typ, seen)
        sets[side] = s
    return train.astype(np.int32), test.astype(np.int32), tri.astype(np.int32), cand, sets, typ


def batches(n_train, B, n_steps, seed=3):
    """The row indices of n_steps batches: a new permutation whenever fewer than B rows are left, then the first B rows of
    the remaining order."""
    rng = np.random.default_rng(seed)
    order, at, out = np.zeros(0, np.int64), 0, []
    for _ in range(n_steps):
        if len(order) - at < B:
            order, at = rng.permutation(n_train), 0
        out.append(order[at:at + B])
        at += B
    return out


def mrr_masked(table, test, all_tri, cand, sets):
    """Filtered MRR, both sides, against the sets (inadmissible candidates skipped), of an fp64 table with the project's
    tie rule (an equal loss with a smaller candidate id pops first)."""
    fh = lambda x: _clip(x, 1.0)[0]
    rr = []
    for side, head, (fx, tr) in (("tail", False, (0, 1)), ("head", True, (1, 0))):
        known = {}
        for row in all_tri:
            known.setdefault((int(row[fx]), int(row[2])), set()).add(int(row[tr]))
        S = query(fh(table[test[:, fx]]), fh(table[test[:, 2]]), head) @ fh(table[cand]).T
        for i, row in enumerate(test):
            j = int(np.nonzero(cand == row[tr])[0][0])
            before = (S[i] < S[i, j]) | ((S[i] == S[i, j]) & (cand < row[tr]))
            skip = np.isin(cand, list(known[(int(row[fx]), int(row[2]))] - {int(row[tr])}))
            rr.append(1.0 / (1 + int((before & ~skip & sets[side][row[2]]).sum())))
    return float(np.mean(rr))
