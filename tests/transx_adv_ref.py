"""NumPy restatement of the self-adversarial negative-sampling loss of TransE / TransH / TransD (include/ge_hip.h's
ge_transx_adv_*) for the tests (product code never imports it): tests/transx_ref.py's projections and per-triple
gradients under tests/rotate_adv_ref.py's softplus, sigmoid, validity rules and draw.  fp64 by default; with
dtype=np.float32 the same statements run in fp32, which is how the GPU tests size their tolerances.

A batch: pos [B,3] (h, t, r), side [B] (0: the tail is replaced, 1: the head), neg_ent [B,K].  Negative j of row i is
(h, neg_ent[i,j], r) or (neg_ent[i,j], t, r); a slot outside [0, E) is empty; a row with a positive id out of range or a
side outside {0, 1} is invalid (loss NaN here, 0 in the batch sum, no gradient).
  u = proj(h) + r - proj(t),  D = sum |u| or sum u^2
  p_ij   = softmax_j(-alpha D-_ij) over the live slots, not differentiated
  loss_i = softplus(D+_i - gamma) + sum_j p_ij softplus(gamma - D-_ij)
`form`: "ref" evaluates u as (proj(h) + r) - proj(t), transx_ref's order; "fixed" evaluates it as the kernel does, from
the fixed side: (proj(h) + r) - proj(t') where tails are replaced, -((proj(t) - r) - proj(h')) where heads are.
"fixed-rev" and "fixed-seq" are "fixed" with every sum in another order: the kernel adds a row's coordinates lane by lane
and then by a tree, a fixed row's contributions team by team with the positive's last, and the restatement's own order
(NumPy's pairwise sums, the positive first) is only one of many.  "fixed-rev" sums every row back to front and adds the
triples' gradients in reverse with the positives last; "fixed-seq" sums every row strictly left to right and adds the
negatives' gradients before the positives'.  In fp64 all forms agree to rounding; in fp32 each is one sample of the
rounding error of these statements, and the tests take the form that deviates most (FORMS32, worst32): with B = 1 a
single form's error at a row is one draw, often several times below what another order of the same sums gives.

The cases of tests/test_gpu_transx_adv.py are built here (step_cases(), other_cases(), build_case()) so that the host tests can check the
L1 sign-stability condition on the very tables and batches the GPU tests use.
"""
from __future__ import annotations

import numpy as np

from tests import rotate_adv_ref as AR
from tests import transx_ref as XR
from tests.rotate_adv_ref import draw, sigmoid, softplus, valid_rows  # noqa: F401  (the same rules and draw)

MODELS = ("transe", "transh", "transd")
PLANE1 = {"transe": {}, "transh": {"normal_vector": "rel"}, "transd": {"ent_transfer": "ent", "rel_transfer": "rel"}}


def _cast(tabs, dtype):
    return {k: np.asarray(v, dtype=dtype) for k, v in tabs.items()}


def residual(model, tabs, tri, head_side, form="ref"):
    """u [n,d] of the triples in the tables' dtype; head_side [n] bool selects the kernel's head-side order under "fixed"."""
    h, t, r = tri[:, 0], tri[:, 1], tri[:, 2]
    ph, pt, rr = XR._proj(model, tabs, h, r), XR._proj(model, tabs, t, r), tabs["rel"][r]
    if not form.startswith("fixed"):
        return ph + rr - pt
    return np.where(np.asarray(head_side, dtype=bool)[:, None], -((pt - rr) - ph), (ph + rr) - pt)


FORMS32 = ("ref", "fixed", "fixed-rev", "fixed-seq")


def _rowsum(x, form):
    """Sum over the last axis in the form's order."""
    if form == "fixed-rev":
        return x[..., ::-1].sum(-1)
    if form == "fixed-seq":
        return np.cumsum(x, axis=-1, dtype=x.dtype)[..., -1] if x.shape[-1] else x.sum(-1)
    return x.sum(-1)


def _dist(u, l1, form="ref"):
    return _rowsum(np.abs(u) if l1 else u * u, form)


def worst32(ref64, *cands):
    """Of several float32 evaluations, the one that deviates most from ref64 (the largest e32)."""
    r = np.asarray(ref64, dtype=np.float64)
    dev = [np.nanmax(np.abs(np.asarray(c, dtype=np.float64) - r), initial=0.0) for c in cands]
    return cands[int(np.argmax(dev))]


def parts(model, tabs, pos, side, neg_ent, margin, alpha, l1=True, dtype=np.float64, form="ref"):
    """Everything the loss is made of: dict(valid [B], live [B,K], Dp [B], Dn [B,K], p [B,K], loss [B] (NaN: invalid),
    pos [B,3], neg [B,K,3], up [B,d], un [B,K,d]) in `dtype`."""
    tabs = _cast(tabs, dtype)
    E, R = len(tabs["ent"]), len(tabs["rel"])
    valid, live, p3, neg = AR._negatives(pos, side, neg_ent, E, R)
    B, K = live.shape
    heads = np.asarray(side, dtype=np.int64) == 1
    gamma, alpha = np.asarray(margin, dtype=dtype), np.asarray(alpha, dtype=dtype)
    up = residual(model, tabs, p3, heads, form)
    un = residual(model, tabs, neg.reshape(-1, 3), np.repeat(heads, K), form)
    Dp, Dn = _dist(up, l1, form), _dist(un, l1, form).reshape(B, K)
    z = np.where(live, -alpha * Dn, -np.inf).astype(dtype)
    mx = np.where(live.any(1), z.max(1, initial=-np.inf), 0).astype(dtype)
    e = np.where(live, np.exp(np.where(live, z - mx[:, None], 0)), 0).astype(dtype)
    s = _rowsum(e, form)
    p = (e / np.where(s > 0, s, 1)[:, None]).astype(dtype)
    loss = softplus(Dp - gamma) + _rowsum((p * softplus(gamma - Dn)).astype(dtype), form)
    loss = np.where(valid, loss, np.nan).astype(dtype)
    return dict(valid=valid, live=live, Dp=Dp, Dn=Dn, p=p, loss=loss, pos=p3, neg=neg, up=up, un=un.reshape(B, K, -1))


def row_losses(model, tabs, pos, side, neg_ent, margin, alpha, l1=True, dtype=np.float64, form="ref"):
    """loss_i [B]; NaN for an invalid row."""
    return parts(model, tabs, pos, side, neg_ent, margin, alpha, l1, dtype, form)["loss"]


def grads(model, tabs, pos, side, neg_ent, margin, alpha, l1=True, dtype=np.float64, form="ref"):
    """(batch loss, {table: summed gradient}, named {table: bool [rows]}): each triple's gradients are
    transx_ref._triple_grads(model, tabs, h, t, r, a f(u)) with a = a+ or a-."""
    P = parts(model, tabs, pos, side, neg_ent, margin, alpha, l1, dtype, form)
    tabs = _cast(tabs, dtype)
    gamma = np.asarray(margin, dtype=dtype)
    valid, live = P["valid"], P["live"]
    a_pos = np.where(valid, sigmoid(P["Dp"] - gamma), 0).astype(dtype)
    a_neg = np.where(live, -P["p"] * sigmoid(gamma - P["Dn"]), 0).astype(dtype)
    out = {k: np.zeros_like(v) for k, v in tabs.items()}
    named = {k: np.zeros(len(v), dtype=bool) for k, v in tabs.items()}
    d = tabs["ent"].shape[1]
    groups = [(P["pos"], a_pos, valid, P["up"]),
              (P["neg"].reshape(-1, 3), a_neg.reshape(-1), live.reshape(-1), P["un"].reshape(-1, d))]
    if form in ("fixed-rev", "fixed-seq"):               # the negatives' gradients first, the positives' last
        groups = groups[::-1]
    if form == "fixed-rev":                              # ... and every group back to front
        groups = [tuple(x[::-1] for x in g) for g in groups]
    for tri, a, on, u in groups:
        h, t, r = tri[:, 0], tri[:, 1], tri[:, 2]
        g = (a[:, None] * XR._fgrad(u, l1)).astype(dtype)
        G = {k: np.asarray(v).astype(dtype) for k, v in XR._triple_grads(model, tabs, h, t, r, g).items()}
        np.add.at(out["ent"], h, G["ent_h"])
        np.add.at(out["ent"], t, G["ent_t"])
        np.add.at(out["rel"], r, G["rel"])
        if model == "transh":
            np.add.at(out["normal_vector"], r, G["normal_vector"])
        if model == "transd":
            np.add.at(out["ent_transfer"], h, G["ent_transfer_h"])
            np.add.at(out["ent_transfer"], t, G["ent_transfer_t"])
            np.add.at(out["rel_transfer"], r, G["rel_transfer"])
        named["ent"][h[on]] = True
        named["ent"][t[on]] = True
        named["rel"][r[on]] = True
    for k, like in PLANE1[model].items():
        named[k] = named[like].copy()
    loss = float(_rowsum(np.where(valid, P["loss"], 0).astype(dtype), form))
    return loss, out, named


def named_rows(model, tabs, pos, side, neg_ent):
    """{table: bool [rows]}: the rows a valid row names (its positive, its live slots, its relation) in every table."""
    base = AR.named_rows(tabs, pos, side, neg_ent)
    return dict(base, **{k: base[like].copy() for k, like in PLANE1[model].items()})


def sgd_step(model, tabs, pos, side, neg_ent, lr, margin, alpha, l1=True, dtype=np.float64, form="ref"):
    """(new tables, loss): every gradient on the pre-step tables, duplicates summed, row -= lr * sum."""
    loss, g, _ = grads(model, tabs, pos, side, neg_ent, margin, alpha, l1, dtype, form)
    lr = np.asarray(lr, dtype=dtype)
    return {k: np.asarray(v, dtype=dtype) - lr * g[k] for k, v in tabs.items()}, loss


def adagrad_step(model, tabs, accs, pos, side, neg_ent, lr, margin, alpha, l1=True, dtype=np.float64, form="ref"):
    """(new tables, new accumulators, loss): per named row acc += s * s, row -= lr * s / sqrt(acc); others as they were."""
    loss, g, named = grads(model, tabs, pos, side, neg_ent, margin, alpha, l1, dtype, form)
    lr = np.asarray(lr, dtype=dtype)
    new_t, new_a = {}, {}
    for k, v in tabs.items():
        v, a, s = np.asarray(v, dtype=dtype), np.asarray(accs[k], dtype=dtype), g[k]
        acc = a + s * s
        upd = v - lr * s / np.sqrt(acc)
        rows = named[k][:, None]
        new_a[k], new_t[k] = np.where(rows, acc, a), np.where(rows, upd, v)
    return new_t, new_a, loss


def largest_dist(model, tabs, pos, side, neg_ent, l1=True):
    """The largest distance a row's loss is formed from (rotate_ref.bound's `scale`)."""
    P = parts(model, tabs, pos, side, neg_ent, 0.0, 0.0, l1)
    vals = np.concatenate([P["Dp"][P["valid"]], P["Dn"][P["live"]]])
    return float(vals.max()) if vals.size else 0.0


def pairwise_accuracy(model, tabs, held, corr, l1=True):
    """Share of rows with D(held) < D(corr): test_gpu_transx.py's held-out figure."""
    return float((XR.score(model, tabs, held, l1) < XR.score(model, tabs, corr, l1)).mean())


# ------------------------------------------------------------------------------------------ L1 sign stability
SIGN_FACTOR = 32.0


def sign_margin(model, tabs, pos, side, neg_ent):
    """min over every residual coordinate of every live triple of |u_fp64| - SIGN_FACTOR |u_fp32 - u_fp64|, u_fp32 the
    fp32 restatement's residual in the form that deviates more at that coordinate.  > 0: sign(u) is the same in fp64,
    in the fp32 restatement and in any fp32 evaluation whose error is within SIGN_FACTOR times the restatement's."""
    P = parts(model, tabs, pos, side, neg_ent, 0.0, 0.0, True)
    worst = np.inf
    for form in ("ref", "fixed"):
        Q = parts(model, tabs, pos, side, neg_ent, 0.0, 0.0, True, np.float32, form)
        for key, on in (("up", P["valid"]), ("un", P["live"])):
            u64, u32 = P[key][on], Q[key][on].astype(np.float64)
            if u64.size:
                worst = min(worst, float((np.abs(u64) - SIGN_FACTOR * np.abs(u32 - u64)).min()))
    return worst


def sign_stable(model, tabs, pos, side, neg_ent):
    return sign_margin(model, tabs, pos, side, neg_ent) > 0


# ------------------------------------------------------------------------------------------ the GPU tests' cases
E_, R_ = 61, 7
SEEDS = 32                      # consecutive seeds an L1 case may try
# (d, bytes past a 16-byte boundary at which every table starts)
SHAPES = [(1, 0), (3, 0), (4, 0), (30, 0), (32, 0), (64, 0), (100, 0), (128, 0), (200, 0), (1023, 0), (1024, 0), (200, 4)]
LARGE_D = 200                   # from here on a shape is paired with a few K only


def n_teams(d, shift=0):
    """Teams per workgroup: a row is read in d / 4 float4 chunks (d % 4 == 0 on 16-byte aligned tables) or d scalars;
    NT = 32 up to 8 chunks, 16 up to 16, 8 up to 32, 4 above; a wave holds NT / 4 teams."""
    nvec = d // 4 if d % 4 == 0 and shift == 0 else d
    return 32 if nvec <= 8 else 16 if nvec <= 16 else 8 if nvec <= 32 else 4


def ks(d, shift=0):
    nt = n_teams(d, shift)
    team_edges = {e + o for e in (nt // 4, nt) for o in (-1, 0, 1) if e + o >= 1}
    if d >= LARGE_D:
        return sorted({1, 2, 63, 64, 65} | team_edges)
    softmax_edges = {e + o for e in (64, 128, 192, 256, 512, 768) for o in (-1, 0, 1)}
    return sorted({1, 2, 1024} | team_edges | softmax_edges)


def tables(model, E, R, d, seed, scale=None):
    """fp32-representable N(0, scale^2) tables of the model (fp64 arrays).  scale defaults to min(0.5, 1.5 / sqrt(d)): the
    distances of a batch then spread by about 1.5 (L1) or less (L2) around their median at every d, so that at
    gamma = the median neither softplus term saturates and every named row's gradient is far above an fp32 ulp of the
    row (at scale 0.5 and d 1023 a distance lies tens of units from the median and sigma(-30) moves no bit)."""
    rng = np.random.default_rng(seed)
    scale = min(0.5, 1.5 / np.sqrt(d)) if scale is None else scale
    rows = {"ent": E, "rel": R, "normal_vector": R, "ent_transfer": E, "rel_transfer": R}
    return {k: (rng.normal(size=(rows[k], d)) * scale).astype(np.float32).astype(np.float64)
            for k in ("ent", "rel") + XR.EXTRA[model]}


def batch(rng, E, R, B, K):
    """Rows over entities [0, E) and relations [0, R), no positive a self-loop (whose head and tail gradients cancel); with
    B >= 2 both sides are in the batch."""
    h = rng.integers(0, E, B)
    t = (h + 1 + rng.integers(0, max(E - 1, 1), B)) % E
    pos = np.stack([h, t, rng.integers(0, R, B)], 1).astype(np.int32)
    side = rng.integers(0, 2, B).astype(np.int32)
    side[:2] = (0, 1)[:B]
    return pos, side, rng.integers(0, E, (B, K)).astype(np.int32)


def margin_for(model, tabs, pos, side, neg_ent, l1):
    """A margin in the middle of the batch's distances, so that both softplus terms carry weight."""
    P = parts(model, tabs, pos, side, neg_ent, 0.0, 0.0, l1)
    vals = np.concatenate([P["Dp"][P["valid"]], P["Dn"][P["live"]]])
    return float(np.float32(np.median(vals))) if vals.size else 1.0


def build_case(model, l1, E, R, d, B, K, seed0, make_batch=batch, ent_hi=None, rel_hi=None, tweak=None):
    """Tables and a batch from the first of SEEDS consecutive seeds from seed0 on that is sign-stable (L1; any seed for
    L2).  The rows name entities below ent_hi and relations below rel_hi; tweak(tabs) edits the tables in place.
    dict(tabs, pos, side, neg_ent, margin, seed)."""
    for seed in range(seed0, seed0 + SEEDS):
        tabs = tables(model, E, R, d, seed)
        if tweak:
            tweak(tabs)
        pos, side, neg_ent = make_batch(np.random.default_rng(seed + 7919), ent_hi or E, rel_hi or R, B, K)
        if not l1 or sign_stable(model, tabs, pos, side, neg_ent):
            return dict(tabs=tabs, pos=pos, side=side, neg_ent=neg_ent, seed=seed,
                        margin=margin_for(model, tabs, pos, side, neg_ent, l1))
    raise AssertionError("no sign-stable seed in [%d, %d) for %s d=%d B=%d K=%d" % (seed0, seed0 + SEEDS, model, d, B, K))


def step_cases(model, l1, opt, d, shift):
    """(K, B, alpha, seed0) of test_loss_rows_and_one_step_match_the_restatement: B cycles through 65, 3, 1 (3 and 1
    above K = 33), alpha through 0, 1, 5.  No shape needed a smaller B to find a sign-stable seed."""
    out = []
    for n, K in enumerate(ks(d, shift)):
        B = (65, 3, 1)[(n + d) % 3] if K <= 33 else (3, 1)[n % 2]
        alpha = (0.0, 1.0, 5.0)[(n + int(l1) + (opt == "adagrad")) % 3]
        out.append((K, B, alpha, 1000 * d + 40 * K + shift))
    return out


def step_case(model, l1, d, K, B, seed0):
    """The rows name entities below E_ - 4 and relations below R_ - 1: the last rows of every table keep their bits."""
    return build_case(model, l1, E_, R_, d, B, K, seed0, ent_hi=E_ - 4, rel_hi=R_ - 1)


# ---- the other blocks of tests/test_gpu_transx_adv.py
GRID = 2048                     # workgroups of the kernel's capped grid, one row each at a time


def _grid_batch(rng, E, R, B, K):
    """B = GRID + 5: workgroups 0..4 take a second row after their first.  Workgroup 1 takes an invalid row, then a valid
    one; workgroup 2 a valid one, then an invalid one; workgroup 3 two invalid ones; workgroups 0 and 4 two valid ones on
    different sides, one of them with an empty slot and the other with every slot empty.  The invalid rows alone name
    entity E - 1 and relation R - 1."""
    G = GRID
    pos, side, neg_ent = batch(rng, E - 1, R - 1, B, K)
    side[[0, G, 4, G + 4]] = (0, 1, 1, 0)
    neg_ent[G, 1] = -1
    neg_ent[G + 4] = (E, -1, E + 7)
    for row, (p, sd) in {1: ((E - 1, E - 1, R - 1), 2), G + 2: ((E, E - 1, R - 1), 0), 3: ((E - 1, -1, R - 1), 1),
                         G + 3: ((E - 1, E - 1, R), 0)}.items():
        pos[row], side[row] = p, sd
        neg_ent[row] = E - 1
    return pos, side, neg_ent


def grid_case(model, l1, d):
    return build_case(model, l1, E_, R_, d, GRID + 5, 3, 17 + d, make_batch=_grid_batch)


def hot_case(model, l1):
    """B = 64, K = 64 over 5 entities and 2 relations: 4,288 slots on 7 keys, every segment cut by many 32-slot windows
    of the apply stage."""
    return build_case(model, l1, 5, 2, 16, 64, 64, 2)


EMPTY_INVALID = [False, False, True, True, True, True, True, True, False]


def _empty_batch(rng, E, R, B, K):
    """Empty slots (-1 and E), a row with every slot empty, sides 2 and -1, positive ids out of range (rows 2..7 are
    invalid: EMPTY_INVALID).  The invalid rows alone name entity E - 1 and relation R - 1."""
    pos, side, neg_ent = batch(rng, E - 1, R - 1, B, K)
    neg_ent[0, [1, 3]] = (-1, E)
    neg_ent[1, :] = (-1, E, -7, E + 5, -1, 1 << 30)
    for row, (p, s) in {2: ((E - 1, E - 1, R - 1), 2), 3: ((E, E - 1, R - 1), 0), 4: ((E - 1, -1, R - 1), 1),
                        5: ((E - 1, E - 1, R), 0), 6: ((E - 1, E - 1, -1), 1), 7: ((E - 1, E - 1, R - 1), -1)}.items():
        pos[row], side[row] = p, s
        neg_ent[row] = E - 1
    return pos, side, neg_ent


def empty_case(model, l1):
    return build_case(model, l1, 40, 4, 16, 9, 6, 5, make_batch=_empty_batch)


def _below_clamp(tabs):
    tabs["normal_vector"][1] = (tabs["normal_vector"][1] * 1e-8).astype(np.float32).astype(np.float64)


def clamp_case(l1):
    """TransH with relation 1's normal row below the clamp (n.n < 1e-12): n^ = 1e6 n, and the normalisation's second
    term is off.  Relation 1 is in the batch."""
    c = build_case("transh", l1, 30, 3, 12, 9, 5, 11, tweak=_below_clamp)
    n = c["tabs"]["normal_vector"][1]
    assert 0 < (n * n).sum() < XR.EPS and (c["pos"][:, 2] == 1).any()
    return c


def other_cases(model, l1):
    out = {"grid d=8": grid_case(model, l1, 8), "grid d=6": grid_case(model, l1, 6), "hot": hot_case(model, l1),
           "empty": empty_case(model, l1)}
    if model == "transh":
        out["clamp"] = clamp_case(l1)
    return out


# ---- the cases of tests/test_gpu_abi_guard_transx_adv.py (its loops run in the squared norm, which has no sign to keep)
GUARD_E, GUARD_R = 300, 9
GUARD_LOSS = [(1, 1), (65, 5), (2, 257), (2051, 2)]          # (B, K)
GUARD_STEPS = [(1, 1), (65, 5), (3, 257), (2051, 2)]
GUARD_DIMS = ((50, 0), (200, 0), (200, 4))                   # scalar, float4, and the scalar path at d 200 (loss only)


def guard_l1(model, d, B):
    """The norm of a guard case: both norms over each entry point's cases, one per case."""
    return bool((MODELS.index(model) + d // 50 + B) % 2)


def _guard_rows(bad):
    def rows(rng, E, R, B, K):
        """Rows that name entity 0 and E - 1 and relation 0 and R - 1 (row 0 on the tail side, the last row on the head
        side), with an empty slot; bad: the middle row has a side of 2, and beyond the kernel's 2,048 workgroups so has
        row 1, whose workgroup then takes the valid row 2,049."""
        pos = np.stack([rng.integers(1, E - 1, B), rng.integers(1, E - 1, B), rng.integers(0, R, B)], 1).astype(np.int32)
        side = rng.integers(0, 2, B).astype(np.int32)
        neg_ent = rng.integers(1, E - 1, (B, K)).astype(np.int32)
        pos[0], side[0], neg_ent[0, 0] = (0, E - 1, R - 1), 0, E - 1
        pos[-1, 2], side[-1] = (0 if B > 1 else R - 1), 1
        neg_ent[-1, -1] = 0
        if K > 1:
            neg_ent[B // 2, K // 2] = -1
        if bad and B > 2:
            side[B // 2] = 2
        if bad and B > 2048:
            side[1] = 2
        return pos, side, neg_ent
    return rows


def guard_case(model, d, B, K, bad):
    return build_case(model, guard_l1(model, d, B), GUARD_E, GUARD_R, d, B, K, 7 * d + B + K, make_batch=_guard_rows(bad))


def guard_cases(model):
    """Every single-call case of the guard file: name -> (l1, case)."""
    out = {}
    for B, K in GUARD_LOSS:
        for d, shift in GUARD_DIMS:
            out["loss d=%d B=%d K=%d" % (d, B, K)] = (guard_l1(model, d, B), guard_case(model, d, B, K, True))
    for B, K in GUARD_STEPS:
        for d, shift in GUARD_DIMS[:2]:
            out["step d=%d B=%d K=%d" % (d, B, K)] = (guard_l1(model, d, B), guard_case(model, d, B, K, B > 2048))
    return out
