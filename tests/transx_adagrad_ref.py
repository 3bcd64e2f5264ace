"""fp64 restatement of the AdaGrad step of TransE / TransH / TransD for the tests (product code never imports it):
TF1's AdagradOptimizer(lr, initial_accumulator_value).minimize(loss) on the IndexedSlices of every table's lookups, in
place of the GradientDescentOptimizer of tests/transx_ref.sgd_step.  Duplicates are summed first, so per table X with
accumulator A_X and per row that at least one active pair names:

    s = the row of transx_ref.hinge_grads' dense gradient,   A_X[row] += s * s,   X[row] -= lr * s / sqrt(A_X[row])

(the updated accumulator, no epsilon).  A row no active pair names keeps both arrays: its s is zero, but TF's sparse
apply does not visit it at all, and `named` says which rows were visited.  Also the derived error bounds the GPU tests
hold the kernels to.
"""
from __future__ import annotations

import numpy as np

from tests import transx_ref as TR


def named_rows(tabs, pos, neg, active):
    """{table: bool [rows]}: the rows at least one ACTIVE pair names (entities: pos h, pos t, neg h, neg t; relations:
    the pair's relation)."""
    pos, neg = np.asarray(pos, dtype=np.int64), np.asarray(neg, dtype=np.int64)
    act = np.asarray(active, dtype=bool)
    E, R = len(tabs["ent"]), len(tabs["rel"])
    ent, rel = np.zeros(E, bool), np.zeros(R, bool)
    ent[np.concatenate([pos[act, 0], pos[act, 1], neg[act, 0], neg[act, 1]])] = True
    rel[pos[act, 2]] = True
    return {k: (ent if k in ("ent", "ent_transfer") else rel) for k in tabs}


def adagrad_step(model, tabs, accs, pos, neg, lr, margin, l1=True):
    """(new tables fp64, new accumulators fp64, loss, the dense summed gradient): every gradient on the pre-step tables."""
    tabs = {k: np.asarray(v, dtype=np.float64) for k, v in tabs.items()}
    accs = {k: np.asarray(v, dtype=np.float64) for k, v in accs.items()}
    loss, g = TR.hinge_grads(model, tabs, pos, neg, margin, l1)
    named = named_rows(tabs, pos, neg, TR.active_mask(model, tabs, pos, neg, margin, l1))
    new_t, new_a = {}, {}
    for k in tabs:
        rows = named[k][:, None]
        a = accs[k] + g[k] * g[k]
        new_a[k] = np.where(rows, a, accs[k])
        new_t[k] = np.where(rows, tabs[k] - lr * g[k] / np.sqrt(a), tabs[k])
    return new_t, new_a, loss, g


TWO18, TWO22 = 2.0 ** -18, 2.0 ** -22


def bounds(model, tabs, accs, pos, neg, lr, margin, l1=True):
    """({table: bound on |table - ref|}, {table: bound on |accumulator - ref|}) of one fp32 step against adagrad_step
    from the same (fp32-held) state.  delta = 2^-18 * mag bounds the fp32 sum of a row's gradient terms in any order
    (mag = hinge_grads(magnitude=True); tests/fuzz_transx.py takes 2^-20 * mag beside an absolute floor, and no floor
    absorbs small elements here, hence times 4).
      table:        lr * delta / sqrt(a_before) + 2^-22 (|t| + lr)     s -> s / sqrt(a + s^2) has slope <= 1 / sqrt(a)
      accumulator:  2 |g| delta + delta^2 + 2^-22 a_new"""
    new_t, new_a, _, g = adagrad_step(model, tabs, accs, pos, neg, lr, margin, l1)
    _, mag = TR.hinge_grads(model, tabs, pos, neg, margin, l1, magnitude=True)
    bt, ba = {}, {}
    for k in new_t:
        delta = TWO18 * mag[k]
        a_before = np.asarray(accs[k], dtype=np.float64)
        bt[k] = lr * delta / np.sqrt(a_before) + TWO22 * (np.abs(np.asarray(tabs[k], dtype=np.float64)) + lr)
        ba[k] = 2.0 * np.abs(g[k]) * delta + delta * delta + TWO22 * new_a[k]
    return bt, ba
