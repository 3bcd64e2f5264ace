"""AdaGrad on the IndexedSlices of holE.py:296, restated in fp64: TF1's AdagradOptimizer(lr, initial_accumulator_value)
with duplicates summed first (_apply_sparse_duplicate_indices).  The gradient is oracle.hole_oracle.hinge_grads (read, not
changed); per distinct row named by the step

    s = sum of its gradient rows,   accum[row] += s * s,   table[row] -= lr * s / sqrt(accum[row])   (no epsilon).

A row that no hinge-active pair names is not touched in either array (TensorFlow adds a zero there)."""
import numpy as np

from oracle import hole_oracle as O


def apply_rows(table, accum, idx, grad, lr):
    """In place on fp64 `table` / `accum`: idx [R] (entries < 0 or >= N skipped), grad [R,d] the gradient rows.
    Returns (the per-row sums [N,d], the mask [N] of the rows named)."""
    N = table.shape[0]
    idx = np.asarray(idx, dtype=np.int64)
    ok = (idx >= 0) & (idx < N)
    s = np.zeros_like(table)
    np.add.at(s, idx[ok], np.asarray(grad, dtype=np.float64)[ok])
    named = np.zeros(N, bool)
    named[idx[ok]] = True
    accum[named] += s[named] ** 2
    table[named] -= lr * s[named] / np.sqrt(accum[named])
    return s, named


def step(table, accum, pos, neg, lr, margin=0.2, max_norm=1.0, model="complex"):
    """One training step in place on fp64 `table` / `accum`.  Returns (loss [B], per-row sums [N,d], rows touched [N]):
    only the gradient rows of hinge-active pairs (loss > 0) name a row."""
    idx, val, loss = O.hinge_grads(pos, neg, table, margin, max_norm, model)
    live = np.tile(loss > 0, 6)
    s, named = apply_rows(table, accum, np.where(live, idx, -1), val, lr)
    return loss, s, named
