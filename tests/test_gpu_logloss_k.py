"""The --log_loss native loop (ge_train_steps_logloss) and the single-step entry point at negative ratios of 16 to
1024, against the fp64 oracle replay of tests/logloss_cases.py: every loss entry of every step, every table row, and
the negatives of all K corrupted batches.  At these ratios most gradient slots of a step belong to rows cut into several
work items of 16 (summed through float atomics), rows run across sort-tile boundaries, and the last tile may hold a
single unit -- none of which the K <= 3 tests of test_gpu_parity.py reach.

Bounds (logloss_cases.py): loss 3e-5 * max(1, |loss|max); table max(2e-5, 4 * D32) with D32 the oracle's own
fp32-vs-fp64 deviation on the case, measured on the host.  Nothing is excluded from a comparison except the NaN
losses of the invalid-id test, which are asserted to be NaN exactly where the replay says so."""
import numpy as np
import pytest
import torch

import logloss_cases as LC
from oracle import hole_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")
    from graphembeddings_amd import hole
    return hole


def dev(a, dtype=None):
    t = torch.as_tensor(np.array(a))          # (a copy: the cases' arrays are read-only)
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def type_tables(H, id_to_type=None):
    _, itt, offsets, ids = LC.type_arrays()
    return H.TypeTables.from_host(np.array(itt if id_to_type is None else id_to_type), offsets, ids, padded_size=1024)


def check_losses(got, want, what):
    worst = 0.0
    for s, (g, w) in enumerate(zip(got, want)):
        tol = LC.loss_tol(w)
        err = float(np.abs(g - w).max())
        worst = max(worst, err / tol)
        assert err < tol, f"{what}: step {s}: loss off by {err:.3g} (bound {tol:.3g}) at entry {int(np.abs(g - w).argmax())}"
    print(f"{what}: largest loss deviation {worst:.3f} of its bound")


def check_table(got, want, tol, counts, what):
    """every row of the table; on a miss, say which slot classes of the last step the rows belong to"""
    err = np.abs(got.astype(np.float64) - want).max(1)
    print(f"{what}: largest table deviation {err.max():.3g}, bound {tol:.3g}")
    assert np.isfinite(err).all(), f"{what}: non-finite rows {np.nonzero(~np.isfinite(err))[0][:8]}"
    bad = np.nonzero(err >= tol)[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} rows beyond {tol:.3g} (worst {err.max():.3g} in row {int(err.argmax())}); "
                           f"last step's slot classes of these rows: {LC.class_of_rows(counts, bad)}")


def case_trainer(H, c):
    tri, table = LC.workload(c.B, c.d, c.tri_seed)
    emb = dev(table).clone()
    tr = H.Trainer(emb, dev(tri), type_tables(H), c.B, learning_rate=LC.LR0, decay_steps=LC.DECAY_STEPS,
                   decay_rate=LC.DECAY_RATE, seed=LC.SEED).enable_log_loss(c.K, c.l2)
    tr.global_step = LC.GS0
    return tr, emb


# ---------------------------------------------------------------- a
@pytest.mark.parametrize("name", [c.name for c in LC.CASES])
def test_native_loop_matches_fp64_at_large_k(H, name):
    """20 dependent steps in two run() calls (the carried scalar restarts at 1 in the second; config5_small also
    crosses a prepare chunk of 16 steps inside it): every step's loss vector, the final table, and the K corrupted
    batches of the last step bit for bit (Philox step keys gs * K + k for every k < K)."""
    c = LC.BY_NAME[name]
    M = LC.units(c)
    t64, olosses = LC.case_replay(name)
    bats = LC.case_batches(name)
    tr, emb = case_trainer(H, c)
    losses = torch.cat([tr.run(n, keep_losses=True) for n in LC.CALLS], 0).cpu().numpy()
    torch.cuda.synchronize()
    assert losses.shape == (LC.STEPS, M)
    check_losses(losses, olosses, name)
    counts = LC.slot_counts(LC.step_triples(*bats[-1]), t64.shape[0])
    check_table(emb.cpu().numpy(), t64, LC.table_tol(c.d32), counts, name)
    neg = tr._neg.cpu().numpy()
    assert neg.shape == (c.K, c.B, 3) and neg.dtype == np.int32
    assert np.array_equal(neg, bats[-1][1])
    tr.close()


# ---------------------------------------------------------------- b
@pytest.mark.parametrize("name", ["one_tile_full", "tile_plus_k1024"])
def test_single_step_api_at_large_k(H, name):
    """LogLossSGD.step (ge_complex_logloss_step: no prepared record, the float-atomic scatter) on the case's first
    batch with all its K corrupted batches, against one oracle step; then lr = 0 leaves the table bit-identical.
    The table bound is the cases' rule with the one-step fp32-vs-fp64 deviation of the oracle, computed here."""
    c = LC.BY_NAME[name]
    _, table = LC.workload(c.B, c.d, c.tri_seed)
    pos, negs = LC.case_batches(name)[0]
    lr = LC.learning_rate(LC.GS0)
    new, oloss = O.logloss_step(table.astype(np.float64), pos, negs, float(lr), c.l2)
    new32, _ = O.logloss_step(np.array(table), pos, negs, np.float32(lr), np.float32(c.l2))
    d32 = float(np.abs(new32.astype(np.float64) - new).max())
    emb = dev(table).clone()
    opt = H.LogLossSGD(emb, l2_regularization=c.l2)
    loss = opt.step(dev(pos), dev(negs), float(lr)).cpu().numpy()
    assert loss.shape == (LC.units(c), 1)
    check_losses([loss[:, 0]], [oloss], name + " single step")
    counts = LC.slot_counts(LC.step_triples(pos, negs), table.shape[0])
    check_table(emb.cpu().numpy(), new, LC.table_tol(d32), counts, name + " single step")
    before = emb.clone()
    opt.step(dev(pos), dev(negs), 0.0)
    torch.cuda.synchronize()
    assert torch.equal(emb, before)


# ---------------------------------------------------------------- c
@pytest.mark.parametrize("l2,steps,min_crossings,scale_lo,scale_hi",
                         [(0.1, 27, 2, 1e23, 1e26), (0.00947265625, 12, 1, 1e-21, 1e-19)])
def test_scalar_leaves_its_range_mid_run(H, l2, steps, min_crossings, scale_lo, scale_hi):
    """B 512, K 1, lr 0.1 constant: l2 = 0.1 makes the dense factor -9.24 (the reference's own defaults), l2 =
    0.00947... makes it 0.03.  In ONE run() call the carried scalar then leaves [9.1e-13, 1.1e12] in the middle of the
    run -- at step indices 12 and 25 of 27, and at 7 of 12 -- so the table is re-materialised there and that step's
    factor is applied by a dense pass (train_logloss_run's dense_now branch), after which the scalar starts again.
    The final table (about 3e24, about 1.5e-20) follows the fp64 replay to 1e-4 of its scale: max(1e-4, 4 x the
    oracle's fp32-vs-fp64 relative deviation, 1.8e-6 and 1.1e-5 measured on the host).
    The growing case found a bug: once rows passed 2^42 the gradient kernel's un-clipped score and sums of squares
    overflowed fp32 and inf * 0 left NaN in every row a step named (complex_logloss_grad_kernel now reads such rows
    scaled down by a power of two)."""
    from graphembeddings_amd import data as D
    fb, id_to_type, offsets, ids = LC.type_arrays()
    B, K, d = 512, 1, 64
    cross = LC.scalar_crossings(0.1, l2, (1 + K) * B, steps)
    print("crossings at step indices", cross)
    assert len([s for s in cross if 0 < s < steps - 1]) >= min_crossings
    tri = D.synthetic_fb15k_triples(fb, n_triples=8 * B, seed=23)
    table = O.init_table(fb.entity_count, d, seed=10)
    emb = dev(table).clone()
    tr = H.Trainer(emb, dev(tri), type_tables(H), B, learning_rate=0.1, decay_rate=0.0, seed=3).enable_log_loss(K, l2)
    tr.run(steps)
    torch.cuda.synchronize()
    bats = LC.batches(tri, B, K, steps, 3, 0)
    t64, _ = LC.replay(table, bats, float(np.float32(l2)), gs0=0, lr0=0.1, decay_steps=0.0)
    scale = float(np.abs(t64).max())
    assert np.isfinite(t64).all() and scale_lo < scale < scale_hi
    got = emb.cpu().numpy().astype(np.float64)
    print(f"l2 {l2}: scale {scale:.3g}, largest deviation {np.abs(got - t64).max() / scale:.3g} of it, bound 1e-4")
    assert np.isfinite(got).all()
    assert np.abs(got - t64).max() < 1e-4 * scale
    tr.close()


# ---------------------------------------------------------------- d
def test_dense_factor_exactly_zero(H):
    """lr 0.125, M 1024, l2 2^-7: lr M l2 is exactly 1, the dense factor exactly 0.  After one step every row that no
    triple of the step names is 0 (or -0) and the others are -lr * gradient; a second step starts from that table.
    Bound: 1e-4 of the compared rows' scale = max(1e-4, 4 x 3.5e-7, the oracle's fp32-vs-fp64 relative deviation)."""
    from graphembeddings_amd import data as D
    fb, id_to_type, offsets, ids = LC.type_arrays()
    B, K, d, lr, l2 = 512, 1, 64, 0.125, 2.0 ** -7
    M = (1 + K) * B
    assert 1.0 - float(np.float32(lr)) * M * float(np.float32(l2)) == 0.0
    tri = D.synthetic_fb15k_triples(fb, n_triples=8 * B, seed=23)
    table = O.init_table(fb.entity_count, d, seed=10)
    emb = dev(table).clone()
    tr = H.Trainer(emb, dev(tri), type_tables(H), B, learning_rate=lr, decay_rate=0.0, seed=3).enable_log_loss(K, l2)
    bats = LC.batches(tri, B, K, 2, 3, 0)
    t64 = table.astype(np.float64)
    for s in range(2):
        t64, _ = LC.replay(t64, bats[s:s + 1], l2, gs0=s, lr0=lr, decay_steps=0.0)
        tr.run(1)
        torch.cuda.synchronize()
        got = emb.cpu().numpy()
        touched = np.zeros(len(table), bool)
        touched[LC.step_triples(*bats[s]).reshape(-1)] = True
        assert (got[~touched] == 0).all()
        nz, onz = np.nonzero((got != 0).any(1))[0], np.nonzero((t64 != 0).any(1))[0]
        assert len(onz) == LC.ZERO_FACTOR_ROWS[s]
        if s == 0:      # (in the second step four rows of 1e-22 are below what fp32 products of 1e-20 can hold)
            assert np.array_equal(nz, onz)
        scale = float(np.abs(t64[touched]).max())
        err = float(np.abs(got.astype(np.float64) - t64)[touched].max())
        print(f"step {s}: {len(onz)} non-zero rows, scale {scale:.3g}, largest deviation {err / scale:.3g} of it, bound 1e-4")
        assert scale > 0 and err < 1e-4 * scale
    tr.close()


# ---------------------------------------------------------------- e
def test_invalid_ids_in_the_logloss_loop(H):
    """About 5 % of the entity ids lose their type: corrupting such an entity gives the id -1 (the reference's default
    row of -1s), so a fifth of a step's triples are invalid.  Their loss is NaN, they contribute no gradient slot and
    no sort key, and the dense factor still counts all M triples."""
    iv = LC.INVALID
    id_to_type, tri, table, bats = LC.invalid_workload()
    t64, olosses, bad = LC.invalid_replay()
    for b in bad:
        assert b.sum() >= 20 and b.mean() <= 0.25
    M = (1 + iv.K) * iv.B
    emb = dev(table).clone()
    tr = H.Trainer(emb, dev(tri), type_tables(H, id_to_type), iv.B, learning_rate=LC.LR0, decay_steps=LC.DECAY_STEPS,
                   decay_rate=LC.DECAY_RATE, seed=LC.SEED).enable_log_loss(iv.K, iv.l2)
    tr.global_step = LC.GS0
    losses = tr.run(iv.steps, keep_losses=True).cpu().numpy()
    torch.cuda.synchronize()                                   # a HIP error of any launch of the loop surfaces here
    assert losses.shape == (iv.steps, M)
    for s in range(iv.steps):
        assert np.array_equal(np.isnan(losses[s]), bad[s]), s
    check_losses([l[~b] for l, b in zip(losses, bad)], [o[~b] for o, b in zip(olosses, bad)], "invalid ids")
    counts = LC.slot_counts(LC.step_triples(*bats[-1]), len(table))
    check_table(emb.cpu().numpy(), t64, LC.table_tol(iv.d32), counts, "invalid ids")
    assert np.array_equal(tr._neg.cpu().numpy(), bats[-1][1])
    tr.close()


# ---------------------------------------------------------------- f
def test_only_last_loss_kept_and_chunk_crossing(H):
    """one_tile_full for 40 steps in one call without keep_losses: a one-tile prepare chunk holds 32 steps, so the run
    crosses into a second chunk, and the table's sum of squares is taken for the last step only."""
    c = LC.BY_NAME["one_tile_full"]
    t64, olosses = LC.case_replay(c.name, LC.LONG_STEPS)
    bats = LC.case_batches(c.name, LC.LONG_STEPS)
    tr, emb = case_trainer(H, c)
    out = tr.run(LC.LONG_STEPS)
    torch.cuda.synchronize()
    assert out.data_ptr() == tr.last_loss.data_ptr() and tuple(tr.last_loss.shape) == (LC.units(c),)
    check_losses([tr.last_loss.cpu().numpy()], [olosses[-1]], "40 steps")
    counts = LC.slot_counts(LC.step_triples(*bats[-1]), t64.shape[0])
    check_table(emb.cpu().numpy(), t64, LC.table_tol(LC.D32_LONG), counts, "40 steps")
    assert np.array_equal(tr._neg.cpu().numpy(), bats[-1][1])
    tr.close()
