"""GPU: AdaGrad for ComplEx and HolE -- ge_adagrad_rows, HingeAdaGrad.step and the native loop ge_train_steps_adagrad
against the fp64 restatement tests/adagrad_ref.py (TF1's AdagradOptimizer on the IndexedSlices of holE.py:296).

Workload: a synthetic table of 300 rows (10 relation rows, 4 entity types), rows scaled to norms in [0.5, 2] so that the
clip's Jacobian runs, one zero row.

Bounds (derived, not measured on the code under test).  The single-step bound TABLE_TOL = 5e-6 at lr = 0.1
(test_gpu_parity.py) implies an error in the summed gradient s of at most DELTA = 5e-5 per element; s -> s / sqrt(a + s^2)
has slope at most 1 / sqrt(a0):
    table        lr * DELTA / sqrt(a0)                      (1.6e-5 at lr = 0.1, a0 = 0.1)
    accumulator  2 * max|s| * DELTA + 4 ulp(accumulator)    (max|s| of the row, from the restatement)
and for a row of more than 16 gradient rows in a step (a hot row, whose sum is far larger) DELTA is scaled by
max(1, max|s|) of that row.  Losses: SCORE_TOL = 1e-5.  The loop is compared step by step, the restatement re-seeded from
the device's own fp32 table and accumulator before every step.  Every check prints its largest error / bound (`-s`)."""
import numpy as np
import pytest
import torch

from oracle import hole_oracle as O
from tests import adagrad_ref as AR

pytestmark = pytest.mark.gpu

SCORE_TOL, DELTA, A0, LR0 = 1e-5, 5e-5, 0.1, 0.1
N, NREL, NTYPES, ZERO_ROW = 300, 10, 4, 17
SEED, PADDED = 21, 64
F32, I32 = np.float32, np.int32
WORST = {}


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")
    from graphembeddings_amd import hole
    return hole


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def table_of(d, seed=3, n=N):
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((n, d))
    t *= (rng.uniform(0.5, 2.0, (n, 1)) / np.linalg.norm(t, axis=1, keepdims=True))
    t[ZERO_ROW] = 0.0
    return t.astype(F32)


def types_of(n=N):
    """Rows [0, NREL) are relations (type -1), entity e has type e % NTYPES."""
    id_to_type = np.full(n, -1, I32)
    ent = np.arange(NREL, n)
    id_to_type[ent] = ent % NTYPES
    lists = [ent[ent % NTYPES == t] for t in range(NTYPES)]
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return id_to_type, offsets, np.concatenate(lists).astype(I32)


def triples_of(T, seed, n=N, one_relation=False):
    rng = np.random.default_rng(seed)
    rel = np.full(T, 3) if one_relation else rng.integers(0, NREL, T)
    return np.stack([rng.integers(NREL, n, T), rng.integers(NREL, n, T), rel], 1).astype(I32)


def lr_at(gs, decay_steps=50.0, decay_rate=0.5):
    return float(F32(LR0) / (F32(1.0) + F32(decay_rate) * (F32(gs) / F32(decay_steps))))


def near(what, err, bound):
    ratio = float(np.max(np.asarray(err, np.float64) / bound)) if np.size(err) else 0.0
    if ratio > WORST.get(what, 0.0):
        WORST[what] = ratio
        print("DEV %s: err/bound %.4g, largest |err| %.4g" % (what, ratio, float(np.max(err))))
    assert np.all(err < bound), (what, float(np.max(err)), float(np.max(bound)), ratio)


def check_update(what, got_t, got_a, ref_t, ref_a, s, counts, lr):
    """The bounds of the module docstring, per row: counts [n] = gradient rows of the step that name the row."""
    smax = np.abs(s).max(1, keepdims=True)
    delta = DELTA * np.where(counts[:, None] > 16, np.maximum(1.0, smax), 1.0)
    near(what + " table", np.abs(got_t - ref_t), np.broadcast_to(lr * delta / np.sqrt(A0), ref_t.shape))
    ulp = np.spacing(ref_a.astype(F32)).astype(np.float64)
    near(what + " accumulator", np.abs(got_a - ref_a), 2.0 * smax * delta + 4.0 * ulp)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(I32), np.asarray(b).view(I32))


def slot_counts(pos, neg, n=N):
    """Gradient rows of one hinge step per table row: the positive's three rows and the negative's differing one."""
    r = np.concatenate([pos.ravel(), neg[pos != neg]])
    return np.bincount(r, minlength=n)


# ------------------------------------------------------------------------------------ ge_adagrad_rows
def rows_case(d, R, hot=0, seed=0):
    rng = np.random.default_rng(seed + 7 * d + R)
    idx = rng.integers(0, N, R).astype(I32)
    if R > 1:
        idx[rng.permutation(R)[:R // 10]] = -1              # empty slots
        idx[rng.permutation(R)[:40]] = 5                    # a row of more than 16 occurrences
        idx[R // 2] = N + 3                                 # one id out of range
        idx[R // 3] = N - 1
        idx[R // 4] = 0
    if hot:
        idx[rng.permutation(R)[:hot]] = 123
    val = (rng.standard_normal((R, d)) * 0.3).astype(F32)
    return idx, val


@pytest.mark.parametrize("d,R,hot", [(d, R, 0) for d in (7, 50, 200, 264) for R in (1, 600)] + [(200, 6000, 5990)])
def test_adagrad_rows_against_the_restatement(H, d, R, hot):
    idx, val = rows_case(d, R, hot)
    if hot:
        assert np.count_nonzero(idx == 123) >= 5990
    table, lr = table_of(d), 0.1
    accum = np.full((N, d), A0, F32)
    accum[::7] += F32(0.37)                                 # not every row at its first step
    ref_t, ref_a = table.astype(np.float64), accum.astype(np.float64)
    s, named = AR.apply_rows(ref_t, ref_a, idx, -val.astype(np.float64), lr)      # val holds MINUS the gradient
    ok = (idx >= 0) & (idx < N)
    counts = np.bincount(idx[ok], minlength=N)
    assert named.sum() == np.count_nonzero(counts) and (R == 1 or not named.all())
    outs = []
    for _ in range(2):
        t, a = dev(table), dev(accum)
        H.adagrad_rows(t, a, dev(idx), dev(val), lr)
        outs.append((t.cpu().numpy(), a.cpu().numpy()))
    got_t, got_a = outs[0]
    check_update("rows", got_t, got_a, ref_t, ref_a, s, counts, lr)
    assert same_bits(got_t[~named], table[~named]) and same_bits(got_a[~named], accum[~named]), "a row not named changed"
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1]), "two runs differ"
    assert not same_bits(got_t[named], table[named])


# ------------------------------------------------------------------------------------ HingeAdaGrad.step
@pytest.mark.parametrize("model", ["complex", "hole"])
@pytest.mark.parametrize("B", [1, 100])
def test_hinge_adagrad_step(H, model, B):
    d, lr, margin = 50, 0.1, 0.2
    table = table_of(d, seed=B)
    pos = triples_of(B, seed=B + 1)
    rng = np.random.default_rng(B)
    neg = pos.copy()
    side = rng.integers(0, 2, B)
    neg[np.arange(B), side] = rng.integers(NREL, N, B)
    if B > 1:
        neg[3] = pos[3]                                     # a pair whose negative is its positive
        pos[10:14], neg[10:14] = pos[9], neg[9]             # a pair five times
        pos[20, 0] = ZERO_ROW
        neg[20] = pos[20]
        neg[20, 1] = ZERO_ROW
    opt = H.HingeAdaGrad(dev(table), B, margin=margin, model=model, initial_accumulator_value=A0)
    assert opt.accumulator.shape == (N, d) and float(opt.accumulator.min()) == float(opt.accumulator.max()) == F32(A0)
    for _ in range(2):                                   # the second step meets accumulators that have moved
        before_t, before_a = opt.embeddings.cpu().numpy(), opt.accumulator.cpu().numpy()
        ref_t, ref_a = before_t.astype(np.float64), before_a.astype(np.float64)
        loss = opt.step(dev(pos), dev(neg), lr)
        assert loss.shape == (B, 1)
        oloss, s, named = AR.step(ref_t, ref_a, pos, neg, lr, margin, model=model)
        near("step loss", np.abs(loss.cpu().numpy()[:, 0] - oloss), SCORE_TOL)
        got_t, got_a = opt.embeddings.cpu().numpy(), opt.accumulator.cpu().numpy()
        check_update("step " + model, got_t, got_a, ref_t, ref_a, s, slot_counts(pos, neg), lr)
        assert same_bits(got_t[~named], before_t[~named]) and same_bits(got_a[~named], before_a[~named])
        assert named.any() and not named.all()


def test_python_refusals(H):
    emb = dev(table_of(8))
    tri, tt = dev(triples_of(64, 1)), H.TypeTables.from_host(*types_of(), padded_size=PADDED)
    with pytest.raises(ValueError):
        H.Trainer(emb.clone(), tri, tt, 16, model="hole", optimizer="adagrad", spectral_resident=True)
    with pytest.raises(ValueError):
        H.Trainer(emb.clone(), tri, tt, 16, optimizer="adam")
    with pytest.raises(ValueError):
        H.Trainer(emb.clone(), tri, tt, 16, optimizer="adagrad", initial_accumulator_value=0.0)
    with pytest.raises(ValueError):
        H.HingeAdaGrad(emb.clone(), 16, model="hole_spectral")
    tr = H.Trainer(emb.clone(), tri, tt, 16, optimizer="adagrad", initial_accumulator_value=0.25)
    assert tr.accumulator.shape == emb.shape and float(tr.accumulator.min()) == 0.25
    with pytest.raises(ValueError):
        tr.enable_log_loss(1, 0.1)
    ev = H.Events(2)
    with pytest.raises(ValueError):
        tr.run(1, events=ev.handles)
    ev.close()
    assert tr.global_step == 0 and H.Trainer(emb.clone(), tri, tt, 16).accumulator is None
    tr.close()


# ------------------------------------------------------------------------------------ the loop
def make_trainer(H, table, tri, B, model="complex", margin=0.2, lookahead=True, types=None):
    tt = H.TypeTables.from_host(*(types or types_of(len(table))), padded_size=PADDED)
    return H.Trainer(dev(table), dev(tri), tt, B, margin=margin, learning_rate=LR0, decay_steps=50.0, decay_rate=0.5,
                     model=model, seed=SEED, optimizer="adagrad", initial_accumulator_value=A0, lookahead=lookahead)


def state(tr):
    torch.cuda.synchronize()
    return tr.embeddings.cpu().numpy(), tr.accumulator.cpu().numpy()


def compare_loop(H, what, model, B, d, steps=20, one_relation=False, margin=0.2, n=N, warm_up=0, live_range=None):
    """`steps` dependent steps, one run() each, every one against the restatement started from the device's own state."""
    types = types_of(n)
    T = 3 * B + 7                                           # wraps inside the run
    tri = triples_of(T, seed=B + d, n=n, one_relation=one_relation)
    tr = make_trainer(H, table_of(d, n=n), tri, B, model, margin, types=types)
    if warm_up:
        tr.run(warm_up)
    live, counts, crossing = follow_loop(what, tr, tri, types, B, steps, margin, "complex" if model == "complex" else "hole")
    if live_range:
        assert all(live_range[0] <= v <= live_range[1] for v in live), live
    tr.close()
    return live, counts, crossing


def follow_loop(what, tr, tri, types, B, steps, margin, omodel, seed=SEED, padded=PADDED, lr_at=lr_at):
    """compare_loop's comparison on a trainer someone else built (test_gpu_complex_shapes.py): tri, types and the
    schedule lr_at are what it was built from.  Returns (hinge-active share per step, the last step's slot counts,
    whether a hot row crossed the first tile boundary)."""
    n, T = tr.embeddings.shape[0], len(tri)
    row, live, crossing = tr.row, [], False
    for _ in range(steps):
        gs = tr.global_step
        before_t, before_a = state(tr)
        loss = tr.run(1).cpu().numpy()
        got_t, got_a = state(tr)
        if row + B > T:
            row = 0
        pos = tri[row:row + B]
        row += B
        neg = O.corrupt_batch(pos, *types, seed, gs, padded, 0)
        assert np.array_equal(tr._neg.cpu().numpy(), neg)
        ref_t, ref_a = before_t.astype(np.float64), before_a.astype(np.float64)
        oloss, s, named = AR.step(ref_t, ref_a, pos, neg, lr_at(gs), margin, model=omodel)
        near(what + " loss", np.abs(loss - oloss), SCORE_TOL)
        counts = slot_counts(pos, neg, n)
        check_update(what, got_t, got_a, ref_t, ref_a, s, counts, lr_at(gs))
        assert same_bits(got_t[~named], before_t[~named]) and same_bits(got_a[~named], before_a[~named]), "an unnamed row moved"
        live.append(float((oloss > 0).mean()))
        # a row of more than 16 slots whose sorted keys lie on both sides of the first tile boundary (4 x 4096 keys)
        start = np.cumsum(counts) - counts
        crossing |= bool(np.any((counts > 16) & (start < 16384) & (start + counts > 16384)))
    assert tr.row == row
    return live, counts, crossing


@pytest.mark.parametrize("B,d", [(1, 200), (100, 50), (100, 264), (4096, 200), (5000, 200)])
def test_loop_matches_the_restatement_step_by_step(H, B, d):
    live, counts, crossing = compare_loop(H, "loop", "complex", B, d)
    assert B != 5000 or crossing, "no hot row across the tile boundary"


@pytest.mark.parametrize("B,items", [(300, (2, 63)), (1500, (64, 10 ** 6)), (5000, (64, 10 ** 6))])
def test_loop_single_relation_hot_row(H, B, items):
    """One relation for every pair: its row collects B gradient rows a step -- ceil(B / 16) work items, reduced by one
    wave below 64 items and by the eight waves of a workgroup from 64 on; at B = 5000 the step has two tiles."""
    assert items[0] <= -(-B // 16) <= items[1]
    live, counts, crossing = compare_loop(H, "hot row", "complex", B, 200, one_relation=True)
    assert counts[3] == B and (B != 5000 or crossing)


def test_loop_hole_direct(H):
    compare_loop(H, "hole", "hole", 100, 50)
    compare_loop(H, "hole", "hole_direct", 100, 50, steps=3)
    compare_loop(H, "hole odd d", "hole", 100, 7, steps=3)       # 4-byte lanes


def test_loop_sparse_rows_in_a_step_of_two_tiles(H):
    """20,000 rows at B = 5000: most rows have one item, in a record of two tiles (the 300-row table has none there)."""
    live, counts, crossing = compare_loop(H, "two tiles, sparse", "complex", 5000, 50, steps=5, n=20000)
    assert np.count_nonzero((counts > 0) & (counts <= 16)) > 5000


def test_margin_minus_one_touches_nothing(H):
    for B in (100, 5000):
        tri = triples_of(3 * B, seed=B)
        tr = make_trainer(H, table_of(50), tri, B, margin=-1.0)
        t0, a0 = state(tr)
        loss = tr.run(4, keep_losses=True).cpu().numpy()
        t1, a1 = state(tr)
        assert not loss.any() and same_bits(t0, t1) and same_bits(a0, a1)
        tr.close()


def test_loop_with_a_share_of_the_pairs_inactive(H):
    """The rows of this table are clipped to the unit ball, so its scores are small and at the default margin 0.2 every
    pair stays live for hundreds of steps.  At margin 0.02, after 100 warm-up steps of this loop, about half of the
    pairs no longer violate the margin (the fp64 restatement, trained alone: 40-56 % live at B = 100, 51-63 % with one
    relation at B = 300): dead slots inside live items, items without a live slot, parked partial sums of zeros.  The
    live share of every compared step is asserted from the losses."""
    compare_loop(H, "partly live", "complex", 100, 50, warm_up=100, margin=0.02, live_range=(0.2, 0.8))
    compare_loop(H, "partly live, hot row", "complex", 300, 50, warm_up=100, margin=0.02, live_range=(0.2, 0.8), steps=10,
                 one_relation=True)


# ------------------------------------------------------------------------------------ bits
def run_plan(H, plan, B=300, d=50, model="complex", lookahead=True, tri=None):
    tri = triples_of(4 * B + 5, seed=9) if tri is None else tri
    tr = make_trainer(H, table_of(d), tri, B, model, lookahead=lookahead)
    losses = [tr.run(n, keep_losses=True).cpu().numpy() for n in plan]
    out = state(tr) + (np.concatenate(losses),)
    tr.close()
    return out


def equal_runs(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("B", [300, 5000])
def test_loop_is_bitwise_reproducible_however_it_is_called(H, B):
    ref = run_plan(H, [20], B)
    assert not same_bits(ref[0], table_of(50)) and ref[1].min() >= F32(A0) and ref[1].max() > F32(A0) and ref[2].shape == (20, B)
    assert equal_runs(ref, run_plan(H, [20], B)), "two runs from the same state differ"
    assert equal_runs(ref, run_plan(H, [10, 10], B)), "run(10); run(10) is not run(20)"
    assert equal_runs(ref, run_plan(H, [20], B, lookahead=False)), "lookahead=False differs"
    assert equal_runs(ref, run_plan(H, [7, 13], B, lookahead=False))


@pytest.mark.parametrize("model", ["complex", "hole_direct"])
def test_pipeline_handle_of_the_sgd_loop_restarts_cleanly(H, model):
    """One workspace and one handle, first the SGD loop, then this one from where that stopped.  ComplEx: the SGD records
    carry direct tags and no items for rows of one slot -- this loop must not take them for its own.  hole_direct: the
    SGD loop prepares without direct tags too, and its records ARE this loop's."""
    B, d = 300, 50
    tri = triples_of(4 * B + 5, seed=9)
    tt = H.TypeTables.from_host(*types_of(), padded_size=PADDED)
    dtri = dev(tri)
    outs = []
    for shared in (False, True):
        ada = H.Trainer(dev(table_of(d)), dtri, tt, B, learning_rate=LR0, model=model, seed=SEED, optimizer="adagrad",
                        initial_accumulator_value=A0)
        if shared:
            sgd = H.Trainer(dev(table_of(d)), dtri, tt, B, learning_rate=LR0, model=model, seed=SEED)
            sgd.run(3)
            ada.close()
            ada._ws, ada._pipe = sgd._ws, sgd._pipe
        ada.global_step, ada.row = 3, 3 * B
        loss = ada.run(6, keep_losses=True).cpu().numpy()
        outs.append(state(ada) + (loss,))
        if shared:
            ada._pipe = None
            sgd.close()
        else:
            ada.close()
    assert equal_runs(*outs)
    assert outs[0][2].shape == (6, B) and outs[0][2].max() > 0 and not same_bits(outs[0][0], table_of(d))


# ------------------------------------------------------------------------------------ smoke
def test_two_hundred_steps_lower_the_hinge(H):
    B = 100
    tri = triples_of(10 * B, seed=4)
    tr = make_trainer(H, table_of(50), tri, B)
    loss = tr.run(200, keep_losses=True).cpu().numpy().mean(1)
    assert np.isfinite(loss).all() and loss[-20:].mean() < loss[:20].mean(), (loss[:20].mean(), loss[-20:].mean())
    assert float(tr.accumulator.min()) >= F32(A0) and torch.isfinite(tr.embeddings).all()
    tr.close()


# ------------------------------------------------------------------------------------ the driver
def test_training_driver_with_adagrad(tmp_path):
    """train.py --optimizer adagrad end to end on the toy graph of test_gpu_train_eval.py: the checkpoint holds the
    accumulator, --resume_checkpoint restores it (an accumulator only grows), a checkpoint of the SGD loop has none and
    resuming from it says so in one line; --model hole stays on the real table."""
    from graphembeddings_amd import data as D
    from graphembeddings_amd import train as T
    from test_gpu_train_eval import _toy_kg
    dd = tmp_path / "data"
    dd.mkdir()
    data_dir = _toy_kg(dd)
    data = D.init_data(data_dir)
    base = ["--data_dir", data_dir, "--batch_size", "64", "--embedding_dim", "32", "--learning_rate", "0.1", "--margin", "0.5",
            "--padded_size", "64", "--seed", "1"]
    parse = lambda out, extra: T.build_parser().parse_args(base + ["--output_dir", out] + extra)
    out = str(tmp_path / "run")
    res = T.run_training(data, parse(out, ["--optimizer", "adagrad", "--adagrad_init", "0.2", "--num_epochs", "30"]), log=lambda *a: None)
    assert res["steps"] == 30 * (data.triple_count // 64 - 1) and np.isfinite(res["final_mean_hinge"])
    assert res["pocket_loss"] < 0.5                              # started at margin 0.5; learning happened
    emb, gs, acc = T.load_checkpoint(out, device="cpu", with_accumulator=True)
    assert acc is not None and acc.shape == emb.shape and float(acc.min()) >= np.float32(0.2) and float(acc.max()) > np.float32(0.2)
    logs = []
    T.run_training(data, parse(out, ["--optimizer", "adagrad", "--adagrad_init", "0.2", "--num_epochs", "1", "--resume_checkpoint"]),
                   log=lambda *a: logs.append(" ".join(str(x) for x in a)))
    assert not any("AdaGrad accumulator" in l for l in logs)
    _, gs2, acc2 = T.load_checkpoint(out, device="cpu", with_accumulator=True)
    assert gs2 >= gs and bool((acc2 >= acc).all()) and bool((acc2 > acc).any())      # restored, not started over
    # an SGD checkpoint: the file it always was; resuming it with AdaGrad starts the accumulator and says so
    out2 = str(tmp_path / "run_sgd")
    T.run_training(data, parse(out2, ["--num_epochs", "2"]), log=lambda *a: None)
    assert T.load_checkpoint(out2, device="cpu", with_accumulator=True)[2] is None
    logs = []
    T.run_training(data, parse(out2, ["--optimizer", "adagrad", "--num_epochs", "1", "--resume_checkpoint"]),
                   log=lambda *a: logs.append(" ".join(str(x) for x in a)))
    assert sum("AdaGrad accumulator" in l for l in logs) == 1
    assert T.load_checkpoint(out2, device="cpu", with_accumulator=True)[2] is not None
    # HolE at an even width: the real table, no spectral residence
    res = T.run_training(data, parse(str(tmp_path / "run_hole"), ["--optimizer", "adagrad", "--model", "hole", "--num_epochs", "3"]),
                         log=lambda *a: None)
    assert np.isfinite(res["final_mean_hinge"])
