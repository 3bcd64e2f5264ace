"""One ComplEx / HolE training step at every instantiation of the shape switch of csrc/ge_complex.hip (twelve (VEC,
LPT, NITER) keys, both ends of each), on every kernel family built from it -- the six-row gradient of the single-step
API, the four-row plan gradient of the loops with and without relation order, the log-loss gradient, each again with
SPEC for HolE in the frequency domain -- and with it every instantiation of the update kernels of csrc/ge_train.hip,
tables off the 16-byte boundary, pairs with an id outside the table, and the widths the kernels refuse.

The cases, the restated dispatch that says which kernel a case runs, and the bounds (the project's bars, checked on
the CPU against the gap between an independent fp32 implementation and the fp64 oracle) are
tests/complex_shape_cases.py's; tests/test_complex_shape_cases_host.py proves them.  References: oracle/hole_oracle.py
(fp64) and tests/adagrad_ref.py.  Negatives replay the loops' Philox keys and are compared bit for bit before anything
else.  `-s` prints every check's largest deviation and its bound."""
import numpy as np
import pytest
import torch

import complex_shape_cases as SC
import logloss_cases as LC
import test_gpu_adagrad as TA
import test_gpu_logloss_k as TL
from graphembeddings_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")
    from graphembeddings_amd import hole
    return hole


def dev(a):
    return torch.as_tensor(np.array(a)).cuda()          # (a copy: the cases' arrays are read-only)


def place(table, offset=0):
    """`table` on the device as a contiguous [N, d] view into a larger 1-D buffer, `offset` bytes past a 16-byte
    boundary."""
    t = torch.as_tensor(np.array(table))
    buf = torch.zeros(t.numel() + 8, dtype=torch.float32, device="cuda")
    view = buf[offset // 4: offset // 4 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == offset and view.is_contiguous()
    return view


def near(test, what, err, bound):
    err = float(err)
    print(f"DEV {test} {what}: {err:.3g} bound {bound:.3g} ratio {err / bound:.3f}")
    assert err < bound, (test, what, err, bound)


def type_tables(H, workload):
    itt, offsets, ids, _ = SC.graph(workload)
    return H.TypeTables.from_host(np.array(itt), np.array(offsets), np.array(ids), padded_size=SC.PADDED)


def case_table(workload, model, d, offset):
    w = SC.WORKLOADS[workload]
    how = SC.route(model, d, SC.alignment_of(offset))
    return SC.table_of(w.N, d, SC.TABLE_SEEDS.get((workload, how, d), 0), how or "complex")


def trainer(H, workload, model, d, offset=0, **kw):
    """The workload's Trainer at the step and row its replay starts from; returns (trainer, its table)."""
    w = SC.WORKLOADS[workload]
    emb = place(case_table(workload, model, d, offset), offset)
    tr = H.Trainer(emb, dev(SC.graph(workload)[3]), type_tables(H, workload), w.B, margin=SC.MARGIN, learning_rate=SC.LR0,
                   decay_steps=SC.DECAY_STEPS, decay_rate=SC.DECAY_RATE, model=model, seed=SC.SEED, **kw)
    tr.global_step, tr.row = w.gs0, w.row0
    return tr, emb


_NEGATIVES_CHECKED = set()


def check_negatives(H, workload):
    """ge_corrupt_batch at the loop's (seed, global step) keys == the replay's negatives, bit for bit (once a workload)."""
    if workload in _NEGATIVES_CHECKED:
        return
    w, tt = SC.WORKLOADS[workload], type_tables(H, workload)
    for pos, neg, gs, _ in SC.batches(workload)[0]:
        for k, n in enumerate(neg.reshape(-1, w.B, 3)):
            step = gs if workload != "logloss" else gs * SC.LOGLOSS_K + k
            got = H.corrupt_batch(tt, w.n_rel, dev(pos), seed=SC.SEED, step=step).cpu().numpy()
            assert np.array_equal(got, n), (workload, gs, k)
    _NEGATIVES_CHECKED.add(workload)


def check_loop(test, workload, how, d, losses, emb, tr):
    """Every step's losses (NaN exactly where the replay has an invalid pair), the table, the row and step the loop
    ends on and the negatives it hands back."""
    w, key = SC.WORKLOADS[workload], (workload, how, d)
    ref = SC.loop_replay(*key)
    loss_bound, table_bound = SC.bounds(key)
    assert losses.shape == (w.steps, w.B)
    worst = 0.0
    for s, want in enumerate(ref.losses):
        bad = np.isnan(want)
        assert np.array_equal(np.isnan(losses[s]), bad), (key, s)
        worst = max(worst, float(np.abs(losses[s][~bad] - want[~bad]).max()))
    near(test, f"{key} loss", worst, loss_bound)
    near(test, f"{key} table", np.abs(emb.cpu().numpy().astype(np.float64) - ref.table).max(), table_bound)
    assert tr.row == ref.row_end and tr.global_step == w.gs0 + w.steps
    assert np.array_equal(tr._neg.cpu().numpy(), SC.batches(workload)[0][-1][1])
    return ref


def run_loop(H, test, workload, model, d, offset=0, det=False):
    w = SC.WORKLOADS[workload]
    how = SC.route(model, d, SC.alignment_of(offset))
    check_negatives(H, workload)
    tr, emb = trainer(H, workload, model, d, offset, deterministic=det)
    losses = tr.run(w.steps, keep_losses=True).cpu().numpy()
    torch.cuda.synchronize()
    ref = check_loop(test, workload, how, d, losses, emb, tr)
    tr.close()
    return losses, emb, ref


def ids_of(runs):
    return ["-".join(str(x) for x in r[1:4]) for r in runs]


# ------------------------------------------------------------------------------------ a: the single step, six-row kernel
@pytest.mark.parametrize("d", sorted(SC.LOW + SC.HIGH))
@pytest.mark.parametrize("model", ["complex", "hole_spectral"])
def test_a_single_step_at_both_ends_of_every_key(H, model, d):
    how, B = SC.step_how(model), SC.STEP_B
    key = ("step", how, d)
    pos, neg = SC.step_batch()
    ref = SC.step_replay(how, d)
    loss_bound, table_bound = SC.bounds(key)
    emb = place(SC.table_of(SC.STEP_N, d, SC.TABLE_SEEDS.get(key, 0), how))
    if model == "hole_spectral":
        H.hole_to_spectral(emb)
    gloss, gi, gv = H.hinge_grad(emb, dev(pos), dev(neg), SC.STEP_LR, margin=SC.MARGIN, model=model)
    # slot order h+, t+, r+, h-, t-, r-; a row both sides share is merged into the positive's slot; inactive pairs: none
    gi, on = gi.cpu().numpy().reshape(B, 6), ref.on[0]
    for X in range(3):
        same = pos[:, X] == neg[:, X]
        assert np.array_equal(gi[:, X], np.where(on, pos[:, X], -1)), (key, X)
        assert np.array_equal(gi[:, 3 + X], np.where(on & ~same, neg[:, X], -1)), (key, X)
    near("a", f"{key} grad loss", np.abs(gloss.cpu().numpy() - ref.losses[0]).max(), loss_bound)
    loss = H.HingeSGD(emb, B, margin=SC.MARGIN, model=model).step(dev(pos), dev(neg), SC.STEP_LR).cpu().numpy()[:, 0]
    near("a", f"{key} loss", np.abs(loss - ref.losses[0]).max(), loss_bound)
    if model == "hole_spectral":
        H.hole_from_spectral(emb)
    near("a", f"{key} table", np.abs(emb.cpu().numpy().astype(np.float64) - ref.table).max(), table_bound)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ b: the one-tile SGD loop
@pytest.mark.parametrize("run", SC.runs_of("b"), ids=ids_of(SC.runs_of("b")))
def test_b_one_tile_loop(H, run):
    """complex_hinge_grad_plan_kernel<SPEC, false, false, ...> + apply_rows_kernel<VW, NJ, false, RW>: `same` pairs,
    direct rows, hot relation rows, a batch that wraps."""
    workload, model, d, offset, det = run
    run_loop(H, "b", workload, model, d, offset, det)


# ------------------------------------------------------------------------------------ c: the multi-tile SGD loop
@pytest.mark.parametrize("run", SC.runs_of("c"), ids=ids_of(SC.runs_of("c")))
def test_c_two_tile_loop(H, run):
    """4100 pairs: the relation-order walk (ORD), the run sums and their merge in LDS, apply_rows_kernel with RW = 0."""
    workload, model, d, offset, det = run
    run_loop(H, "c", workload, model, d, offset, det)


# ------------------------------------------------------------------------------------ d: deterministic mode
@pytest.mark.parametrize("run", SC.runs_of("d"), ids=ids_of(SC.runs_of("d")))
def test_d_deterministic_loop(H, run):
    """apply_rows_kernel<..., DET> + hot_rows_kernel<NJ>: within the bound of the oracle, and two runs bitwise equal."""
    workload, model, d, offset, det = run
    assert det
    first = run_loop(H, "d", workload, model, d, offset, det)
    second = run_loop(H, "d", workload, model, d, offset, det)
    assert np.array_equal(first[0].view(np.int32), second[0].view(np.int32)) and torch.equal(first[1], second[1])


# ------------------------------------------------------------------------------------ e: the log-loss loop
@pytest.mark.parametrize("d", SC.LOW)
def test_e_logloss_loop(H, d):
    w = SC.WORKLOADS["logloss"]
    check_negatives(H, "logloss")
    tr, emb = trainer(H, "logloss", "complex", d)
    tr.enable_log_loss(SC.LOGLOSS_K, SC.LOGLOSS_L2)
    losses = tr.run(w.steps, keep_losses=True).cpu().numpy()
    torch.cuda.synchronize()
    t64, olosses = SC.logloss_replay(d)
    bats, row_end = SC.batches("logloss")
    what = f"DEV e logloss d={d}"
    assert losses.shape == (w.steps, (1 + SC.LOGLOSS_K) * w.B)
    TL.check_losses(losses, olosses, what)
    counts = LC.slot_counts(LC.step_triples(bats[-1][0], bats[-1][1]), w.N)
    TL.check_table(emb.cpu().numpy(), t64, LC.table_tol(SC.LOGLOSS_D32[d]), counts, what)
    assert tr.row == row_end and np.array_equal(tr._neg.cpu().numpy(), bats[-1][1])
    tr.close()


# ------------------------------------------------------------------------------------ f: the AdaGrad loop
@pytest.mark.parametrize("d", SC.LOW)
def test_f_adagrad_loop(H, d):
    """test_gpu_adagrad.py's comparison (every step against the restatement started from the device's own table and
    accumulator, its derived bounds) on `small`: the six-row gradient kernel at lr = 1 and the AdaGrad update kernels."""
    w = SC.WORKLOADS["small"]
    itt, offsets, ids, tri = SC.graph("small")
    tr, emb = trainer(H, "small", "complex", d, optimizer="adagrad", initial_accumulator_value=TA.A0)
    live, _, _ = TA.follow_loop(f"f d={d}", tr, tri, (itt, offsets, ids), w.B, w.steps, SC.MARGIN, "complex", seed=SC.SEED,
                                padded=SC.PADDED, lr_at=SC.learning_rate)
    assert tr.row == SC.batches("small")[1] and all(0.5 < v < 1.0 for v in live)
    torch.cuda.synchronize()
    tr.close()


# ------------------------------------------------------------------------------------ g: tables off the boundary
@pytest.mark.parametrize("run", SC.runs_of("g"), ids=["%s-%d+%d" % (r[1], r[2], r[3]) for r in SC.runs_of("g")])
def test_g_misaligned_table(H, run):
    """The one-tile loop on a table 4 and 8 bytes past a 16-byte boundary: narrower vectors in the gradient kernel
    (another key) and in the update kernel.  Against the oracle, not the aligned run: the lane-local order of the sums
    changes with VEC."""
    workload, model, d, offset, det = run
    run_loop(H, "g", workload, model, d, offset, det)


# ------------------------------------------------------------------------------------ h: pairs with an id of -1
@pytest.mark.parametrize("run", SC.runs_of("h"), ids=ids_of(SC.runs_of("h")))
def test_h_invalid_pairs(H, run):
    """Corrupting an entity of unknown type gives the id -1: the pair's loss is NaN, it has no gradient slot (the
    prepared record drops it) and every other pair and the table are as the oracle has them."""
    workload, model, d, offset, det = run
    losses, _, ref = run_loop(H, "h", workload, model, d, offset, det)
    for row in losses:
        assert 20 <= int(np.isnan(row).sum()) <= SC.WORKLOADS[workload].B // 4


# ------------------------------------------------------------------------------------ i: refusals
def refused_code(fn):
    with pytest.raises(_lib.GeError) as e:
        fn()
    return e.value.code


@pytest.mark.parametrize("d,offset", SC.REFUSED)
def test_i_complex_refuses_and_touches_nothing(H, d, offset):
    """Every entry point of model = complex answers GE_ENOTSUP at a width the shape switch does not take; the table
    and the accumulator are bitwise what they were."""
    w = SC.WORKLOADS["small"]
    pos, neg, _, _ = SC.batches("small")[0][0]
    table = case_table("small", "complex", d, offset)
    emb = place(table, offset)
    before = emb.clone()
    dpos, dneg = dev(pos), dev(neg)
    assert refused_code(lambda: H.evaluate_triples(dpos, emb)) == _lib.GE_ENOTSUP
    assert refused_code(lambda: H.hinge_loss(dpos, dneg, emb, margin=SC.MARGIN)) == _lib.GE_ENOTSUP
    opt = H.HingeSGD(emb, w.B, margin=SC.MARGIN)
    assert refused_code(lambda: opt.step(dpos, dneg, SC.STEP_LR)) == _lib.GE_ENOTSUP
    for kw, log_loss in ((dict(), False), (dict(deterministic=True), False), (dict(lookahead=False), False),
                         (dict(optimizer="adagrad", initial_accumulator_value=SC.A0), False), (dict(), True)):
        tr, _ = trainer(H, "small", "complex", d, offset, **kw)
        assert tr.embeddings.data_ptr() % 16 == offset and torch.equal(tr.embeddings, before)
        if log_loss:
            tr.enable_log_loss(SC.LOGLOSS_K, SC.LOGLOSS_L2)
        assert refused_code(lambda: tr.run(2)) == _lib.GE_ENOTSUP, kw
        torch.cuda.synchronize()
        assert torch.equal(tr.embeddings, before) and tr.global_step == w.gs0 and tr.row == w.row0, kw
        if tr.accumulator is not None:
            assert bool((tr.accumulator == SC.A0).all())
        tr.close()
    torch.cuda.synchronize()
    assert torch.equal(emb, before)


@pytest.mark.parametrize("run", SC.runs_of("i"), ids=["%s-%d+%d" % (r[1], r[2], r[3]) for r in SC.runs_of("i")])
def test_i_hole_trains_on_the_direct_kernels_where_the_shape_is_refused(H, run):
    """model = hole at an even d the ComplEx-shaped kernels refuse, up to 512: the loop runs the direct-correlation
    kernels on the real table (no transform) and matches the HolE oracle."""
    workload, model, d, offset, det = run
    assert SC.route(model, d, SC.alignment_of(offset)) == "direct" and SC.route("complex", d, SC.alignment_of(offset)) is None
    run_loop(H, "i", workload, model, d, offset, det)


@pytest.mark.parametrize("d,offset", [c for c in SC.REFUSED if c not in SC.HOLE_DIRECT])
def test_i_hole_refuses_above_the_direct_kernels_with_the_table_intact(H, d, offset):
    """model = hole beyond both kernel families: GE_ENOTSUP before the forward transform -- the table comes back
    real-valued, bit for bit."""
    w = SC.WORKLOADS["small"]
    assert SC.route("hole", d, SC.alignment_of(offset)) is None and d > SC.HOLE_DIRECT_MAX_DIM
    for kw in (dict(), dict(lookahead=False), dict(deterministic=True)):
        tr, emb = trainer(H, "small", "hole", d, offset, **kw)
        before = emb.clone()
        assert refused_code(lambda: tr.run(2)) == _lib.GE_ENOTSUP
        torch.cuda.synchronize()
        assert torch.equal(emb, before) and tr.global_step == w.gs0, kw
        tr.close()


@pytest.mark.parametrize("d,offset", SC.REFUSED)
def test_i_resident_spectral_trainer_refuses_with_the_spectrum_intact(H, d, offset):
    """spectral_resident=True transforms in the constructor; run() refuses and leaves the spectral table bit for bit,
    and to_real() gives back the original within test_hole_spectral_transform_round_trip's bound."""
    table = case_table("small", "hole", d, offset)
    tr, emb = trainer(H, "small", "hole", d, offset, spectral_resident=True)
    torch.cuda.synchronize()
    spectrum = emb.clone()
    assert not torch.equal(spectrum, dev(table))
    assert refused_code(lambda: tr.run(2)) == _lib.GE_ENOTSUP
    torch.cuda.synchronize()
    assert torch.equal(emb, spectrum)
    tr.to_real()
    assert np.abs(emb.cpu().numpy() - table).max() < 2e-6 * max(1.0, float(np.abs(table).max()))
    torch.cuda.synchronize()
    tr.close()
