"""GPU: what the ge_transx_adv_* entry points (the self-adversarial loss of TransE / TransH / TransD) may touch -- the
cases of tests/test_gpu_abi_guard.py for their five writing entry points, built with its drive() / claimed() and
tests/abi_guard.py: guard-banded tables, accumulators, outputs and workspaces of EXACTLY the declared sizes, 0x00 / 0xFF
poison, bitwise-equal runs, `need - 1` -> GE_ENOMEM, the workspace offset by 16 bytes -> GE_EINVAL, outputs still poison
after a refusal.  The workspace is the model's own size: TransE's has one gradient plane, so a write to a second plane
lands in its tail guard.  The results against tests/transx_adv_ref.py within test_gpu_transx_adv.py's bound
(rotate_ref.bound: 8 e32 + 1e-7, e32 the largest over the restatement's float32 forms); the single-call cases come from
transx_adv_ref.guard_case (sign-stable where the norm is L1), the loops run in the squared norm.

The cases register in test_gpu_abi_guard.GUARDED at import, which is what its test_every_writing_entry_point_is_guarded
reads: the files are collected together (`pytest tests -m gpu`)."""
import numpy as np
import pytest
import torch

import test_gpu_abi_guard as G
from graphembeddings_amd import _lib
from oracle import transx_oracle as TO
from tests import rotate_ref as RR
from tests import transx_adv_ref as AR

pytestmark = pytest.mark.gpu

I32, F32 = np.int32, np.float32
A0 = 0.1
LR = float(np.float32(0.05))
ALPHA = 1.0
FAMILY = 29                                     # G.near's family of these cases
NAMES = ("ent", "rel", "normal_vector", "ent_transfer", "rel_transfer")


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")
    G.CALLED.clear()


def near(got, ref64, r32, scale=0.0):
    """test_gpu_transx_adv.py's rule through G.near: |got - ref64| <= rotate_ref.bound with the float32 form (of the list
    r32, one per transx_adv_ref.FORMS32) that deviates most."""
    bound, base, e32 = RR.bound(ref64, AR.worst32(ref64, *r32), scale)
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref64, dtype=np.float64))
    if np.any(err > base):
        print("ULP-TERM guard: |err| %.4g above 8 e32 + 1e-7 = %.4g (e32 %.4g, largest |ref| %.4g, scale %.4g)"
              % (float(err.max()), float(base.min()), e32, float(np.abs(ref64).max()), scale))
    G.near(FAMILY, err, bound)


def f32(tabs):
    return {k: v.astype(F32) for k, v in tabs.items()}


def aargs(A, model, l1, tabs):
    """G.xargs with the five accumulator arguments in front of d (absent tables: null)."""
    a = G.xargs(A, model, l1, tabs, "table")
    accs = {k: A.table("acc_" + k, np.full(v.shape, A0, F32)) for k, v in tabs.items()}
    return (*a[:-1], *[accs[k].ptr if k in accs else None for k in NAMES], a[-1])


def ws_need(model, E, R, d, B, K):
    need = int(_lib.load().ge_transx_adv_step_workspace_bytes(AR.MODELS.index(model), E, R, d, B, K))
    assert need > 0 and need % 256 == 0
    return need


@G.guards("ge_transx_adv_loss")
@pytest.mark.parametrize("B,K", AR.GUARD_LOSS)
@pytest.mark.parametrize("model", AR.MODELS)
def test_transx_adv_loss(model, B, K):
    """out [B] of exactly 4 B bytes; d = 50 takes the scalar path, d = 200 the float4 one, shift = 4 the scalar one at
    d = 200 too."""
    for d, shift in AR.GUARD_DIMS:
        l1 = AR.guard_l1(model, d, B)
        c = AR.guard_case(model, d, B, K, True)
        t64, tabs = c["tabs"], f32(c["tabs"])
        pos, side, neg_ent, gamma = c["pos"], c["side"], c["neg_ent"], c["margin"] - 1.0   # (off the median: B = K = 1 cancels there)
        ref = AR.row_losses(model, t64, pos, side, neg_ent, gamma, ALPHA, l1)
        r32 = [AR.row_losses(model, t64, pos, side, neg_ent, gamma, ALPHA, l1, F32, form) for form in AR.FORMS32]
        bad_rows = list(np.nonzero(np.isnan(ref))[0])

        def case(A, mode):
            a = G.xargs(A, model, l1, tabs, shift=shift)
            return A.call("ge_transx_adv_loss", *a, A.data("pos", pos).ptr, A.data("side", side).ptr,
                          A.data("neg_ent", neg_ent).ptr, B, K, gamma, ALPHA, A.out("out", 4 * B).ptr, G.S())

        def verify(A):
            got = A["out"].get(F32)
            ok = G.check_nan_rows(got, bad_rows)
            near(got[ok], ref[ok], [x[ok] for x in r32], scale=AR.largest_dist(model, t64, pos, side, neg_ent, l1))
        G.drive(case, verify)
    G.claimed(test_transx_adv_loss)


@G.guards("ge_transx_adv_step", "ge_transx_adv_adagrad_step")
@pytest.mark.parametrize("B,K", AR.GUARD_STEPS)
@pytest.mark.parametrize("model", AR.MODELS)
def test_transx_adv_single_steps(model, B, K):
    """d = 50 takes the scalar kernels, d = 200 the float4 ones.  B = 2,051: three workgroups take a second row, one of
    them after an invalid first one."""
    E, R = AR.GUARD_E, AR.GUARD_R
    for d, _ in AR.GUARD_DIMS[:2]:
        l1 = AR.guard_l1(model, d, B)
        c = AR.guard_case(model, d, B, K, B > 2048)
        t64, tabs = c["tabs"], f32(c["tabs"])
        pos, side, neg_ent, gamma = c["pos"], c["side"], c["neg_ent"], c["margin"] - 1.0   # (off the median: B = K = 1 cancels there)
        need = ws_need(model, E, R, d, B, K)
        named = AR.named_rows(model, t64, pos, side, neg_ent)
        scale = AR.largest_dist(model, t64, pos, side, neg_ent, l1)
        for entry in ("ge_transx_adv_step", "ge_transx_adv_adagrad_step"):
            ada = entry.endswith("adagrad_step")
            a64 = {k: np.full(v.shape, np.float64(F32(A0))) for k, v in tabs.items()}
            if ada:
                f = lambda **kw: AR.adagrad_step(model, t64, a64, pos, side, neg_ent, LR, gamma, ALPHA, l1, **kw)
            else:
                f = lambda **kw: AR.sgd_step(model, t64, pos, side, neg_ent, LR, gamma, ALPHA, l1, **kw)
            r64, r32 = f(), [f(dtype=F32, form=form) for form in AR.FORMS32]      # (tables, [accumulators,] loss)

            def case(A, mode):
                a = aargs(A, model, l1, tabs) if ada else G.xargs(A, model, l1, tabs, "table")
                p, s, n = A.data("pos", pos), A.data("side", side), A.data("neg_ent", neg_ent)
                loss, w = A.out("loss", 4), A.ws("workspace", need)
                return A.call(entry, *a, p.ptr, s.ptr, n.ptr, B, K, gamma, ALPHA, LR, loss.ptr, *G.ws_args(w, mode), G.S())

            def verify(A):
                near(A["loss"].get(F32)[:1], [r64[-1]], [[x[-1]] for x in r32], scale=scale)
                for k in tabs:
                    after = A[k].get(F32, tabs[k].shape)
                    near(after, r64[0][k], [x[0][k] for x in r32])
                    G.unnamed_rows_unchanged(tabs[k], after, np.nonzero(named[k])[0])
                    ends = (0, -1) if len(tabs[k]) == E or B > 1 else (-1,)    # (B = 1 names relation R - 1 alone)
                    assert all((after[r] != tabs[k][r]).any() for r in ends), k   # row 0 and the last row were updated
                    if ada:
                        acc = A["acc_" + k].get(F32, tabs[k].shape)
                        near(acc, r64[1][k], [x[1][k] for x in r32])
                        G.unnamed_rows_unchanged(np.full(tabs[k].shape, A0, F32), acc, np.nonzero(named[k])[0])
                        assert all((acc[r] > F32(A0)).any() for r in ends), k
            G.drive(case, verify, ws=True)
    G.claimed(test_transx_adv_single_steps)


def _sampler_args(A, tri32, idx):
    return (A.data("triples", tri32).ptr, len(tri32), A.data("bh_key", idx.bh_key).ptr, A.data("bh_ent", idx.bh_ent).ptr,
            A.data("bt_key", idx.bt_key).ptr, A.data("bt_ent", idx.bt_ent).ptr, len(tri32), A.data("thr", idx.tail_threshold).ptr)


@G.guards("ge_transx_adv_train_steps", "ge_transx_adv_train_steps_adagrad")
@pytest.mark.parametrize("B,K", [(255, 3), (257, 17)])
@pytest.mark.parametrize("model", AR.MODELS)
def test_transx_adv_train_steps(model, B, K):
    """Three steps on the restatement's draws: every loss and the final tables and accumulators against the fp64 replay,
    with e32 taken from the same replay run in float32 in both forms."""
    tri, E, R = G.loop_kg()
    idx = TO.BernoulliIndex(tri, 0, E, R)
    tri32 = tri.astype(I32)
    seed, first, STEPS, D, gamma = 21, 4, G.STEPS, G.D_LOOP, 3.0
    draws = [AR.draw(tri32, idx, seed, first + s, B, K) for s in range(STEPS)]
    tabs = G.xtabs(model, E, R, D, seed=B)
    need = ws_need(model, E, R, D, B, K)
    for entry in ("ge_transx_adv_train_steps", "ge_transx_adv_train_steps_adagrad"):
        ada = entry.endswith("adagrad")

        def case(A, mode):
            a = aargs(A, model, False, tabs) if ada else G.xargs(A, model, False, tabs, "table")
            losses, w = A.out("losses", 4 * STEPS), A.ws("workspace", need)
            return A.call(entry, *a, *_sampler_args(A, tri32, idx), seed, first, STEPS, B, K, gamma, ALPHA, LR, losses.ptr,
                          *G.ws_args(w, mode), G.S())

        def verify(A):
            runs = []
            for dtype, form in [(np.float64, "ref")] + [(F32, form) for form in AR.FORMS32]:
                t, a, ls = G.f64(tabs), {k: np.full(v.shape, np.float64(F32(A0))) for k, v in tabs.items()}, []
                for p_, s_, n_ in draws:
                    if ada:
                        t, a, loss = AR.adagrad_step(model, t, a, p_, s_, n_, LR, gamma, ALPHA, False, dtype, form)
                    else:
                        t, loss = AR.sgd_step(model, t, p_, s_, n_, LR, gamma, ALPHA, False, dtype, form)
                    ls.append(loss)
                runs.append((t, a, ls))
            (rt, ra, rl), r32 = runs[0], runs[1:]
            near(A["losses"].get(F32), rl, [x[2] for x in r32])
            for k in tabs:
                near(A[k].get(F32, tabs[k].shape), rt[k], [x[0][k] for x in r32])
                if ada:
                    near(A["acc_" + k].get(F32, tabs[k].shape), ra[k], [x[1][k] for x in r32])
        G.drive(case, verify, ws=True)
    G.claimed(test_transx_adv_train_steps)
