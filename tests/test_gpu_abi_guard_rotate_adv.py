"""GPU: what the ge_rotate_adv_* entry points (RotatE's self-adversarial loss) may touch -- the cases of
tests/test_gpu_abi_guard.py for their six writing entry points, built with its drive() / claimed() and
tests/abi_guard.py: guard-banded tables, accumulators, outputs and workspaces of EXACTLY the declared sizes, 0x00 / 0xFF
poison, bitwise-equal runs, `need - 1` -> GE_ENOMEM, the workspace offset by 16 bytes -> GE_EINVAL, outputs still poison
after a refusal.  rel and acc_rel are [n_rel, d / 2]: a write of a d-wide relation row to relation R - 1 (which every step
case names) lands in the tail guard.  The results against tests/rotate_adv_ref.py within test_gpu_rotate_adv.py's bound
(rotate_ref.bound: 8 e32 + 1e-7, e32 the larger of the restatement's two forms).

The cases register in test_gpu_abi_guard.GUARDED at import, which is what its test_every_writing_entry_point_is_guarded
reads: the files are collected together (`pytest tests -m gpu`)."""
import numpy as np
import pytest
import torch

import test_gpu_abi_guard as G
from graphembeddings_amd import _lib
from oracle import transx_oracle as TO
from tests import rotate_adv_ref as AR
from tests import rotate_ref as RR

pytestmark = pytest.mark.gpu

I32, F32 = np.int32, np.float32
A0 = 0.1
LR = float(np.float32(0.05))
GAMMA, ALPHA = 3.0, 1.0
FAMILY = 28                                     # G.near's family of these cases


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")
    G.CALLED.clear()


def near(got, ref64, a32, b32, scale=0.0):
    """test_gpu_rotate_adv.py's rule through G.near: |got - ref64| <= rotate_ref.bound with the float32 form that deviates more."""
    bound, base, e32 = RR.bound(ref64, AR.worse32(ref64, a32, b32), scale)
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref64, dtype=np.float64))
    if np.any(err > base):
        print("ULP-TERM guard: |err| %.4g above 8 e32 + 1e-7 = %.4g (e32 %.4g, largest |ref| %.4g, scale %.4g)"
              % (float(err.max()), float(base.min()), e32, float(np.abs(ref64).max()), scale))
    G.near(FAMILY, err, bound)


def rtabs(E, R, d, seed):
    rng = np.random.default_rng(seed)
    return {"ent": (rng.standard_normal((E, d)) * 0.5).astype(F32), "rel": rng.uniform(-np.pi, np.pi, (R, d // 2)).astype(F32)}


def rargs(A, l1, tabs, kind="in", shift=0):
    b = {k: A.data(k, v, kind, shift) for k, v in tabs.items()}
    return (int(l1), b["ent"].ptr, tabs["ent"].shape[0], b["rel"].ptr, tabs["rel"].shape[0], tabs["ent"].shape[1])


def aargs(A, l1, tabs):
    a = rargs(A, l1, tabs, "table")
    accs = {k: A.table("acc_" + k, np.full(v.shape, A0, F32)) for k, v in tabs.items()}
    return (*a[:-1], accs["ent"].ptr, accs["rel"].ptr, a[-1])


def rows_of(E, R, B, K, seed, bad=False):
    """Rows that name entity 0 and E - 1 and relation 0 and R - 1 (row 0 on the tail side, the last row on the head side),
    with an empty slot; bad: the middle row has a side of 2, and beyond the gradient kernel's 2,048 workgroups so has row 1,
    whose workgroup then takes the valid row 2,049."""
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.integers(1, E - 1, B), rng.integers(1, E - 1, B), rng.integers(0, R, B)], 1).astype(I32)
    side = rng.integers(0, 2, B).astype(I32)
    neg_ent = rng.integers(1, E - 1, (B, K)).astype(I32)
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


@G.guards("ge_rotate_adv_loss")
@pytest.mark.parametrize("B,K", [(1, 1), (3, 33), (65, 5), (2, 257), (2051, 2)])
def test_rotate_adv_loss(B, K):
    """out [B] of exactly 4 B bytes; d = 50 takes the scalar path, d = 200 the vector one, shift = 4 the scalar one at
    d = 200 too."""
    E, R = 300, 9
    for d, shift in ((50, 0), (200, 0), (200, 4), (2, 0)):
        for l1 in (True, False):
            tabs = rtabs(E, R, d, seed=d + B)
            pos, side, neg_ent = rows_of(E, R, B, K, seed=B + K, bad=True)
            t64 = G.f64(tabs)
            ref = AR.row_losses(t64, pos, side, neg_ent, GAMMA, ALPHA, l1)
            a32 = AR.row_losses(t64, pos, side, neg_ent, GAMMA, ALPHA, l1, F32, "tail")
            b32 = AR.row_losses(t64, pos, side, neg_ent, GAMMA, ALPHA, l1, F32, "head")
            bad_rows = list(np.nonzero(np.isnan(ref))[0])

            def case(A, mode):
                a = rargs(A, l1, tabs, shift=shift)
                return A.call("ge_rotate_adv_loss", *a, A.data("pos", pos).ptr, A.data("side", side).ptr,
                              A.data("neg_ent", neg_ent).ptr, B, K, GAMMA, ALPHA, A.out("out", 4 * B).ptr, G.S())

            def verify(A):
                got = A["out"].get(F32)
                ok = G.check_nan_rows(got, bad_rows)
                near(got[ok], ref[ok], a32[ok], b32[ok], scale=AR.largest_dist(t64, pos, side, neg_ent, l1))
            G.drive(case, verify)
    G.claimed(test_rotate_adv_loss)


@G.guards("ge_rotate_adv_step", "ge_rotate_adv_adagrad_step")
@pytest.mark.parametrize("B,K", [(1, 1), (65, 5), (3, 257), (2051, 2)])
def test_rotate_adv_single_steps(B, K):
    """d = 50 takes the scalar kernels, d = 200 the float4 ones, d = 520 the float4 gradient kernel's 64-lane teams (65
    chunks: lane 0 holds a second one), d = 134 the scalar one's (67 chunks).  B = 2,051: three workgroups take a second
    row, one of them after an invalid first one."""
    E, R = 300, 9
    lib = _lib.load()
    pos, side, neg_ent = rows_of(E, R, B, K, seed=B + K, bad=B > 2048)
    for entry in ("ge_rotate_adv_step", "ge_rotate_adv_adagrad_step"):
        ada = entry.endswith("adagrad_step")
        for d in (50, 200, 520, 134):
            for l1 in (True, False):
                tabs = rtabs(E, R, d, seed=d + B)
                need = int(lib.ge_rotate_adv_step_workspace_bytes(E, R, d, B, K))
                assert need > 0 and need % 256 == 0
                t64 = G.f64(tabs)
                a64 = {k: np.full(v.shape, np.float64(F32(A0))) for k, v in tabs.items()}
                if ada:
                    f = lambda **kw: AR.adagrad_step(t64, a64, pos, side, neg_ent, LR, GAMMA, ALPHA, l1, **kw)
                    (rt, ra, rloss), (st, sa, sloss), (ut, ua, uloss) = f(), f(dtype=F32, form="tail"), f(dtype=F32, form="head")
                else:
                    f = lambda **kw: AR.sgd_step(t64, pos, side, neg_ent, LR, GAMMA, ALPHA, l1, **kw)
                    (rt, rloss), (st, sloss), (ut, uloss) = f(), f(dtype=F32, form="tail"), f(dtype=F32, form="head")
                named = AR.named_rows(t64, pos, side, neg_ent)

                def case(A, mode):
                    a = aargs(A, l1, tabs) if ada else rargs(A, l1, tabs, "table")
                    p, s, n = A.data("pos", pos), A.data("side", side), A.data("neg_ent", neg_ent)
                    loss, w = A.out("loss", 4), A.ws("workspace", need)
                    return A.call(entry, *a, p.ptr, s.ptr, n.ptr, B, K, GAMMA, ALPHA, LR, loss.ptr, *G.ws_args(w, mode), G.S())

                def verify(A):
                    near(A["loss"].get(F32)[:1], [rloss], [sloss], [uloss], scale=AR.largest_dist(t64, pos, side, neg_ent, l1))
                    for k in tabs:
                        after = A[k].get(F32, tabs[k].shape)
                        near(after, rt[k], st[k], ut[k])
                        G.unnamed_rows_unchanged(tabs[k], after, np.nonzero(named[k])[0])
                        ends = (0, -1) if k == "ent" or B > 1 else (-1,)    # (B = 1 names relation R - 1 alone)
                        assert all((after[r] != tabs[k][r]).any() for r in ends), k   # row 0 and the last row were updated
                        if ada:
                            acc = A["acc_" + k].get(F32, tabs[k].shape)
                            near(acc, ra[k], sa[k], ua[k])
                            G.unnamed_rows_unchanged(np.full(tabs[k].shape, A0, F32), acc, np.nonzero(named[k])[0])
                            assert all((acc[r] > F32(A0)).any() for r in ends), k
                G.drive(case, verify, ws=True)
    G.claimed(test_rotate_adv_single_steps)


def _sampler_args(A, tri32, idx):
    return (A.data("triples", tri32).ptr, len(tri32), A.data("bh_key", idx.bh_key).ptr, A.data("bh_ent", idx.bh_ent).ptr,
            A.data("bt_key", idx.bt_key).ptr, A.data("bt_ent", idx.bt_ent).ptr, len(tri32), A.data("thr", idx.tail_threshold).ptr)


@G.guards("ge_rotate_adv_draw_batch")
@pytest.mark.parametrize("B,K", [(1, 1), (255, 3), (257, 64), (5, 1024)])
def test_rotate_adv_draw(B, K):
    """pos [B,3], side [B] and neg_ent [B,K] of exactly their sizes, equal to the restatement's."""
    tri, E, R = G.loop_kg()
    idx = TO.BernoulliIndex(tri, 0, E, R)
    tri32 = tri.astype(I32)
    seed, step = 21, 4
    want = AR.draw(tri32, idx, seed, step, B, K)

    def case(A, mode):
        s = _sampler_args(A, tri32, idx)
        pos, side, neg = A.out("pos", 12 * B), A.out("side", 4 * B), A.out("neg_ent", 4 * B * K)
        return A.call("ge_rotate_adv_draw_batch", *s[:2], B, *s[2:], R, E, seed, step, K, pos.ptr, side.ptr, neg.ptr, G.S())

    def verify(A):
        assert np.array_equal(A["pos"].get(I32, (B, 3)), want[0]) and np.array_equal(A["side"].get(I32), want[1])
        assert np.array_equal(A["neg_ent"].get(I32, (B, K)), want[2])
    G.drive(case, verify)
    G.claimed(test_rotate_adv_draw)


@G.guards("ge_rotate_adv_train_steps", "ge_rotate_adv_train_steps_adagrad")
@pytest.mark.parametrize("B,K", [(255, 3), (257, 17), (1025, 4)])
def test_rotate_adv_train_steps(B, K):
    """Three steps on the restatement's draws: every loss and the final tables and accumulators against the fp64 replay,
    with e32 taken from the same replay run in float32 in both forms."""
    lib = _lib.load()
    tri, E, R = G.loop_kg()
    idx = TO.BernoulliIndex(tri, 0, E, R)
    tri32 = tri.astype(I32)
    seed, first, STEPS, D = 21, 4, G.STEPS, G.D_LOOP
    D += D % 2
    draws = [AR.draw(tri32, idx, seed, first + s, B, K) for s in range(STEPS)]
    tabs = rtabs(E, R, D, seed=B)
    need = int(lib.ge_rotate_adv_step_workspace_bytes(E, R, D, B, K))
    assert need > 0
    for entry in ("ge_rotate_adv_train_steps", "ge_rotate_adv_train_steps_adagrad"):
        ada = entry.endswith("adagrad")

        def case(A, mode):
            a = aargs(A, False, tabs) if ada else rargs(A, False, tabs, "table")
            losses, w = A.out("losses", 4 * STEPS), A.ws("workspace", need)
            return A.call(entry, *a, *_sampler_args(A, tri32, idx), seed, first, STEPS, B, K, GAMMA, ALPHA, LR, losses.ptr,
                          *G.ws_args(w, mode), G.S())

        def verify(A):
            runs = []
            for dtype, form in ((np.float64, "tail"), (F32, "tail"), (F32, "head")):
                t, a, ls = G.f64(tabs), {k: np.full(v.shape, np.float64(F32(A0))) for k, v in tabs.items()}, []
                for p_, s_, n_ in draws:
                    if ada:
                        t, a, loss = AR.adagrad_step(t, a, p_, s_, n_, LR, GAMMA, ALPHA, False, dtype, form)
                    else:
                        t, loss = AR.sgd_step(t, p_, s_, n_, LR, GAMMA, ALPHA, False, dtype, form)
                    ls.append(loss)
                runs.append((t, a, ls))
            (rt, ra, rl), (st, sa, sl), (ut, ua, ul) = runs
            near(A["losses"].get(F32), rl, sl, ul)
            for k in tabs:
                near(A[k].get(F32, tabs[k].shape), rt[k], st[k], ut[k])
                if ada:
                    near(A["acc_" + k].get(F32, tabs[k].shape), ra[k], sa[k], ua[k])
        G.drive(case, verify, ws=True)
    G.claimed(test_rotate_adv_train_steps)
