"""GPU: what ge_transx_adagrad_step and ge_transx_train_steps_adagrad may touch -- the cases of tests/test_gpu_abi_guard.py
for the two writing entry points of the TransX AdaGrad optimizer, built with its drive() / claimed() and
tests/abi_guard.py: guard-banded tables AND accumulators of EXACTLY the declared sizes with row 0 and the last row named
(so a write to row -1 or row N shows), 0x00 / 0xFF poison, bitwise-equal runs, `need - 1` -> GE_ENOMEM, the workspace
offset by 16 bytes -> GE_EINVAL, outputs still poison after a refusal; the results against tests/transx_adagrad_ref.py
within its derived bounds (the loop's intermediate states never leave the device, so its three steps' bounds add up).

The cases register in test_gpu_abi_guard.GUARDED at import, which is what its test_every_writing_entry_point_is_guarded
reads: the two files are collected together (`pytest tests -m gpu`)."""
import numpy as np
import pytest
import torch

import test_gpu_abi_guard as G
from graphembeddings_amd import _lib
from oracle import transx_oracle as TO
from tests import transx_adagrad_ref as AR
from tests import transx_ref as XR

pytestmark = pytest.mark.gpu

I32, F32 = np.int32, np.float32
A0 = 0.1
LR = float(np.float32(0.05))
ACC_ORDER = ("ent", "rel", "normal_vector", "ent_transfer", "rel_transfer")


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")
    G.CALLED.clear()


def aargs(A, model, l1, tabs):
    """The leading arguments of both entry points: G.xargs' tables as guarded in-place buffers, then one guarded
    accumulator of exact size per table the model has (NULL for the others), then d."""
    a = G.xargs(A, model, l1, tabs, "table")
    accs = {k: A.table("acc_" + k, np.full(v.shape, A0, F32)) for k, v in tabs.items()}
    return (*a[:-1], *(accs[k].ptr if k in accs else None for k in ACC_ORDER), a[-1])


def named_ids(k, pos, neg):
    return (pos[:, :2], neg[:, :2]) if k in ("ent", "ent_transfer") else (pos[:, 2],)


@G.guards("ge_transx_adagrad_step")
@pytest.mark.parametrize("B", [1, 65, 257])
def test_transx_adagrad_single_steps(B):
    """pairs_of names entity 0 and E - 1 and relation 0 and R - 1; d = 50 takes the scalar apply, d = 200 the float4 one."""
    E, R = 300, 9
    pos, neg = G.pairs_of(E, R, B, seed=B)
    lib = _lib.load()
    for model in G.XMODELS:
        for d in (50, 200):
            # xtabs at a tenth of its scale (std 0.05): D is then about 10 at d = 200 and an ulp of D (1e-6) stays under
            # the loss bound even at B = 1, where the loss is one z of about 1.  At xtabs' own scale D is about 110, its
            # ulp 7.6e-6, and the hinge term D+ - D- + margin of the (unchanged) gradient kernel cannot meet
            # 5e-6 max(1, |z|): 9.4e-6 was measured there, 1.2 ulp of D.
            tabs = {k: (v * F32(0.1)).astype(F32) for k, v in G.xtabs(model, E, R, d, seed=d + B).items()}
            need = lib.ge_transx_step_workspace_bytes(E, R, d, B)
            assert need > 0
            t64, a64 = G.f64(tabs), {k: np.full(v.shape, np.float64(F32(A0))) for k, v in tabs.items()}
            # the least margin >= 1 at which pairs 0 and 1, which name the first and the last rows, are active with z >= 1
            z0 = XR.score(model, t64, pos[:2], True) - XR.score(model, t64, neg[:2], True)
            margin = float(F32(max(1.0, np.ceil(1.0 - z0.min()))))
            rt, ra, rloss, _ = AR.adagrad_step(model, t64, a64, pos, neg, LR, margin, True)
            bt, ba = AR.bounds(model, t64, a64, pos, neg, LR, margin, True)
            assert XR.active_mask(model, t64, pos, neg, margin, True)[:2].all()

            def case(A, mode):
                a = aargs(A, model, True, tabs)
                p, n = A.data("pos", pos), A.data("neg", neg)
                loss, w = A.out("loss", 4), A.ws("workspace", need)
                return A.call("ge_transx_adagrad_step", *a, p.ptr, n.ptr, B, margin, LR, loss.ptr, *G.ws_args(w, mode), G.S())

            def verify(A):
                G.near(9, abs(float(A["loss"].get(F32)[0]) - rloss), 5e-6 * max(1.0, abs(rloss)))
                for k in tabs:
                    after, acc = A[k].get(F32, tabs[k].shape), A["acc_" + k].get(F32, tabs[k].shape)
                    G.near(9, np.abs(after - rt[k]), bt[k])
                    G.near(9, np.abs(acc - ra[k]), ba[k])
                    G.unnamed_rows_unchanged(tabs[k], after, *named_ids(k, pos, neg))
                    G.unnamed_rows_unchanged(np.full(tabs[k].shape, A0, F32), acc, *named_ids(k, pos, neg))
                    ends = (0, -1) if k in ("ent", "ent_transfer") or B > 1 else (-1,)   # (B = 1 names relation R - 1 alone)
                    assert all((acc[r] > F32(A0)).any() for r in ends), k   # row 0 and the last row were updated
            G.drive(case, verify, ws=True)
    G.claimed(test_transx_adagrad_single_steps)


@G.guards("ge_transx_train_steps_adagrad")
@pytest.mark.parametrize("B", [255, 257, 4097])
def test_transx_adagrad_train_steps(B):
    """Three steps on the oracle's draws: every loss and the final tables and accumulators against the fp64 replay, the
    per-step bounds summed (each taken at the replay's own state of that step)."""
    lib = _lib.load()
    tri, E, R = G.loop_kg()
    idx = TO.BernoulliIndex(tri, 0, E, R)
    tri32 = tri.astype(I32)
    seed, first, margin, STEPS, D = 21, 4, 1.0, G.STEPS, G.D_LOOP
    draws = []
    for s in range(STEPS):
        p_ = tri32[XR.draw_positive_rows(len(tri), B, seed, first + s)]
        draws.append((p_, TO.bernoulli_corrupt_batch(p_, idx, seed, first + s)))

    def sampler_args(A):
        return (A.data("triples", tri32).ptr, len(tri), A.data("bh_key", idx.bh_key).ptr, A.data("bh_ent", idx.bh_ent).ptr,
                A.data("bt_key", idx.bt_key).ptr, A.data("bt_ent", idx.bt_ent).ptr, len(tri), A.data("thr", idx.tail_threshold).ptr)

    for model in G.XMODELS:
        tabs = G.xtabs(model, E, R, D, seed=B)
        need = int(lib.ge_transx_step_workspace_bytes(E, R, D, B))

        def case(A, mode):
            a = aargs(A, model, False, tabs)
            losses, w = A.out("losses", 4 * STEPS), A.ws("workspace", need)
            return A.call("ge_transx_train_steps_adagrad", *a, *sampler_args(A), seed, first, STEPS, B, margin, LR,
                          losses.ptr, *G.ws_args(w, mode), G.S())

        def verify(A):
            rt, ra = G.f64(tabs), {k: np.full(v.shape, np.float64(F32(A0))) for k, v in tabs.items()}
            bt, ba = {k: 0.0 for k in tabs}, {k: 0.0 for k in tabs}
            losses = A["losses"].get(F32)
            for s, (p_, n_) in enumerate(draws):
                st, sa = AR.bounds(model, rt, ra, p_, n_, LR, margin, False)
                rt, ra, rloss, _ = AR.adagrad_step(model, rt, ra, p_, n_, LR, margin, False)
                bt, ba = {k: bt[k] + st[k] for k in tabs}, {k: ba[k] + sa[k] for k in tabs}
                G.near(9, abs(float(losses[s]) - rloss), 5e-6 * max(1.0, abs(rloss)))
            for k in tabs:
                G.near(9, np.abs(A[k].get(F32, tabs[k].shape) - rt[k]), bt[k])
                G.near(9, np.abs(A["acc_" + k].get(F32, tabs[k].shape) - ra[k]), ba[k])
        G.drive(case, verify, ws=True)
    G.claimed(test_transx_adagrad_train_steps)
