"""GPU: what ge_softmax_masked_loss and ge_softmax_masked_grad may touch -- the cases of tests/test_gpu_abi_guard.py for
the two writing entry points of the type-constrained softmax objective, built with its drive() / claimed() and
tests/abi_guard.py: guard-banded buffers of EXACTLY the declared sizes (the table, the mask and the row sets included),
0x00 / 0xFF poison, bitwise-equal runs, `need - 1` -> GE_ENOMEM, the workspace offset by 16 bytes -> GE_EINVAL, outputs
still poison after a refusal, the table, the mask and the row sets unchanged; the results against
tests/softmax_masked_ref.py within the bound of tests/test_gpu_softmax_masked.py (8 e32 + 1e-7).

The cases register in test_gpu_abi_guard.GUARDED at import, which is what its test_every_writing_entry_point_is_guarded
reads: the two files are collected together (`pytest tests -m gpu`)."""
import numpy as np
import pytest
import torch

import test_gpu_abi_guard as G
import test_gpu_softmax_masked as TM
from graphembeddings_amd import _lib
from tests import softmax_masked_ref as MR

pytestmark = pytest.mark.gpu

I32, F32 = np.int32, np.float32
SHAPES = [(1, 1, 8), (65, 129, 64), (130, 300, 200)]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")
    G.CALLED.clear()


def inputs(B, K, d, head):
    """The case of tests/test_gpu_softmax_masked.py with a row of a bad set id and a candidate outside the table (which
    every set admits) appended.  The mask has exactly n_sets * ge_candidate_mask_words(K + 1) words."""
    t, hr, true, cand, rs, sets = TM.build(B, K, d, 1.0, head)
    N = t.shape[0]
    hr = np.concatenate([hr, hr[:1]]).astype(I32)
    true = np.concatenate([true, true[:1]]).astype(I32)
    cand = np.concatenate([cand, [N + 2]]).astype(I32)
    rs = np.concatenate([rs, [len(sets)]]).astype(I32)
    sets = np.concatenate([sets, np.ones((len(sets), 1), bool)], 1)
    return t, hr, true, cand, rs, sets


def bound(t, hr, true, cand, scale, head, rs, sets, ref):
    l32, _, v32 = MR.evaluate(t, hr, true, cand, 1.0, scale, head, rs, sets, dtype=np.float32)
    ok = ~np.isnan(ref[0])
    return 8 * np.abs(l32 - ref[0])[ok].max() + 1e-7, 8 * np.abs(v32 - ref[2]).max() + 1e-7


def unchanged(bufs, t, rs, mask):
    tb, rb, mb = bufs
    assert np.array_equal(tb.get(F32, t.shape).view(I32), t.view(I32))
    assert np.array_equal(rb.get(I32), rs) and np.array_equal(mb.get(I32, mask.shape), mask.view(I32))


@G.guards("ge_softmax_masked_loss")
@pytest.mark.parametrize("head", [0, 1])
@pytest.mark.parametrize("B,K,d", SHAPES)
def test_softmax_masked_loss(B, K, d, head):
    scale = 20.0
    t, hr, true, cand, rs, sets = inputs(B, K, d, head)
    mask = MR.pack(sets, True)
    N, B1, K1 = t.shape[0], B + 1, K + 1
    lib = _lib.load()
    need = int(lib.ge_softmax_masked_workspace_bytes(B1, K1, d))
    assert need > 0 and need % 256 == 0 and mask.shape[1] == lib.ge_candidate_mask_words(K1)
    ref = MR.evaluate(t, hr, true, cand, 1.0, scale, bool(head), rs, sets)
    bl, _ = bound(t, hr, true, cand, scale, bool(head), rs, sets, ref)

    def case(A, mode):
        tb, hb, ib, cb = A.data("table", t), A.data("hr", hr), A.data("true_id", true), A.data("cand", cand)
        rb, mb = A.data("row_set", rs), A.data("mask", mask.view(I32))
        loss, w = A.out("loss", 4 * B1), A.ws("workspace", need)
        rc = A.call("ge_softmax_masked_loss", tb.ptr, N, d, hb.ptr, B1, ib.ptr, cb.ptr, K1, 1.0, scale, 0, head, loss.ptr,
                    *G.ws_args(w, mode), rb.ptr, mb.ptr, len(sets), G.S())
        torch.cuda.synchronize()
        unchanged((tb, rb, mb), t, rs, mask)
        return rc

    def verify(A):
        loss = A["loss"].get(F32)
        assert np.isnan(loss[B]) and np.isnan(ref[0][B])
        G.near(9, np.abs(loss[:B] - ref[0][:B]), bl)
    G.drive(case, verify, ws=True)
    G.claimed(test_softmax_masked_loss)


@G.guards("ge_softmax_masked_grad")
@pytest.mark.parametrize("head", [0, 1])
@pytest.mark.parametrize("B,K,d", SHAPES)
def test_softmax_masked_grad(B, K, d, head):
    scale, lr = 20.0, 0.25
    t, hr, true, cand, rs, sets = inputs(B, K, d, head)
    mask = MR.pack(sets, True)
    N, B1, K1 = t.shape[0], B + 1, K + 1
    R = K1 + 2 * B1
    need = int(_lib.load().ge_softmax_masked_workspace_bytes(B1, K1, d))
    ref = MR.evaluate(t, hr, true, cand, 1.0, scale, bool(head), rs, sets, lr=lr)
    bl, bg = bound(t, hr, true, cand, scale, bool(head), rs, sets, MR.evaluate(t, hr, true, cand, 1.0, scale, bool(head), rs, sets))

    def case(A, mode):
        tb, hb, ib, cb = A.data("table", t), A.data("hr", hr), A.data("true_id", true), A.data("cand", cand)
        rb, mb = A.data("row_set", rs), A.data("mask", mask.view(I32))
        loss, gi, gv, w = A.out("loss", 4 * B1), A.out("grad_idx", 4 * R), A.out("grad_val", 4 * R * d), A.ws("workspace", need)
        rc = A.call("ge_softmax_masked_grad", tb.ptr, N, d, hb.ptr, B1, ib.ptr, cb.ptr, K1, 1.0, scale, lr, 0, head, loss.ptr,
                    gi.ptr, gv.ptr, *G.ws_args(w, mode), rb.ptr, mb.ptr, len(sets), G.S())
        torch.cuda.synchronize()
        unchanged((tb, rb, mb), t, rs, mask)
        return rc

    def verify(A):
        loss, gi, gv = A["loss"].get(F32), A["grad_idx"].get(I32), A["grad_val"].get(F32, (R, d))
        assert np.isnan(loss[B]) and np.array_equal(gi, ref[1])
        assert gi[K] == -1 and not gv[K].any() and (gi[-2:] == -1).all() and not gv[-2:].any()
        G.near(9, np.abs(loss[:B] - ref[0][:B]), bl)
        G.near(9, np.abs(gv - ref[2]), lr * bg)
    G.drive(case, verify, ws=True)
    G.claimed(test_softmax_masked_grad)
