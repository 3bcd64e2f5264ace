"""GPU: what ge_softmax_sampled_loss and ge_softmax_sampled_grad may touch -- the cases of tests/test_gpu_abi_guard.py for
the two writing entry points of the sampled softmax objective, built with its drive() / claimed() and tests/abi_guard.py:
guard-banded buffers of EXACTLY the declared sizes (the table included), 0x00 / 0xFF poison, bitwise-equal runs,
`need - 1` -> GE_ENOMEM, the workspace offset by 16 bytes -> GE_EINVAL, outputs still poison after a refusal, the table
unchanged; the results against tests/softmax_sampled_ref.py within the bound of tests/test_gpu_softmax_sampled.py
(8 e32 + 1e-7).

The cases register in test_gpu_abi_guard.GUARDED at import, which is what its test_every_writing_entry_point_is_guarded
reads: the two files are collected together (`pytest tests -m gpu`)."""
import numpy as np
import pytest
import torch

import test_gpu_abi_guard as G
import test_gpu_softmax_sampled as TS
from graphembeddings_amd import _lib
from tests import softmax_sampled_ref as SS

pytestmark = pytest.mark.gpu

I32, F32 = np.int32, np.float32
# (512, 4095, 8): with the appended row and candidate B1 = 513, K1 = 4096 -- sm_split(K1, B1) * K1 = sm_gc_rows(B1, K1) =
# 32,768 (csrc/ge_softmax_route.h): the candidate-side partials, the workspace's last part, end on its last row
SHAPES = [(1, 1, 8), (65, 129, 64), (130, 300, 200), (512, 4095, 8)]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")
    G.CALLED.clear()


def inputs(B, K, d, head):
    """The case of tests/test_gpu_softmax_sampled.py with an invalid row and a candidate outside the table appended."""
    t, hr, true, cand = TS.build(B, K, d, 1.0, head)
    N = t.shape[0]
    hr = np.concatenate([hr, [[N, 0]]]).astype(I32)
    true = np.concatenate([true, true[:1]]).astype(I32)
    cand = np.concatenate([cand, [N + 2]]).astype(I32)
    return t, hr, true, cand


def bound(t, hr, true, cand, scale, head, ref):
    l32, _, v32 = SS.evaluate(t, hr, true, cand, 1.0, scale, head, dtype=np.float32)
    return 8 * np.nanmax(np.abs(l32 - ref[0])) + 1e-7, 8 * np.abs(v32 - ref[2]).max() + 1e-7


@G.guards("ge_softmax_sampled_loss")
@pytest.mark.parametrize("head", [0, 1])
@pytest.mark.parametrize("B,K,d", SHAPES)
def test_softmax_sampled_loss(B, K, d, head):
    scale = 20.0
    t, hr, true, cand = inputs(B, K, d, head)
    N, B1, K1 = t.shape[0], B + 1, K + 1
    need = int(_lib.load().ge_softmax_sampled_workspace_bytes(B1, K1, d))
    assert need > 0 and need % 256 == 0
    ref = SS.evaluate(t, hr, true, cand, 1.0, scale, bool(head))
    bl, _ = bound(t, hr, true, cand, scale, bool(head), ref)

    def case(A, mode):
        tb, hb, ib, cb = A.data("table", t), A.data("hr", hr), A.data("true_id", true), A.data("cand", cand)
        loss, w = A.out("loss", 4 * B1), A.ws("workspace", need)
        rc = A.call("ge_softmax_sampled_loss", tb.ptr, N, d, hb.ptr, B1, ib.ptr, cb.ptr, K1, 1.0, scale, 0, head, loss.ptr,
                    *G.ws_args(w, mode), G.S())
        torch.cuda.synchronize()
        assert np.array_equal(tb.get(F32, (N, d)).view(I32), t.view(I32))
        return rc

    def verify(A):
        loss = A["loss"].get(F32)
        assert np.isnan(loss[B]) and np.isnan(ref[0][B])
        G.near(9, np.abs(loss[:B] - ref[0][:B]), bl)
    G.drive(case, verify, ws=True)
    G.claimed(test_softmax_sampled_loss)


@G.guards("ge_softmax_sampled_grad")
@pytest.mark.parametrize("head", [0, 1])
@pytest.mark.parametrize("B,K,d", SHAPES)
def test_softmax_sampled_grad(B, K, d, head):
    scale, lr = 20.0, 0.25
    t, hr, true, cand = inputs(B, K, d, head)
    N, B1, K1 = t.shape[0], B + 1, K + 1
    R = K1 + 3 * B1
    need = int(_lib.load().ge_softmax_sampled_workspace_bytes(B1, K1, d))
    ref = SS.evaluate(t, hr, true, cand, 1.0, scale, bool(head), lr=lr)
    bl, bg = bound(t, hr, true, cand, scale, bool(head), SS.evaluate(t, hr, true, cand, 1.0, scale, bool(head)))

    def case(A, mode):
        tb, hb, ib, cb = A.data("table", t), A.data("hr", hr), A.data("true_id", true), A.data("cand", cand)
        loss, gi, gv, w = A.out("loss", 4 * B1), A.out("grad_idx", 4 * R), A.out("grad_val", 4 * R * d), A.ws("workspace", need)
        rc = A.call("ge_softmax_sampled_grad", tb.ptr, N, d, hb.ptr, B1, ib.ptr, cb.ptr, K1, 1.0, scale, lr, 0, head, loss.ptr,
                    gi.ptr, gv.ptr, *G.ws_args(w, mode), G.S())
        torch.cuda.synchronize()
        assert np.array_equal(tb.get(F32, (N, d)).view(I32), t.view(I32))
        return rc

    def verify(A):
        loss, gi, gv = A["loss"].get(F32), A["grad_idx"].get(I32), A["grad_val"].get(F32, (R, d))
        assert np.isnan(loss[B]) and np.array_equal(gi, ref[1])
        assert gi[K] == -1 and not gv[K].any() and (gi[-3:] == -1).all() and not gv[-3:].any()
        G.near(9, np.abs(loss[:B] - ref[0][:B]), bl)
        G.near(9, np.abs(gv - ref[2]), lr * bg)
    G.drive(case, verify, ws=True)
    G.claimed(test_softmax_sampled_grad)
