"""GPU: what ge_softmax_labels_loss and ge_softmax_labels_grad may touch -- the cases of tests/test_gpu_abi_guard.py for
the two writing entry points of the multi-label softmax objective, built with its drive() / claimed() and
tests/abi_guard.py: guard-banded buffers of EXACTLY the declared sizes (the table, the offsets [B + 1] and the label
positions [L] included), 0x00 / 0xFF poison, bitwise-equal runs, `need - 1` -> GE_ENOMEM, the workspace offset by 16 bytes
-> GE_EINVAL, outputs still poison after a refusal, the table and the labels unchanged; the results against
tests/softmax_labels_ref.py within the bound of tests/test_gpu_softmax_labels.py (8 e32 + 1e-7).

The cases register in test_gpu_abi_guard.GUARDED at import, which is what its test_every_writing_entry_point_is_guarded
reads: the two files are collected together (`pytest tests -m gpu`)."""
import numpy as np
import pytest
import torch

import test_gpu_abi_guard as G
import test_gpu_softmax_labels as TL
from graphembeddings_amd import _lib
from tests import softmax_labels_ref as LR

pytestmark = pytest.mark.gpu

I32, F32 = np.int32, np.float32
SHAPES = [(1, 1, 8), (65, 129, 64), (130, 300, 200)]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")
    G.CALLED.clear()


def inputs(B, K, d, head):
    """The mixed case of tests/test_gpu_softmax_labels.py with a candidate outside the table appended, and two rows: one
    whose label is that candidate's position, one whose last offset points past the label array (the last entry of
    label_off is then NOT L: the kernels may follow neither)."""
    t, hr, off, pos, cand = TL.case(B, K, d, 1.0, bool(head), "mixed")
    N, L = t.shape[0], len(pos)
    hr = np.concatenate([hr, hr[:1], hr[:1]]).astype(I32)
    cand = np.concatenate([cand, [N + 2]]).astype(I32)
    pos = np.concatenate([pos, [K, 0]]).astype(I32)
    off = np.concatenate([off, [L + 1, L + 1000]]).astype(I32)
    return t, hr, off, pos, cand


def bound(t, hr, off, pos, cand, scale, head, ref):
    l32, _, v32 = LR.evaluate(t, hr, off, pos, cand, 1.0, scale, head, dtype=np.float32)
    ok = ~np.isnan(ref[0])
    return 8 * np.abs(l32 - ref[0])[ok].max() + 1e-7, 8 * np.abs(v32 - ref[2]).max() + 1e-7


def unchanged(bufs, t, off, pos):
    tb, ob, pb = bufs
    assert np.array_equal(tb.get(F32, t.shape).view(I32), t.view(I32))
    assert np.array_equal(ob.get(I32), off) and np.array_equal(pb.get(I32), pos)


@G.guards("ge_softmax_labels_loss")
@pytest.mark.parametrize("head", [0, 1])
@pytest.mark.parametrize("B,K,d", SHAPES)
def test_softmax_labels_loss(B, K, d, head):
    scale = 20.0
    t, hr, off, pos, cand = inputs(B, K, d, head)
    N, B1, K1, L = t.shape[0], B + 2, K + 1, len(pos)
    need = int(_lib.load().ge_softmax_labels_workspace_bytes(B1, K1, d, L))
    assert need > 0 and need % 256 == 0
    ref = LR.evaluate(t, hr, off, pos, cand, 1.0, scale, bool(head))
    bl, _ = bound(t, hr, off, pos, cand, scale, bool(head), ref)

    def case(A, mode):
        tb, hb, ob, pb, cb = A.data("table", t), A.data("hr", hr), A.data("label_off", off), A.data("label_pos", pos), A.data("cand", cand)
        loss, w = A.out("loss", 4 * B1), A.ws("workspace", need)
        rc = A.call("ge_softmax_labels_loss", tb.ptr, N, d, hb.ptr, B1, ob.ptr, pb.ptr, L, cb.ptr, K1, 1.0, scale, 0, head,
                    loss.ptr, *G.ws_args(w, mode), G.S())
        torch.cuda.synchronize()
        unchanged((tb, ob, pb), t, off, pos)
        return rc

    def verify(A):
        loss = A["loss"].get(F32)
        assert np.isnan(loss[B:]).all() and np.isnan(ref[0][B:]).all()
        G.near(9, np.abs(loss[:B] - ref[0][:B]), bl)
    G.drive(case, verify, ws=True)
    G.claimed(test_softmax_labels_loss)


@G.guards("ge_softmax_labels_grad")
@pytest.mark.parametrize("head", [0, 1])
@pytest.mark.parametrize("B,K,d", SHAPES)
def test_softmax_labels_grad(B, K, d, head):
    scale, lr = 20.0, 0.25
    t, hr, off, pos, cand = inputs(B, K, d, head)
    N, B1, K1, L = t.shape[0], B + 2, K + 1, len(pos)
    R = K1 + 2 * B1 + L
    need = int(_lib.load().ge_softmax_labels_workspace_bytes(B1, K1, d, L))
    ref = LR.evaluate(t, hr, off, pos, cand, 1.0, scale, bool(head), lr=lr)
    bl, bg = bound(t, hr, off, pos, cand, scale, bool(head), LR.evaluate(t, hr, off, pos, cand, 1.0, scale, bool(head)))

    def case(A, mode):
        tb, hb, ob, pb, cb = A.data("table", t), A.data("hr", hr), A.data("label_off", off), A.data("label_pos", pos), A.data("cand", cand)
        loss, gi, gv, w = A.out("loss", 4 * B1), A.out("grad_idx", 4 * R), A.out("grad_val", 4 * R * d), A.ws("workspace", need)
        rc = A.call("ge_softmax_labels_grad", tb.ptr, N, d, hb.ptr, B1, ob.ptr, pb.ptr, L, cb.ptr, K1, 1.0, scale, lr, 0, head,
                    loss.ptr, gi.ptr, gv.ptr, *G.ws_args(w, mode), G.S())
        torch.cuda.synchronize()
        unchanged((tb, ob, pb), t, off, pos)
        return rc

    def verify(A):
        loss, gi, gv = A["loss"].get(F32), A["grad_idx"].get(I32), A["grad_val"].get(F32, (R, d))
        assert np.isnan(loss[B:]).all() and np.array_equal(gi, ref[1])
        assert gi[K] == -1 and not gv[K].any() and (gi[-2:] == -1).all() and not gv[-2:].any()
        assert (gi[K1 + 2 * B:K1 + 2 * B1] == -1).all() and not gv[K1 + 2 * B:K1 + 2 * B1].any()
        G.near(9, np.abs(loss[:B] - ref[0][:B]), bl)
        G.near(9, np.abs(gv - ref[2]), lr * bg)
    G.drive(case, verify, ws=True)
    G.claimed(test_softmax_labels_grad)
