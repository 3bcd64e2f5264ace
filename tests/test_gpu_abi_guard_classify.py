"""GPU: what ge_threshold_fit and ge_threshold_classify may touch -- the cases of tests/test_gpu_abi_guard.py for the two
entry points of triple classification, built with its drive() / claimed() and tests/abi_guard.py: guard-banded buffers of
EXACTLY the declared sizes, 0x00 / 0xFF poison, bitwise-equal runs, `need - 1` -> GE_ENOMEM, the workspace offset by 16
bytes -> GE_EINVAL, outputs still poison after a refusal; the results exact against tests/classify_ref.py.

The cases register in test_gpu_abi_guard.GUARDED at import, which is what its test_every_writing_entry_point_is_guarded
reads: the two files are collected together (`pytest tests -m gpu`)."""
import numpy as np
import pytest
import torch

import test_gpu_abi_guard as G
from graphembeddings_amd import _lib
from tests import classify_ref as R

pytestmark = pytest.mark.gpu

I32, F32, U8 = np.int32, np.float32, np.uint8
FIELDS = ("thr_lo", "thr_hi", "best_correct", "n_pos", "n_neg")


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")
    G.CALLED.clear()


def tile():
    from graphembeddings_amd import classify
    return classify.FIT_TILE


def inputs(M, n_seg, seed, bad_segments=False):
    rng = np.random.default_rng(seed)
    seg = rng.integers(-2 if bad_segments else 0, n_seg + (2 if bad_segments else 0), M).astype(I32)
    score = rng.choice(np.array([-1.0, 0.25, 0.5, 2.0, np.inf], F32), M) if seed % 2 else rng.standard_normal(M).astype(F32)
    score[rng.random(M) < 0.1] = np.nan
    return score, seg, rng.integers(0, 2, M).astype(U8)


def fit_case(score, seg, label, n_seg):
    M = len(score)
    need = int(_lib.load().ge_threshold_fit_workspace_bytes(M, n_seg))
    assert need > 0

    def case(A, mode):
        s, g, l = A.data("score", score), A.data("seg", seg), A.data("label", label)
        outs = [A.out(k, 4 * n_seg) for k in FIELDS]
        w = A.ws("workspace", need)
        return A.call("ge_threshold_fit", s.ptr, g.ptr, l.ptr, M, n_seg, *(o.ptr for o in outs), *G.ws_args(w, mode), G.S())
    return case


@G.guards("ge_threshold_fit")
@pytest.mark.parametrize("shape", ["1x1", "65x7", "T+1x3", "3T+17x1345", "5000x20000"])
def test_threshold_fit(shape):
    t = tile()
    M, n_seg = {"1x1": (1, 1), "65x7": (65, 7), "T+1x3": (t + 1, 3), "3T+17x1345": (3 * t + 17, 1345),
                "5000x20000": (5000, 20000)}[shape]
    score, seg, label = inputs(M, n_seg, seed=M + n_seg, bad_segments=M > 100)
    o = R.sort_order(score, seg)
    score, seg, label = score[o], seg[o], label[o]
    ref = R.fit(score, seg, label, n_seg)

    def verify(A):
        for k in FIELDS:
            got = A[k].get(ref[k].dtype)
            assert np.array_equal(got.view(I32), ref[k].view(I32)), k
    G.drive(fit_case(score, seg, label, n_seg), verify, ws=True)
    # input that is not ordered: the numbers mean nothing (and where two elements claim a segment's start they may
    # differ between runs), every store stays inside its buffer
    score, seg, label = inputs(M, n_seg, seed=M + n_seg + 1, bad_segments=True)
    G.drive(fit_case(score, seg, label, n_seg), compare=lambda o0, o1: None)
    G.claimed(test_threshold_fit)


@G.guards("ge_threshold_classify")
@pytest.mark.parametrize("M,n_seg", [(1, 1), (63, 2), (65, 7), (70001, 1345), (8193, 2048), (5000, 20000)])
def test_threshold_classify(M, n_seg):
    score, seg, label = inputs(M, n_seg, seed=3 * M + n_seg, bad_segments=True)
    if M > 1000:
        seg[:1000] = n_seg // 2                         # whole waves of one segment
    rng = np.random.default_rng(M)
    thr = rng.standard_normal(n_seg).astype(F32)
    thr[::5] = np.inf
    thr[1::7] = np.nan
    for with_labels in (True, False):
        def case(A, mode):
            s, g, t = A.data("score", score), A.data("seg", seg), A.data("thr", thr)
            pred = A.out("pred", M)
            l = c = None
            if with_labels:
                l, c = A.data("label", label).ptr, A.out("confusion", 16 * n_seg).ptr
            return A.call("ge_threshold_classify", s.ptr, g.ptr, l, M, n_seg, t.ptr, pred.ptr, c, G.S())

        def verify(A):
            rp, rc = R.classify(score, seg, thr, n_seg, label if with_labels else None)
            assert np.array_equal(A["pred"].get(U8), rp)
            if with_labels:
                assert np.array_equal(A["confusion"].get(I32, (n_seg, 4)), rc)
        G.drive(case, verify)
    # confusion without labels is refused, and nothing is touched
    A = G.AG.Arena("", 0xFF)
    s, g, t = A.data("score", score), A.data("seg", seg), A.data("thr", thr)
    pred, conf = A.out("pred", M), A.out("confusion", 16 * n_seg)
    assert A.call("ge_threshold_classify", s.ptr, g.ptr, None, M, n_seg, t.ptr, pred.ptr, conf.ptr, G.S()) == G.EINVAL
    A.assert_intact()
    A.assert_outputs_poison()
    G.claimed(test_threshold_classify)
