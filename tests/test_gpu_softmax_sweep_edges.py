"""GPU: the four softmax objectives of ComplEx at the instantiations, range splits and live-bitmap words of
softmax_sweep_kernel (csrc/ge_softmax_kern.h) that the shape list of their own suites never reaches.  The shapes and the
reason for each: tests/softmax_sweep_cases.py; that they reach what they claim, and that a wrong bitmap index fails case E:
tests/test_softmax_sweep_cases_host.py (CPU).

  C  widths 72, 128, 136, 192 (MAXCB 2 and 3, odd and even block counts), 256 (the X-resident edge, the largest LDS
     request) and 264, 272, 280 (the chunked path's ragged last chunk), at B = 130, K = 300 as every file's test_widths,
     through each file's own build / reference / check_case; the two-identical-calls and loss-only-entry bit equalities of
     test_exact_properties at each; one label against the 1-vs-all call at d = 128 and 264.
  D  sampled, B = 577: the candidate-side gradient sweep over eight query ranges of two tiles, three of them empty.
  E  masked, K = 4161, B = 448: seven query tiles whose one live candidate tile is 0, 31, 32, 33, 63, 64 or 65 -- words 0, 1
     and 2 of the live bitmap, both blocks of softmax_live_kernel -- in two arrangements.
  (F, the sampled workspace's exact fit, is a shape of tests/test_gpu_abi_guard_softmax_sampled.py.)

One test per width (shape, arrangement): the sides and the file's (max_norm, scale) pairs -- and the layouts for labels --
are run inside it, every one of them to its end, and the test fails with the list of the cases that failed (422 cases in
47 tests: the suite's test count grows by the kernel paths reached, not by their product with the norms).

Bounds: the project's own, not re-tuned -- per case e32 = the largest absolute deviation of the reference's float32
evaluation from its fp64 evaluation, separately for the loss and the gradient rows; the GPU must be within 8 * e32 + 1e-7
of the fp64 oracle.  Every case prints its four figures (`-s`); DESIGN.md sections 22 to 25 have the measured tables."""
import functools
import itertools

import numpy as np
import pytest
import torch

import test_gpu_softmax as TS
import test_gpu_softmax_labels as TL
import test_gpu_softmax_masked as TM
import test_gpu_softmax_sampled as TP
from graphembeddings_amd import hole as H
from tests import softmax_masked_ref as MR
from tests import softmax_sweep_cases as C

pytestmark = pytest.mark.gpu

I32, F32 = np.int32, np.float32
dev, bits = TS.dev, TS.bits
B, K = C.WIDTH_B, C.WIDTH_K
WIDTHS = [d for d, _ in C.WIDTHS]
SIDES = [False, True]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")


def same(x, y):
    return all(np.array_equal(bits(u), bits(v)) for u, v in zip(x, y))


def every(check, cases):
    """check(*case) for every case, each to its end; fails with every case whose assertion failed.  (An error that is no
    assertion -- a HIP error among them -- ends the test at once: nothing more is started on the GPU.)"""
    cases, bad = list(cases), []
    for c in cases:
        try:
            check(*c)
        except AssertionError as e:
            bad.append("%r: %s" % (c, str(e).split("\n")[0]))
    assert not bad, "%d of %d cases failed:\n%s" % (len(bad), len(cases), "\n".join(bad))


# ------------------------------------------------------------------------------------------------ C: widths
@pytest.mark.parametrize("d", WIDTHS)
def test_widths_one_vs_all(d):
    every(lambda ns, head: TS.check_case(B, K, d, *ns, head), itertools.product(TS.NORMS_SCALES, SIDES))


@pytest.mark.parametrize("d", WIDTHS)
def test_widths_sampled(d):
    every(lambda ns, head: TP.check_case(B, K, d, *ns, head), itertools.product(TP.NORMS_SCALES, SIDES))


@pytest.mark.parametrize("d", WIDTHS)
def test_widths_masked(d):
    every(lambda ns, head: TM.check_case(B, K, d, *ns, head), itertools.product(TM.NORMS_SCALES, SIDES))


@pytest.mark.parametrize("d", WIDTHS)
def test_widths_labels(d):
    every(lambda ns, head, layout: TL.check_case(B, K, d, *ns, head, layout), itertools.product(TS.NORMS_SCALES, SIDES, TL.LAYOUTS))


def exact_properties(d, head):
    """Of each file's test_exact_properties: two identical calls give the same bits, and the loss-only entry gives the
    gradient entry's loss (its LSE sweep is the MAXCB 1 instantiation whatever the width: the same X-resident or chunked
    score GEMM).  Masked: all bits set is the unmasked call, bit for bit."""
    mn, scale, side = 1.0, 20.0, "head" if head else "tail"
    t, hr, true, cand = TS.build(B, K, d, mn, head)
    a = TS.gpu_grad(t, hr, true, cand, mn, scale, head)
    assert same(a, TS.gpu_grad(t, hr, true, cand, mn, scale, head))
    assert np.array_equal(bits(H.softmax_loss(dev(t), dev(hr), dev(true), dev(cand), scale=scale, max_norm=mn, side=side)), bits(a[0]))

    t, hr, true, cand = TP.build(B, K, d, mn, head)
    a = TP.gpu_grad(t, hr, true, cand, mn, scale, head)
    assert same(a, TP.gpu_grad(t, hr, true, cand, mn, scale, head))
    lo = H.softmax_sampled_loss(dev(t), dev(hr), dev(true), dev(cand), scale=scale, max_norm=mn, side=side)
    assert np.array_equal(bits(lo), bits(a[0]))

    t, hr, true, cand, rs, sets = TM.build(B, K, d, mn, head)
    mask = MR.pack(sets, True)
    a = TM.gpu_masked(t, hr, true, cand, mn, scale, head, rs, mask)
    assert same(a, TM.gpu_masked(t, hr, true, cand, mn, scale, head, rs, mask))
    assert np.array_equal(bits(TM.gpu_masked(t, hr, true, cand, mn, scale, head, rs, mask, grad=False)), bits(a[0]))
    plain = TM.gpu_plain(t, hr, true, cand, mn, scale, head)
    assert same(TM.gpu_masked(t, hr, true, cand, mn, scale, head, np.maximum(rs, 0), np.full_like(mask, 0xFFFFFFFF)), plain)
    assert not same(a, plain)

    c = TL.case(B, K, d, mn, head, "mixed")
    a = TL.gpu_grad(*c, mn, scale, head)
    assert same(a, TL.gpu_grad(*c, mn, scale, head))
    lo = H.softmax_labels_loss(dev(c[0]), dev(c[1]), dev(c[2]), dev(c[3]), dev(c[4]), scale=scale, max_norm=mn, side=side)
    assert np.array_equal(bits(lo), bits(a[0]))


@pytest.mark.parametrize("d", WIDTHS)
def test_widths_exact_properties(d):
    every(lambda head: exact_properties(d, head), [(h,) for h in SIDES])


@pytest.mark.parametrize("d", [d for d, _ in C.ONE_LABEL_WIDTHS])
def test_widths_one_label_is_the_one_vs_all_call(d):
    """tests/test_gpu_softmax_labels.py's comparison as it stands there (the ids equal, the loss and the gradient summed
    per table row within the case's bound; not bitwise, for the reason it gives)."""
    every(lambda head: TL.test_one_label_is_the_one_vs_all_call(B, K, d, 1.0, 20.0, head), [(h,) for h in SIDES])


# ------------------------------------------------------------------------------------------------ D: sampled, query-side ranges
@pytest.mark.parametrize("shape", [s for s, _ in C.SAMPLED_RANGES])
def test_sampled_query_ranges(shape):
    every(lambda ns, head: TP.check_case(*shape, *ns, head), itertools.product(C.SAMPLED_NORMS_SCALES, SIDES))


def test_sampled_query_ranges_invalid_rows_appended():
    """The six appended rows lengthen the fifth range's second tile (B = 583: still ten tiles): every other output keeps its
    bits."""
    every(lambda head: TP.test_invalid_rows_appended(*C.SAMPLED_APPENDED, head), [(h,) for h in SIDES])


# ------------------------------------------------------------------------------------------------ E: the live bitmap
@functools.lru_cache(maxsize=None)
def bitmap_reference(order, max_norm, scale, head):
    t, hr, true, cand, rs, sets = C.bitmap_case(order, max_norm)
    return TM.e32_of(t, hr, true, cand, max_norm, scale, head, rs, sets)


def bitmap_check(order, max_norm, scale, head):
    Bq, Kc = C.BITMAP_B, C.BITMAP_K
    t, hr, true, cand, rs, sets = C.bitmap_case(order, max_norm)
    l64, idx, v64, e_l, e_g = bitmap_reference(order, max_norm, scale, head)
    loss, gi, gv = TM.gpu_masked(t, hr, true, cand, max_norm, scale, head, rs, MR.pack(sets, True))
    assert np.isfinite(l64).all() and np.array_equal(gi, idx)
    dl, dg = float(np.abs(loss - l64).max()), float(np.abs(gv - v64).max())
    print("SOFTMAX-MASKED bitmap B=%d K=%d d=%d order=%s max_norm=%g scale=%g side=%s: loss e32 %.3g gpu %.3g | grad e32 %.3g gpu %.3g"
          % (Bq, Kc, C.BITMAP_D, "forward" if order[0] == 0 else "reversed", max_norm, scale, "head" if head else "tail",
             e_l, dl, e_g, dg))
    assert np.isfinite(loss).all() and np.isfinite(gv).all(), "NaN rows: %s" % np.nonzero(~np.isfinite(loss))[0][:8]
    assert dl <= 8 * e_l + 1e-7, ("loss", dl, e_l)
    assert dg <= 8 * e_g + 1e-7, ("grad", dg, e_g)
    # the rows of the set that admits position 4160 alone: one candidate, loss 0 and exact zero query gradients
    one = np.nonzero(rs == 6)[0]
    assert not loss[one].any() and not l64[one].any() and not gv[Kc + 2 * one].any() and not gv[Kc + 2 * one + 1].any()
    # a candidate no row admits has its id and an exact zero row (an admitted one's row is the bound's business: at
    # scale 200 the softmax saturates and many a p underflows to an exact zero)
    nobody = ~sets.any(0)
    assert np.array_equal(gi[:Kc], cand) and not gv[:Kc][nobody].any() and gv[:Kc][~nobody].any()


@pytest.mark.parametrize("order", [o for o, _ in C.BITMAP_ORDERS], ids=["forward", "reversed"])
def test_masked_live_bitmap_beyond_word_0(order):
    """A live bit read or written at a wrong place skips the only candidate tile some query tile admits: its rows' true
    candidate is never found and their loss is NaN (tests/test_softmax_sweep_cases_host.py shows it for each wrong
    indexing).  A tile wrongly taken for live changes no output bit, so only this direction can show here."""
    every(lambda ns, head: bitmap_check(order, *ns, head), itertools.product(C.BITMAP_NORMS_SCALES, SIDES))
