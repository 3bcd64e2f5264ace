"""GPU: ge_copy_if -- dst[s] <- src[s] for up to 16 segments iff a device flag is set, one launch.

Every buffer is a guard-banded one of tests/abi_guard.py, EXACTLY count words long, its payload starting 0, 4, 8 or 12 bytes
past a 256-byte boundary; every dst is pre-filled with 0xFF bytes (a NaN as float, -1 as int32).  All comparisons are bitwise,
as int32.  With the flag set every dst equals its src, the guards are intact and the sources unchanged; with the flag 0 every
dst byte is still poison.  Counts: around the 4-word vector, around one chunk (ge_copy_if_chunk() words a workgroup) and past
two chunks, so that a segment spans several workgroups and ends in a partial one."""
import numpy as np
import pytest
import torch

from graphembeddings_amd import _lib
from tests import abi_guard as AG

pytestmark = pytest.mark.gpu

I32 = np.int32
POISON = 0xFF
OFFSETS = (0, 4, 8, 12)


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")


def chunk() -> int:
    return int(_lib.load().ge_copy_if_chunk())


def counts():
    c = chunk()
    return [1, 3, 4, 5, c - 1, c, c + 1, 2 * c + 7]


def words(n, seed):
    """n int32 words that cover every byte value, among them NaNs with payloads, infinities and -0.0."""
    rng = np.random.default_rng(seed)
    w = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(I32)
    special = np.array([0x7FC12345, 0x7F800001, 0x7F800000, 0x00000001], dtype=np.int64).astype(I32)
    special = np.concatenate([special, np.array([-1, -2 ** 31, -(2 ** 31) + 0x00400001], dtype=I32)])   # 0xFFFFFFFF, -0.0, 0x80400001
    k = min(n, special.size)
    w[rng.permutation(n)[:k]] = special[:k]
    return w


def copy(segments, flag_value):
    """One ge_copy_if over [(count, src shift, dst shift)]; returns (arena, src data, dst buffers) after a synchronise."""
    A = AG.Arena("ge_copy_if", POISON)
    data, srcs, dsts = [], [], []
    for k, (n, s_shift, d_shift) in enumerate(segments):
        data.append(words(n, 1000 * k + n))
        srcs.append(A.data("src%d" % k, data[-1], "in", s_shift))
        d = A._new("dst%d" % k, 4 * n, "out", d_shift)
        d.fill(POISON)
        dsts.append(d)
    flag = torch.tensor([flag_value], dtype=torch.int32, device="cuda")
    rc = A.call("ge_copy_if", flag.data_ptr(), *_lib.copy_if_args([b.ptr for b in srcs], [b.ptr for b in dsts],
                                                                [n for n, _, _ in segments]), AG.stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert int(flag[0]) == flag_value
    return A, data, srcs, dsts


def check(segments, flag_value):
    A, data, srcs, dsts = copy(segments, flag_value)
    A.assert_intact("flag %d, segments %s" % (flag_value, segments))
    for k, (n, s_shift, d_shift) in enumerate(segments):
        assert srcs[k].ptr % 256 == s_shift and dsts[k].ptr % 256 == d_shift
        assert np.array_equal(srcs[k].get(I32), data[k]), ("src changed", k, segments[k])
        got = dsts[k].get(I32)
        if flag_value:
            bad = np.nonzero(got != data[k])[0]
            assert bad.size == 0, ("segment %d %s: %d words differ, first at %d" % (k, segments[k], bad.size, bad[0]))
        else:
            assert dsts[k].all_bytes_are(POISON), ("flag 0 wrote segment", k, segments[k])


def test_chunk_is_what_the_header_states():
    assert chunk() == 8192


@pytest.mark.parametrize("flag_value", [1, 0])
@pytest.mark.parametrize("which", range(8))
def test_every_alignment_pair_at_one_count(which, flag_value):
    """16 segments of one count: every (src, dst) pair of byte offsets 0 / 4 / 8 / 12 -- both 16-byte aligned (the vector
    path), both off by the same amount, and mixed (dwords)."""
    n = counts()[which]
    check([(n, so, do) for so in OFFSETS for do in OFFSETS], flag_value)


@pytest.mark.parametrize("which", range(8))
def test_single_segment(which):
    n = counts()[which]
    for so, do in ((0, 0), (4, 4), (0, 8), (12, 0)):
        for flag_value in (1, 0):
            check([(n, so, do)], flag_value)


def mixed():
    c = chunk()
    sizes = [1, c + 1, 3, 4, 5, c - 1, 2, 0, c, 7, 2 * c + 7, 6, 8, 1, 3 * c, 9]     # a zero-length one in the middle
    assert len(sizes) == 16 and sizes[7] == 0
    return [(n, OFFSETS[k % 4], OFFSETS[(k // 4) % 4]) for k, n in enumerate(sizes)]


@pytest.mark.parametrize("flag_value", [1, 0, 7, -1])
def test_sixteen_mixed_segments(flag_value):
    """Mixed sizes and alignments in one call: workgroups find their segment among 15 chunk starts; any non-zero flag
    counts as set."""
    check(mixed(), flag_value)


def test_empty_segment_pointers_are_not_looked_at():
    segs = [(5, 0, 0), (0, 0, 0), (9, 4, 0)]
    A = AG.Arena("ge_copy_if", POISON)
    d0, d2 = words(5, 1), words(9, 2)
    s = [A.data("src0", d0), None, A.data("src2", d2, "in", 4)]
    d = [A.out("dst0", 20), None, A.out("dst2", 36)]
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    rc = A.call("ge_copy_if", flag.data_ptr(), *_lib.copy_if_args([s[0].ptr, None, s[2].ptr], [d[0].ptr, 2, d[2].ptr],
                                                                [n for n, _, _ in segs]), AG.stream())
    torch.cuda.synchronize()
    assert rc == 0
    A.assert_intact()
    assert np.array_equal(d[0].get(I32), d0) and np.array_equal(d[2].get(I32), d2)


@pytest.mark.parametrize("flag_value", [1, 0])
def test_touching_segments_of_one_buffer(flag_value):
    """16 segments laid back to back in ONE source and ONE destination buffer (touching is not overlapping; odd sizes move
    the later segments off 16 bytes), passed in a shuffled order: the whole destination equals the whole source."""
    sizes = [n for n, _, _ in mixed()]
    total = sum(sizes)
    data = words(total, 77)
    A = AG.Arena("ge_copy_if", POISON)
    src, dst = A.data("src", data), A.out("dst", 4 * total)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    order = np.random.default_rng(5).permutation(16)
    flag = torch.tensor([flag_value], dtype=torch.int32, device="cuda")
    rc = A.call("ge_copy_if", flag.data_ptr(), *_lib.copy_if_args([src.ptr + 4 * int(starts[k]) for k in order],
                                                                [dst.ptr + 4 * int(starts[k]) for k in order],
                                                                [sizes[k] for k in order]), AG.stream())
    torch.cuda.synchronize()
    assert rc == 0
    A.assert_intact()
    assert np.array_equal(src.get(I32), data)
    if flag_value:
        assert np.array_equal(dst.get(I32), data)
    else:
        assert dst.all_bytes_are(POISON)


def test_flag_is_read_when_the_kernel_runs():
    """The flag is a device word read by the kernel, not by the call: ge_rank_metrics' `improved` of an earlier launch on
    the same stream gates the copy, with no synchronisation in between."""
    n = chunk() + 5
    data = words(n, 3)
    A = AG.Arena("ge_copy_if", POISON)
    src, dst_yes, dst_no = A.data("src", data), A.out("dst_yes", 4 * n), A.out("dst_no", 4 * n)
    nb = torch.zeros(4, dtype=torch.int32, device="cuda")
    nk = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.zeros(2, 8, dtype=torch.float32, device="cuda")
    best = torch.zeros(1, dtype=torch.float32, device="cuda")
    imp = torch.full((2,), 5, dtype=torch.int32, device="cuda")
    S = AG.stream()
    for i, dst in enumerate((dst_yes, dst_no)):             # the first tick improves on 0 (MRR 1), the second ties
        _lib.call("ge_rank_metrics", nb.data_ptr(), nk.data_ptr(), None, 4, out.data_ptr() + 32 * i, best.data_ptr(),
                  imp.data_ptr() + 4 * i, S)
        assert A.call("ge_copy_if", imp.data_ptr() + 4 * i, *_lib.copy_if_args([src.ptr], [dst.ptr], [n]), S) == 0
    torch.cuda.synchronize()
    A.assert_intact()
    assert imp.tolist() == [1, 0] and float(best[0]) == 1.0
    assert np.array_equal(dst_yes.get(I32), data) and dst_no.all_bytes_are(POISON)
