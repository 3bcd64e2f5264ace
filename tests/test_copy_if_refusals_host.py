"""Host: what ge_copy_if answers to bad arguments.  Every refusal comes before the launch, and so does the good call whose
counts are all 0 (nothing to launch): no case here reaches a kernel, and every device pointer is a fake address that is
never dereferenced.  As in test_rotate_refusals_host.py the cases are skipped where a GPU is visible, so that a case that
slipped through validation could never launch on a fake pointer.  (Touching ranges, which are no overlap, are copied for
real in test_gpu_copy_if.py.)"""
import ctypes as C

import pytest
import torch

from graphembeddings_amd import _lib

host_only = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: host-only refusals")
EINVAL, ENOTSUP = _lib.GE_EINVAL, _lib.GE_ENOTSUP
A = 1 << 12                                   # a fake, 256-byte aligned, never-dereferenced address
M = 1 << 20                                   # the fake buffers lie 1 MiB apart
FLAG = A + 100 * M
MAX = 16


def copy_if(src, dst, count, flag=FLAG, n_seg=None, arrays=(True, True, True)):
    """ge_copy_if on host arrays built from the lists; arrays[i] False passes NULL for src / dst / count."""
    n, s, d, c = _lib.copy_if_args(src, dst, count)
    s, d, c = (x if keep else None for x, keep in zip((s, d, c), arrays))
    return _lib.load().ge_copy_if(flag, n if n_seg is None else n_seg, s, d, c, None)


def segs(n, words=10):
    """n disjoint segments: (src addresses, dst addresses, counts)."""
    return [A + 2 * k * M for k in range(n)], [A + (2 * k + 1) * M for k in range(n)], [words] * n


def test_prototype_version_and_chunk():
    lib = _lib.load()
    assert lib.ge_version() >= 449
    assert len(_lib.SYMBOLS["ge_copy_if"][1]) == 6 and _lib.SYMBOLS["ge_copy_if_chunk"][1] == []
    chunk = int(lib.ge_copy_if_chunk())
    assert chunk == 8192 and chunk % (256 * 4) == 0       # the header states it; whole 16-byte words for 256 lanes


@host_only
def test_nothing_to_copy_returns_before_any_launch():
    for n in (1, 3, MAX):
        s, d, _ = segs(n)
        assert copy_if(s, d, [0] * n) == 0
    assert copy_if([None, None], [None, None], [0, 0]) == 0          # an empty segment's pointers are not looked at
    assert copy_if([A + 2], [A + 1], [0]) == 0


@host_only
def test_null_arguments_and_segment_count():
    s, d, c = segs(2)
    assert copy_if(s, d, c, flag=None) == EINVAL
    for arrays in ((False, True, True), (True, False, True), (True, True, False)):
        assert copy_if(s, d, c, arrays=arrays) == EINVAL, arrays
        assert copy_if(s, d, [0, 0], arrays=arrays) == EINVAL, arrays  # ... whatever the counts
    for n_seg in (0, -1, MAX + 1, 1 << 20):
        s, d, c = segs(MAX)
        assert copy_if(s, d, [0] * MAX, n_seg=n_seg) == EINVAL, n_seg
    s, d, c = segs(MAX)
    assert copy_if(s, d, [0] * MAX, n_seg=MAX) == 0 and copy_if(s, d, [0] * MAX, n_seg=1) == 0


@host_only
def test_counts_and_pointers():
    s, d, c = segs(3)
    for k in range(3):
        bad = list(c)
        bad[k] = -1
        assert copy_if(s, d, bad) == EINVAL
        assert copy_if(s, d, [-1 if j == k else 0 for j in range(3)]) == EINVAL     # ... with nothing else to copy
        for off in (1, 2, 3, 5, 6, 7, 13):                  # 4-byte alignment is all that is asked, and it is asked
            for which in (0, 1):
                p = [list(s), list(d)]
                p[which][k] += off
                assert copy_if(p[0], p[1], c) == EINVAL, (k, off, which)
        for which in (0, 1):
            p = [list(s), list(d)]
            p[which][k] = None
            assert copy_if(p[0], p[1], c) == EINVAL, (k, which)
    # a count beyond 2^44 words is refused as unsupported, after every GE_EINVAL
    assert copy_if([A], [A + (1 << 50)], [(1 << 44) + 1]) == ENOTSUP
    assert copy_if([A], [A + 4], [(1 << 44) + 1]) == EINVAL             # (overlaps)
    assert copy_if([A, A + 2], [A + (1 << 50), A + (1 << 51)], [(1 << 44) + 1, 4]) == EINVAL


def both_orders(s, d, c):
    """The status codes of the segments as given and reversed: the overlap check does not depend on the order."""
    return {copy_if(s, d, c), copy_if(s[::-1], d[::-1], c[::-1])}


@host_only
def test_overlapping_ranges_are_refused_in_any_order():
    w = 10                                                  # words a segment
    for n in (2, 5, MAX):
        s, d, c = segs(n, w)
        for k in range(1, n):
            # dst k against dst 0: equal, its first word on the other's last, its last word on the other's first
            for p in (d[0], d[0] + 4 * (w - 1), d[0] - 4 * (w - 1)):
                dd = list(d)
                dd[k] = p
                assert both_orders(s, dd, c) == {EINVAL}, (n, k, "dst-dst", p - d[0])
            # dst k against src 0 (another segment's source) and against its own source
            for j in (0, k):
                for p in (s[j], s[j] + 4 * (w - 1), s[j] - 4 * (w - 1)):
                    dd = list(d)
                    dd[k] = p
                    assert both_orders(s, dd, c) == {EINVAL}, (n, k, "dst-src", j, p - s[j])
    # a single segment copied onto itself, or shifted by one word
    assert copy_if([A], [A], [w]) == EINVAL and copy_if([A], [A + 4], [w]) == EINVAL and copy_if([A + 4], [A], [w]) == EINVAL
    # an empty segment overlaps nothing: with every other count 0 the call has nothing to do
    assert copy_if([A, A], [A, A], [0, 0]) == 0
    # sources may overlap each other (they are only read): the refusal of this call is the bad count, not the sources
    assert copy_if([A, A], [A + M, A + 2 * M], [w, -1]) == EINVAL


def test_copy_if_args_builds_host_arrays():
    n, s, d, c = _lib.copy_if_args([8, 16], [24, 32], [3, 0])
    assert n == 2 and list(s) == [8, 16] and list(d) == [24, 32] and list(c) == [3, 0]
    assert isinstance(c, C.Array) and C.sizeof(c) == 16 and C.sizeof(s) == 16
