"""GPU: what ge_copy_if may touch -- the cases of tests/test_gpu_abi_guard.py for the gated multi-buffer copy, built with
its drive() / claimed() and tests/abi_guard.py: guard-banded buffers of EXACTLY count words each, 0x00 / 0xFF poison in every
destination, bitwise-equal runs, every guard intact, the sources and the flag unchanged; with the flag 0, and after a refusal
(overlapping destinations, passed with real buffers), every destination is still all poison.

The cases register in test_gpu_abi_guard.GUARDED at import, which is what its test_every_writing_entry_point_is_guarded
reads: the two files are collected together (`pytest tests -m gpu`).  ge_copy_if_chunk is claimed with it: it writes
nothing, but it is no size function in that test's sense, and the case calls it."""
import numpy as np
import pytest
import torch

import test_gpu_abi_guard as G
from graphembeddings_amd import _lib
from tests import abi_guard as AG

pytestmark = pytest.mark.gpu

I32 = np.int32


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")
    G.CALLED.clear()


def sizes_of(n_seg, chunk):
    pool = [chunk + 3, 1, 0, 2 * chunk, 5, chunk - 1, 4, 3, chunk, 7, 2, 6, 8, 9, 10, 11]
    return pool[:n_seg]


def buffers(A, sizes, shift):
    """(src buffers, dst buffers, data): segment k's source starts `shift` bytes past a 256-byte boundary, its destination
    (shift * k) % 16 bytes past one."""
    data = [np.random.default_rng(31 * k + n).integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(I32) for k, n in enumerate(sizes)]
    srcs = [A.data("src%d" % k, d, "in", shift) for k, d in enumerate(data)]
    dsts = []
    for k, n in enumerate(sizes):
        b = A._new("dst%d" % k, 4 * n, "out", (shift * k) % 16)
        b.fill(A.poison)
        dsts.append(b)
    return srcs, dsts, data


@G.guards("ge_copy_if", "ge_copy_if_chunk")
@pytest.mark.parametrize("n_seg,shift", [(1, 0), (1, 4), (2, 12), (5, 0), (16, 4), (16, 8)])
def test_copy_if(n_seg, shift):
    chunk = int(_lib.load().ge_copy_if_chunk())
    sizes = sizes_of(n_seg, chunk)
    want = {}

    def case_with(flag_value, overlap=False):
        def case(A, mode):
            assert A.call("ge_copy_if_chunk") == chunk == 8192
            srcs, dsts, data = buffers(A, sizes, shift)
            want["data"] = data
            flag = A.data("flag", np.array([flag_value], I32))
            d_ptrs = [b.ptr for b in dsts]
            if overlap:                                     # the last destination starts on the first one's first word
                d_ptrs[-1] = d_ptrs[0]
            rc = A.call("ge_copy_if", flag.ptr, *_lib.copy_if_args([b.ptr for b in srcs], d_ptrs, sizes), G.S())
            torch.cuda.synchronize()
            assert flag.get(I32)[0] == flag_value
            for b, d in zip(srcs, data):
                assert np.array_equal(b.get(I32), d), b.name
            return rc
        return case

    def verify(A):
        for k, d in enumerate(want["data"]):
            assert np.array_equal(A["dst%d" % k].get(I32), d), (k, sizes[k])
    G.drive(case_with(1), verify)
    G.drive(case_with(-7), verify)

    for poison in (0x00, 0xFF):                             # flag 0: a launch that writes nothing
        A = AG.Arena("", poison)
        assert case_with(0)(A, "exact") == 0
        A.assert_intact("(flag 0)")
        A.assert_outputs_poison("flag 0")
    if n_seg > 1 and sizes[0] > 0 and sizes[-1] > 0:        # a refusal: nothing launched
        A = AG.Arena("", 0xFF)
        assert case_with(1, overlap=True)(A, "exact") == _lib.GE_EINVAL
        A.assert_intact("(refused: overlapping destinations)")
        A.assert_outputs_poison("overlapping destinations")
    G.claimed(test_copy_if)
