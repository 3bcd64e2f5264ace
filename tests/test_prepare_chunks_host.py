"""Host: the length of a prepare chunk (ge_train_max_chunk_steps) and the workspace sizes cut from it.  A step of one
sort tile (<= 4096 units) takes longer chunks than it used to; above that the lengths are the ones the multi-tile
sequence was measured with, and the workspace sizes, which are maxima over all smaller batches, rely on the length never
rising with the batch size."""
import pytest

from graphembeddings_amd import _lib

# (B, negative_ratio) -> steps per chunk above one tile, as before the one-tile chunks grew
UNCHANGED = {
    (4097, 0): 31, (16384, 0): 16, (32768, 0): 16, (65536, 0): 8, (262144, 0): 8, (300000, 0): 2,
    (4097, 1): 16, (16384, 1): 16, (32768, 1): 8, (65536, 1): 8, (262144, 1): 2, (300000, 1): 2,
    (4097, 3): 16, (16384, 3): 8, (32768, 3): 8, (65536, 3): 8, (262144, 3): 2, (300000, 3): 2,
}
GRID = sorted({1, 2, 7, 8, 255, 256, 257, 1023, 1024, 1025, 1365, 1366, 2047, 2048, 2049, 4095, 4096, 4097, 5000, 8191, 8192,
               8193, 16384, 16385, 32768, 32769, 65536, 65537, 131072, 262144, 262145, 300000, 1 << 20, 1 << 24})


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("negs", [0, 1, 3])
def test_chunk_steps_positive_and_never_rising_with_the_batch(lib, negs):
    steps = [int(lib.ge_train_max_chunk_steps(B, negs)) for B in GRID]
    assert all(s >= 1 for s in steps)
    assert all(a >= b for a, b in zip(steps, steps[1:])), list(zip(GRID, steps))
    # one tile: the same length whatever the batch, and longer than any multi-tile chunk
    one_tile = {int(lib.ge_train_max_chunk_steps(B, negs)) for B in GRID if (1 + negs) * B <= 4096}
    assert len(one_tile) == 1 and min(one_tile) > 31
    assert lib.ge_train_max_chunk_steps(0, negs) == 0 and lib.ge_train_max_chunk_steps(-4, negs) == 0
    assert lib.ge_train_max_chunk_steps(8, -1) == 0


def test_chunk_steps_above_one_tile_are_unchanged(lib):
    got = {k: int(lib.ge_train_max_chunk_steps(*k)) for k in UNCHANGED}
    assert got == UNCHANGED


@pytest.mark.parametrize("d", [8, 200])
def test_workspaces_never_shrink_as_the_batch_grows(lib, d):
    sizes = [int(lib.ge_train_workspace_bytes(B, d)) for B in GRID]
    assert all(s > 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), list(zip(GRID, sizes))
    assert [int(lib.ge_train_adagrad_workspace_bytes(B, d)) for B in GRID] == sizes
    for K in (1, 3):
        sizes = [int(lib.ge_train_logloss_workspace_bytes(B, K, d)) for B in GRID if (1 + K) * B <= 1 << 24]
        assert all(s > 0 for s in sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (K, list(zip(GRID, sizes)))


def test_workspace_holds_two_chunks_of_records(lib):
    """The need the documents state: two buffers of chunk x record words (4 bytes each) behind the gradient rows."""
    import ctypes as C
    for B, d in ((8, 8), (4096, 200)):
        lay = (C.c_int64 * 8)()
        assert lib.ge_train_prepared_layout(B, lay) == 0
        records = 2 * int(lib.ge_train_max_chunk_steps(B, 0)) * int(lay[0]) * 4
        need = int(lib.ge_train_workspace_bytes(B, d))
        assert records <= need <= records + 17 * (6 * B * d * 4 + 256) + 6 * B * 4 + 4096
