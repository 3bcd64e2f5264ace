"""Host: the size functions of include/ge_hip.h (*_workspace_bytes, *_planes_bytes, ge_train_prepare_bytes,
ge_shard_owner_record_words).  No pointer is passed and no kernel runs: 0 for each documented bad size, non-decreasing
in every size argument over a grid that crosses the kernels' tile sizes, and a multiple of 256 where the entry point
demands a 256-byte aligned workspace (so that workspaces can be laid out back to back)."""
import itertools

import pytest
import torch

from graphembeddings_amd import _lib

# one below, at and one above: the sweeps' 16 rows, the 64 / 128 tiles, the 256-pair granule, 1024, the 4096-unit sort
# tile (and two of them), the relation rank's 65,536-row chunk
SIZES = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193,
         65535, 65536, 65537]
KS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128]
SMALL = [1, 2, 3, 9, 32, 33]
CAPS = sorted(SIZES + [16383, 16384, 16385])          # the owner records' 16,384-key tile

# name: (arguments in ABI order with their grids (monotone ones in a list, fixed ones as a 1-tuple), bad argument tuples,
#        whether the result must be a multiple of 256)
E, R = (3000,), (9,)
CASES = {
    "ge_hinge_step_workspace_bytes": ([SIZES, (8, 200)], [(0, 8), (-1, 8), (5, 0)], True),
    "ge_logloss_step_workspace_bytes": ([SIZES, (8, 200)], [(0, 8), (5, 0)], True),
    "ge_validation_workspace_bytes": ([SIZES], [(0,), (-3,)], True),
    "ge_validation_logloss_workspace_bytes": ([SIZES, SMALL], [(0, 1), (5, 0)], True),
    "ge_train_workspace_bytes": ([SIZES, (8, 200)], [(0, 8), (5, 0)], True),
    # negative_ratio is a fixed argument here ON PURPOSE: include/ge_hip.h states that this size is not monotone in it
    # (test_logloss_workspace_is_not_monotone_in_the_negative_ratio pins the documented example)
    "ge_train_logloss_workspace_bytes": ([SIZES, (1, 3, 7, 8, 33), (8,)], [(0, 1, 8), (5, 0, 8), (5, 1, 0)], True),
    "ge_train_prepare_bytes": ([SIZES, SMALL], [(0, 1), (5, 0)], True),
    "ge_shard_plan_workspace_bytes": ([SIZES, SMALL], [(0, 1), (5, 0)], True),
    "ge_shard_owner_record_words": ([CAPS], [(0,), (-1,)], False),
    "ge_shard_owner_workspace_bytes": ([CAPS, SMALL], [(0, 1), (5, 0)], True),
    "ge_transx_step_workspace_bytes": ([E, R, (16,), SIZES], [(0, 9, 16, 5), (10, 0, 16, 5), (10, 9, 0, 5), (10, 9, 1025, 5),
                                                             (10, 9, 16, 0)], True),
    "ge_transr_step_workspace_bytes": ([E, R, (8,), (12,), SIZES], [(0, 9, 8, 12, 5), (10, 0, 8, 12, 5), (10, 9, 0, 12, 5),
                                                                   (10, 9, 8, 257, 5), (10, 9, 8, 12, 0)], True),
    "ge_transx_rank_workspace_bytes": ([(0, 1, 2), E, R, (16,), SIZES], [(3, 10, 9, 16, 5), (0, 0, 9, 16, 5), (0, 10, 0, 16, 5),
                                                                         (0, 10, 9, 0, 5), (0, 10, 9, 16, 0)], True),
    "ge_transr_rank_workspace_bytes": ([E, R, (8,), (12,), SIZES], [(0, 9, 8, 12, 5), (10, 9, 8, 300, 5), (10, 9, 8, 12, 0)], True),
    "ge_transx_relation_rank_workspace_bytes": ([(0, 1, 2), E, R, (16,), SIZES], [(-1, 10, 9, 16, 5), (0, 10, 9, 16, 0),
                                                                                  (0, 10, 9, 2000, 5)], True),
    "ge_transr_relation_rank_workspace_bytes": ([E, R, (8,), (12,), SIZES], [(10, 9, 8, 12, 0), (10, 0, 8, 12, 5)], True),
    "ge_transx_topk_workspace_bytes": ([(0, 1, 2), E, R, (16,), SIZES, KS], [(0, 10, 9, 16, 5, 0), (0, 10, 9, 16, 5, 129),
                                                                             (0, 10, 9, 16, 0, 5), (3, 10, 9, 16, 5, 5)], True),
    "ge_transr_topk_workspace_bytes": ([E, R, (8,), (12,), SIZES, KS], [(10, 9, 8, 12, 5, 0), (10, 9, 8, 12, 5, 129),
                                                                        (10, 9, 8, 12, 0, 5)], True),
    "ge_neighbor_workspace_bytes": ([SIZES, SIZES[::3], KS], [(0, 10, 1), (1, 0, 1), (1, 10, 0), (1, 10, 129)], True),
    "ge_topk_workspace_bytes": ([SIZES, SIZES[::3], KS], [(0, 10, 1), (1, 0, 1), (1, 10, 0), (1, 10, 129)], True),
    "ge_neighbor_planes_bytes": ([SIZES, (1, 64, 65, 288)], [(0, 8), (10, 0), (10, 289)], True),
    "ge_rank_planes_bytes": ([(70000,), (56, 64, 200, 288), SIZES], [(0, 64, 10), (100, 0, 10), (100, 40, 10)], True),
}

# These two hold rocprim's radix-sort scratch, whose size rocprim works out from the device's properties once the batch
# has more than a few hundred keys: on a host without a device they report 0 (cannot size) from there on, and the
# grid stops at the first 0.  With a device the whole grid is checked.
NEEDS_DEVICE = ("ge_transx_step_workspace_bytes", "ge_transr_step_workspace_bytes")


def test_every_size_function_is_listed():
    names = {n for n in _lib.SYMBOLS if n.endswith("_bytes") or n.endswith("_words")}
    assert names == set(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_size_function(name):
    fn = getattr(_lib.load(), name)
    grids, bad, aligned = CASES[name]
    for args in bad:
        assert int(fn(*args)) == 0, (name, args)
    varying = [i for i, g in enumerate(grids) if isinstance(g, list)]
    for i in varying:
        # the other monotone arguments at their smallest, a middle and their largest value; fixed ones at every value
        others = [(g if isinstance(g, tuple) else (g[0], g[len(g) // 2], g[-1])) if j != i else (None,)
                  for j, g in enumerate(grids)]
        for combo in itertools.product(*others):
            vals = []
            for x in grids[i]:
                a = list(combo)
                a[i] = x
                vals.append(int(fn(*a)))
            if name in NEEDS_DEVICE and not torch.cuda.is_available() and 0 in vals:
                vals = vals[:vals.index(0)]
            assert all(v > 0 for v in vals), (name, i, combo, vals)
            assert vals == sorted(vals), "%s is not non-decreasing in argument %d at %s: %s" % (name, i, combo, vals)
            if aligned:
                assert all(v % 256 == 0 for v in vals), (name, i, combo, [v for v in vals if v % 256])


def test_logloss_workspace_is_not_monotone_in_the_negative_ratio():
    """The header's caveat, pinned: the steps prepared per chunk and the gradient ring shrink as (1 + negative_ratio) * B
    grows, so a larger ratio can need fewer bytes.  A caller sizes the workspace for the ratio it uses."""
    fn = _lib.load().ge_train_logloss_workspace_bytes
    assert int(fn(1024, 31, 8)) > int(fn(1024, 32, 8)) > 0


@pytest.mark.parametrize("name,rest", [("ge_train_workspace_bytes", (8,)), ("ge_train_workspace_bytes", (200,)),
                                       ("ge_train_logloss_workspace_bytes", (1, 8)),
                                       ("ge_train_logloss_workspace_bytes", (3, 200))])
def test_training_workspaces_never_shrink_with_the_batch(name, rest):
    """The two sizes are the largest layout of any batch up to B, found by walking the plateaus of two step functions
    (largest_need_up_to in ge_train.hip: it relies on the steps only falling and on the layout growing between two
    falls).  Held here against every B up to 20,000, every 7th up to 300,000 and the neighbours of every power of two:
    a layout change that breaks either property shows as a size that shrinks."""
    fn = getattr(_lib.load(), name)
    Bs = sorted(set(range(1, 20001)) | set(range(20001, 300001, 7)) |
                {(1 << p) + o for p in range(15, 23) for o in (-1, 0, 1)})
    prev = 0
    for B in Bs:
        v = int(fn(B, *rest))
        assert v >= prev > -1 and v % 256 == 0, (B, v, prev)
        prev = v
