"""CPU: csrc/ge_sweep_route.h routes every shape to the kernel the former chain of launchers ran for it
(tests/sweep_route_ref.py), and answers for the top-k and candidate-set sweeps what their launchers' fronts answered,
compiled as plain host C++ under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

from tests import sweep_route_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "graphembeddings_amd", "csrc")
N = 1 << 23
K_PLANES = 40330 * 128       # d = 200: 4 slices x 13 k blocks x 2 KiB = 106,496 bytes a tile; 2^32 / 106,496 = 40,329.85 tiles


def _shapes():
    dims = list(range(2, 301, 2)) + [1, 7, 55]
    bk = [(0, 300), (130, 0), (1, 1), (130, 300),
          (2816, 2816), (2817, 2816),                       # 22 x 22 = 484 and 23 x 22 = 506 tiles: not big
          (2048, 3968), (2048, 4096),                       # 16 x 31 = 496, 16 x 32 = 512: across the cut
          (128 * 65535, 300), (128 * 65535 + 1, 300),       # the fp32 kernel's and the tile kernels' grid.y
          (130, K_PLANES - 128), (130, K_PLANES)]           # the planes' 32-bit byte offsets
    return [(entry, N, d, B, K, mn, mod16) for entry in ("rank", "score") for d in dims for mn in (1.0, 8.0, 8.5)
            for mod16 in (0, 4) for B, K in bk]


B_BLOCKS = (R.INT32_MAX // 8) * 128      # the last B of INT32_MAX / 8 row blocks: the candidate-set forms' limit


def _f16_only_shapes():
    """(entry, N, d, B, K, max_norm, mod16, k) of the top-k and candidate-set entries, on both sides of every limit their
    launchers' fronts drew: the dim, max_norm, the planes' 2^32 bytes, the row blocks, the table's alignment, k, B == 0."""
    bk = [(0, 300), (130, 300), (130, 0), (130, K_PLANES - 128), (130, K_PLANES), (0, K_PLANES), (B_BLOCKS, 300),
          (B_BLOCKS + 1, 300)]
    return [(entry, N, d, B, K, mn, mod16, k) for entry in ("topk", "masked_rank", "masked_topk")
            for d in (48, 56, 200, 288, 296) for mn in (8.0, 8.5) for mod16 in (0, 4) for k in (0, 1, 128, 129)
            for B, K in bk]


def _run(dump, lines):
    p = subprocess.run([dump], input="".join(lines), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    out = p.stdout.split("\n")[:-1]
    assert len(out) == len(lines)
    return [[int(x) for x in line.split()] for line in out]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("route") / "sweep_route_dump")
    tried = []
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if not cxx or not shutil.which(cxx):
            continue
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "sweep_route_dump.cpp"), "-o", exe]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode == 0:
            return exe
        tried.append("%s: %s" % (cxx, p.stderr[-500:]))
    pytest.fail("no host C++ compiler built sweep_route_dump.cpp with the sanitizers:\n" + "\n".join(tried))


def test_the_restatement_reaches_every_kernel():
    seen = {R.route(*s)[0] for s in _shapes()}
    assert seen == set(R.KERNELS)
    # ... and the planes pair lies on both sides of 2^32 bytes: the last addressable K, then the first that is not
    assert R.route("rank", N, 200, 130, K_PLANES - 128, 1.0, 0) == ("F16", 0)
    assert R.route("rank", N, 200, 130, K_PLANES, 1.0, 0) == ("Pipe40", 0)


def test_route_equals_the_former_chain_on_every_shape(dump):
    shapes = _shapes()
    got = _run(dump, ["%s %d %d %d %d %r %d 0\n" % s for s in shapes])
    bad = []
    for s, (kernel, status) in zip(shapes, got):
        if (R.KERNELS[kernel], status) != R.route(*s):
            bad.append((s, R.KERNELS[kernel], status, R.route(*s)))
    assert not bad, "%d of %d shapes differ, first: %r" % (len(bad), len(shapes), bad[:5])


def test_the_restatement_of_the_f16_only_fronts_gives_every_answer():
    for entry in ("topk", "masked_rank", "masked_topk"):
        seen = {R.route(*s) for s in _f16_only_shapes() if s[0] == entry}
        want = {("F16", 0), ("None", 0), ("None", R.GE_ENOTSUP)}
        if entry != "masked_rank":
            want.add(("None", R.GE_EINVAL))           # topk without sets: k < 1 alone; with sets: the alignment too
        assert seen >= want, entry
    assert R.route("masked_rank", N, 200, 130, 300, 8.0, 4, 1) == ("None", R.GE_EINVAL)
    # each limit from both sides
    assert R.route("topk", N, 200, 130, K_PLANES - 128, 8.0, 0, 128) == ("F16", 0)
    assert R.route("topk", N, 200, 130, K_PLANES, 8.0, 0, 128) == ("None", R.GE_ENOTSUP)
    assert R.route("masked_topk", N, 200, B_BLOCKS, 300, 8.0, 0, 1) == ("F16", 0)
    assert R.route("masked_topk", N, 200, B_BLOCKS + 1, 300, 8.0, 0, 1) == ("None", R.GE_ENOTSUP)
    assert R.route("topk", N, 200, B_BLOCKS + 1, 300, 8.0, 4, 1) == ("F16", 0)      # neither asked of the plain top-k
    assert R.route("masked_topk", N, 56, 130, 300, 8.0, 0, 129) == ("None", R.GE_ENOTSUP)
    assert R.route("masked_topk", N, 56, 130, 300, 8.0, 4, 129) == ("None", R.GE_EINVAL)   # the alignment before k


def test_topk_and_masked_routes_equal_the_former_launchers_on_every_shape(dump):
    shapes = _f16_only_shapes()
    got = _run(dump, ["%s %d %d %d %d %r %d %d\n" % s for s in shapes])
    bad = []
    for s, (kernel, status) in zip(shapes, got):
        if (R.KERNELS[kernel], status) != R.route(*s):
            bad.append((s, R.KERNELS[kernel], status, R.route(*s)))
    assert not bad, "%d of %d shapes differ, first: %r" % (len(bad), len(shapes), bad[:5])


def test_topk_workspace_and_grid_equal_the_former_functions(dump):
    """topk_splits, topk_ws_bytes and the grid limit across 256 row blocks, one and many candidate tiles, the k range
    and INT32_MAX workgroups."""
    Bs = [1, 128, 129, 1000, 128 * 255, 128 * 255 + 1, 32768, 32769, 128 * 300, R.INT32_MAX * 128, R.INT32_MAX * 128 + 1]
    Ks = [0, 1, 128, 129, 300, 128 * 40, 14951, 128 * 255, 128 * 256 + 1, 1200000]
    grid = [(B, K, k) for B in Bs for K in Ks for k in (0, 1, 5, 32, 33, 64, 128, 129)]
    got = _run(dump, ["ws 1 200 %d %d 1.0 0 %d\n" % t for t in grid])
    want = [[R.topk_splits(B, K), R.topk_ws_bytes(B, K, k), int(R.topk_grid_ok(B, K))] for B, K, k in grid]
    bad = [(t, g, w) for t, g, w in zip(grid, got, want) if g != w]
    assert not bad, "%d of %d differ, first: %r" % (len(bad), len(grid), bad[:5])
    assert {w[2] for w in want} == {0, 1} and {w[0] for w in want} >= {1, 2, 40, 256}


