"""CPU: csrc/ge_sweep_route.h routes every shape to the kernel the former chain of launchers ran for it
(tests/sweep_route_ref.py), compiled as plain host C++ under the address and undefined-behaviour sanitizers."""
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
    text = "".join("%s %d %d %d %d %r %d\n" % s for s in shapes)
    p = subprocess.run([dump], input=text, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split("\n")[:-1]
    assert len(lines) == len(shapes)
    bad = []
    for s, line in zip(shapes, lines):
        kernel, status = (int(x) for x in line.split())
        if (R.KERNELS[kernel], status) != R.route(*s):
            bad.append((s, R.KERNELS[kernel], status, R.route(*s)))
    assert not bad, "%d of %d shapes differ, first: %r" % (len(bad), len(shapes), bad[:5])
