"""CPU: same_source of csrc/ge_step_id.h -- what decides whether the pipeline handle's look-ahead records are reused --
compares every field of the source (tests/step_identity_check.cpp), compiled as plain host C++ under the address and
undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "graphembeddings_amd", "csrc")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("identity") / "step_identity_check")
    tried = []
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if not cxx or not shutil.which(cxx):
            continue
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "step_identity_check.cpp"), "-o", exe]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode == 0:
            return exe
        tried.append("%s: %s" % (cxx, p.stderr[-500:]))
    pytest.fail("no host C++ compiler built step_identity_check.cpp with the sanitizers:\n" + "\n".join(tried))


def test_same_source_compares_every_field(check):
    p = subprocess.run([check], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert p.stdout.strip().endswith("17 fields, 0 wrong")
