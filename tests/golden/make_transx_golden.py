#!/usr/bin/env python3
"""Generates tests/golden/transx_init_batches_v1.npz: the first batches the reference's native sampler
(oracle/_ref/init.so, built by `make -C oracle ref` where the reference tree is present) draws on the
generated graphs of tests/test_transx_oracle.py.  Only the binary's outputs are stored.

    python tests/golden/make_transx_golden.py
"""
import importlib.util
import os
import pathlib
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def main():
    spec = importlib.util.spec_from_file_location("tt", os.path.join(ROOT, "tests", "test_transx_oracle.py"))
    tt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tt)
    if not os.path.exists(tt.REF_SO):
        sys.exit(f"{tt.REF_SO} is not built (make -C oracle ref)")
    out = {}
    for seed in (0, 1):
        tri, E, R = tt._make_kg(seed)
        with tempfile.TemporaryDirectory() as work:
            batches, totals = tt.run_reference_binary(pathlib.Path(work), tri, E, R)
        out[f"seed{seed}/triples"] = tri
        out[f"seed{seed}/batches"] = batches
        out[f"seed{seed}/totals"] = np.asarray(totals, dtype=np.int64)
    path = os.path.join(HERE, "transx_init_batches_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
