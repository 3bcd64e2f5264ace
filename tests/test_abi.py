"""The C-ABI library loads and exports every symbol include/ge_hip.h declares (no GPU needed;
no compute entry point is called here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "ge_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ge_[a-z0-9_A-Z]+)\s*\(", src)))


def _prototypes():
    """{name: (return type, [argument types])} of every ge_* prototype in ge_hip.h; a pointer is "*"."""
    src = open(os.path.join(ROOT, "include", "ge_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r"^\s*([a-z_0-9]+)\s+(ge_[a-z0-9_A-Z]+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        args = [a.strip() for a in args.split(",")] if args.strip() != "void" else []
        # "const int32_t* pos" -> "*", "int64_t N" -> "int64_t"
        protos[name] = (ret, ["*" if "*" in a else a.replace("const ", "").split()[0] for a in args])
    return protos


def test_ctypes_table_matches_header_prototypes():
    """_lib.SYMBOLS passes every argument with the C type ge_hip.h gives it (a width mismatch would pass garbage)."""
    from graphembeddings_amd import _lib
    scalar = {"int": {ctypes.c_int, ctypes.c_int32}, "int32_t": {ctypes.c_int, ctypes.c_int32},
              "int64_t": {ctypes.c_int64}, "uint64_t": {ctypes.c_uint64}, "uint32_t": {ctypes.c_uint32},
              "size_t": {ctypes.c_size_t}, "float": {ctypes.c_float}}
    protos = _prototypes()
    assert set(protos) == set(_declared()), "prototype parser missed a declaration"
    for name, (ret, args) in protos.items():
        res, argtypes = _lib.SYMBOLS[name]
        assert res in scalar[ret], f"{name}: returns {ret}, ctypes restype {res.__name__}"
        assert len(argtypes) == len(args), f"{name}: {len(args)} arguments in ge_hip.h, {len(argtypes)} in SYMBOLS"
        for i, (c, py) in enumerate(zip(args, argtypes)):
            if c == "*":
                assert py is ctypes.c_void_p or issubclass(py, ctypes._Pointer), f"{name} argument {i}: pointer"
            else:
                assert py in scalar[c], f"{name} argument {i}: {c} in ge_hip.h, {py.__name__} in SYMBOLS"


def test_header_declares_expected_entry_points():
    names = _declared()
    for must in ("ge_complex_score", "ge_hole_score", "ge_complex_hinge_step", "ge_hole_hinge_step",
                 "ge_corrupt_batch", "ge_complex_score_1vK", "ge_hinge_grad", "ge_scatter_add_rows", "ge_shard_plan", "ge_shard_grad", "ge_shard_apply",
                 "ge_gather_rows", "ge_hinge_loss", "ge_version"):
        assert must in names


def test_library_builds_loads_and_exports_every_declared_symbol():
    from graphembeddings_amd import _lib, build
    path = build.build()
    assert os.path.exists(path)
    lib = ctypes.CDLL(path)
    for name in _declared():
        assert hasattr(lib, name), f"{name} declared in ge_hip.h but not exported"
    assert set(_declared()) == set(_lib.SYMBOLS), "ctypes table and header diverge"
    loaded = _lib.load()
    assert loaded.ge_version() >= 300
    assert loaded.ge_max_dim() >= 200
    # pure host helper: workspace = 6B int32 (256-B padded) + 6B*d fp32
    assert loaded.ge_hinge_step_workspace_bytes(4096, 200) == 6 * 4096 * 4 + 6 * 4096 * 200 * 4
    assert loaded.ge_hinge_step_workspace_bytes(0, 200) == 0


def test_product_path_has_no_cpu_fallback():
    import torch
    from graphembeddings_amd import hole
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="CUDA"):
        hole.evaluate_triples(torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 8))


def test_product_code_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "graphembeddings_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f
                assert "libge_oracle" not in text, f
