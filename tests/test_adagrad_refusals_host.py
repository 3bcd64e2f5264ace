"""Host: what ge_adagrad_rows and ge_train_steps_adagrad answer to bad arguments, and their size function.

As in test_train_refusals_host.py nothing here reaches a kernel: every case carries an argument the entry point refuses,
or a count of 0, which returns before any launch, and every pointer is a fake address that is never dereferenced.  The
refusal cases are skipped where a GPU is visible, so that a case that slipped through validation could never launch on a
fake pointer."""
import pytest
import torch

import test_abi_workspace_host as W
from graphembeddings_amd import _lib

# The size function joins the table test_abi_workspace_host.py checks (its test_every_size_function_is_listed reads CASES
# when it runs, after every module is collected): ge_train_workspace_bytes' grid and bad sizes.
W.CASES["ge_train_adagrad_workspace_bytes"] = ([W.SIZES, (8, 200)], [(0, 8), (-1, 8), (5, 0)], True)

host_only = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: host-only refusals")

EINVAL, ENOTSUP, ENOMEM = _lib.GE_EINVAL, _lib.GE_ENOTSUP, _lib.GE_ENOMEM
A = 1 << 12                                   # a fake, 256-byte aligned, never-dereferenced address
ACC = A + (1 << 20)                           # 100 x 8 floats behind A end far in front of it

ROWS = ["table", "accum", "N", "d", "idx", "val", "perm", "R", "lr", "stream"]
LOOP = ["table", "accum", "N", "d", "triples", "T", "first_row", "B", "n_steps", "id_to_type", "type_offsets", "n_types",
        "type_ids", "seed", "step", "padded_size", "mode", "margin", "lr0", "decay_steps", "decay_rate", "max_norm", "model",
        "loss", "keep", "neg_ws", "workspace", "workspace_bytes", "pipeline", "stream"]
GOOD = dict(table=A, accum=ACC, N=100, d=8, idx=A, val=A, perm=A, R=0, lr=0.1, triples=A, T=100, first_row=0, B=4, n_steps=0,
            id_to_type=A, type_offsets=A, n_types=2, type_ids=A, seed=7, step=0, padded_size=16, mode=0, margin=0.2, lr0=0.1,
            decay_steps=0.0, decay_rate=0.5, max_norm=1.0, model=0, loss=A, keep=0, neg_ws=A, workspace=A,
            workspace_bytes="NEED", pipeline=None, stream=None)


def call(name, **kw):
    lib = _lib.load()
    a = dict(GOOD, **kw)
    if a["workspace_bytes"] in ("NEED", "NEED-1"):
        need = int(lib.ge_train_adagrad_workspace_bytes(a["B"], a["d"]))
        assert need > 0 or a["workspace_bytes"] == "NEED"
        a["workspace_bytes"] = need - (a["workspace_bytes"] == "NEED-1")
    return getattr(lib, name)(*[a[n] for n in (ROWS if name == "ge_adagrad_rows" else LOOP)])


def test_prototypes_and_version():
    lib = _lib.load()
    assert lib.ge_version() >= 420
    assert len(ROWS) == len(_lib.SYMBOLS["ge_adagrad_rows"][1]) and len(LOOP) == len(_lib.SYMBOLS["ge_train_steps_adagrad"][1])


def test_adagrad_workspace_size_function():
    W.test_size_function("ge_train_adagrad_workspace_bytes")
    fn = _lib.load().ge_train_adagrad_workspace_bytes
    # never shrinks as B grows: every B up to 20,000, every 7th up to 300,000 and the neighbours of the powers of two
    Bs = sorted(set(range(1, 20001)) | set(range(20001, 300001, 7)) | {(1 << p) + o for p in range(15, 23) for o in (-1, 0, 1)})
    for d in (8, 200):
        prev = 0
        for B in Bs:
            v = int(fn(B, d))
            assert v >= prev and v % 256 == 0, (B, d, v, prev)
            prev = v


@host_only
def test_adagrad_rows_refuses_bad_arguments_without_launching():
    n = "ge_adagrad_rows"
    assert call(n) == 0                                    # R = 0: nothing to do
    assert call(n, idx=None, val=None, perm=None) == 0     # ... and the slices matter only when R > 0
    for bad in (dict(table=None), dict(accum=None), dict(N=0), dict(d=0), dict(R=-1), dict(accum=A), dict(accum=A + 4),
                dict(accum=A - 4), dict(accum=A + 100 * 8 * 4 - 4), dict(table=A + 2), dict(accum=ACC + 1),
                dict(R=5, idx=None), dict(R=5, val=None), dict(R=5, perm=None), dict(R=5, accum=None)):
        assert call(n, **bad) == EINVAL, bad
    assert call(n, accum=A + 100 * 8 * 4) == 0             # the accumulator may start where the table ends
    assert call(n, table=A + 100 * 8 * 4, accum=A) == 0


@host_only
def test_train_steps_adagrad_refuses_bad_arguments_without_launching():
    n = "ge_train_steps_adagrad"
    assert call(n) == 0                                    # no steps
    for m in (0, 1, 3):
        assert call(n, model=m) == 0
    assert call(n, model=1, d=7) == 0                      # HolE on the real table takes an odd width
    bad_einval = [dict(accum=None), dict(accum=A), dict(accum=A + 64), dict(accum=ACC + 2), dict(table=A + 1),
                  dict(table=None), dict(N=0), dict(d=0), dict(max_norm=0.0), dict(B=0), dict(B=-1), dict(n_steps=-1),
                  dict(first_row=-1), dict(T=3), dict(triples=None), dict(loss=None), dict(neg_ws=None), dict(workspace=None),
                  dict(workspace=A + 16), dict(workspace=A + 128), dict(model=-1), dict(model=4), dict(model=0x100),
                  dict(id_to_type=None), dict(type_offsets=None), dict(type_ids=None),
                  # the sampler's ranges, as ge_train_steps refuses them
                  dict(mode=-1), dict(mode=4), dict(padded_size=-1), dict(n_types=-1)]
    for bad in bad_einval:
        assert call(n, **bad) == EINVAL, bad
        assert call(n, **dict(dict(n_steps=1), **bad)) == EINVAL, bad          # ... in front of the step count
    for ok in (dict(mode=3), dict(padded_size=0), dict(n_types=0)):
        assert call(n, **ok) == 0
    # the spectral table is not supported, with or without steps
    assert call(n, model=2) == ENOTSUP and call(n, model=2, n_steps=1) == ENOTSUP
    assert call(n, d=1 << 20, accum=A + (1 << 40)) == ENOTSUP   # wider than the update kernels
    # widths the gradient kernel of the step refuses (tests/complex_shape_cases.py REFUSED): before anything is launched
    for bad in (dict(d=258), dict(d=1022), dict(d=512, table=A + 4), dict(d=520, table=A + 8)):
        assert call(n, n_steps=1, **bad) == ENOTSUP, bad
        assert call(n, **bad) == 0 and call(n, n_steps=1, workspace_bytes="NEED-1", **bad) == ENOMEM, bad
    assert call(n, n_steps=1, model=1, d=1022) == ENOTSUP and call(n, n_steps=1, model=3, d=520) == ENOTSUP
    assert call(n, n_steps=1, d=7) == EINVAL               # the ComplEx pairs take no odd width
    # the prepared path only: one byte short is refused, whatever the step count
    assert call(n, workspace_bytes="NEED-1") == ENOMEM and call(n, workspace_bytes="NEED-1", n_steps=1) == ENOMEM
    assert call(n, workspace_bytes=0, n_steps=1) == ENOMEM
    lib = _lib.load()
    assert call(n, workspace_bytes=int(lib.ge_hinge_step_workspace_bytes(4, 8)), n_steps=1) == ENOMEM   # no fallback branch
    # two at once: GE_EINVAL before GE_ENOTSUP before GE_ENOMEM
    assert call(n, accum=None, workspace_bytes=0) == EINVAL
    assert call(n, mode=4, model=2) == EINVAL
    assert call(n, model=2, workspace_bytes=0) == ENOTSUP
