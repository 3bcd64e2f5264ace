"""Host: what ge_softmax_masked_loss and ge_softmax_masked_grad answer to bad arguments -- the table and the order of
tests/test_softmax_refusals_host.py with the sets' arguments in their groups --, their size function, and the driver's
--softmax_candidate_sets flag.

Nothing here reaches a kernel: every call carries an argument the entry point refuses, and every pointer is a fake
address that is never dereferenced.  The refusal cases are skipped where a GPU is visible, so that a case that slipped
through validation could never launch on a fake pointer."""
import math

import pytest
import torch

import test_abi_workspace_host as W
from graphembeddings_amd import _lib
from graphembeddings_amd import train as T

# The size function joins the table test_abi_workspace_host.py checks (its test_every_size_function_is_listed reads CASES
# when it runs, after every module is collected)
W.CASES["ge_softmax_masked_workspace_bytes"] = (
    [W.SIZES, W.SIZES[::3], (8, 64, 200, 288)],
    [(0, 5, 8), (5, 0, 8), (-1, 5, 8), (5, 5, 0), (5, 5, 7), (5, 5, 12), (5, 5, 296)], True)

host_only = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: host-only refusals")

EINVAL, ENOTSUP, ENOMEM = _lib.GE_EINVAL, _lib.GE_ENOTSUP, _lib.GE_ENOMEM
A = 1 << 12                                   # a fake, 256-byte aligned, never-dereferenced address

LOSS = ["table", "N", "d", "hr", "B", "true_id", "cand", "K", "max_norm", "scale", "model", "cand_is_head", "loss",
        "workspace", "workspace_bytes", "row_set", "mask", "n_sets", "stream"]
GRAD = ["table", "N", "d", "hr", "B", "true_id", "cand", "K", "max_norm", "scale", "lr", "model", "cand_is_head", "loss",
        "grad_idx", "grad_val", "workspace", "workspace_bytes", "row_set", "mask", "n_sets", "stream"]
GOOD = dict(table=A, N=100, d=8, hr=A, B=4, true_id=A, cand=A, K=9, max_norm=1.0, scale=20.0, lr=1.0, model=0, cand_is_head=0,
            loss=A, grad_idx=A, grad_val=A, workspace=A, workspace_bytes="NEED", row_set=A, mask=A, n_sets=3, stream=None)


def call(name, **kw):
    lib = _lib.load()
    a = dict(GOOD, **kw)
    if a["workspace_bytes"] in ("NEED", "NEED-1"):
        need = int(lib.ge_softmax_masked_workspace_bytes(a["B"], a["K"], a["d"]))
        a["workspace_bytes"] = max(need, 1) - (a["workspace_bytes"] == "NEED-1")
    return getattr(lib, name)(*[a[n] for n in (LOSS if name == "ge_softmax_masked_loss" else GRAD)])


def test_prototypes_and_version():
    lib = _lib.load()
    assert lib.ge_version() >= 443
    S = _lib.SYMBOLS
    for new, old in (("ge_softmax_masked_loss", "ge_softmax_loss"), ("ge_softmax_masked_grad", "ge_softmax_grad")):
        # the unmasked call's arguments up to workspace_bytes, then row_set, mask, n_sets, stream
        assert S[new][0] == S[old][0] and S[new][1][:-4] == S[old][1][:-1]
        assert S[new][1][-4:] == [_lib._p, _lib._p, _lib._i32, _lib._p]
    assert S["ge_softmax_masked_workspace_bytes"] == S["ge_softmax_workspace_bytes"]


def test_softmax_masked_workspace_size_function():
    W.test_size_function("ge_softmax_masked_workspace_bytes")
    fn, full = _lib.load().ge_softmax_masked_workspace_bytes, _lib.load().ge_softmax_workspace_bytes
    # one bit per (64-row, 64-candidate) tile pair on top of the unmasked layout, in rows of whole word pairs
    for B, K, d in ((1, 1, 8), (130, 300, 64), (4096, 14951, 200), (70000, 70000, 288)):
        tb, tk = (B + 63) // 64, (K + 63) // 64
        live = 4 * tb * 2 * ((tk + 63) // 64)
        assert int(fn(B, K, d)) == int(full(B, K, d)) + (live + 255) // 256 * 256
    assert int(fn(4096, 14951, 200)) - int(full(4096, 14951, 200)) < 4096
    for d in (8, 200, 288):
        for fixed in (lambda n: (n, 300, d), lambda n: (130, n, d)):
            prev = 0
            for n in list(range(1, 700)) + list(range(700, 70000, 97)):
                v = int(fn(*fixed(n)))
                assert v >= prev and v % 256 == 0
                prev = v
    vals = [int(fn(130, 300, d)) for d in range(8, 289, 8)]
    assert vals == sorted(vals) and all(v > 0 for v in vals)


@host_only
@pytest.mark.parametrize("n", ["ge_softmax_masked_loss", "ge_softmax_masked_grad"])
def test_softmax_masked_refuses_bad_arguments_without_launching(n):
    bad_einval = [dict(table=None), dict(hr=None), dict(true_id=None), dict(cand=None), dict(loss=None), dict(workspace=None),
                  dict(N=0), dict(N=-1), dict(B=0), dict(B=-3), dict(K=0), dict(K=-1), dict(d=0), dict(d=-8),
                  dict(scale=0.0), dict(scale=-1.0), dict(scale=math.inf), dict(scale=math.nan),
                  dict(max_norm=0.0), dict(max_norm=-1.0), dict(table=A + 4), dict(table=A + 8),
                  dict(workspace=A + 16), dict(workspace=A + 128),
                  dict(row_set=None), dict(mask=None), dict(n_sets=0), dict(n_sets=-1), dict(mask=A + 1), dict(mask=A + 2)]
    if n == "ge_softmax_masked_grad":
        bad_einval += [dict(grad_idx=None), dict(grad_val=None), dict(grad_val=A + 2)]
    for bad in bad_einval:
        assert call(n, **bad) == EINVAL, bad
    for bad in (dict(d=4), dict(d=12), dict(d=7), dict(d=296), dict(d=1024), dict(model=1), dict(model=2), dict(model=3),
                dict(model=-1), dict(model=7)):
        assert call(n, **bad) == ENOTSUP, bad
    for ok_d in (8, 56, 200, 288):
        assert call(n, d=ok_d, workspace_bytes="NEED-1") == ENOMEM
    assert call(n, workspace_bytes=0) == ENOMEM
    # the unmasked calls' workspace is too small for these: the bitmap comes on top
    assert call(n, workspace_bytes=int(_lib.load().ge_softmax_workspace_bytes(4, 9, 8))) == ENOMEM
    # the order: the null pointers and n_sets with GE_EINVAL's first group, before GE_ENOTSUP; the alignments (the mask's
    # among them) after GE_ENOTSUP and before GE_ENOMEM
    assert call(n, scale=0.0, model=1) == EINVAL
    assert call(n, hr=None, d=12, workspace_bytes=0) == EINVAL
    assert call(n, row_set=None, d=12, workspace_bytes=0) == EINVAL
    assert call(n, mask=None, model=1) == EINVAL
    assert call(n, n_sets=0, model=1, workspace_bytes=0) == EINVAL
    assert call(n, mask=A + 2, model=1) == ENOTSUP
    assert call(n, mask=A + 2, d=12) == ENOTSUP
    assert call(n, mask=A + 2, workspace_bytes=0) == EINVAL
    assert call(n, workspace=A + 16, workspace_bytes=0) == EINVAL
    assert call(n, model=1, workspace_bytes=0) == ENOTSUP


# ------------------------------------------------------------------------------------------------ the driver's flags
def parse(*argv):
    return T.build_parser().parse_args(["--data_dir", "D", "--output_dir", "O", *argv])


def test_default_is_unchanged():
    a, b = parse(), parse("--softmax_candidate_sets", "none")
    assert a.softmax_candidate_sets == "none" and vars(a) == vars(b)
    T.check_objective_flags(a)
    T.check_objective_flags(parse("--objective", "softmax", "--optimizer", "adagrad"))
    T.check_objective_flags(parse("--objective", "softmax", "--optimizer", "adagrad", "--softmax_samples", "32"))


def test_softmax_candidate_sets_flag():
    soft = ["--objective", "softmax", "--optimizer", "adagrad"]
    for kind in ("types", "observed"):
        ok = parse(*soft, "--softmax_candidate_sets", kind)
        assert ok.softmax_candidate_sets == kind
        T.check_objective_flags(ok)
        T.check_objective_flags(parse(*soft, "--softmax_candidate_sets", kind, "--softmax_samples", "0"))
        for argv in (["--softmax_candidate_sets", kind], ["--objective", "hinge", "--softmax_candidate_sets", kind],
                     ["--optimizer", "adagrad", "--softmax_candidate_sets", kind],
                     [*soft, "--softmax_candidate_sets", kind, "--softmax_samples", "32"]):
            with pytest.raises(SystemExit) as e:
                T.check_objective_flags(parse(*argv))
            assert isinstance(e.value.code, str) and "softmax_candidate_sets" in e.value.code, (argv, e.value.code)
        # refused with what the objective is refused with
        for extra, word in ((["--optimizer", "sgd"], "adagrad"), (["--optimizer", "adagrad", "--model", "hole"], "hole"),
                            (["--optimizer", "adagrad", "--gpus", "2"], "gpus"), (["--optimizer", "adagrad", "--log_loss"], "log_loss")):
            with pytest.raises(SystemExit) as e:
                T.check_objective_flags(parse("--objective", "softmax", "--softmax_candidate_sets", kind, *extra))
            assert isinstance(e.value.code, str) and word in e.value.code, (extra, e.value.code)
    # the existing messages stay
    with pytest.raises(SystemExit) as e:
        T.check_objective_flags(parse("--softmax_samples", "32", "--softmax_candidate_sets", "types"))
    assert "softmax_samples needs --objective softmax" in e.value.code
    with pytest.raises(SystemExit):
        parse("--softmax_candidate_sets", "all")
