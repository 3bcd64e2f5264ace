"""Host: what ge_softmax_sampled_loss and ge_softmax_sampled_grad answer to bad arguments -- the table and the order of
tests/test_softmax_refusals_host.py --, their size function, and the driver's --softmax_samples flag.

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
W.CASES["ge_softmax_sampled_workspace_bytes"] = (
    [W.SIZES, W.SIZES[::3], (8, 64, 200, 288)],
    [(0, 5, 8), (5, 0, 8), (-1, 5, 8), (5, 5, 0), (5, 5, 7), (5, 5, 12), (5, 5, 296)], True)

host_only = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: host-only refusals")

EINVAL, ENOTSUP, ENOMEM = _lib.GE_EINVAL, _lib.GE_ENOTSUP, _lib.GE_ENOMEM
A = 1 << 12                                   # a fake, 256-byte aligned, never-dereferenced address

LOSS = ["table", "N", "d", "hr", "B", "true_id", "cand", "K", "max_norm", "scale", "model", "cand_is_head", "loss",
        "workspace", "workspace_bytes", "stream"]
GRAD = ["table", "N", "d", "hr", "B", "true_id", "cand", "K", "max_norm", "scale", "lr", "model", "cand_is_head", "loss",
        "grad_idx", "grad_val", "workspace", "workspace_bytes", "stream"]
GOOD = dict(table=A, N=100, d=8, hr=A, B=4, true_id=A, cand=A, K=9, max_norm=1.0, scale=20.0, lr=1.0, model=0, cand_is_head=0,
            loss=A, grad_idx=A, grad_val=A, workspace=A, workspace_bytes="NEED", stream=None)


def call(name, **kw):
    lib = _lib.load()
    a = dict(GOOD, **kw)
    if a["workspace_bytes"] in ("NEED", "NEED-1"):
        need = int(lib.ge_softmax_sampled_workspace_bytes(a["B"], a["K"], a["d"]))
        a["workspace_bytes"] = max(need, 1) - (a["workspace_bytes"] == "NEED-1")
    return getattr(lib, name)(*[a[n] for n in (LOSS if name == "ge_softmax_sampled_loss" else GRAD)])


def test_prototypes_and_version():
    lib = _lib.load()
    assert lib.ge_version() > 441
    S = _lib.SYMBOLS
    assert S["ge_softmax_sampled_loss"] == S["ge_softmax_loss"] and S["ge_softmax_sampled_grad"] == S["ge_softmax_grad"]
    assert S["ge_softmax_sampled_workspace_bytes"] == S["ge_softmax_workspace_bytes"]


def test_softmax_sampled_workspace_size_function():
    W.test_size_function("ge_softmax_sampled_workspace_bytes")
    fn, full = _lib.load().ge_softmax_sampled_workspace_bytes, _lib.load().ge_softmax_workspace_bytes
    # T', z_true and the candidate partials come on top of the unsampled layout; far below a [B, K] matrix all the same
    assert int(full(4096, 1024, 200)) < int(fn(4096, 1024, 200)) < 64 << 20
    assert int(full(4096, 14951, 200)) < int(fn(4096, 14951, 200)) < 96 << 20
    # never shrinks in any argument, every step of the way -- through every change of the number of query ranges
    # (tiles(B) up to 8, 512 / tiles(K) down to 1 at K = 32768)
    for d in (8, 200, 288):
        prev = 0
        for n in list(range(1, 700)) + list(range(700, 70000, 97)):
            v = int(fn(n, 300, d))
            assert v >= prev and v % 256 == 0
            prev = v
        prev = 0
        for n in list(range(1, 700)) + list(range(700, 70000, 97)):
            v = int(fn(130, n, d))
            assert v >= prev and v % 256 == 0
            prev = v
        prev = 0
        for n in list(range(3000, 40000, 61)):
            v = int(fn(4096, n, d))
            assert v >= prev and v % 256 == 0
            prev = v
    vals = [int(fn(130, 300, d)) for d in range(8, 289, 8)]
    assert vals == sorted(vals) and all(v > 0 for v in vals)


@host_only
@pytest.mark.parametrize("n", ["ge_softmax_sampled_loss", "ge_softmax_sampled_grad"])
def test_softmax_sampled_refuses_bad_arguments_without_launching(n):
    bad_einval = [dict(table=None), dict(hr=None), dict(true_id=None), dict(cand=None), dict(loss=None), dict(workspace=None),
                  dict(N=0), dict(N=-1), dict(B=0), dict(B=-3), dict(K=0), dict(K=-1), dict(d=0), dict(d=-8),
                  dict(scale=0.0), dict(scale=-1.0), dict(scale=math.inf), dict(scale=math.nan),
                  dict(max_norm=0.0), dict(max_norm=-1.0), dict(table=A + 4), dict(table=A + 8),
                  dict(workspace=A + 16), dict(workspace=A + 128)]
    if n == "ge_softmax_sampled_grad":
        bad_einval += [dict(grad_idx=None), dict(grad_val=None)]
    for bad in bad_einval:
        assert call(n, **bad) == EINVAL, bad
    for bad in (dict(d=4), dict(d=12), dict(d=7), dict(d=296), dict(d=1024), dict(model=1), dict(model=2), dict(model=3),
                dict(model=-1), dict(model=7)):
        assert call(n, **bad) == ENOTSUP, bad
    for ok_d in (8, 56, 200, 288):
        assert call(n, d=ok_d, workspace_bytes="NEED-1") == ENOMEM
    assert call(n, workspace_bytes=0) == ENOMEM
    # the unsampled calls' workspace is too small for these
    assert call(n, workspace_bytes=int(_lib.load().ge_softmax_workspace_bytes(4, 9, 8))) == ENOMEM
    # two at once: GE_EINVAL before GE_ENOTSUP before GE_ENOMEM
    assert call(n, scale=0.0, model=1) == EINVAL
    assert call(n, hr=None, d=12, workspace_bytes=0) == EINVAL
    assert call(n, model=1, workspace_bytes=0) == ENOTSUP


# ------------------------------------------------------------------------------------------------ the driver's flags
def parse(*argv):
    return T.build_parser().parse_args(["--data_dir", "D", "--output_dir", "O", *argv])


def test_hinge_default_is_unchanged():
    a, b = parse(), parse("--objective", "hinge")
    assert a.objective == "hinge" and a.softmax_samples == 0 and vars(a) == vars(b)
    T.check_objective_flags(a)
    T.check_objective_flags(parse("--log_loss"))
    T.check_objective_flags(parse("--model", "hole", "--gpus", "2"))


def test_softmax_samples_flag():
    soft = ["--objective", "softmax", "--optimizer", "adagrad"]
    assert parse(*soft).softmax_samples == 0
    T.check_objective_flags(parse(*soft))
    T.check_objective_flags(parse(*soft, "--softmax_samples", "0"))
    ok = parse(*soft, "--softmax_samples", "32")
    assert ok.softmax_samples == 32
    T.check_objective_flags(ok)
    for argv in ([*soft, "--softmax_samples", "-1"], ["--softmax_samples", "-1"], ["--softmax_samples", "32"],
                 ["--objective", "hinge", "--softmax_samples", "32"], ["--optimizer", "adagrad", "--softmax_samples", "1"]):
        with pytest.raises(SystemExit) as e:
            T.check_objective_flags(parse(*argv))
        assert isinstance(e.value.code, str) and "softmax_samples" in e.value.code, (argv, e.value.code)
    # the sampled objective is refused with what the objective is refused with
    for extra, word in ((["--optimizer", "sgd"], "adagrad"), (["--optimizer", "adagrad", "--model", "hole"], "hole"),
                        (["--optimizer", "adagrad", "--gpus", "2"], "gpus")):
        with pytest.raises(SystemExit) as e:
            T.check_objective_flags(parse("--objective", "softmax", "--softmax_samples", "32", *extra))
        assert isinstance(e.value.code, str) and word in e.value.code, (extra, e.value.code)
    with pytest.raises(SystemExit):
        parse("--softmax_samples", "many")
