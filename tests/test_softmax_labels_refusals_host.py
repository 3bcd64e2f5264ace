"""Host: what ge_softmax_labels_loss and ge_softmax_labels_grad answer to bad arguments -- the table and the order of
tests/test_softmax_refusals_host.py with the labels' arguments in their groups --, their size function, and the driver's
--softmax_labels flag.

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
# when it runs, after every module is collected); L = 0 is a size the calls take
W.CASES["ge_softmax_labels_workspace_bytes"] = (
    [W.SIZES, W.SIZES[::3], (8, 64, 200, 288), [0] + W.SIZES],
    [(0, 5, 8, 3), (5, 0, 8, 3), (-1, 5, 8, 3), (5, 5, 0, 3), (5, 5, 7, 3), (5, 5, 12, 3), (5, 5, 296, 3), (5, 5, 8, -1)], True)

host_only = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: host-only refusals")

EINVAL, ENOTSUP, ENOMEM = _lib.GE_EINVAL, _lib.GE_ENOTSUP, _lib.GE_ENOMEM
A = 1 << 12                                   # a fake, 256-byte aligned, never-dereferenced address

LOSS = ["table", "N", "d", "hr", "B", "label_off", "label_pos", "L", "cand", "K", "max_norm", "scale", "model", "cand_is_head",
        "loss", "workspace", "workspace_bytes", "stream"]
GRAD = ["table", "N", "d", "hr", "B", "label_off", "label_pos", "L", "cand", "K", "max_norm", "scale", "lr", "model",
        "cand_is_head", "loss", "grad_idx", "grad_val", "workspace", "workspace_bytes", "stream"]
GOOD = dict(table=A, N=100, d=8, hr=A, B=4, label_off=A, label_pos=A, L=11, cand=A, K=9, max_norm=1.0, scale=20.0, lr=1.0,
            model=0, cand_is_head=0, loss=A, grad_idx=A, grad_val=A, workspace=A, workspace_bytes="NEED", stream=None)


def call(name, **kw):
    lib = _lib.load()
    a = dict(GOOD, **kw)
    if a["workspace_bytes"] in ("NEED", "NEED-1"):
        need = int(lib.ge_softmax_labels_workspace_bytes(a["B"], a["K"], a["d"], a["L"]))
        a["workspace_bytes"] = max(need, 1) - (a["workspace_bytes"] == "NEED-1")
    return getattr(lib, name)(*[a[n] for n in (LOSS if name == "ge_softmax_labels_loss" else GRAD)])


def test_prototypes_and_version():
    lib = _lib.load()
    assert lib.ge_version() >= 444
    S = _lib.SYMBOLS
    for new, old in (("ge_softmax_labels_loss", "ge_softmax_loss"), ("ge_softmax_labels_grad", "ge_softmax_grad")):
        # the 1-vs-all call's arguments with true_id replaced by label_off, label_pos, L
        assert S[new][0] == S[old][0]
        assert S[new][1] == S[old][1][:5] + [_lib._p, _lib._p, _lib._i64] + S[old][1][6:]
    assert S["ge_softmax_labels_workspace_bytes"] == (S["ge_softmax_workspace_bytes"][0],
                                                      S["ge_softmax_workspace_bytes"][1] + [_lib._i64])


def test_softmax_labels_workspace_size_function():
    W.test_size_function("ge_softmax_labels_workspace_bytes")
    fn, full = _lib.load().ge_softmax_labels_workspace_bytes, _lib.load().ge_softmax_workspace_bytes
    up = lambda v: (v + 255) // 256 * 256
    # the 1-vs-all layout, then the label-sum rows [B,d] fp32, the label means [B] fp64 and the row of every entry [L] int32
    for B, K, d, L in ((1, 1, 8, 0), (1, 1, 8, 1), (130, 300, 64, 517), (4096, 14951, 200, 40000), (70000, 70000, 288, 1 << 20)):
        assert int(fn(B, K, d, L)) == int(full(B, K, d)) + up(4 * B * d) + up(8 * B) + up(4 * L)
    for d in (8, 200, 288):
        for fixed in (lambda n: (n, 300, d, 77), lambda n: (130, n, d, 77), lambda n: (130, 300, d, n)):
            prev = 0
            for n in list(range(1, 700)) + list(range(700, 70000, 97)):
                v = int(fn(*fixed(n)))
                assert v >= prev and v % 256 == 0
                prev = v
    vals = [int(fn(130, 300, d, 77)) for d in range(8, 289, 8)]
    assert vals == sorted(vals) and all(v > 0 for v in vals)


@host_only
@pytest.mark.parametrize("n", ["ge_softmax_labels_loss", "ge_softmax_labels_grad"])
def test_softmax_labels_refuses_bad_arguments_without_launching(n):
    bad_einval = [dict(table=None), dict(hr=None), dict(label_off=None), dict(label_pos=None), dict(cand=None), dict(loss=None),
                  dict(workspace=None), dict(N=0), dict(N=-1), dict(B=0), dict(B=-3), dict(K=0), dict(K=-1), dict(d=0), dict(d=-8),
                  dict(L=-1), dict(L=-100),
                  dict(scale=0.0), dict(scale=-1.0), dict(scale=math.inf), dict(scale=math.nan),
                  dict(max_norm=0.0), dict(max_norm=-1.0), dict(table=A + 4), dict(table=A + 8),
                  dict(workspace=A + 16), dict(workspace=A + 128)]
    if n == "ge_softmax_labels_grad":
        bad_einval += [dict(grad_idx=None), dict(grad_val=None), dict(grad_val=A + 2)]
    for bad in bad_einval:
        assert call(n, **bad) == EINVAL, bad
    for bad in (dict(d=4), dict(d=12), dict(d=7), dict(d=296), dict(d=1024), dict(model=1), dict(model=2), dict(model=3),
                dict(model=-1), dict(model=7), dict(N=1 << 31)):
        assert call(n, **bad) == ENOTSUP, bad
    for ok_d in (8, 56, 200, 288):
        assert call(n, d=ok_d, workspace_bytes="NEED-1") == ENOMEM
    assert call(n, workspace_bytes=0) == ENOMEM
    assert call(n, L=0, workspace_bytes="NEED-1") == ENOMEM                  # L = 0 is taken as far as the size check
    # the 1-vs-all calls' workspace is too small for these: the label parts come on top
    assert call(n, workspace_bytes=int(_lib.load().ge_softmax_workspace_bytes(4, 9, 8))) == ENOMEM
    # the order: the null pointers and L < 0 with GE_EINVAL's first group, before GE_ENOTSUP; the alignments after
    # GE_ENOTSUP and before GE_ENOMEM
    assert call(n, scale=0.0, model=1) == EINVAL
    assert call(n, hr=None, d=12, workspace_bytes=0) == EINVAL
    assert call(n, label_off=None, d=12, workspace_bytes=0) == EINVAL
    assert call(n, label_pos=None, model=1) == EINVAL
    assert call(n, L=-1, model=1, workspace_bytes=0) == EINVAL
    assert call(n, table=A + 8, model=1) == ENOTSUP
    assert call(n, workspace=A + 16, d=12) == ENOTSUP
    assert call(n, workspace=A + 16, workspace_bytes=0) == EINVAL
    assert call(n, model=1, workspace_bytes=0) == ENOTSUP


# ------------------------------------------------------------------------------------------------ the driver's flags
def parse(*argv):
    return T.build_parser().parse_args(["--data_dir", "D", "--output_dir", "O", *argv])


def test_default_is_unchanged():
    a, b = parse(), parse("--softmax_labels", "one")
    assert a.softmax_labels == "one" and vars(a) == vars(b)
    T.check_objective_flags(a)
    soft = ["--objective", "softmax", "--optimizer", "adagrad"]
    T.check_objective_flags(parse(*soft))
    T.check_objective_flags(parse(*soft, "--softmax_labels", "one", "--softmax_samples", "32"))
    T.check_objective_flags(parse(*soft, "--softmax_labels", "one", "--softmax_candidate_sets", "types"))


def test_softmax_labels_flag():
    soft = ["--objective", "softmax", "--optimizer", "adagrad"]
    ok = parse(*soft, "--softmax_labels", "all")
    assert ok.softmax_labels == "all"
    T.check_objective_flags(ok)
    T.check_objective_flags(parse(*soft, "--softmax_labels", "all", "--softmax_samples", "0", "--softmax_candidate_sets", "none"))
    for argv in (["--softmax_labels", "all"], ["--objective", "hinge", "--softmax_labels", "all"],
                 ["--optimizer", "adagrad", "--softmax_labels", "all"],
                 [*soft, "--softmax_labels", "all", "--softmax_samples", "32"],
                 [*soft, "--softmax_labels", "all", "--softmax_candidate_sets", "types"],
                 [*soft, "--softmax_labels", "all", "--softmax_candidate_sets", "observed"]):
        with pytest.raises(SystemExit) as e:
            T.check_objective_flags(parse(*argv))
        assert isinstance(e.value.code, str) and "softmax_labels" in e.value.code, (argv, e.value.code)
    # refused with what the objective is refused with
    for extra, word in ((["--optimizer", "sgd"], "adagrad"), (["--optimizer", "adagrad", "--model", "hole"], "hole"),
                        (["--optimizer", "adagrad", "--gpus", "2"], "gpus"), (["--optimizer", "adagrad", "--log_loss"], "log_loss")):
        with pytest.raises(SystemExit) as e:
            T.check_objective_flags(parse("--objective", "softmax", "--softmax_labels", "all", *extra))
        assert isinstance(e.value.code, str) and word in e.value.code, (extra, e.value.code)
    # the existing messages stay
    with pytest.raises(SystemExit) as e:
        T.check_objective_flags(parse("--softmax_samples", "32", "--softmax_labels", "all"))
    assert "softmax_samples needs --objective softmax" in e.value.code
    with pytest.raises(SystemExit) as e:
        T.check_objective_flags(parse(*soft, "--softmax_candidate_sets", "types", "--softmax_samples", "32", "--softmax_labels", "all"))
    assert "softmax_candidate_sets belongs to the 1-vs-all objective" in e.value.code
    with pytest.raises(SystemExit):
        parse("--softmax_labels", "some")
