"""Host: what ge_rank_metrics and ge_rank_validation_tick answer to bad arguments -- codes and order --, the tick's size
function, and the driver's --softmax_validation_ticks / --softmax_validation_rows / --softmax_patience flags.

Nothing here reaches a kernel: every call carries an argument the entry point refuses, and every pointer is a fake
address that is never dereferenced.  The refusal cases are skipped where a GPU is visible, so that a case that slipped
through validation could never launch on a fake pointer."""
import pytest
import torch

import test_abi_workspace_host as W
from graphembeddings_amd import _lib
from graphembeddings_amd import train as T

# the size function joins the table test_abi_workspace_host.py checks (read when its test runs, after collection)
W.CASES["ge_rank_tick_workspace_bytes"] = ([W.SIZES], [(0,), (-1,), (-1 << 40,)], True)

host_only = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: host-only refusals")

EINVAL, ENOTSUP, ENOMEM = _lib.GE_EINVAL, _lib.GE_ENOTSUP, _lib.GE_ENOMEM
A = 1 << 12                                   # a fake, 256-byte aligned, never-dereferenced address

METRICS = ["n_before", "n_known_before", "true_loss", "M", "metrics_out", "best", "improved", "stream"]
TICK = ["table", "N", "d", "hr", "true_id", "V", "cand", "K", "max_norm", "model", "known_off_tail", "known_rc_tail",
        "known_off_head", "known_rc_head", "planes", "row_set", "mask_tail", "mask_head", "n_sets", "accumulator", "metrics_out",
        "best", "pocket", "pocket_accumulator", "workspace", "workspace_bytes", "stream"]
GOOD = dict(table=A, N=300, d=64, hr=A, true_id=A, V=5, cand=A, K=292, max_norm=1.0, model=0, known_off_tail=A, known_rc_tail=A,
            known_off_head=A, known_rc_head=A, planes=A, row_set=None, mask_tail=None, mask_head=None, n_sets=0, accumulator=A,
            metrics_out=A, best=A, pocket=A, pocket_accumulator=A, workspace=A, workspace_bytes="NEED", stream=None)
SETS = dict(row_set=A, mask_tail=A, mask_head=A, n_sets=8)


def tick(**kw):
    lib = _lib.load()
    a = dict(GOOD, **kw)
    if a["workspace_bytes"] in ("NEED", "NEED-1"):
        need = int(lib.ge_rank_tick_workspace_bytes(a["V"]))
        a["workspace_bytes"] = max(need, 1) - (a["workspace_bytes"] == "NEED-1")
    return lib.ge_rank_validation_tick(*[a[n] for n in TICK])


def metrics(**kw):
    a = dict(dict(n_before=A, n_known_before=A, true_loss=A, M=10, metrics_out=A, best=A, improved=A, stream=None), **kw)
    return _lib.load().ge_rank_metrics(*[a[n] for n in METRICS])


def test_prototypes_and_version():
    lib = _lib.load()
    assert lib.ge_version() >= 445
    S = _lib.SYMBOLS
    assert len(S["ge_rank_metrics"][1]) == len(METRICS) and len(S["ge_rank_validation_tick"][1]) == len(TICK)
    assert S["ge_rank_tick_workspace_bytes"] == (_lib._sz, [_lib._i64])


def test_rank_tick_workspace_size_function():
    W.test_size_function("ge_rank_tick_workspace_bytes")
    fn = _lib.load().ge_rank_tick_workspace_bytes
    up = lambda v: (v + 255) // 256 * 256
    prev = 0
    for V in list(range(1, 3000)) + list(range(3000, 1 << 23, 4099)) + [1 << 23]:
        v = int(fn(V))
        # two int32 counts and a float true loss per row of both sides, and the flag
        assert v == up(2 * V * 12 + 16) and v >= prev and v % 256 == 0
        prev = v
    for V in (0, -1, -(1 << 33)):
        assert int(fn(V)) == 0


@host_only
def test_rank_metrics_refuses_bad_arguments_without_launching():
    for bad in (dict(n_before=None), dict(n_known_before=None), dict(metrics_out=None), dict(M=0), dict(M=-1)):
        assert metrics(**bad) == EINVAL, bad
    assert metrics(M=(1 << 24) + 1) == ENOTSUP
    assert metrics(M=1 << 40) == ENOTSUP
    # the order: a null pointer before the row limit
    assert metrics(M=(1 << 24) + 1, metrics_out=None) == EINVAL
    assert metrics(M=(1 << 24) + 1, n_before=None) == EINVAL


@host_only
def test_rank_tick_refuses_bad_arguments_without_launching():
    # the tick's own refusals
    for bad in (dict(V=0), dict(V=-1), dict(K=0), dict(K=-1), dict(metrics_out=None), dict(best=None), dict(workspace=None),
                dict(row_set=A), dict(mask_tail=A), dict(mask_head=A), dict(row_set=A, mask_tail=A), dict(row_set=A, mask_head=A),
                dict(mask_tail=A, mask_head=A), dict(mask_tail=A, mask_head=A, n_sets=8), dict(n_sets=8), dict(n_sets=-1),
                dict(accumulator=None), dict(workspace=A + 16), dict(workspace=A + 128)):
        assert tick(**bad) == EINVAL, bad
    assert tick(accumulator=None, pocket_accumulator=None, workspace_bytes="NEED-1") == ENOMEM     # both absent: taken
    assert tick(V=(1 << 23) + 1) == ENOTSUP
    assert tick(V=1 << 23, workspace_bytes="NEED-1") == ENOMEM             # 2V = 2^24 is taken as far as the size check
    # what the rank entry points refuse, with their codes
    for bad in (dict(table=None), dict(N=0), dict(N=-1), dict(d=0), dict(d=-8), dict(max_norm=0.0), dict(max_norm=-1.0),
                dict(hr=None), dict(true_id=None), dict(cand=None), dict(model=-1), dict(model=4), dict(model=7),
                dict(known_off_tail=None), dict(known_rc_tail=None), dict(known_off_head=None), dict(known_rc_head=None),
                dict(planes=A + 16), dict(planes=A, d=32), dict(d=63), dict(d=7), dict(table=A + 8), dict(table=A + 4)):
        assert tick(**bad) == EINVAL, bad
    for bad in (dict(model=1), dict(model=3), dict(d=12, planes=None), dict(d=36, planes=None), dict(d=296, planes=None),
                dict(d=1024, planes=None), dict(d=240, max_norm=9.0, planes=None)):
        assert tick(**bad) == ENOTSUP, bad
    assert tick(known_off_tail=None, known_rc_tail=None, known_off_head=None, known_rc_head=None,
                workspace_bytes="NEED-1") == ENOMEM                        # unfiltered is taken
    assert tick(known_off_head=None, known_rc_head=None, workspace_bytes="NEED-1") == ENOMEM
    # the masked form: sets are checked ahead of the model, and ask for the split-precision range
    assert tick(**SETS, workspace_bytes="NEED-1") == ENOMEM
    for bad in (dict(n_sets=0), dict(n_sets=-3), dict(row_set=A + 2), dict(mask_tail=A + 1), dict(mask_head=A + 2)):
        assert tick(**dict(SETS, **bad)) == EINVAL, bad
    for d in (8, 32, 48, 296):
        assert tick(**SETS, d=d, planes=None) == ENOTSUP, d
    assert tick(**SETS, max_norm=9.0) == ENOTSUP
    assert tick(**dict(SETS, n_sets=0), model=1) == EINVAL
    assert tick(**SETS, model=1) == ENOTSUP
    assert tick(**SETS, table=A + 8) == EINVAL
    # the planes: NULL iff the split-precision sweep does not run
    assert tick(planes=None) == EINVAL
    for d in (8, 32, 40, 48):
        assert tick(d=d, planes=None, workspace_bytes="NEED-1") == ENOMEM, d          # the fp32 route, as far as the size check
    # a pocket copy_if cannot write
    assert tick(pocket=A + 4) == EINVAL
    assert tick(pocket_accumulator=A + 8) == EINVAL
    assert tick(pocket=None, pocket_accumulator=None, workspace_bytes="NEED-1") == ENOMEM
    # the workspace's size comes last
    for V in (1, 127, 128, 129, 300):
        assert tick(V=V, workspace_bytes="NEED-1") == ENOMEM
    assert tick(workspace_bytes=0) == ENOMEM
    # the order: the tick's own GE_EINVALs, then 2V > 2^24, then the rank entry points' checks, then GE_ENOMEM
    assert tick(metrics_out=None, V=(1 << 23) + 1, model=1, workspace_bytes=0) == EINVAL
    assert tick(mask_tail=A, V=(1 << 23) + 1) == EINVAL
    assert tick(accumulator=None, model=1) == EINVAL
    assert tick(workspace=A + 16, V=(1 << 23) + 1) == EINVAL
    assert tick(V=(1 << 23) + 1, table=None, workspace_bytes=0) == ENOTSUP
    assert tick(model=1, workspace_bytes=0) == ENOTSUP
    assert tick(table=None, workspace_bytes=0) == EINVAL
    assert tick(d=12, planes=None, workspace_bytes=0) == ENOTSUP
    assert tick(planes=None, workspace_bytes=0) == EINVAL
    assert tick(pocket=A + 4, workspace_bytes=0) == EINVAL


# ------------------------------------------------------------------------------------------------ the driver's flags
def parse(*argv):
    return T.build_parser().parse_args(["--data_dir", "D", "--output_dir", "O", *argv])


SOFT = ["--objective", "softmax", "--optimizer", "adagrad"]


def test_default_is_unchanged():
    a = parse()
    assert (a.softmax_validation_ticks, a.softmax_validation_rows, a.softmax_patience) == (0, 0, 0)
    assert vars(a) == vars(parse("--softmax_validation_ticks", "0"))
    assert vars(a) == vars(parse("--softmax_validation_rows", "0", "--softmax_patience", "0"))
    T.check_objective_flags(a)
    T.check_objective_flags(parse(*SOFT))
    T.check_objective_flags(parse(*SOFT, "--softmax_validation_ticks", "0"))


def test_validation_tick_flags():
    ok = parse(*SOFT, "--softmax_validation_ticks", "4", "--softmax_validation_rows", "1000", "--softmax_patience", "3")
    assert (ok.softmax_validation_ticks, ok.softmax_validation_rows, ok.softmax_patience) == (4, 1000, 3)
    T.check_objective_flags(ok)
    for extra in (["--softmax_samples", "32"], ["--softmax_labels", "all"], ["--softmax_candidate_sets", "types", "--embedding_dim", "64"],
                  ["--softmax_candidate_sets", "observed", "--embedding_dim", "288"], ["--embedding_dim", "32"], ["--embedding_dim", "296"]):
        T.check_objective_flags(parse(*SOFT, "--softmax_validation_ticks", "2", *extra))
    flags = ("softmax_validation_ticks", "softmax_validation_rows", "softmax_patience")

    def refused(argv, word):
        with pytest.raises(SystemExit) as e:
            T.check_objective_flags(parse(*argv))
        assert isinstance(e.value.code, str) and word in e.value.code, (argv, e.value.code)
    for f in flags:
        # without --objective softmax, and negative
        refused(["--" + f, "2"], f)
        refused(["--objective", "hinge", "--optimizer", "adagrad", "--" + f, "2"], f)
        refused([*SOFT, "--softmax_validation_ticks", "2", "--" + f, "-1"], f)
        refused(["--" + f, "-1"], f)
    # patience and rows need ticks
    refused([*SOFT, "--softmax_patience", "2"], "softmax_patience")
    refused([*SOFT, "--softmax_validation_rows", "100"], "softmax_validation_rows")
    refused([*SOFT, "--softmax_validation_ticks", "0", "--softmax_patience", "2"], "softmax_validation_ticks")
    # candidate sets rank on the masked sweep
    for d in ("8", "32", "48", "60", "296"):
        for kind in ("types", "observed"):
            refused([*SOFT, "--softmax_validation_ticks", "2", "--softmax_candidate_sets", kind, "--embedding_dim", d],
                    "softmax_validation_ticks")
        T.check_objective_flags(parse(*SOFT, "--softmax_candidate_sets", "types", "--embedding_dim", d))      # no ticks: as before
    # refused with what the objective is refused with
    for extra, word in ((["--optimizer", "sgd"], "adagrad"), (["--optimizer", "adagrad", "--model", "hole"], "hole"),
                        (["--optimizer", "adagrad", "--gpus", "2"], "gpus"), (["--optimizer", "adagrad", "--log_loss"], "log_loss")):
        refused(["--objective", "softmax", "--softmax_validation_ticks", "2", *extra], word)
    with pytest.raises(SystemExit):
        parse("--softmax_validation_ticks", "some")
