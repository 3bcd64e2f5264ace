"""Host: what the ge_rotate_* entry points answer to bad arguments, and in which order; their size functions; the
driver's flags and the Python class's refusals.

As in test_transx_adagrad_host.py no refusal case reaches a kernel: each carries an argument the entry point refuses, or
B = 0 / n_steps = 0, which returns before any launch, and every pointer is a fake address that is never dereferenced.  The
refusal cases are skipped where a GPU is visible, so that a case that slipped through validation could never launch on a
fake pointer."""
import numpy as np
import pytest
import torch

import test_abi_workspace_host as W
from graphembeddings_amd import _lib

# The two size functions join the table test_abi_workspace_host.py checks (its test_every_size_function_is_listed reads
# CASES when it runs, after every module is collected).  The step's holds rocprim's sort scratch, as ge_transx_step_*'s.
W.CASES["ge_rotate_step_workspace_bytes"] = ([W.E, W.R, (16,), W.SIZES], [(0, 9, 16, 5), (10, 0, 16, 5), (10, 9, 0, 5),
                                                                        (10, 9, 15, 5), (10, 9, 1026, 5), (10, 9, 16, 0)], True)
W.CASES["ge_rotate_rank_workspace_bytes"] = ([W.E, W.R, (16,), W.SIZES], [(0, 9, 16, 5), (10, 0, 16, 5), (10, 9, 0, 5),
                                                                        (10, 9, 7, 5), (10, 9, 1026, 5), (10, 9, 16, 0)], True)
W.NEEDS_DEVICE = tuple(W.NEEDS_DEVICE) + ("ge_rotate_step_workspace_bytes",)

host_only = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: host-only refusals")
EINVAL, ENOTSUP, ENOMEM = _lib.GE_EINVAL, _lib.GE_ENOTSUP, _lib.GE_ENOMEM
A = 1 << 12                                   # a fake, 256-byte aligned, never-dereferenced address
M = 1 << 20                                   # the fake buffers lie 1 MiB apart
E_, R_, D_ = 100, 10, 8
ENT_BYTES, REL_BYTES = E_ * D_ * 4, R_ * (D_ // 2) * 4      # rel and acc_rel are [n_rel, d / 2]

TABLES = ["l1", "ent", "n_ent", "rel", "n_rel", "d"]
ADA = ["l1", "ent", "n_ent", "rel", "n_rel", "acc_ent", "acc_rel", "d"]
WS = ["workspace", "workspace_bytes", "stream"]
STEP_TAIL = ["pos", "neg", "B", "margin", "lr", "loss"] + WS
LOOP_TAIL = ["triples", "T", "bh_key", "bh_ent", "bt_key", "bt_ent", "n_known", "tail_threshold", "seed", "first_step",
             "n_steps", "B", "margin", "lr", "losses"] + WS
ARGS = {
    "ge_rotate_score": TABLES + ["triples", "B", "out", "stream"],
    "ge_rotate_hinge_step": TABLES + STEP_TAIL,
    "ge_rotate_adagrad_step": ADA + STEP_TAIL,
    "ge_rotate_train_steps": TABLES + LOOP_TAIL,
    "ge_rotate_train_steps_adagrad": ADA + LOOP_TAIL,
    "ge_rotate_rank": TABLES + ["triples", "B", "cand_is_head", "known_off", "known_rc", "n_before", "n_known_before",
                                "true_dist", "scores_out"] + WS,
}
GOOD = dict(l1=1, ent=A, n_ent=E_, rel=A + M, n_rel=R_, acc_ent=A + 5 * M, acc_rel=A + 6 * M, d=D_, pos=A + 10 * M,
            neg=A + 11 * M, B=4, margin=1.0, lr=0.05, loss=A + 12 * M, losses=A + 12 * M, triples=A + 13 * M, T=50,
            bh_key=A + 14 * M, bh_ent=A + 14 * M, bt_key=A + 14 * M, bt_ent=A + 14 * M, n_known=50,
            tail_threshold=A + 15 * M, seed=7, first_step=0, n_steps=0, workspace=A + 16 * M, workspace_bytes="NEED",
            stream=None, out=A + 17 * M, cand_is_head=0, known_off=None, known_rc=None, n_before=A + 18 * M,
            n_known_before=A + 19 * M, true_dist=A + 20 * M, scores_out=None)
SCORE, STEP, ADASTEP, LOOP, ADALOOP, RANK = ARGS
STEPS, LOOPS, ADAS = (STEP, ADASTEP), (LOOP, ADALOOP), (ADASTEP, ADALOOP)


def call(name, **kw):
    lib = _lib.load()
    a = dict(GOOD, **kw)
    if name in (SCORE, RANK) and "B" not in kw:
        a["B"] = 0                                         # these two launch at B > 0: the good call is the empty one
    if a["workspace_bytes"] in ("NEED", "NEED-1"):
        size = lib.ge_rotate_rank_workspace_bytes if name == RANK else lib.ge_rotate_step_workspace_bytes
        need = int(size(a["n_ent"], a["n_rel"], a["d"], max(a["B"], 1)))
        assert need > 0 or a["workspace_bytes"] == "NEED"
        a["workspace_bytes"] = need - (a["workspace_bytes"] == "NEED-1")
    return getattr(lib, name)(*[a[n] for n in ARGS[name]])


def test_prototypes_and_version():
    lib = _lib.load()
    assert lib.ge_version() >= 446 and lib.ge_rotate_max_dim() == 1024
    for name, args in ARGS.items():
        assert len(args) == len(_lib.SYMBOLS[name][1]), name
    # the arguments of the ge_transx_* counterpart: no `model`, (ent, n_ent, rel, n_rel, d) for its five tables and d,
    # (acc_ent, acc_rel) for its five accumulators; everything after d as it is
    X = _lib.SYMBOLS
    for rot, tx, n_tx in ((SCORE, "ge_transx_score", 10), (STEP, "ge_transx_hinge_step", 10), (LOOP, "ge_transx_train_steps", 10),
                          (RANK, "ge_transx_rank", 10), (ADASTEP, "ge_transx_adagrad_step", 15),
                          (ADALOOP, "ge_transx_train_steps_adagrad", 15)):
        n_rot = len(ADA if rot in ADAS else TABLES)
        assert X[rot][1][n_rot:] == X[tx][1][n_tx:], rot
    assert X["ge_rotate_step_workspace_bytes"] == X["ge_transx_step_workspace_bytes"]


def test_size_functions():
    W.test_size_function("ge_rotate_step_workspace_bytes")
    W.test_size_function("ge_rotate_rank_workspace_bytes")
    lib = _lib.load()
    # the rank workspace: q [B, d] and the targets [B], each padded to 256 bytes
    assert int(lib.ge_rotate_rank_workspace_bytes(10, 9, 16, 5)) == 512 + 256
    assert int(lib.ge_rotate_rank_workspace_bytes(10, 9, 1024, 1 << 28)) > 0 and int(lib.ge_rotate_rank_workspace_bytes(10, 9, 16, (1 << 28) + 1)) == 0
    # a refused shape has size 0: odd, beyond the maximum
    for d in (-2, 0, 1, 7, 1025, 1026, 2048):
        assert int(lib.ge_rotate_step_workspace_bytes(10, 9, d, 5)) == 0 and int(lib.ge_rotate_rank_workspace_bytes(10, 9, d, 5)) == 0
    assert int(lib.ge_rotate_step_workspace_bytes(10, 9, 2, 5)) > 0 and int(lib.ge_rotate_step_workspace_bytes(10, 9, 1024, 5)) > 0


# what every entry point refuses about the shape and the two tables, in the family's order.  A later stage's fault is put
# beside each wherever the codes differ, so that the expected code shows which check came first.
def table_cases(name):
    cases = []
    add = lambda code, **kw: cases.append((kw, code))
    late = dict(workspace_bytes=0) if name not in (SCORE,) else {}      # a short workspace: GE_ENOMEM, the last check
    add(EINVAL, ent=None, **late)
    add(EINVAL, rel=None, **late)
    add(EINVAL, n_ent=0, **late)
    add(EINVAL, n_rel=0, **late)
    add(EINVAL, n_ent=-5, d=7)                              # sizes before GE_ENOTSUP
    add(EINVAL, n_ent=(1 << 31) - R_, **late)               # n_ent + n_rel fit the sort's 32-bit keys
    add(EINVAL, d=0, **late)
    add(EINVAL, d=-2, **late)
    add(ENOTSUP, d=7, **late)                               # odd
    add(ENOTSUP, d=1, **late)
    add(ENOTSUP, d=1026, **late)                            # beyond ge_rotate_max_dim()
    add(ENOTSUP, d=1025, **late)
    add(ENOTSUP, d=7, ent=A + 2)                            # GE_ENOTSUP before the misaligned table's GE_EINVAL
    add(EINVAL, ent=A + 2, **late)
    add(EINVAL, rel=A + M + 1, **late)
    return cases


def accumulator_cases():
    cases = []
    add = lambda code, **kw: cases.append((kw, code))
    add(ENOTSUP, d=7, acc_ent=None)                         # GE_ENOTSUP, not the missing accumulator's GE_EINVAL
    add(ENOTSUP, d=2048, acc_rel=A + 6 * M + 2)             # ... nor the misaligned one's
    add(ENOTSUP, d=1026, acc_ent=A)                         # ... nor the overlapping one's
    add(EINVAL, acc_ent=None, workspace_bytes=0)            # missing, in front of GE_ENOMEM
    add(EINVAL, acc_rel=None, workspace_bytes=0)
    add(EINVAL, acc_ent=A + 5 * M + 2, workspace_bytes=0)   # misaligned
    add(EINVAL, acc_rel=A + 6 * M + 1, workspace_bytes=0)
    add(EINVAL, acc_ent=A, workspace_bytes=0)               # overlaps: equal to a table
    add(EINVAL, acc_rel=A + M, workspace_bytes=0)
    add(EINVAL, acc_rel=A, workspace_bytes=0)               # ... to the other table
    add(EINVAL, acc_ent=A + M - ENT_BYTES + 4, workspace_bytes=0)              # its last float is rel's first
    add(EINVAL, acc_rel=A - REL_BYTES + 4, workspace_bytes=0)                  # its last float is ent's first
    add(EINVAL, acc_rel=A + ENT_BYTES - 4, workspace_bytes=0)                  # its first float is ent's last
    add(EINVAL, acc_ent=A + M + REL_BYTES - 4, workspace_bytes=0)              # its first float is rel's last
    add(EINVAL, acc_rel=A + 5 * M, workspace_bytes=0)                          # == acc_ent
    add(EINVAL, acc_rel=A + 5 * M + ENT_BYTES - 4, workspace_bytes=0)          # its first float is acc_ent's last
    add(EINVAL, acc_ent=A + 6 * M + REL_BYTES - 4, workspace_bytes=0)          # its first float is acc_rel's last
    # touching is not overlapping, and rel / acc_rel end after n_rel * d / 2 floats, not n_rel * d: the later stage's
    # code shows the accumulators passed
    add(ENOMEM, acc_ent=A + ENT_BYTES, workspace_bytes="NEED-1")
    add(ENOMEM, acc_rel=A - REL_BYTES, workspace_bytes="NEED-1")
    add(ENOMEM, acc_ent=A + M + REL_BYTES, workspace_bytes="NEED-1")
    add(ENOMEM, acc_ent=A + 6 * M + REL_BYTES, workspace_bytes="NEED-1")
    add(ENOMEM, acc_rel=A + 5 * M + ENT_BYTES, workspace_bytes="NEED-1")
    return cases


@host_only
@pytest.mark.parametrize("name", sorted(ARGS))
def test_shape_and_tables_are_checked_in_order(name):
    if name not in STEPS:                                   # (a good single step would launch)
        assert call(name) == 0                              # the good call: B = 0 or n_steps = 0
    for kw, code in table_cases(name):
        assert call(name, **kw) == code, (kw, code)
        if name in LOOPS:                                   # ... in front of the step count
            assert call(name, **dict(kw, n_steps=3)) == code, (kw, code)
        if name in (SCORE, RANK):                           # ... and of the batch
            assert call(name, **dict(kw, B=5)) == code, (kw, code)


@host_only
@pytest.mark.parametrize("name", ADAS)
def test_accumulators_are_checked_in_order(name):
    for kw, code in accumulator_cases():
        assert call(name, **kw) == code, (kw, code)
        if name == ADALOOP:
            assert call(name, **dict(kw, n_steps=3)) == code, (kw, code)


@host_only
@pytest.mark.parametrize("name", STEPS)
def test_steps_refuse_what_the_family_step_refuses(name):
    for bad in (dict(B=0), dict(B=-1), dict(B=(1 << 31) // 5), dict(pos=None), dict(neg=None), dict(loss=None),
                dict(workspace=None), dict(pos=A + 10 * M + 2), dict(neg=A + 11 * M + 1), dict(loss=A + 12 * M + 2),
                dict(workspace=A + 16 * M + 16), dict(workspace=A + 16 * M + 128)):
        assert call(name, **dict(bad, workspace_bytes=0)) == EINVAL, bad      # in front of GE_ENOMEM
    assert call(name, workspace_bytes="NEED-1") == ENOMEM and call(name, workspace_bytes=0) == ENOMEM
    for d in (2, 6, 8, 1024):
        assert call(name, d=d, acc_ent=A + 50 * M, workspace_bytes="NEED-1") == ENOMEM


@host_only
@pytest.mark.parametrize("name", LOOPS)
def test_loops_refuse_what_the_family_loop_refuses(name):
    assert call(name) == 0                                  # n_steps = 0: 0 after the checks
    assert call(name, l1=0, d=6) == 0
    assert call(name, n_known=0, bh_key=None, bh_ent=None, bt_key=None, bt_ent=None) == 0
    for bad in (dict(B=0), dict(B=-1), dict(n_steps=-1), dict(losses=None), dict(workspace=None), dict(workspace=A + 16 * M + 16),
                dict(triples=None), dict(T=0), dict(T=(1 << 32) + 1), dict(tail_threshold=None), dict(n_known=-1),
                dict(bh_key=None), dict(bh_ent=None), dict(bt_key=None), dict(bt_ent=None)):
        for n in (0, 3):
            assert call(name, **dict(bad, n_steps=bad.get("n_steps", n), workspace_bytes=0)) == EINVAL, bad
    for n in (0, 3):                                        # one byte short is refused, whatever the step count
        assert call(name, n_steps=n, workspace_bytes="NEED-1") == ENOMEM
        assert call(name, n_steps=n, workspace_bytes=0) == ENOMEM


@host_only
def test_score_and_rank_refuse_bad_batches_and_outputs():
    assert call(SCORE, triples=None, out=None) == 0         # B = 0: the buffers matter only when B > 0
    for bad in (dict(B=-1), dict(B=5, triples=None), dict(B=5, out=None), dict(B=5, triples=A + 13 * M + 2),
                dict(B=5, out=A + 17 * M + 1)):
        assert call(SCORE, **bad) == EINVAL, bad
    assert call(RANK, triples=None, n_before=None, n_known_before=None, true_dist=None, workspace=None) == 0
    for bad in (dict(B=-1), dict(B=(1 << 28) + 1), dict(known_off=A + 21 * M), dict(known_rc=A + 21 * M),
                dict(B=5, triples=None), dict(B=5, n_before=None), dict(B=5, n_known_before=None), dict(B=5, true_dist=None),
                dict(B=5, workspace=None), dict(B=5, workspace=A + 16 * M + 16), dict(B=5, true_dist=A + 20 * M + 2),
                dict(B=5, scores_out=A + 22 * M + 1)):
        assert call(RANK, **dict(bad, workspace_bytes=0)) == EINVAL, bad      # in front of GE_ENOMEM
    assert call(RANK, B=5, workspace_bytes="NEED-1") == ENOMEM and call(RANK, B=5, workspace_bytes=0) == ENOMEM
    assert call(RANK, B=5, cand_is_head=1, workspace_bytes="NEED-1") == ENOMEM


@host_only
def test_transx_entry_points_still_refuse_other_model_codes():
    lib = _lib.load()
    for model in (3, 4, -1):
        assert lib.ge_transx_score(model, 1, A, E_, A + M, R_, None, None, None, D_, None, 0, None, None) == EINVAL
        assert int(lib.ge_transx_rank_workspace_bytes(model, E_, R_, D_, 5)) == 0


# ------------------------------------------------------------------------------------ the driver and the class
def test_driver_flags():
    from graphembeddings_amd import rotate_train as D
    a = D.build_parser().parse_args([])
    assert a.optimizer == "sgd" and a.adagrad_init == 0.1 and a.l1 and a.hidden_size == 100 and a.predict_k is None
    D.check_args(a)
    a = D.build_parser().parse_args(["--optimizer", "adagrad", "--adagrad_init", "0.5", "--l2", "--hidden_size", "64"])
    assert a.optimizer == "adagrad" and a.adagrad_init == 0.5 and not a.l1
    D.check_args(a)
    for bad in (["--hidden_size", "7"], ["--hidden_size", "0"], ["--hidden_size", "1026"], ["--adagrad_init", "0"],
                ["--nbatches", "0"], ["--learning_rate", "0"], ["--seed", "-1"], ["--filter_file", "x"]):
        with pytest.raises(ValueError):
            D.check_args(D.build_parser().parse_args(bad))
    # the flags of the operations RotatE does not have are not defined
    for flag in (["--predict_k", "3"], ["--candidate_sets", "observed"], ["--relation_ranks"], ["--predict_relations_k", "3"],
                 ["--classify"], ["--neighbors_k", "3"], ["--model", "transe"], ["--optimizer", "adam"]):
        with pytest.raises(SystemExit):
            D.build_parser().parse_args(flag)


def test_python_argument_checks_need_no_gpu():
    """The refusals of the class raise before any device work; built on the class alone (no tables, no GPU)."""
    from graphembeddings_amd import rotate
    for bad in (dict(d=7), dict(d=0), dict(d=1026), dict(n_ent=0), dict(n_rel=0)):
        with pytest.raises(ValueError):
            rotate.RotatE(**dict(dict(n_ent=5, n_rel=2, d=8), **bad))
    m = rotate.RotatE.__new__(rotate.RotatE)
    m.tables = {}
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="initial_accumulator_value"):
            m.enable_adagrad(bad)
        with pytest.raises(ValueError, match="initial_accumulator_value"):
            m.trainer(np.zeros((1, 3)), 1, optimizer="adagrad", initial_accumulator_value=bad)
    assert m.accumulators is None
    with pytest.raises(ValueError, match="optimizer"):
        m.trainer(np.zeros((1, 3)), 1, optimizer="adam")
    with pytest.raises(RuntimeError, match="enable_adagrad"):
        m._adagrad_ptrs()
    t = np.zeros((1, 3))
    for what, f in (("top-k prediction", lambda: m.predict(t[:, :2], 3)), ("top-k prediction", lambda: m.topk_candidates(t, 3)),
                    ("relation prediction", lambda: m.relation_ranks(t)), ("relation prediction", lambda: m.relation_rank_counts(t)),
                    ("relation prediction", lambda: m.predict_relations(t[:, :2], 3)),
                    ("candidate sets", lambda: m.ranks(t, candidate_sets=object())),
                    ("candidate sets", lambda: m.rank_counts(t, row_set=object(), mask=object())),
                    ("top-k prediction", lambda: m._ws_bytes("topk", 1, 3)),
                    ("relation prediction", lambda: m._ws_bytes("relation_rank", 1))):
        with pytest.raises(NotImplementedError, match=what):
            f()
