"""Host: what the ge_transx_adv_* entry points (the self-adversarial loss of TransE / TransH / TransD) answer to bad
arguments, and in which order; their size function; the driver's flags and the Python class's refusals.

As in test_rotate_adv_refusals_host.py no refusal case reaches a kernel: each carries an argument the entry point refuses,
or B = 0 / n_steps = 0, which returns before any launch, and every pointer is a fake address that is never dereferenced.
The refusal cases are skipped where a GPU is visible, so that a case that slipped through validation could never launch on
a fake pointer."""
import numpy as np
import pytest
import torch

import test_abi_workspace_host as W
from graphembeddings_amd import _lib

KS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024]
# joins the table test_abi_workspace_host.py checks; it holds rocprim's sort scratch, as ge_transx_step_workspace_bytes
W.CASES["ge_transx_adv_step_workspace_bytes"] = (
    [(0, 1, 2), W.E, W.R, [1, 3, 4, 16, 17], W.SIZES, KS],
    [(-1, 10, 9, 16, 5, 4), (3, 10, 9, 16, 5, 4), (0, 0, 9, 16, 5, 4), (1, 10, 0, 16, 5, 4), (2, 10, 9, 0, 5, 4),
     (0, 10, 9, 1025, 5, 4), (0, 10, 9, 16, 0, 4), (1, 10, 9, 16, -1, 4), (2, 10, 9, 16, 5, 0), (0, 10, 9, 16, 5, -1),
     (0, 10, 9, 16, 5, 1025), (0, 10, 9, 16, (1 << 31) // 7 + 1, 4)], True)
W.NEEDS_DEVICE = tuple(W.NEEDS_DEVICE) + ("ge_transx_adv_step_workspace_bytes",)

host_only = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: host-only refusals")
EINVAL, ENOTSUP, ENOMEM = _lib.GE_EINVAL, _lib.GE_ENOTSUP, _lib.GE_ENOMEM
A = 1 << 12                                   # a fake, 256-byte aligned, never-dereferenced address
M = 1 << 20                                   # the fake buffers lie 1 MiB apart
E_, R_, D_ = 100, 10, 8
NAN, INF = float("nan"), float("inf")

TABLES = ["model", "l1", "ent", "n_ent", "rel", "n_rel", "normal", "ent_transfer", "rel_transfer", "d"]
ACCS = ["acc_ent", "acc_rel", "acc_normal", "acc_ent_transfer", "acc_rel_transfer"]
ADA = TABLES[:-1] + ACCS + ["d"]
WS = ["workspace", "workspace_bytes", "stream"]
ROWS = ["pos", "side", "neg_ent", "B", "K", "margin", "alpha"]
SAMPLER = ["triples", "T", "bh_key", "bh_ent", "bt_key", "bt_ent", "n_known", "tail_threshold"]
LOOP_TAIL = SAMPLER + ["seed", "first_step", "n_steps", "B", "K", "margin", "alpha", "lr", "losses"] + WS
ARGS = {
    "ge_transx_adv_loss": TABLES + ROWS + ["out", "stream"],
    "ge_transx_adv_step": TABLES + ROWS + ["lr", "loss"] + WS,
    "ge_transx_adv_adagrad_step": ADA + ROWS + ["lr", "loss"] + WS,
    "ge_transx_adv_train_steps": TABLES + LOOP_TAIL,
    "ge_transx_adv_train_steps_adagrad": ADA + LOOP_TAIL,
}
GOOD = dict(model=2, l1=1, ent=A, n_ent=E_, rel=A + M, n_rel=R_, normal=A + 2 * M, ent_transfer=A + 3 * M,
            rel_transfer=A + 4 * M, acc_ent=A + 5 * M, acc_rel=A + 6 * M, acc_normal=A + 7 * M, acc_ent_transfer=A + 8 * M,
            acc_rel_transfer=A + 9 * M, d=D_, pos=A + 10 * M, side=A + 11 * M, neg_ent=A + 21 * M, B=4, K=3, margin=3.0,
            alpha=1.0, lr=0.05, loss=A + 12 * M, losses=A + 12 * M, triples=A + 13 * M, T=50, bh_key=A + 14 * M,
            bh_ent=A + 14 * M, bt_key=A + 14 * M, bt_ent=A + 14 * M, n_known=50, tail_threshold=A + 15 * M, seed=7,
            first_step=0, n_steps=0, workspace=A + 16 * M, workspace_bytes="NEED", stream=None, out=A + 17 * M)
LOSS, STEP, ADASTEP, LOOP, ADALOOP = ARGS
STEPS, LOOPS, ADAS = (STEP, ADASTEP), (LOOP, ADALOOP), (ADASTEP, ADALOOP)


def call(name, **kw):
    lib = _lib.load()
    a = dict(GOOD, **kw)
    if name == LOSS and "B" not in kw:
        a["B"] = 0                                         # it launches at B > 0: the good call is the empty one
    if a["workspace_bytes"] in ("NEED", "NEED-1"):
        ok = 1 <= a["K"] <= 1024
        model = a["model"] if a["model"] in (0, 1, 2) else 0
        need = int(lib.ge_transx_adv_step_workspace_bytes(model, a["n_ent"], a["n_rel"], a["d"], max(a["B"], 1), a["K"] if ok else 1))
        assert need > 0 or a["workspace_bytes"] == "NEED"
        a["workspace_bytes"] = need - (a["workspace_bytes"] == "NEED-1")
    return getattr(lib, name)(*[a[n] for n in ARGS[name]])


def test_prototypes_and_version():
    lib = _lib.load()
    assert lib.ge_version() >= 448 and lib.ge_transx_adv_max_negatives() == 1024 == lib.ge_rotate_adv_max_negatives()
    for name, args in ARGS.items():
        assert len(args) == len(_lib.SYMBOLS[name][1]), name
    X = _lib.SYMBOLS
    # the hinge counterparts with (side, neg_ent) for neg, K after B and alpha after margin
    assert X[STEP][1][:10] == X["ge_transx_hinge_step"][1][:10] and X[ADASTEP][1][:15] == X["ge_transx_adagrad_step"][1][:15]
    assert X[LOOP][1][:22] == X["ge_transx_train_steps"][1][:22] and X[LOOP][1][-6:] == X["ge_transx_train_steps"][1][-6:]
    assert X[ADALOOP][1][:27] == X["ge_transx_train_steps_adagrad"][1][:27]
    # ... and ge_rotate_adv_*'s arguments after the tables
    for mine, theirs, k in ((LOSS, "ge_rotate_adv_loss", 6), (STEP, "ge_rotate_adv_step", 6), (LOOP, "ge_rotate_adv_train_steps", 6),
                            (ADASTEP, "ge_rotate_adv_adagrad_step", 8), (ADALOOP, "ge_rotate_adv_train_steps_adagrad", 8)):
        assert X[mine][1][len(ARGS[mine]) - (len(X[theirs][1]) - k):] == X[theirs][1][k:], mine
    assert X["ge_transx_adv_step_workspace_bytes"][1][0] is X[STEP][1][0]            # it takes the model first
    assert "ge_transx_adv_draw_batch" not in X                                       # the draw is ge_rotate_adv_draw_batch


def test_size_function():
    W.test_size_function("ge_transx_adv_step_workspace_bytes")
    fn = _lib.load().ge_transx_adv_step_workspace_bytes
    for model in (-1, 3, 4):
        assert int(fn(model, 10, 9, 16, 5, 4)) == 0
    for d in (-2, 0, 1025, 1026):
        assert int(fn(0, 10, 9, d, 5, 4)) == 0
    for K in (-1, 0, 1025, 4096):
        assert int(fn(1, 10, 9, 16, 5, K)) == 0
    assert int(fn(0, 10, 9, 1, 1, 1)) > 0 and int(fn(2, 10, 9, 1024, 2, 64)) > 0 and int(fn(0, 10, 9, 7, 3, 5)) > 0
    if torch.cuda.is_available():                           # (rocprim sizes a sort of more than a few hundred keys on a device only)
        assert int(fn(2, 10, 9, 1024, 2, 1024)) > 0
    # (K + 3) B fits the sort's 31-bit positions
    assert int(fn(0, 10, 9, 16, ((1 << 31) - 1) // 1027 + 1, 1024)) == 0
    # TransE does not pay for a second gradient plane: TransH and TransD are larger by one plane of (K + 3) B rows
    B, K, d = 64, 3, 16
    e, h, t = (int(fn(m, 10, 9, d, B, K)) for m in (0, 1, 2))
    plane = (K + 3) * B * d * 4
    assert h == t == e + plane and plane % 256 == 0
    # TransE's is RotatE's of the same shape: the same parts
    assert e == int(_lib.load().ge_rotate_adv_step_workspace_bytes(10, 9, d, B, K))


def table_cases(name):
    """What ge_transx_hinge_step refuses about the model and its tables, in its order; a later stage's fault beside each."""
    cases = []
    add = lambda code, **kw: cases.append((kw, code))
    late = dict(workspace_bytes=0) if name != LOSS else {}
    for extra in (late, dict(K=0), dict(alpha=-1.0)):       # ... in front of GE_ENOMEM and of this loss's own refusals
        add(EINVAL, model=-1, **extra)
        add(EINVAL, model=3, **extra)
        add(EINVAL, ent=None, **extra)
        add(EINVAL, rel=None, **extra)
        add(EINVAL, n_ent=0, **extra)
        add(EINVAL, n_rel=0, **extra)
        add(EINVAL, n_ent=(1 << 31) - R_, **extra)
        add(EINVAL, d=0, **extra)
        add(ENOTSUP, d=1025, **extra)
        add(EINVAL, model=1, normal=None, **extra)
        add(EINVAL, model=2, ent_transfer=None, **extra)
        add(EINVAL, model=2, rel_transfer=None, **extra)
        add(EINVAL, ent=A + 2, **extra)
        add(EINVAL, rel=A + M + 1, **extra)
        add(EINVAL, model=1, normal=A + 2 * M + 2, **extra)
        add(EINVAL, ent_transfer=A + 3 * M + 1, **extra)
    add(EINVAL, model=3, d=1025)                            # the model code before GE_ENOTSUP
    add(EINVAL, n_ent=-5, d=1025)                           # sizes before GE_ENOTSUP
    add(ENOTSUP, d=1025, ent=A + 2)                         # GE_ENOTSUP before the misaligned table's GE_EINVAL
    add(ENOTSUP, d=1025, model=1, normal=None)              # ... and before the missing table's
    add(ENOTSUP, d=1025, K=0)                               # the shape before K
    add(EINVAL, ent=None, K=2000)                           # the tables before K's GE_ENOTSUP
    return cases


@host_only
@pytest.mark.parametrize("name", [LOSS, STEP, ADASTEP, LOOP, ADALOOP])
def test_model_and_tables_come_first(name):
    if name not in STEPS:
        for model in (0, 1, 2):
            assert call(name, model=model) == 0             # the good call: B = 0 or n_steps = 0
        assert call(name, model=0, normal=None, ent_transfer=None, rel_transfer=None, acc_normal=None,
                    acc_ent_transfer=None, acc_rel_transfer=None) == 0      # tables a model does not have are not looked at
        assert call(name, model=0, normal=A + 2 * M + 1) == EINVAL          # ... but a given one is 4-byte aligned
    for kw, code in table_cases(name):
        assert call(name, **kw) == code, (kw, code)
        if name in LOOPS:
            assert call(name, **dict(kw, n_steps=3)) == code, (kw, code)
        if name == LOSS:
            assert call(name, **dict(kw, B=5)) == code, (kw, code)


@host_only
@pytest.mark.parametrize("name", ADAS)
def test_accumulators_come_before_this_losss_refusals(name):
    bads = (dict(acc_ent=None), dict(acc_rel=None), dict(acc_ent_transfer=None), dict(acc_rel_transfer=None),
            dict(model=1, acc_normal=None), dict(acc_ent=A + 5 * M + 2), dict(acc_ent=A), dict(acc_rel=A + 5 * M),
            dict(acc_rel_transfer=A + 3 * M))
    for bad in bads:
        for extra in (dict(workspace_bytes=0), dict(K=2000), dict(K=0, alpha=NAN)):
            assert call(name, **dict(bad, **extra)) == EINVAL, (bad, extra)
    assert call(name, d=1025, acc_ent=None) == ENOTSUP       # the shape in front of the accumulators
    assert call(name, acc_ent=A + 5 * M, K=2000) == ENOTSUP  # good accumulators: K is reached
    assert call(name, model=0, acc_normal=None, acc_ent_transfer=A, K=2000) == ENOTSUP   # those of absent tables are dropped


def own_cases(rows):
    """This loss's refusals in their order; beside each, the fault of the NEXT stage (and of the stages after it), so
    that the code shows which check came first.  rows: the call takes side and neg_ent."""
    cases = []
    add = lambda code, **kw: cases.append((kw, code))
    big = ((1 << 31) - 1) // 6 + 1                          # (K + 3) B = 2^31 - 1 + ... at K = 3
    add(EINVAL, K=0, workspace_bytes=0)
    add(EINVAL, K=-4, workspace_bytes=0)
    add(ENOTSUP, K=1025, workspace_bytes=0)
    add(ENOTSUP, K=1025, B=big)                             # K's range before the slot count
    add(ENOTSUP, K=1025, alpha=-1.0)
    add(ENOTSUP, K=1 << 30, margin=NAN)
    add(EINVAL, B=big, workspace_bytes=0)
    add(EINVAL, B=(1 << 31) // 4, K=1, workspace_bytes=0)
    add(EINVAL, B=1 << 40, K=1024, workspace_bytes=0)
    if rows:
        add(EINVAL, side=None, workspace_bytes=0)
        add(EINVAL, neg_ent=None, workspace_bytes=0)
        add(ENOTSUP, K=1025, side=None)                     # K before the null side
    for bad in (dict(margin=NAN), dict(margin=INF), dict(margin=-INF), dict(alpha=NAN), dict(alpha=INF), dict(alpha=-1.0),
                dict(alpha=-1e-30)):
        add(EINVAL, workspace_bytes=0, **bad)
        add(ENOTSUP, K=1025, **bad)                         # K before the hyperparameters
    return cases


@host_only
@pytest.mark.parametrize("model", [0, 1, 2])
@pytest.mark.parametrize("name", [STEP, ADASTEP, LOOP, ADALOOP])
def test_own_refusals_sit_between_the_tables_and_the_workspace(name, model):
    for kw, code in own_cases(name in STEPS):
        for n in ((0, 3) if name in LOOPS else (0,)):
            assert call(name, **dict(kw, n_steps=n, model=model)) == code, (kw, code)
    # what passes: alpha = 0, a negative margin, K = 1 and K = 64; GE_ENOMEM shows it
    for ok in (dict(alpha=0.0), dict(margin=-2.0), dict(K=1), dict(K=64), dict(alpha=1e30)):
        assert call(name, **dict(ok, workspace_bytes="NEED-1", model=model)) == ENOMEM, ok
    # (a host without a device cannot size rocprim's sort of this many keys: the code is then the runtime's, which still
    # shows that no argument check refused)
    for ok in (dict(K=1024), dict(B=((1 << 31) - 1) // 6)):
        assert call(name, **dict(ok, workspace_bytes=0, model=model)) not in (0, EINVAL, ENOTSUP), ok
    # ... and the shared checks come after them, in front of GE_ENOMEM
    shared = [dict(B=0), dict(B=-1), dict(workspace=None), dict(workspace=A + 16 * M + 16)]
    shared += [dict(pos=None), dict(loss=None), dict(pos=A + 10 * M + 2), dict(side=A + 11 * M + 1), dict(neg_ent=A + 21 * M + 2),
               dict(loss=A + 12 * M + 2)] if name in STEPS else \
              [dict(n_steps=-1), dict(losses=None), dict(triples=None), dict(T=0), dict(tail_threshold=None), dict(n_known=-1),
               dict(bh_key=None)]
    for bad in shared:
        assert call(name, **dict(bad, workspace_bytes=0, model=model)) == EINVAL, bad
        if "B" not in bad:
            assert call(name, **dict(bad, K=1025, model=model)) == ENOTSUP, bad          # K in front of them
    assert call(name, workspace_bytes=0, model=model) == ENOMEM
    if name in LOOPS:
        assert call(name, model=model) == 0 and call(name, model=model, l1=0, d=7, K=64, alpha=0.0) == 0
        assert call(name, model=model, n_known=0, bh_key=None, bh_ent=None, bt_key=None, bt_ent=None) == 0
        assert call(name, model=model, n_steps=3, workspace_bytes="NEED-1") == ENOMEM
    # TransE's workspace is too small for the models with a second plane
    if model != 0:
        small = int(_lib.load().ge_transx_adv_step_workspace_bytes(0, E_, R_, D_, 4, 3))
        assert call(name, model=model, workspace_bytes=small) == ENOMEM


@host_only
def test_loss_refuses_bad_batches_and_outputs():
    assert call(LOSS, pos=None, side=None, neg_ent=None, out=None) == 0          # B = 0: the buffers matter only when B > 0
    for kw, code in own_cases(False):
        kw = {k: v for k, v in kw.items() if k != "workspace_bytes"}
        assert call(LOSS, **dict(dict(B=5), **kw)) == code, kw
    for bad in (dict(B=-1), dict(B=5, pos=None), dict(B=5, out=None), dict(B=5, side=None), dict(B=5, neg_ent=None),
                dict(B=5, pos=A + 10 * M + 2), dict(B=5, side=A + 11 * M + 2), dict(B=5, neg_ent=A + 21 * M + 1),
                dict(B=5, out=A + 17 * M + 1)):
        assert call(LOSS, **bad) == EINVAL, bad
    assert call(LOSS, B=5, side=None, K=1025) == ENOTSUP


@host_only
def test_the_hinge_family_still_refuses_other_model_codes():
    lib = _lib.load()
    for model in (-1, 3, 4):
        assert lib.ge_transx_score(model, 1, A, E_, A + M, R_, A + 2 * M, A + 3 * M, A + 4 * M, D_, None, 0, None, None) == EINVAL
        assert int(lib.ge_transx_rank_workspace_bytes(model, E_, R_, D_, 4)) == 0


# ------------------------------------------------------------------------------------ the driver and the class
def test_driver_flags():
    from graphembeddings_amd import transx_train as D
    a = D.build_parser().parse_args([])
    D.check_args(a)
    assert a.loss == "hinge" and a.negatives is None and a.adversarial_temperature is None
    a = D.build_parser().parse_args(["--loss", "self_adversarial"])
    D.check_args(a)
    assert a.negatives == 64 and a.adversarial_temperature == 1.0
    a = D.build_parser().parse_args(["--model", "transd", "--loss", "self_adversarial", "--negatives", "1024",
                                     "--adversarial_temperature", "0", "--margin", "6", "--optimizer", "adagrad"])
    D.check_args(a)
    assert a.negatives == 1024 and a.adversarial_temperature == 0.0 and a.margin == 6.0
    adv = ["--loss", "self_adversarial"]
    for bad in (["--negatives", "8"], ["--adversarial_temperature", "1"], ["--loss", "hinge", "--negatives", "8"],
                adv + ["--negatives", "0"], adv + ["--negatives", "1025"], adv + ["--negatives", "-3"],
                adv + ["--adversarial_temperature", "-0.5"], adv + ["--adversarial_temperature", "nan"],
                adv + ["--adversarial_temperature", "inf"], adv + ["--margin", "nan"], adv + ["--hidden_size", "1025"]):
        with pytest.raises(ValueError):
            D.check_args(D.build_parser().parse_args(bad))
    for flag in (["--loss", "logistic"], ["--negatives", "x"]):
        with pytest.raises(SystemExit):
            D.build_parser().parse_args(flag)
    # the three flags are transx_train's own: rotate_train keeps defining its own, transr_train still rejects them
    import argparse
    from graphembeddings_amd import rotate_train, transr_train
    p = argparse.ArgumentParser()
    D.add_common_flags(p, ("hidden_size",), "x")
    assert not {"loss", "negatives", "adversarial_temperature"} & set(vars(p.parse_args([])))
    assert rotate_train.build_parser().parse_args(adv + ["--negatives", "5"]).negatives == 5
    for flag in (adv, ["--negatives", "4"], ["--adversarial_temperature", "1"]):
        with pytest.raises(SystemExit):
            transr_train.build_parser().parse_args(flag)
    # a Namespace built without the flags (the checks' other callers) is the hinge
    ns = D.build_parser().parse_args([])
    for k in ("loss", "negatives", "adversarial_temperature"):
        delattr(ns, k)
    D.check_args(ns)


def test_python_argument_checks_need_no_gpu():
    """Shapes, dtypes, K and the hyperparameters raise ValueError before any device work; built on the class alone (no
    tables, no GPU)."""
    from graphembeddings_amd import rotate, transr, transx
    # the shared pieces are one object under both names
    assert rotate.AdvTrainer is transx.AdvTrainer and rotate.check_adv_hyperparameters is transx.check_adv_hyperparameters
    assert rotate.MAX_NEGATIVES == transx.MAX_NEGATIVES == 1024 and rotate.LOSSES == ("hinge", "self_adversarial")
    assert rotate.RotatE._adv_batch is transx.TransX._adv_batch
    for model in ("transe", "transh", "transd"):
        m = transx.TransX.__new__(transx.TransX)
        m.tables = {}
        m.model, m.n_ent, m.n_rel, m.d, m.l1 = model, 5, 2, 8, True
        t = np.zeros((1, 3))
        adv = dict(loss="self_adversarial")
        for bad in (dict(loss="logistic"), dict(negatives=4), dict(adversarial_temperature=1.0), dict(loss="hinge", negatives=4),
                    dict(adv, negatives=0), dict(adv, negatives=1025), dict(adv, negatives=2.5), dict(adv, negatives=True),
                    dict(adv, adversarial_temperature=-1.0), dict(adv, adversarial_temperature=float("nan")),
                    dict(adv, adversarial_temperature=float("inf")), dict(adv, margin=float("nan")), dict(adv, optimizer="adam"),
                    dict(adv, optimizer="adagrad", initial_accumulator_value=0)):
            with pytest.raises(ValueError):
                m.trainer(t, 1, **bad)
        assert m.accumulators is None
        pos, side, neg = torch.zeros(4, 3, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), torch.zeros(4, 6, dtype=torch.int32)
        bad_batches = (dict(pos=pos[:, :2]), dict(pos=pos[:0], side=side[:0], neg_ent=neg[:0]), dict(pos=pos.float()),
                       dict(side=side[:3]), dict(side=side[:, None]), dict(side=side.double()), dict(neg_ent=neg[:3]),
                       dict(neg_ent=neg[0]), dict(neg_ent=neg[:, :0]), dict(neg_ent=torch.zeros(4, 1025, dtype=torch.int32)),
                       dict(neg_ent=neg.float()), dict(alpha=-1.0), dict(alpha=float("nan")), dict(margin=float("inf")),
                       dict(pos=pos.numpy()))
        for bad in bad_batches:
            a = dict(dict(pos=pos, side=side, neg_ent=neg, margin=3.0, alpha=1.0), **bad)
            for f in (m.adv_loss, lambda *x: m.adv_step(*x, 0.1), lambda *x: m.adv_adagrad_step(*x, 0.1)):
                with pytest.raises((ValueError, RuntimeError)) as e:
                    f(a["pos"], a["side"], a["neg_ent"], a["margin"], a["alpha"])
                if f == m.adv_loss:
                    assert e.type is ValueError, bad
        with pytest.raises(RuntimeError, match="enable_adagrad"):
            m.adv_adagrad_step(pos, side, neg, 3.0, 1.0, 0.1)
        with pytest.raises(RuntimeError, match="CUDA"):         # good host tensors: refused as host tensors, after the checks
            m.adv_loss(pos, side, neg, 3.0, 1.0)
    # TransR has no such loss: ValueError, whatever else is passed; its hinge keywords are as they were
    r = transr.TransR.__new__(transr.TransR)
    r.tables = {}
    r.n_ent, r.n_rel = 5, 2
    for kw in (dict(loss="self_adversarial"), dict(loss="self_adversarial", negatives=4), dict(loss="logistic"),
               dict(negatives=4), dict(optimizer="adagrad")):
        with pytest.raises(ValueError):
            r.trainer(np.zeros((1, 3)), 1, **kw)
    assert not hasattr(r, "adv_loss") and not hasattr(r, "adv_step")
