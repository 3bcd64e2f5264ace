"""Host: the fp64 restatement of the TransX AdaGrad step (tests/transx_adagrad_ref.py) against torch.optim.Adagrad on
torch-CPU autograd of the same hinge; the prototypes of ge_transx_adagrad_step / ge_transx_train_steps_adagrad; what both
answer to bad arguments; the driver's flags.

As in test_adagrad_refusals_host.py no refusal case reaches a kernel: each carries an argument the entry point refuses, or
n_steps = 0, which returns before any launch, and every pointer is a fake address that is never dereferenced.  The refusal
cases are skipped where a GPU is visible, so that a case that slipped through validation could never launch on a fake
pointer."""
import numpy as np
import pytest
import torch

from graphembeddings_amd import _lib
from tests import transx_adagrad_ref as AR
from tests import transx_ref as TR

MODELS = ("transe", "transh", "transd")


# ------------------------------------------------------------------------------------ the restatement
def _torch_loss(model, P, pos, neg, margin, l1):
    """sum max(D(pos) - D(neg) + margin, 0) on torch fp64 parameters P, written from transE.py / transH.py / transD.py."""
    def proj(e_id, r_id):
        e = P["ent"][e_id]
        if model == "transe":
            return e
        if model == "transh":
            n = P["normal_vector"][r_id]
            nh = n / torch.sqrt(torch.clamp((n * n).sum(1, keepdim=True), min=TR.EPS))
            return e - (e * nh).sum(1, keepdim=True) * nh
        return e + (e * P["ent_transfer"][e_id]).sum(1, keepdim=True) * P["rel_transfer"][r_id]

    def dist(tri):
        h, t, r = (torch.as_tensor(tri[:, c], dtype=torch.long) for c in range(3))
        u = proj(h, r) + P["rel"][r] - proj(t, r)
        return u.abs().sum(1) if l1 else (u * u).sum(1)
    return torch.clamp(dist(pos) - dist(neg) + margin, min=0).sum()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("l1", [True, False])
def test_restatement_equals_torch_adagrad(model, l1):
    """Three dependent steps, random data (no ties: no pair at z = 0, no residual at 0, n.n far from the clamp)."""
    E, R, d, B, lr, a0, margin = 40, 5, 6, 64, 0.05, 0.1, 0.2
    rng = np.random.default_rng(3 + MODELS.index(model) + 10 * l1)
    rows = {"ent": E, "rel": R, "normal_vector": R, "ent_transfer": E, "rel_transfer": R}
    tabs = {k: rng.normal(size=(rows[k], d)) * 0.2 for k in ("ent", "rel") + TR.EXTRA[model]}
    accs = {k: np.full_like(v, a0) for k, v in tabs.items()}
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in tabs.items()}
    opt = torch.optim.Adagrad(list(P.values()), lr=lr, initial_accumulator_value=a0, eps=0)
    seen_inactive = False
    for step in range(3):
        pos = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, R, B)], 1)
        neg = pos.copy()
        neg[np.arange(B), rng.integers(0, 2, B)] = rng.integers(0, E, B)
        seen_inactive |= not TR.active_mask(model, tabs, pos, neg, margin, l1).all()
        opt.zero_grad()
        loss = _torch_loss(model, P, pos, neg, margin, l1)
        loss.backward()
        tabs, accs, rloss, g = AR.adagrad_step(model, tabs, accs, pos, neg, lr, margin, l1)
        for k in tabs:
            assert np.abs(P[k].grad.numpy() - g[k]).max() <= 1e-12, (step, k)
        opt.step()
        assert abs(float(loss.detach()) - rloss) <= 1e-12 * max(1.0, abs(rloss))
        for k, p in P.items():
            assert np.abs(p.detach().numpy() - tabs[k]).max() <= 1e-12, (step, k)
            assert np.abs(opt.state[p]["sum"].numpy() - accs[k]).max() <= 1e-12, (step, k)
    assert seen_inactive                                   # some pairs sat out: the named-rows rule was exercised


def test_rows_no_active_pair_names_keep_both_arrays():
    tabs = TR.exact_tables("transd", 12, 3, 4, seed=1)
    accs = {k: np.full_like(v, 0.1) for k, v in tabs.items()}
    pos = np.array([[0, 1, 0], [2, 3, 1]])
    neg = np.array([[0, 4, 0], [2, 3, 1]])                  # pair 1: neg == pos, z = margin < 0: inactive
    new_t, new_a, _, _ = AR.adagrad_step("transd", tabs, accs, pos, neg, 0.05, -0.5, True)
    act = TR.active_mask("transd", tabs, pos, neg, -0.5, True)
    assert not act[1]
    named = AR.named_rows(tabs, pos, neg, act)
    assert not named["ent"][[2, 3]].any() and not named["rel"][1]
    for k in tabs:
        assert np.array_equal(new_t[k][~named[k]], tabs[k][~named[k]]) and np.array_equal(new_a[k][~named[k]], accs[k][~named[k]])


# ------------------------------------------------------------------------------------ prototypes and refusals
host_only = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: host-only refusals")
EINVAL, ENOTSUP, ENOMEM = _lib.GE_EINVAL, _lib.GE_ENOTSUP, _lib.GE_ENOMEM
A = 1 << 12                                   # a fake, 256-byte aligned, never-dereferenced address
M = 1 << 20                                   # the fake buffers lie 1 MiB apart: 100 x 8 floats never reach the next
E_, R_, D_ = 100, 10, 8
ENT_BYTES, REL_BYTES = E_ * D_ * 4, R_ * D_ * 4

TABLES = ["model", "l1", "ent", "n_ent", "rel", "n_rel", "normal", "ent_transfer", "rel_transfer", "acc_ent", "acc_rel",
          "acc_normal", "acc_ent_transfer", "acc_rel_transfer", "d"]
WS = ["workspace", "workspace_bytes", "stream"]
ARGS = {
    "ge_transx_adagrad_step": TABLES + ["pos", "neg", "B", "margin", "lr", "loss"] + WS,
    "ge_transx_train_steps_adagrad": TABLES + ["triples", "T", "bh_key", "bh_ent", "bt_key", "bt_ent", "n_known",
                                               "tail_threshold", "seed", "first_step", "n_steps", "B", "margin", "lr",
                                               "losses"] + WS,
}
GOOD = dict(model=2, l1=1, ent=A, n_ent=E_, rel=A + M, n_rel=R_, normal=A + 2 * M, ent_transfer=A + 3 * M,
            rel_transfer=A + 4 * M, acc_ent=A + 5 * M, acc_rel=A + 6 * M, acc_normal=A + 7 * M, acc_ent_transfer=A + 8 * M,
            acc_rel_transfer=A + 9 * M, d=D_, pos=A + 10 * M, neg=A + 11 * M, B=4, margin=1.0, lr=0.05, loss=A + 12 * M,
            losses=A + 12 * M, triples=A + 13 * M, T=50, bh_key=A + 14 * M, bh_ent=A + 14 * M, bt_key=A + 14 * M,
            bt_ent=A + 14 * M, n_known=50, tail_threshold=A + 15 * M, seed=7, first_step=0, n_steps=0, workspace=A + 16 * M,
            workspace_bytes="NEED", stream=None)
STEP, LOOP = "ge_transx_adagrad_step", "ge_transx_train_steps_adagrad"


def call(name, **kw):
    lib = _lib.load()
    a = dict(GOOD, **kw)
    if a["workspace_bytes"] in ("NEED", "NEED-1"):
        need = int(lib.ge_transx_step_workspace_bytes(a["n_ent"], a["n_rel"], a["d"], a["B"]))
        assert need > 0 or a["workspace_bytes"] == "NEED"
        a["workspace_bytes"] = need - (a["workspace_bytes"] == "NEED-1")
    return getattr(lib, name)(*[a[n] for n in ARGS[name]])


def test_prototypes_and_version():
    lib = _lib.load()
    assert lib.ge_version() >= 430
    for name, args in ARGS.items():
        assert len(args) == len(_lib.SYMBOLS[name][1]), name
    # "exactly the arguments of ge_transx_train_steps from `d` on", and of ge_transx_hinge_step for the single step
    for ada, sgd in ((LOOP, "ge_transx_train_steps"), (STEP, "ge_transx_hinge_step")):
        assert _lib.SYMBOLS[ada][1][14:] == _lib.SYMBOLS[sgd][1][9:] and _lib.SYMBOLS[ada][1][:9] == _lib.SYMBOLS[sgd][1][:9]


# what both entry points refuse about the tables and the accumulators, in the header's order.  A later stage's fault is
# put beside each (a missing workspace byte, GE_ENOMEM; an unsupported width, GE_ENOTSUP) wherever the codes differ, so
# that the expected code shows which check came first.
ACC_OF = {"ent": "acc_ent", "rel": "acc_rel", "normal": "acc_normal", "ent_transfer": "acc_ent_transfer",
          "rel_transfer": "acc_rel_transfer"}
MODEL_TABLES = {0: ("ent", "rel"), 1: ("ent", "rel", "normal"), 2: ("ent", "rel", "ent_transfer", "rel_transfer")}


def table_and_accumulator_cases():
    cases = []
    add = lambda code, **kw: cases.append((kw, code))
    # 1. what transx_model refuses comes first: in front of a missing accumulator and of a short workspace
    add(EINVAL, model=3, acc_ent=None)
    add(EINVAL, model=-1, workspace_bytes=0)
    add(EINVAL, ent=None, workspace_bytes=0)
    add(EINVAL, n_ent=0, workspace_bytes=0)
    add(EINVAL, d=0, acc_ent=None)
    add(ENOTSUP, d=2048, acc_ent=None)                      # GE_ENOTSUP, not the missing accumulator's GE_EINVAL
    add(ENOTSUP, d=2048, acc_rel=A + 6 * M + 2)             # ... nor the misaligned one's
    add(ENOTSUP, d=2048, acc_ent=A)                         # ... nor the overlapping one's
    add(EINVAL, model=1, normal=None, workspace_bytes=0)
    add(EINVAL, model=2, rel_transfer=None, workspace_bytes=0)
    add(EINVAL, ent=A + 2, workspace_bytes=0)
    # 2. a missing accumulator of a table the model has, in front of GE_ENOMEM
    for model, names in MODEL_TABLES.items():
        for t in names:
            add(EINVAL, model=model, workspace_bytes=0, **{ACC_OF[t]: None})
    # 3. an accumulator that is not 4-byte aligned
    for model, names in MODEL_TABLES.items():
        for t in names:
            add(EINVAL, model=model, workspace_bytes=0, **{ACC_OF[t]: GOOD[ACC_OF[t]] + 2})
    add(EINVAL, acc_ent=None, acc_rel=A + 6 * M + 1)
    # 4. overlaps: the accumulator equals a table; it ends one float inside a table; two accumulators are equal
    add(EINVAL, acc_ent=A, workspace_bytes=0)
    add(EINVAL, acc_rel=A + M, workspace_bytes=0)
    add(EINVAL, acc_rel=A, workspace_bytes=0)                                  # ... of another table
    add(EINVAL, acc_ent=A + M - ENT_BYTES + 4, workspace_bytes=0)              # its last float is rel's first
    add(EINVAL, acc_rel=A - REL_BYTES + 4, workspace_bytes=0)                  # its last float is ent's first
    add(EINVAL, acc_rel_transfer=A + ENT_BYTES - 4, workspace_bytes=0)         # its first float is ent's last
    add(EINVAL, acc_ent_transfer=A + 5 * M, workspace_bytes=0)                 # == acc_ent
    add(EINVAL, acc_rel_transfer=A + 6 * M, workspace_bytes=0)                 # == acc_rel
    add(EINVAL, acc_rel=A + 5 * M + ENT_BYTES - 4, workspace_bytes=0)          # its first float is acc_ent's last
    add(EINVAL, model=1, acc_normal=A + 2 * M, workspace_bytes=0)
    # touching is not overlapping: the later stage's code shows the accumulators passed
    add(ENOMEM, acc_ent=A + ENT_BYTES, workspace_bytes="NEED-1")
    add(ENOMEM, acc_rel=A - REL_BYTES, workspace_bytes="NEED-1")
    add(ENOMEM, acc_rel=A + 5 * M + ENT_BYTES, workspace_bytes="NEED-1")
    # an accumulator of a table the model does not have is ignored, as its table is: missing, misaligned, overlapping
    add(ENOMEM, model=0, acc_normal=None, acc_ent_transfer=A + 1, acc_rel_transfer=A, workspace_bytes="NEED-1")
    add(ENOMEM, model=1, acc_ent_transfer=A + 5 * M, acc_rel_transfer=None, workspace_bytes="NEED-1")
    add(ENOMEM, model=2, acc_normal=A + 3, workspace_bytes="NEED-1")
    add(ENOMEM, model=0, normal=A + 5 * M, ent_transfer=A + 6 * M, workspace_bytes="NEED-1")   # nor is an unused table
    return cases


@host_only
@pytest.mark.parametrize("name", [STEP, LOOP])
def test_tables_and_accumulators_are_checked_in_order(name):
    for kw, code in table_and_accumulator_cases():
        assert call(name, **kw) == code, (kw, code)
        if name == LOOP:                                   # ... in front of the step count
            assert call(name, **dict(kw, n_steps=3)) == code, (kw, code)


@host_only
def test_adagrad_step_refuses_what_the_hinge_step_refuses():
    for bad in (dict(B=0), dict(B=-1), dict(B=(1 << 31) // 5), dict(pos=None), dict(neg=None), dict(loss=None),
                dict(workspace=None), dict(pos=A + 10 * M + 2), dict(neg=A + 11 * M + 1), dict(loss=A + 12 * M + 2),
                dict(workspace=A + 16 * M + 16), dict(workspace=A + 16 * M + 128)):
        assert call(STEP, **dict(bad, workspace_bytes=0)) == EINVAL, bad      # in front of GE_ENOMEM
    assert call(STEP, workspace_bytes="NEED-1") == ENOMEM and call(STEP, workspace_bytes=0) == ENOMEM
    for model in (0, 1, 2):
        for d in (7, 8):
            assert call(STEP, model=model, d=d, workspace_bytes="NEED-1") == ENOMEM


@host_only
def test_train_steps_adagrad_refuses_what_the_sgd_loop_refuses():
    assert call(LOOP) == 0                                  # n_steps = 0: 0 after the checks
    for model in (0, 1, 2):
        assert call(LOOP, model=model, l1=0, d=7) == 0
    assert call(LOOP, n_known=0, bh_key=None, bh_ent=None, bt_key=None, bt_ent=None) == 0
    assert call(LOOP, model=0, normal=None, ent_transfer=None, rel_transfer=None, acc_normal=None, acc_ent_transfer=None,
                acc_rel_transfer=None) == 0
    for bad in (dict(B=0), dict(B=-1), dict(n_steps=-1), dict(losses=None), dict(workspace=None), dict(workspace=A + 16 * M + 16),
                # the sampler checks
                dict(triples=None), dict(T=0), dict(T=(1 << 32) + 1), dict(tail_threshold=None), dict(n_known=-1),
                dict(bh_key=None), dict(bh_ent=None), dict(bt_key=None), dict(bt_ent=None)):
        for n in (0, 3):
            assert call(LOOP, **dict(bad, n_steps=bad.get("n_steps", n), workspace_bytes=0)) == EINVAL, bad
    for n in (0, 3):                                        # one byte short is refused, whatever the step count
        assert call(LOOP, n_steps=n, workspace_bytes="NEED-1") == ENOMEM
        assert call(LOOP, n_steps=n, workspace_bytes=0) == ENOMEM


# ------------------------------------------------------------------------------------ the driver's flags
def test_driver_flags():
    from graphembeddings_amd import transr_train, transx_train as D
    a = D.build_parser().parse_args([])
    assert a.optimizer == "sgd" and a.adagrad_init == 0.1
    D.check_args(a)
    a = D.build_parser().parse_args(["--optimizer", "adagrad", "--adagrad_init", "0.5", "--learning_rate", "0.05"])
    assert a.optimizer == "adagrad" and a.adagrad_init == 0.5
    D.check_args(a)
    for bad in ("0", "-0.1", "nan"):
        with pytest.raises(ValueError, match="adagrad_init"):
            D.check_args(D.build_parser().parse_args(["--optimizer", "adagrad", "--adagrad_init", bad]))
    with pytest.raises(ValueError, match="adagrad_init"):   # checked whatever the optimizer, like every flag
        D.check_args(D.build_parser().parse_args(["--adagrad_init", "0"]))
    with pytest.raises(SystemExit):
        D.build_parser().parse_args(["--optimizer", "adam"])
    for flag in ("--optimizer", "--adagrad_init"):          # transx_train only: TransR trains with Adam
        with pytest.raises(SystemExit):
            transr_train.build_parser().parse_args([flag, "adagrad" if flag == "--optimizer" else "0.1"])


def test_python_argument_checks_need_no_gpu():
    """enable_adagrad and trainer() refuse before any device work; built on the class alone (no tables, no GPU)."""
    from graphembeddings_amd import transr, transx
    m = transx.TransX.__new__(transx.TransX)
    m.tables = {}
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="initial_accumulator_value"):
            m.enable_adagrad(bad)
        with pytest.raises(ValueError, match="initial_accumulator_value"):
            m.trainer(np.zeros((1, 3)), 1, optimizer="adagrad", initial_accumulator_value=bad)
    assert m.accumulators is None
    with pytest.raises(ValueError, match="optimizer"):
        m.trainer(np.zeros((1, 3)), 1, optimizer="adam")
    r = transr.TransR.__new__(transr.TransR)
    with pytest.raises(ValueError, match="Adam"):
        r.trainer(np.zeros((1, 3)), 1, optimizer="adagrad")
    with pytest.raises(RuntimeError, match="enable_adagrad"):
        m._adagrad_ptrs()
