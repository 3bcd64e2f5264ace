"""Host: what the ComplEx / HolE training entry points (the sampler, the single steps, the validation ticks, the
native loops and their prepare launch) answer to bad arguments, and which code wins when two arguments are bad at once.

Nothing here reaches a kernel: every case carries an argument the entry point refuses, or a batch / step count of 0,
which returns before any launch, and every pointer is a fake address that is never dereferenced.  The module is
skipped where a GPU is visible, so that a case that slipped through validation could never launch on a fake pointer.

The range check on (mode, padded_size, n_types) is NOT the same everywhere, and that is part of the record:
ge_train_steps, ge_train_steps_logloss and ge_train_prepare_steps apply it themselves, in front of GE_ENOTSUP and (the
prepare launch) GE_ENOMEM; ge_corrupt_batch leaves it to its launcher, behind its own pointer checks; the two validation
ticks do not look at the three values before their workspace, so a tick with mode 4 and a short workspace answers
GE_ENOMEM where ge_train_prepare_steps answers GE_EINVAL.

The expected codes were recorded from the library before the type sampler and the step sequence became descriptors
behind the C ABI and passed there unchanged."""
import pytest
import torch

from graphembeddings_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: host-only refusals")

EINVAL, ENOTSUP, ENOMEM = _lib.GE_EINVAL, _lib.GE_ENOTSUP, _lib.GE_ENOMEM
A = 1 << 12                                   # a fake, 256-byte aligned, never-dereferenced address
P24 = 1 << 24
# (d, table alignment) no ComplEx-shaped kernel takes; the odd entries are beyond HolE's direct kernels (d > 512) as well
REFUSED_SHAPES = (dict(d=258), dict(d=1022), dict(d=512, table=A + 4), dict(d=520, table=A + 8))

TABLE = ["table", "N", "d"]
TYPES = ["id_to_type", "type_offsets", "n_types", "type_ids"]
WS = ["workspace", "workspace_bytes"]
SEQ = ["triples", "T", "first_row", "B", "n_steps"]
LR = ["lr0", "decay_steps", "decay_rate", "max_norm"]
TICK = TABLE + ["valid", "V", "B"] + TYPES + ["seed", "step", "padded_size", "mode"]
TICK_OUT = WS + ["mean_out", "best", "pocket", "stream"]

# entry point: its arguments in ABI order
ENTRIES = {
    "ge_corrupt_batch": ["pos", "B", "id_to_type", "N", "type_offsets", "n_types", "type_ids", "seed", "step", "padded_size",
                         "mode", "neg", "stream"],
    "ge_hinge_loss": TABLE + ["pos", "neg", "B", "margin", "max_norm", "model", "loss", "sig_out", "stream"],
    "ge_hinge_grad": TABLE + ["pos", "neg", "B", "margin", "lr", "max_norm", "model", "loss", "grad_idx", "grad_val", "stream"],
    "ge_complex_hinge_step": TABLE + ["pos", "neg", "B", "margin", "lr", "max_norm", "loss"] + WS + ["stream"],
    "ge_hole_hinge_step": TABLE + ["pos", "neg", "B", "margin", "lr", "max_norm", "loss"] + WS + ["stream"],
    "ge_complex_logloss": TABLE + ["triples", "B", "label", "l2", "max_norm", "loss"] + WS + ["stream"],
    "ge_complex_logloss_step": TABLE + ["triples", "labels", "B", "lr", "l2", "max_norm", "loss"] + WS + ["stream"],
    "ge_validation_tick": TICK + ["margin", "max_norm", "model"] + TICK_OUT,
    "ge_validation_tick_logloss": TICK + ["K", "l2", "max_norm"] + TICK_OUT,
    "ge_train_steps": TABLE + SEQ + TYPES + ["seed", "step", "padded_size", "mode", "margin"] + LR +
                      ["model", "loss", "keep", "neg_ws"] + WS + ["ev_pairs", "ev_kernel", "pipeline", "stream"],
    "ge_train_steps_logloss": TABLE + SEQ + TYPES + ["seed", "step", "padded_size", "mode", "K", "l2"] + LR +
                              ["loss", "keep", "neg_ws"] + WS + ["pipeline", "stream"],
    "ge_train_prepare_steps": SEQ + ["id_to_type", "N", "type_offsets", "n_types", "type_ids", "seed", "step", "padded_size",
                                     "mode", "direct", "out", "workspace_bytes", "stream"],
}

# a call every entry point would accept (never made as it stands)
GOOD = dict(table=A, N=100, d=8, pos=A, neg=A, B=4, triples=A, T=100, first_row=0, n_steps=1, valid=A, V=50,
            id_to_type=A, type_offsets=A, n_types=2, type_ids=A, seed=7, step=0, padded_size=16, mode=0, margin=0.2,
            lr=0.1, lr0=0.1, decay_steps=0.0, decay_rate=0.5, max_norm=1.0, model=0, loss=A, sig_out=None, grad_idx=A,
            grad_val=A, label=1.0, labels=A, l2=0.1, K=1, keep=0, neg_ws=A, workspace=A, ev_pairs=None, ev_kernel=0,
            pipeline=None, mean_out=A, best=A, pocket=None, direct=0, out=A, stream=None)

# the size function a workspace_bytes of "NEED" / "NEED-1" stands for
SIZE_FN = {
    "ge_complex_hinge_step": ("ge_hinge_step_workspace_bytes", ["B", "d"]),
    "ge_hole_hinge_step": ("ge_hinge_step_workspace_bytes", ["B", "d"]),
    "ge_complex_logloss": (None, 256),
    "ge_complex_logloss_step": ("ge_logloss_step_workspace_bytes", ["B", "d"]),
    "ge_validation_tick": ("ge_validation_workspace_bytes", ["B"]),
    "ge_validation_tick_logloss": ("ge_validation_logloss_workspace_bytes", ["B", "K"]),
    "ge_train_steps": ("ge_hinge_step_workspace_bytes", ["B", "d"]),       # below it no step can run; from it, the fallback
    "ge_train_steps_logloss": ("ge_train_logloss_workspace_bytes", ["B", "K", "d"]),
    "ge_train_prepare_steps": ("ge_train_prepare_bytes", ["B", "n_steps"]),
}

LOOPS = ("ge_train_steps", "ge_train_steps_logloss", "ge_train_prepare_steps")
TICKS = ("ge_validation_tick", "ge_validation_tick_logloss")
SHORT = dict(workspace_bytes="NEED-1")


def _table_cases(add, zero):
    """`zero`: overrides that make the call return 0 before any launch (B = 0, or no steps), added to accepted values."""
    add(EINVAL, table=None)
    add(EINVAL, N=0)
    add(EINVAL, d=0)
    add(EINVAL, max_norm=0.0)
    add(EINVAL, max_norm=-1.0)
    add(0, **zero)


def _sampler_cases(add, name):
    """The type tables: every null pointer, both sides of the three ranges."""
    for p in ("id_to_type", "type_offsets", "type_ids"):
        add(EINVAL, **{p: None})
    if name in LOOPS:
        zero = dict(n_steps=0)
        for bad in (dict(mode=-1), dict(mode=4), dict(padded_size=-1), dict(n_types=-1)):
            add(EINVAL, **bad)
            add(EINVAL, **bad, **zero)                        # the range comes before the step count
        for ok in (dict(mode=0), dict(mode=3), dict(padded_size=0), dict(n_types=0)):
            add(0, **ok, **zero)
    elif name == "ge_corrupt_batch":
        zero = dict(B=0)
        for bad in (dict(mode=-1), dict(mode=4), dict(padded_size=-1), dict(n_types=-1)):
            add(EINVAL, **bad, **zero)                        # (the launcher's check, in front of its B == 0)
            add(EINVAL, **bad, pos=None)
        for ok in (dict(mode=0), dict(mode=3), dict(padded_size=0), dict(n_types=0)):
            add(0, **ok, **zero)
    else:
        # the ticks look at the workspace first: what the loops refuse as GE_EINVAL is GE_ENOMEM here
        for any_ in (dict(mode=-1), dict(mode=4), dict(padded_size=-1), dict(n_types=-1), dict(mode=0), dict(mode=3),
                     dict(padded_size=0), dict(n_types=0)):
            add(ENOMEM, **any_, **SHORT)
            add(EINVAL, **any_, workspace=A + 128)


def _workspace_cases(add, first_fault):
    add(EINVAL, workspace=None)
    add(EINVAL, workspace=A + 128)
    add(ENOMEM, **SHORT)
    add(EINVAL, workspace=None, **SHORT)                      # two at once: the pointer before the size
    add(EINVAL, workspace=A + 128, workspace_bytes=0)
    add(EINVAL, **first_fault, **SHORT)                       # GE_EINVAL before GE_ENOMEM


def _cases(name):
    """(overrides of GOOD, expected code) of one entry point; every case is refused or returns 0 before any launch."""
    out = []
    add = lambda code, **kw: out.append((kw, code))
    if name == "ge_corrupt_batch":
        add(EINVAL, B=-1)
        add(EINVAL, N=0)
        add(EINVAL, pos=None)
        add(EINVAL, neg=None)
        add(0, B=0)
        add(0, B=0, pos=None, neg=None)                       # the batch matters only when B > 0
        add(EINVAL, B=0, id_to_type=None)
        _sampler_cases(add, name)
        return out
    if name in ("ge_hinge_loss", "ge_hinge_grad"):
        _table_cases(add, dict(B=0))
        add(EINVAL, B=-1)
        add(EINVAL, model=-1)
        add(EINVAL, model=3)
        add(0, B=0, model=2)
        add(0, B=0, model=1, d=7)                             # HolE on the real table takes an odd width
        add(EINVAL, B=0, d=7)                                 # ... the ComplEx pairs do not
        add(EINVAL, B=0, model=2, d=7)
        ptrs = ("pos", "neg", "loss") + (("grad_idx", "grad_val") if name == "ge_hinge_grad" else ())
        for p in ptrs:
            add(EINVAL, **{p: None})
        add(0, B=0, **{p: None for p in ptrs})
        add(EINVAL, model=3, pos=None)
        add(EINVAL, B=0, table=None)
        add(ENOTSUP, B=0, d=1 << 20)                          # wider than any kernel
        add(EINVAL, B=0, d=1 << 20, model=3)                  # two at once: GE_EINVAL before GE_ENOTSUP
        add(EINVAL, d=1 << 20, pos=None)
        return out
    if name in ("ge_complex_hinge_step", "ge_hole_hinge_step"):
        _table_cases(add, dict(B=0))
        add(EINVAL, B=-1)
        for p in ("pos", "neg", "loss"):
            add(EINVAL, **{p: None})
        add(0, B=0, pos=None, neg=None, loss=None, workspace=None, workspace_bytes=0)
        _workspace_cases(add, dict(pos=None))
        add(EINVAL, B=-1, workspace_bytes=0)
        add(ENOMEM, d=1 << 20, workspace_bytes=0)             # the size before the width the kernels refuse
        return out
    if name in ("ge_complex_logloss", "ge_complex_logloss_step"):
        _table_cases(add, dict(B=0))
        add(EINVAL, B=-1)
        for p in ("triples", "loss") + (("labels",) if name.endswith("_step") else ()):
            add(EINVAL, **{p: None})
        add(0, B=0, triples=None, loss=None, workspace=None, workspace_bytes=0)
        _workspace_cases(add, dict(triples=None))
        add(EINVAL, max_norm=0.0, **SHORT)
        add(ENOMEM, d=7, **SHORT)                             # the size before the odd width
        return out
    if name in TICKS:
        add(EINVAL, table=None)
        add(EINVAL, N=0)
        add(EINVAL, d=0)
        add(EINVAL, max_norm=0.0)
        add(EINVAL, B=0)                                      # a tick of no rows is refused
        add(EINVAL, B=-1)
        add(EINVAL, V=0)
        for p in ("valid", "mean_out", "best"):
            add(EINVAL, **{p: None})
        add(ENOMEM, pocket=A, **SHORT)
        if name == "ge_validation_tick":
            add(EINVAL, model=-1)
            add(EINVAL, model=3)
            add(ENOMEM, model=2, **SHORT)
            add(EINVAL, model=3, **SHORT)
        else:
            add(EINVAL, K=0)
            add(ENOMEM, K=1, **SHORT)
            add(ENOMEM, K=1024, **SHORT)
            add(ENOMEM, K=1025, **SHORT)                      # the ticks put no upper limit on the ratio
            add(EINVAL, K=0, workspace_bytes=0)
            add(ENOMEM, d=7, **SHORT)
        _sampler_cases(add, name)
        _workspace_cases(add, dict(valid=None))
        return out
    assert name in LOOPS
    zero = dict(n_steps=0)
    if name != "ge_train_prepare_steps":
        _table_cases(add, zero)
        add(EINVAL, loss=None)
        add(EINVAL, neg_ws=None)
    else:
        add(EINVAL, N=0)
        add(EINVAL, out=None)
        add(0, **zero)
        add(0, workspace_bytes=0, **zero)
    add(EINVAL, B=0)
    add(EINVAL, B=-1)
    add(EINVAL, n_steps=-1)
    add(EINVAL, first_row=-1)
    add(EINVAL, triples=None)
    add(EINVAL, T=3)                                          # T < B
    add(0, T=4, **zero)                                       # T == B
    add(EINVAL, T=3, **zero)
    _sampler_cases(add, name)
    if name == "ge_train_steps":
        _workspace_cases(add, dict(triples=None))
        add(0, first_row=10 ** 12, **zero)
        for m in (-1, 4, 0x100 | 4):
            add(EINVAL, model=m)
        for m in (0, 1, 2, 3, 0x100, 0x100 | 3):
            add(0, model=m, **zero)
        add(EINVAL, model=2, d=7)                             # a spectral table has an even width
        add(EINVAL, model=0x100 | 2, d=7, **zero)
        add(0, model=1, d=7, **zero)
        add(EINVAL, ev_pairs=A, ev_kernel=3)
        add(EINVAL, ev_pairs=A, ev_kernel=-1)
        add(0, ev_pairs=None, ev_kernel=3, **zero)            # the selector matters only with events
        add(0, ev_pairs=A, ev_kernel=2, **zero)
        add(ENOMEM, mode=4, **SHORT)                          # two at once: the size before the sampler's ranges
        add(ENOMEM, ev_pairs=A, ev_kernel=3, **SHORT)
        add(EINVAL, model=4, **SHORT)
        add(EINVAL, ev_pairs=A, ev_kernel=3, mode=4)
        add(0, d=1 << 20, **zero)                             # no step, no kernel: the width is not looked at
        # widths the shape switch of ge_complex.hip does not take (tests/complex_shape_cases.py REFUSED): decided before
        # the first launch -- and, model 1, before the forward transform -- whatever the mode
        for bad in REFUSED_SHAPES:
            for m in (0, 2, 0x100, 0x100 | 2):
                add(ENOTSUP, model=m, **bad)
            add(0, **bad, **zero)
            add(ENOMEM, **bad, **SHORT)                       # the size before the width
        for bad in REFUSED_SHAPES[1::2]:                      # wider than the direct-correlation kernels too: HolE
            add(ENOTSUP, model=1, **bad)
            add(ENOTSUP, model=0x100 | 1, **bad)
            add(ENOTSUP, model=3, **bad)
        add(EINVAL, d=7, model=0)                             # the ComplEx pairs take no odd width
    elif name == "ge_train_steps_logloss":
        for bad in REFUSED_SHAPES:
            add(ENOTSUP, **bad)
            add(0, **bad, **zero)
            add(ENOMEM, **bad, **SHORT)
        add(EINVAL, workspace=None)
        add(EINVAL, workspace=A + 128)
        add(ENOMEM, **SHORT)
        add(0, workspace_bytes=0, **zero)                     # the size is the loop's own check, behind its step count
        add(EINVAL, workspace=None, **SHORT)
        add(EINVAL, triples=None, **SHORT)                    # GE_EINVAL before GE_ENOMEM
        add(EINVAL, d=7)
        add(EINVAL, d=7, **zero)
        add(EINVAL, K=0)
        add(EINVAL, K=1025)
        add(0, K=1, **zero)
        add(0, K=1024, **zero)
        add(ENOMEM, K=1024, **SHORT)
        big = dict(B=P24 // 2, T=P24 // 2, K=1)               # (1 + K) B = 2^24: the largest step
        add(0, **big, **zero)
        add(ENOMEM, **big, workspace_bytes=0)
        nxt = dict(B=65281, T=65281, K=256)                   # 257 x 65,281 = 2^24 + 1: the first step refused
        assert (1 + nxt["K"]) * nxt["B"] == P24 + 1
        add(ENOTSUP, **nxt)
        add(ENOTSUP, **nxt, **zero)
        add(ENOTSUP, **nxt, workspace_bytes=0)
        add(EINVAL, **nxt, mode=4)
        over = dict(B=P24 // 2 + 1, T=P24, K=1)               # 2^24 + 2
        add(ENOTSUP, **over)
        add(ENOTSUP, B=P24 // 4 + 1, T=P24, K=3)              # 2^24 + 4
        add(ENOTSUP, B=(P24 + 1) // 1025 + 1, T=P24, K=1024)
        add(ENOTSUP, **over, **zero)                          # ... before the step count
        add(ENOTSUP, **over, workspace_bytes=0)               # ... and before GE_ENOMEM
        add(EINVAL, **over, mode=4)                           # two at once: GE_EINVAL before GE_ENOTSUP
        add(EINVAL, **over, workspace=A + 128)
        add(EINVAL, **dict(over, K=1025))
    else:
        add(ENOMEM, **SHORT)
        add(EINVAL, mode=4, **SHORT)                          # two at once: GE_EINVAL before GE_ENOMEM
        add(EINVAL, triples=None, **SHORT)
        add(EINVAL, out=None, workspace_bytes=0)
        add(ENOMEM, B=4097, T=5000, n_steps=2, **SHORT)       # a step of two tiles: the sort's scratch is part of the size
        add(0, direct=1, **zero)
    return out


def _call(lib, name, overrides):
    a = dict(GOOD, **overrides)
    if name in SIZE_FN and a.get("workspace_bytes", "NEED") in ("NEED", "NEED-1"):
        fn, names = SIZE_FN[name]
        need = names if fn is None else int(getattr(lib, fn)(*[a[n] for n in names]))
        if a.get("workspace_bytes") == "NEED-1":
            assert need > 0, (name, overrides)
            need -= 1
        a["workspace_bytes"] = need
    return getattr(lib, name)(*[a[n] for n in ENTRIES[name]])


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_entry_refuses_bad_arguments_without_launching(name):
    lib = _lib.load()
    assert len(ENTRIES[name]) == len(_lib.SYMBOLS[name][1])
    cases = _cases(name)
    assert len(cases) >= 15 and any(len(kw) >= 2 and code != 0 for kw, code in cases)
    got = [(kw, _call(lib, name, kw)) for kw, _ in cases]
    wrong = [(kw, code, g) for (kw, code), (_, g) in zip(cases, got) if g != code]
    assert not wrong, f"{name}: (overrides, expected, got) = {wrong}"
