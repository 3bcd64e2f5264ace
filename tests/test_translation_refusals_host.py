"""Host: what every ge_transx_* / ge_transr_* entry point (and ge_transx_draw_batch) answers to bad arguments, and which
code wins when two arguments are bad at once.  The order inside each entry point is: the model's tables, then the
outputs / batch, then B == 0 (returns 0), then the workspace size (GE_ENOMEM).

Nothing here reaches a kernel: every case carries at least one argument that the entry point refuses (or B == 0, which
returns before any launch), and every pointer is a fake address that is never dereferenced.  The module is skipped where
a GPU is visible, so that a case that slipped through validation could never launch on a fake pointer.

The expected codes were recorded from the library before the translation entry points were folded onto one descriptor
(ge_trans.h) and passed there unchanged."""
import pytest
import torch

from graphembeddings_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: host-only refusals")

EINVAL, ENOTSUP, ENOMEM = _lib.GE_EINVAL, _lib.GE_ENOTSUP, _lib.GE_ENOMEM
A = 1 << 12                                   # a fake, 256-byte aligned, never-dereferenced address
P31, P28 = 1 << 31, 1 << 28

TX = ["model", "l1", "ent", "n_ent", "rel", "n_rel", "normal", "ent_transfer", "rel_transfer", "d"]
TR = ["l1", "ent", "n_ent", "rel", "rel_matrix", "n_rel", "dim_e", "dim_r"]
SAMPLER = ["triples", "T", "bh_key", "bh_ent", "bt_key", "bt_ent", "n_known", "tail_threshold"]
RANK_OUT = ["known_off", "known_rc", "n_before", "n_known_before", "true_dist", "scores_out"]
WS = ["workspace", "workspace_bytes", "stream"]
ADAM = ["b1", "b2", "eps"]

# entry point: its arguments in ABI order
ENTRIES = {
    "ge_transx_score": TX + ["triples", "B", "out", "stream"],
    "ge_transx_hinge_step": TX + ["pos", "neg", "B", "margin", "lr", "loss"] + WS,
    "ge_transx_draw_batch": ["triples", "T", "B", "bh_key", "bh_ent", "bt_key", "bt_ent", "n_known", "tail_threshold",
                             "n_rel32", "n_ent32", "seed", "step", "pos", "neg", "stream"],
    "ge_transx_train_steps": TX + SAMPLER + ["seed", "step", "n_steps", "B", "margin", "lr", "losses"] + WS,
    "ge_transx_rank": TX + ["triples", "B", "cand_is_head"] + RANK_OUT + WS,
    "ge_transx_relation_rank": TX + ["triples", "B"] + RANK_OUT + WS,
    "ge_transx_topk": TX + ["triples", "B", "cand_is_head", "known_off", "known_rc", "k", "out_id", "out_dist"] + WS,
    "ge_transr_score": TR + ["triples", "B", "out", "stream"],
    "ge_transr_adam_step": TR + ["m", "v", "pos", "neg", "B", "margin", "lr"] + ADAM + ["t", "loss"] + WS,
    "ge_transr_train_steps": TR + ["m", "v"] + SAMPLER + ["seed", "step", "n_steps", "B", "margin", "lr"] + ADAM +
                             ["t", "losses"] + WS,
    "ge_transr_rank": TR + ["triples", "B", "cand_is_head"] + RANK_OUT + WS,
    "ge_transr_relation_rank": TR + ["triples", "B"] + RANK_OUT + WS,
    "ge_transr_topk": TR + ["triples", "B", "cand_is_head", "known_off", "known_rc", "k", "out_id", "out_dist"] + WS,
}

# a call every entry point would accept (never made as it stands)
GOOD = dict(model=0, l1=0, ent=A, n_ent=10, rel=A, n_rel=4, normal=A, ent_transfer=A, rel_transfer=A, d=8,
            rel_matrix=A, dim_e=8, dim_r=12, triples=A, B=2, out=A, stream=None, pos=A, neg=A, margin=1.0, lr=0.01,
            loss=A, losses=A, workspace=A, T=100, bh_key=A, bh_ent=A, bt_key=A, bt_ent=A, n_known=3, tail_threshold=A,
            n_rel32=4, n_ent32=10, seed=7, step=0, n_steps=1, cand_is_head=0, known_off=None, known_rc=None, n_before=A,
            n_known_before=A, true_dist=A, scores_out=None, k=5, out_id=A, out_dist=A, m=A, v=A, b1=0.9, b2=0.999,
            eps=1e-8, t=1)

SIZE_FN = {
    "ge_transx_hinge_step": ("ge_transx_step_workspace_bytes", ["n_ent", "n_rel", "d", "B"]),
    "ge_transx_train_steps": ("ge_transx_step_workspace_bytes", ["n_ent", "n_rel", "d", "B"]),
    "ge_transx_rank": ("ge_transx_rank_workspace_bytes", ["model", "n_ent", "n_rel", "d", "B"]),
    "ge_transx_relation_rank": ("ge_transx_relation_rank_workspace_bytes", ["model", "n_ent", "n_rel", "d", "B"]),
    "ge_transx_topk": ("ge_transx_topk_workspace_bytes", ["model", "n_ent", "n_rel", "d", "B", "k"]),
    "ge_transr_adam_step": ("ge_transr_step_workspace_bytes", ["n_ent", "n_rel", "dim_e", "dim_r", "B"]),
    "ge_transr_train_steps": ("ge_transr_step_workspace_bytes", ["n_ent", "n_rel", "dim_e", "dim_r", "B"]),
    "ge_transr_rank": ("ge_transr_rank_workspace_bytes", ["n_ent", "n_rel", "dim_e", "dim_r", "B"]),
    "ge_transr_relation_rank": ("ge_transr_relation_rank_workspace_bytes", ["n_ent", "n_rel", "dim_e", "dim_r", "B"]),
    "ge_transr_topk": ("ge_transr_topk_workspace_bytes", ["n_ent", "n_rel", "dim_e", "dim_r", "B", "k"]),
}

SWEEPS = ("rank", "relation_rank", "topk")
STEPS = ("hinge_step", "adam_step", "train_steps")


def _kind(name):
    return name.split("_", 2)[2]


def _cases(name, lib):
    """(overrides of GOOD, expected code) of one entry point.  NEED stands for the workspace size of the case's own
    shapes; every case is refused, or has B == 0."""
    kind, tx = _kind(name), name.startswith("ge_transx") and name != "ge_transx_draw_batch"
    out = []
    add = lambda code, **kw: out.append((kw, code))
    if name == "ge_transx_draw_batch":
        add(EINVAL, triples=None)
        add(EINVAL, tail_threshold=None)
        for p in ("bh_key", "bh_ent", "bt_key", "bt_ent"):
            add(EINVAL, **{p: None})
        add(EINVAL, T=0)
        add(EINVAL, T=(1 << 32) + 1)
        add(EINVAL, n_known=-1)
        add(EINVAL, B=-1)
        add(EINVAL, n_rel32=0)
        add(EINVAL, n_ent32=0)
        add(EINVAL, pos=None)
        add(EINVAL, neg=None)
        add(0, B=0)
        add(0, B=0, pos=None, neg=None)                       # the outputs matter only when B > 0
        add(0, B=0, n_known=0, bh_key=None, bh_ent=None, bt_key=None, bt_ent=None)
        add(EINVAL, B=0, triples=None)                        # two at once: the sampler's tables come before B == 0
        add(EINVAL, B=0, n_rel32=0)
        return out
    # ---- the model's tables
    if tx:
        dmax = lib.ge_transx_max_dim()
        add(EINVAL, ent=None)
        add(EINVAL, rel=None)
        add(EINVAL, model=1, normal=None)
        add(EINVAL, model=2, ent_transfer=None)
        add(EINVAL, model=2, rel_transfer=None)
        for p in ("ent", "rel", "normal", "ent_transfer", "rel_transfer"):
            add(EINVAL, **{p: A + 1})                         # (a table the model does not read is checked too)
        add(EINVAL, model=-1)
        add(EINVAL, model=3)
        add(EINVAL, d=0)
        add(ENOTSUP, d=dmax + 1)
        add(EINVAL, n_ent=0)
        add(EINVAL, n_rel=0)
        add(EINVAL, n_ent=P31 - 4, n_rel=4)                   # n_ent + n_rel = 2^31
        # two at once
        add(ENOTSUP, d=dmax + 1, ent=A + 1)                   # the width comes before the alignment
        add(ENOTSUP, d=dmax + 1, model=1, normal=None)        # ... and before the model's own tables
        add(EINVAL, d=dmax + 1, model=3)
        add(EINVAL, d=dmax + 1, ent=None)
        add(ENOTSUP, d=dmax + 1, B=-1)                        # the tables come before the batch
        big = dict(n_ent=P31 - 5, n_rel=4)                    # n_ent + n_rel = 2^31 - 1: accepted
    else:
        dmax = lib.ge_transr_max_dim()
        for p in ("ent", "rel", "rel_matrix"):
            add(EINVAL, **{p: None})
            add(EINVAL, **{p: A + 1})
        add(EINVAL, dim_e=0)
        add(EINVAL, dim_r=0)
        add(ENOTSUP, dim_e=dmax + 1)
        add(ENOTSUP, dim_r=dmax + 1)
        add(EINVAL, n_ent=0)
        add(EINVAL, n_rel=0)
        add(EINVAL, n_ent=P31)
        add(EINVAL, n_rel=P31)
        add(ENOTSUP, dim_e=dmax + 1, rel_matrix=A + 1)
        add(EINVAL, dim_r=dmax + 1, ent=None)
        add(EINVAL, dim_e=dmax + 1, dim_r=0)
        add(ENOTSUP, dim_r=dmax + 1, B=-1)
        big = dict(n_ent=P31 - 4, n_rel=4)                    # TransR bounds each count alone: the sum 2^31 is accepted
    # ---- batch, outputs, workspace
    add(EINVAL, B=-1)
    if kind == "score":
        add(0, B=0)
        add(0, B=0, triples=None, out=None)
        add(0, B=0, **big)
        add(EINVAL, triples=None)
        add(EINVAL, out=None)
        add(EINVAL, triples=A + 2)
        add(EINVAL, out=A + 2)
        add(EINVAL, B=P28 + 1, out=None)
        return out
    add(EINVAL, workspace=None)
    add(EINVAL, workspace=A + 8)
    add(ENOMEM, workspace_bytes="NEED-1")
    add(EINVAL, workspace=None, workspace_bytes="NEED-1")     # two at once: the pointer before the size
    add(EINVAL, workspace=A + 8, workspace_bytes=0)
    add(EINVAL, B=-1, workspace_bytes=0)
    if kind in SWEEPS:
        add(EINVAL, B=P28 + 1)
        add(ENOMEM, B=P28, workspace_bytes=0)                 # the largest B is accepted
        add(0, B=0)
        add(0, B=0, **big)
        add(0, B=0, triples=None, workspace=None, workspace_bytes=0)
        add(EINVAL, known_off=A)
        add(EINVAL, known_rc=A)
        add(EINVAL, B=0, known_off=A)                         # two at once: the pair test comes before B == 0
        add(ENOMEM, known_off=A, known_rc=A, workspace_bytes="NEED-1")
        add(EINVAL, known_off=A + 2, known_rc=A)
        add(ENOMEM, known_off=A, known_rc=A + 1, workspace_bytes=0)   # uint16 cells: no alignment asked
        add(EINVAL, triples=None)
        add(EINVAL, triples=A + 2)
        if kind == "topk":
            kmax = lib.ge_transx_topk_max_k()
            add(EINVAL, k=0)
            add(EINVAL, k=kmax + 1)
            add(ENOMEM, k=kmax, workspace_bytes="NEED-1")
            add(EINVAL, k=0, B=0)                             # two at once: k comes before B == 0
            add(EINVAL, k=kmax + 1, workspace_bytes=0)
            add(EINVAL, k=0, B=0, triples=None)
            for p in ("out_id", "out_dist"):
                add(EINVAL, **{p: None})
                add(EINVAL, **{p: A + 2})
        else:
            for p in ("n_before", "n_known_before", "true_dist"):
                add(EINVAL, **{p: None})
                add(EINVAL, **{p: A + 2})
            add(EINVAL, scores_out=A + 2)
            add(ENOMEM, scores_out=A, workspace_bytes="NEED-1")
        add(ENOTSUP, workspace=None, **({"d": dmax + 1} if tx else {"dim_e": dmax + 1}))   # the tables before the outputs
        return out
    assert kind in STEPS
    add(EINVAL, B=0)                                          # a step of no rows is refused
    add(EINVAL, B=0, workspace_bytes=0)
    if kind == "train_steps":
        add(EINVAL, losses=None)
        add(EINVAL, n_steps=-1)
        add(EINVAL, triples=None)
        add(EINVAL, tail_threshold=None)
        add(EINVAL, T=0)
        add(EINVAL, T=(1 << 32) + 1)
        add(EINVAL, n_known=-1)
        for p in ("bh_key", "bh_ent", "bt_key", "bt_ent"):
            add(EINVAL, **{p: None})
        add(ENOMEM, n_known=0, bh_key=None, bh_ent=None, bt_key=None, bt_ent=None, workspace_bytes="NEED-1")
        add(EINVAL, triples=None, workspace_bytes=0)          # two at once: the sampler before the size
        add(ENOMEM, n_steps=0, workspace_bytes="NEED-1")
    else:
        for p in ("pos", "neg", "loss"):
            add(EINVAL, **{p: None})
            add(EINVAL, **{p: A + 2})
        add(EINVAL, pos=None, workspace_bytes=0)
    if not tx:
        add(EINVAL, B=P28 + 1)
        add(EINVAL, b1=1.0)
        add(EINVAL, b2=-0.1)
        add(EINVAL, eps=-1.0)
        add(EINVAL, t=0)
        add(EINVAL, m=None)
        add(EINVAL, v=A + 2)
        add(EINVAL, b1=1.0, workspace_bytes=0)
        add(ENOTSUP, dim_e=dmax + 1, t=0)
    return out


def _call(lib, name, overrides):
    a = dict(GOOD, **overrides)
    if name in SIZE_FN and ("workspace_bytes" not in overrides or a["workspace_bytes"] == "NEED-1"):
        fn, names = SIZE_FN[name]
        need = int(getattr(lib, fn)(*[a[n] for n in names]))
        if a.get("workspace_bytes") == "NEED-1":
            assert need > 0, (name, overrides)
            need -= 1
        a["workspace_bytes"] = need
    return getattr(lib, name)(*[a[n] for n in ENTRIES[name]])


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_entry_refuses_bad_arguments_without_launching(name):
    lib = _lib.load()
    assert len(ENTRIES[name]) == len(_lib.SYMBOLS[name][1])
    cases = _cases(name, lib)
    assert len(cases) >= 15 and any(len(kw) >= 2 and code != 0 for kw, code in cases)
    got = [(kw, _call(lib, name, kw)) for kw, _ in cases]
    wrong = [(kw, code, g) for (kw, code), (_, g) in zip(cases, got) if g != code]
    assert not wrong, f"{name}: (overrides, expected, got) = {wrong}"
