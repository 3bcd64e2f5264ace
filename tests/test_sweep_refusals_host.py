"""Host: what the ComplEx / HolE 1-vs-K entry points (ranks, ranks against stored losses, top-k, their candidate-set
forms, the planes and mask builders, ge_complex_score_1vK) answer to bad arguments, and which code wins when two
arguments are bad at once.

Nothing here reaches a kernel or any other HIP call: every case carries at least one argument that is refused before
the first one, or has B == 0 (K == 0 for ge_rank_planes and ge_complex_score_1vK), which returns before it; every
pointer is a fake address that is never dereferenced.  The module is skipped where a GPU is visible, so that a case
that slipped through validation could never launch on a fake pointer.
  * Rank entries: the refusals of the C ABI's own checks and B == 0 -- behind them the counters are zeroed on the
    stream, so what the route (tests/test_sweep_route_host.py) and the launchers answer is out of reach here.
  * Top-k entries: the whole front -- shape, table alignment (candidate-set form), k range, B == 0, workspace pointer,
    workspace size, row blocks x candidate ranges -- runs before the planes are touched, and all of it is covered.

The expected codes were recorded from the library before these entry points were folded onto one checker and one body
per operation (ge_capi.hip: sweep_args) and passed there unchanged.  They show where the entry points differ: see the
comment at sweep_args."""
import pytest
import torch

from graphembeddings_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: host-only refusals")

EINVAL, ENOTSUP, ENOMEM = _lib.GE_EINVAL, _lib.GE_ENOTSUP, _lib.GE_ENOMEM
COMPLEX, HOLE, SPECTRAL, DIRECT = 0, 1, 2, 3
A = 1 << 12                                   # a fake, 256-byte aligned, never-dereferenced address
INT32_MAX = (1 << 31) - 1
K_PLANES = 40330 * 128                        # d = 200: the first K whose planes reach 2^32 bytes (test_sweep_route_host)
B_BLOCKS = (INT32_MAX // 8 + 1) * 128         # the first B with more than INT32_MAX / 8 row blocks
B_GRID = (1 << 31) * 128                      # 2^31 row blocks x one candidate range: past the top-k grid

HEAD = ["table", "N", "d", "hr", "B"]
KNOWN = ["known_off", "known_rc"]
RANK_OUT = ["n_before", "n_known_before", "true_loss", "scores_out"]
TOPK = HEAD + ["cand", "K", "max_norm", "model", "cand_is_head"] + KNOWN + ["k", "out_id", "out_loss", "planes",
                                                                           "workspace", "workspace_bytes"]
SETS = ["row_set", "mask", "n_sets"]

# entry point: its arguments in ABI order
ENTRIES = {
    "ge_rank_planes": ["table", "N", "d", "cand", "K", "max_norm", "model", "planes_out", "stream"],
    "ge_rank_1vK_planes": HEAD + ["true_id", "cand", "K", "max_norm", "model", "cand_is_head"] + KNOWN + RANK_OUT +
                          ["planes", "stream"],
    "ge_rank_1vK": HEAD + ["true_id", "cand", "K", "max_norm", "model", "cand_is_head"] + KNOWN + RANK_OUT + ["stream"],
    "ge_complex_rank_1vK": HEAD + ["true_id", "cand", "K", "max_norm", "cand_is_head"] + KNOWN + RANK_OUT + ["stream"],
    "ge_rank_1vK_vs_loss": HEAD + ["true_id", "ref_loss", "cand", "K", "max_norm", "model", "cand_is_head"] + KNOWN +
                           ["n_before", "n_known_before", "planes", "stream"],
    "ge_rank_1vK_masked": HEAD + ["true_id", "cand", "K", "max_norm", "model", "cand_is_head"] + KNOWN + RANK_OUT +
                          ["planes"] + SETS + ["stream"],
    "ge_topk_1vK_planes": TOPK + ["stream"],
    "ge_topk_1vK_masked": TOPK + SETS + ["stream"],
    "ge_complex_score_1vK": HEAD + ["cand", "K", "max_norm", "apply_sigmoid", "cand_is_head", "out", "stream"],
    "ge_candidate_mask_from_classes": ["cand_class", "K", "allow", "n_sets", "n_class", "mask", "stream"],
    "ge_candidate_mask_from_cells": ["cells", "M", "n_sets", "K", "mask", "stream"],
}

# a call every entry point would accept (never made as it stands)
GOOD = dict(table=A, N=1000, d=200, hr=A, B=2, true_id=A, ref_loss=A, cand=A, K=300, max_norm=1.0, model=COMPLEX,
            cand_is_head=0, known_off=None, known_rc=None, n_before=A, n_known_before=A, true_loss=A, scores_out=None,
            planes=None, planes_out=A, row_set=A, mask=A, n_sets=2, k=5, out_id=A, out_loss=A, workspace=A,
            apply_sigmoid=0, out=A, cand_class=A, allow=A, n_class=3, cells=A, M=4, stream=None)

RANKS = ("ge_rank_1vK_planes", "ge_rank_1vK", "ge_complex_rank_1vK", "ge_rank_1vK_vs_loss", "ge_rank_1vK_masked")
TOPKS = ("ge_topk_1vK_planes", "ge_topk_1vK_masked")


def _cases(name):
    """(overrides of GOOD, expected code) of one entry point.  NEED stands for ge_topk_workspace_bytes of the case's
    own shapes; every case is refused before the first HIP call, or returns 0 before it."""
    out = []
    add = lambda code, **kw: out.append((kw, code))
    masked, has_model = name.endswith("_masked"), "model" in ENTRIES[name]
    has_planes = "planes" in ENTRIES[name]
    if name == "ge_candidate_mask_from_classes":
        for kw in (dict(K=0), dict(K=INT32_MAX + 1), dict(n_sets=0), dict(n_class=0), dict(cand_class=None),
                   dict(allow=None), dict(mask=None), dict(cand_class=A + 2), dict(allow=A + 1), dict(mask=A + 2)):
            add(EINVAL, **kw)
        add(ENOTSUP, K=INT32_MAX, n_sets=INT32_MAX)           # n_sets x mask words: past the grid
        add(EINVAL, K=INT32_MAX, n_sets=INT32_MAX, mask=None)  # two at once: the pointers come first
        add(EINVAL, K=INT32_MAX, n_sets=INT32_MAX, allow=A + 2)
        add(EINVAL, K=0, n_sets=0)
        add(EINVAL, n_class=0, mask=A + 1)
        return out
    if name == "ge_candidate_mask_from_cells":
        for kw in (dict(K=0), dict(K=INT32_MAX + 1), dict(n_sets=0), dict(M=-1), dict(mask=None), dict(cells=None),
                   dict(cells=A + 2), dict(mask=A + 2), dict(M=0, cells=A + 1), dict(M=0, mask=None)):
            add(EINVAL, **kw)
        add(ENOTSUP, M=1 << 40)                               # the cells: past the grid
        add(EINVAL, M=1 << 40, mask=None)                     # two at once
        add(EINVAL, M=1 << 40, cells=A + 2)
        add(EINVAL, M=1 << 40, K=0)
        add(EINVAL, M=-1, n_sets=0)
        return out
    if name == "ge_rank_planes":
        for kw in (dict(K=-1), dict(table=None), dict(N=0), dict(d=0), dict(max_norm=0.0), dict(max_norm=-1.0),
                   dict(planes_out=None), dict(cand=None), dict(model=-1), dict(model=4)):
            add(EINVAL, **kw)
        add(ENOTSUP, model=HOLE)
        add(ENOTSUP, model=DIRECT)
        # the launcher, all of it ahead of its first HIP call: the shape, then the two alignments, then K == 0
        for kw in (dict(d=48), dict(d=296), dict(d=57), dict(max_norm=8.5), dict(K=K_PLANES)):
            add(ENOTSUP, **kw)
        add(EINVAL, planes_out=A + 128)
        add(EINVAL, table=A + 4)
        add(0, K=0)
        add(0, K=0, cand=None)
        add(0, K=0, model=SPECTRAL)
        # two at once
        add(ENOTSUP, model=HOLE, cand=None)                   # the model comes before the candidates
        add(EINVAL, model=HOLE, planes_out=None)              # ... and behind the table, max_norm and the planes pointer
        add(EINVAL, model=HOLE, max_norm=0.0)
        add(ENOTSUP, d=48, planes_out=A + 128)                # the shape comes before the alignments
        add(ENOTSUP, d=48, K=0)                               # ... and before K == 0
        add(EINVAL, table=A + 4, K=0)
        add(ENOTSUP, model=HOLE, d=48)
        add(EINVAL, model=7, d=48)
        return out
    if name == "ge_complex_score_1vK":
        for kw in (dict(B=-1), dict(K=-1), dict(table=None), dict(N=0), dict(d=0), dict(max_norm=0.0), dict(d=7),
                   dict(hr=None), dict(cand=None), dict(out=None)):
            add(EINVAL, **kw)
        add(0, B=0)
        add(0, K=0)
        add(0, B=0, hr=None, cand=None, out=None)
        add(0, K=0, hr=None, cand=None, out=None)
        add(0, B=0, table=A + 4)
        add(EINVAL, B=0, d=7)                                 # two at once: an odd dim comes before B == 0
        add(EINVAL, K=0, max_norm=0.0)
        add(EINVAL, B=-1, K=0)
        # route_score refuses what no kernel's grid holds: more than 65,535 row tiles off the main road
        add(ENOTSUP, B=128 * 65535 + 1, table=A + 4)
        add(ENOTSUP, B=128 * 65535 + 1, d=50)
        add(EINVAL, B=128 * 65535 + 1, table=A + 4, out=None)
        return out
    # ---- the rank and top-k sweeps: table, shape and max_norm first
    first = [dict(B=-1), dict(table=None), dict(N=0), dict(d=0), dict(d=-8), dict(max_norm=0.0), dict(max_norm=-1.0)]
    for kw in first:
        add(EINVAL, **kw)
    if name in RANKS:
        add(EINVAL, K=-1)
    else:
        for kw in (dict(K=-1), dict(K=0), dict(k=0), dict(k=-3), dict(K=0, B=0), dict(k=0, B=0)):
            add(EINVAL, **kw)                                 # top-k: no empty candidate list, and k in the first line
    if masked:
        for kw in (dict(row_set=None), dict(mask=None), dict(n_sets=0), dict(n_sets=-1), dict(row_set=A + 2),
                   dict(mask=A + 1)):
            add(EINVAL, **kw)
            add(EINVAL, B=0, **kw)
        add(EINVAL, row_set=None, model=HOLE)                 # two at once: the sets come before the model
        add(EINVAL, mask=A + 2, model=7)
        add(EINVAL, n_sets=0, d=48)
        add(EINVAL, n_sets=0, B=-1)
    if has_model:
        add(ENOTSUP, model=HOLE)
        add(ENOTSUP, model=DIRECT)
        add(EINVAL, model=-1)
        add(EINVAL, model=4)
        add(ENOTSUP, model=HOLE, B=0)
        add(EINVAL, model=HOLE, table=None)                   # two at once: the table comes before the model
        add(EINVAL, model=HOLE, max_norm=0.0)
        add(ENOTSUP, model=HOLE, hr=None)                     # ... and the model before the pointers
        add(ENOTSUP, model=HOLE, known_off=A)
        add(ENOTSUP, model=HOLE, d=48)
    # ---- pointers (B > 0 only), the known pair, the planes
    ptrs = ["hr", "cand", "out_id", "out_loss"] if name in TOPKS else ["hr", "true_id", "cand", "n_before", "n_known_before"]
    if name == "ge_rank_1vK_vs_loss":
        ptrs.append("ref_loss")
    for p in ptrs:
        add(EINVAL, **{p: None})
    add(0, B=0)
    add(0, B=0, **{p: None for p in ptrs})
    add(0, B=0, table=A + 4) if not masked or name in RANKS else add(EINVAL, B=0, table=A + 4)
    add(EINVAL, known_off=A)
    add(EINVAL, known_rc=A)
    add(EINVAL, B=0, known_off=A)                             # two at once: the pair test comes before B == 0
    add(0, B=0, known_off=A, known_rc=A)
    add(0, B=0, known_off=A + 2, known_rc=A + 1)              # no alignment asked of the lists
    if has_planes:
        add(EINVAL, planes=A + 128)                           # 256-byte alignment
        add(EINVAL, B=0, planes=A + 128)                      # two at once: the planes come before B == 0
        add(EINVAL, planes=A, K=K_PLANES)                     # planes no sweep could address
        add(0, B=0, planes=A)
        add(EINVAL, planes=A + 128, known_off=A)
        add(EINVAL, planes=A + 128, hr=None)
    if name in RANKS:
        add(0, B=0, K=0)
        add(0, B=0, K=0, cand=None)
        add(EINVAL, B=1, K=-1, cand=None)
        if has_planes:
            add(EINVAL, planes=A, K=0)                        # no planes of no candidates
            add(EINVAL, planes=A, K=0, B=0)
        # what the route or the launcher would refuse is not looked at when B == 0 ... except by the candidate-set form,
        # which asks for the split-precision range ahead of the planes and of B == 0
        code = ENOTSUP if masked else 0
        for kw in (dict(d=48), dict(d=296), dict(d=57), dict(max_norm=8.5)):
            add(code, B=0, **kw)
        if masked:
            for kw in (dict(d=48), dict(d=296), dict(d=57), dict(max_norm=8.5)):
                add(ENOTSUP, **kw)
            add(ENOTSUP, d=48, planes=A + 128)                # two at once: the range comes before the planes
            add(EINVAL, d=48, known_off=A)                    # ... and behind the pair test
            add(EINVAL, d=48, hr=None)
        elif has_planes:
            add(EINVAL, B=0, d=48, planes=A)                  # (no planes at this dim)
        return out
    # ---- top-k: the launcher's front, in its order
    for kw in (dict(d=48), dict(d=296), dict(d=57), dict(max_norm=8.5), dict(K=K_PLANES)):
        add(ENOTSUP, **kw)
        add(ENOTSUP, B=0, **kw)                               # two at once: the shape comes before B == 0
    add(ENOTSUP, d=48, workspace=None)                        # ... before the workspace
    add(ENOTSUP, d=48, workspace_bytes=0)
    add(ENOTSUP, d=48, k=129)
    add(ENOTSUP, d=48, table=A + 4)
    add(ENOTSUP if masked else EINVAL, d=48, planes=A)        # the candidate-set form: the range before the planes
    add(EINVAL, d=48, hr=None)
    # more than INT32_MAX / 8 row blocks: the candidate-set form alone
    add(ENOTSUP if masked else ENOMEM, B=B_BLOCKS, workspace_bytes=0)
    add(ENOMEM, B=B_BLOCKS - 128, workspace_bytes=0)
    # a table that is not 16-byte aligned: refused by the candidate-set form alone, behind the shape and ahead of k
    add(EINVAL if masked else ENOMEM, table=A + 4, workspace_bytes="NEED-1")
    add(EINVAL if masked else ENOTSUP, table=A + 4, k=129)
    add(EINVAL if masked else ENOMEM, table=A + 8, workspace_bytes=0)
    add(ENOTSUP, k=129)
    add(ENOMEM, k=128, workspace_bytes="NEED-1")
    add(ENOTSUP, k=129, B=0)                                  # two at once: the k range comes before B == 0
    add(ENOTSUP, k=129, workspace=None)
    add(0, B=0, workspace=None, workspace_bytes=0)
    add(0, B=0, workspace=A + 8)
    add(EINVAL, workspace=None)
    add(EINVAL, workspace=A + 128)
    add(ENOMEM, workspace_bytes="NEED-1")
    add(ENOMEM, workspace_bytes=0)
    add(EINVAL, workspace=None, workspace_bytes="NEED-1")     # two at once: the pointer before the size
    add(EINVAL, workspace=A + 8, workspace_bytes=0)
    add(ENOMEM, known_off=A, known_rc=A, workspace_bytes="NEED-1")
    add(ENOMEM, planes=A, workspace_bytes="NEED-1")
    add(ENOMEM, model=SPECTRAL, workspace_bytes="NEED-1")
    add(ENOMEM, K=128 * 40, B=1, workspace_bytes="NEED-1")    # many candidate ranges
    add(ENOMEM, B=128 * 256, workspace_bytes="NEED-1")        # one range
    # row blocks x candidate ranges past INT32_MAX, behind the size: the candidate-set form stops at its row blocks
    add(ENOTSUP, B=B_GRID, workspace_bytes=1 << 62)
    add(ENOTSUP if masked else ENOMEM, B=B_GRID, workspace_bytes="NEED-1")
    add(ENOTSUP if masked else EINVAL, B=B_GRID, workspace=None)
    return out


def _call(lib, name, overrides):
    a = dict(GOOD, **overrides)
    if name in TOPKS and ("workspace_bytes" not in overrides or a["workspace_bytes"] == "NEED-1"):
        need = int(lib.ge_topk_workspace_bytes(a["B"], a["K"], a["k"]))
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
