"""GPU: what the C ABI (include/ge_hip.h) may touch.  Every entry point that writes device memory is called straight
through _lib on guard-banded, poisoned buffers of EXACTLY the declared sizes (tests/abi_guard.py), and each case asserts

  (a) every guard of every buffer is intact after the call;
  (b) the outputs agree with the project's high-precision reference of the operation, within the bound the existing
      GPU test of that entry point uses (named where it is applied);
  (c) two runs from identical inputs, outputs and workspace pre-filled 0x00 and 0xFF, give bitwise equal outputs and
      tables (a float-atomic path is compared within its existing tolerance instead, and says so);
  (d) for a workspace: `need - 1` bytes is GE_ENOMEM, the pointer offset by 16 bytes is GE_EINVAL, and after either
      refusal every output is still all poison.  Those calls pass the real, full-size guarded buffers and lie only in
      the number.

Record buffers (ge_train_prepare_steps, ge_shard_plan, ge_shard_owner_plan) have words the header leaves undefined --
items and slot lists past n_items, req_row past the requested count: (c) compares what the header defines.
"""
import numpy as np
import pytest
import torch

from graphembeddings_amd import _lib
from oracle import c_oracle as CO
from oracle import hole_oracle as O
from oracle import transx_oracle as TO
from tests import abi_guard as AG
from tests import neighbors_ref as NR
from tests import relation_rank_ref as RRK
from tests import topk_ref as TK
from tests import translation_rank_ref as RK
from tests import transr_ref as RR
from tests import transx_ref as XR

pytestmark = pytest.mark.gpu

ENOMEM, EINVAL = _lib.GE_ENOMEM, _lib.GE_EINVAL
SCORE_TOL, TABLE_TOL = 1e-5, 5e-6        # test_gpu_parity.py
F32_EPS = 2.0 ** -23                     # test_gpu_transr.py
I32, I64, F32, U16 = np.int32, np.int64, np.float32, np.uint16
XMODELS = ("transe", "transh", "transd")

# entry point -> the test that guards it (test_every_writing_entry_point_is_guarded checks this against _lib.SYMBOLS;
# each test checks that it really called what it claims)
GUARDED = {}
CALLED = set()                                          # the entry points the running case has called through drive()


def guards(*names):
    def deco(fn):
        for n in names:
            GUARDED.setdefault(n, fn.__name__)
        fn.guarded = names
        return fn
    return deco


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")
    CALLED.clear()                                      # what THIS case calls (claimed() checks it at the case's end)


def S():
    return AG.stream()


def ws_args(buf, mode):
    """(pointer, byte count) of a workspace for the three calls of (d)."""
    if mode == "short":
        return buf.ptr, buf.nbytes - 1
    if mode == "offset":
        return buf.ptr + 16, buf.nbytes
    return buf.ptr, buf.nbytes


def drive(case, verify=None, ws=False, offset=True, compare=None, canon=None):
    """case(A, mode) -> status code: allocates on arena A and calls; mode "exact" | "short" | "offset" reaches the
    workspace arguments through ws_args.  Returns the 0x00-poisoned arena of the good call."""
    runs = []
    for poison in (0x00, 0xFF):
        A = AG.Arena("", poison)
        rc = case(A, "exact")
        assert rc == 0, "%s returned %d" % (A.entry, rc)
        A.assert_intact("(poison 0x%02X)" % poison)
        runs.append(A)
        CALLED.update(A.called)
    outs = [canon(A) if canon else A.outputs() for A in runs]
    if compare is None:
        AG.assert_bitwise_equal(runs[0].entry, outs[0], outs[1])
    else:
        compare(outs[0], outs[1])
    if verify is not None:
        verify(runs[0])
    if ws:
        for mode, code in (("short", ENOMEM), ("offset", EINVAL))[:2 if offset else 1]:
            A = AG.Arena("", 0xFF)
            rc = case(A, mode)
            assert rc == code, "%s with a %s workspace returned %d, not %d" % (A.entry, mode, rc, code)
            A.assert_intact("(refused: %s workspace)" % mode)
            A.assert_outputs_poison(mode)
    return runs[0]


def claimed(fn):
    missing = set(fn.guarded) - CALLED
    assert not missing, "the test never called %s" % sorted(missing)


# largest deviation from the reference per family, as a fraction of the bound (and in absolute terms): printed by every
# check so that a run with `-s` records them
WORST = {}


def near(family, err, bound, strict=False):
    """assert err <= bound (err < bound when strict) elementwise; remembers the family's worst err / bound."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if err.size:
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
        w = WORST.setdefault(family, [0.0, 0.0])
        if float(np.max(ratio)) > w[0]:
            w[0], w[1] = float(np.max(ratio)), float(np.max(err))
            print("DEV family %d: err/bound %.4g, largest |err| %.4g" % (family, w[0], w[1]))
    assert np.all(err < bound) if strict else np.all(err <= bound), (float(np.max(err)) if err.size else 0.0, np.max(bound))


def table_of(N, d, seed, scale=0.3):
    rng = np.random.default_rng(seed)
    t = (rng.standard_normal((N, d)) * scale).astype(F32)
    t[::3] *= 4.0                                       # a third of the rows outside the unit ball: the clip
    return t


def triples_of(N, B, seed, bad):
    rng = np.random.default_rng(seed)
    tr = rng.integers(0, N, size=(B, 3)).astype(I32)
    if bad:
        tr[B // 2, 1] = N                               # one id out of range: NaN there, nothing else touched
    return tr


def types_of(N, n_rel, n_types=4):
    """Shared holE.py table: rows [0, n_rel) are relations (type -1), entity e has type e % n_types."""
    id_to_type = np.full(N, -1, I32)
    ent = np.arange(n_rel, N)
    id_to_type[ent] = ent % n_types
    lists = [ent[ent % n_types == t] for t in range(n_types)]
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(I64)
    return id_to_type, offsets, np.concatenate(lists).astype(I32)


def from_spectral(p):
    """ge_hole_from_spectral in fp64: the real rows whose packed half spectra are the rows of p."""
    d = p.shape[1]
    k = d // 2
    X = np.zeros((p.shape[0], k + 1), dtype=np.complex128)
    X[:, :k] = p[:, :k]
    X[:, k] = p[:, k]
    X[:, 1:k] += 1j * p[:, k + 1:]
    return np.fft.irfft(X, n=d, axis=1)


def to_spectral(x):
    """ge_hole_to_spectral in fp64: [Re X_0 .. Re X_{k-1} | Re X_k, Im X_1 .. Im X_{k-1}] of X = fft(x)."""
    d = x.shape[1]
    k = d // 2
    X = np.fft.fft(x.astype(np.float64), axis=1)
    return np.concatenate([X[:, :k].real, X[:, k:k + 1].real, X[:, 1:k].imag], 1)


def xtabs(model, E, R, d, seed):
    rng = np.random.default_rng(seed)
    rows = {"ent": E, "rel": R, "normal_vector": R, "ent_transfer": E, "rel_transfer": R}
    return {k: (rng.standard_normal((rows[k], d)) * 0.5).astype(F32) for k in ("ent", "rel") + XR.EXTRA[model]}


def xargs(A, model, l1, tabs, kind="in", shift=0):
    """The leading arguments every ge_transx_* entry takes; the tables as guarded buffers of kind `kind` (shift = 4:
    every table starts 4 bytes past a 16-byte boundary, the misaligned variant of the sweeps)."""
    b = {k: A.data(k, v, kind, shift) for k, v in tabs.items()}
    p = lambda k: b[k].ptr if k in b else None
    return (XMODELS.index(model), int(l1), p("ent"), tabs["ent"].shape[0], p("rel"), tabs["rel"].shape[0],
            p("normal_vector"), p("ent_transfer"), p("rel_transfer"), tabs["ent"].shape[1])


def rtabs(E, R, dim_e, dim_r, seed):
    return {k: v.astype(F32) for k, v in RR.random_tables(E, R, dim_e, dim_r, np.random.default_rng(seed), 0.5).items()}


def rargs(A, l1, tabs, kind="in", shift=0):
    b = {k: A.data(k, v, kind, shift) for k, v in tabs.items()}
    dim_e, dim_r = RR.dims(tabs)
    return (int(l1), b["ent"].ptr, tabs["ent"].shape[0], b["rel"].ptr, b["rel_matrix"].ptr, tabs["rel"].shape[0],
            dim_e, dim_r)


def f64(tabs):
    return {k: v.astype(np.float64) for k, v in tabs.items()}


def check_nan_rows(got, bad_rows):
    ok = np.ones(len(got), bool)
    ok[list(bad_rows)] = False
    assert np.isnan(got[~ok]).all() and np.isfinite(got[ok]).all()
    return ok


# =============================================================== 1. scores and losses (out [B])
@guards("ge_complex_score", "ge_complex_score_strided", "ge_hole_score", "ge_hole_spectral_score", "ge_complex_logloss",
        "ge_hinge_loss")
@pytest.mark.parametrize("B,bad", [(1, False), (1, True), (63, True), (64, True), (65, True)])
@pytest.mark.parametrize("d", [2, 50, 200])
def test_scores_and_losses(B, d, bad):
    """Bounds: SCORE_TOL (test_gpu_parity.py test_score_*, test_hinge_loss_forward), 2e-5 relative for the log-loss
    (test_evaluate_triples_with_label_is_the_logloss_branch)."""
    N = 97
    table = table_of(N, d, seed=d)
    t64 = table.astype(np.float64)
    tr = triples_of(N, B, seed=B, bad=bad)
    neg = tr.copy()
    neg[:, 0] = np.random.default_rng(B + 1).integers(0, N, B)
    bad_rows = [B // 2] if bad else []
    ok = np.ones(B, bool)
    ok[bad_rows] = False

    def score_case(name, tab, ld=None):
        def case(A, mode):
            t = A.data("table", tab)
            trb, out = A.data("triples", tr), A.out("out", 4 * B)
            extra = () if ld is None else (ld,)
            return A.call(name, t.ptr, N, d, *extra, trb.ptr, B, 1.0, 1, out.ptr, S())
        return case

    def verify_with(ref):
        def verify(A):
            got = A["out"].get(F32)
            check_nan_rows(got, bad_rows)
            if ok.any():
                near(1, np.abs(got[ok] - ref(tr[ok])), SCORE_TOL, strict=True)
        return verify

    drive(score_case("ge_complex_score", table), verify_with(lambda t: O.evaluate_triples(t, t64)[:, 0]))
    ld = d + 3                                          # padded rows; the pad columns hold NaN and are never read into a result
    padded = np.full((N, ld), np.nan, F32)
    padded[:, :d] = table
    drive(score_case("ge_complex_score_strided", padded, ld), verify_with(lambda t: O.evaluate_triples(t, t64)[:, 0]))
    drive(score_case("ge_hole_score", table), verify_with(lambda t: O.hole_evaluate_triples(t, t64)[:, 0]))
    drive(score_case("ge_hole_spectral_score", to_spectral(table).astype(F32)),
          verify_with(lambda t: O.hole_evaluate_triples(t, t64)[:, 0]))

    l2 = 0.1

    def logloss(A, mode):
        t, trb = A.data("table", table), A.data("triples", tr)
        out, w = A.out("out", 4 * B), A.ws("workspace", 256)
        return A.call("ge_complex_logloss", t.ptr, N, d, trb.ptr, B, -1.0, l2, 1.0, out.ptr, *ws_args(w, mode), S())

    def verify_logloss(A):
        got = A["out"].get(F32)
        check_nan_rows(got, bad_rows)
        if ok.any():
            exp = O.logloss_values(tr[ok], -np.ones(int(ok.sum())), t64, l2)
            near(1, np.abs(got[ok] - exp), 2e-5 * max(1.0, np.abs(exp).max()), strict=True)
    drive(logloss, verify_logloss, ws=True)

    for model, name, tab in ((0, "complex", table), (1, "hole", table), (2, "hole", to_spectral(table).astype(F32))):
        def hinge(A, mode, model=model, tab=tab):
            t, p, n = A.data("table", tab), A.data("pos", tr), A.data("neg", neg)
            loss, sig = A.out("loss", 4 * B), A.out("sig_out", 8 * B)
            return A.call("ge_hinge_loss", t.ptr, N, d, p.ptr, n.ptr, B, 0.2, 1.0, model, loss.ptr, sig.ptr, S())

        def verify_hinge(A, name=name):
            loss, sig = A["loss"].get(F32), A["sig_out"].get(F32)
            check_nan_rows(loss, bad_rows)
            if ok.any():
                ev = O.evaluate_triples if name == "complex" else O.hole_evaluate_triples
                near(1, np.abs(loss[ok] - O.evaluate_batch(tr[ok], neg[ok], t64, 0.2, model=name)[:, 0]), SCORE_TOL, strict=True)
                near(1, np.abs(sig[:B][ok] - ev(tr[ok], t64)[:, 0]), SCORE_TOL, strict=True)
                near(1, np.abs(sig[B:][ok] - ev(neg[ok], t64)[:, 0]), SCORE_TOL, strict=True)
        drive(hinge, verify_hinge)
    claimed(test_scores_and_losses)


@guards("ge_transx_score", "ge_transr_score")
@pytest.mark.parametrize("B,bad", [(1, False), (1, True), (63, True), (64, True), (65, True)])
def test_translation_scores(B, bad):
    """Bounds: 1e-5 |ref| + 1e-7 (test_gpu_transx.py test_score_matches_fp64); TransR (2|4) (dim_e + dim_r + 8) eps
    * magnitude (test_gpu_transr.py test_score_matches_fp64)."""
    E, R = 61, 7
    rng = np.random.default_rng(B)
    tr = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, R, B)], 1).astype(I32)
    bad_rows = [B // 2] if bad else []
    if bad:
        tr[B // 2, 0] = E
    ok = np.ones(B, bool)
    ok[bad_rows] = False
    for model in XMODELS:
        for d in (2, 50, 200):
            for l1 in (True, False):
                tabs = xtabs(model, E, R, d, seed=d)

                def case(A, mode):
                    a = xargs(A, model, l1, tabs)
                    trb, out = A.data("triples", tr), A.out("out", 4 * B)
                    return A.call("ge_transx_score", *a, trb.ptr, B, out.ptr, S())

                def verify(A):
                    got = A["out"].get(F32).astype(np.float64)
                    check_nan_rows(got, bad_rows)
                    if ok.any():
                        ref = XR.score(model, f64(tabs), tr[ok], l1)
                        near(1, np.abs(got[ok] - ref), 1e-5 * np.abs(ref) + 1e-7)
                drive(case, verify)
    for dim_e, dim_r in ((7, 33), (64, 64)):
        for l1 in (True, False):
            tabs = rtabs(E, R, dim_e, dim_r, seed=dim_e)

            def case(A, mode):
                a = rargs(A, l1, tabs)
                trb, out = A.data("triples", tr), A.out("out", 4 * B)
                return A.call("ge_transr_score", *a, trb.ptr, B, out.ptr, S())

            def verify(A):
                got = A["out"].get(F32).astype(np.float64)
                check_nan_rows(got, bad_rows)
                if ok.any():
                    ref, mag = RR.score(f64(tabs), tr[ok], l1), RR.score_magnitude(f64(tabs), tr[ok], l1)
                    near(1, np.abs(got[ok] - ref), (2.0 if l1 else 4.0) * (dim_e + dim_r + 8) * F32_EPS * mag + 1e-30)
            drive(case, verify)
    claimed(test_translation_scores)


# =============================================================== 2. gradients and single steps
def distinct_pairs(N, B, seed, lo=0):
    """(pos, neg) whose 4B named rows are all different (no row receives two gradient slots: the scatter's float
    atomics have nothing to reorder) and include row `lo` and row N - 1.  neg replaces the head or the tail."""
    assert 4 * B <= N - lo
    rng = np.random.default_rng(seed)
    ids = np.concatenate([[lo, N - 1], lo + 1 + rng.permutation(N - lo - 2)[:4 * B - 2]])
    rng.shuffle(ids)
    q = ids.reshape(B, 4)
    pos = q[:, :3].astype(I32)
    neg = pos.copy()
    side = rng.integers(0, 2, B)
    neg[np.arange(B), side] = q[:, 3]
    return pos, neg


def unnamed_rows_unchanged(before, after, *named):
    keep = np.ones(len(before), bool)
    for ids in named:
        ids = np.asarray(ids).ravel()
        keep[ids[(ids >= 0) & (ids < len(before))]] = False
    assert np.array_equal(before[keep].view(I32), after[keep].view(I32)), "a row the batch does not name changed"


@guards("ge_hinge_grad", "ge_complex_hinge_step", "ge_hole_hinge_step", "ge_complex_logloss_step", "ge_scatter_add_rows",
        "ge_gather_rows")
@pytest.mark.parametrize("B", [1, 65, 257])
@pytest.mark.parametrize("d", [50, 200])
def test_gradients_and_single_steps(B, d):
    """Bounds: SCORE_TOL / TABLE_TOL (test_gpu_parity.py test_indexed_slices_match_closed_form,
    test_hinge_step_matches_golden, test_logloss_step_matches_oracle), exact gather, 1e-5 for the float-atomic scatter
    (test_gather_and_scatter_rows)."""
    N, lr, margin = 1100, 0.05, 0.2
    table = table_of(N, d, seed=d + B)
    t64 = table.astype(np.float64)
    pos, neg = distinct_pairs(N, B, seed=B)
    lib = _lib.load()

    for model, name in ((0, "complex"), (1, "hole"), (2, "hole")):
        tab = to_spectral(table).astype(F32) if model == 2 else table

        def grad(A, mode, model=model, tab=tab):
            t, p, n = A.data("rows", tab), A.data("pos", pos), A.data("neg", neg)
            loss, gi, gv = A.out("loss", 4 * B), A.out("grad_idx", 24 * B), A.out("grad_val", 24 * B * d)
            return A.call("ge_hinge_grad", t.ptr, N, d, p.ptr, n.ptr, B, margin, lr, 1.0, model, loss.ptr, gi.ptr,
                          gv.ptr, S())

        def verify_grad(A, model=model, name=name):
            loss, gi, gv = A["loss"].get(F32), A["grad_idx"].get(I32), A["grad_val"].get(F32, (6 * B, d))
            idx, val, oloss = O.hinge_grads(pos, neg, t64, margin=margin, model=name)
            near(2, np.abs(loss - oloss), SCORE_TOL, strict=True)
            sfun = O.complex_score if name == "complex" else O.hole_score
            on = O.sigmoid(sfun(pos, t64)) - O.sigmoid(sfun(neg, t64)) + margin >= 0
            gi2 = gi.reshape(B, 6)
            for X in range(3):
                same = pos[:, X] == neg[:, X]
                assert np.array_equal(gi2[:, X], np.where(on, pos[:, X], -1))
                assert np.array_equal(gi2[:, 3 + X], np.where(on & ~same, neg[:, X], -1))
            acc, exp = np.zeros_like(t64), np.zeros_like(t64)
            np.add.at(acc, gi[gi >= 0], gv[gi >= 0].astype(np.float64))
            np.add.at(exp, idx, -lr * val)
            if model == 2:              # spectral gradient rows: the transform is linear, so back in the real domain they
                acc = from_spectral(acc)    # are the HolE update (TABLE_TOL there, as
                                            # test_hole_spectral_scores_and_step_match_the_hole_oracle holds the step)
            near(2, np.abs(acc - exp), TABLE_TOL, strict=True)
        def grad_canon(A):
            # (the header defines no value for the gradient row of an empty slot, grad_idx = -1: those rows are left out)
            o = A.outputs()
            o["grad_val"] = o["grad_val"].reshape(6 * B, 4 * d)[A["grad_idx"].get(I32) >= 0]
            return o
        drive(grad, verify_grad, canon=grad_canon)

    need = lib.ge_hinge_step_workspace_bytes(B, d)
    for fn, name in (("ge_complex_hinge_step", "complex"), ("ge_hole_hinge_step", "hole")):
        def step(A, mode, fn=fn):
            t, p, n = A.table("table", table), A.data("pos", pos), A.data("neg", neg)
            loss, w = A.out("loss", 4 * B), A.ws("workspace", need)
            return A.call(fn, t.ptr, N, d, p.ptr, n.ptr, B, margin, lr, 1.0, loss.ptr, *ws_args(w, mode), S())

        def verify_step(A, name=name):
            new, oloss = O.sgd_step(t64, pos, neg, lr=lr, margin=margin, model=name)
            after = A["table"].get(F32, (N, d))
            near(2, np.abs(A["loss"].get(F32) - oloss), SCORE_TOL, strict=True)
            near(2, np.abs(after - new), TABLE_TOL, strict=True)
            unnamed_rows_unchanged(table, after, pos, neg)
        drive(step, verify_step, ws=True)

    # the log-loss step scatters one slot per (triple, column): 3M distinct rows, so no atomics meet
    M = B
    tri = distinct_pairs(N, M, seed=B + 7)[0]
    labels = np.where(np.arange(M) % 2 == 0, 1.0, -1.0).astype(F32)
    l2, lr2 = 0.003, 0.01
    need_ll = lib.ge_logloss_step_workspace_bytes(M, d)

    def llstep(A, mode):
        t, tb, lb = A.table("table", table), A.data("triples", tri), A.data("labels", labels)
        loss, w = A.out("loss", 4 * M), A.ws("workspace", need_ll)
        return A.call("ge_complex_logloss_step", t.ptr, N, d, tb.ptr, lb.ptr, M, lr2, l2, 1.0, loss.ptr,
                      *ws_args(w, mode), S())

    def verify_ll(A):
        # the oracle's step on these triples and labels (logloss_step's formula with its labels made explicit)
        oloss = O.logloss_values(tri, labels.astype(np.float64), t64, l2)
        s = O.complex_score(tri, t64)
        y = labels.astype(np.float64)
        gh, gt, gr = O._side_grads(tri, t64, -y * O.sigmoid(-y * s), 1.0, "complex")
        new = t64 * (1.0 - lr2 * M * l2)
        for col, g in ((0, gh), (1, gt), (2, gr)):
            np.subtract.at(new, tri[:, col], lr2 * g)
        loss = A["loss"].get(F32)
        near(2, np.abs(loss - oloss), 2e-5 * max(1.0, np.abs(oloss).max()), strict=True)
        near(2, np.abs(A["table"].get(F32, (N, d)) - new), TABLE_TOL, strict=True)  # (the dense decay moves every row)
    drive(llstep, verify_ll, ws=True)

    R = 6 * B
    rng = np.random.default_rng(B)
    gidx = np.full(R, -1, I32)
    live = rng.permutation(R)[:min(R, N) // 2]
    gidx[live] = np.concatenate([[0, N - 1], 1 + rng.permutation(N - 2)])[:len(live)]
    gval = rng.standard_normal((R, d)).astype(F32)

    def gather(A, mode):
        t, ib, out = A.data("table", table), A.data("idx", gidx), A.out("out", 4 * R * d)
        return A.call("ge_gather_rows", t.ptr, N, d, ib.ptr, R, out.ptr, S())

    def verify_gather(A):
        exp = np.where((gidx >= 0)[:, None], table[np.clip(gidx, 0, N - 1)], 0.0).astype(F32)
        assert np.array_equal(A["out"].get(F32, (R, d)), exp)
    drive(gather, verify_gather)

    def scatter_case(idx):
        def scatter(A, mode):
            t, ib, vb = A.table("table", table), A.data("idx", idx), A.data("val", gval)
            return A.call("ge_scatter_add_rows", t.ptr, N, d, ib.ptr, vb.ptr, R, S())

        def verify(A):
            exp = t64.copy()
            np.add.at(exp, idx[idx >= 0], gval[idx >= 0].astype(np.float64))
            after = A["table"].get(F32, (N, d))
            near(2, np.abs(after - exp), 1e-5, strict=True)
            unnamed_rows_unchanged(table, after, idx)
        return scatter, verify
    drive(*scatter_case(gidx))                          # distinct rows: bitwise
    dup = gidx.copy()
    dup[live[:8]] = 3                                   # DELIBERATELY float-atomic: eight slots on row 3 meet in scheduler
    dup[live[-1]] = N - 1                               # order, so the two runs are compared within the existing 1e-5
                                                        # (eight unit-scale addends, as few as that test's own duplicates)

    def close(o0, o1):
        a, b = o0["table"].view(F32), o1["table"].view(F32)
        assert np.abs(a.astype(np.float64) - b).max() < 1e-5
    if B > 1:
        drive(*scatter_case(dup), compare=close)
    claimed(test_gradients_and_single_steps)


def pairs_of(E, R, B, seed):
    """(pos, neg): random ids that name entity 0 and E - 1 and relation 0 and R - 1; neg keeps the relation."""
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, R, B)], 1).astype(I32)
    pos[0] = (0, E - 1, R - 1)
    neg = pos.copy()
    side = rng.integers(0, 2, B)
    neg[np.arange(B), side] = rng.integers(0, E, B)
    if B > 1:
        pos[1, 2] = neg[1, 2] = 0
    return pos, neg


@guards("ge_transx_hinge_step", "ge_transr_adam_step")
@pytest.mark.parametrize("B", [1, 65, 257])
def test_translation_single_steps(B):
    """Bounds: 5e-6 (test_gpu_transx.py _check_step); TransR's m, v and x as test_twenty_dependent_adam_steps bounds them."""
    E, R, lr, margin = 300, 9, 0.01, 1.0
    pos, neg = pairs_of(E, R, B, seed=B)
    lib = _lib.load()
    for model in XMODELS:
        for d in (50, 200):
            tabs = xtabs(model, E, R, d, seed=d + B)
            need = lib.ge_transx_step_workspace_bytes(E, R, d, B)
            assert need > 0

            def case(A, mode):
                a = xargs(A, model, True, tabs, "table")
                p, n = A.data("pos", pos), A.data("neg", neg)
                loss, w = A.out("loss", 4), A.ws("workspace", need)
                return A.call("ge_transx_hinge_step", *a, p.ptr, n.ptr, B, margin, lr, loss.ptr, *ws_args(w, mode), S())

            def verify(A):
                new, rloss = XR.sgd_step(model, f64(tabs), pos, neg, lr, margin, True)
                near(2, abs(float(A["loss"].get(F32)[0]) - rloss), 5e-6 * max(1.0, abs(rloss)))
                for k in tabs:
                    after = A[k].get(F32, tabs[k].shape)
                    near(2, np.abs(after - new[k]), 5e-6)
                    named = (pos[:, :2], neg[:, :2]) if tabs[k].shape[0] == E else (pos[:, 2],)
                    unnamed_rows_unchanged(tabs[k], after, *named)
            drive(case, verify, ws=True)
    b1, b2, eps, alr = 0.9, 0.999, 1e-8, 0.01
    for dim_e, dim_r in ((7, 33), (64, 64)):
        tabs = rtabs(E, R, dim_e, dim_r, seed=dim_e + B)
        n_mom = sum(v.size for v in tabs.values())
        need = lib.ge_transr_step_workspace_bytes(E, R, dim_e, dim_r, B)
        assert need > 0

        def case(A, mode):
            a = rargs(A, False, tabs, "table")
            m, v = A.table("m", np.zeros(n_mom, F32)), A.table("v", np.zeros(n_mom, F32))
            p, n = A.data("pos", pos), A.data("neg", neg)
            loss, w = A.out("loss", 4), A.ws("workspace", need)
            return A.call("ge_transr_adam_step", *a, m.ptr, v.ptr, p.ptr, n.ptr, B, margin, alr, b1, b2, eps, 1, loss.ptr,
                          *ws_args(w, mode), S())

        def verify(A):
            t64_ = f64(tabs)
            rloss, g = RR.hinge_grads(t64_, pos, neg, margin, False)
            _, mag = RR.hinge_grads(t64_, pos, neg, margin, False, magnitude=True)
            # the batch loss: each D within test_score_matches_fp64's bound, summed over the 2B distances
            ltol = sum(4.0 * (dim_e + dim_r + 8) * F32_EPS * RR.score_magnitude(t64_, t, False).sum() for t in (pos, neg))
            near(2, abs(float(A["loss"].get(F32)[0]) - rloss), ltol + 2 * B * F32_EPS * abs(rloss))
            a = RR.lr_t(*(float(np.float32(x)) for x in (alr, b1, b2)), 1)
            m_all, v_all, off = A["m"].get(F32).astype(np.float64), A["v"].get(F32).astype(np.float64), 0
            for k in RR.TABLES:
                n = tabs[k].size
                m1, v1 = m_all[off:off + n].reshape(tabs[k].shape), v_all[off:off + n].reshape(tabs[k].shape)
                off += n
                tol_g = (dim_e + dim_r + 2 * len(pos)) * 2 * F32_EPS * mag[k]
                mref, vref = (1 - np.float32(b1)) * g[k], (1 - np.float32(b2)) * g[k] ** 2
                near(2, np.abs(m1 - mref), 0.1 * tol_g + 4 * F32_EPS * np.abs(g[k]))
                near(2, np.abs(v1 - vref), 0.001 * (2 * np.abs(g[k]) + tol_g) * tol_g + 4 * F32_EPS * g[k] ** 2)
                xref = t64_[k] - a * m1 / (np.sqrt(v1) + eps)
                upd = a * np.abs(m1) / (np.sqrt(v1) + eps)
                near(2, np.abs(A[k].get(F32, tabs[k].shape) - xref), 4 * F32_EPS * (np.abs(xref) + upd))
        drive(case, verify, ws=True)
    claimed(test_translation_single_steps)


# =============================================================== 3. samplers and transforms
@guards("ge_corrupt_batch", "ge_bernoulli_corrupt_batch", "ge_transx_draw_batch")
@pytest.mark.parametrize("B", [1, 65])
def test_samplers(B):
    """Exact against the C port / the pinned Bernoulli oracle (test_corrupt_batch_bit_exact,
    test_bernoulli_sampler_bit_exact_vs_pinned_oracle, test_loop_equals_single_steps_and_draws_match)."""
    N, n_rel = 120, 8
    id_to_type, offsets, ids = types_of(N, n_rel)
    rng = np.random.default_rng(B)
    pos = np.stack([rng.integers(n_rel, N, B), rng.integers(n_rel, N, B), rng.integers(0, n_rel, B)], 1).astype(I32)
    for mode_ in range(4):
        for padded in (0, 16):
            def case(A, mode):
                p, it, to, ti = A.data("pos", pos), A.data("id_to_type", id_to_type), A.data("off", offsets), A.data("ids", ids)
                neg = A.out("neg", 12 * B)
                return A.call("ge_corrupt_batch", p.ptr, B, it.ptr, N, to.ptr, len(offsets) - 1, ti.ptr, 7, 3, padded,
                              mode_, neg.ptr, S())

            def verify(A):
                assert np.array_equal(A["neg"].get(I32, (B, 3)), CO.corrupt_batch(pos, id_to_type, offsets, ids, 7, 3, padded, mode_))
            drive(case, verify)
    E, R = 65, 5
    known = np.unique(np.stack([rng.integers(0, E, 400), rng.integers(0, E, 400), rng.integers(0, R, 400)], 1), axis=0)
    idx = TO.BernoulliIndex(known, 0, E, R)
    bpos = known[rng.integers(0, len(known), B)].astype(I32)

    def index_args(A):
        return (A.data("bh_key", idx.bh_key).ptr, A.data("bh_ent", idx.bh_ent).ptr, A.data("bt_key", idx.bt_key).ptr,
                A.data("bt_ent", idx.bt_ent).ptr, len(known), A.data("thr", idx.tail_threshold).ptr)

    def bern(A, mode):
        p, neg = A.data("pos", bpos), A.out("neg", 12 * B)
        return A.call("ge_bernoulli_corrupt_batch", p.ptr, B, *index_args(A), R, 0, E, 11, 5, neg.ptr, S())

    def verify_bern(A):
        assert np.array_equal(A["neg"].get(I32, (B, 3)), TO.bernoulli_corrupt_batch(bpos, idx, 11, 5))
    drive(bern, verify_bern)
    tri = known.astype(I32)

    def draw(A, mode):
        t, p, n = A.data("triples", tri), A.out("pos", 12 * B), A.out("neg", 12 * B)
        return A.call("ge_transx_draw_batch", t.ptr, len(tri), B, *index_args(A), R, E, 11, 6, p.ptr, n.ptr, S())

    def verify_draw(A):
        p_ = tri[XR.draw_positive_rows(len(tri), B, 11, 6)]
        assert np.array_equal(A["pos"].get(I32, (B, 3)), p_)
        assert np.array_equal(A["neg"].get(I32, (B, 3)), TO.bernoulli_corrupt_batch(p_, idx, 11, 6))
    drive(draw, verify_draw)
    claimed(test_samplers)


@guards("ge_hole_to_spectral", "ge_hole_from_spectral")
@pytest.mark.parametrize("N", [1, 65])
@pytest.mark.parametrize("d", [2, 50, 200])
def test_spectral_transforms_in_place(N, d):
    """Bound: 2e-6 max(1, |ref|) each way (test_hole_spectral_transform_round_trip)."""
    x = np.random.default_rng(N + d).standard_normal((N, d)).astype(F32)
    ref = to_spectral(x)

    def fwd(A, mode):
        t = A.table("table", x)
        return A.call("ge_hole_to_spectral", t.ptr, N, d, S())

    def verify_fwd(A):
        near(3, np.abs(A["table"].get(F32, (N, d)) - ref), 2e-6 * max(1.0, np.abs(ref).max()), strict=True)
    A = drive(fwd, verify_fwd)
    spec = A["table"].get(F32, (N, d))

    def inv(A, mode):
        t = A.table("table", spec)
        return A.call("ge_hole_from_spectral", t.ptr, N, d, S())

    def verify_inv(A):
        near(3, np.abs(A["table"].get(F32, (N, d)) - x), 2e-6 * max(1.0, np.abs(x).max()), strict=True)
    drive(inv, verify_inv)
    claimed(test_spectral_transforms_in_place)


# =============================================================== 4. candidate sweeps (ComplEx / spectral HolE)
def known_index(kn, n_rows, side):
    """evaluate.KnownIndex on the host: (key = fixed * n_rows + second ascending, ent) int64, duplicates removed."""
    kn = np.asarray(kn, dtype=I64).reshape(-1, 3)
    if side == "relation":
        fixed, second, other = kn[:, 0], kn[:, 1], kn[:, 2]
    else:
        fixed, other = (kn[:, 0], kn[:, 1]) if side == "tail" else (kn[:, 1], kn[:, 0])
        second = kn[:, 2]
    packed = np.unique((fixed * n_rows + second) * n_rows + other)
    return (packed // n_rows).astype(I64), (packed % n_rows).astype(I64)


def sort_cells(off, rc):
    """The cells of every tile in ascending order (the header leaves the order inside a tile open)."""
    rc = rc.copy()
    for t in range(len(off) - 1):
        rc[off[t]:off[t + 1]] = np.sort(rc[off[t]:off[t + 1]])
    return rc


def guarded_known_cells(kn, n_rows, side, fixed, rel, pos_of, n_cand, mask):
    """ge_known_cells, both passes, on buffers of exactly tiles / tiles + 1 / total entries; the cells against the
    [B, n_cand] bool `mask` (exact, as test_known_cells_kernel_matches_brute_force).  Returns (known_off, known_rc)."""
    key, ent = known_index(kn, n_rows, side)
    B = len(fixed)
    n_ct = (n_cand + 127) // 128
    tiles = ((B + 127) // 128) * n_ct
    box = {}

    def case(A, mode):
        kb, eb = A.data("known_key", key), A.data("known_ent", ent)
        fb, rb, pb = A.data("fixed", fixed.astype(I64)), A.data("rel", rel.astype(I64)), A.data("pos_of", pos_of.astype(I64))
        scratch, off = A.ws("tile_scratch", 4 * tiles), A.out("known_off", 4 * (tiles + 1))
        args = (kb.ptr, eb.ptr, len(key), fb.ptr, rb.ptr, B, pb.ptr, n_rows, n_cand, scratch.ptr, off.ptr)
        rc = A.call("ge_known_cells", 0, *args, None, S())
        if rc:
            return rc
        torch.cuda.synchronize()
        total = int(off.get(I32)[-1])
        assert 0 <= total <= int(mask.sum())
        cells = A.out("known_rc", 2 * total)
        return A.call("ge_known_cells", 1, *args, cells.ptr, S()) if total else 0

    def canon(A):
        off = A["known_off"].get(I32)
        return {"known_off": off, "known_rc": sort_cells(off, A["known_rc"].get(U16))}

    def verify(A):
        c = canon(A)
        off, rc = c["known_off"], c["known_rc"]
        got = set()
        for t in range(tiles):
            for v in rc[off[t]:off[t + 1]].astype(I64):
                got.add(((t // n_ct) * 128 + int(v) // 128, (t % n_ct) * 128 + int(v) % 128))
        assert off[0] == 0 and got == {(int(i), int(j)) for i, j in np.argwhere(mask)} and off[-1] == len(got)
        box["off"], box["rc"] = off, rc
    drive(case, verify, canon=canon)
    return box["off"], box["rc"]


def sweep_reference(table, hr, cand, head, spectral, real):
    """[B, K] fp64 losses of the oracle: ComplEx on `table`, or HolE on the real-valued table `real`."""
    B, K = len(hr), len(cand)
    fixed, rel, c = np.repeat(hr[:, 0], K), np.repeat(hr[:, 1], K), np.tile(cand, B)
    tr = np.stack([c, fixed, rel], 1) if head else np.stack([fixed, c, rel], 1)
    if spectral:
        return O.hole_evaluate_triples(tr, real.astype(np.float64))[:, 0].reshape(B, K)
    return O.evaluate_triples(tr, table.astype(np.float64))[:, 0].reshape(B, K)


def implied_counts(sc, cand, ref_loss, ref_id, mask):
    before = (sc < ref_loss[:, None]) | ((sc == ref_loss[:, None]) & (cand[None, :] < ref_id[:, None]))
    return before.sum(1).astype(I32), (before & mask).sum(1).astype(I32)


@guards("ge_complex_score_1vK", "ge_complex_rank_1vK", "ge_rank_1vK", "ge_rank_planes", "ge_rank_1vK_planes",
        "ge_rank_1vK_vs_loss", "ge_topk_1vK_planes", "ge_known_cells")
@pytest.mark.parametrize("B,K", [(1, 1), (127, 63), (128, 64), (129, 65), (5, 257)])
@pytest.mark.parametrize("d", [40, 56, 64])
def test_candidate_sweeps(B, K, d):
    """d = 40 / 56 / 64 select the generic, fp32-pipeline and f16 kernels.  Bounds: losses within 1e-5 of the fp64 oracle;
    counts, true_loss and the top-k lists exact against the sweep's own stored losses
    (test_gpu_train_eval.py test_gpu_ranks_equal_reference_heap_semantics, test_rank_sweep_small_and_ragged_shapes,
    test_hole_ranks_from_the_spectral_sweep; test_gpu_topk.py test_gpu_topk_equals_heap_over_sweep_losses)."""
    lib = _lib.load()
    N, R = 300, 10
    rng = np.random.default_rng(1000 * B + K + d)
    real = (rng.standard_normal((N, d)) * 0.25).astype(F32)
    real[50], real[60] = real[51], real[61]                 # exact ties between candidates
    cand = np.concatenate([[50, 51, 60, 61], rng.permutation(np.setdiff1d(np.arange(R, N), [50, 51, 60, 61]))])[:K]
    cand = rng.permutation(cand).astype(I32)
    hr = np.stack([rng.integers(R, N, B), rng.integers(0, R, B)], 1).astype(I32)
    tid = cand[rng.integers(0, K, B)].astype(I32)
    head = (B + d // 8) % 2
    side = "head" if head else "tail"
    rows = np.repeat(np.arange(B), 4)
    kn = np.stack([hr[rows, 0], rng.choice(cand, rows.size), hr[rows, 1]], 1).astype(I64)
    if head:
        kn = kn[:, [1, 0, 2]]
    pos_of = np.full(N, -1, I64)
    pos_of[cand] = np.arange(K)
    ks = set(map(tuple, kn.tolist()))
    mask = np.array([[((int(c), int(f), int(r)) if head else (int(f), int(c), int(r))) in ks for c in cand] for f, r in hr], bool)
    koff, krc = guarded_known_cells(kn, N, side, hr[:, 0], hr[:, 1], pos_of, K, mask)
    tiles = ((B + 127) // 128) * ((K + 127) // 128)
    assert len(koff) == tiles + 1
    col = pos_of[tid]

    def score_1vk(A, mode):
        t, h, c = A.data("table", real), A.data("hr", hr), A.data("cand", cand)
        out = A.out("out", 4 * B * K)
        return A.call("ge_complex_score_1vK", t.ptr, N, d, h.ptr, B, c.ptr, K, 1.0, 1, head, out.ptr, S())

    def verify_1vk(A):
        near(4, np.abs(A["out"].get(F32, (B, K)) - sweep_reference(real, hr, cand, head, False, real)), SCORE_TOL, strict=True)
    drive(score_1vk, verify_1vk)

    for model in (0, 2):
        table = to_spectral(real).astype(F32) if model == 2 else real
        ref = sweep_reference(table, hr, cand, head, model == 2, real)
        pbytes = int(lib.ge_rank_planes_bytes(N, d, K))
        assert (pbytes > 0) == (d >= 56)
        state = {}

        def rank_case(entry, filtered, planes):
            def case(A, mode):
                t, h, ti, c = A.data("table", table), A.data("hr", hr), A.data("true_id", tid), A.data("cand", cand)
                ko = A.data("known_off", koff).ptr if filtered else None
                kr = A.data("known_rc", krc).ptr if filtered else None
                nb, nk = A.out("n_before", 4 * B), A.out("n_known_before", 4 * B)
                tl, sc = A.out("true_loss", 4 * B), A.out("scores_out", 4 * B * K)
                pl = ()
                if planes:
                    p = A.ws("planes", pbytes)
                    rc = A.call("ge_rank_planes", t.ptr, N, d, c.ptr, K, 1.0, model, p.ptr, S())
                    assert rc == 0
                    p.kind = "in"
                    pl = (p.ptr,)
                m = () if entry == "ge_complex_rank_1vK" else (model,)
                return A.call(entry, t.ptr, N, d, h.ptr, B, ti.ptr, c.ptr, K, 1.0, *m, head, ko, kr, nb.ptr, nk.ptr,
                              tl.ptr, sc.ptr, *pl, S())

            def verify(A):
                sc, tl = A["scores_out"].get(F32, (B, K)), A["true_loss"].get(F32)
                near(4, np.abs(sc - ref), 1e-5, strict=True)
                assert np.array_equal(tl.view(I32), sc[np.arange(B), col].view(I32))
                enb, enk = implied_counts(sc, cand, tl, tid, mask)
                assert np.array_equal(A["n_before"].get(I32), enb)
                assert np.array_equal(A["n_known_before"].get(I32), enk if filtered else np.zeros(B, I32))
                state["sc"], state["tl"] = sc, tl
            return case, verify

        if model == 0:
            drive(*rank_case("ge_complex_rank_1vK", False, False))
        drive(*rank_case("ge_rank_1vK", True, False))
        if pbytes:
            def planes_case(A, mode):
                t, c, p = A.data("table", table), A.data("cand", cand), A.out("planes", pbytes)
                return A.call("ge_rank_planes", t.ptr, N, d, c.ptr, K, 1.0, model, p.ptr if mode != "offset" else p.ptr + 16, S())
            # include/ge_hip.h: the planes are opaque and the padding of their tiles is undefined (never written, never
            # read into a result).  (c) holds them through what the sweeps below compute from planes built in poisoned
            # buffers, not bit for bit.
            drive(planes_case, compare=lambda o0, o1: None)
            A = AG.Arena("ge_rank_planes", 0xFF)
            assert planes_case(A, "offset") == EINVAL       # (no size is passed: only the alignment can be refused)
            A.assert_intact()
            A.assert_outputs_poison()
            drive(*rank_case("ge_rank_1vK_planes", True, True))
            drive(*rank_case("ge_rank_1vK_planes", False, True))
        sc, tl = state["sc"], state["tl"]

        for filtered in (True, False):
            def vs_loss(A, mode, filtered=filtered):
                t, h, c = A.data("table", table), A.data("hr", hr), A.data("cand", cand)
                ri, rl = A.data("ref_id", tid), A.data("ref_loss", tl)
                ko = A.data("known_off", koff).ptr if filtered else None
                kr = A.data("known_rc", krc).ptr if filtered else None
                nb, nk = A.out("n_before", 4 * B), A.out("n_known_before", 4 * B)
                return A.call("ge_rank_1vK_vs_loss", t.ptr, N, d, h.ptr, B, ri.ptr, rl.ptr, c.ptr, K, 1.0, model, head, ko,
                              kr, nb.ptr, nk.ptr, None, S())

            def verify_vs(A, filtered=filtered):
                enb, enk = implied_counts(sc, cand, tl, tid, mask)
                assert np.array_equal(A["n_before"].get(I32), enb)
                assert np.array_equal(A["n_known_before"].get(I32), enk if filtered else np.zeros(B, I32))
            drive(vs_loss, verify_vs)

        if not pbytes:
            continue
        for k in (1, 128):                                  # 128 > K for every K here but 257
            need = int(lib.ge_topk_workspace_bytes(B, K, k))
            assert need > 0
            for filtered, with_planes in ((True, True), (False, False)):
                def topk(A, mode, filtered=filtered, with_planes=with_planes):
                    t, h, c = A.data("table", table), A.data("hr", hr), A.data("cand", cand)
                    ko = A.data("known_off", koff).ptr if filtered else None
                    kr = A.data("known_rc", krc).ptr if filtered else None
                    oid, ol, w = A.out("out_id", 4 * B * k), A.out("out_loss", 4 * B * k), A.ws("workspace", need)
                    pl = None
                    if with_planes:
                        p = A.ws("planes", pbytes)
                        assert A.call("ge_rank_planes", t.ptr, N, d, c.ptr, K, 1.0, model, p.ptr, S()) == 0
                        p.kind, pl = "in", p.ptr
                    return A.call("ge_topk_1vK_planes", t.ptr, N, d, h.ptr, B, c.ptr, K, 1.0, model, head, ko, kr, k,
                                  oid.ptr, ol.ptr, pl, *ws_args(w, mode), S())

                def verify_topk(A, filtered=filtered):
                    eid, el = TK.first_k_rows(sc, cand, k, mask if filtered else None)
                    assert np.array_equal(A["out_id"].get(I32, (B, k)), eid)
                    assert np.array_equal(A["out_loss"].get(F32, (B, k)).view(I32), el.view(I32))
                drive(topk, verify_topk, ws=True)
    if d >= 56:                                             # (d = 40 has no split-precision sweep: no planes, no top-k)
        claimed(test_candidate_sweeps)


# =============================================================== 5. translation sweeps
def cells_from_mask(mask):
    """ge_known_cells' lists of a [B, n_cand] bool mask (pos_of = the identity): (known_off int32, known_rc uint16)."""
    B, K = mask.shape
    n_rt, n_ct = (B + 127) // 128, (K + 127) // 128
    off, rc = [0], []
    for rt in range(n_rt):
        for ct in range(n_ct):
            r, c = np.nonzero(mask[rt * 128:(rt + 1) * 128, ct * 128:(ct + 1) * 128])
            rc.append(((r << 7) | c).astype(U16))
            off.append(off[-1] + len(r))
    rc = np.concatenate(rc) if rc else np.zeros(0, U16)
    return np.asarray(off, I32), (rc if len(rc) else np.zeros(1, U16))


def model_tabs(model, E, R, seed):
    return rtabs(E, R, 8, 12, seed) if model == "transr" else xtabs(model, E, R, 16, seed)


def model_args(A, model, l1, tabs, shift=0):
    return rargs(A, l1, tabs, shift=shift) if model == "transr" else xargs(A, model, l1, tabs, shift=shift)


def model_ws(kind, model, tabs, B, *extra):
    lib = _lib.load()
    E, R = tabs["ent"].shape[0], tabs["rel"].shape[0]
    if model == "transr":
        return int(getattr(lib, "ge_transr_%s_workspace_bytes" % kind)(E, R, *RR.dims(tabs), B, *extra))
    return int(getattr(lib, "ge_transx_%s_workspace_bytes" % kind)(XMODELS.index(model), E, R, tabs["ent"].shape[1], B, *extra))


def sweep_tol(tabs, l1):
    """(2 d + 8) 2^-24, x 2 for the squares, 2 d = entity width + distance width
    (test_gpu_translation_rank.py test_random_tables_within_bound_and_self_consistent, test_gpu_relation_rank.py _tol)."""
    return (tabs["ent"].shape[1] + tabs["rel"].shape[1] + 8) * RK.U * (1 if l1 else 2)


def check_rank_outputs(A, D, M, tol, target, mask, filtered, state, with_scores):
    """Counts inside count_bounds of the fp64 distances and equal to those implied by the stored distances; true_dist
    bitwise the stored distance of the target."""
    n = len(D)
    nb, nk, td = A["n_before"].get(I32), A["n_known_before"].get(I32), A["true_dist"].get(F32)
    lo, hi = RK.count_bounds(D, M, target, tol)
    assert np.all(lo <= nb) and np.all(nb <= hi)
    if with_scores:
        sc = A["scores_out"].get(F32, D.shape)
        near(5, np.abs(sc - D), tol * M)
        state["sc"] = sc
    sc = state["sc"]                                    # (a run without scores_out is held to the stored run's values)
    assert np.array_equal(td.view(I32), sc[np.arange(n), target].view(I32))
    snb, snk = RK.counts(sc.astype(np.float64), target, mask)
    assert np.array_equal(nb, snb) and np.array_equal(nk, snk if filtered else np.zeros(n, I64))


@guards("ge_transx_rank", "ge_transx_topk", "ge_transx_relation_rank", "ge_transr_rank", "ge_transr_topk",
        "ge_transr_relation_rank")
@pytest.mark.parametrize("model", XMODELS + ("transr",))
@pytest.mark.parametrize("B", [15, 16, 17])
def test_translation_sweeps(model, B):
    """B around the sweeps' 16 rows per workgroup; n_ent around the 256 candidates of a workgroup.  Bounds: sweep_tol
    for the distances and count_bounds for the counts, the rest exact (test_gpu_translation_rank.py,
    test_gpu_relation_rank.py); the top-k lists bitwise the (D, id) sort of the rank sweep's stored distances
    (test_gpu_translation_topk.py test_random_tables_bitwise_and_filtered_rank)."""
    pre = "ge_transr" if model == "transr" else "ge_transx"
    for E, R, shift in ((255, 1, 0), (256, 9, 0), (257, 9, 0), (257, 1, 0), (255, 9, 0), (256, 1, 0), (257, 9, 4)):
        rng = np.random.default_rng(E * 10 + R + B)
        l1 = bool((E + R) % 2)
        head = (E + B) % 2
        side = "head" if head else "tail"
        tabs = model_tabs(model, E, R, seed=E + R)
        t64_ = f64(tabs)
        tol = sweep_tol(tabs, l1)
        test = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, R, B)], 1).astype(I32)
        test[0, :2] = (0, E - 1)
        test[B - 1, :2] = (E - 1, 0)
        fixed = test[:, 1] if head else test[:, 0]
        target = RK.true_ids(test, side)
        mask = rng.random((B, E)) < 0.05                    # known cells of each row (a row's own list)
        koff, krc = cells_from_mask(mask)
        D = RK.distances(model, t64_, test, side, l1)
        M = RK.distances(model, t64_, test, side, l1, magnitude=True)
        state = {}
        for with_scores, filtered in ((True, True), (False, False)):
            need = model_ws("rank", model, tabs, B)
            assert need > 0

            def rank(A, mode):
                a = model_args(A, model, l1, tabs, shift)
                tb = A.data("triples", test)
                ko = A.data("known_off", koff).ptr if filtered else None
                kr = A.data("known_rc", krc).ptr if filtered else None
                nb, nk, td = A.out("n_before", 4 * B), A.out("n_known_before", 4 * B), A.out("true_dist", 4 * B)
                sc = A.out("scores_out", 4 * B * E).ptr if with_scores else None
                w = A.ws("workspace", need)
                return A.call(pre + "_rank", *a, tb.ptr, B, head, ko, kr, nb.ptr, nk.ptr, td.ptr, sc, *ws_args(w, mode), S())
            drive(rank, lambda A: check_rank_outputs(A, D, M, tol, target, mask, filtered, state, with_scores), ws=True)
        queries = np.stack([fixed, test[:, 2]], 1).astype(I32)
        for k, filtered in ((1, True), (128, False), (128, True)):
            need = model_ws("topk", model, tabs, B, k)
            assert need > 0

            def topk(A, mode):
                a = model_args(A, model, l1, tabs, shift)
                qb = A.data("queries", queries)
                ko = A.data("known_off", koff).ptr if filtered else None
                kr = A.data("known_rc", krc).ptr if filtered else None
                oid, od, w = A.out("out_id", 4 * B * k), A.out("out_dist", 4 * B * k), A.ws("workspace", need)
                return A.call(pre + "_topk", *a, qb.ptr, B, head, ko, kr, k, oid.ptr, od.ptr, *ws_args(w, mode), S())

            def verify_topk(A):
                eid, ed = TK.first_k_rows(state["sc"], np.arange(E), k, mask if filtered else None)
                assert np.array_equal(A["out_id"].get(I32, (B, k)), eid)
                assert np.array_equal(A["out_dist"].get(F32, (B, k)).view(I32), ed.view(I32))
            drive(topk, verify_topk, ws=True)
        relation_rank_case(model, tabs, test, l1, rng, shift)
    missing = {n for n in test_translation_sweeps.guarded if n.startswith(pre + "_")} - CALLED
    assert not missing, "the test never called %s" % sorted(missing)


def relation_rank_case(model, tabs, test, l1, rng, shift=0, dense_known=True):
    """ge_*_relation_rank with scores_out given (filtered) and NULL (unfiltered) on `test`."""
    pre = "ge_transr" if model == "transr" else "ge_transx"
    B, E, R = len(test), tabs["ent"].shape[0], tabs["rel"].shape[0]
    tol = (tabs["ent"].shape[1] + tabs["rel"].shape[1] + 8) * RRK.U * (1 if l1 else 2)       # test_gpu_relation_rank.py _tol
    t64_ = f64(tabs)
    D = RRK.distances(model, t64_, test, l1)
    M = RRK.distances(model, t64_, test, l1, magnitude=True)
    # known relations per (h, t) pair, as bits: rows that share a pair share its list
    bits = rng.integers(0, 1 << R, E * E) & rng.integers(0, 1 << R, E * E)
    mask = ((bits[test[:, 0].astype(I64) * E + test[:, 1]][:, None] >> np.arange(R)[None, :]) & 1).astype(bool)
    koff, krc = cells_from_mask(mask)
    need = model_ws("relation_rank", model, tabs, B)
    assert need > 0
    state = {}
    for with_scores, filtered in ((True, True), (False, False)):
        def relrank(A, mode):
            a = model_args(A, model, l1, tabs, shift)
            tb = A.data("triples", test)
            ko = A.data("known_off", koff).ptr if filtered else None
            kr = A.data("known_rc", krc).ptr if filtered else None
            nb, nk, td = A.out("n_before", 4 * B), A.out("n_known_before", 4 * B), A.out("true_dist", 4 * B)
            sc = A.out("scores_out", 4 * B * R).ptr if with_scores else None
            w = A.ws("workspace", need)
            return A.call(pre + "_relation_rank", *a, tb.ptr, B, ko, kr, nb.ptr, nk.ptr, td.ptr, sc, *ws_args(w, mode), S())
        drive(relrank, lambda A: check_rank_outputs(A, D, M, tol, test[:, 2].astype(I64), mask, filtered, state, with_scores),
              ws=True)


@pytest.mark.parametrize("model", XMODELS + ("transr",))
@pytest.mark.parametrize("B", [65535, 65536, 65537])
def test_relation_rank_row_chunk(model, B):
    """One row below, at and above the relation rank's row chunk (65,536 rows at n_rel = 9: chunk_rows in
    ge_transx_relrank.hip)."""
    E, R = 50, 9
    rng = np.random.default_rng(B)
    tabs = model_tabs(model, E, R, seed=3)
    test = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, R, B)], 1).astype(I32)
    relation_rank_case(model, tabs, test, True, rng)


# =============================================================== 6. neighbours
@guards("ge_neighbor_planes", "ge_neighbor_dists", "ge_neighbor_topk")
@pytest.mark.parametrize("K", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("d", [1, 64, 65])
def test_neighbours(K, B, d):
    """Bounds: neighbors_ref.dist_bound per cell for the stored distances, the fused lists bitwise the (D, id) sort of
    them (test_gpu_neighbors.py test_stored_distances_within_the_per_cell_bound,
    test_fused_topk_equals_the_sorted_stored_distances)."""
    lib = _lib.load()
    N = 200
    rng = np.random.default_rng(100 * K + 10 * B + d)
    X = rng.standard_normal((N, d)).astype(F32)
    X[N - 3:] = X[:3]                                       # exact ties
    cand = np.concatenate([[0, N - 1], 1 + rng.permutation(N - 2)])[:K]
    cand = rng.permutation(cand).astype(I32)
    q = np.concatenate([cand[:B // 2 + 1], rng.integers(0, N, B)])[:B].astype(I32)      # inside and outside the list
    pbytes = int(lib.ge_neighbor_planes_bytes(K, d))
    assert pbytes > 0

    def planes_case(A, mode):
        t, c, p = A.data("table", X), A.data("cand", cand), A.out("planes", pbytes)
        return A.call("ge_neighbor_planes", t.ptr, N, d, c.ptr, K, p.ptr + (16 if mode == "offset" else 0), S())
    drive(planes_case)
    A = AG.Arena("ge_neighbor_planes", 0xFF)
    assert planes_case(A, "offset") == EINVAL               # (no size is passed: only the alignment can be refused)
    A.assert_intact()
    A.assert_outputs_poison()

    def built_planes(A, t, c):
        p = A.ws("planes", pbytes)
        assert A.call("ge_neighbor_planes", t.ptr, N, d, c.ptr, K, p.ptr, S()) == 0
        p.kind = "in"
        return p

    for metric, mname in ((0, "cosine"), (1, "euclidean")):
        state = {}

        def dists(A, mode):
            t, c, qb = A.data("table", X), A.data("cand", cand), A.data("queries", q)
            p, out = built_planes(A, t, c), A.out("out", 4 * B * K)
            return A.call("ge_neighbor_dists", t.ptr, N, d, qb.ptr, B, c.ptr, K, metric, p.ptr, out.ptr, S())

        def verify_dists(A):
            D = A["out"].get(F32, (B, K))
            err = np.abs(D.astype(np.float64) - NR.distances(X, q, cand, mname))
            assert np.isfinite(D).all() and (D >= 0).all() and not np.signbit(D).any()
            near(6, err, NR.dist_bound(X, q, cand, mname))
            state["D"] = D
        drive(dists, verify_dists)
        for k in (1, 128):
            need = int(lib.ge_neighbor_workspace_bytes(B, K, k))
            assert need > 0
            for excl in (1, 0):
                def topk(A, mode):
                    t, c, qb = A.data("table", X), A.data("cand", cand), A.data("queries", q)
                    p = built_planes(A, t, c)
                    oid, od, w = A.out("out_id", 4 * B * k), A.out("out_dist", 4 * B * k), A.ws("workspace", need)
                    return A.call("ge_neighbor_topk", t.ptr, N, d, qb.ptr, B, c.ptr, K, k, metric, excl, p.ptr, oid.ptr,
                                  od.ptr, *ws_args(w, mode), S())

                def verify_topk(A):
                    eid, ed = NR.topk_of(state["D"], q, cand, k, bool(excl))
                    assert np.array_equal(A["out_id"].get(I32, (B, k)), eid)
                    assert np.array_equal(A["out_dist"].get(F32, (B, k)).view(I32), ed.view(I32))
                drive(topk, verify_topk, ws=True)
    claimed(test_neighbours)


# =============================================================== 7. native loops and the planner
N_LOOP, NREL_LOOP, D_LOOP, STEPS = 3000, 600, 8, 3


def balanced_triples(T, N=N_LOOP, n_rel=NREL_LOOP, a=7, b=11):
    """Triples whose every window of B <= 4100 consecutive rows names each relation row at most 7 times and each entity
    row at most twice as head and twice as tail (a, b coprime with the entity count): with the negatives of a step no
    row collects more than 16 gradient slots (checked per case by slots_per_row), so the prepared update runs no float
    atomics."""
    i = np.arange(T, dtype=I64)
    n_ent = N - n_rel
    assert np.gcd(a, n_ent) == 1 and np.gcd(b, n_ent) == 1
    return np.stack([n_rel + (i * a) % n_ent, n_rel + (i * b + 1) % n_ent, i % n_rel], 1).astype(I32)


def slots_per_row(pos, neg, N):
    """Gradient slots of one hinge step per table row: the positive's three rows and the negative's differing one."""
    rows = [pos.ravel()]
    diff = pos != neg
    rows.append(neg[diff])
    r = np.concatenate(rows)
    return np.bincount(r[(r >= 0) & (r < N)], minlength=N)


def loop_rows(first_row, T, B, n):
    out, row = [], first_row % T
    for _ in range(n):
        if row + B > T:
            row = 0
        out.append(row)
        row += B
    return out


def lr_at(lr0, gs, decay_steps, decay_rate):
    return float(np.float32(lr0) / (np.float32(1.0) + np.float32(decay_rate) * (np.float32(gs) / np.float32(decay_steps))))


def type_bufs(A, types):
    id_to_type, offsets, ids = types
    return (A.data("id_to_type", id_to_type).ptr, A.data("type_offsets", offsets).ptr, len(offsets) - 1,
            A.data("type_ids", ids).ptr)


def record_parts(rec, B, lay, n_steps, direct=True):
    """The words of prepared records that include/ge_hip.h defines, flattened (items and slot lists up to n_items)."""
    import prep_model as PM
    out = {}
    for s in range(n_steps):
        g = PM.parse_record(rec[s], B, lay)
        out["neg%d" % s] = g["neg"].copy()
        out["n_items%d" % s] = np.asarray(g["n_items"], I32)
        out["items%d" % s] = np.concatenate([x.ravel() for x in g["items"]])
        out["islots%d" % s] = np.concatenate([x.ravel() for x in g["islots"]])
        if direct:
            out["slot_item%d" % s] = g["slot_item"].copy()
    return out


def layout_of(B):
    import ctypes as C
    out = (C.c_int64 * 8)()
    assert _lib.load().ge_train_prepared_layout(B, out) == 0
    return tuple(int(v) for v in out)


LOOP_BS = [255, 256, 257, 4095, 4096, 4097]


@guards("ge_train_prepare_steps")
@pytest.mark.parametrize("B", LOOP_BS)
def test_prepare_steps(B):
    """Word for word against tests/prep_model.py and the C port's negatives (test_prepared_records_equal_numpy_model)."""
    import prep_model as PM
    lib = _lib.load()
    types = types_of(N_LOOP, NREL_LOOP)
    T, first_row, seed, gs0 = 2 * B + 50, 7, 99, 41
    tri = balanced_triples(T)
    tri[3, 0] = -3                                          # an invalid pair: no slots
    lay = layout_of(B)
    need = int(lib.ge_train_prepare_bytes(B, STEPS))
    assert need >= 4 * STEPS * lay[0]
    padded = 1024 if B < 1000 else 0

    def case(A, mode):
        trb = A.data("triples", tri)
        ty = type_bufs(A, types)
        out = A.out("out", need)
        nbytes = need - 1 if mode == "short" else need
        return A.call("ge_train_prepare_steps", trb.ptr, T, first_row, B, STEPS, ty[0], N_LOOP, *ty[1:], seed, gs0, padded,
                      1, 1, out.ptr, nbytes, S())

    def canon(A):
        rec = A["out"].get(I32)[:STEPS * lay[0]].reshape(STEPS, lay[0])
        return record_parts(rec, B, lay, STEPS)

    def verify(A):
        got = canon(A)
        for s, row in enumerate(loop_rows(first_row, T, B, STEPS)):
            pos = tri[row:row + B]
            neg = CO.corrupt_batch(pos, *types, seed, gs0 + s, padded, 1)
            exp = PM.expected_record(pos, neg, N_LOOP, True, lay)
            assert np.array_equal(got["neg%d" % s], neg), s
            assert got["n_items%d" % s].tolist() == exp["n_items"], s
            assert np.array_equal(got["items%d" % s], np.concatenate([x.ravel() for x in exp["items"]])), s
            assert np.array_equal(got["islots%d" % s], np.concatenate([x.ravel() for x in exp["islots"]])), s
            assert np.array_equal(got["slot_item%d" % s], exp["slot_item"]), s
    # `out` is an output with a size, not a workspace: the size is enforced, no alignment is asked of it
    drive(case, verify, ws=True, offset=False, canon=canon)
    claimed(test_prepare_steps)


@guards("ge_train_steps")
@pytest.mark.parametrize("B", LOOP_BS)
def test_train_steps(B):
    """Prepared and fallback workspace sizes, keep_all_losses 1 and 0, pipeline = NULL, against the C port replaying the
    loop: losses within 2e-5, the table within 1e-4, neg_ws exact (test_train_steps_match_c_port_step_by_step,
    test_train_steps_large_batch_and_fallback_branch)."""
    lib = _lib.load()
    types = types_of(N_LOOP, NREL_LOOP)
    d, T, first_row, seed, gs0 = D_LOOP, 2 * B + 50, 7, 21, 3
    margin, lr0, dsteps, drate = 0.2, 0.1, 50.0, 0.5
    tri = balanced_triples(T)
    table = table_of(N_LOOP, d, seed=B)
    padded = 1024 if B < 1000 else 0
    hinge_need, train_need = int(lib.ge_hinge_step_workspace_bytes(B, d)), int(lib.ge_train_workspace_bytes(B, d))
    assert 0 < hinge_need < train_need
    ctab, closs, negs = table.copy(), [], None
    for s, row in enumerate(loop_rows(first_row, T, B, STEPS)):
        pos = tri[row:row + B]
        negs = CO.corrupt_batch(pos, *types, seed, gs0 + s, padded, 0)
        assert slots_per_row(pos, negs, N_LOOP).max() <= 16, "the batch would take the float-atomic path"
        closs.append(CO.hinge_step(ctab, pos, negs, margin, lr_at(lr0, gs0 + s, dsteps, drate)))

    def case_of(need, keep):
        def case(A, mode):
            t, trb = A.table("table", table), A.data("triples", tri)
            ty = type_bufs(A, types)
            loss, ng, w = A.out("loss", 4 * B * (STEPS if keep else 1)), A.out("neg_ws", 12 * B), A.ws("workspace", need)
            # (d): below ge_hinge_step_workspace_bytes the loop must refuse (above it, it falls back)
            wp, wb = (w.ptr, hinge_need - 1) if mode == "short" else ws_args(w, mode)
            return A.call("ge_train_steps", t.ptr, N_LOOP, d, trb.ptr, T, first_row, B, STEPS, ty[0], *ty[1:], seed, gs0,
                          padded, 0, margin, lr0, dsteps, drate, 1.0, 0, loss.ptr, keep, ng.ptr, wp, wb, None, 0, None, S())

        def verify(A):
            loss = A["loss"].get(F32, (-1, B))
            for s in (range(STEPS) if keep else [STEPS - 1]):
                near(7, np.abs(loss[s if keep else 0] - closs[s]), 2e-5, strict=True)
            near(7, np.abs(A["table"].get(F32, (N_LOOP, d)) - ctab), 1e-4, strict=True)
            assert np.array_equal(A["neg_ws"].get(I32, (B, 3)), negs)
        return case, verify

    drive(*case_of(train_need, 1), ws=True)
    drive(*case_of(train_need, 0))

    def close(o0, o1):
        # DELIBERATELY the fallback branch (per-step sampler + float-atomic scatter): the two runs are compared within the
        # bounds test_train_steps_large_batch_and_fallback_branch holds that branch to
        assert np.array_equal(o0["neg_ws"], o1["neg_ws"])
        assert np.abs(o0["loss"].view(F32).astype(np.float64) - o1["loss"].view(F32)).max() < 2e-5
        assert np.abs(o0["table"].view(F32).astype(np.float64) - o1["table"].view(F32)).max() < 1e-4
    drive(*case_of(hinge_need, 1), ws=True, compare=close)
    claimed(test_train_steps)


@guards("ge_train_steps_logloss")
@pytest.mark.parametrize("B,K", [(255, 1), (256, 3), (257, 3), (1023, 3), (1024, 3), (1025, 3)])
def test_train_steps_logloss(B, K):
    """(1 + K) B = 4092 / 4096 / 4100 triples: where a second sort tile begins.  Against the fp64 oracle: losses within
    3e-5 max(1, |loss|), the table within 2e-5, neg_ws exact
    (test_native_logloss_loop_matches_oracle_over_twenty_dependent_steps)."""
    lib = _lib.load()
    types = types_of(N_LOOP, NREL_LOOP)
    d, T, first_row, seed, gs0 = D_LOOP, 2 * B + 50, 7, 77, 5
    l2, lr0, dsteps, drate = 3e-5, 0.05, 40.0, 0.5
    tri = balanced_triples(T)
    table = table_of(N_LOOP, d, seed=B + K)
    M = (1 + K) * B
    need = int(lib.ge_train_logloss_workspace_bytes(B, K, d))
    assert need > 0
    t64, oloss, negs = table.astype(np.float64), [], None
    for s, row in enumerate(loop_rows(first_row, T, B, STEPS)):
        pos = tri[row:row + B]
        gs = gs0 + s
        negs = np.stack([CO.corrupt_batch(pos, *types, seed, gs * K + k, 0, 0) for k in range(K)])
        every = np.concatenate([pos] + list(negs)).ravel()
        assert np.bincount(every, minlength=N_LOOP).max() <= 16, "the batch would take the float-atomic path"
        t64, ol = O.logloss_step(t64, pos, negs, lr_at(lr0, gs, dsteps, drate), l2)
        oloss.append(ol)

    def case_of(keep):
        def case(A, mode):
            t, trb = A.table("table", table), A.data("triples", tri)
            ty = type_bufs(A, types)
            loss, ng = A.out("loss", 4 * M * (STEPS if keep else 1)), A.out("neg_ws", 12 * K * B)
            w = A.ws("workspace", need)
            return A.call("ge_train_steps_logloss", t.ptr, N_LOOP, d, trb.ptr, T, first_row, B, STEPS, ty[0], *ty[1:], seed,
                          gs0, 0, 0, K, l2, lr0, dsteps, drate, 1.0, loss.ptr, keep, ng.ptr, *ws_args(w, mode), None, S())

        def verify(A):
            loss = A["loss"].get(F32, (-1, M))
            for s in (range(STEPS) if keep else [STEPS - 1]):
                near(7, np.abs(loss[s if keep else 0] - oloss[s]), 3e-5 * max(1.0, np.abs(oloss[s]).max()), strict=True)
            near(7, np.abs(A["table"].get(F32, (N_LOOP, d)) - t64), 2e-5, strict=True)
            assert np.array_equal(A["neg_ws"].get(I32, (K, B, 3)), negs)
        return case, verify
    drive(*case_of(1), ws=True)
    drive(*case_of(0))
    claimed(test_train_steps_logloss)


def valid_rows(seed, counter, B, V):
    """The validation batch of a tick (the Philox draw test_validation_tick_matches_oracle_and_keeps_the_best_table states)."""
    i = np.arange(B, dtype=np.uint64)
    lo, hi = i & np.uint64(0xFFFFFFFF), i >> np.uint64(32)
    k0, k1 = (seed & 0xFFFFFFFF) ^ 0x7673656C, (seed >> 32) & 0xFFFFFFFF
    w0 = O.philox4x32_10(counter & 0xFFFFFFFF, counter >> 32, lo, hi, k0, k1)[0].astype(np.uint64)
    w1 = O.philox4x32_10(counter & 0xFFFFFFFF, counter >> 32, lo, hi ^ np.uint64(0x80000000), k0, k1)[0].astype(np.uint64)
    return (((w1 << np.uint64(32)) | w0) % np.uint64(V)).astype(I64)


@guards("ge_validation_tick", "ge_validation_tick_logloss")
@pytest.mark.parametrize("B", [255, 256, 257])
def test_validation_ticks(B):
    """With `pocket` given.  B around the 256-pair granule only: a tick scores its batch and takes a mean, it sorts
    nothing, so the 4095 / 4096 / 4097 group of the loops (a second sort tile) has no counterpart here.  The mean within 1e-5 (hinge) / 2e-6 relative (log-loss) of the oracle, best the mean's own
    bits, the pocket the table's (test_validation_tick_matches_oracle_and_keeps_the_best_table,
    test_logloss_validation_tick_matches_oracle)."""
    lib = _lib.load()
    types = types_of(N_LOOP, NREL_LOOP)
    d, V, seed, counter = D_LOOP, 1000, 0xABCDEF0123, 7
    valid = balanced_triples(V)
    table = table_of(N_LOOP, d, seed=B)
    t64 = table.astype(np.float64)
    pos = valid[valid_rows(seed, counter, B, V)]

    def tick(entry, need, head, expect, rel_tol):
        def case(A, mode):
            t, vb = A.data("table", table), A.data("valid", valid)
            ty = type_bufs(A, types)
            mean, best = A.out("mean_out", 4), A.table("best", np.array([2.0], F32))
            pocket, w = A.out("pocket", 4 * N_LOOP * d), A.ws("workspace", need)
            return A.call(entry, t.ptr, N_LOOP, d, vb.ptr, V, B, ty[0], *ty[1:], seed, counter, 1024, 0, *head,
                          *ws_args(w, mode), mean.ptr, best.ptr, pocket.ptr, S())

        def verify(A):
            mean = A["mean_out"].get(F32)
            near(7, abs(float(mean[0]) - expect), rel_tol, strict=True)
            assert np.array_equal(A["best"].get(I32), mean.view(I32))
            assert np.array_equal(A["pocket"].get(F32, (N_LOOP, d)).view(I32), table.view(I32))
        drive(case, verify, ws=True)

    neg = O.corrupt_batch(pos, *types, seed, counter, 1024, 0)
    tick("ge_validation_tick", int(lib.ge_validation_workspace_bytes(B)), (0.2, 1.0, 0),
         float(O.evaluate_batch(pos, neg, t64, 0.2).mean()), 1e-5)
    K, l2 = 3, 1e-4
    negs = [O.corrupt_batch(pos, *types, seed, counter * K + k, 1024, 0) for k in range(K)]
    exp = float(O.logloss_values(np.concatenate([pos] + negs, 0), np.concatenate([np.ones(B), -np.ones(K * B)]), t64, l2).mean())
    tick("ge_validation_tick_logloss", int(lib.ge_validation_logloss_workspace_bytes(B, K)), (K, l2, 1.0), exp, 2e-6 * exp)
    claimed(test_validation_ticks)


def loop_kg(E=3000, R=20, T=20000, seed=0):
    rng = np.random.default_rng(seed)
    tri = np.stack([rng.integers(0, E, T), rng.integers(0, E, T), rng.integers(0, R, T)], 1)
    return np.unique(tri, axis=0).astype(I64), E, R


@guards("ge_transx_train_steps", "ge_transr_train_steps")
@pytest.mark.parametrize("B", LOOP_BS)
def test_translation_train_steps(B):
    """TransE / TransH / TransD: every step's batch loss and the final tables within 5e-6 of the fp64 replay of the
    oracle's draws (test_gpu_transx.py test_twenty_dependent_steps, test_loop_equals_single_steps_and_draws_match).
    TransR: the loop equals ge_transr_adam_step on the same draws bit for bit (test_gpu_transr.py
    test_loop_equals_single_steps_and_draws_match); the single step is held to fp64 in test_translation_single_steps."""
    lib = _lib.load()
    tri, E, R = loop_kg()
    idx = TO.BernoulliIndex(tri, 0, E, R)
    tri32 = tri.astype(I32)
    seed, first, lr, margin = 21, 4, 0.01, 1.0
    draws = []
    for s in range(STEPS):
        p_ = tri32[XR.draw_positive_rows(len(tri), B, seed, first + s)]
        draws.append((p_, TO.bernoulli_corrupt_batch(p_, idx, seed, first + s)))

    def sampler_args(A):
        return (A.data("triples", tri32).ptr, len(tri), A.data("bh_key", idx.bh_key).ptr, A.data("bh_ent", idx.bh_ent).ptr,
                A.data("bt_key", idx.bt_key).ptr, A.data("bt_ent", idx.bt_ent).ptr, len(tri), A.data("thr", idx.tail_threshold).ptr)

    for model in XMODELS:
        tabs = xtabs(model, E, R, D_LOOP, seed=B)
        need = int(lib.ge_transx_step_workspace_bytes(E, R, D_LOOP, B))

        def case(A, mode):
            a = xargs(A, model, False, tabs, "table")
            losses, w = A.out("losses", 4 * STEPS), A.ws("workspace", need)
            return A.call("ge_transx_train_steps", *a, *sampler_args(A), seed, first, STEPS, B, margin, lr, losses.ptr,
                          *ws_args(w, mode), S())

        def verify(A):
            ref, losses = f64(tabs), A["losses"].get(F32)
            for s, (p_, n_) in enumerate(draws):
                ref, rloss = XR.sgd_step(model, ref, p_, n_, lr, margin, False)
                near(7, abs(float(losses[s]) - rloss), 5e-6 * max(1.0, abs(rloss)))
            for k in tabs:
                near(7, np.abs(A[k].get(F32, tabs[k].shape) - ref[k]), 5e-6)
        drive(case, verify, ws=True)

    tabs = rtabs(E, R, 8, 12, seed=B)
    n_mom = sum(v.size for v in tabs.values())
    need = int(lib.ge_transr_step_workspace_bytes(E, R, 8, 12, B))
    b1, b2, eps = 0.9, 0.999, 1e-8

    def rcase(A, mode):
        a = rargs(A, True, tabs, "table")
        m, v = A.table("m", np.zeros(n_mom, F32)), A.table("v", np.zeros(n_mom, F32))
        losses, w = A.out("losses", 4 * STEPS), A.ws("workspace", need)
        return A.call("ge_transr_train_steps", *a, m.ptr, v.ptr, *sampler_args(A), seed, first, STEPS, B, margin, lr, b1, b2,
                      eps, 1, losses.ptr, *ws_args(w, mode), S())

    def rverify(A):
        C = AG.Arena("ge_transr_adam_step", 0x00)
        a = rargs(C, True, tabs, "table")
        m, v = C.table("m", np.zeros(n_mom, F32)), C.table("v", np.zeros(n_mom, F32))
        loss, w = C.out("loss", 4), C.ws("workspace", need)
        for s, (p_, n_) in enumerate(draws):
            p, n = C.data("pos%d" % s, p_), C.data("neg%d" % s, n_)
            assert C.call("ge_transr_adam_step", *a, m.ptr, v.ptr, p.ptr, n.ptr, B, margin, lr, b1, b2, eps, 1 + s, loss.ptr,
                          w.ptr, need, S()) == 0
            assert np.array_equal(loss.get(I32), A["losses"].get(I32)[s:s + 1]), s
        C.assert_intact()
        for k in list(tabs) + ["m", "v"]:
            assert np.array_equal(A[k].get(I32), C[k].get(I32)), k
    drive(rcase, rverify, ws=True)
    claimed(test_translation_train_steps)


# =============================================================== 8. the row-sharded step: one process plays one rank of G = 3
G_SH, N_SH, NREL_SH, S_SH = 3, 3001, 600, 2          # N = 3k + 1: rank 0 holds R = 1001 rows, ranks 1 and 2 one fewer


def owner_tiles(words, cap):
    """(keys per tile, tiles) of an owner record of `words` words: tiles of { n_items, pad to 64 | items[P][2] | islots[P][16] }."""
    P = 16384                                            # kOwnerP in ge_shard.hip
    n_sub = (cap + P - 1) // P
    assert words == n_sub * (64 + 18 * P)
    return P, n_sub


@guards("ge_shard_plan", "ge_shard_grad", "ge_shard_apply", "ge_shard_owner_plan", "ge_shard_owner_apply")
@pytest.mark.parametrize("rank", [0, 2])
@pytest.mark.parametrize("B", [257, 4097])
def test_row_sharded_step(B, rank):
    """The plan word for word against tests/prep_model.py (test_shard_plan_equals_numpy_model); the steps against the C
    port on the full table: losses within 1e-5, rows within 2e-5 (test_gpu_sharded.py
    test_sharded_real_kernels_match_c_port).  grad_idx / grad_val travel from ge_shard_grad to ge_shard_apply: rows of
    empty and directly applied slots are undefined, so they are guarded but not compared between the poison runs."""
    import prep_model as PM
    lib = _lib.load()
    G, N, S_, d = G_SH, N_SH, S_SH, D_LOOP
    R = (N + G - 1) // G
    rows_local = (N - rank + G - 1) // G
    assert rows_local == (R if rank == 0 else R - 1)
    types = types_of(N, NREL_SH)
    tri = balanced_triples(S_ * B, N, NREL_SH, 5, 11)
    pos = tri.reshape(S_, B, 3).copy()
    neg = np.stack([CO.corrupt_batch(pos[s], *types, 4, s, 0, 0) for s in range(S_)])
    pos[1, 5, 0] = -3                                       # an invalid pair: no slots
    neg[0, 3] = pos[0, 3]                                   # negative == positive: no row of its own
    for s in range(S_):
        ok = (pos[s] >= 0).all(1)
        assert slots_per_row(pos[s][ok], neg[s][ok], N).max() <= 16, "a row would combine atomically"
    lay = layout_of(B)
    cap_req = 4 * lay[1] * lay[2]
    need = int(lib.ge_shard_plan_workspace_bytes(B, S_))
    assert need > 0
    exp = [PM.expected_shard_plan(pos[s], neg[s], N, G, rank, lay) for s in range(S_)]

    def plan_bufs(A, mode="exact"):
        p, n = A.data("pos", pos), A.data("neg", neg)
        rec, ps, ns = A.out("records", 4 * S_ * lay[0]), A.out("pos_src", 12 * S_ * B), A.out("neg_src", 4 * S_ * B)
        rq, cn, w = A.out("req_row", 4 * S_ * cap_req), A.out("counts", 4 * S_ * G), A.ws("workspace", need)
        return A.call("ge_shard_plan", p.ptr, n.ptr, S_, B, N, G, rank, rec.ptr, ps.ptr, ns.ptr, rq.ptr, cn.ptr,
                      *ws_args(w, mode), 0, S())

    def plan_canon(A):
        rec = A["records"].get(I32, (S_, lay[0]))
        out = record_parts(rec, B, lay, S_)
        for s in range(S_):
            del out["neg%d" % s]                            # (a shard record carries no negatives)
            out["req_row%d" % s] = A["req_row"].get(I32, (S_, cap_req))[s, :len(exp[s]["req_row"])]
        out.update(pos_src=A["pos_src"].get(I32), neg_src=A["neg_src"].get(I32), counts=A["counts"].get(I32))
        return out

    def plan_verify(A):
        got = plan_canon(A)
        for s in range(S_):
            assert np.array_equal(got["counts"].reshape(S_, G)[s], exp[s]["counts"]), s
            assert np.array_equal(got["req_row%d" % s], exp[s]["req_row"]), s
            assert np.array_equal(got["pos_src"].reshape(S_, B, 3)[s], exp[s]["pos_src"]), s
            assert np.array_equal(got["neg_src"].reshape(S_, B)[s], exp[s]["neg_src"]), s
            assert np.array_equal(got["slot_item%d" % s], exp[s]["slot_item"]), s
            assert got["n_items%d" % s].tolist() == exp[s]["n_items"], s
            assert np.array_equal(got["items%d" % s], np.concatenate([x.ravel() for x in exp[s]["items"]])), s
            assert np.array_equal(got["islots%d" % s], np.concatenate([x.ravel() for x in exp[s]["islots"]])), s
    drive(plan_bufs, plan_verify, ws=True, canon=plan_canon)

    # ---- the two steps: staged rows come from a full table that the test keeps as the other owners would
    table = table_of(N, d, seed=B + rank)
    margin, lr = 0.2, 0.1
    ctab, closs = table.copy(), []
    for s in range(S_):
        ok = (pos[s] >= 0).all(1)
        full = CO.hinge_step(ctab, np.where(ok[:, None], pos[s], 0), np.where(ok[:, None], neg[s], 0), margin, lr)
        closs.append((full, ok))                            # (the invalid pair scored as (0, 0, 0) vs itself: no gradient)

    def staged_ids(s):
        owners = [o for o in range(G) if o != rank]
        ids, at = [], 0
        for o in owners:
            c = int(exp[s]["counts"][o])
            ids.append(exp[s]["req_row"][at:at + c].astype(I64) * G + o)
            at += c
        return np.concatenate(ids)

    def steps(A, mode):
        assert plan_bufs(A) == 0
        for name in ("records", "pos_src", "neg_src", "req_row", "counts", "workspace"):
            A[name].kind = "in"
        cur = table.copy()
        shard = A.table("shard", cur[rank::G])
        assert shard.nbytes == 4 * rows_local * d
        rec_b, ps_b, ns_b = A["records"], A["pos_src"], A["neg_src"]
        for s in range(S_):
            ids = staged_ids(s)
            U = len(ids)
            staged = A.data("staged%d" % s, cur[ids])
            gsum = A.table("gsum%d" % s, np.zeros((U, d), F32))        # "must be zero beforehand"
            loss = A.out("loss%d" % s, 4 * B)
            gi, gv = A.ws("grad_idx%d" % s, 24 * B), A.ws("grad_val%d" % s, 24 * B * d)
            rc = A.call("ge_shard_grad", shard.ptr, rows_local, d, staged.ptr, U, ps_b.ptr + 12 * B * s, ns_b.ptr + 4 * B * s,
                        rec_b.ptr + 4 * lay[0] * s, B, N, G, margin, lr, 1.0, 0, loss.ptr, gi.ptr, gv.ptr, gsum.ptr, None, S())
            if rc:
                return rc
            rc = A.call("ge_shard_apply", shard.ptr, rows_local, d, rec_b.ptr + 4 * lay[0] * s, B, N, G, gi.ptr, gv.ptr,
                        gsum.ptr, S())
            if rc:
                return rc
            torch.cuda.synchronize()
            cur[rank::G] = shard.get(F32, (rows_local, d))
            cur[ids] += gsum.get(F32, (U, d))                           # what the owners would add
        A.final = cur
        return 0

    def steps_verify(A):
        for s in range(S_):
            full, ok = closs[s]
            near(8, np.abs(A["loss%d" % s].get(F32)[ok] - full[ok]), 1e-5, strict=True)
        near(8, np.abs(A.final - ctab), 2e-5, strict=True)
    drive(steps, steps_verify)

    # ---- owner side: the lists the two peers would send this rank for the same batches; step 1 asks for nothing
    lists = []
    for p_ in [o for o in range(G) if o != rank]:
        e = PM.expected_shard_plan(pos[0], neg[0], N, G, p_, lay)
        at = sum(int(e["counts"][o]) for o in range(rank) if o != p_)
        lists.append(e["req_row"][at:at + int(e["counts"][rank])].astype(I32))
    lists[0] = np.union1d(lists[0], [0, rows_local - 1]).astype(I32)       # the shard's first and last row
    req_all = np.concatenate(lists)
    cap = len(req_all)
    req_start = np.array([0, cap, cap], I64)                                # step 1: an empty request list
    words = int(lib.ge_shard_owner_record_words(cap))
    P_own, n_sub_own = owner_tiles(words, cap)
    oneed = int(lib.ge_shard_owner_workspace_bytes(cap, S_))
    assert words > 0 and oneed > 0
    recv = np.random.default_rng(B).standard_normal((cap, d)).astype(F32)
    shard0 = table[rank::G].copy()

    def owner(A, mode):
        ra, rs = A.data("req_all", req_all), A.data("req_start", req_start)
        rec, w = A.out("records", 4 * S_ * words), A.ws("workspace", oneed)
        rc = A.call("ge_shard_owner_plan", ra.ptr, rs.ptr, S_, cap, rows_local, rec.ptr, *ws_args(w, mode), S())
        if rc:
            return rc
        shard = A.table("shard", shard0)
        rv, none = A.data("recv", recv), A.data("recv_empty", np.zeros((0, d), F32))
        for s, r in ((0, rv), (1, none)):
            rc = A.call("ge_shard_owner_apply", shard.ptr, rows_local, d, rec.ptr + 4 * words * s, cap, r.ptr, S())
            if rc:
                return rc
        return 0

    def owner_canon(A):
        rec = A["records"].get(I32, (S_, words))
        out = {"shard": A["shard"].get(I32)}
        for s in range(S_):
            for t in range(n_sub_own):
                tile = rec[s, t * (64 + 18 * P_own):(t + 1) * (64 + 18 * P_own)]
                n = int(tile[0])
                assert 0 <= n <= P_own
                out["n%d_%d" % (s, t)] = tile[:1].copy()
                out["items%d_%d" % (s, t)] = tile[64:64 + 2 * n].copy()
                out["islots%d_%d" % (s, t)] = tile[64 + 2 * P_own:64 + 2 * P_own + 16 * n].copy()
        return out

    def owner_verify(A):
        want = shard0.astype(np.float64)
        np.add.at(want, req_all, recv.astype(np.float64))
        after = A["shard"].get(F32, (rows_local, d))
        near(8, np.abs(after - want), 2e-5, strict=True)
        unnamed_rows_unchanged(shard0, after, req_all)
        c = owner_canon(A)
        assert sum(int(c["n1_%d" % t][0]) for t in range(n_sub_own)) == 0           # the empty step has no items
        items = np.concatenate([c["items0_%d" % t] for t in range(n_sub_own)]).reshape(-1, 2)
        assert np.array_equal(np.unique(items[:, 0]), np.unique(req_all))            # one item per distinct row (<= 16 slots each)
        assert (items[:, 1] & 0x3FFFFFFF).sum() == cap
    drive(owner, owner_verify, ws=True, canon=owner_canon)
    claimed(test_row_sharded_step)


# =============================================================== coverage
def test_every_writing_entry_point_is_guarded():
    """Every symbol of the ABI that writes device memory is claimed by a guarded case above (and each case checks that
    it called what it claims).  Exempt: events, the pipeline handle, *_max_*, ge_version, the size functions and
    ge_train_prepared_layout, which fills a host array."""
    def exempt(n):
        return (n.startswith("ge_event_") or n.startswith("ge_train_pipeline_") or "_max_" in n or n == "ge_version"
                or n.endswith("_bytes") or n.endswith("_words") or n == "ge_train_prepared_layout")
    missing = sorted(n for n in _lib.SYMBOLS if not exempt(n) and n not in GUARDED)
    assert not missing, "no guarded case for %s" % missing
    assert all(n in _lib.SYMBOLS for n in GUARDED)
