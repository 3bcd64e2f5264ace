"""GPU: what the ge_rotate_* entry points may touch -- the cases of tests/test_gpu_abi_guard.py for RotatE's six writing
entry points, built with its drive() / claimed() and tests/abi_guard.py: guard-banded tables, accumulators, outputs and
workspaces of EXACTLY the declared sizes, 0x00 / 0xFF poison, bitwise-equal runs, `need - 1` -> GE_ENOMEM, the workspace
offset by 16 bytes -> GE_EINVAL, outputs still poison after a refusal.  rel and acc_rel are [n_rel, d / 2]: a write of a
d-wide relation row to relation R - 1 (which every step case names) lands in the tail guard.  The results against
tests/rotate_ref.py within test_gpu_rotate.py's bound (rotate_ref.bound: 8 e32 + 1e-7).

The cases register in test_gpu_abi_guard.GUARDED at import, which is what its test_every_writing_entry_point_is_guarded
reads: the two files are collected together (`pytest tests -m gpu`)."""
import numpy as np
import pytest
import torch

import test_gpu_abi_guard as G
from graphembeddings_amd import _lib
from oracle import transx_oracle as TO
from tests import rotate_ref as RR
from tests import transx_ref as XR

pytestmark = pytest.mark.gpu

I32, F32 = np.int32, np.float32
A0 = 0.1
LR = float(np.float32(0.05))
FAMILY = 27                                     # G.near's family of these cases


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")
    G.CALLED.clear()


def near(got, ref64, ref32, scale=0.0):
    """test_gpu_rotate.py's rule (rotate_ref.bound) through G.near: |got - ref64| <= 8 e32 + 1e-7, plus one fp32 ulp in a
    case whose e32 is below that ulp; scale: the largest distance a loss is formed from.  Prints each case that needed
    the ulp term."""
    bound, base, e32 = RR.bound(ref64, ref32, scale)
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref64, dtype=np.float64))
    if np.any(err > base):
        print("ULP-TERM guard: |err| %.4g above 8 e32 + 1e-7 = %.4g (e32 %.4g, largest |ref| %.4g, scale %.4g)"
              % (float(err.max()), float(base.min()), e32, float(np.abs(ref64).max()), scale))
    G.near(FAMILY, err, bound)


def rtabs(E, R, d, seed):
    rng = np.random.default_rng(seed)
    return {"ent": (rng.standard_normal((E, d)) * 0.5).astype(F32), "rel": rng.uniform(-np.pi, np.pi, (R, d // 2)).astype(F32)}


def rargs(A, l1, tabs, kind="in", shift=0):
    """The leading arguments every ge_rotate_* entry takes; the tables as guarded buffers of exactly [E, d] and [R, d / 2]."""
    b = {k: A.data(k, v, kind, shift) for k, v in tabs.items()}
    return (int(l1), b["ent"].ptr, tabs["ent"].shape[0], b["rel"].ptr, tabs["rel"].shape[0], tabs["ent"].shape[1])


def aargs(A, l1, tabs):
    """rargs with the tables updated in place and one guarded accumulator of exact size per table in front of d."""
    a = rargs(A, l1, tabs, "table")
    accs = {k: A.table("acc_" + k, np.full(v.shape, A0, F32)) for k, v in tabs.items()}
    return (*a[:-1], accs["ent"].ptr, accs["rel"].ptr, a[-1])


def named_ids(k, pos, neg):
    return (pos[:, :2], neg[:, :2]) if k == "ent" else (pos[:, 2],)


@G.guards("ge_rotate_score")
@pytest.mark.parametrize("B,bad", [(1, False), (1, True), (63, True), (64, True), (65, True), (257, True)])
def test_rotate_scores(B, bad):
    """out [B] of exactly 4 B bytes; d = 50 takes the scalar path, d = 200 the vector one, shift = 4 the scalar one at
    d = 200 too."""
    E, R = 300, 9
    for d, shift in ((50, 0), (200, 0), (200, 4), (2, 0)):
        for l1 in (True, False):
            tabs = rtabs(E, R, d, seed=d + B)
            tri = G.triples_of(E, B, seed=B, bad=bad)
            tri[:, 2] %= R
            if B > 1:
                tri[0], tri[1] = (0, E - 1, R - 1), (E - 1, 0, 0)
            bad_rows = [B // 2] if bad else []

            def case(A, mode):
                a = rargs(A, l1, tabs, shift=shift)
                return A.call("ge_rotate_score", *a, A.data("triples", tri).ptr, B, A.out("out", 4 * B).ptr, G.S())

            def verify(A):
                got = A["out"].get(F32)
                ok = G.check_nan_rows(got, bad_rows)
                t64 = G.f64(tabs)
                near(got[ok], RR.dist(t64, tri[ok], l1), RR.dist(t64, tri[ok], l1, F32))
            G.drive(case, verify)
    G.claimed(test_rotate_scores)


@G.guards("ge_rotate_hinge_step", "ge_rotate_adagrad_step")
@pytest.mark.parametrize("B", [1, 65, 257])
def test_rotate_single_steps(B):
    """pairs_of names entity 0 and E - 1 and relation 0 and R - 1; d = 50 takes the scalar kernels, d = 200 the float4
    ones, d = 520 the float4 gradient kernel's 64-lane groups (65 chunks: lane 0 holds a second one), d = 134 the
    scalar one's (67 chunks).  The margin is the least one >= 1 at which pairs 0 and 1, which name the first and the last
    rows, are active."""
    E, R = 300, 9
    pos, neg = G.pairs_of(E, R, B, seed=B)
    lib = _lib.load()
    for entry in ("ge_rotate_hinge_step", "ge_rotate_adagrad_step"):
        ada = entry.endswith("adagrad_step")
        for d in (50, 200, 520, 134):
            for l1 in (True, False):
                tabs = rtabs(E, R, d, seed=d + B)
                need = int(lib.ge_rotate_step_workspace_bytes(E, R, d, B))
                assert need > 0
                t64 = G.f64(tabs)
                a64 = {k: np.full(v.shape, np.float64(F32(A0))) for k, v in tabs.items()}
                z0 = RR.dist(t64, pos[:2], l1) - RR.dist(t64, neg[:2], l1)
                margin = float(F32(max(1.0, np.ceil(1.0 - z0.min()))))
                act = RR.active_mask(t64, pos, neg, margin, l1)
                assert act[:2].all() and np.array_equal(act, RR.active_mask(t64, pos, neg, margin, l1, F32))
                if ada:
                    rt, ra, rloss = RR.adagrad_step(t64, a64, pos, neg, LR, margin, l1)
                    st, sa, sloss = RR.adagrad_step(t64, a64, pos, neg, LR, margin, l1, F32)
                else:
                    (rt, rloss), (st, sloss) = RR.sgd_step(t64, pos, neg, LR, margin, l1), RR.sgd_step(t64, pos, neg, LR, margin, l1, F32)

                def case(A, mode):
                    a = aargs(A, l1, tabs) if ada else rargs(A, l1, tabs, "table")
                    p, n = A.data("pos", pos), A.data("neg", neg)
                    loss, w = A.out("loss", 4), A.ws("workspace", need)
                    return A.call(entry, *a, p.ptr, n.ptr, B, margin, LR, loss.ptr, *G.ws_args(w, mode), G.S())

                def verify(A):
                    near(A["loss"].get(F32)[:1], [rloss], [sloss], scale=RR.largest_dist(t64, pos, neg, l1))
                    for k in tabs:
                        after = A[k].get(F32, tabs[k].shape)
                        near(after, rt[k], st[k])
                        G.unnamed_rows_unchanged(tabs[k], after, *named_ids(k, pos[act], neg[act]))
                        ends = (0, -1) if k == "ent" or B > 1 else (-1,)    # (B = 1 names relation R - 1 alone)
                        assert all((after[r] != tabs[k][r]).any() for r in ends), k   # row 0 and the last row were updated
                        if ada:
                            acc = A["acc_" + k].get(F32, tabs[k].shape)
                            near(acc, ra[k], sa[k])
                            G.unnamed_rows_unchanged(np.full(tabs[k].shape, A0, F32), acc, *named_ids(k, pos[act], neg[act]))
                            assert all((acc[r] > F32(A0)).any() for r in ends), k
                G.drive(case, verify, ws=True)
    G.claimed(test_rotate_single_steps)


@G.guards("ge_rotate_train_steps", "ge_rotate_train_steps_adagrad")
@pytest.mark.parametrize("B", [255, 257, 4097])
def test_rotate_train_steps(B):
    """Three steps on the oracle's draws: every loss and the final tables and accumulators against the fp64 replay, with
    e32 taken from the same replay run in float32 (the loop's intermediate states never leave the device)."""
    lib = _lib.load()
    tri, E, R = G.loop_kg()
    idx = TO.BernoulliIndex(tri, 0, E, R)
    tri32 = tri.astype(I32)
    seed, first, margin, STEPS, D = 21, 4, 1.0, G.STEPS, G.D_LOOP
    D += D % 2
    draws = []
    for s in range(STEPS):
        p_ = tri32[XR.draw_positive_rows(len(tri), B, seed, first + s)]
        draws.append((p_, TO.bernoulli_corrupt_batch(p_, idx, seed, first + s)))

    def sampler_args(A):
        return (A.data("triples", tri32).ptr, len(tri), A.data("bh_key", idx.bh_key).ptr, A.data("bh_ent", idx.bh_ent).ptr,
                A.data("bt_key", idx.bt_key).ptr, A.data("bt_ent", idx.bt_ent).ptr, len(tri), A.data("thr", idx.tail_threshold).ptr)

    tabs = rtabs(E, R, D, seed=B)
    need = int(lib.ge_rotate_step_workspace_bytes(E, R, D, B))
    assert need > 0
    for entry in ("ge_rotate_train_steps", "ge_rotate_train_steps_adagrad"):
        ada = entry.endswith("adagrad")

        def case(A, mode):
            a = aargs(A, False, tabs) if ada else rargs(A, False, tabs, "table")
            losses, w = A.out("losses", 4 * STEPS), A.ws("workspace", need)
            return A.call(entry, *a, *sampler_args(A), seed, first, STEPS, B, margin, LR, losses.ptr, *G.ws_args(w, mode), G.S())

        def verify(A):
            runs = []
            for dtype in (np.float64, F32):
                t, a, ls = G.f64(tabs), {k: np.full(v.shape, np.float64(F32(A0))) for k, v in tabs.items()}, []
                for p_, n_ in draws:
                    if ada:
                        t, a, loss = RR.adagrad_step(t, a, p_, n_, LR, margin, False, dtype)
                    else:
                        t, loss = RR.sgd_step(t, p_, n_, LR, margin, False, dtype)
                    ls.append(loss)
                runs.append((t, a, ls))
            (rt, ra, rl), (st, sa, sl) = runs
            near(A["losses"].get(F32), rl, sl)
            for k in tabs:
                near(A[k].get(F32, tabs[k].shape), rt[k], st[k])
                if ada:
                    near(A["acc_" + k].get(F32, tabs[k].shape), ra[k], sa[k])
        G.drive(case, verify, ws=True)
    G.claimed(test_rotate_train_steps)


@G.guards("ge_rotate_rank")
@pytest.mark.parametrize("B", [15, 16, 17])
def test_rotate_rank(B):
    """B around the sweep's 16 rows per workgroup; n_ent around the 256 candidates of a workgroup; with scores_out and the
    known lists, and without either.  The counts equal those implied by the stored distances; true_dist is bitwise the
    stored distance of the target."""
    lib = _lib.load()
    for E, R, d, shift in ((255, 1, 6, 0), (256, 9, 16, 0), (257, 9, 16, 0), (257, 9, 16, 4)):
        rng = np.random.default_rng(E * 10 + R + B)
        l1, head = bool((E + R) % 2), (E + B) % 2
        side = "head" if head else "tail"
        tabs = rtabs(E, R, d, seed=E + R)
        t64 = G.f64(tabs)
        test = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, R, B)], 1).astype(I32)
        test[0, :2] = (0, E - 1)
        test[B - 1, :2] = (E - 1, 0)
        target = test[:, 0] if head else test[:, 1]
        mask = rng.random((B, E)) < 0.05                    # known cells of each row (a row's own list)
        koff, krc = G.cells_from_mask(mask)
        _, _, td64, sc64 = RR.ranks(t64, test, side, l1)
        _, _, td32, sc32 = RR.ranks(t64, test, side, l1, dtype=F32)
        need = int(lib.ge_rotate_rank_workspace_bytes(E, R, d, B))
        assert need > 0
        state = {}
        for with_scores, filtered in ((True, True), (False, False)):
            def rank(A, mode):
                a = rargs(A, l1, tabs, shift=shift)
                tb = A.data("triples", test)
                ko = A.data("known_off", koff).ptr if filtered else None
                kr = A.data("known_rc", krc).ptr if filtered else None
                nb, nk, td = A.out("n_before", 4 * B), A.out("n_known_before", 4 * B), A.out("true_dist", 4 * B)
                sc = A.out("scores_out", 4 * B * E).ptr if with_scores else None
                w = A.ws("workspace", need)
                return A.call("ge_rotate_rank", *a, tb.ptr, B, head, ko, kr, nb.ptr, nk.ptr, td.ptr, sc, *G.ws_args(w, mode), G.S())

            def verify(A):
                nb, nk, td = A["n_before"].get(I32), A["n_known_before"].get(I32), A["true_dist"].get(F32)
                if with_scores:
                    state["sc"] = A["scores_out"].get(F32, (B, E))
                    near(state["sc"], sc64, sc32)
                sc = state["sc"]                            # (a run without scores_out is held to the stored run's values)
                near(td, td64, td32)
                assert np.array_equal(td.view(I32), sc[np.arange(B), target].view(I32))
                snb, snk = RR.counts_from(sc, td, target, mask)
                assert np.array_equal(nb, snb) and np.array_equal(nk, snk if filtered else np.zeros(B, np.int64))
            G.drive(rank, verify, ws=True)
    G.claimed(test_rotate_rank)
