"""GPU: what ge_adagrad_rows and ge_train_steps_adagrad may touch -- the cases of tests/test_gpu_abi_guard.py for the two
writing entry points of the AdaGrad optimizer, built with its drive() / claimed() and tests/abi_guard.py: guard-banded
buffers of EXACTLY the declared sizes (the table and the accumulator included, so a write to row -1 or row N shows),
0x00 / 0xFF poison, bitwise-equal runs, `need - 1` -> GE_ENOMEM, the workspace offset by 16 bytes -> GE_EINVAL, outputs
still poison after a refusal; the results against tests/adagrad_ref.py within the bounds of tests/test_gpu_adagrad.py.

The cases register in test_gpu_abi_guard.GUARDED at import, which is what its test_every_writing_entry_point_is_guarded
reads: the two files are collected together (`pytest tests -m gpu`)."""
import numpy as np
import pytest
import torch

import test_gpu_abi_guard as G
from graphembeddings_amd import _lib
from oracle import c_oracle as CO
from tests import adagrad_ref as AR

pytestmark = pytest.mark.gpu

I32, F32 = np.int32, np.float32
A0, DELTA = 0.1, 5e-5                                   # tests/test_gpu_adagrad.py


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")
    G.CALLED.clear()


def check(A, N, d, ref_t, ref_a, s, counts, lr, steps=1):
    """The bounds of tests/test_gpu_adagrad.py per step; `steps` free-running steps add up."""
    smax = np.abs(s).max(1, keepdims=True)
    delta = steps * DELTA * np.where(counts[:, None] > 16, np.maximum(1.0, smax), 1.0)
    G.near(8, np.abs(A["table"].get(F32, (N, d)) - ref_t), np.broadcast_to(lr * delta / np.sqrt(A0), ref_t.shape), strict=True)
    ulp = np.spacing(ref_a.astype(F32)).astype(np.float64)
    G.near(8, np.abs(A["accum"].get(F32, (N, d)) - ref_a), 2.0 * smax * delta + 4.0 * steps * ulp, strict=True)


@G.guards("ge_adagrad_rows")
@pytest.mark.parametrize("d", [7, 50, 200])
@pytest.mark.parametrize("R", [1, 390, 4000])
def test_adagrad_rows(R, d):
    """Row 0 and row N - 1 named, empty slots, an id past the table, perm entries outside [0, R) (skipped, never
    dereferenced), one row that takes most of the occurrences at R = 4000."""
    N, lr = 64 if R > 1 else 2, 0.1
    rng = np.random.default_rng(R + d)
    table, accum = G.table_of(N, d, seed=R), np.full((N, d), A0, F32)
    idx = rng.integers(0, N, R).astype(I32)
    if R > 1:
        idx[rng.permutation(R)[:R // 8]] = -1
        idx[:3] = [0, N - 1, N + 5]
        idx[rng.permutation(R)[:R // 2 if R > 1000 else 20]] = 9
    val = (rng.standard_normal((R, d)) * 0.3).astype(F32)
    key = np.where(idx < 0, N, idx)
    perm = np.argsort(key, kind="stable").astype(I32)
    ok = (idx >= 0) & (idx < N)
    counts = np.bincount(idx[ok], minlength=N)
    ref_t, ref_a = table.astype(np.float64), accum.astype(np.float64)
    s, named = AR.apply_rows(ref_t, ref_a, idx, -val.astype(np.float64), lr)

    def case_of(pm):
        def case(A, mode):
            t, a = A.table("table", table), A.table("accum", accum)
            ib, vb, pb = A.data("idx", idx), A.data("val", val), A.data("perm", pm)
            return A.call("ge_adagrad_rows", t.ptr, a.ptr, N, d, ib.ptr, vb.ptr, pb.ptr, R, lr, G.S())
        return case

    def verify(A):
        check(A, N, d, ref_t, ref_a, s, counts, lr)
        G.unnamed_rows_unchanged(table, A["table"].get(F32, (N, d)), idx)
        G.unnamed_rows_unchanged(accum, A["accum"].get(F32, (N, d)), idx)
    G.drive(case_of(perm), verify)
    # entries outside [0, R) at the tail of the order (where the empty slots sort to): the rows before them as above
    if R > 1:
        bad = perm.copy()
        bad[-2:] = [R, -1]
        assert not ok[perm[-2:]].any()
        G.drive(case_of(bad), verify)
    # refused: the accumulator inside the table, and nothing is touched
    A = G.AG.Arena("", 0xFF)
    t, ib, vb, pb = A.table("table", table), A.data("idx", idx), A.data("val", val), A.data("perm", perm)
    assert A.call("ge_adagrad_rows", t.ptr, t.ptr + 4 * d * (N - 1), N, d, ib.ptr, vb.ptr, pb.ptr, R, lr, G.S()) == G.EINVAL
    A.assert_intact()
    assert np.array_equal(A["table"].get(F32, (N, d)).view(I32), table.view(I32))
    G.claimed(test_adagrad_rows)


@G.guards("ge_train_steps_adagrad")
@pytest.mark.parametrize("model", [0, 3])
@pytest.mark.parametrize("B", [257, 4097])
def test_train_steps_adagrad(B, model):
    """One tile and two; keep_all_losses 1 and 0, pipeline = NULL; ComplEx and the direct-correlation HolE kernels.
    Against the fp64 restatement replaying the three steps: losses within 2e-5 (test_train_steps), neg_ws exact."""
    lib = _lib.load()
    N, NREL, STEPS = G.N_LOOP, G.NREL_LOOP, G.STEPS
    types = G.types_of(N, NREL)
    d, T, first_row, seed, gs0 = G.D_LOOP, 2 * B + 50, 7, 21, 3
    margin, lr0, dsteps, drate = 0.2, 0.1, 50.0, 0.5
    tri = G.balanced_triples(T)
    tri[:, 2] %= 40                                     # 40 relation rows: more than 16 slots each at B = 4097
    table, accum = G.table_of(N, d, seed=B), np.full((N, d), A0, F32)
    need = int(lib.ge_train_adagrad_workspace_bytes(B, d))
    assert need > 0 and need == int(lib.ge_train_workspace_bytes(B, d))
    ref_t, ref_a = table.astype(np.float64), accum.astype(np.float64)
    oloss, negs, smax, cmax = [], None, np.zeros((N, d)), np.zeros(N, np.int64)
    for k, row in enumerate(G.loop_rows(first_row, T, B, STEPS)):
        pos = tri[row:row + B]
        negs = CO.corrupt_batch(pos, *types, seed, gs0 + k, 0, 0)
        ol, s, named = AR.step(ref_t, ref_a, pos, negs, G.lr_at(lr0, gs0 + k, dsteps, drate), margin,
                               model="hole" if model else "complex")
        oloss.append(ol)
        smax, cmax = np.maximum(smax, np.abs(s)), np.maximum(cmax, G.slots_per_row(pos, negs, N))
    assert cmax.max() > 16 or B < 4000

    def case_of(keep):
        def case(A, mode):
            t, a, trb = A.table("table", table), A.table("accum", accum), A.data("triples", tri)
            ty = G.type_bufs(A, types)
            loss, ng, w = A.out("loss", 4 * B * (STEPS if keep else 1)), A.out("neg_ws", 12 * B), A.ws("workspace", need)
            return A.call("ge_train_steps_adagrad", t.ptr, a.ptr, N, d, trb.ptr, T, first_row, B, STEPS, ty[0], *ty[1:], seed,
                          gs0, 0, 0, margin, lr0, dsteps, drate, 1.0, model, loss.ptr, keep, ng.ptr, *G.ws_args(w, mode), None,
                          G.S())

        def verify(A):
            loss = A["loss"].get(F32, (-1, B))
            for k in (range(STEPS) if keep else [STEPS - 1]):
                G.near(8, np.abs(loss[k if keep else 0] - oloss[k]), 2e-5, strict=True)
            check(A, N, d, ref_t, ref_a, smax, cmax, lr0, steps=STEPS)
            assert np.array_equal(A["neg_ws"].get(I32, (B, 3)), negs)
        return case, verify
    G.drive(*case_of(1), ws=True)
    G.drive(*case_of(0))
    G.claimed(test_train_steps_adagrad)
