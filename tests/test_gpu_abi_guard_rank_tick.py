"""GPU: what ge_rank_metrics and ge_rank_validation_tick may touch -- the cases of tests/test_gpu_abi_guard.py for the two
entry points of the rank validation tick, built with its drive() / claimed() and tests/abi_guard.py: guard-banded buffers
of EXACTLY the declared sizes (hr [2V,2], true_id / row_set [2V], the known lists of each side, metrics_out [8], the
scalars), 0x00 / 0xFF poison in the outputs, the planes and the workspace, bitwise-equal runs, `need - 1` -> GE_ENOMEM,
the workspace offset by 16 bytes -> GE_EINVAL, outputs, planes and pockets still poison after a refusal, the table and the
accumulator unchanged; the metrics against tests/rank_tick_ref.py over the counts of ge_rank_1vK_planes /
ge_rank_1vK_masked on the same rows, within its bounds.

The cases register in test_gpu_abi_guard.GUARDED at import, which is what its test_every_writing_entry_point_is_guarded
reads: the two files are collected together (`pytest tests -m gpu`)."""
import numpy as np
import pytest
import torch

import test_gpu_abi_guard as G
from graphembeddings_amd import _lib
from tests import rank_tick_ref as RT

pytestmark = pytest.mark.gpu

I32, U32, F32 = np.int32, np.uint32, np.float32
N, R = 300, 8


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")
    G.CALLED.clear()


@G.guards("ge_rank_metrics")
@pytest.mark.parametrize("M", [1, 65, 1025])
@pytest.mark.parametrize("with_loss", [False, True])
def test_rank_metrics(M, with_loss):
    rng = np.random.default_rng(M)
    nb = rng.integers(0, 300, M).astype(I32)
    nk = np.minimum(rng.integers(0, 9, M), nb).astype(I32)
    tl = rng.random(M).astype(F32)
    if M > 1:
        nb[M // 2], nk[M // 2], tl[M // 2] = 0, 0, np.nan
        nk[0] = nb[0] + 1
    ref = RT.rank_metrics(nb, nk, tl if with_loss else None)

    def case(A, mode):
        a, b = A.data("n_before", nb), A.data("n_known_before", nk)
        c = A.data("true_loss", tl).ptr if with_loss else None
        out, imp = A.out("metrics_out", 32), A.out("improved", 4)
        best = A.table("best", np.zeros(1, F32))
        rc = A.call("ge_rank_metrics", a.ptr, b.ptr, c, M, out.ptr, best.ptr, imp.ptr, G.S())
        torch.cuda.synchronize()
        assert np.array_equal(a.get(I32), nb) and np.array_equal(b.get(I32), nk)
        return rc

    def verify(A):
        got = A["metrics_out"].get(F32)
        RT.check_metrics(got, ref, "guard M=%d" % M)
        assert A["improved"].get(I32)[0] == 1 and A["best"].get(I32)[0] == got[:1].view(I32)[0]
    G.drive(case, verify)
    G.claimed(test_rank_metrics)


def words(K):
    return 4 * ((K + 127) // 128)


def pack(bits, n_words):
    full = np.zeros((bits.shape[0], n_words * 32), bool)
    full[:, :bits.shape[1]] = bits
    return np.packbits(full, axis=1, bitorder="little").view(U32).reshape(bits.shape[0], n_words)


@G.guards("ge_rank_validation_tick")
@pytest.mark.parametrize("V,K,d,masked", [(1, 1, 64, False), (129, 65, 64, True), (130, 292, 64, False), (130, 292, 64, True),
                                          (129, 65, 32, False)])
def test_rank_validation_tick(V, K, d, masked):
    lib = _lib.load()
    rng = np.random.default_rng(1000 * V + K + d + masked)
    table = G.table_of(N, d, V + K, 0.25)
    accum = (0.1 + rng.random((N, d))).astype(F32)
    cand = rng.permutation(np.arange(R, N))[:K].astype(I32)
    hr = np.stack([rng.integers(R, N, 2 * V), rng.integers(0, R, 2 * V)], 1).astype(I32)
    tid = cand[rng.integers(0, K, 2 * V)].astype(I32)
    if V > 1:
        hr[V // 2, 0] = N + 3                                   # a bad row a side: counts 0, true loss NaN, not counted
        hr[V + 1, 0] = -1
    known = rng.random((2 * V, K)) < 0.1
    lists = G.cells_from_mask(known[:V]) + G.cells_from_mask(known[V:])
    row_set = hr[:, 1].copy()
    if V > 1:
        row_set[3] = -1                                         # unrestricted
    adm = rng.random((2, R, K)) < 0.5
    masks = [pack(adm[s], words(K)) for s in (0, 1)]
    pbytes, need = int(lib.ge_rank_planes_bytes(N, d, K)), int(lib.ge_rank_tick_workspace_bytes(V))
    assert (pbytes > 0) == (d == 64) and need > 0 and need % 256 == 0

    # the counts of the rank entry points on the same rows, plain tensors
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    exp = {}
    t_d, c_d = dev(table), dev(cand)
    for s in (0, 1):
        sl = slice(s * V, (s + 1) * V)
        h_d, ti_d, ko, kr = dev(hr[sl]), dev(tid[sl]), dev(lists[2 * s]), dev(lists[2 * s + 1].view(np.int16))
        nb, nk, tl = (torch.zeros(V, dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, torch.float32))
        args = [t_d.data_ptr(), N, d, h_d.data_ptr(), V, ti_d.data_ptr(), c_d.data_ptr(), K, 1.0, 0, s, ko.data_ptr(),
                kr.data_ptr(), nb.data_ptr(), nk.data_ptr(), tl.data_ptr(), None, None]
        if masked:
            rs_d, mk_d = dev(row_set[sl]), dev(masks[s].view(I32))
            _lib.call("ge_rank_1vK_masked", *args, rs_d.data_ptr(), mk_d.data_ptr(), R, G.S())
        else:
            _lib.call("ge_rank_1vK_planes", *args, G.S())
        torch.cuda.synchronize()
        exp[s] = (nb.cpu().numpy(), nk.cpu().numpy(), tl.cpu().numpy())
    ref = RT.rank_metrics(*(np.concatenate([exp[0][i], exp[1][i]]) for i in range(3)))
    assert ref[7] == 2 * V - (2 if V > 1 else 0)

    def case(A, mode):
        t, ac = A.data("table", table), A.data("accumulator", accum)
        h, ti, c = A.data("hr", hr), A.data("true_id", tid), A.data("cand", cand)
        kn = [A.data(n, a) for n, a in zip(("known_off_tail", "known_rc_tail", "known_off_head", "known_rc_head"), lists)]
        pl = A.ws("planes", pbytes).ptr if pbytes else None
        sets = (None, None, None, 0)
        if masked:
            sets = (A.data("row_set", row_set).ptr, A.data("mask_tail", masks[0]).ptr, A.data("mask_head", masks[1]).ptr, R)
        out, pk, pa, w = A.out("metrics_out", 32), A.out("pocket", 4 * N * d), A.out("pocket_accumulator", 4 * N * d), A.ws("workspace", need)
        best = A.table("best", np.zeros(1, F32))
        rc = A.call("ge_rank_validation_tick", t.ptr, N, d, h.ptr, ti.ptr, V, c.ptr, K, 1.0, 0, *[b.ptr for b in kn], pl, *sets,
                    ac.ptr, out.ptr, best.ptr, pk.ptr, pa.ptr, *G.ws_args(w, mode), G.S())
        torch.cuda.synchronize()
        assert np.array_equal(t.get(I32), table.view(I32).reshape(-1)) and np.array_equal(ac.get(I32), accum.view(I32).reshape(-1))
        if rc != 0:
            assert best.get(F32)[0] == 0.0
        return rc

    def verify(A):
        got = A["metrics_out"].get(F32)
        RT.check_metrics(got, ref, "guard tick V=%d K=%d d=%d masked=%d" % (V, K, d, masked))
        assert got[0] > 0 and A["best"].get(I32)[0] == got[:1].view(I32)[0]
        assert np.array_equal(A["pocket"].get(I32), table.view(I32).reshape(-1))
        assert np.array_equal(A["pocket_accumulator"].get(I32), accum.view(I32).reshape(-1))
    G.drive(case, verify, ws=True)
    G.claimed(test_rank_validation_tick)
