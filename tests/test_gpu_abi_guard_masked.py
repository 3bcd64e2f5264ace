"""GPU: what ge_rank_1vK_masked, ge_topk_1vK_masked, ge_candidate_mask_from_classes and ge_candidate_mask_from_cells may
touch -- the cases of tests/test_gpu_abi_guard.py for the four entry points of the per-relation candidate sets, built with
its drive() / claimed() and tests/abi_guard.py: guard-banded buffers of EXACTLY the declared sizes (the mask of n_sets * W
words, row_set of B), 0x00 / 0xFF poison, bitwise-equal runs, `need - 1` -> GE_ENOMEM, the workspace offset by 16 bytes ->
GE_EINVAL, outputs still poison after a refusal; the results exact against numpy over the unmasked sweep's stored losses.

The cases register in test_gpu_abi_guard.GUARDED at import, which is what its test_every_writing_entry_point_is_guarded
reads: the two files are collected together (`pytest tests -m gpu`)."""
import numpy as np
import pytest
import torch

import test_gpu_abi_guard as G
from graphembeddings_amd import _lib
from tests import topk_ref as TK

pytestmark = pytest.mark.gpu

I32, I64, U32, F32 = np.int32, np.int64, np.uint32, np.float32


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")
    G.CALLED.clear()


def words(K):
    return 4 * ((K + 127) // 128)


def pack(bits, n_words):
    full = np.zeros((bits.shape[0], n_words * 32), bool)
    full[:, :bits.shape[1]] = bits
    return np.packbits(full, axis=1, bitorder="little").view(U32).reshape(bits.shape[0], n_words)


@G.guards("ge_candidate_mask_from_classes", "ge_candidate_mask_from_cells")
@pytest.mark.parametrize("K,n_sets,n_class", [(1, 1, 1), (127, 3, 33), (129, 70, 32), (417, 5, 70)])
def test_mask_builders(K, n_sets, n_class):
    rng = np.random.default_rng(K + n_sets)
    W = int(_lib.load().ge_candidate_mask_words(K))
    assert W == words(K)
    cls = rng.integers(-1, n_class + 1, K).astype(I32)
    allow_b = rng.random((n_sets, n_class)) < 0.5
    allow = pack(allow_b, (n_class + 31) // 32)
    ok = (cls >= 0) & (cls < n_class)
    adm = np.zeros((n_sets, K), bool)
    adm[:, ok] = allow_b[:, cls[ok]]

    def classes(A, mode):
        c, a = A.data("cand_class", cls), A.data("allow", allow)
        m = A.out("mask", 4 * n_sets * W)
        return A.call("ge_candidate_mask_from_classes", c.ptr, K, a.ptr, n_sets, n_class, m.ptr, G.S())

    def verify_classes(A):
        assert np.array_equal(A["mask"].get(U32, (n_sets, W)), pack(adm, W))
    G.drive(classes, verify_classes)

    M = 3 * K + 5
    cells = np.stack([rng.integers(-1, n_sets + 1, M), rng.integers(-1, K + 33, M)], 1).astype(I32)
    cells[0] = [n_sets - 1, K - 1]
    inside = (cells[:, 0] >= 0) & (cells[:, 0] < n_sets) & (cells[:, 1] >= 0) & (cells[:, 1] < K)
    adm2 = np.zeros((n_sets, K), bool)
    adm2[cells[inside, 0], cells[inside, 1]] = True

    def from_cells(A, mode):
        c = A.data("cells", cells)
        m = A.out("mask", 4 * n_sets * W)
        return A.call("ge_candidate_mask_from_cells", c.ptr, M, n_sets, K, m.ptr, G.S())

    def verify_cells(A):
        assert np.array_equal(A["mask"].get(U32, (n_sets, W)), pack(adm2, W))
    G.drive(from_cells, verify_cells)
    G.claimed(test_mask_builders)


@G.guards("ge_rank_1vK_masked", "ge_topk_1vK_masked")
@pytest.mark.parametrize("B,K", [(1, 1), (127, 63), (128, 64), (129, 65), (5, 257)])
@pytest.mark.parametrize("d", [56, 64])
def test_masked_sweeps(B, K, d):
    """test_gpu_abi_guard.test_candidate_sweeps' shapes on the split-precision dims, with sets: counts, true_loss and the
    top-k lists exact against the stored losses of the unmasked sweep."""
    lib = _lib.load()
    N, R, n_sets = 300, 10, 7
    rng = np.random.default_rng(1000 * B + K + d)
    real = (rng.standard_normal((N, d)) * 0.25).astype(F32)
    real[50], real[60] = real[51], real[61]
    cand = np.concatenate([[50, 51, 60, 61], rng.permutation(np.setdiff1d(np.arange(R, N), [50, 51, 60, 61]))])[:K]
    cand = rng.permutation(cand).astype(I32)
    hr = np.stack([rng.integers(R, N, B), rng.integers(0, R, B)], 1).astype(I32)
    tid = cand[rng.integers(0, K, B)].astype(I32)
    head = (B + d // 8) % 2
    known = rng.random((B, K)) < 0.1
    koff, krc = G.cells_from_mask(known)
    W = words(K)
    adm = rng.random((n_sets, K)) < 0.5
    adm[0], adm[1] = False, True
    padded = np.ones((n_sets, 32 * W), bool)                # the bits behind K are set: they are ignored
    padded[:, :K] = adm
    mask = pack(padded, W)
    row_set = rng.integers(-1, n_sets, B).astype(I32)
    rows = np.where((row_set < 0)[:, None], True, adm[np.maximum(row_set, 0)])
    pos_of = np.full(N, -1, I64)
    pos_of[cand] = np.arange(K)
    col = pos_of[tid]
    pbytes = int(lib.ge_rank_planes_bytes(N, d, K))
    assert pbytes > 0

    for model in (0, 2):
        table = G.to_spectral(real).astype(F32) if model == 2 else real
        state = {}

        def base(A, mode):
            t, h, ti, c = A.data("table", table), A.data("hr", hr), A.data("true_id", tid), A.data("cand", cand)
            nb, nk = A.out("n_before", 4 * B), A.out("n_known_before", 4 * B)
            tl, sc = A.out("true_loss", 4 * B), A.out("scores_out", 4 * B * K)
            return A.call("ge_rank_1vK_planes", t.ptr, N, d, h.ptr, B, ti.ptr, c.ptr, K, 1.0, model, head, None, None,
                          nb.ptr, nk.ptr, tl.ptr, sc.ptr, None, G.S())

        def keep(A):
            state["sc"], state["tl"] = A["scores_out"].get(F32, (B, K)), A["true_loss"].get(F32)
        G.drive(base, keep)
        sc, tl = state["sc"], state["tl"]
        before = (sc < tl[:, None]) | ((sc == tl[:, None]) & (cand[None, :] < tid[:, None]))
        enb, enk = (before & rows).sum(1).astype(I32), (before & rows & known).sum(1).astype(I32)

        for filtered, scores, planes in ((True, True, False), (True, False, True), (False, False, False)):
            def rank(A, mode, filtered=filtered, scores=scores, planes=planes):
                t, h, ti, c = A.data("table", table), A.data("hr", hr), A.data("true_id", tid), A.data("cand", cand)
                ko = A.data("known_off", koff).ptr if filtered else None
                kr = A.data("known_rc", krc).ptr if filtered else None
                rs, mk = A.data("row_set", row_set), A.data("mask", mask)
                nb, nk, tl_o = A.out("n_before", 4 * B), A.out("n_known_before", 4 * B), A.out("true_loss", 4 * B)
                so = A.out("scores_out", 4 * B * K).ptr if scores else None
                pl = None
                if planes:
                    p = A.ws("planes", pbytes)
                    assert A.call("ge_rank_planes", t.ptr, N, d, c.ptr, K, 1.0, model, p.ptr, G.S()) == 0
                    p.kind, pl = "in", p.ptr
                return A.call("ge_rank_1vK_masked", t.ptr, N, d, h.ptr, B, ti.ptr, c.ptr, K, 1.0, model, head, ko, kr,
                              nb.ptr, nk.ptr, tl_o.ptr, so, pl, rs.ptr, mk.ptr, n_sets, G.S())

            def verify(A, filtered=filtered, scores=scores):
                assert np.array_equal(A["n_before"].get(I32), enb)
                assert np.array_equal(A["n_known_before"].get(I32), enk if filtered else np.zeros(B, I32))
                assert np.array_equal(A["true_loss"].get(I32), tl.view(I32))
                assert np.array_equal(tl.view(I32), sc[np.arange(B), col].view(I32))
                if scores:
                    assert np.array_equal(A["scores_out"].get(I32, (B, K)), sc.view(I32))
            G.drive(rank, verify)

        for k in (1, 128):
            need = int(lib.ge_topk_workspace_bytes(B, K, k))
            assert need > 0
            for filtered, with_planes in ((True, True), (False, False)):
                def topk(A, mode, filtered=filtered, with_planes=with_planes):
                    t, h, c = A.data("table", table), A.data("hr", hr), A.data("cand", cand)
                    ko = A.data("known_off", koff).ptr if filtered else None
                    kr = A.data("known_rc", krc).ptr if filtered else None
                    rs, mk = A.data("row_set", row_set), A.data("mask", mask)
                    oid, ol, w = A.out("out_id", 4 * B * k), A.out("out_loss", 4 * B * k), A.ws("workspace", need)
                    pl = None
                    if with_planes:
                        p = A.ws("planes", pbytes)
                        assert A.call("ge_rank_planes", t.ptr, N, d, c.ptr, K, 1.0, model, p.ptr, G.S()) == 0
                        p.kind, pl = "in", p.ptr
                    return A.call("ge_topk_1vK_masked", t.ptr, N, d, h.ptr, B, c.ptr, K, 1.0, model, head, ko, kr, k,
                                  oid.ptr, ol.ptr, pl, *G.ws_args(w, mode), rs.ptr, mk.ptr, n_sets, G.S())

                def verify_topk(A, filtered=filtered):
                    eid, el = TK.first_k_rows(sc, cand, k, (known | ~rows) if filtered else ~rows)
                    assert np.array_equal(A["out_id"].get(I32, (B, k)), eid)
                    assert np.array_equal(A["out_loss"].get(F32, (B, k)).view(I32), el.view(I32))
                G.drive(topk, verify_topk, ws=True)
    G.claimed(test_masked_sweeps)
