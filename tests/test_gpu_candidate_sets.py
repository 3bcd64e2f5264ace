"""GPU: per-relation candidate sets on the ComplEx / HolE sweeps (ge_rank_1vK_masked, ge_topk_1vK_masked, the two mask
builders, evaluate.CandidateSets, link_prediction_ranks / predict_links with candidate_sets, train.py --candidate_sets).

The oracle is numpy over the losses the UNMASKED ge_rank_1vK_planes stores in scores_out for the same inputs: every
integer must be equal and every float bitwise equal."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu

I32, U32, F32 = np.int32, np.uint32, np.float32
R_REL = 5                                    # relation rows 0 ... 4, entities behind them
TIE = (53, 54, 55)                           # three table rows with identical contents


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")


def words(K):
    return 4 * ((K + 127) // 128)


def pack(adm, pad_ones=False):
    """uint32 [n_sets, W] of a bool [n_sets, K]: bit c & 31 of word c >> 5.  pad_ones: the bits behind K are set (the
    entry points must ignore them)."""
    n_sets, K = adm.shape
    full = np.full((n_sets, words(K) * 32), pad_ones, dtype=bool)
    full[:, :K] = adm
    return np.packbits(full, axis=1, bitorder="little").view(U32).reshape(n_sets, words(K))


def make_table(N, d, scale, seed):
    """scale "table": test_gpu_topk.py's _table (duplicates, near-duplicates a few ulps apart: scores inside the bracket
    of the exact comparison).  "init": the untrained initializer's sigma = sqrt(2.6 / (N + d)) at N = 5 M rows, 0.0007
    (at this test's 700 rows the same formula gives 0.06 and losses 1e-3 apart; at 1.2 M rows a spectral table's losses
    still spread over 1.4e-6): every loss of a row lies within 1e-6 of every other, inside the bracket -- asserted.  "saturated": rows +-20 u + 5 % noise for one direction u with zero imaginary part, clipped to
    max_norm = 8: |score| = 512 / sqrt(d / 2) >= 42, the sigmoid saturates and the bracket is infinite."""
    rng = np.random.default_rng(seed)
    if scale == "saturated":
        u = np.zeros(d, F32)
        u[:d // 2] = 1.0 / np.sqrt(d // 2)
        sign = rng.choice(np.array([-1.0, 1.0], F32), (N, 1))
        table = (20.0 * sign * u[None, :] * (1.0 + 0.05 * rng.standard_normal((N, d)))).astype(F32)
    else:
        sigma = 0.2 if scale == "table" else np.sqrt(2.6 / 5e6)
        table = (rng.standard_normal((N, d)) * sigma).astype(F32)
        table[50] = table[51]
        table[60] = table[61]
        for j in range(70, 90):
            table[j] = table[52] * np.float32(1.0 + 2e-7 * (j - 79.5))
    table[TIE[1]] = table[TIE[0]]
    table[TIE[2]] = table[TIE[0]]
    return table


def make_problem(N, d, K, B, side, model, scale="table", seed=0):
    """A sweep with ties: the candidates hold the three identical rows TIE, rows 0 ... 2 have the middle one as their
    true entity; known cells at density 0.1."""
    from graphembeddings_amd import hole as H
    rng = np.random.default_rng(seed)
    emb = torch.as_tensor(make_table(N, d, scale, seed + 1)).cuda()
    if model == "hole_spectral":
        emb = H.hole_to_spectral(emb)
    special = np.array(list(TIE) + [50, 51, 60, 61, 52] + list(range(70, 90)))
    rest = rng.permutation(np.setdiff1d(np.arange(R_REL, N), special))
    cand = rng.permutation(np.concatenate([special, rest])[:K]).astype(I32)
    hr = np.stack([rng.integers(R_REL, N, B), rng.integers(0, R_REL, B)], 1).astype(I32)
    p0 = int(np.nonzero(cand == 60)[0][0])            # the position of the "one bit" sets: never a true candidate
    tid = rng.choice(np.delete(cand, p0), B).astype(I32)
    tid[:3] = TIE[1]
    known = rng.random((B, K)) < 0.1
    return dict(N=N, d=d, K=K, B=B, side=side, model=model, emb=emb, cand=cand, hr=hr, tid=tid, p0=p0, known=known,
                max_norm=8.0 if scale == "saturated" else 1.0, rng=rng)


def cells_from_mask(mask):
    """ge_known_cells' per-tile lists of a [B, K] bool matrix."""
    B, K = mask.shape
    off, rc = [0], []
    for rt in range((B + 127) // 128):
        for ct in range((K + 127) // 128):
            r, c = np.nonzero(mask[rt * 128:(rt + 1) * 128, ct * 128:(ct + 1) * 128])
            rc.append(((r << 7) | c).astype(np.uint16))
            off.append(off[-1] + len(r))
    rc = np.concatenate(rc)
    return (torch.as_tensor(np.asarray(off, I32)).cuda(),
            torch.as_tensor((rc if len(rc) else np.zeros(1, np.uint16)).view(np.int16)).cuda())


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def sets_of(P, adm, pad_ones=False):
    from graphembeddings_amd import evaluate as E
    mask = dev(pack(adm, pad_ones).view(I32))
    return E.CandidateSets(P["cand_t"], mask, adm.sum(1))


def prepare(P):
    """The device tensors, the known-cell lists and the unmasked sweep's stored losses, counts and true losses."""
    from graphembeddings_amd import hole as H
    P["cand_t"], P["hr_t"], P["tid_t"] = dev(P["cand"]), dev(P["hr"]), dev(P["tid"])
    P["off"], P["rc"] = cells_from_mask(P["known"])
    P["kw"] = dict(cand_is_head=(P["side"] == "head"), max_norm=P["max_norm"], model=P["model"])
    nb, nk, tl, sc = H.rank_candidates(P["emb"], P["hr_t"], P["tid_t"], P["cand_t"], known_off=P["off"], known_rc=P["rc"],
                                       return_true_loss=True, return_scores=True, **P["kw"])
    P["nb"], P["nk"], P["tl"], P["sc"] = (x.cpu().numpy() for x in (nb, nk, tl, sc))
    pos = {int(c): i for i, c in enumerate(P["cand"])}
    P["tpos"] = np.array([pos[int(t)] for t in P["tid"]])
    # the three identical rows really tie, bit for bit, in every row of the sweep
    tp = [pos[t] for t in TIE]
    assert np.array_equal(P["sc"][:, tp[0]].view(I32), P["sc"][:, tp[1]].view(I32))
    assert np.array_equal(P["sc"][:, tp[0]].view(I32), P["sc"][:, tp[2]].view(I32))
    assert np.array_equal(P["tl"].view(I32), P["sc"][np.arange(P["B"]), P["tpos"]].view(I32))
    return P


def expected_counts(P, adm_rows):
    sc, cand, tid = P["sc"], P["cand"].astype(np.int64), P["tid"].astype(np.int64)
    tl = sc[np.arange(P["B"]), P["tpos"]]
    before = (sc < tl[:, None]) | ((sc == tl[:, None]) & (cand[None, :] < tid[:, None]))
    before &= adm_rows
    return before.sum(1).astype(I32), (before & P["known"]).sum(1).astype(I32)


def rows_of(adm, row_set):
    return np.where((row_set < 0)[:, None], True, adm[np.maximum(row_set, 0)])


def set_families(P, n_sets):
    """(adm bool [n_sets, K], row_set int32 [B], rows whose set is a density-0.5 one).
    1 set: random.  3: empty, full, random.  70: empty, full, one bit (not a true candidate's), the tie group's strict
    subsets {first} and {first, third} (+ random others), 32 sets "only row j's true candidate", random ones."""
    rng, K, B = P["rng"], P["K"], P["B"]
    pos = {int(c): i for i, c in enumerate(P["cand"])}
    adm = rng.random((n_sets, K)) < 0.5
    random_sets = np.ones(n_sets, bool)
    row_set = rng.integers(-1, n_sets, B).astype(I32)
    if n_sets == 1:
        row_set[::7] = -1
        row_set[0] = 0
    if n_sets >= 3:
        adm[0], adm[1] = False, True
        random_sets[:2] = False
    if n_sets == 70:
        adm[2] = False
        adm[2, P["p0"]] = True
        adm[3] = False
        adm[3, pos[TIE[0]]] = True
        adm[4, [pos[t] for t in TIE]] = [True, False, True]
        random_sets[2:4] = False
        for j in range(32):
            adm[5 + j] = False
            random_sets[5 + j] = False
            if j < B:
                adm[5 + j, P["tpos"][j]] = True
                if j % 2 == 0:
                    row_set[j] = 5 + j
        row_set[:3] = [3, 4, 7][:B]                      # the tie rows: strict subsets of the group, the true one alone
        if B > 10:
            row_set[3:7] = [0, 1, 2, -1]
    is_random = (row_set >= 0) & random_sets[np.maximum(row_set, 0)]
    return adm, row_set, is_random


def check_masked_ranks(P, adm, row_set, is_random=None, pad_ones=False):
    """ge_rank_1vK_masked with and without scores_out (MODE 1 and MODE 0) against numpy over the stored losses."""
    from graphembeddings_amd import hole as H
    cs = sets_of(P, adm, pad_ones)
    rs = dev(row_set)
    enb, enk = expected_counts(P, rows_of(adm, row_set))
    args = (P["emb"], P["hr_t"], P["tid_t"], P["cand_t"])
    kw = dict(known_off=P["off"], known_rc=P["rc"], candidate_sets=cs, row_sets=rs, return_true_loss=True, **P["kw"])
    nb1, nk1, tl1, sc1 = (x.cpu().numpy() for x in H.rank_candidates(*args, return_scores=True, **kw))
    nb0, nk0, tl0 = (x.cpu().numpy() for x in H.rank_candidates(*args, **kw))
    for nb, nk, tl in ((nb1, nk1, tl1), (nb0, nk0, tl0)):
        assert np.array_equal(nb, enb), (np.nonzero(nb != enb)[0][:5], nb[nb != enb][:5], enb[nb != enb][:5])
        assert np.array_equal(nk, enk)
        assert np.array_equal(tl.view(I32), P["tl"].view(I32))
    assert np.array_equal(sc1.view(I32), P["sc"].view(I32))
    # unfiltered: no known cells, n_known_before = 0
    nbu, nku = (x.cpu().numpy() for x in H.rank_candidates(*args, candidate_sets=cs, row_sets=rs, **P["kw"]))
    assert np.array_equal(nbu, enb) and not nku.any()
    if is_random is not None and is_random.any():
        # a kernel that ignores the mask cannot pass: at density 0.5 the count changes on at least half the rows
        assert (nb0[is_random] != P["nb"][is_random]).mean() >= 0.5
    return nb0, nk0


@pytest.mark.parametrize("model", ["complex", "hole_spectral"])
@pytest.mark.parametrize("side", ["tail", "head"])
@pytest.mark.parametrize("B", [1, 129, 200])
@pytest.mark.parametrize("K", [129, 130, 417])
@pytest.mark.parametrize("d", [56, 200, 288])
def test_masked_ranks_equal_numpy_over_stored_losses(d, K, B, side, model):
    """K = 129 / 130 / 417: a last tile of 1, 2 and 33 candidates.  n_sets 1, 3 and 70 with every kind of set; the tie
    group; known cells over admissible and inadmissible candidates; MODE 0 against MODE 1; all ones and row_set = -1
    against the unmasked entry point."""
    P = prepare(make_problem(700, d, K, B, side, model, seed=d + K + B))
    for n_sets in (1, 3, 70):
        adm, row_set, is_random = set_families(P, n_sets)
        rows = rows_of(adm, row_set)
        if B > 1 and is_random.any():
            assert (P["known"] & rows).any() and (P["known"] & ~rows).any()
        check_masked_ranks(P, adm, row_set, is_random, pad_ones=(n_sets == 3))
        if B == 1 and n_sets == 70:                       # one row: each kind of set in turn
            for s in (0, 1, 2, 3, 4, 5, 40, -1):
                check_masked_ranks(P, adm, np.array([s], I32))
    # every bit set, and row_set = -1 with any mask: the unmasked outputs, bitwise
    ones = np.ones((3, K), bool)
    for adm, row_set in ((ones, np.arange(B, dtype=I32) % 3), (np.zeros((3, K), bool), np.full(B, -1, I32))):
        nb, nk = check_masked_ranks(P, adm, row_set)
        assert np.array_equal(nb, P["nb"]) and np.array_equal(nk, P["nk"])


@pytest.mark.parametrize("scale", ["init", "saturated"])
@pytest.mark.parametrize("model,side", [("complex", "tail"), ("hole_spectral", "head")])
@pytest.mark.parametrize("K,B", [(129, 129), (417, 200)])
@pytest.mark.parametrize("d", [56, 200, 288])
def test_masked_ranks_inside_the_bracket_and_at_saturation(d, K, B, model, side, scale):
    """The two other table scales: the initializer's (every score inside the true candidate's bracket: the exact
    comparison decides every bit) and saturated sigmoids (an infinite bracket, losses that tie in their thousands)."""
    P = prepare(make_problem(700, d, K, B, side, model, scale=scale, seed=d + K))
    if scale == "saturated":
        assert ((P["sc"] < 1e-5) | (P["sc"] > 1 - 1e-5)).mean() > 0.9          # it does saturate
    else:
        assert np.ptp(P["sc"]) < 1e-6                                           # all inside every row's bracket
    for n_sets in (1, 70):
        adm, row_set, is_random = set_families(P, n_sets)
        check_masked_ranks(P, adm, row_set, is_random)


def test_masked_bad_row_sets_and_refusals():
    """Through the raw ABI: a set index outside [-1, n_sets) makes the row a bad row (counts 0, NaN losses; top-k -1 / NaN);
    null pointers and n_sets < 1 are GE_EINVAL; other dims GE_ENOTSUP.  The wrappers raise ValueError on the host."""
    from graphembeddings_amd import _lib
    from graphembeddings_amd import evaluate as E
    from graphembeddings_amd import hole as H
    P = prepare(make_problem(700, 64, 130, 6, "tail", "complex", seed=9))
    B, K, n_sets = P["B"], P["K"], 3
    adm = np.ones((n_sets, K), bool)
    mask = dev(pack(adm).view(I32))
    row_set = np.array([0, n_sets, -2, 2, 2 ** 30, -1], I32)
    rs = dev(row_set)
    bad = np.array([False, True, True, False, True, False])
    nb = torch.full((B,), 77, dtype=torch.int32, device="cuda")
    nk, tl = torch.full_like(nb, 77), torch.zeros(B, device="cuda")
    sc = torch.zeros(B, K, device="cuda")
    emb, S = P["emb"], torch.cuda.current_stream().cuda_stream
    lib = _lib.load()

    def rank(d=64, row_set_p=rs.data_ptr(), mask_p=mask.data_ptr(), n=n_sets, max_norm=1.0, model=0):
        return int(lib.ge_rank_1vK_masked(emb.data_ptr(), 700 * 64 // d, d, P["hr_t"].data_ptr(), B, P["tid_t"].data_ptr(),
                                          P["cand_t"].data_ptr(), K, max_norm, model, 0, None, None, nb.data_ptr(),
                                          nk.data_ptr(), tl.data_ptr(), sc.data_ptr(), None, row_set_p, mask_p, n, S))
    assert rank() == 0
    nb_h, tl_h, sc_h = nb.cpu().numpy(), tl.cpu().numpy(), sc.cpu().numpy()
    assert not nb_h[bad].any() and not nk.cpu().numpy().any()
    assert np.isnan(tl_h[bad]).all() and np.isnan(sc_h[bad]).all()
    assert np.array_equal(nb_h[~bad], P["nb"][~bad]) and np.array_equal(sc_h[~bad].view(I32), P["sc"][~bad].view(I32))
    k = 4
    oid = torch.zeros(B, k, dtype=torch.int32, device="cuda")
    ol = torch.zeros(B, k, device="cuda")
    ws = torch.empty(int(lib.ge_topk_workspace_bytes(B, K, k)), dtype=torch.uint8, device="cuda")

    def topk(d=64, row_set_p=rs.data_ptr(), mask_p=mask.data_ptr(), n=n_sets, max_norm=1.0, model=0):
        return int(lib.ge_topk_1vK_masked(emb.data_ptr(), 700 * 64 // d, d, P["hr_t"].data_ptr(), B, P["cand_t"].data_ptr(), K,
                                          max_norm, model, 0, None, None, k, oid.data_ptr(), ol.data_ptr(), None,
                                          ws.data_ptr(), ws.numel(), row_set_p, mask_p, n, S))
    assert topk() == 0
    assert (oid.cpu().numpy()[bad] == -1).all() and np.isnan(ol.cpu().numpy()[bad]).all()
    eid, el = TR.first_k_rows(P["sc"][~bad], P["cand"], k)
    assert np.array_equal(oid.cpu().numpy()[~bad], eid) and np.array_equal(ol.cpu().numpy()[~bad].view(I32), el.view(I32))
    for f in (rank, topk):
        assert f(row_set_p=None) == _lib.GE_EINVAL and f(mask_p=None) == _lib.GE_EINVAL and f(n=0) == _lib.GE_EINVAL
        assert f(d=40) == _lib.GE_ENOTSUP and f(d=320) == _lib.GE_ENOTSUP and f(max_norm=9.0) == _lib.GE_ENOTSUP
        assert f(model=1) == _lib.GE_ENOTSUP                                    # a real-valued HolE table
    cs = E.CandidateSets(P["cand_t"], mask, adm.sum(1))
    with pytest.raises(ValueError):
        H.rank_candidates(emb, P["hr_t"], P["tid_t"], P["cand_t"], candidate_sets=cs, row_sets=rs)
    with pytest.raises(ValueError):
        H.topk_candidates(emb, P["hr_t"], P["cand_t"], 3, candidate_sets=cs, row_sets=rs[:3])
    with pytest.raises(ValueError):                                             # a mask for another candidate list
        H.topk_candidates(emb, P["hr_t"], P["cand_t"].flip(0).contiguous(), 3, candidate_sets=cs)
    with pytest.raises(ValueError):                                             # a mask of another shape
        H.rank_candidates(emb, P["hr_t"], P["tid_t"], P["cand_t"], candidate_sets=E.CandidateSets(P["cand_t"], mask[:, :4].contiguous(), adm.sum(1)))
    with pytest.raises(ValueError):
        H.rank_candidates(emb, P["hr_t"], P["tid_t"], P["cand_t"], row_sets=rs)


# ------------------------------------------------------------------ top-k
def topk_oracle(sc, cand, k, skip):
    """First k (loss, id) ascending per row of non-negative losses, skipped cells left out, -1 / +inf padding: the sort
    of TR.first_k_rows on integer keys (loss bits << 32 | id), vectorised."""
    key = (sc.view(U32).astype(np.uint64) << np.uint64(32)) | cand.astype(np.uint64)[None, :]
    none = np.uint64(2 ** 64 - 1)
    key = np.where(skip, none, key)
    if key.shape[1] < k:
        key = np.concatenate([key, np.full((key.shape[0], k - key.shape[1]), none)], 1)
    key = np.sort(key, axis=1)[:, :k]
    ids = np.where(key == none, -1, (key & np.uint64(0xFFFFFFFF)).astype(np.int64))
    ls = np.where(key == none, np.uint32(0x7F800000), (key >> np.uint64(32)).astype(U32)).astype(U32).view(F32)
    return ids, ls


def check_masked_topk(P, adm, row_set, k, with_known=True):
    from graphembeddings_amd import hole as H
    cs = sets_of(P, adm)
    skip = ~rows_of(adm, row_set)
    kn = {}
    if with_known:
        skip |= P["known"]
        kn = dict(known_off=P["off"], known_rc=P["rc"])
    ids, ls = H.topk_candidates(P["emb"], P["hr_t"], P["cand_t"], k, candidate_sets=cs, row_sets=dev(row_set), **kn, **P["kw"])
    eid, el = topk_oracle(P["sc"], P["cand"], k, skip)
    assert np.array_equal(ids.cpu().numpy(), eid)
    assert np.array_equal(ls.cpu().numpy().view(I32), el.view(I32))
    return ids.cpu().numpy(), ls.cpu().numpy(), (~skip).sum(1)


@pytest.mark.parametrize("k", [1, 5, 128])
@pytest.mark.parametrize("d,K,B,side,model", [(56, 129, 129, "tail", "complex"), (200, 417, 200, "head", "hole_spectral"),
                                              (288, 130, 1, "tail", "hole_spectral"), (200, 130, 200, "head", "complex")])
def test_masked_topk_equals_the_first_admissible_pops(d, K, B, side, model, k):
    """The first k pops that are admissible and not known, over the stored losses; rows with fewer than k of them (the
    empty, one-bit and single-candidate sets) are padded -1 / +inf; all ones and row_set = -1 equal the unmasked call."""
    from graphembeddings_amd import hole as H
    P = prepare(make_problem(700, d, K, B, side, model, seed=d + K + B + k))
    eid, el = TR.first_k_rows(P["sc"], P["cand"], k, P["known"])               # the vectorised oracle against the heap's
    oid, ol = topk_oracle(P["sc"], P["cand"], k, P["known"])
    assert np.array_equal(eid, oid) and np.array_equal(el.view(I32), ol.view(I32))
    short = 0
    for n_sets in (1, 3, 70):
        adm, row_set, _ = set_families(P, n_sets)
        ids, ls, n_ok = check_masked_topk(P, adm, row_set, k)
        short += int((n_ok < k).sum())
        assert ((ids >= 0).sum(1) == np.minimum(n_ok, k)).all() and np.isinf(ls[ids < 0]).all()
        check_masked_topk(P, adm, row_set, k, with_known=False)
    assert short > 0 or k == 1 and B == 1
    kn = dict(known_off=P["off"], known_rc=P["rc"])
    uid, ul = H.topk_candidates(P["emb"], P["hr_t"], P["cand_t"], k, **kn, **P["kw"])
    for adm, row_set in ((np.ones((2, K), bool), np.arange(B, dtype=I32) % 2), (np.zeros((2, K), bool), np.full(B, -1, I32))):
        ids, ls, _ = check_masked_topk(P, adm, row_set, k)
        assert np.array_equal(ids, uid.cpu().numpy()) and np.array_equal(ls.view(I32), ul.cpu().numpy().view(I32))


def test_masked_topk_over_several_candidate_ranges():
    """B = 3, K = 700: one row block cut into six candidate ranges whose partial lists meet in the merge."""
    P = prepare(make_problem(800, 64, 700, 3, "tail", "complex", seed=21))
    for k in (1, 5, 128):
        adm, row_set, _ = set_families(P, 70)
        check_masked_topk(P, adm, row_set, k)
        adm, row_set, _ = set_families(P, 1)
        check_masked_topk(P, adm, np.zeros(3, I32), k)


def test_masked_topk_single_range_many_row_blocks():
    """256 row blocks (no candidate ranges), d = 56, K = 130."""
    B = 256 * 128
    P = make_problem(700, 56, 130, B, "head", "complex", seed=33)
    P["known"] = np.zeros((B, 130), bool)
    P["known"][::3, ::5] = True
    prepare(P)
    adm, row_set, _ = set_families(P, 70)
    ids, _, n_ok = check_masked_topk(P, adm, row_set, 5)
    assert (n_ok < 5).any() and (n_ok >= 5).any()


# ------------------------------------------------------------------ the mask builders
@pytest.mark.parametrize("K,n_sets,n_class", [(1, 1, 1), (33, 3, 33), (130, 70, 64), (417, 5, 70), (14951, 7, 3)])
def test_mask_builders_equal_numpy(K, n_sets, n_class):
    from graphembeddings_amd import _lib
    rng = np.random.default_rng(K + n_sets)
    S = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    W = int(lib.ge_candidate_mask_words(K))
    assert W == words(K)
    # classes: some outside [0, n_class) on both sides
    cls = rng.integers(-2, n_class + 2, K).astype(I32)
    allow_b = rng.random((n_sets, n_class)) < 0.4
    aw = (n_class + 31) // 32
    full = np.zeros((n_sets, aw * 32), bool)
    full[:, :n_class] = allow_b
    allow = np.packbits(full, axis=1, bitorder="little").view(U32).reshape(n_sets, aw)
    ok = (cls >= 0) & (cls < n_class)
    adm = np.zeros((n_sets, K), bool)
    adm[:, ok] = allow_b[:, cls[ok]]
    mask = torch.full((n_sets, W), -1, dtype=torch.int32, device="cuda")
    c_t, a_t = dev(cls), dev(allow.view(I32))
    assert int(lib.ge_candidate_mask_from_classes(c_t.data_ptr(), K, a_t.data_ptr(), n_sets, n_class, mask.data_ptr(), S)) == 0
    assert np.array_equal(mask.cpu().numpy().view(U32), pack(adm))
    # cells: duplicates and pairs outside [0, n_sets) x [0, K) on every side
    M = 5 * K + 7
    cells = np.stack([rng.integers(-1, n_sets + 1, M), rng.integers(-1, K + 40, M)], 1).astype(I32)
    cells[:3] = [[0, K - 1], [n_sets - 1, 0], [2 ** 30, 2 ** 30]]
    inside = (cells[:, 0] >= 0) & (cells[:, 0] < n_sets) & (cells[:, 1] >= 0) & (cells[:, 1] < K)
    adm = np.zeros((n_sets, K), bool)
    adm[cells[inside, 0], cells[inside, 1]] = True
    mask.fill_(-1)                                                              # the entry point zeroes it first
    ce_t = dev(cells)
    assert int(lib.ge_candidate_mask_from_cells(ce_t.data_ptr(), M, n_sets, K, mask.data_ptr(), S)) == 0
    assert np.array_equal(mask.cpu().numpy().view(U32), pack(adm))
    assert int(lib.ge_candidate_mask_from_cells(None, 0, n_sets, K, mask.data_ptr(), S)) == 0
    assert not mask.cpu().numpy().any()


def test_candidate_sets_builders_on_the_device():
    from graphembeddings_amd import evaluate as E
    rng = np.random.default_rng(4)
    R, N = 6, 500
    cand = rng.permutation(np.arange(R, N))[:417]
    pos = {int(c): i for i, c in enumerate(cand)}
    triples = np.stack([rng.integers(R, N, 900), rng.integers(R, N, 900), rng.integers(0, R - 1, 900)], 1)   # relation 5 unseen
    types = rng.integers(-1, 40, N)
    for side, col in (("tail", 1), ("head", 0)):
        obs = np.zeros((R, len(cand)), bool)
        ty = np.zeros((R, len(cand)), bool)
        for t in triples:
            if int(t[col]) in pos:
                obs[t[2], pos[int(t[col])]] = True
            if types[t[col]] >= 0:
                ty[t[2]] |= types[cand] == types[t[col]]
        cs = E.CandidateSets.from_observed(cand, triples, R, side)
        assert np.array_equal(cs.mask.cpu().numpy().view(U32), pack(obs)) and np.array_equal(cs.counts, obs.sum(1))
        cs = E.CandidateSets.from_types(cand, types, triples, R, side)
        assert np.array_equal(cs.mask.cpu().numpy().view(U32), pack(ty)) and np.array_equal(cs.counts, ty.sum(1))
        assert cs.n_sets == R and cs.counts[R - 1] == 0
    lists = {0: cand[:5], 3: cand[100:300], 4: []}
    cs = E.CandidateSets.from_lists(cand, lists, n_sets=6)
    adm = np.zeros((6, len(cand)), bool)
    adm[0, :5] = True
    adm[3, 100:300] = True
    assert np.array_equal(cs.mask.cpu().numpy().view(U32), pack(adm)) and np.array_equal(cs.counts, adm.sum(1))
    rs = torch.tensor([0, 3, -1, 4], device="cuda")
    assert np.array_equal(cs.admissible(rs).cpu().numpy(), rows_of(adm, rs.cpu().numpy()))
    p = torch.tensor([4, 99, 7, 0], device="cuda")
    assert cs.admissible(rs, p).cpu().tolist() == [True, False, True, False]


# ------------------------------------------------------------------ the evaluator and the driver
def _order_is_stable(losses, tpos, skip, k, tol=1e-6):
    """(rows whose rank, rows whose first k pops) cannot depend on which kernel computed the losses: two kernels' losses
    differ by less than 3e-7 (include/ge_hip.h), so the true entity's rank is fixed when no other loss lies within tol of
    its loss, and the first k pops when the k + 1 smallest eligible losses are more than tol apart."""
    L = losses.astype(np.float64)
    near = np.abs(L - L[np.arange(len(L)), tpos][:, None]) < tol
    near[np.arange(len(L)), tpos] = False
    s = np.sort(np.where(skip, np.inf, L), axis=1)[:, :k + 1]
    with np.errstate(invalid="ignore"):
        close = (np.diff(s, axis=1) < tol) & np.isfinite(s[:, 1:])
    return ~near.any(1), ~close.any(1)


@pytest.mark.parametrize("d", [48, 64])
@pytest.mark.parametrize("side", ["tail", "head"])
def test_link_prediction_and_predictions_fused_against_fallback(d, side):
    """d = 64: the masked sweep; d = 48: the stored losses of the fp32 rank kernel; fused=False: score_candidates' losses
    in chunks of 1024 rows.  Each path against numpy over its own losses; the paths against each other on the rows whose
    order cannot depend on the last bits of a loss."""
    from graphembeddings_amd import evaluate as E
    from graphembeddings_amd import hole as H
    rng = np.random.default_rng(d)
    R, N, B, K, k = 4, 500, 1100, 300, 10                   # (1100 rows: two chunks of the fallback)
    table = (rng.standard_normal((N, d)) * 0.2).astype(F32)
    emb = torch.as_tensor(table).cuda()
    cand = rng.permutation(np.arange(R, N))[:K]
    fixed, rel, true = rng.integers(R, N, B), rng.integers(0, R, B), rng.choice(cand, B)
    test = np.stack([fixed, true, rel], 1) if side == "tail" else np.stack([true, fixed, rel], 1)
    rows = np.repeat(np.arange(B), 20)
    kn = np.stack([fixed[rows], rng.choice(cand, rows.size), rel[rows]], 1)
    if side == "head":
        kn = kn[:, [1, 0, 2]]
    adm = rng.random((R + 1, K)) < 0.5
    adm[R] = False
    cs = E.CandidateSets(dev(cand.astype(I32)), dev(pack(adm).view(I32)), adm.sum(1))
    row_sets = rel.copy()
    row_sets[::11] = -1
    row_sets[5::13] = R                                      # the empty set
    a_rows = rows_of(adm, row_sets)
    known = np.zeros((B, K), bool)                          # (rows that share (fixed, relation) share their known cells)
    pos = {int(c): i for i, c in enumerate(cand)}
    by_query = {}
    for f, c, r in zip(fixed[rows], kn[:, 1 if side == "tail" else 0], rel[rows]):
        by_query.setdefault((int(f), int(r)), set()).add(pos[int(c)])
    for i in range(B):
        known[i, sorted(by_query[(int(fixed[i]), int(rel[i]))])] = True
    tpos = np.array([pos[int(t)] for t in true])
    hq, cq = dev(np.stack([fixed, rel], 1).astype(I32)), dev(cand.astype(I32))
    out = {}
    for fused in (True, False):
        raw, fil, admt = E.link_prediction_ranks(emb, test, cand, kn, side, fused=fused, candidate_sets=cs, row_sets=row_sets,
                                                 return_admissible=True)
        if fused:
            losses = H.rank_candidates(emb, hq, dev(true.astype(I32)), cq, cand_is_head=(side == "head"), return_scores=True)[-1]
        else:
            losses = H.score_candidates(emb, hq, cq, cand_is_head=(side == "head"))
        losses = losses.cpu().numpy()
        tl = losses[np.arange(B), tpos]
        before = ((losses < tl[:, None]) | ((losses == tl[:, None]) & (cand[None, :] < true[:, None]))) & a_rows
        assert np.array_equal(raw, before.sum(1) + 1) and np.array_equal(fil, raw - (before & known).sum(1))
        assert np.array_equal(admt, a_rows[np.arange(B), tpos])
        q = np.stack([fixed, rel], 1)
        if d == 48 and fused:
            with pytest.raises(ValueError):
                E.predict_links(emb, q, cand, k, known_triples=kn, side=side, fused=True, candidate_sets=cs, row_sets=row_sets)
            ids = None
        else:
            ids, ls = E.predict_links(emb, q, cand, k, known_triples=kn, side=side, fused=fused, candidate_sets=cs,
                                      row_sets=row_sets)
            eid, el = topk_oracle(losses, cand, k, known | ~a_rows)
            assert np.array_equal(ids, eid) and np.array_equal(ls.view(I32), el.view(I32))
            assert (ids[row_sets == R] == -1).all()
        out[fused] = (raw, fil, ids) + _order_is_stable(losses, tpos, known | ~a_rows, k)
    stable = out[True][3] & out[False][3]
    assert stable.mean() > 0.5
    assert np.array_equal(out[True][0][stable], out[False][0][stable]) and np.array_equal(out[True][1][stable], out[False][1][stable])
    if out[True][2] is not None:
        stable = out[True][4] & out[False][4]
        assert stable.mean() > 0.5
        assert np.array_equal(out[True][2][stable], out[False][2][stable])
    # k above the kernel's 128: the sweep's stored losses, masked on the host
    if d == 64:
        ids, ls = E.predict_links(emb, q[:200], cand, 150, known_triples=kn, side=side, candidate_sets=cs, row_sets=row_sets[:200])
        losses = H.rank_candidates(emb, hq[:200], dev(true[:200].astype(I32)), cq, cand_is_head=(side == "head"), return_scores=True)[-1]
        eid, el = topk_oracle(losses.cpu().numpy(), cand, 150, (known | ~a_rows)[:200])
        assert np.array_equal(ids, eid) and np.array_equal(ls.view(I32), el.view(I32))
    with pytest.raises(ValueError):
        E.link_prediction_ranks(emb, test, cand, kn, side, candidate_sets=cs, row_sets=np.full(B, R + 1))
    with pytest.raises(ValueError):
        E.link_prediction_ranks(emb, test, cand[:-1], kn, side, candidate_sets=cs)
    with pytest.raises(ValueError):
        E.predict_links(emb, q, cand, k, side=side, candidate_sets=cs, row_sets=row_sets[:5])


def _toy_kg(tmp_path, n_ent=120, gsz=6, seed=0):
    """tests/test_gpu_train_eval.py's learnable toy KG, with four entity types: groups of six linked inside (relation 0)
    and to the next group (relation 1); the type follows the position in the group, so relation 1 links equal types."""
    rng = np.random.default_rng(seed)
    R = 2
    rows = [(i, f"r{i}", f"r{i}", "RELATION") for i in range(R)]
    rows += [(R + e, f"e{e}", f"e{e}", "ABCD"[(e % gsz) % 4]) for e in range(n_ent)]
    with open(tmp_path / "entity_metadata.tsv", "w") as f:
        f.write("Index\tId\tName\tType\n")
        for r in rows:
            f.write("\t".join(str(x) for x in r) + "\n")
    (tmp_path / "relation_ids.txt").write_text("".join(f"r{i}\t{i}\n" for i in range(R)))
    r0, r1 = [], []
    ng = n_ent // gsz
    for g in range(ng):
        mem = [R + g * gsz + i for i in range(gsz)]
        r0 += [[a, b, 0] for a in mem for b in mem if a != b]
        r1 += [[R + g * gsz + i, R + ((g + 1) % ng) * gsz + i, 1] for i in range(0, gsz, 2)]    # types A and C only
    r0 = np.array(r0, dtype=np.int64)
    rng.shuffle(r0)
    r1 = np.array(r1, dtype=np.int64)
    rng.shuffle(r1)
    n_test, n_valid = 40, 64
    np.savetxt(tmp_path / "test_positive_triples.txt", np.concatenate([r0[:n_test], r1[:10]]), fmt="%d", delimiter="\t")
    np.savetxt(tmp_path / "triples-valid.txt", r0[n_test:n_test + n_valid], fmt="%d", delimiter="\t")
    train = np.concatenate([r0[n_test + n_valid:], r1[10:]])
    rng.shuffle(train)
    np.savetxt(tmp_path / "triples.txt", train, fmt="%d", delimiter="\t")
    return str(tmp_path)


@pytest.mark.parametrize("kind", ["types", "observed"])
def test_driver_candidate_sets(tmp_path, kind, capsys):
    """train.py --infer --candidate_sets: the `constrained` block is the API's over sets built from train + valid, the usual
    numbers are unchanged, and with --predict_k no predicted tail lies outside its relation's set."""
    from graphembeddings_amd import data as D
    from graphembeddings_amd import evaluate as E
    from graphembeddings_amd import train as T
    dd = tmp_path / "data"
    dd.mkdir()
    data_dir = _toy_kg(dd)
    out = str(tmp_path / "run")
    argv = ["--data_dir", data_dir, "--output_dir", out, "--batch_size", "64", "--embedding_dim", "64",
            "--num_epochs", "20", "--learning_rate", "0.5", "--margin", "0.5", "--padded_size", "64", "--seed", "1"]
    T.run_training(D.init_data(data_dir), T.build_parser().parse_args(argv), log=lambda *a: None)
    infer = argv + ["--infer", "--infer_threshold", "0.9"]
    m0 = T.infer_triples(T.build_parser().parse_args(infer), log=lambda *a: None)
    capsys.readouterr()
    m1 = T.infer_triples(T.build_parser().parse_args(infer + ["--candidate_sets", kind, "--predict_k", "3"]), log=lambda *a: None)
    assert "constrained:" in capsys.readouterr().out
    block = m1.pop("constrained")
    assert m0 == m1
    data = D.init_inference_data(data_dir)
    emb, _ = T.load_checkpoint(out)
    R, N = data.relation_count, data.entity_count
    cand = np.arange(R, N)
    known = np.concatenate([data.triples, data.validation_triples])
    raw, fil, adm, size = [], [], [], []
    sets = {}
    for side in ("tail", "head"):
        sets[side] = cs = (E.CandidateSets.from_types(cand, data.type_arrays()[1], known, R, side) if kind == "types"
                           else E.CandidateSets.from_observed(cand, known, R, side))
        r, f, a = E.link_prediction_ranks(emb, data.test_array, cand, known, side, candidate_sets=cs, return_admissible=True)
        raw.append(r); fil.append(f); adm.append(a); size.append(cs.counts[data.test_array[:, 2]])
    assert block["mrr_and_hits"] == E.mrr_and_hits(np.concatenate(raw), np.concatenate(fil))
    assert block["admissible_true"] == float(np.concatenate(adm).mean())
    assert block["mean_set_size"] == float(np.concatenate(size).mean())
    # the sets restrict: relation 1 links entities of types A and C only
    assert sets["tail"].counts[1] < len(cand) and sets["tail"].counts[1] > 0
    # the sets, by hand, and every predicted tail inside its relation's
    col = 1
    seen = {r: set() for r in range(R)}
    for t in known:
        seen[int(t[2])].add(int(t[col]) if kind == "observed" else data.id_to_type[int(t[col])])
    lines = open(os.path.join(out, "inference_results.tsv")).read().splitlines()
    assert len(lines) > 0
    for line in lines:
        _, h, t, r, _ = line.split("\t")
        assert (int(t) if kind == "observed" else data.id_to_type[int(t)]) in seen[int(r)], line
    # against the API: the first pops of every confident query come from predict_links with the tail sets
    hr_all = data.test_array[:, [0, 2]]
    _, first = np.unique(hr_all, axis=0, return_index=True)
    queries = hr_all[np.sort(first)]
    ids, ls = E.predict_links(emb, queries, cand, 1, side="tail", candidate_sets=sets["tail"])
    firsts = {}
    for line in lines:
        l, h, t, r, _ = line.split("\t")
        firsts.setdefault((int(h), int(r)), int(t))
    for i, (h, r) in enumerate(queries):
        if ids[i, 0] >= 0 and ls[i, 0] < 0.9:
            assert firsts[(int(h), int(r))] == ids[i, 0]
        else:
            assert (int(h), int(r)) not in firsts
