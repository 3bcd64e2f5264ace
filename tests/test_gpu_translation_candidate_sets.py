"""GPU: per-relation candidate sets on the translation models' sweeps over every entity -- ge_transx_rank_masked,
ge_transr_rank_masked, ge_transx_topk_masked, ge_transr_topk_masked and the Python layers above them.

The oracle (tests/translation_sets_ref.py; torch on the device for the one large case) works over the distances the
UNMASKED ge_transx_rank / ge_transr_rank store in scores_out for the same inputs: every integer equal, every float
bitwise equal.  The entity tables hold duplicated rows, so exact ties and the (D, id) tie-break are exercised."""
import json

import numpy as np
import pytest
import torch

from graphembeddings_amd import _lib, evaluate as EV
from graphembeddings_amd.transr import TransR
from graphembeddings_amd.transx import TransX
from tests import translation_rank_ref as RK
from tests import translation_sets_ref as REF

pytestmark = pytest.mark.gpu

I32, I64 = np.int32, np.int64
MODELS = ("transe", "transh", "transd", "transr")
N_REL = 5


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def cells(known):
    """ge_known_cells' lists of a [B, E] bool mask on the device (the uint16 cells as int16 bits, as KnownIndex.cells)."""
    off, rc = REF.cells_from_mask(known)
    return dev(off), dev(rc.view(np.int16))


def make_model(name, E, l1, d, seed=0, R=N_REL):
    """d = 8: the VEC = 4 sweep (TransR 8 x 12); d = 6: the VEC = 1 sweep (TransR 6 x 5).  Entities 3, 4, 5 are one
    row (a run of tied duplicates), E - 1 is a copy of entity 0 and E - 2 of entity 1."""
    if name == "transr":
        m = TransR(E, R, dim_e=d, dim_r=12 if d == 8 else 5, l1=l1, seed=seed)
    else:
        m = TransX(name, E, R, d, l1=l1, seed=seed)
    for t in m.tables.values():
        if t.shape[0] != E:
            continue
        if E >= 6:
            t[4], t[5] = t[3], t[3]
        if E >= 12:
            t[E - 1], t[E - 2] = t[0], t[1]
    return m


def make_sets(E, rng, targets):
    """bool [8, E]: 0 empty (its pad bits are packed as ones and set 1's row starts with ones: a read past a mask row, or
    a use of bits >= E, changes a count) | 1 full | 2 one bit that is no row's true entity (where E allows) | 3 half, with
    exactly one member (4) of the tied run 3, 4, 5 | 4 density 0.02 | 5 density 0.5 | 6 density 1.0 | 7 half."""
    adm = np.zeros((8, E), bool)
    adm[1] = True
    free = np.setdiff1d(np.arange(E), targets)
    adm[2, free[len(free) // 2] if len(free) else 0] = True
    adm[3] = rng.random(E) < 0.5
    if E >= 6:
        adm[3, 3:6] = (False, True, False)
    adm[4] = rng.random(E) < 0.02
    adm[5] = rng.random(E) < 0.5
    adm[6] = rng.random(E) < 1.0
    adm[7] = rng.random(E) < 0.5
    return adm


def make_rows(E, B, rng, side):
    tri = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, N_REL, B)], 1).astype(I32)
    if E >= 6 and B >= 3:
        tri[1, :2] = (4, 4)                                   # the true entity inside the tied run
        tri[2, :2] = (5, 3)
    tri = tri[np.argsort(tri[:, 2], kind="stable")]           # grouped by relation, as the host layers pass them
    target = tri[:, 0] if side == "head" else tri[:, 1]
    fixed = tri[:, 1] if side == "head" else tri[:, 0]
    return tri, fixed.astype(I64), target.astype(I64)


def stored(m, tri, head, koff=None, krc=None):
    """The unmasked entry point on the same rows: (n_before, n_known_before, true_dist, scores_out) numpy."""
    nb, nk, td, sc = m.rank_counts(dev(tri), cand_is_head=head, known_off=koff, known_rc=krc, return_scores=True)
    return nb.cpu().numpy(), nk.cpu().numpy(), td.cpu().numpy(), sc.cpu().numpy()


def check_ranks(m, tri, head, target, sc, td0, adm, row_set, mask_t, known, koff, krc):
    rs_t = dev(row_set.astype(I32))
    outs = []
    for _ in range(2):                                        # two identical calls agree bitwise
        nb, nk, td = m.rank_counts(dev(tri), cand_is_head=head, known_off=koff, known_rc=krc, row_set=rs_t, mask=mask_t)
        outs.append((nb.cpu().numpy(), nk.cpu().numpy(), td.cpu().numpy()))
    for a, b in zip(*outs):
        assert np.array_equal(a.view(I32), b.view(I32))
    nb, nk, td = outs[0]
    enb, enk, bad = REF.masked_counts(sc, target, adm, row_set, known if koff is not None else None)
    assert np.array_equal(nb, enb), (nb, enb)
    assert np.array_equal(nk, enk), (nk, enk)
    assert np.isnan(td[bad]).all()
    assert np.array_equal(td[~bad].view(I32), td0[~bad].view(I32))
    assert np.array_equal(td0.view(I32), sc[np.arange(len(tri)), target].view(I32))
    return nb, nk


def check_topk(m, fixed, rel, head, k, sc, adm, row_set, mask_t, known, koff, krc):
    q = dev(np.stack([fixed, rel], 1).astype(I32))
    rs_t = dev(row_set.astype(I32))
    outs = []
    for _ in range(2):
        ids, dist = m.topk_candidates(q, k, cand_is_head=head, known_off=koff, known_rc=krc, row_set=rs_t, mask=mask_t)
        outs.append((ids.cpu().numpy(), dist.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1].view(I32), outs[1][1].view(I32))
    eid, ed = REF.masked_topk(sc, k, adm, row_set, known if koff is not None else None)
    assert np.array_equal(outs[0][0], eid)
    assert np.array_equal(outs[0][1].view(I32), ed.view(I32))
    return outs[0]


# (n_ent, B, d): n_ent around the 256-candidate source block (at 300 a mask row has 12 words while the second source
# block spans words 8 .. 15; at 513 a third block holds one entity), B around the 16-row chunk and the 128-row tile of
# the known cells, d = 8 -> VEC 4, d = 6 -> VEC 1
SHAPES = [(1, 1, 8), (255, 15, 6), (256, 16, 8), (257, 17, 6), (300, 130, 8), (513, 17, 6), (300, 1, 6), (513, 130, 8)]


@pytest.mark.parametrize("side", ["tail", "head"])
@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("model", MODELS)
def test_masked_sweeps_equal_the_oracle_over_stored_distances(model, l1, side):
    """Every shape: chunks that mix several sets, -1 and real sets, and (B >= 15) bad set indices next to good rows; the
    empty, one-bit, tied-run, full and 0.02 / 0.5 / 1.0 sets; known cells at density 0.1; true entities inside and outside
    their sets; top-k at k = 1, 5, 128 with rows that have fewer than k admissible candidates.  Then the same rows with
    every bit set and with row_set = -1 everywhere: bitwise the unmasked entry points' outputs."""
    head = side == "head"
    for E, B, d in SHAPES:
        rng = np.random.default_rng(1000 * E + B + d)
        m = make_model(model, E, l1, d, seed=E + B)
        tri, fixed, target = make_rows(E, B, rng, side)
        adm = make_sets(E, rng, target)
        n_sets = adm.shape[0]
        mask_t = dev(REF.pack(adm, pad=True).view(I32))
        assert mask_t.shape == (n_sets, int(_lib.load().ge_candidate_mask_words(E)))
        row_set = rng.integers(-1, n_sets, B)
        row_set[:min(B, n_sets)] = rng.permutation(n_sets)[:min(B, n_sets)]   # every set is some row's
        if B >= 15:
            row_set[[3, 9]] = (n_sets, -2)                    # bad indices next to good rows
        known = rng.random((B, E)) < 0.1
        koff, krc = cells(known)
        nb0, nk0, td0, sc = stored(m, tri, head, koff, krc)
        inside = REF.admitted(adm, row_set)[np.arange(B), target]
        if B >= 15:
            assert inside.any() and not inside.all()          # true entities admissible and not
        for ko, kr in ((koff, krc), (None, None)):
            check_ranks(m, tri, head, target, sc, td0, adm, row_set, mask_t, known, ko, kr)
            for k in (1, 5, 128):
                check_topk(m, fixed, tri[:, 2], head, k, sc, adm, row_set, mask_t, known, ko, kr)
        # every bit set / no row restricted: the unmasked entry points, called here, bit for bit
        full_t = dev(REF.pack(np.ones((n_sets, E), bool), pad=True).view(I32))
        free = np.full(B, -1)
        good = np.where(REF.bad_rows(row_set, n_sets), 0, row_set)
        for rs, mk in ((good, full_t), (free, mask_t)):
            rs_t = dev(rs.astype(I32))
            nb, nk, td = m.rank_counts(dev(tri), cand_is_head=head, known_off=koff, known_rc=krc, row_set=rs_t, mask=mk)
            assert np.array_equal(nb.cpu().numpy(), nb0) and np.array_equal(nk.cpu().numpy(), nk0)
            assert np.array_equal(td.cpu().numpy().view(I32), td0.view(I32))
            q = dev(np.stack([fixed, tri[:, 2]], 1).astype(I32))
            for k in (1, 128):
                a = m.topk_candidates(q, k, cand_is_head=head, known_off=koff, known_rc=krc, row_set=rs_t, mask=mk)
                b = m.topk_candidates(q, k, cand_is_head=head, known_off=koff, known_rc=krc)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


@pytest.mark.parametrize("model", MODELS)
def test_topk_candidate_j_has_masked_filtered_rank_j_plus_1(model):
    """The j-th candidate of the masked top-k, ranked as the true entity by the masked rank entry with the same sets and
    known cells, has n_before - n_known_before = j."""
    E, B, d, k = 300, 40, 8, 5
    rng = np.random.default_rng(5)
    m = make_model(model, E, True, d, seed=3)
    tri, fixed, target = make_rows(E, B, rng, "tail")
    adm = make_sets(E, rng, target)
    mask_t = dev(REF.pack(adm, pad=True).view(I32))
    row_set = rng.integers(-1, adm.shape[0], B)
    known = rng.random((B, E)) < 0.1
    koff, krc = cells(known)
    sc = stored(m, tri, False)[3]
    ids, _ = check_topk(m, fixed, tri[:, 2], False, k, sc, adm, row_set, mask_t, known, koff, krc)
    rows, js = np.nonzero(ids >= 0)
    assert len(rows) > B                                      # (most rows return k candidates; the empty set none)
    tri2 = np.stack([fixed[rows], ids[rows, js], tri[rows, 2]], 1).astype(I32)
    k2off, k2rc = cells(known[rows])
    nb, nk, _ = m.rank_counts(dev(tri2), known_off=k2off, known_rc=k2rc, row_set=dev(row_set[rows].astype(I32)), mask=mask_t)
    assert np.array_equal((nb - nk).cpu().numpy(), js)


@pytest.mark.parametrize("model", ["transe", "transr"])
def test_nan_entity_flags_a_topk_row_only_where_admissible_and_not_known(model):
    E, d, k = 300, 8, 5
    m = make_model(model, E, False, d, seed=9)
    m.tables["ent"][10] = float("nan")
    adm = np.ones((3, E), bool)
    adm[1, 10] = False                                        # set 1 does not admit the NaN entity
    adm[2, :] = False
    adm[2, [10, 11]] = True
    fixed = np.array([20, 21, 22, 23, 24, 25], I64)
    rel = np.array([0, 0, 1, 1, 2, 2], I64)
    row_set = np.array([0, 1, 0, -1, 2, 1])
    known = np.zeros((6, E), bool)
    known[2, 10] = True                                       # row 2 admits entity 10 but knows it
    known[0, 11] = True
    koff, krc = cells(known)
    tri = np.stack([fixed, np.full(6, 30), rel], 1).astype(I32)
    sc = stored(m, tri, False)[3]
    assert np.isnan(sc[:, 10]).all() and not np.isnan(np.delete(sc, 10, 1)).any()
    mask_t = dev(REF.pack(adm, pad=True).view(I32))
    ids, dist = check_topk(m, fixed, rel, False, k, sc, adm, row_set, mask_t, known, koff, krc)
    flagged = np.isnan(dist).all(1)
    assert flagged.tolist() == [True, False, False, True, True, False]
    assert (ids[flagged] == -1).all() and (ids[~flagged][:, 0] >= 0).all()


@pytest.mark.parametrize("side", ["tail", "head"])
@pytest.mark.parametrize("model", ["transe", "transr"])
def test_masked_topk_with_two_merge_rounds(model, side):
    """n_ent = 4,353: 18 source blocks (the 18th holds one entity), so 18 candidate ranges for one or two row chunks and
    two merge rounds, 18 -> 2 -> 1, through the merge loop that the masked and the unmasked top-k share."""
    E, d, head = 4353, 8, side == "head"
    for B in (1, 17):
        rng = np.random.default_rng(7 * B + head)
        m = make_model(model, E, True, d, seed=B)
        tri, fixed, target = make_rows(E, B, rng, side)
        adm = make_sets(E, rng, target)
        n_sets = adm.shape[0]
        mask_t = dev(REF.pack(adm, pad=True).view(I32))
        row_set = rng.integers(-1, n_sets, B)
        row_set[:min(B, n_sets)] = rng.permutation(n_sets)[:min(B, n_sets)]
        known = rng.random((B, E)) < 0.1
        koff, krc = cells(known)
        sc = stored(m, tri, head)[3]
        full_t = dev(REF.pack(np.ones((n_sets, E), bool), pad=True).view(I32))
        q = dev(np.stack([fixed, tri[:, 2]], 1).astype(I32))
        for k in (1, 128):
            check_topk(m, fixed, tri[:, 2], head, k, sc, adm, row_set, mask_t, known, koff, krc)
            a = m.topk_candidates(q, k, cand_is_head=head, known_off=koff, known_rc=krc, row_set=dev(row_set.astype(I32)),
                                  mask=full_t)
            b = m.topk_candidates(q, k, cand_is_head=head, known_off=koff, known_rc=krc)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def block_sets(E, rng):
    """Sets with a chosen number of admissible entities in every 256-entity source block (per_block[s][b]); None: the
    whole block."""
    n_cb = (E + 255) // 256
    last = n_cb - 1
    per_block = [
        [128] * n_cb,                                         # 0: the queue reaches exactly 256 on every second block
        [128] * (last - (last % 2)) + [0] * (n_cb - last + (last % 2)),   # 1: ... and the last blocks add nothing
        [200] * n_cb,                                         # 2: entries carried over from block to block
        [5] * n_cb,                                           # 3: sparse: one partial flush at the end
        [None] * n_cb,                                        # 4: full
        [0] * n_cb,                                           # 5: empty
    ]
    adm = np.zeros((len(per_block), E), bool)
    for s, counts in enumerate(per_block):
        for b, n in enumerate(counts):
            lo, hi = b * 256, min(E, b * 256 + 256)
            ids = np.arange(lo, hi)
            adm[s, ids if n is None else rng.permutation(ids)[:min(n, hi - lo)]] = True
    return adm


def test_compaction_edges_many_rows_on_the_device():
    """The queue's own edges need a workgroup that walks several source blocks, which the grid rule gives only to many
    rows: gridDim.y = ceil(2 * 2048 / n_chunks) (ranks) or ceil(2048 / n_chunks) (top-k), n_chunks = ceil(B / 16).
      ranks  B = 16,400, n_ent = 2,400: n_chunks = 1,025, gridDim.y = 4 over 10 source blocks -- the workgroups y = 0, 1
             walk three blocks (y, y + 4, y + 8), y = 2, 3 two;
      top-k  B = 16,400, n_ent = 1,100: gridDim.y = 2 over 5 blocks -- y = 0 walks blocks 0, 2, 4 and y = 1 blocks 1, 3.
    Every chunk of 16 rows names ONE set (a chunk's queue holds the union of its rows' sets), from block_sets:
      set 0  128 per block: the queue holds exactly 256 after the second block (one full batch, nothing carried), then
             the third block leaves a partial flush; with two blocks the run ends on an EMPTY flush
      set 1  the same, but nothing in the last blocks: three-block workgroups end on an empty flush too
      set 2  200 per block: 200 -> 400 (batch, 144 carried) -> 344 (batch, 88 carried) -> partial flush
      set 3  5 per block: no batch before the flush;  set 4 full: a batch per block;  set 5 empty: nothing at all.
    Some chunks mix sets and -1 rows.  The oracle runs in torch on the device over the unmasked sweep's stored distances;
    d = 8 (VEC 4), TransE, L1."""
    B, d = 16400, 8
    g = torch.Generator().manual_seed(0)
    for what, E in (("rank", 2400), ("topk", 1100)):
        rng = np.random.default_rng(E)
        m = make_model("transe", E, True, d, seed=E)
        adm = block_sets(E, rng)
        n_sets = adm.shape[0]
        assert adm[0, :256].sum() == 128 and adm[2, 256:512].sum() == 200
        adm_t = dev(adm)
        mask_t = dev(REF.pack(adm, pad=True).view(I32))
        tri = torch.stack([torch.randint(0, E, (B,), generator=g), torch.randint(0, E, (B,), generator=g),
                           torch.zeros(B, dtype=torch.int64)], 1).to(torch.int32).cuda()
        chunk_set = torch.arange((B + 15) // 16) % n_sets
        row_set = chunk_set.repeat_interleave(16)[:B].clone()
        row_set[16 * 700:16 * 700 + 16] = torch.tensor([0, 0, 2, 2, -1, 3, 3, 5, 5, 5, 1, 1, 4, 0, 2, -1])   # mixed chunks
        row_set[16 * 701 + 3] = -1
        row_set[16 * 702 + 5] = 3
        row_set = row_set.cuda()
        rows = adm_t[row_set.clamp(min=0)] | (row_set < 0).view(-1, 1)
        nb0, _, td0, sc = m.rank_counts(tri, return_scores=True)
        rs_t = row_set.to(torch.int32).contiguous()
        if what == "rank":
            target = tri[:, 1].to(torch.int64)
            dt = sc.gather(1, target.view(-1, 1))
            before = (sc < dt) | ((sc == dt) & (torch.arange(E, device="cuda").view(1, -1) < target.view(-1, 1)))
            want = (before & rows).sum(1).to(torch.int32)
            nb, nk, td = m.rank_counts(tri, row_set=rs_t, mask=mask_t)
            assert torch.equal(nb, want) and int(nk.abs().max()) == 0
            assert torch.equal(td.view(torch.int32), td0.view(torch.int32))
            full = row_set == 4
            assert torch.equal(nb[full], nb0[full])
        else:
            k = 5
            q = tri[:, [0, 2]].contiguous()
            # ascending (D, id): D >= +0, so its bit pattern orders as the float does
            key = (sc.view(torch.int32).to(torch.int64) << 32) | torch.arange(E, device="cuda").view(1, -1)
            none = 2 ** 63 - 1                               # above every key: the bits of +inf << 32 are below it
            key = torch.where(rows & (sc < float("inf")), key, torch.full_like(key, none))
            top = torch.sort(key, dim=1).values[:, :k]
            pad = top == none
            want_id = torch.where(pad, torch.full_like(top, -1), top & 0xFFFFFFFF).to(torch.int32)
            want_bits = torch.where(pad, torch.full_like(top, 0x7F800000), top >> 32).to(torch.int32)
            ids, dist = m.topk_candidates(q, k, row_set=rs_t, mask=mask_t)
            assert torch.equal(ids, want_id)
            assert torch.equal(dist.view(torch.int32), want_bits)
            ids2, dist2 = m.topk_candidates(q, k, row_set=rs_t, mask=mask_t)
            assert torch.equal(ids, ids2) and torch.equal(dist.view(torch.int32), dist2.view(torch.int32))


# ------------------------------------------------------------------ the Python layer
def small_kg(E, rng, n_known=400, n_test=60):
    known = np.unique(np.stack([rng.integers(0, E, n_known), rng.integers(0, E, n_known),
                                rng.integers(0, N_REL, n_known)], 1), axis=0)
    test = np.stack([rng.integers(0, E, n_test), rng.integers(0, E, n_test), rng.integers(0, N_REL, n_test)], 1)
    return known, test


def observed_bits(E, triples, side):
    adm = np.zeros((N_REL, E), bool)
    adm[triples[:, 2], triples[:, 1 if side == "tail" else 0]] = True
    return adm


@pytest.mark.parametrize("model", ["transe", "transr"])
def test_python_layer_ranks_predict_and_evaluate(model):
    E, d = 300, 8
    rng = np.random.default_rng(11)
    m = make_model(model, E, True, d, seed=4)
    known, test = small_kg(E, rng)
    sets, cons = {}, {}
    for side in ("tail", "head"):
        head = side == "head"
        cs = EV.CandidateSets.from_observed(np.arange(E), known, N_REL, side)
        sets[side] = cs
        adm = observed_bits(E, known, side)
        assert np.array_equal(cs.counts, adm.sum(1))
        target = test[:, 0] if head else test[:, 1]
        sc = stored(m, test.astype(I32), head)[3]
        kmask = RK.known_mask(test, known, E, side)
        enb, enk, _ = REF.masked_counts(sc, target, adm, test[:, 2], kmask)
        raw, fil, inside = m.ranks(test, known, side=side, candidate_sets=cs, return_admissible=True)
        assert np.array_equal(raw, enb + 1) and np.array_equal(fil, enb + 1 - enk)
        assert np.array_equal(inside, adm[test[:, 2], target])
        cons[side] = (raw, fil, inside, cs.counts[test[:, 2]])
        # explicit row sets, -1 among them
        rs = rng.integers(-1, N_REL, len(test))
        enb, enk, _ = REF.masked_counts(sc, target, adm, rs, kmask)
        raw, fil = m.ranks(test, known, side=side, candidate_sets=cs, row_sets=rs)
        assert np.array_equal(raw, enb + 1) and np.array_equal(fil, enb + 1 - enk)
        # predict: fused, the stored-distance route, and k above the fused limit
        fixed = test[:, 1] if head else test[:, 0]
        queries = np.stack([fixed, test[:, 2]], 1)
        for k in (1, 5):
            eid, ed = REF.masked_topk(sc, k, adm, test[:, 2], kmask)
            for fused in (None, False):
                ids, dist = m.predict(queries, k, known, side=side, candidate_sets=cs, fused=fused)
                assert np.array_equal(ids, eid) and np.array_equal(dist.view(I32), ed.view(I32))
        ids128, d128 = m.predict(queries, 128, known, side=side, candidate_sets=cs, row_sets=rs)
        ids129, d129 = m.predict(queries, 129, known, side=side, candidate_sets=cs, row_sets=rs)
        assert np.array_equal(ids129[:, :128], ids128) and np.array_equal(d129[:, :128].view(I32), d128.view(I32))
        eid, ed = REF.masked_topk(sc, 129, adm, rs, kmask)
        assert np.array_equal(ids129, eid) and np.array_equal(d129.view(I32), ed.view(I32))
    plain = EV.evaluate_translation(m, test, known)
    res = EV.evaluate_translation(m, test, known, candidate_sets=sets)
    con = res.pop("constrained")
    assert res == plain
    raw, fil, inside, size = (np.concatenate([cons[s][i] for s in ("tail", "head")]) for i in range(4))
    want = EV.mrr_and_hits(raw, fil)
    assert {k: con[k] for k in want} == want
    assert con["admissible_true"] == float(inside.mean()) and con["mean_set_size"] == float(size.mean())


@pytest.mark.parametrize("driver", ["transx_train", "transr_train"])
def test_driver_writes_the_constrained_block(driver, tmp_path, capsys):
    import importlib
    mod = importlib.import_module("graphembeddings_amd." + driver)
    E, rng = 40, np.random.default_rng(2)
    known, test = small_kg(E, rng, n_known=200, n_test=12)
    extra = known[:50]
    data = tmp_path / "data"
    data.mkdir()
    (data / "entity2id.txt").write_text("%d\n" % E)
    (data / "relation2id.txt").write_text("%d\n" % N_REL)
    fmt = lambda t: "%d\n" % len(t) + "".join("%d %d %d\n" % tuple(r) for r in t)
    (data / "triple2id.txt").write_text(fmt(known[50:]))
    (tmp_path / "test2id.txt").write_text(fmt(test))
    (tmp_path / "valid2id.txt").write_text(fmt(extra))
    out = tmp_path / "out"
    dims = ["--hidden_size", "8"] if driver == "transx_train" else ["--hidden_size_e", "8", "--hidden_size_r", "12"]
    rc = mod.main(["--data_dir", str(data), "--output_dir", str(out), "--train_times", "1", "--nbatches", "2", *dims,
                   "--test_file", str(tmp_path / "test2id.txt"), "--filter_file", str(tmp_path / "valid2id.txt"),
                   "--candidate_sets", "observed", "--predict_k", "3"])
    assert rc == 0
    name = "transe" if driver == "transx_train" else "transr"
    res = json.load(open(out / (name + "_test.json")))
    con = res["constrained"]
    assert set(con) >= {"raw_mrr", "filtered_mrr", "hits10", "admissible_true", "mean_set_size"}
    sizes = {s: observed_bits(E, known, s).sum(1) for s in ("tail", "head")}    # triple2id.txt + the filter file
    assert con["mean_set_size"] == pytest.approx(np.concatenate([sizes[s][test[:, 2]] for s in ("tail", "head")]).mean())
    printed = capsys.readouterr().out
    assert "constrained: raw MRR" in printed and printed.index("constrained:") > printed.index("both:")
    # the predictions come from the relation's set only
    for line in open(out / (name + "_predict.tsv")):
        side, f, r, pos, c, dist, in_test = line.split("\t")
        assert observed_bits(E, known, side)[int(r), int(c)]
