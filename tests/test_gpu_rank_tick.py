"""GPU: ge_rank_validation_tick and evaluate.RankPocket on a random table of 8 relation rows plus 292 entities (K = 292,
three 128-candidate tiles with a ragged last one) and random known triples.

V in {1, 127, 128, 129, 300}: one row, the sweeps' 128-row block with its neighbours, three blocks a side.  d = 64 runs the
split-precision sweep on the tick's planes; the one case at d = 32 takes the fp32 route with planes NULL, unmasked.

Metrics: the tick's eight numbers against evaluate.mrr_and_hits of evaluate.link_prediction_ranks over both sides on the
same inputs, within the bounds of tests/rank_tick_ref.py (entries 2-7 exactly float32 of the reference, the two MRRs
within 2^-23): the tick's counts are the rank entry points' bit for bit, so only the summary's arithmetic differs."""
import functools

import numpy as np
import pytest
import torch

from graphembeddings_amd import _lib
from graphembeddings_amd import evaluate as EV
from graphembeddings_amd import hole as H
from tests import rank_tick_ref as RT

pytestmark = pytest.mark.gpu

I32, I64, F32 = np.int32, np.int64, np.float32
R, N, K = 8, 300, 292
CAND = np.arange(R, N, dtype=I32)
VS = [1, 127, 128, 129, 300]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def graph():
    """(known [2300,3], valid [300,3]) int64 (head, tail, relation): random triples over the entity rows; the validation
    triples are known too, as train + valid is the evaluation's filter."""
    rng = np.random.default_rng(7)
    tri = np.unique(np.stack([rng.integers(R, N, 2600), rng.integers(R, N, 2600), rng.integers(0, R, 2600)], 1), axis=0)
    tri = tri[rng.permutation(len(tri))][:2300].astype(I64)
    return tri, tri[:300].copy()


def table(d, seed=0, scale=0.2):
    t = (np.random.default_rng(seed).standard_normal((N, d)) * scale).astype(F32)
    t[::5] *= 6.0                                            # a fifth of the rows outside the unit ball: the clip
    return t


def reference(emb, valid, sets=None, valid_head=None):
    """(metrics [8] float64 in the tick's order, raw, fil) of link_prediction_ranks over both sides (valid_head: other
    triples on the head side)."""
    known = graph()[0]
    raw, fil = [], []
    for side, rows in (("tail", valid), ("head", valid if valid_head is None else valid_head)):
        r, f = EV.link_prediction_ranks(emb, rows, CAND, known, side, candidate_sets=None if sets is None else sets[side])
        raw.append(r)
        fil.append(f)
    raw, fil = np.concatenate(raw), np.concatenate(fil)
    m = EV.mrr_and_hits(raw, fil)
    return np.array([m[k] for k in RT.KEYS[:7]] + [float(raw.size)]), raw, fil


@functools.lru_cache(maxsize=None)
def observed_sets():
    known = graph()[0]
    return {side: EV.CandidateSets.from_observed(CAND, known, R, side) for side in ("tail", "head")}


class RawTick:
    """ge_rank_validation_tick called straight through _lib on per-side rows (fixed, relation, true id, row set): what
    the bad-row cases need, which evaluate.RankPocket refuses on the host."""

    def __init__(self, emb, tail_rows, head_rows, sets=None, pocket=None):
        self.emb, self.sets, self.pocket = emb, sets, pocket
        tail_rows, head_rows = np.asarray(tail_rows, I64), np.asarray(head_rows, I64)
        assert tail_rows.shape == head_rows.shape
        self.V = V = len(tail_rows)
        d = emb.shape[1]
        rows = np.concatenate([tail_rows, head_rows])
        self.hr, self.true_id, self.row_set = dev(rows[:, :2].astype(I32)), dev(rows[:, 2].astype(I32)), dev(rows[:, 3].astype(I32))
        self.cand = dev(CAND)
        pos_of = torch.full((N,), -1, dtype=torch.int64, device="cuda")
        pos_of[self.cand.to(torch.int64)] = torch.arange(K, device="cuda")
        self.known = []
        for side, part in (("tail", tail_rows), ("head", head_rows)):
            index = EV.KnownIndex(graph()[0], N, side, "cuda")
            self.known += list(index.cells(dev(part[:, 0]), dev(part[:, 1]), pos_of, K))
        nbytes = int(_lib.load().ge_rank_planes_bytes(N, d, K))
        self.planes = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda") if nbytes else None
        self.ws = torch.full((int(_lib.load().ge_rank_tick_workspace_bytes(V)),), 0xFF, dtype=torch.uint8, device="cuda")
        self.out = torch.full((8,), -7.0, dtype=torch.float32, device="cuda")
        self.best = torch.zeros((), dtype=torch.float32, device="cuda")

    def __call__(self):
        ptr = lambda t: None if t is None else t.data_ptr()
        sets = (self.row_set.data_ptr(), self.sets["tail"].mask.data_ptr(), self.sets["head"].mask.data_ptr(),
                self.sets["tail"].n_sets) if self.sets else (None, None, None, 0)
        e = self.emb
        rc = _lib.load().ge_rank_validation_tick(e.data_ptr(), e.shape[0], e.shape[1], self.hr.data_ptr(), self.true_id.data_ptr(),
                                                 self.V, self.cand.data_ptr(), K, 1.0, 0, *[t.data_ptr() for t in self.known],
                                                 ptr(self.planes), *sets, None, self.out.data_ptr(), self.best.data_ptr(),
                                                 ptr(self.pocket), None, self.ws.data_ptr(), self.ws.numel(), stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        return self.out.cpu().numpy()


def side_rows(valid):
    """(tail-side rows, head-side rows) as (fixed, relation, true id, row set = relation)."""
    return valid[:, [0, 2, 1, 2]], valid[:, [1, 2, 0, 2]]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("V", VS)
def test_metrics_parity(V, masked):
    valid = graph()[1][:V]
    emb = dev(table(64, seed=V))
    sets = observed_sets() if masked else None
    ref, _, _ = reference(emb, valid, sets)
    vp = EV.RankPocket(emb, valid, CAND, graph()[0], candidate_sets=sets, keep_table=False)
    vp.tick(5)
    vp.tick(6)
    (s1, m1), (s2, m2) = vp.read()
    assert (s1, s2) == (5, 6) and vp.read() == []
    got = np.array([m1[k] for k in RT.KEYS], F32)
    RT.check_metrics(got, ref, "V=%d masked=%d" % (V, masked))
    assert m1["counted"] == 2 * V and isinstance(m1["counted"], int)
    assert m1 == m2                                                         # two ticks on one table agree bitwise
    assert float(vp.best) == m1["filtered_mrr"] > 0
    # three bad rows a side: a fixed id outside the table, a true id that is no candidate, a row set outside the range
    # (the last is a bad row only where sets are read: without masks it is a fourth good row).  The metrics are those
    # of the remaining rows.
    t_rows, h_rows = side_rows(valid)
    bad = np.array([[N + 5, 1, R + 3, 1], [R + 9, 2, 3, 2], [R + 4, 3, R + 11, R + 2]], I64)
    raw = RawTick(emb, np.concatenate([t_rows[:V // 2], bad, t_rows[V // 2:]]), np.concatenate([bad, h_rows]), sets)
    got_bad = raw()
    if masked:
        RT.check_metrics(got_bad, ref, "V=%d masked bad rows" % V)
        assert got_bad[7] == 2 * V
    else:
        # the fourth good row: (fixed R + 4, relation 3, true R + 11) is the triple's head on one side, its tail on the other
        ref4, _, _ = reference(emb, np.concatenate([valid, np.array([[R + 4, R + 11, 3]], I64)]), None,
                               np.concatenate([valid, np.array([[R + 11, R + 4, 3]], I64)]))
        RT.check_metrics(got_bad, ref4, "V=%d bad rows" % V)
        assert got_bad[7] == 2 * V + 2


def test_fp32_route():
    """d = 32: no split-precision sweep, planes NULL, the fp32 pipeline ranks; unmasked."""
    V = 129
    valid = graph()[1][:V]
    emb = dev(table(32, seed=3))
    assert int(_lib.load().ge_rank_planes_bytes(N, 32, K)) == 0
    vp = EV.RankPocket(emb, valid, CAND, graph()[0])
    assert vp.planes is None
    vp.tick(1)
    (_, m), = vp.read()
    RT.check_metrics(np.array([m[k] for k in RT.KEYS], F32), reference(emb, valid)[0], "d=32")
    assert bool(torch.equal(vp.pocket, emb))
    with pytest.raises(ValueError, match="masked sweep"):
        EV.RankPocket(emb, valid, CAND, graph()[0], candidate_sets=observed_sets())


def test_unfiltered():
    valid = graph()[1][:130]
    emb = dev(table(64, seed=4))
    vp = EV.RankPocket(emb, valid, CAND, None, keep_table=False)
    vp.tick(0)
    (_, m), = vp.read()
    assert m["filtered_mrr"] == m["raw_mrr"] and m["mean_filtered_pos"] == m["mean_raw_pos"]
    raw = np.concatenate([EV.link_prediction_ranks(emb, valid, CAND, None, side)[0] for side in ("tail", "head")])
    ref = EV.mrr_and_hits(raw, raw)
    RT.check_metrics(np.array([m[k] for k in RT.KEYS], F32), np.array([ref[k] for k in RT.KEYS[:7]] + [260.0]), "unfiltered")


@functools.lru_cache(maxsize=None)
def trained():
    """A table trained for 150 softmax steps on the known triples (the validation triples among them)."""
    emb = dev((np.random.default_rng(1).standard_normal((N, 64)) * 0.1).astype(F32))
    tr = H.SoftmaxTrainer(emb, dev(graph()[0].astype(I32)), dev(CAND), 256, scale=20.0, learning_rate=0.1, seed=2,
                          initial_accumulator_value=0.1)
    tr.run(150)
    torch.cuda.synchronize()
    return emb.cpu().numpy().copy()


def test_pocket():
    valid = graph()[1]
    rng = np.random.default_rng(11)
    tB = trained()
    tA = (tB + rng.standard_normal(tB.shape) * 0.04).astype(F32)
    tC = (tB + rng.standard_normal(tB.shape) * 0.3).astype(F32)
    accs = {k: (0.1 + rng.random(tB.shape)).astype(F32) for k in "ABCD"}
    emb, acc = dev(tA), dev(accs["A"])
    mrr = {}
    for k, t in (("A", tA), ("B", tB), ("C", tC)):
        emb.copy_(dev(t))
        mrr[k] = reference(emb, valid)[0][0]
    print("RANK TICK pocket: MRR A %.4f, B %.4f, C %.4f" % (mrr["A"], mrr["B"], mrr["C"]))
    assert mrr["B"] > mrr["A"] + 1e-4 and mrr["A"] > mrr["C"] + 1e-4     # the order the test is about, checked first
    vp = EV.RankPocket(emb, valid, CAND, graph()[0], accumulator=acc)
    vp.pocket.fill_(float("nan"))
    vp.pocket_accumulator.fill_(float("nan"))
    seen = []
    for step, (k, t) in enumerate((("A", tA), ("B", tB), ("C", tC), ("D", tB)), 1):
        emb.copy_(dev(t))
        acc.copy_(dev(accs[k]))
        vp.tick(step)
        torch.cuda.synchronize()
        seen.append((vp.pocket.cpu().numpy().copy(), vp.pocket_accumulator.cpu().numpy().copy(), float(vp.best)))
    hist = vp.read()
    assert [s for s, _ in hist] == [1, 2, 3, 4]
    m = [h["filtered_mrr"] for _, h in hist]
    for k, got in zip("ABC", m):
        assert abs(got - float(F32(mrr[k]))) <= RT.MRR_TOL
    bits = lambda a: a.view(I32)
    assert np.array_equal(bits(seen[0][0]), bits(tA)) and np.array_equal(bits(seen[0][1]), bits(accs["A"])) and seen[0][2] == m[0]
    for i in (1, 2, 3):      # after B, after C (untouched), after B again with another accumulator (a tie: untouched)
        assert np.array_equal(bits(seen[i][0]), bits(tB)) and np.array_equal(bits(seen[i][1]), bits(accs["B"])), i
        assert seen[i][2] == m[1]
    assert m[3] == m[1] and RT.pocket(m) == ([m[0], m[1], m[1], m[1]], [True, True, False, False])
    assert bool(torch.equal(emb, dev(tB))) and bool(torch.equal(acc, dev(accs["D"])))         # the inputs are only read


def test_all_bad_rows_leave_a_poisoned_pocket():
    emb = dev(table(64, seed=5))
    t_rows, h_rows = side_rows(graph()[1][:130])
    t_rows, h_rows = t_rows.copy(), h_rows.copy()
    t_rows[:, 0] = N + 1
    h_rows[:, 0] = N + 2
    pocket = torch.full((N, 64), float("nan"), dtype=torch.float32, device="cuda")
    raw = RawTick(emb, t_rows, h_rows, None, pocket)
    got = raw()
    assert np.isnan(got[:7]).all() and got[7] == 0
    assert float(raw.best) == 0.0 and bool(torch.isnan(pocket).all())


def test_host_checks():
    valid, known = graph()[1][:20], graph()[0]
    emb = dev(table(64))
    with pytest.raises(ValueError, match="empty"):
        EV.RankPocket(emb, valid[:0], CAND, known)
    bad = valid.copy()
    bad[3, 1] = 2                                                          # a relation row: in the table, no candidate
    with pytest.raises(ValueError, match="not in the candidate list"):
        EV.RankPocket(emb, bad, CAND, known)
    with pytest.raises(ValueError, match="not in the candidate list"):
        EV.RankPocket(emb, valid, CAND[CAND != valid[7, 0]], known)
    with pytest.raises(ValueError, match="accumulator"):
        EV.RankPocket(emb, valid, CAND, known, accumulator=torch.zeros(N, 32, device="cuda"))
    vp = EV.RankPocket(emb, valid, CAND, known, keep_table=False, capacity=2)
    assert vp.pocket is None and vp.pocket_accumulator is None and float(vp.best) == 0.0
    vp.tick(1)
    vp.tick(2)
    with pytest.raises(RuntimeError, match="read"):
        vp.tick(3)
    assert [s for s, _ in vp.read()] == [1, 2]
    vp.tick(3)
    (s, m), = vp.read()
    assert s == 3 and set(m) == set(RT.KEYS) == set(EV.mrr_and_hits([1], [1])) | {"counted"}
