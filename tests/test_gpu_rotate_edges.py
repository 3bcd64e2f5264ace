"""RotatE's hinge path (ge_rotate_score, ge_rotate_hinge_step, ge_rotate_adagrad_step, the native loop and
ge_rotate_rank through graphembeddings_amd.rotate.RotatE) at the edges test_gpu_rotate.py's shapes never reach, on the
fixtures of tests/rotate_edge_cases.py: every (VEC, LPT) instantiation of the score and gradient kernels on both sides
of each nvec boundary, one pointer alone off a 16-byte boundary, every grid-stride loop on its second trip, the apply
stage's windows with relation rows k < d wide, the sort's key width, the rank sweep's candidate loop going round with
an uneven share of blocks, the filter kernel wrapping and crossing empty tiles, and the sweep's scalar path, d = 2,
d = 1024 and drifted phases.

Exact cases (theta = 0, small integers, the squared norm, lr a power of two) compare bits with the fp64 restatement.
Float cases use rotate_ref.bound, test_gpu_rotate.py's rule (8 e32 + 1e-7, plus the one-ulp term), with e32 measured per
case from the float32 restatement; every block prints its worst deviation / bound (`-s` shows them).
tests/test_rotate_edge_cases_host.py proves the fixtures are what this file takes them for."""
import numpy as np
import pytest
import torch

from tests import rotate_edge_cases as EC
from tests import rotate_ref as RR
from tests.test_gpu_rotate import near, _bits, _cells

pytestmark = pytest.mark.gpu
F32 = np.float32
A0 = 0.1


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                  # a copy: the fixtures are read-only


def _load(m, tabs):
    for k, v in tabs.items():
        m.tables[k].copy_(torch.from_numpy(np.array(v, dtype=np.float32)))


def _off(t, shift):
    """A copy of t `shift` bytes (a multiple of 4) past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device="cuda")
    view = buf[shift // 4:shift // 4 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == shift % 16
    return view


def _model(tabs, l1, shifts=None, adagrad=False):
    """A model on the given tables; shifts: {"ent" | "rel" | "acc_ent" | "acc_rel": bytes past a 16-byte boundary}."""
    from graphembeddings_amd import rotate
    E, d = tabs["ent"].shape
    m = rotate.RotatE(E, len(tabs["rel"]), d, l1=l1, seed=0)
    _load(m, tabs)
    if adagrad:
        m.enable_adagrad(A0)
    for name, shift in (shifts or {}).items():
        if shift and name.startswith("acc_"):
            m.accumulators[name[4:]] = _off(m.accumulators[name[4:]], shift)
        elif shift:
            m.tables[name] = _off(m.tables[name], shift)
    return m


def _step(m, opt, case):
    f = m.adagrad_step if opt == "adagrad" else m.step
    return float(f(_dev(case["pos"]), _dev(case["neg"]), case["lr"], case["margin"]))


def _run(case, l1, opt, shifts=None):
    """(loss, tables, accumulators, tables before, accumulators before) of one step on a fresh model."""
    m = _model(case["tabs"], l1, shifts, opt == "adagrad")
    before, before_acc = _bits(m), (_bits(m, m.accumulators) if opt == "adagrad" else {})
    loss = _step(m, opt, case)
    return loss, _bits(m), (_bits(m, m.accumulators) if opt == "adagrad" else {}), before, before_acc


def _same(a, b):
    assert a[0] == b[0], "losses differ"
    for x, y in ((a[1], b[1]), (a[2], b[2])):
        for k in x:
            assert np.array_equal(x[k].view(np.int32), y[k].view(np.int32)), k


def _valid(case):
    tabs, pos, neg = case["tabs"], case["pos"], case["neg"]
    ok = RR.valid_mask(pos, neg, len(tabs["ent"]), len(tabs["rel"]))
    return pos[ok], neg[ok]


def _float_step(block, case, l1, opt, shifts=None, twice=True):
    """One step on a float case against rotate_ref within the bound; rows no active pair names bit-identical in every
    array; two runs from one state bit-equal.  Returns the run."""
    tabs = case["tabs"]
    out = _run(case, l1, opt, shifts)
    if twice:
        _same(out, _run(case, l1, opt, shifts))
    loss, after, after_acc, before, before_acc = out
    p, n = _valid(case)
    lr32, margin = float(F32(case["lr"])), case["margin"]
    accs = {k: np.full(v.shape, np.float64(F32(A0))) for k, v in tabs.items()}
    act = RR.active_mask(tabs, p, n, margin, l1)
    if opt == "adagrad":
        t64, a64, l64 = RR.adagrad_step(tabs, accs, p, n, lr32, margin, l1)
        t32, a32, l32 = RR.adagrad_step(tabs, accs, p, n, lr32, margin, l1, F32)
    else:
        (t64, l64), (t32, l32) = RR.sgd_step(tabs, p, n, lr32, margin, l1), RR.sgd_step(tabs, p, n, lr32, margin, l1, F32)
    near(block + " loss", loss, l64, l32, scale=RR.largest_dist(tabs, p, n, l1))
    named = RR.named_rows(tabs, p, n, act)
    for k in tabs:
        near(block + " tables", after[k], t64[k], t32[k])
        assert np.array_equal(after[k][~named[k]].view(np.int32), before[k][~named[k]].view(np.int32)), k
        assert (after[k][named[k]] != before[k][named[k]]).any(), k
        if opt == "adagrad":
            near(block + " accumulators", after_acc[k], a64[k], a32[k])
            assert np.array_equal(after_acc[k][~named[k]].view(np.int32), before_acc[k][~named[k]].view(np.int32)), k
    return out


def _exact_step(case, shifts=None):
    """One SGD step of the squared norm on an exact case: the loss and both tables equal the fp64 restatement bitwise."""
    loss, after, _, before, _ = _run(case, False, "sgd", shifts)
    p, n = _valid(case)
    new, rloss = RR.sgd_step(case["tabs"], p, n, case["lr"], case["margin"], False)
    assert loss == rloss
    for k in new:
        bad = np.argwhere(after[k].astype(np.float64) != new[k])
        assert len(bad) == 0, (k, "first (row, col) off:", bad[:4].tolist(), len(bad))
    assert (after["ent"] != before["ent"]).any() and (after["rel"] != before["rel"]).any()
    return after


def _score(tabs, l1, tri, shifts=None):
    return _model(tabs, l1, shifts).score(_dev(tri)).cpu().numpy()


# =============================================================================================== A: every variant
@pytest.mark.parametrize("d,shift", EC.names("variant"))
@pytest.mark.parametrize("l1", [True, False])
def test_variant_score(l1, d, shift):
    """203 triples at every (VEC, LPT)."""
    case = EC.variant_case(d, bool(shift))
    got = _score(case["tabs"], l1, case["tri"], {"ent": shift, "rel": shift})
    near("variant score", got, RR.dist(case["tabs"], case["tri"], l1), RR.dist(case["tabs"], case["tri"], l1, F32))


@pytest.mark.parametrize("d,shift", EC.names("variant"))
@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("l1", [True, False])
def test_variant_step(l1, opt, d, shift):
    """One step of 157 pairs at every (VEC, LPT).  The loss is one number: the host test test_float_cases_are_fair keeps
    seeds on which the fp32 restatement's errors cancel in it by chance out of the fixtures."""
    case = EC.variant_case(d, bool(shift))
    _float_step("variant step", case, l1, opt, {"ent": shift, "rel": shift})


# =============================================================================================== B: one pointer off
@pytest.mark.parametrize("which", EC.names("one_pointer_off"))
def test_one_pointer_off(which):
    """d = 72 (float4, 16 lanes, when aligned): one pointer alone 4 bytes off sends the whole step down the scalar
    kernels, the same kernels on the same values as the run with every pointer off."""
    case = EC.variant_case(EC.ONE_OFF_D, True)
    opt = "adagrad" if which.startswith("acc_") else "sgd"
    every = {"ent": 4, "rel": 4, "acc_ent": 4, "acc_rel": 4} if opt == "adagrad" else {"ent": 4, "rel": 4}
    for l1 in (True, False):
        one = _float_step("one pointer off", case, l1, opt, {which: 4}, twice=False)
        _same(one, _run(case, l1, opt, every))
        if opt == "sgd":
            a, b = _score(case["tabs"], l1, case["tri"], {which: 4}), _score(case["tabs"], l1, case["tri"], every)
            assert np.array_equal(a.view(np.int32), b.view(np.int32))
            near("one pointer off score", a, RR.dist(case["tabs"], case["tri"], l1), RR.dist(case["tabs"], case["tri"], l1, F32))


# =============================================================================================== C: wraps
@pytest.mark.parametrize("lpt", EC.names("wrap"))
def test_wrap_score(lpt):
    case, W = EC.wrap_score_case(lpt), EC.score_wrap_B(lpt)
    for l1 in (True, False):
        m = _model(case["tabs"], l1)
        got = m.score(_dev(case["tri"])).cpu().numpy()
        near("wrap score", got, RR.dist(case["tabs"], case["tri"], l1), RR.dist(case["tabs"], case["tri"], l1, F32))
        tail = m.score(_dev(case["tri"][W:])).cpu().numpy()         # the second trip's rows on a first trip
        assert np.array_equal(tail.view(np.int32), got[W:].view(np.int32))
        first = m.score(_dev(case["tri"][:W])).cpu().numpy()
        assert np.array_equal(first.view(np.int32), got[:W].view(np.int32))


@pytest.mark.parametrize("lpt", EC.names("wrap"))
def test_wrap_exact_step_bitwise(lpt):
    """Rows W ... W + 4 run on the second trip of the lane groups that handled an active pair, an inactive one (the
    `continue`), a bad id, a foreign relation and an active pair (test_wrap_second_trip_rows on the host)."""
    _exact_step(EC.wrap_exact_case(lpt))


@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("lpt", EC.names("wrap"))
def test_wrap_float_step(lpt, l1):
    _float_step("wrap step", EC.wrap_float_case(lpt), l1, "sgd", twice=False)


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
def test_wrap_loop_equals_draws_plus_single_steps_bitwise(opt):
    case = EC.wrap_loop_case()
    B, n, lr = case["B"], EC.LOOP_STEPS, 0.05
    a, b = _model(case["tabs"], True), _model(case["tabs"], True)
    tr = a.trainer(case["triples"], B, margin=1.0, learning_rate=lr, seed=21, optimizer=opt)
    if opt == "adagrad":
        b.enable_adagrad(0.1)
    la = tr.run(n).cpu().numpy()
    for s in range(n):
        pos, neg = tr.draw(s)
        lb = float((b.adagrad_step if opt == "adagrad" else b.step)(pos, neg, lr, 1.0))
        assert lb == la[s], s
    assert la[0] > 0
    for k in a.tables:
        assert torch.equal(a.tables[k], b.tables[k]), k
        if opt == "adagrad":
            assert torch.equal(a.accumulators[k], b.accumulators[k]), k


# =============================================================================================== D: apply layouts
@pytest.mark.parametrize("d,v4", EC.LAYOUT_DIMS)
def test_layout_sgd_bitwise(d, v4):
    for name in EC.LAYOUTS:
        _exact_step(EC.layout_case(name, d))


@pytest.mark.parametrize("d,v4", EC.LAYOUT_DIMS)
def test_layout_modulus_norm(d, v4):
    """The same layouts with the modulus norm on collinear tables: its gradients (3/5, 4/5) are not exact."""
    for name in EC.LAYOUTS:
        _float_step("layout l1 sgd", EC.layout_case(name, d, True), True, "sgd", twice=False)


@pytest.mark.parametrize("d,v4", EC.LAYOUT_DIMS)
def test_layout_adagrad(d, v4):
    """AdaGrad on the exact batches, by bound; the relation accumulator rows are k wide and no row outside the named
    ones changes (_float_step)."""
    for name in EC.LAYOUTS:
        case = EC.layout_case(name, d)
        out = _float_step("layout adagrad", case, False, "adagrad", twice=False)
        assert out[2]["rel"].shape == (len(case["tabs"]["rel"]), d // 2) and out[2]["ent"].shape == case["tabs"]["ent"].shape


# =============================================================================================== E: key width
@pytest.mark.parametrize("total", EC.names("key_width"))
def test_key_width_bitwise(total):
    case = EC.key_width_case(total)
    after = _exact_step(case)
    E, R = len(case["tabs"]["ent"]), len(case["tabs"]["rel"])
    assert (after["ent"][E - 1] != case["tabs"]["ent"][E - 1]).any() and (after["rel"][R - 1] != 0).any()


# =============================================================================================== F - H: ranks
def _rank_call(m, test, known, side):
    off, rc = _cells(m, test, known, side)
    return [x.cpu().numpy() for x in m.rank_counts(_dev(test), cand_is_head=side == "head", known_off=off, known_rc=rc,
                                                   return_scores=True)]


def _rank_float(block, m, tabs, test, known, side, l1, km, twice=True):
    """(a) the counts and the filtered counts equal, for every row, the counts recomputed from the call's own scores_out
    and true_dist; (b) scores_out and true_dist within the bound of fp64; two calls bit-equal."""
    nb, nk, td, sc = _rank_call(m, test, known, side)
    target = test[:, 0] if side == "head" else test[:, 1]
    snb, snk = RR.counts_from(sc, td, target, km)
    assert np.array_equal(nb, snb), np.flatnonzero(nb != snb)[:8]
    assert np.array_equal(nk, snk), np.flatnonzero(nk != snk)[:8]
    assert np.array_equal(td.view(np.int32), sc[np.arange(len(test)), target].view(np.int32))
    _, _, td64, sc64 = EC.rank_reference(tabs, test, side, l1, None)
    _, _, td32, sc32 = EC.rank_reference(tabs, test, side, l1, None, F32)
    near(block + " scores_out", sc, sc64, sc32)
    near(block + " true_dist", td, td64, td32)
    if twice:
        for x, y in zip((nb, nk, td, sc), _rank_call(m, test, known, side)):
            assert np.array_equal(x.view(np.int32), y.view(np.int32))
    return nb, nk, td, td64, td32


@pytest.mark.parametrize("side,l1", EC.names("rank_trip"))
def test_rank_trip_exact(side, l1):
    """gridDim.y = 2 over three candidate blocks: every count, filtered count, distance and rank equals fp64's outright,
    on tables where every target ties with a twin in another block."""
    test, known = EC.rank_trip_rows()
    tabs, km = EC.rank_trip_tables(l1), EC.rank_trip_mask(side)
    enb, enk, etd, esc = EC.rank_reference(tabs, test, side, l1, km)
    nb, nk, td, sc = _rank_call(_model(tabs, l1), test, known, side)
    assert np.array_equal(td.astype(np.float64), etd)
    assert np.array_equal(nb, enb), np.flatnonzero(nb != enb)[:8]
    assert np.array_equal(nk, enk), np.flatnonzero(nk != enk)[:8]
    assert np.array_equal(sc, esc.astype(F32))


def test_rank_trip_float():
    test, known = EC.rank_trip_rows()
    tabs = EC.rank_trip_tables(True, exact=False)
    _rank_float("rank trip", _model(tabs, True), tabs, test, known, "head", True, EC.rank_trip_mask("head"))


@pytest.mark.parametrize("side", EC.names("rank_sparse"))
def test_rank_sparse_known_tiles(side):
    case = EC.rank_sparse_case(side)
    km = RR.known_mask(case["test"], case["known"], EC.SPARSE_E, side)
    for l1 in (True, False):
        nb, nk, *_ = _rank_float("rank sparse", _model(case["tabs"], l1), case["tabs"], case["test"], case["known"], side, l1, km)
        assert nk.sum() > 0 and (nk <= km.sum(1)).all()


@pytest.mark.parametrize("name", EC.names("rank_edge"))
@pytest.mark.parametrize("side", ["tail", "head"])
@pytest.mark.parametrize("l1", [True, False])
def test_rank_edges(l1, side, name):
    """(a), (b) of _rank_float; (c) true_dist within the bound of ge_rotate_score on the same rows (two roundings of one
    number: the larger e32 of the two forms).  d1024 is the case that made the sweep sum a distance in blocks of 32
    coordinates: one serial fp32 sum of its 512 coordinates lay up to 1.31 of the bound from fp64."""
    case = EC.rank_edge_case(name)
    tabs, test, known = case["tabs"], case["test"], case["known"][side]
    m = _model(tabs, l1, {"ent": case["shift"]})
    km = RR.known_mask(test, known, len(tabs["ent"]), side)
    nb, nk, td, td64, td32 = _rank_float("rank edge " + name, m, tabs, test, known, side, l1, km)
    score = m.score(_dev(test.astype(np.int32))).cpu().numpy()
    form = RR.dist(tabs, test, l1, F32)
    worse = form if np.abs(form - td64).max() > np.abs(td32 - td64).max() else td32
    assert np.all(np.abs(td.astype(np.float64) - score) <= RR.bound(td64, worse)[0]), (l1, side)
    assert (nk > 0).any() and (nb > nk).any()
