"""The self-adversarial negative-sampling loss of TransE / TransH / TransD on the MI355X through
graphembeddings_amd.transx (ge_transx_adv_*) against the NumPy restatement tests/transx_adv_ref.py.

Tolerances: test_gpu_rotate.py's rule, rotate_ref.bound -- 8 e32 + 1e-7 with its one-ulp clause, e32 the largest
deviation of this restatement run in float32 from its fp64 value.  The kernel evaluates every residual from the row's
fixed side, (proj(h) + r) - proj(t') or -((proj(t) - r) - proj(h')), and adds every sum in an order of its own, so e32 is
the largest over the restatement's float32 forms (transx_adv_ref.FORMS32: the reference order, the fixed-side order, and
the latter with every sum back to front and strictly left to right): each is one sample of these statements' rounding
error, and at B = 1 a single sample is often several times below the next (with "ref" and "fixed" alone one of this
file's cases -- TransE, d 100, L1, AdaGrad accumulators -- measured 1.14 of the bound).  `scale` is the largest distance a
loss is formed from; gamma is the median distance of the batch.  Every block prints its worst deviation / bound (`-s`
shows them).  Every L1 case is built by transx_adv_ref.build_case, which
takes the first of 32 seeds at which no residual sits near a sign change (test_transx_adv_ref_host.py checks them all).

Shapes.  One workgroup works on a row; its lanes form NT teams that take the row's negatives j = team, team + NT, ...
NT depends on the number of chunks a row is read in (d scalars, or d / 4 float4 when d % 4 == 0 on 16-byte aligned
tables): NT = 32 up to 8 chunks (8 lanes a team), 16 up to 16, 8 up to 32, 4 above (a whole wave a team, one or more chunks
a lane, the last of them ragged at d 1023 and at d 200 read as scalars); a wave holds NT / 4 teams.  The softmax gives
thread x the negatives x, x + 256, ...  So K runs over 1, 2; NT / 4 and NT (the first negative of a second wave, of a
second round), each -1, +0 and +1; 64, 128, 192 (the softmax's waves), 256, 512, 768 (a thread's second, third and fourth
negative), each -1, +0 and +1; and the maximum 1024.  From d 200 on the softmax's edges are 63, 64, 65 alone, so that no
case takes more than a few seconds (transx_adv_ref.ks).
The kernel runs at most 2,048 workgroups, one row each at a time: rows from 2,048 on are a workgroup's second trip
through its loop (test_rows_beyond_the_grid).
"""
import numpy as np
import pytest
import torch

import test_gpu_rotate as TR
from oracle import transx_oracle as TO
from tests import transx_adv_ref as AR
from tests import transx_ref as XR

pytestmark = pytest.mark.gpu
F32 = np.float32
A0 = 0.1
MODELS = AR.MODELS
near, _dev, _host, _bits, _load = TR.near, TR._dev, TR._host, TR._bits, TR._load


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")


def _make(model, tabs, l1, shift=0):
    """A TransX on the given tables; shift: bytes past a 16-byte boundary at which every table starts."""
    from graphembeddings_amd import transx as X
    E, d = tabs["ent"].shape
    m = X.TransX(model, E, len(tabs["rel"]), d, l1=l1, seed=0)
    _load(m, tabs)
    if shift:
        for k, t in list(m.tables.items()):
            buf = torch.empty(t.numel() + 4, dtype=torch.float32, device="cuda")
            view = buf[shift // 4:shift // 4 + t.numel()].view(t.shape)
            view.copy_(t)
            assert view.data_ptr() % 16 == shift
            m.tables[k] = view
    return m


def _all32(f, *a, **kw):
    """The restatement in float32 in each of its forms."""
    return [f(*a, dtype=F32, form=form, **kw) for form in AR.FORMS32]


def _pick(runs, *idx):
    """Component idx of every run (a run is a tuple; its tables are dicts)."""
    out = runs
    for i in idx:
        out = [r[i] for r in out]
    return out


def _check_loss_rows(block, m, tabs, pos, side, neg_ent, margin, alpha):
    model, l1 = m.model, m.l1
    got = m.adv_loss(_dev(pos), _dev(side), _dev(neg_ent), margin, alpha).cpu().numpy()
    ref = AR.row_losses(model, tabs, pos, side, neg_ent, margin, alpha, l1)
    r32 = _all32(AR.row_losses, model, tabs, pos, side, neg_ent, margin, alpha, l1)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), block           # NaN exactly on the invalid rows
    ok = ~np.isnan(ref)
    near(block + " loss rows", got[ok], ref[ok], AR.worst32(ref[ok], *[x[ok] for x in r32]),
         scale=AR.largest_dist(model, tabs, pos, side, neg_ent, l1))
    again = m.adv_loss(_dev(pos), _dev(side), _dev(neg_ent), margin, alpha).cpu().numpy()
    assert np.array_equal(got.view(np.int32), again.view(np.int32)), block
    return got


def _run_step(m, opt, pos, side, neg_ent, margin, alpha, lr):
    f = m.adv_adagrad_step if opt == "adagrad" else m.adv_step
    return float(f(_dev(pos), _dev(side), _dev(neg_ent), margin, alpha, lr))


def _check_step(block, make, opt, pos, side, neg_ent, margin, alpha, lr):
    """One step on make()'s tables against the restatement; rows no valid row names bit-identical in every array; two
    runs from one state bit-equal."""
    outs = []
    for _ in range(2):
        m = make()
        if opt == "adagrad":
            m.enable_adagrad(A0)
        before, before_acc = _bits(m), (_bits(m, m.accumulators) if opt == "adagrad" else {})
        tabs = _host(m)
        loss = _run_step(m, opt, pos, side, neg_ent, margin, alpha, lr)
        outs.append((loss, _bits(m), _bits(m, m.accumulators) if opt == "adagrad" else {}))
    assert outs[0][0] == outs[1][0], (block, "two runs differ in the loss")
    for arrs in (1, 2):
        for k in outs[0][arrs]:
            assert np.array_equal(outs[0][arrs][k].view(np.int32), outs[1][arrs][k].view(np.int32)), (block, k, "two runs differ")
    loss, after, after_acc = outs[0]
    model, l1, lr32 = m.model, m.l1, float(F32(lr))
    accs = {k: np.full(v.shape, np.float64(F32(A0))) for k, v in tabs.items()}
    if opt == "adagrad":
        t64, a64, l64 = AR.adagrad_step(model, tabs, accs, pos, side, neg_ent, lr32, margin, alpha, l1)
        r32 = _all32(AR.adagrad_step, model, tabs, accs, pos, side, neg_ent, lr32, margin, alpha, l1)
    else:
        t64, l64 = AR.sgd_step(model, tabs, pos, side, neg_ent, lr32, margin, alpha, l1)
        r32 = _all32(AR.sgd_step, model, tabs, pos, side, neg_ent, lr32, margin, alpha, l1)
    near(block + " loss", loss, l64, AR.worst32(l64, *_pick(r32, -1)), scale=AR.largest_dist(model, tabs, pos, side, neg_ent, l1))
    named = AR.named_rows(model, tabs, pos, side, neg_ent)
    assert set(named) == set(tabs) == set(after)
    for k in tabs:
        near(block + " tables", after[k], t64[k], AR.worst32(t64[k], *_pick(r32, 0, k)))
        assert np.array_equal(after[k][~named[k]].view(np.int32), before[k][~named[k]].view(np.int32)), (block, k)
        # (TransH at d 1 projects every entity to 0 and n^ = +-1 whatever n is: every distance of a row is |r|, and only
        # rel has a gradient, which the negatives' cancel where they all weigh alike)
        if named[k].any() and (model != "transh" or tabs[k].shape[1] > 1):
            assert (after[k][named[k]] != before[k][named[k]]).any(), (block, k)
        if opt == "adagrad":
            near(block + " accumulators", after_acc[k], a64[k], AR.worst32(a64[k], *_pick(r32, 1, k)))
            assert np.array_equal(after_acc[k][~named[k]].view(np.int32), before_acc[k][~named[k]].view(np.int32)), (block, k)
    return tabs


def _case_args(c):
    return c["pos"], c["side"], c["neg_ent"], c["margin"]


# =============================================================================================== loss rows, one step
@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("d,shift", AR.SHAPES)
@pytest.mark.parametrize("model", MODELS)
def test_loss_rows_and_one_step_match_the_restatement(model, opt, l1, d, shift):
    """E = 61, R = 7; the rows name entities below E - 4 and relations below R - 1, so that the last rows of every table
    must keep their bits.  B cycles through 65, 3, 1 (3 and 1 above K = 33), alpha through 0, 1, 5."""
    seen_B, seen_alpha = set(), set()
    for K, B, alpha, seed0 in AR.step_cases(model, l1, opt, d, shift):
        seen_B.add(B); seen_alpha.add(alpha)
        c = AR.step_case(model, l1, d, K, B, seed0)
        pos, side, neg_ent, margin = _case_args(c)
        make = lambda: _make(model, c["tabs"], l1, shift)
        block = "%s adv K=%d" % (model, K) if K in (1, 1024) else "%s adv" % model
        _check_step(block, make, opt, pos, side, neg_ent, margin, alpha, 0.01)
        if opt == "sgd":
            _check_loss_rows(block, make(), c["tabs"], pos, side, neg_ent, margin, alpha)
    assert seen_B == {1, 3, 65} and seen_alpha == {0.0, 1.0, 5.0}


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("d", [8, 6])
@pytest.mark.parametrize("model", MODELS)
def test_rows_beyond_the_grid(model, opt, l1, d):
    """B = 2,053 (transx_adv_ref._grid_batch): second trips after a valid row and after an invalid row, on the float4 path
    (d 8) and the scalar one (d 6)."""
    E, R, G = AR.E_, AR.R_, AR.GRID
    c = AR.grid_case(model, l1, d)
    pos, side, neg_ent, margin = _case_args(c)
    make = lambda: _make(model, c["tabs"], l1)
    _check_step("%s adv B>2048" % model, make, opt, pos, side, neg_ent, margin, 1.0, 0.002)
    named = AR.named_rows(model, c["tabs"], pos, side, neg_ent)
    assert not named["ent"][E - 1] and not named["rel"][R - 1]
    if opt == "sgd":
        got = _check_loss_rows("%s adv B>2048" % model, make(), c["tabs"], pos, side, neg_ent, margin, 1.0)
        assert sorted(np.nonzero(np.isnan(got))[0]) == [1, 3, G + 2, G + 3]
        # rows 2,048.. on their own are the same rows: a first trip and a second trip give the same bits
        tail = make().adv_loss(_dev(pos[G:]), _dev(side[G:]), _dev(neg_ent[G:]), margin, 1.0).cpu().numpy()
        assert np.array_equal(got[G:].view(np.int32), tail.view(np.int32))


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("model", MODELS)
def test_hot_rows(model, opt, l1):
    """B = 64, K = 64 over 5 entities and 2 relations: 4,288 slots on 7 keys, every segment cut by many 32-slot windows
    of the apply stage, in both planes."""
    c = AR.hot_case(model, l1)
    pos, side, neg_ent, margin = _case_args(c)
    for alpha in (0.0, 1.0):
        _check_step("%s adv hot rows" % model, lambda: _make(model, c["tabs"], l1), opt, pos, side, neg_ent, margin, alpha, 0.01)


@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("model", MODELS)
def test_empty_slots_and_invalid_rows(model, l1):
    """Empty slots (-1 and E), a row with every slot empty, sides 2 and -1, positive ids out of range: each writes what
    the contract says.  The invalid rows alone name entity E - 1 and relation R - 1, which keep their bits."""
    c = AR.empty_case(model, l1)
    pos, side, neg_ent, _ = _case_args(c)
    tabs = c["tabs"]
    E, R = len(tabs["ent"]), len(tabs["rel"])
    make = lambda: _make(model, tabs, l1)
    got = _check_loss_rows("%s adv empty/invalid" % model, make(), tabs, pos, side, neg_ent, 3.0, 1.0)
    assert np.array_equal(np.isnan(got), AR.EMPTY_INVALID)
    P = AR.parts(model, tabs, pos, side, neg_ent, 3.0, 1.0, l1)
    P32 = AR.parts(model, tabs, pos, side, neg_ent, 3.0, 1.0, l1, F32, "fixed")
    one = AR.softplus(P["Dp"][1] - 3.0)                              # the all-empty row: its positive term alone
    near("%s adv empty/invalid loss rows" % model, got[1:2], [one], [AR.softplus(P32["Dp"][1] - F32(3.0))], scale=P["Dp"][1])
    for opt in ("sgd", "adagrad"):
        _check_step("%s adv empty/invalid" % model, make, opt, pos, side, neg_ent, 3.0, 1.0, 0.05)
    named = AR.named_rows(model, tabs, pos, side, neg_ent)
    assert not named["ent"][E - 1] and not named["rel"][R - 1]
    # a batch of invalid rows alone: loss 0, nothing moves, in the tables and in the accumulators
    for opt in ("sgd", "adagrad"):
        m = make()
        if opt == "adagrad":
            m.enable_adagrad(A0)
        before = dict(_bits(m), **({"acc_" + k: v for k, v in _bits(m, m.accumulators).items()} if opt == "adagrad" else {}))
        assert _run_step(m, opt, pos[2:8], side[2:8], neg_ent[2:8], 3.0, 1.0, 0.05) == 0.0
        after = dict(_bits(m), **({"acc_" + k: v for k, v in _bits(m, m.accumulators).items()} if opt == "adagrad" else {}))
        assert all(np.array_equal(before[k].view(np.int32), after[k].view(np.int32)) for k in before)


@pytest.mark.parametrize("model", MODELS)
def test_int64_ids_beyond_int32_stay_out_of_range(model):
    """An int64 id that int32 does not hold is an empty slot / an invalid row, not the valid id it would wrap into."""
    m = _make(model, AR.tables(model, 30, 3, 8, seed=4), True)
    pos = np.array([[3, 4, 1], [5, 6, 2], [7, 8, 0], [9, 10, 1]], dtype=np.int64)
    side = np.array([0, 1, 0, 1], dtype=np.int64)
    neg = np.array([[11, 12], [13, 14], [15, 16], [17, 18]], dtype=np.int64)
    wide, small = (pos.copy(), side.copy(), neg.copy()), (pos.copy(), side.copy(), neg.copy())
    wide[2][0, 1], small[2][0, 1] = (1 << 32) + 12, -1                    # would wrap to 12
    wide[0][1, 0], small[0][1, 0] = (1 << 32) + 5, -1                     # ... to 5
    wide[1][2], small[1][2] = 1 << 32, 2                                  # ... to 0
    wide[2][3, 0], small[2][3, 0] = -(1 << 32) + 17, -1                   # ... to 17
    a = m.adv_loss(*(_dev(x) for x in wide), 3.0, 1.0).cpu().numpy()
    b = m.adv_loss(*(_dev(x.astype(np.int32)) for x in small), 3.0, 1.0).cpu().numpy()
    assert np.array_equal(np.isnan(a), [False, True, True, False]) and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("l1", [True, False])
def test_transh_normal_row_below_the_clamp(l1):
    """Relation 1's normal row has n.n < 1e-12: n^ = 1e6 n and l2_normalize's second term is off (the max takes the
    epsilon).  Loss rows and both steps against the restatement, which differentiates that branch."""
    c = AR.clamp_case(l1)
    pos, side, neg_ent, margin = _case_args(c)
    make = lambda: _make("transh", c["tabs"], l1)
    _check_loss_rows("transh adv clamp", make(), c["tabs"], pos, side, neg_ent, margin, 1.0)
    for opt in ("sgd", "adagrad"):
        _check_step("transh adv clamp", make, opt, pos, side, neg_ent, margin, 1.0, 0.01)


@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("model", MODELS)
def test_equal_negatives_weigh_as_one(model, l1):
    """A row whose 64 negatives are one entity has the K = 1 row's loss: the softmax weights sum to 1."""
    tabs = AR.tables(model, 30, 3, 16, seed=9)
    m = _make(model, tabs, l1)
    pos = np.array([[3, 4, 1], [5, 6, 2]], dtype=np.int32)
    side = np.array([0, 1], dtype=np.int32)
    one = np.array([[11], [12]], dtype=np.int32)
    for alpha in (0.0, 1.0, 5.0):
        got = m.adv_loss(_dev(pos), _dev(side), _dev(np.repeat(one, 64, 1)), 3.0, alpha).cpu().numpy()
        ref = AR.row_losses(model, tabs, pos, side, one, 3.0, alpha, l1)
        r32 = _all32(AR.row_losses, model, tabs, pos, side, one, 3.0, alpha, l1)
        near("%s adv equal negatives" % model, got, ref, AR.worst32(ref, *r32),
             scale=AR.largest_dist(model, tabs, pos, side, one, l1))


# =============================================================================================== draw and loop
def _adv_trainer(m, tri, B, K, seed, opt="sgd", alpha=1.0, margin=3.0, lr=0.05):
    return m.trainer(tri, B, loss="self_adversarial", negatives=K, adversarial_temperature=alpha, margin=margin,
                     learning_rate=lr, seed=seed, optimizer=opt, initial_accumulator_value=A0)


def _kg(seed=4, E=50, R=4, T=600):
    rng = np.random.default_rng(seed)
    return np.unique(np.stack([rng.integers(0, E, T), rng.integers(0, E, T), rng.integers(0, R, T)], 1), axis=0), E, R


def test_draw_is_the_shared_one():
    """The trainer's draw is ge_rotate_adv_draw_batch: the restatement's batch, the hinge loop's positives and sides."""
    tri, E, R = _kg()
    m = _make("transe", AR.tables("transe", E, R, 8, seed=2), True)
    B, K, seed = 65, 5, 21
    tr, hinge = _adv_trainer(m, tri, B, K, seed), m.trainer(tri, B, seed=seed)
    assert type(tr).__name__ == "AdvTrainer" and type(hinge).__name__ == "Trainer"
    idx = TO.BernoulliIndex(tri, 0, E, R)
    for step in (0, 3):
        pos, side, neg_ent = (x.cpu().numpy() for x in tr.draw(step))
        hpos, hneg = (x.cpu().numpy() for x in hinge.draw(step))
        assert np.array_equal(pos, hpos) and np.array_equal(side, (hneg[:, 0] != hpos[:, 0]).astype(np.int32))
        rpos, rside, rneg = AR.draw(tri, idx, seed, step, B, K)
        assert np.array_equal(pos, rpos) and np.array_equal(side, rside) and np.array_equal(neg_ent, rneg)


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("model", MODELS)
def test_loop_equals_draws_plus_single_steps_bitwise(model, opt):
    tri, E, R = _kg()
    d, B, K, n, seed, lr = 8, 33, 5, 4, 21, 0.05
    tabs = AR.tables(model, E, R, d, seed=2)
    a, b = _make(model, tabs, True), _make(model, tabs, True)
    tr = _adv_trainer(a, tri, B, K, seed, opt, alpha=1.0, margin=2.0, lr=lr)
    if opt == "adagrad":
        b.enable_adagrad(A0)
    la = tr.run(n).cpu().numpy()
    assert tr.step_count == n
    for s in range(n):
        pos, side, neg_ent = tr.draw(s)
        lb = float((b.adv_adagrad_step if opt == "adagrad" else b.adv_step)(pos, side, neg_ent, 2.0, 1.0, lr))
        assert lb == la[s], s
    assert la[0] > 0
    for k in a.tables:
        assert torch.equal(a.tables[k], b.tables[k]), k
        if opt == "adagrad":
            assert torch.equal(a.accumulators[k], b.accumulators[k]), k
    # state_dict carries no hyperparameter of this loss
    plain = set(_make(model, tabs, True).state_dict())
    assert set(a.state_dict()) == plain | ({"adagrad_init"} | {"adagrad_" + k for k in a.tables} if opt == "adagrad" else set())
    assert tr.run(0).numel() == 0 and tr.step_count == n


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("model", MODELS)
def test_hinge_trainer_and_step_give_the_entry_points_bits(model, opt):
    """loss="hinge" (and no loss argument) is the trainer it was, and step / adagrad_step the steps they were: the same
    calls made directly on the hinge entry points give the same bits, before and after self-adversarial steps ran in the
    process on a model of the same shape."""
    from graphembeddings_amd import _lib
    from graphembeddings_amd.hole import _stream
    tri, E, R = _kg()
    d, B, seed, lr, margin = 8, 33, 5, 0.05, 1.0
    tabs = AR.tables(model, E, R, d, seed=3)
    ada = opt == "adagrad"

    def fresh():
        m = _make(model, tabs, True)
        if ada:
            m.enable_adagrad(A0)
        return m

    def via_class(kw):
        m = fresh()
        tr = m.trainer(tri, B, margin=margin, learning_rate=lr, seed=seed, optimizer=opt, initial_accumulator_value=A0, **kw)
        assert type(tr).__name__ == "Trainer"
        losses = tr.run(3)
        pos, neg = tr.draw(7)
        one = (m.adagrad_step if ada else m.step)(pos, neg, lr, margin)
        return m, torch.cat([losses, one.view(1)])

    def via_entry_points():
        m = fresh()
        tr = m.trainer(tri, B, margin=margin, learning_rate=lr, seed=seed)        # (its sampler arrays and draw only)
        ws, losses, loss = m.workspace(B), torch.empty(3, dtype=torch.float32, device="cuda"), torch.empty(1, dtype=torch.float32, device="cuda")
        ptrs = m._adagrad_ptrs() if ada else m._ptrs()
        _lib.call("ge_transx_train_steps_adagrad" if ada else "ge_transx_train_steps", *ptrs, *tr._sampler_args(), seed, 0, 3, B,
                  margin, lr, losses.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        pos, neg = tr.draw(7)
        _lib.call("ge_transx_adagrad_step" if ada else "ge_transx_hinge_step", *ptrs, pos.data_ptr(), neg.data_ptr(), B, margin,
                  lr, loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        return m, torch.cat([losses, loss])

    def same(x, y):
        assert torch.equal(x[1], y[1])
        for k in x[0].tables:
            assert torch.equal(x[0].tables[k], y[0].tables[k]), k
            if ada:
                assert torch.equal(x[0].accumulators[k], y[0].accumulators[k]), k

    ref = via_entry_points()
    same(via_class({}), ref)
    same(via_class(dict(loss="hinge")), ref)
    other = fresh()
    _adv_trainer(other, tri, B, 5, seed, opt).run(2)
    pos, side, neg_ent = AR.batch(np.random.default_rng(0), E, R, 4, 3)
    _run_step(other, opt, pos, side, neg_ent, 2.0, 1.0, lr)
    same(via_class(dict(loss="hinge")), ref)
    same(via_entry_points(), ref)
    # a hinge trainer of a model that has trained adversarially still runs the hinge loop on its own workspace
    assert np.isfinite(other.trainer(tri, B, seed=seed, optimizer=opt).run(2).cpu().numpy()).all()


def test_transr_has_no_self_adversarial_trainer():
    from graphembeddings_amd import transr
    tri, E, R = _kg()
    m = transr.TransR(E, R, 8, 8)
    with pytest.raises(ValueError, match="self-adversarial"):
        m.trainer(tri, 4, loss="self_adversarial")
    assert type(m.trainer(tri, 4, loss="hinge")).__name__ == type(m.trainer(tri, 4)).__name__
    assert not hasattr(m, "adv_loss")


def _write(path, rows, count=None):
    with open(path, "w") as f:
        f.write(f"{len(rows) if count is None else count}\n")
        for r in rows:
            f.write(" ".join(str(int(x)) for x in r) + "\n")


def test_driver_trains_saves_reloads_and_evaluates(tmp_path, capsys):
    import json
    from graphembeddings_amd import transx_train as D
    tri = XR.planted_kg(n_ent=120, n_rel=4, n_triples=900, seed=1)
    cut = int(0.9 * len(tri))
    dd = tmp_path / "data"
    dd.mkdir()
    _write(str(dd / "entity2id.txt"), [], 120)
    _write(str(dd / "relation2id.txt"), [], 4)
    _write(str(dd / "triple2id.txt"), tri[:cut])
    _write(str(dd / "test2id.txt"), tri[cut:])
    common = ["--data_dir", str(dd), "--model", "transd", "--nbatches", "5", "--hidden_size", "12", "--optimizer", "adagrad",
              "--learning_rate", "0.05", "--loss", "self_adversarial", "--negatives", "8", "--adversarial_temperature", "0.5",
              "--margin", "2"]
    assert D.main(common + ["--output_dir", str(tmp_path / "a"), "--train_times", "3"]) == 0
    out = capsys.readouterr().out
    losses = [float(x) for x in out.split("\n")[1::2][:3]]
    assert len(losses) == 3 and losses[2] < losses[0]
    state = torch.load(tmp_path / "a" / "transd.pt", map_location="cpu")
    assert state["model"] == "transd" and "adagrad_rel_transfer" in state
    assert not any("negatives" in k or "temperature" in k or "loss" in k for k in state)
    # reload, no training, evaluate: the saved tables, ranked
    assert D.main(common + ["--output_dir", str(tmp_path / "b"), "--train_times", "0", "--load", str(tmp_path / "a" / "transd.pt"),
                            "--test_file", str(dd / "test2id.txt")]) == 0
    out = capsys.readouterr().out
    assert any(line.startswith("both:") and "filtered MRR" in line for line in out.splitlines()), out
    again = torch.load(tmp_path / "b" / "transd.pt", map_location="cpu")
    assert all(torch.equal(again[k], state[k]) for k in state if isinstance(state[k], torch.Tensor))
    assert json.load(open(tmp_path / "b" / "transd_test.json"))["sweeps"] == 2 * (len(tri) - cut)


# =============================================================================================== learning
def test_planted_kg_learns_with_the_self_adversarial_loss():
    """TransE on transx_ref.planted_kg(seed=0) with the split and corruption of test_planted_kg_learns_with_adagrad: d 32,
    L1, B = len(train) // 20, K 16, gamma 2, alpha 1, AdaGrad lr 0.05 with accumulator 0.1, 300 steps of the native loop,
    from Xavier-normal tables drawn here with NumPy.  The measure is the fp64 replay of the loop's own batches: the replay
    reaches held-out pairwise accuracy >= 0.887 (the family's hinge-AdaGrad figure at 600 steps) and the GPU's is at
    least the replay's - 0.02."""
    from graphembeddings_amd import evaluate as EV
    tri = XR.planted_kg(seed=0)
    E, R, d, K, steps, lr, gamma, alpha = 2000, 20, 32, 16, 300, 0.05, 2.0, 1.0
    cut = int(0.9 * len(tri))
    train, held = tri[:cut], tri[cut:]
    rng = np.random.default_rng(1)
    corr = held.copy()
    side = rng.integers(0, 2, len(held))
    corr[np.arange(len(held)), side] = rng.integers(0, E, len(held))
    keep = ~np.all(corr == held, 1)
    held, corr = held[keep], corr[keep]
    rng = np.random.default_rng(0)
    tabs = {"ent": (rng.normal(size=(E, d)) * np.sqrt(2 / (E + d))).astype(F32).astype(np.float64),
            "rel": (rng.normal(size=(R, d)) * np.sqrt(2 / (R + d))).astype(F32).astype(np.float64)}
    accs = {k: np.full(v.shape, np.float64(F32(A0))) for k, v in tabs.items()}
    m = _make("transe", tabs, True)
    dheld, dcorr = _dev(held.astype(np.int32)), _dev(corr.astype(np.int32))
    acc = lambda mm: float((mm.score(dheld) < mm.score(dcorr)).float().mean())
    mrr = lambda mm: EV.evaluate_translation(mm, held, tri)["filtered_mrr"]
    acc0, mrr0 = acc(m), mrr(m)
    B = len(train) // 20
    tr = _adv_trainer(m, train, B, K, 3, "adagrad", alpha=alpha, margin=gamma, lr=lr)
    draws = [[x.cpu().numpy() for x in tr.draw(s)] for s in range(steps)]
    losses = tr.run(steps).cpu().numpy()
    assert np.isfinite(losses).all() and losses[-50:].mean() < losses[:50].mean()
    lr32 = float(F32(lr))
    for pos, sd, neg_ent in draws:
        tabs, accs, _ = AR.adagrad_step("transe", tabs, accs, pos, sd, neg_ent, lr32, gamma, alpha, True)
    acc1, mrr1 = acc(m), mrr(m)
    replay = AR.pairwise_accuracy("transe", tabs, held, corr, True)
    m2 = _make("transe", tabs, True)
    mrr_replay = mrr(m2)
    print("planted KG (%d rows, %d train), TransE self-adversarial B %d K %d gamma %g alpha %g, adagrad lr %g, %d steps: "
          "held-out pairwise accuracy untrained %.4f, GPU %.4f, fp64 replay %.4f; filtered MRR untrained %.4f, GPU %.4f, "
          "fp64 replay %.4f" % (len(tri), len(train), B, K, gamma, alpha, lr, steps, acc0, acc1, replay, mrr0, mrr1, mrr_replay))
    assert replay >= 0.887 and acc1 >= replay - 0.02
