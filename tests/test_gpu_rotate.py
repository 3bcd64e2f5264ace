"""RotatE on the MI355X through the C ABI (graphembeddings_amd.rotate) against the NumPy restatement
tests/rotate_ref.py.

Tolerances.  Per case, e32 is the largest deviation of rotate_ref evaluated in float32 from its fp64 value; the GPU must
lie within 8 e32 plus the absolute floor 1e-7 (test_gpu_transx.py's).  This is the factor-8 rule of test_gpu_softmax.py;
the margin is there because the GPU sums in another order.  Only in a case whose e32 is itself below one fp32 ulp of the
case's largest value, 2^-23 max(1, |ref|), one such ulp is added: there the fp32 restatement happens to land on the fp64
values, and a correctly rounded fp32 result may still sit one ulp (1.19e-7 at |ref| <= 1, more above) from them.  For a
batch loss that ulp is taken at the largest distance the loss is formed from (rotate_ref.bound's `scale`).  Every
block of cases prints its worst deviation / bound and each case that needed that term (`-s` shows them).
"""
import numpy as np
import pytest
import torch

from tests import rotate_ref as RR

pytestmark = pytest.mark.gpu
F32 = np.float32
WORST = {}


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")


def near(block, got, ref64, ref32, scale=0.0):
    """assert |got - ref64| <= rotate_bound elementwise; remembers and prints the block's worst deviation / bound, and
    every case that needed the ulp term."""
    got = np.asarray(got, dtype=np.float64)
    if not got.size:
        return
    bound, base, e32 = RR.bound(ref64, ref32, scale)
    err = np.abs(got - np.asarray(ref64, dtype=np.float64))
    ratio = float((err / bound).max())
    if ratio > WORST.get(block, -1.0):
        WORST[block] = ratio
        print("DEV %s: worst deviation / bound %.4g (|err| %.4g, e32 %.4g)" % (block, ratio, float(err.max()), e32))
    if np.any(err > base):
        print("ULP-TERM %s: |err| %.4g above 8 e32 + 1e-7 = %.4g (e32 %.4g, largest |ref| %.4g)"
              % (block, float(err.max()), float(base.min()), e32, float(np.abs(ref64).max())))
    assert np.all(err <= bound), (block, float(err.max()), float(bound.min()), e32)


def _model(E, R, d, l1=True, seed=0):
    from graphembeddings_amd import rotate
    return rotate.RotatE(E, R, d, l1=l1, seed=seed)


def _load(m, tabs):
    for k, v in tabs.items():
        m.tables[k].copy_(torch.as_tensor(np.asarray(v), dtype=torch.float32))


def _host(m, what=None):
    return {k: v.cpu().numpy().astype(np.float64) for k, v in (what or m.tables).items()}


def _bits(m, what=None):
    return {k: v.cpu().numpy().copy() for k, v in (what or m.tables).items()}


def _shift_tables(m, shift):
    """Both tables moved `shift` bytes (a multiple of 4) past a 16-byte boundary: views into buffers one row larger."""
    for k in ("ent", "rel"):
        t = m.tables[k]
        buf = torch.empty(t.numel() + 4, dtype=torch.float32, device="cuda")
        view = buf[shift // 4:shift // 4 + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == shift
        m.tables[k] = view


def _rand_model(E, R, d, l1, seed, theta=np.pi, scale=0.5, shift=0):
    """A model on tables of this file's own: entities N(0, scale^2), phases uniform in [-theta, theta); shift: bytes
    past a 16-byte boundary at which both tables start (not 0: the scalar kernels at any d)."""
    rng = np.random.default_rng(seed)
    m = _model(E, R, d, l1, seed=seed)
    _load(m, {"ent": rng.normal(size=(E, d)) * scale, "rel": rng.uniform(-theta, theta, size=(R, d // 2))})
    if shift:
        _shift_tables(m, shift)
    return m


def _pairs(rng, E, R, B):
    pos = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, R, B)], 1).astype(np.int32)
    neg = pos.copy()
    side = rng.integers(0, 2, B)
    neg[np.arange(B), side] = rng.integers(0, E, B)
    return pos, neg


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


# =============================================================================================== score
BS = (1, 63, 64, 65, 257)


@pytest.mark.parametrize("d", [2, 6, 8, 64, 200, 1024])
def test_score_matches_fp64(d):
    E, R = 61, 7
    for l1 in (True, False):
        m = _rand_model(E, R, d, l1, seed=d)
        tabs = _host(m)
        for B in BS:
            tri = _pairs(np.random.default_rng(B + d), E, R, B)[0]
            got = m.score(_dev(tri)).cpu().numpy()
            near("score", got, RR.dist(tabs, tri, l1), RR.dist(tabs, tri, l1, F32))


def test_score_on_misaligned_tables_takes_the_scalar_path():
    """d = 8 with both tables 4 bytes past a 16-byte boundary: the vector path would fault or read shifted rows."""
    E, R, d = 61, 7, 8
    for l1 in (True, False):
        m = _rand_model(E, R, d, l1, seed=3, shift=4)
        tabs = _host(m)
        for B in BS:
            tri = _pairs(np.random.default_rng(B), E, R, B)[0]
            near("score misaligned", m.score(_dev(tri)).cpu().numpy(), RR.dist(tabs, tri, l1), RR.dist(tabs, tri, l1, F32))


def test_score_bad_ids_are_nan():
    E, R = 10, 2
    m = _model(E, R, 8)
    tri = np.array([[0, 1, 0], [-1, 1, 0], [E, 1, 0], [0, -1, 0], [0, E, 0], [0, 1, -1], [0, 1, R], [3, 3, 1]], dtype=np.int32)
    out = m.score(_dev(tri)).cpu().numpy()
    assert np.array_equal(np.isnan(out), [False, True, True, True, True, True, True, False])


def test_score_with_drifted_phases():
    """|theta| up to 1e3: the accurate sincosf keeps its accuracy there (the fast intrinsic would not)."""
    E, R, d = 61, 7, 64
    for l1 in (True, False):
        m = _rand_model(E, R, d, l1, seed=1, theta=1e3)
        tabs = _host(m)
        assert np.abs(tabs["rel"]).max() > 900
        tri = _pairs(np.random.default_rng(4), E, R, 257)[0]
        near("score |theta| <= 1e3", m.score(_dev(tri)).cpu().numpy(), RR.dist(tabs, tri, l1), RR.dist(tabs, tri, l1, F32))


# =============================================================================================== one step
A0 = 0.1


def _run_step(m, opt, pos, neg, lr, margin):
    f = m.adagrad_step if opt == "adagrad" else m.step
    return float(f(_dev(pos), _dev(neg), lr, margin))


def _check_step(block, E, R, d, l1, opt, pos, neg, lr, margin, seed=0, invalid=(), shift=0):
    """One step on _rand_model's tables against rotate_ref (the pairs listed in `invalid` left out of the reference);
    rows no active pair names bit-identical in every array; two runs from one state bit-equal."""
    outs = []
    for _ in range(2):
        m = _rand_model(E, R, d, l1, seed, shift=shift)
        if opt == "adagrad":
            m.enable_adagrad(A0)
        before, before_acc = _bits(m), (_bits(m, m.accumulators) if opt == "adagrad" else {})
        tabs = _host(m)
        loss = _run_step(m, opt, pos, neg, lr, margin)
        outs.append((loss, _bits(m), _bits(m, m.accumulators) if opt == "adagrad" else {}))
    assert outs[0][0] == outs[1][0]
    for arrs in (1, 2):
        for k in outs[0][arrs]:
            assert np.array_equal(outs[0][arrs][k], outs[1][arrs][k]), (k, "two runs differ")
    loss, after, after_acc = outs[0]
    keep = np.ones(len(pos), dtype=bool)
    keep[list(invalid)] = False
    p, n = pos[keep], neg[keep]
    lr32, accs = float(F32(lr)), {k: np.full(v.shape, np.float64(F32(A0))) for k, v in tabs.items()}
    act = RR.active_mask(tabs, p, n, margin, l1)
    assert np.array_equal(act, RR.active_mask(tabs, p, n, margin, l1, F32)), "a pair too close to z = 0 for this test"
    assert 0 < act.sum()
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
    return act


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("d,shift", [(2, 0), (6, 0), (8, 0), (64, 0), (200, 0), (1024, 0), (1022, 0), (200, 4)])
def test_one_step_matches_rotate_ref(opt, l1, d, shift):
    """B = 500 over 300 entities and 9 relations; margin 0, so that a good part of the pairs is inactive; pairs with an id
    out of range or another relation in the negative, which name entity E - 1 and relation R - 1 alone, write nothing.
    The last three shapes run the gradient kernel's 64-lane groups, whose lanes hold more than one chunk of cached
    rotations: d = 1024 on the float4 path (128 chunks: two per lane), d = 1022 on the scalar path (511: eight per lane,
    the last ragged) and d = 200 on tables 4 bytes off a 16-byte boundary (the scalar path at 100: two per lane)."""
    E, R, B = 300, 9, 500
    pos, neg = _pairs(np.random.default_rng(11), E - 1, R - 1, B)
    bad = [3, 77, 250, 499]
    pos[bad] = [[E - 1, 5, R - 1], [E - 1, E, 0], [-1, E - 1, R - 1], [E - 1, 6, R]]
    neg[bad] = [[E - 1, 9, 0], [E - 1, 7, 0], [E - 1, 2, R - 1], [E - 1, 6, R]]
    act = _check_step("step", E, R, d, l1, opt, pos, neg, 0.01, 0.0, seed=d, invalid=bad, shift=shift)
    assert act.sum() < len(act)                             # inactive pairs were there


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("l1", [True, False])
def test_hot_rows(opt, l1):
    """Every pair on one relation (a 300-slot relation row, k floats wide); entity 17 the head of 70 positives and their
    negatives (140 slots: its run is cut by more than two window edges of 32); one pair whose head is its tail."""
    E, R, B, d = 200, 5, 300, 16
    pos, neg = _pairs(np.random.default_rng(2), E, R, B)
    pos[:, 2] = neg[:, 2] = 3
    pos[100:170, 0] = neg[100:170, 0] = 17
    neg[100:170, 1] = np.random.default_rng(3).integers(0, E, 70)
    pos[5] = [40, 40, 3]
    neg[5] = [40, 41, 3]
    act = _check_step("step hot rows", E, R, d, l1, opt, pos, neg, 0.01, 8.0 if l1 else 16.0, seed=7)
    assert act[100:170].sum() > 64 and act[5]


def test_exact_fixture_squared_norm():
    """theta = 0, integer coordinates, squared norm: the loss, the activity (pair 0 sits at z == 0 exactly and is active)
    and every summed row equal the integer arithmetic bit for bit."""
    E, R, d, B, lr = 40, 3, 8, 200, 0.5
    tabs = RR.exact_tables_l2(E, R, d, seed=4)
    pos, neg = _pairs(np.random.default_rng(6), E, R, B)
    margin = float(RR.dist(tabs, neg[:1], False)[0] - RR.dist(tabs, pos[:1], False)[0])
    act = RR.active_mask(tabs, pos, neg, margin, False)
    assert act[0] and 0 < act.sum() < B
    new, loss = RR.sgd_step(tabs, pos, neg, lr, margin, False)
    m = _model(E, R, d, l1=False)
    _load(m, tabs)
    got = _run_step(m, "sgd", pos, neg, lr, margin)
    assert got == loss and loss == np.round(loss)
    for k in tabs:
        assert np.array_equal(new[k], new[k].astype(F32).astype(np.float64))          # fp32 holds the expectation
        assert np.array_equal(m.tables[k].cpu().numpy(), new[k].astype(F32)), k
    # without pair 0 the loss is the same (its term is 0) but its rows move: it was active
    _load(m, tabs)
    assert _run_step(m, "sgd", pos[1:], neg[1:], lr, margin) == loss
    assert not np.array_equal(m.tables["ent"].cpu().numpy(), new["ent"].astype(F32))


def test_exact_fixture_modulus_norm():
    """theta = 0, heads real powers of two, tails h - n (3 + 4i): every modulus is the integer 5 |n|, so the loss and the
    activity are exact (pair 0 at z == 0, active; pair 1 inactive).  Every row is named by one slot only, and each
    gradient entry is one correctly rounded quotient (3n / 5|n|, 4n / 5|n|) or one exact product with a power of two, so
    the updated rows equal the restatement run in float32 bit for bit."""
    B, d, lr = 8, 8, 0.5
    k, E, R = d // 2, 4 * B, B
    rng = np.random.default_rng(8)
    ent = np.zeros((E, d))
    for e in range(0, E, 2):                                # (e, e + 1) = (head, tail) of a positive or a negative
        ent[e, :k] = rng.choice([-4, -2, -1, 1, 2, 4], k)
        n = rng.integers(-2, 3, k)
        ent[e + 1, :k], ent[e + 1, k:] = ent[e, :k] - 3 * n, -4 * n
    tabs = {"ent": ent, "rel": np.zeros((R, k))}
    i = np.arange(B)
    pos, neg = np.stack([4 * i, 4 * i + 1, i], 1).astype(np.int32), np.stack([4 * i + 2, 4 * i + 3, i], 1).astype(np.int32)
    ent[1, :k], ent[1, k:] = ent[0, :k], 0.0                # pair 0: D+ = 0 (u = 0 in every coordinate), D- = 60
    ent[3, :k], ent[3, k:] = ent[2, :k] - 3 * 3, -4 * 3
    ent[5, :k], ent[5, k:] = ent[4, :k], 0.0                # pair 1: D+ = 0, D- = 180: inactive
    ent[7, :k], ent[7, k:] = ent[6, :k] - 3 * 9, -4 * 9
    dp, dn = RR.dist(tabs, pos), RR.dist(tabs, neg)
    assert np.array_equal(dp % 5, np.zeros(B)) and np.array_equal(dn % 5, np.zeros(B))
    margin = float(dn[0] - dp[0])
    act = RR.active_mask(tabs, pos, neg, margin, True)
    assert margin == 60.0 and act[0] and not act[1] and act.sum() == B - 1
    new32, loss32 = RR.sgd_step(tabs, pos, neg, lr, margin, True, F32)
    new64, loss64 = RR.sgd_step(tabs, pos, neg, lr, margin, True)
    assert loss32 == loss64 == np.round(loss64)
    m = _model(E, R, d, l1=True)
    _load(m, tabs)
    assert _run_step(m, "sgd", pos, neg, lr, margin) == loss64
    for key in tabs:
        assert new32[key].dtype == F32 and np.abs(new32[key] - new64[key]).max() < 1e-6
        assert np.array_equal(m.tables[key].cpu().numpy().view(np.int32), new32[key].view(np.int32)), key
    assert np.array_equal(m.tables["ent"].cpu().numpy()[4:8], ent[4:8].astype(F32))      # the inactive pair's rows


# =============================================================================================== the native loop
def _kg(seed=0, E=300, R=8, T=3000):
    rng = np.random.default_rng(seed)
    tri = np.stack([rng.integers(0, E, T), rng.integers(0, E, T), rng.integers(0, R, T)], 1)
    tri[:400, 2] = 0                                          # one busy relation
    return np.unique(tri, axis=0).astype(np.int64), E, R


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("l1", [True, False])
def test_loop_equals_draws_plus_single_steps_bitwise(opt, l1):
    tri, E, R = _kg(1)
    B, n, seed, lr = 700, 5, 21, 0.05
    a, b = _rand_model(E, R, 48, l1, seed=2), _rand_model(E, R, 48, l1, seed=2)
    tr = a.trainer(tri, B, margin=1.0, learning_rate=lr, seed=seed, optimizer=opt)
    if opt == "adagrad":
        b.enable_adagrad(0.1)
    la = tr.run(n).cpu().numpy()
    for s in range(n):
        pos, neg = tr.draw(s)
        assert torch.equal(pos[:, 2], neg[:, 2])
        lb = float((b.adagrad_step if opt == "adagrad" else b.step)(pos, neg, lr, 1.0))
        assert lb == la[s], s
    assert la[0] > 0
    for k in a.tables:
        assert torch.equal(a.tables[k], b.tables[k]), k
        if opt == "adagrad":
            assert torch.equal(a.accumulators[k], b.accumulators[k]), k


def test_state_dict_round_trip():
    m = _model(20, 3, 8, seed=1)
    m.enable_adagrad(0.25)
    pos, neg = _pairs(np.random.default_rng(0), 20, 3, 16)
    m.adagrad_step(_dev(pos), _dev(neg), 0.1, 1.0)
    state = m.state_dict()
    assert state["model"] == "rotate" and set(state) >= {"ent", "rel", "adagrad_init", "adagrad_ent", "adagrad_rel", "l1", "d"}
    assert tuple(state["rel"].shape) == (3, 4) and tuple(state["adagrad_rel"].shape) == (3, 4)
    m2 = _model(20, 3, 8, seed=2)
    m2.load_state_dict(state)
    for k in m.tables:
        assert torch.equal(m.tables[k], m2.tables[k]) and torch.equal(m.accumulators[k], m2.accumulators[k])
    assert m2.adagrad_init == 0.25
    from graphembeddings_amd import transx
    with pytest.raises(ValueError, match="model"):
        transx.TransX("transe", 20, 3, 8).load_state_dict(state)
    rel = m.tables["rel"].cpu().numpy()
    init = _model(500, 40, 16, seed=0).tables["rel"].cpu().numpy()
    assert init.min() >= -np.pi and init.max() < np.pi and init.std() > 1.5 and rel.shape == (3, 4)


# =============================================================================================== ranks
def _cells(m, test, known, side):
    from graphembeddings_amd import evaluate as EV
    n_rows = max(m.n_ent, m.n_rel)
    idx = EV.KnownIndex(known, n_rows, side, "cuda")
    pos_of = torch.arange(n_rows, dtype=torch.int64, device="cuda")
    pos_of[m.n_ent:] = -1
    t = torch.as_tensor(test).cuda()
    return idx.cells(t[:, 0 if side == "tail" else 1], t[:, 2], pos_of, m.n_ent)


def _known_mask(test, known, E, side):
    """[n, E] bool: cell (i, c) is known iff the row with c in the candidate's place is a known triple."""
    have = {tuple(x) for x in np.asarray(known).tolist()}
    km = np.zeros((len(test), E), dtype=bool)
    for i, (h, t, r) in enumerate(np.asarray(test).tolist()):
        for c in range(E):
            km[i, c] = ((h, c, r) if side == "tail" else (c, t, r)) in have
    return km


def _rank_call(m, test, known, side):
    off, rc = _cells(m, test, known, side)
    return [x.cpu().numpy() for x in m.rank_counts(_dev(test), cand_is_head=side == "head", known_off=off, known_rc=rc,
                                                   return_scores=True)]


@pytest.mark.parametrize("d", [6, 64])
@pytest.mark.parametrize("E", [1, 255, 256, 257, 600])
def test_ranks(E, d):
    """Rows of several relations in any order, both sides, both norms, B in {1, 15, 16, 17, 40}.  (a) the counts and the
    filtered counts equal, for every row, the counts recomputed on the host from the call's own scores_out and true_dist
    with the (D, id) rule; (b) scores_out and true_dist within the bound of fp64; (c) true_dist within the bound of
    ge_rotate_score on the same rows; two calls bit-equal."""
    R = 5
    for l1 in (True, False):
        m = _rand_model(E, R, d, l1, seed=E + d)
        tabs = _host(m)
        for side in ("tail", "head"):
            for B in (1, 15, 16, 17, 40) + ((130,) if (E, d) == (257, 6) else ()):    # 130: a second 128-row tile of known cells
                rng = np.random.default_rng(B + E)
                test = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, R, B)], 1)
                known = test[rng.integers(0, B, 40 * B)]                        # about 40 known cells per row ...
                known[:, 1 if side == "tail" else 0] = rng.integers(0, E, 40 * B)
                known = np.concatenate([known, test[: (B + 1) // 2]], 0)        # ... and half of the targets themselves
                nb, nk, td, sc = _rank_call(m, test, known, side)
                target = test[:, 0] if side == "head" else test[:, 1]
                km = _known_mask(test, known, E, side)
                snb, snk = RR.counts_from(sc, td, target, km)                   # (a): exact, every row
                assert np.array_equal(nb, snb) and np.array_equal(nk, snk), (l1, side, B)
                assert np.array_equal(td.view(np.int32), sc[np.arange(B), target].view(np.int32))
                _, _, td64, sc64 = RR.ranks(tabs, test, side, l1)
                _, _, td32, sc32 = RR.ranks(tabs, test, side, l1, dtype=F32)
                near("rank scores_out", sc, sc64, sc32)                         # (b)
                near("rank true_dist", td, td64, td32)
                score = m.score(_dev(test.astype(np.int32))).cpu().numpy()      # (c): two roundings of one number
                form = RR.dist(tabs, test, l1, F32)                             # ... the larger e32 of the two forms
                worse = form if np.abs(form - td64).max() > np.abs(td32 - td64).max() else td32
                assert np.all(np.abs(td.astype(np.float64) - score) <= RR.bound(td64, worse)[0]), (l1, side, B)
                again = _rank_call(m, test, known, side)
                for x, y in zip((nb, nk, td, sc), again):
                    assert np.array_equal(x.view(np.int32), y.view(np.int32))
                if E > 1 and B == 40:
                    assert (nk > 0).any() and (nb > nk).any()


@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("side", ["tail", "head"])
def test_ranks_exact_fixture_with_ties(l1, side):
    """(d) theta = 0 and integer coordinates (collinear multiples of 3 + 4i for the modulus norm): every distance is an
    integer fp32 holds, many candidates tie with the target, and the ranks equal the fp64 ranks outright."""
    E, R, d, B = 300, 3, 6, 40
    tabs = RR.collinear_tables(E, R, d, seed=1, amp=1) if l1 else RR.exact_tables_l2(E, R, d, seed=1, amp=1)
    m = _model(E, R, d, l1)
    _load(m, tabs)
    rng = np.random.default_rng(3)
    test = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, R, B)], 1)
    known = np.concatenate([np.stack([rng.integers(0, E, 2000), rng.integers(0, E, 2000), rng.integers(0, R, 2000)], 1),
                            test[:20], test[:5]], 0)
    km = _known_mask(test, known, E, side)
    enb, enk, etd, esc = RR.ranks(tabs, test, side, l1, km)
    nb, nk, td, sc = _rank_call(m, test, known, side)
    assert np.array_equal(sc.astype(np.float64), esc) and np.array_equal(td.astype(np.float64), etd)
    assert np.array_equal(nb, enb) and np.array_equal(nk, enk)
    assert ((esc == etd[:, None]).sum(1) > 3).all() and (enk > 0).any()         # planted ties on every row
    raw, fil = m.ranks(test, known, side=side)
    assert np.array_equal(raw, enb + 1) and np.array_equal(fil, enb + 1 - enk)


def test_ranks_bad_ids():
    """(e) -1 / -1 / NaN for a row with an id out of range; its neighbours are ranked as if it were not there."""
    E, R, d = 300, 4, 8
    m = _rand_model(E, R, d, True, seed=5)
    good = np.array([[1, 2, 0], [3, 4, 1], [5, 6, 2], [7, 8, 3], [9, 10, 0], [11, 12, 1], [13, 14, 2], [15, 16, 3],
                     [17, 299, 0], [0, 18, 3]])
    test = good.copy()
    bad = {0: (0, -1), 2: (0, E), 3: (1, -1), 4: (1, E), 5: (2, -1), 6: (2, R)}
    for row, (col, val) in bad.items():
        test[row, col] = val
    for side in ("tail", "head"):
        nb, nk, td = [x.cpu().numpy() for x in m.rank_counts(_dev(test), cand_is_head=side == "head")]
        gb, gk, gd = [x.cpu().numpy() for x in m.rank_counts(_dev(good), cand_is_head=side == "head")]
        for row in range(len(test)):
            if row in bad:
                assert nb[row] == -1 and nk[row] == -1 and np.isnan(td[row])
            else:
                assert nb[row] == gb[row] and nk[row] == 0 and td[row] == gd[row]
    with pytest.raises(ValueError):
        m.ranks(test)


def test_out_of_scope_operations_raise():
    m = _model(30, 3, 8)
    q = _dev(np.zeros((2, 2), dtype=np.int32))
    t = np.zeros((2, 3), dtype=np.int64)
    from graphembeddings_amd import evaluate as EV
    for what, f in (("top-k", lambda: m.predict(q, 3)), ("relation", lambda: m.relation_ranks(t)),
                    ("relation", lambda: EV.evaluate_translation(m, t, t, relations=True)),
                    ("candidate sets", lambda: m.ranks(t, candidate_sets=object()))):
        with pytest.raises(NotImplementedError, match=what):
            f()


def _write(path, rows, count=None):
    with open(path, "w") as f:
        f.write(f"{len(rows) if count is None else count}\n")
        for r in rows:
            f.write(" ".join(str(int(x)) for x in r) + "\n")


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
def test_driver_trains_evaluates_and_reloads(tmp_path, capsys, opt):
    """rotate_train's main(): two epochs, rotate.pt and rotate_test.json; --load with --train_times 0 gives the same
    evaluation; with AdaGrad the saved file carries the accumulators."""
    import json
    from graphembeddings_amd import rotate_train as D
    tri = RR.planted_rotation_kg(n_ent=120, n_rel=6, n_triples=1500, seed=2)
    cut = int(0.9 * len(tri))
    d = tmp_path / "data"
    d.mkdir()
    _write(str(d / "entity2id.txt"), [], 120)
    _write(str(d / "relation2id.txt"), [], 6)
    _write(str(d / "triple2id.txt"), tri[:cut])
    _write(str(d / "test2id.txt"), tri[cut:])
    _write(str(d / "valid2id.txt"), tri[cut:cut + 20])
    common = ["--data_dir", str(d), "--nbatches", "5", "--hidden_size", "16", "--test_file", str(d / "test2id.txt"),
              "--filter_file", str(d / "valid2id.txt"), "--optimizer", opt, "--learning_rate", "0.05"]
    assert D.main(common + ["--output_dir", str(tmp_path / "a"), "--train_times", "2"]) == 0
    out = capsys.readouterr().out
    for side in ("tail:", "head:", "both:"):
        assert any(line.startswith(side) and "filtered MRR" in line for line in out.splitlines()), out
    j1 = json.load(open(tmp_path / "a" / "rotate_test.json"))
    assert j1["sweeps"] == 2 * (len(tri) - cut)
    state = torch.load(tmp_path / "a" / "rotate.pt", map_location="cpu")
    assert state["model"] == "rotate" and tuple(state["rel"].shape) == (6, 8)
    assert ("adagrad_rel" in state) == (opt == "adagrad")
    assert D.main(common + ["--output_dir", str(tmp_path / "b"), "--train_times", "0", "--load",
                            str(tmp_path / "a" / "rotate.pt")]) == 0
    assert json.load(open(tmp_path / "b" / "rotate_test.json")) == j1


# =============================================================================================== learning
_PLANTED = {}


def _planted():
    """The planted rotational KG, its 90/10 split and the corrupted held-out rows, built once."""
    if not _PLANTED:
        tri = RR.planted_rotation_kg()
        cut = int(0.9 * len(tri))
        train, held = tri[:cut], tri[cut:]
        rng = np.random.default_rng(1)
        corr = held.copy()
        side = rng.integers(0, 2, len(held))
        corr[np.arange(len(held)), side] = rng.integers(0, 500, len(held))
        keep = ~np.all(corr == held, 1)
        _PLANTED.update(tri=tri, train=train, held=held[keep], corr=corr[keep])
    return _PLANTED


def _learn(opt, lr, steps):
    """(untrained, GPU, replay) held-out pairwise accuracies D(true) < D(corrupted) and (untrained, trained) filtered MRR.
    The replay is rotate_ref's fp64 step on the loop's own batches (trainer.draw(s))."""
    from graphembeddings_amd import evaluate as EV
    P = _planted()
    E, R, d, B = 500, 40, 16, 512
    m = _model(E, R, d, l1=True, seed=0)
    m.tables["ent"].copy_(torch.as_tensor(np.random.default_rng(0).normal(size=(E, d)) * 0.3, dtype=torch.float32))
    tabs = _host(m)
    accs = {k: np.full(v.shape, np.float64(F32(A0))) for k, v in tabs.items()}
    held, corr = _dev(P["held"].astype(np.int32)), _dev(P["corr"].astype(np.int32))
    acc = lambda: float((m.score(held) < m.score(corr)).float().mean())
    acc0, mrr0 = acc(), EV.evaluate_translation(m, P["held"], P["tri"])["filtered_mrr"]
    tr = m.trainer(P["train"], B, margin=1.0, learning_rate=lr, seed=3, optimizer=opt, initial_accumulator_value=A0)
    draws = [tr.draw(s) for s in range(steps)]
    pos = torch.stack([p for p, _ in draws]).cpu().numpy()
    neg = torch.stack([n for _, n in draws]).cpu().numpy()
    losses = tr.run(steps).cpu().numpy()
    assert np.isfinite(losses).all() and losses[-50:].mean() < losses[:50].mean()
    lr32 = float(F32(lr))
    for s in range(steps):
        if opt == "adagrad":
            tabs, accs, _ = RR.adagrad_step(tabs, accs, pos[s], neg[s], lr32, 1.0, True)
        else:
            tabs, _ = RR.sgd_step(tabs, pos[s], neg[s], lr32, 1.0, True)
    acc1, mrr1 = acc(), EV.evaluate_translation(m, P["held"], P["tri"])["filtered_mrr"]
    replay = RR.pairwise_accuracy(tabs, P["held"], P["corr"], True)
    print("planted rotational KG (%d rows, %d train), %s lr %g, %d steps: held-out pairwise accuracy untrained %.4f, "
          "GPU %.4f, fp64 replay %.4f; filtered MRR untrained %.4f, trained %.4f"
          % (len(P["tri"]), len(P["train"]), opt, lr, steps, acc0, acc1, replay, mrr0, mrr1))
    return acc0, acc1, replay


def test_triple_classification_works_unchanged():
    """classify.triple_classification needs only score and the sampler: after 600 AdaGrad steps the per-relation
    thresholds separate held-out triples from drawn negatives better than the untrained table does."""
    P = _planted()
    half = len(P["held"]) // 2
    valid, test = P["held"][:half], P["held"][half:]
    m = _model(500, 40, 16, l1=True, seed=0)
    before = m.triple_classification(valid, test, known=P["tri"], seed=1)
    m.trainer(P["train"], 512, margin=1.0, learning_rate=0.5, seed=3, optimizer="adagrad").run(600)
    after = m.triple_classification(valid, test, known=P["tri"], seed=1)
    print("triple classification on the planted rotational KG: accuracy %.4f untrained, %.4f trained" % (before["accuracy"], after["accuracy"]))
    # positives and drawn negatives are balanced: 0.5 is chance
    assert after["n"] == before["n"] > len(test) and after["accuracy"] > max(before["accuracy"], 0.55)


def test_planted_kg_learns_sgd():
    """d = 16, B = 512, margin 1, modulus norm, ent N(0, 0.3^2), SGD lr 0.01, 3,000 steps: the fp64 replay of the loop's
    own batches reaches >= 0.80 held-out pairwise accuracy, the GPU is within 0.03 of it, the untrained table <= 0.55."""
    acc0, acc1, replay = _learn("sgd", 0.01, 3000)
    assert acc0 <= 0.55 and replay >= 0.80 and abs(acc1 - replay) <= 0.03


def test_planted_kg_learns_adagrad():
    """The shorter case: AdaGrad lr 0.5, 1,000 steps, replay >= 0.75, same closeness."""
    acc0, acc1, replay = _learn("adagrad", 0.5, 1000)
    assert acc0 <= 0.55 and replay >= 0.75 and abs(acc1 - replay) <= 0.03
