"""RotatE's self-adversarial negative-sampling loss on the MI355X through graphembeddings_amd.rotate (ge_rotate_adv_*)
against the NumPy restatement tests/rotate_adv_ref.py.

Tolerances: test_gpu_rotate.py's rule, rotate_ref.bound -- 8 e32 + 1e-7 with its one-ulp clause, e32 the largest
deviation of the restatement run in float32 from its fp64 value.  Where heads are replaced the kernel evaluates
|h' - t e^{-i theta}|, so e32 is the larger of the restatement's two forms ("tail": rotate_ref.dist, "head":
rotate_ref.dist_head_form).  `scale` is the largest distance a loss is formed from.  Every block prints its worst
deviation / bound (`-s` shows them).

Shapes.  One workgroup works on a row; its lanes form NT teams that take the row's negatives j = team, team + NT, ...
NT depends on the number of chunks a row is read in (d / 2 scalars, or d / 8 float4 when d % 8 == 0 on 16-byte
aligned tables): NT = 32 up to 8 chunks, 16 up to 16, 8 up to 32, 4 above; a wave holds NT / 4 teams.  The softmax gives
thread x the negatives x, x + 256, ...  So for every d K runs over 1, 2; NT / 4 and NT (the first negative of a second
wave, of a second round), each -1 and +1; 64, 128, 192 (the softmax's waves), 256, 512, 768 (a thread's second, third
and fourth negative), each -1 and +1; and the maximum 1024.
The gradient kernel runs at most 2,048 workgroups, one row each at a time: rows from 2,048 on are a workgroup's second
trip through its loop (test_rows_beyond_the_grid).
"""
import numpy as np
import pytest
import torch

import test_gpu_rotate as TR
from oracle import transx_oracle as TO
from tests import rotate_adv_ref as AR
from tests import rotate_ref as RR

pytestmark = pytest.mark.gpu
F32 = np.float32
A0 = 0.1
near, _dev, _host, _bits, _rand_model = TR.near, TR._dev, TR._host, TR._bits, TR._rand_model


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")


def n_teams(d, shift=0):
    nvec = d // 8 if d % 8 == 0 and shift == 0 else d // 2
    return 32 if nvec <= 8 else 16 if nvec <= 16 else 8 if nvec <= 32 else 4


def _batch(rng, E, R, B, K):
    """Rows over entities [0, E) and relations [0, R); with B >= 2 both sides are in the batch."""
    pos = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, R, B)], 1).astype(np.int32)
    side = rng.integers(0, 2, B).astype(np.int32)
    side[:2] = (0, 1)[:B]
    return pos, side, rng.integers(0, E, (B, K)).astype(np.int32)


def _both32(f, *a, **kw):
    """The restatement in float32 in both forms."""
    return f(*a, dtype=F32, form="tail", **kw), f(*a, dtype=F32, form="head", **kw)


def _check_loss_rows(block, m, tabs, pos, side, neg_ent, margin, alpha):
    l1 = m.l1
    got = m.adv_loss(_dev(pos), _dev(side), _dev(neg_ent), margin, alpha).cpu().numpy()
    ref = AR.row_losses(tabs, pos, side, neg_ent, margin, alpha, l1)
    a32, b32 = _both32(AR.row_losses, tabs, pos, side, neg_ent, margin, alpha, l1)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), block
    ok = ~np.isnan(ref)
    near(block + " loss rows", got[ok], ref[ok], AR.worse32(ref[ok], a32[ok], b32[ok]),
         scale=AR.largest_dist(tabs, pos, side, neg_ent, l1))
    again = m.adv_loss(_dev(pos), _dev(side), _dev(neg_ent), margin, alpha).cpu().numpy()
    assert np.array_equal(got.view(np.int32), again.view(np.int32)), block
    return got


def _run_step(m, opt, pos, side, neg_ent, margin, alpha, lr):
    f = m.adv_adagrad_step if opt == "adagrad" else m.adv_step
    return float(f(_dev(pos), _dev(side), _dev(neg_ent), margin, alpha, lr))


def _check_step(block, make, opt, pos, side, neg_ent, margin, alpha, lr):
    """One step on make()'s tables against the restatement; rows no valid row names bit-identical in every array; two
    runs from one state bit-equal; the batch loss equal to the sum of ge_rotate_adv_loss's rows within the bound."""
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
    l1, lr32 = m.l1, float(F32(lr))
    accs = {k: np.full(v.shape, np.float64(F32(A0))) for k, v in tabs.items()}
    if opt == "adagrad":
        t64, a64, l64 = AR.adagrad_step(tabs, accs, pos, side, neg_ent, lr32, margin, alpha, l1)
        (t32a, a32a, l32a), (t32b, a32b, l32b) = _both32(AR.adagrad_step, tabs, accs, pos, side, neg_ent, lr32, margin, alpha, l1)
    else:
        t64, l64 = AR.sgd_step(tabs, pos, side, neg_ent, lr32, margin, alpha, l1)
        (t32a, l32a), (t32b, l32b) = _both32(AR.sgd_step, tabs, pos, side, neg_ent, lr32, margin, alpha, l1)
    near(block + " loss", loss, l64, AR.worse32(l64, l32a, l32b), scale=AR.largest_dist(tabs, pos, side, neg_ent, l1))
    named = AR.named_rows(tabs, pos, side, neg_ent)
    for k in tabs:
        near(block + " tables", after[k], t64[k], AR.worse32(t64[k], t32a[k], t32b[k]))
        assert np.array_equal(after[k][~named[k]].view(np.int32), before[k][~named[k]].view(np.int32)), (block, k)
        if named[k].any():
            assert (after[k][named[k]] != before[k][named[k]]).any(), (block, k)
        if opt == "adagrad":
            near(block + " accumulators", after_acc[k], a64[k], AR.worse32(a64[k], a32a[k], a32b[k]))
            assert np.array_equal(after_acc[k][~named[k]].view(np.int32), before_acc[k][~named[k]].view(np.int32)), (block, k)
    return tabs


def _margin_for(tabs, pos, side, neg_ent, l1):
    """A margin in the middle of the batch's distances, so that both softplus terms carry weight."""
    P = AR.parts(tabs, pos, side, neg_ent, 0.0, 0.0, l1)
    return float(F32(np.median(np.concatenate([P["Dp"], P["Dn"].ravel()]))))


# =============================================================================================== loss rows, one step
SHAPES = [(2, 0), (6, 0), (8, 0), (64, 0), (96, 0), (200, 0), (1024, 0), (1022, 0), (200, 4)]


def _ks(d, shift):
    nt = n_teams(d, shift)
    edges = [nt // 4, nt, 64, 128, 192, 256, 512, 768]
    return sorted({1, 2, 1024} | {e + o for e in edges for o in (-1, 0, 1) if e + o >= 1})


def test_the_k_lists_cross_every_team_count():
    assert {n_teams(d, s) for d, s in SHAPES} == {32, 16, 8, 4}
    assert n_teams(200, 0) == 8 and n_teams(200, 4) == 4 and n_teams(96, 0) == 16 and n_teams(1022, 0) == 4


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("d,shift", SHAPES)
def test_loss_rows_and_one_step_match_the_restatement(opt, l1, d, shift):
    """E = 61, R = 7; the rows name entities below E - 4 and relations below R - 1, so that the last rows of both tables
    must keep their bits.  B cycles through 65, 3, 1 (3 and 1 above K = 33), alpha through 0, 1, 5."""
    E, R = 61, 7
    seen_B, seen_alpha = set(), set()
    for n, K in enumerate(_ks(d, shift)):
        B = (65, 3, 1)[(n + d) % 3] if K <= 33 else (3, 1)[n % 2]
        alpha = (0.0, 1.0, 5.0)[(n + int(l1) + (opt == "adagrad")) % 3]
        seen_B.add(B); seen_alpha.add(alpha)
        pos, side, neg_ent = _batch(np.random.default_rng(1000 * d + K), E - 4, R - 1, B, K)
        make = lambda: _rand_model(E, R, d, l1, seed=d + K, shift=shift)
        tabs = _host(make())
        margin = _margin_for(tabs, pos, side, neg_ent, l1)
        block = "adv K=%d" % K if K in (1, 1024) else "adv"
        _check_step(block, make, opt, pos, side, neg_ent, margin, alpha, 0.01)
        if opt == "sgd":
            _check_loss_rows(block, make(), tabs, pos, side, neg_ent, margin, alpha)
    assert seen_B == {1, 3, 65} and seen_alpha == {0.0, 1.0, 5.0}


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("d", [8, 6])
def test_rows_beyond_the_grid(opt, l1, d):
    """B = 2,053: workgroups 0..4 take a second row (2,048..2,052) after their first, on the float4 path (d 8) and the
    scalar one (d 6).  Workgroup 1 takes an invalid row, then a valid one; workgroup 2 a valid one, then an invalid one;
    workgroup 3 two invalid ones; workgroups 0 and 4 two valid ones on different sides, one of them with an empty slot
    and the other with every slot empty.  The invalid rows alone name entity E - 1 and relation R - 1."""
    E, R, K, G = 61, 7, 3, 2048
    B = G + 5
    pos, side, neg_ent = _batch(np.random.default_rng(17 + d), E - 1, R - 1, B, K)
    side[[0, G, 4, G + 4]] = (0, 1, 1, 0)
    neg_ent[G, 1] = -1
    neg_ent[G + 4] = (E, -1, E + 7)
    for row, (p, sd) in {1: ((E - 1, E - 1, R - 1), 2), G + 2: ((E, E - 1, R - 1), 0), 3: ((E - 1, -1, R - 1), 1),
                         G + 3: ((E - 1, E - 1, R), 0)}.items():
        pos[row], side[row] = p, sd
        neg_ent[row] = E - 1
    make = lambda: _rand_model(E, R, d, l1, seed=d)
    tabs = _host(make())
    margin = _margin_for(tabs, pos, side, neg_ent, l1)
    _check_step("adv B>2048", make, opt, pos, side, neg_ent, margin, 1.0, 0.002)
    named = AR.named_rows(tabs, pos, side, neg_ent)
    assert not named["ent"][E - 1] and not named["rel"][R - 1]
    if opt == "sgd":
        got = _check_loss_rows("adv B>2048", make(), tabs, pos, side, neg_ent, margin, 1.0)
        assert sorted(np.nonzero(np.isnan(got))[0]) == [1, 3, G + 2, G + 3]
        # rows 2,048.. on their own are the same rows: a first trip and a second trip give the same bits
        tail = make().adv_loss(_dev(pos[G:]), _dev(side[G:]), _dev(neg_ent[G:]), margin, 1.0).cpu().numpy()
        assert np.array_equal(got[G:].view(np.int32), tail.view(np.int32))


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("l1", [True, False])
def test_hot_rows(opt, l1):
    """B = 64, K = 64 over 5 entities and 2 relations: 4,288 slots on 7 keys, every segment cut by many 32-slot windows
    of the apply stage."""
    E, R, B, K, d = 5, 2, 64, 64, 16
    pos, side, neg_ent = _batch(np.random.default_rng(2), E, R, B, K)
    make = lambda: _rand_model(E, R, d, l1, seed=7)
    for alpha in (0.0, 1.0):
        _check_step("adv hot rows", make, opt, pos, side, neg_ent, 4.0 if l1 else 6.0, alpha, 0.01)


@pytest.mark.parametrize("l1", [True, False])
def test_empty_slots_and_invalid_rows(l1):
    """Empty slots (-1 and E), a row with every slot empty, a side of 2, positive ids out of range: each writes what the
    contract says.  The invalid rows alone name entity E - 1 and relation R - 1, which keep their bits."""
    E, R, d, K = 40, 4, 16, 6
    rng = np.random.default_rng(5)
    pos, side, neg_ent = _batch(rng, E - 1, R - 1, 9, K)
    neg_ent[0, [1, 3]] = (-1, E)
    neg_ent[1, :] = (-1, E, -7, E + 5, -1, 1 << 30)
    for row, (p, s) in {2: ((E - 1, E - 1, R - 1), 2), 3: ((E, E - 1, R - 1), 0), 4: ((E - 1, -1, R - 1), 1),
                        5: ((E - 1, E - 1, R), 0), 6: ((E - 1, E - 1, -1), 1), 7: ((E - 1, E - 1, R - 1), -1)}.items():
        pos[row], side[row] = p, s
        neg_ent[row] = E - 1
    make = lambda: _rand_model(E, R, d, l1, seed=3)
    tabs = _host(make())
    got = _check_loss_rows("adv empty/invalid", make(), tabs, pos, side, neg_ent, 3.0, 1.0)
    assert np.array_equal(np.isnan(got), [False, False, True, True, True, True, True, True, False])
    P = AR.parts(tabs, pos, side, neg_ent, 3.0, 1.0, l1)
    one = AR.softplus(P["Dp"][1] - 3.0)                              # the all-empty row: its positive term alone
    near("adv empty/invalid loss rows", got[1:2], [one], [F32(AR.softplus(F32(P["Dp"][1]) - F32(3.0)))], scale=P["Dp"][1])
    for opt in ("sgd", "adagrad"):
        _check_step("adv empty/invalid", make, opt, pos, side, neg_ent, 3.0, 1.0, 0.05)
    named = AR.named_rows(tabs, pos, side, neg_ent)
    assert not named["ent"][E - 1] and not named["rel"][R - 1]
    # a batch of invalid rows alone: loss 0, nothing moves
    m = make()
    before = _bits(m)
    assert _run_step(m, "sgd", pos[2:8], side[2:8], neg_ent[2:8], 3.0, 1.0, 0.05) == 0.0
    assert all(np.array_equal(before[k].view(np.int32), _bits(m)[k].view(np.int32)) for k in before)


def test_int64_ids_beyond_int32_stay_out_of_range():
    """An int64 id that int32 does not hold is an empty slot / an invalid row, not the valid id it would wrap into."""
    E, R, d = 30, 3, 8
    m = _rand_model(E, R, d, True, seed=4)
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
def test_equal_negatives_weigh_as_one(l1):
    """A row whose 64 negatives are one entity has the K = 1 row's loss: the softmax weights sum to 1."""
    E, R, d = 30, 3, 16
    m = _rand_model(E, R, d, l1, seed=9)
    tabs = _host(m)
    pos = np.array([[3, 4, 1], [5, 6, 2]], dtype=np.int32)
    side = np.array([0, 1], dtype=np.int32)
    one = np.array([[11], [12]], dtype=np.int32)
    for alpha in (0.0, 1.0, 5.0):
        got = m.adv_loss(_dev(pos), _dev(side), _dev(np.repeat(one, 64, 1)), 3.0, alpha).cpu().numpy()
        ref = AR.row_losses(tabs, pos, side, one, 3.0, alpha, l1)
        a32, b32 = _both32(AR.row_losses, tabs, pos, side, one, 3.0, alpha, l1)
        near("adv equal negatives", got, ref, AR.worse32(ref, a32, b32), scale=AR.largest_dist(tabs, pos, side, one, l1))


# =============================================================================================== draw and loop
def _adv_trainer(m, tri, B, K, seed, opt="sgd", alpha=1.0, margin=3.0, lr=0.05):
    return m.trainer(tri, B, loss="self_adversarial", negatives=K, adversarial_temperature=alpha, margin=margin,
                     learning_rate=lr, seed=seed, optimizer=opt, initial_accumulator_value=A0)


@pytest.mark.parametrize("K", [1, 5, 64])
def test_draw_matches_the_restatement_and_the_hinge_loops_rows(K):
    tri, E, R = TR._kg(1)
    m = _rand_model(E, R, 8, True, seed=2)
    B, seed = 257, 21
    tr, hinge = _adv_trainer(m, tri, B, K, seed), m.trainer(tri, B, seed=seed)
    assert type(tr).__name__ == "AdvTrainer" and type(hinge).__name__ == "Trainer"
    idx = TO.BernoulliIndex(tri, 0, E, R)
    have = {tuple(x) for x in tri.tolist()}
    for step in (0, 3, (1 << 40) + 5):
        pos, side, neg_ent = (x.cpu().numpy() for x in tr.draw(step))
        hpos, hneg = (x.cpu().numpy() for x in hinge.draw(step))
        assert np.array_equal(pos, hpos)                                    # bit for bit the hinge loop's positives
        assert np.array_equal(side, (hneg[:, 0] != hpos[:, 0]).astype(np.int32))          # ... and its replaced column
        rpos, rside, rneg = AR.draw(tri, idx, seed, step, B, K)
        assert np.array_equal(pos, rpos) and np.array_equal(side, rside) and np.array_equal(neg_ent, rneg)
        assert side.dtype == np.int32 and neg_ent.shape == (B, K) and set(side.tolist()) == {0, 1}
        for i in range(0, B, 7):
            h, t, r = pos[i].tolist()
            assert all(((h, c, r) if side[i] == 0 else (c, t, r)) not in have for c in neg_ent[i].tolist())


def test_draw_gives_minus_ones_where_no_entity_is_free():
    E, R = 3, 2
    tri = np.array([[0, 0, 0], [0, 1, 0], [0, 2, 0], [1, 2, 0], [2, 2, 0], [1, 0, 1]])
    m = _rand_model(E, R, 8, True, seed=2)
    tr = _adv_trainer(m, tri, 200, 4, 3)
    pos, side, neg_ent = (x.cpu().numpy() for x in tr.draw(0))
    rpos, rside, rneg = AR.draw(tri, TO.BernoulliIndex(tri, 0, E, R), 3, 0, 200, 4)
    assert np.array_equal(pos, rpos) and np.array_equal(side, rside) and np.array_equal(neg_ent, rneg)
    none_free = ((pos[:, 0] == 0) & (pos[:, 2] == 0) & (side == 0)) | ((pos[:, 1] == 2) & (pos[:, 2] == 0) & (side == 1))
    assert none_free.any() and (~none_free).any()
    assert (neg_ent[none_free] == -1).all() and (neg_ent[~none_free] >= 0).all()
    assert np.isfinite(tr.run(2).cpu().numpy()).all()                      # such rows train on their positive term alone


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("l1", [True, False])
def test_loop_equals_draws_plus_single_steps_bitwise(opt, l1):
    rng = np.random.default_rng(4)
    E, R, d, B, K, n, seed, lr = 50, 4, 8, 33, 5, 4, 21, 0.05
    tri = np.unique(np.stack([rng.integers(0, E, 600), rng.integers(0, E, 600), rng.integers(0, R, 600)], 1), axis=0)
    a, b = _rand_model(E, R, d, l1, seed=2), _rand_model(E, R, d, l1, seed=2)
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
    # the hinge trainer of the same model is untouched by this one's workspace, and state_dict carries no hyperparameter
    assert set(a.state_dict()) == set(_rand_model(E, R, d, l1, seed=2).state_dict()) | ({"adagrad_init", "adagrad_ent", "adagrad_rel"} if opt == "adagrad" else set())
    assert np.isfinite(a.trainer(tri, B, seed=seed, optimizer=opt).run(2).cpu().numpy()).all()


def test_driver_trains_with_the_self_adversarial_loss(tmp_path, capsys):
    import json
    from graphembeddings_amd import rotate_train as D
    tri = RR.planted_rotation_kg(n_ent=120, n_rel=6, n_triples=1500, seed=2)
    cut = int(0.9 * len(tri))
    d = tmp_path / "data"
    d.mkdir()
    TR._write(str(d / "entity2id.txt"), [], 120)
    TR._write(str(d / "relation2id.txt"), [], 6)
    TR._write(str(d / "triple2id.txt"), tri[:cut])
    TR._write(str(d / "test2id.txt"), tri[cut:])
    common = ["--data_dir", str(d), "--nbatches", "5", "--hidden_size", "16", "--test_file", str(d / "test2id.txt"),
              "--optimizer", "adagrad", "--learning_rate", "0.5", "--loss", "self_adversarial", "--negatives", "8",
              "--adversarial_temperature", "0.5", "--margin", "3"]
    assert D.main(common + ["--output_dir", str(tmp_path / "a"), "--train_times", "2"]) == 0
    out = capsys.readouterr().out
    assert any(line.startswith("both:") and "filtered MRR" in line for line in out.splitlines()), out
    state = torch.load(tmp_path / "a" / "rotate.pt", map_location="cpu")
    assert state["model"] == "rotate" and "adagrad_rel" in state and not any("negatives" in k or "temperature" in k for k in state)
    assert json.load(open(tmp_path / "a" / "rotate_test.json"))["sweeps"] == 2 * (len(tri) - cut)


# =============================================================================================== learning
def test_planted_kg_learns_with_the_self_adversarial_loss():
    """test_gpu_rotate.py's planted rotational KG, split and ent ~ N(0, 0.3^2); d 16, B 512, K 16, gamma 3, alpha 1, AdaGrad
    lr 0.5 with accumulator 0.1, 300 steps.  The fp64 replay of the loop's own batches reaches held-out pairwise accuracy
    >= 0.95 and filtered MRR >= 0.30 (tails and heads, evaluate_translation on the replay's tables); the GPU's accuracy is
    within 0.03 of the replay's.  (The hinge: 0.885 / 0.137 after 3,000 SGD steps, 0.765 / 0.065 after 1,000 AdaGrad
    steps.)"""
    from graphembeddings_amd import evaluate as EV
    P = TR._planted()
    E, R, d, B, K, steps, lr, gamma, alpha = 500, 40, 16, 512, 16, 300, 0.5, 3.0, 1.0
    m = TR._model(E, R, d, l1=True, seed=0)
    m.tables["ent"].copy_(torch.as_tensor(np.random.default_rng(0).normal(size=(E, d)) * 0.3, dtype=torch.float32))
    tabs = _host(m)
    accs = {k: np.full(v.shape, np.float64(F32(A0))) for k, v in tabs.items()}
    held, corr = _dev(P["held"].astype(np.int32)), _dev(P["corr"].astype(np.int32))
    acc = lambda mm: float((mm.score(held) < mm.score(corr)).float().mean())
    mrr = lambda mm: EV.evaluate_translation(mm, P["held"], P["tri"])["filtered_mrr"]
    acc0, mrr0 = acc(m), mrr(m)
    tr = _adv_trainer(m, P["train"], B, K, 3, "adagrad", alpha=alpha, margin=gamma, lr=lr)
    draws = [[x.cpu().numpy() for x in tr.draw(s)] for s in range(steps)]
    losses = tr.run(steps).cpu().numpy()
    assert np.isfinite(losses).all() and losses[-50:].mean() < losses[:50].mean()
    lr32 = float(F32(lr))
    for pos, side, neg_ent in draws:
        tabs, accs, _ = AR.adagrad_step(tabs, accs, pos, side, neg_ent, lr32, gamma, alpha, True)
    acc1, mrr1 = acc(m), mrr(m)
    replay = RR.pairwise_accuracy(tabs, P["held"], P["corr"], True)
    m2 = TR._model(E, R, d, l1=True, seed=0)
    TR._load(m2, tabs)
    mrr_replay = mrr(m2)
    print("planted rotational KG (%d rows, %d train), self-adversarial K %d gamma %g alpha %g, adagrad lr %g, %d steps: "
          "held-out pairwise accuracy untrained %.4f, GPU %.4f, fp64 replay %.4f; filtered MRR untrained %.4f, GPU %.4f, "
          "fp64 replay %.4f" % (len(P["tri"]), len(P["train"]), K, gamma, alpha, lr, steps, acc0, acc1, replay, mrr0, mrr1,
                                mrr_replay))
    assert acc0 <= 0.55 and replay >= 0.95 and mrr_replay >= 0.30 and abs(acc1 - replay) <= 0.03
