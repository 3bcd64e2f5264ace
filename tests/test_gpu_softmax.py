"""GPU: the 1-vs-all softmax objective of ComplEx (ge_softmax_loss / ge_softmax_grad, hole.SoftmaxAdaGrad /
SoftmaxTrainer) against tests/softmax_ref.py.

Tiling of csrc/ge_softmax.hip: tiles of 64 query rows x 64 candidates (so the issue's B in {1, 63, 64, 65, 130} and
K in {1, 2, 63, 64, 65, 129, 300} are its own tile neighbours); the candidates of the query-side sweeps are split into at
most 8 ranges of ceil(tiles / ranges) tiles each -- one tile a range up to K = 512, so K = 577 (10 tiles, 5 ranges of 2)
is added for a range that holds more than one tile and a last range that ends inside a tile; the gradient GEMM's output
is walked in 32-column blocks, two waves a block row: d = 8, 56, 200, 288 are 1, 2, 7 and 9 blocks.

Bounds.  Per case e32 = the largest absolute deviation of softmax_ref's float32 evaluation from its fp64 evaluation,
separately for the loss and for the gradient rows; the GPU must be within 8 * e32 + 1e-7 of the fp64 oracle (the factor
is for the different summation order: tiles, the MFMA's k-ordered chain, partials merged per range).  Every case prints
its four figures (`-s`).

Measured on MI355X: all 528 cases of test_shapes and test_widths are inside the bound; the worst deviation / bound is
0.27 for more than one row and 0.90 for one row (DESIGN.md section 22 has the table).  The cases of ONE query row are the
thin ones: there e32 of the loss is one rounding sample and can be far below the spacing of fp32 at the loss itself
(9.4e-10 at a loss near 5), so only a loss that rounds to the fp32 number nearest the oracle passes -- which is why the
kernel keeps lse as a (max, log sum) pair, sums the score GEMM in four chains and merges the partials in double."""
import functools

import numpy as np
import pytest
import torch

from graphembeddings_amd import evaluate as EV
from graphembeddings_amd import hole as H
from tests import softmax_ref as SR
from tests import transx_ref as XR

pytestmark = pytest.mark.gpu

I32, F32 = np.int32, np.float32
N_REL, EXTRA = 4, 40
A0, DELTA = 0.1, 5e-5                                   # tests/test_gpu_adagrad.py


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(I32) if a.dtype == F32 else a


@functools.lru_cache(maxsize=None)
def build(B, K, d, max_norm, head, seed=0):
    """(table [N,d] f32, hr [B,2], true [B], cand [K]).  Table rows 0..3 are the relations, then K + 40 entities of which K
    (shuffled) are the candidates.  Row norms are log-normal around max_norm (none within 1 % of it, none zero): about
    half the clips active on each operand.  The true candidate sits in column 0, in column K - 1 and on both sides of
    every 64-column boundary.  Rows 0..2 share their fixed entity, which is candidate 0.  Rows with B in (63, 130) all
    share relation 1.  For every fourth row behind those the true candidate's row is -1.5 max_norm Q'_i / |Q'_i| (clipped back to
    max_norm): z_true = scale * max_norm * |Q'_i|, the largest logit the row can have, and p_true is near 1."""
    rng = np.random.default_rng(1000 * B + 7 * K + d + seed)
    n_ent = K + EXTRA
    N = N_REL + n_ent
    t = rng.standard_normal((N, d))
    norms = max_norm * np.exp(rng.normal(0.0, 0.5, N))
    norms = np.where(np.abs(norms / max_norm - 1) < 0.01, 1.05 * max_norm, norms)
    norms[:N_REL] = max_norm * np.array([0.6, 1.7, 0.8, 2.5])
    t = (t * (norms / np.linalg.norm(t, axis=1))[:, None]).astype(F32)
    ents = N_REL + rng.permutation(n_ent)
    cand, extra = ents[:K].astype(I32), ents[K:]
    hr = np.stack([rng.integers(N_REL, N, B), rng.integers(0, N_REL, B)], 1).astype(I32)
    if B in (63, 130):
        hr[:, 1] = 1
    hr[:3, 0] = cand[0]
    cols = sorted({0, K - 1} | {c for b in range(64, K, 64) for c in (b - 1, b)})
    col = rng.integers(0, K, B)
    col[:len(cols)] = cols[:B]
    # every fourth row: its own true column and its own fixed entity, which is no candidate
    special = list(range(len(cols) + 3, B, 4))[:max(0, K - len(cols))]
    free = [c for c in rng.permutation(K) if c not in set(cols)]
    for n, i in enumerate(special):
        col[i] = free[n]
        hr[i, 0] = extra[n % EXTRA]
    for i in special:
        f, r = t[hr[i, 0]].astype(np.float64)[None], t[hr[i, 1]].astype(np.float64)[None]
        q = SR.query(SR._clip(f, max_norm)[0], SR._clip(r, max_norm)[0], head)[0]
        t[cand[col[i]]] = (-1.5 * max_norm * q / np.linalg.norm(q)).astype(F32)
    nrm = np.linalg.norm(t.astype(np.float64), axis=1)
    assert (np.abs(nrm / max_norm - 1) > 0.005).all() and (nrm > 0).all()
    return t, hr, cand[col].astype(I32), cand


@functools.lru_cache(maxsize=None)
def reference(B, K, d, max_norm, scale, head, seed=0):
    """(fp64 loss, idx, val at lr = 1; e32 of the loss; e32 of the gradient rows)."""
    t, hr, true, cand = build(B, K, d, max_norm, head, seed)
    l64, idx, v64 = SR.evaluate(t, hr, true, cand, max_norm, scale, head)
    l32, i32_, v32 = SR.evaluate(t, hr, true, cand, max_norm, scale, head, dtype=np.float32)
    assert np.array_equal(idx, i32_)
    return l64, idx, v64, float(np.nanmax(np.abs(l32 - l64))), float(np.abs(v32 - v64).max())


def gpu_grad(t, hr, true, cand, max_norm, scale, head, lr=1.0):
    loss, gi, gv = H.softmax_grad(dev(t), dev(hr), dev(true), dev(cand), lr, scale=scale, max_norm=max_norm,
                                  side="head" if head else "tail")
    torch.cuda.synchronize()
    return loss.cpu().numpy(), gi.cpu().numpy(), gv.cpu().numpy()


def check_case(B, K, d, max_norm, scale, head):
    t, hr, true, cand = build(B, K, d, max_norm, head)
    l64, idx, v64, e_l, e_g = reference(B, K, d, max_norm, scale, head)
    loss, gi, gv = gpu_grad(t, hr, true, cand, max_norm, scale, head)
    assert np.isfinite(l64).all() and np.array_equal(gi, idx)
    dl, dg = float(np.abs(loss - l64).max()), float(np.abs(gv - v64).max())
    print("SOFTMAX B=%d K=%d d=%d max_norm=%g scale=%g side=%s: loss e32 %.3g gpu %.3g | grad e32 %.3g gpu %.3g"
          % (B, K, d, max_norm, scale, "head" if head else "tail", e_l, dl, e_g, dg))
    assert np.isfinite(loss).all() and np.isfinite(gv).all()
    assert dl <= 8 * e_l + 1e-7, ("loss", dl, e_l)
    assert dg <= 8 * e_g + 1e-7, ("grad", dg, e_g)


NORMS_SCALES = [(1.0, 1.0), (1.0, 20.0), (1.0, 200.0), (4.0, 1.0), (4.0, 20.0), (4.0, 200.0)]


@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("max_norm,scale", NORMS_SCALES)
@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 129, 300, 577])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_shapes(B, K, max_norm, scale, head):
    check_case(B, K, 64, max_norm, scale, head)


@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("max_norm,scale", NORMS_SCALES)
@pytest.mark.parametrize("d", [8, 56, 200, 288])
def test_widths(d, max_norm, scale, head):
    check_case(130, 300, d, max_norm, scale, head)


def test_running_maximum_is_needed():
    """The case a logsumexp without the running maximum fails: at max_norm = 4, scale = 200 the largest logit is far
    beyond log(FLT_MAX) = 88.7, and p_true is near 1 on the rows built for it."""
    l64, idx, v64, _, _ = reference(130, 300, 64, 4.0, 200.0, False)
    t, hr, true, cand = build(130, 300, 64, 4.0, False)
    f, r = SR._clip(t[hr[:, 0]].astype(np.float64), 4.0)[0], SR._clip(t[hr[:, 1]].astype(np.float64), 4.0)[0]
    z = -200.0 * SR.query(f, r, False) @ SR._clip(t[cand].astype(np.float64), 4.0)[0].T
    assert z.max() > 200 and (l64 < 1e-3).sum() >= 10


@pytest.mark.parametrize("head", [False, True])
def test_invalid_rows_and_a_bad_candidate(head):
    """Invalid rows of each kind (fixed, relation or true id outside [0, N); a true id that is no candidate) and one
    candidate id outside [0, N): NaN / -1 / zero rows, and the neighbours' results are bit for bit what they are without
    them (they are appended: the valid rows and candidates keep their tiles)."""
    B, K, d, mn, scale = 65, 129, 64, 1.0, 20.0
    t, hr, true, cand = build(B, K, d, mn, head)
    N = t.shape[0]
    base = gpu_grad(t, hr, true, cand, mn, scale, head)
    outside = int(sorted(set(range(N_REL, N)) - set(cand.tolist()))[0])       # an entity that is no candidate
    hr2 = np.concatenate([hr, [[N, 0], [cand[1], -1], [cand[1], N + 9], [cand[2], 1], [cand[3], 2], [-5, 1]]]).astype(I32)
    true2 = np.concatenate([true, [cand[0], cand[0], cand[0], N, outside, cand[0]]]).astype(I32)
    cand2 = np.concatenate([cand, [N + 3]]).astype(I32)
    loss, gi, gv = gpu_grad(t, hr2, true2, cand2, mn, scale, head)
    l64, idx, v64 = SR.evaluate(t, hr2, true2, cand2, mn, scale, head)
    assert np.isnan(loss[B:]).all() and np.isnan(l64[B:]).all() and np.array_equal(gi, idx)
    assert gi[K] == -1 and not gv[K].any() and (gi[K + 1 + 2 * B:] == -1).all() and not gv[K + 1 + 2 * B:].any()
    assert np.array_equal(bits(loss[:B]), bits(base[0]))
    assert np.array_equal(gi[:K], base[1][:K]) and np.array_equal(bits(gv[:K]), bits(base[2][:K]))
    assert np.array_equal(gi[K + 1:K + 1 + 2 * B], base[1][K:]) and np.array_equal(bits(gv[K + 1:K + 1 + 2 * B]), bits(base[2][K:]))
    _, _, _, e_l, e_g = reference(B, K, d, mn, scale, head)
    assert np.abs(loss[:B] - l64[:B]).max() <= 8 * e_l + 1e-7 and np.abs(gv - v64).max() <= 8 * e_g + 1e-7


@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("B,K,d", [(130, 300, 64), (65, 577, 200), (1, 1, 8)])
def test_exact_properties(B, K, d, head):
    mn, scale = 1.0, 20.0
    t, hr, true, cand = build(B, K, d, mn, head)
    a, b = gpu_grad(t, hr, true, cand, mn, scale, head), gpu_grad(t, hr, true, cand, mn, scale, head)
    for x, y in zip(a, b):                             # two identical calls
        assert np.array_equal(bits(x), bits(y))
    lo = H.softmax_loss(dev(t), dev(hr), dev(true), dev(cand), scale=scale, max_norm=mn, side="head" if head else "tail")
    assert np.array_equal(bits(lo), bits(a[0]))
    half = gpu_grad(t, hr, true, cand, mn, scale, head, lr=0.5)
    assert np.array_equal(half[1], a[1]) and np.array_equal(bits(half[2]), bits((F32(0.5) * a[2]).astype(F32)))
    perm = np.random.default_rng(B).permutation(B)
    p = gpu_grad(t, hr[perm], true[perm], cand, mn, scale, head)
    assert np.array_equal(bits(p[0]), bits(a[0][perm]))
    q = lambda g: g[K:].reshape(B, 2, -1)
    assert np.array_equal(q(p[1])[:, :, 0], q(a[1])[perm][:, :, 0]) and np.array_equal(bits(q(p[2])), bits(q(a[2])[perm]))


def test_host_checks():
    t, hr, true, cand = build(63, 64, 64, 1.0, False)
    T, h, tr, c = dev(t), dev(hr), dev(true), dev(cand)
    for kw in (dict(scale=0.0), dict(scale=float("inf")), dict(scale=20.0, max_norm=0.0), dict(scale=20.0, side="both")):
        with pytest.raises(ValueError):
            H.softmax_loss(T, h, tr, c, **kw)
    with pytest.raises(ValueError):
        H.softmax_loss(T, h[:, :1], tr, c, scale=20.0)
    with pytest.raises(ValueError):
        H.softmax_loss(T, h, tr[:-1], c, scale=20.0)
    with pytest.raises(ValueError):
        H.softmax_loss(T[:, :60].contiguous(), h, tr, c, scale=20.0)


# ------------------------------------------------------------------------------------------------ the step
def step_case():
    """(table, triples [B,3], cand): the tail-side case of build(130, 300, 64) as triples (head, tail, relation); heads
    of rows 0..2 are candidate 0, so that entity is a candidate, a head and (row 5) a tail of the same step."""
    t, hr, true, cand = build(130, 300, 64, 1.0, False)
    tri = np.stack([hr[:, 0], true, hr[:, 1]], 1).astype(I32)
    tri[5, 1] = cand[0]
    # heads must be candidates of the head side: rows whose head is none take candidate 7
    tri[~np.isin(tri[:, 0], cand), 0] = cand[7]
    return t, tri, cand


def check_step(got_t, got_a, ref_t, ref_a, s, counts, lr, gb, steps=1):
    """The per-step bounds of tests/test_gpu_adagrad.py (DELTA on the summed gradient, scaled by max(1, max|s|) on a row
    of more than 16 slots), with the gradient bound gb = 8 e32 + 1e-7 added to DELTA."""
    smax = np.abs(s).max(1, keepdims=True)
    delta = steps * (DELTA * np.where(counts[:, None] > 16, np.maximum(1.0, smax), 1.0) + gb)
    et, ea = np.abs(got_t - ref_t), np.abs(got_a - ref_a)
    bt = np.broadcast_to(lr * delta / np.sqrt(A0), ref_t.shape)
    ba = 2.0 * smax * delta + 4.0 * steps * np.spacing(ref_a.astype(F32)).astype(np.float64)
    print("SOFTMAX step: table err/bound %.3g (|err| %.3g), accumulator err/bound %.3g (|err| %.3g)"
          % ((et / bt).max(), et.max(), (ea / ba).max(), ea.max()))
    assert np.all(et < bt) and np.all(ea < ba)


def test_step():
    t, tri, cand = step_case()
    N, d = t.shape
    B, K, lr, scale = len(tri), len(cand), 0.1, 20.0
    ref_t, ref_a = t.astype(np.float64), np.full((N, d), A0, np.float64)
    ref_loss, s, named = SR.step(ref_t, ref_a, tri, cand, 1.0, scale, lr)
    e = []
    for head, (fx, tr) in ((False, (0, 1)), (True, (1, 0))):
        g64 = SR.evaluate(t, tri[:, [fx, 2]], tri[:, tr], cand, 1.0, scale, head)
        g32 = SR.evaluate(t, tri[:, [fx, 2]], tri[:, tr], cand, 1.0, scale, head, dtype=np.float32)
        e.append((np.abs(g32[0] - g64[0]).max(), np.abs(g32[2] - g64[2]).max()))
    gb = 8 * max(x[1] for x in e) + 1e-7
    counts = np.bincount(np.concatenate([cand, cand, tri[:, 0], tri[:, 1], tri[:, 2], tri[:, 2]]), minlength=N)
    assert counts[cand[0]] >= 6 and counts[tri[0, 2]] > 16 and not named.all()
    emb = dev(t)
    opt = H.SoftmaxAdaGrad(emb, dev(cand), B, scale=scale, initial_accumulator_value=A0)
    assert float(opt.accumulator.min()) == float(opt.accumulator.max()) == F32(A0)
    loss = opt.step(dev(tri), lr)
    torch.cuda.synchronize()
    assert loss.shape == (B, 2)
    assert np.abs(loss.cpu().numpy() - ref_loss).max() <= 8 * max(x[0] for x in e) + 1e-7
    got_t, got_a = emb.cpu().numpy(), opt.accumulator.cpu().numpy()
    check_step(got_t, got_a, ref_t, ref_a, s, counts, lr, gb)
    # rows that are neither candidates nor named by the batch: bit-identical in both arrays
    assert np.array_equal(bits(got_t[~named]), bits(t[~named])) and (got_a[~named] == F32(A0)).all()
    assert (got_a[named] > F32(A0)).any()
    with pytest.raises(ValueError):
        opt.step(dev(tri[:-1]), lr)


def test_step_is_reproducible():
    t, tri, cand = step_case()
    runs = []
    for _ in range(2):
        emb = dev(t)
        opt = H.SoftmaxAdaGrad(emb, dev(cand), len(tri), scale=20.0, initial_accumulator_value=A0)
        for k in range(5):
            opt.step(dev(np.roll(tri, 7 * k, axis=0)), 0.1)
        torch.cuda.synchronize()
        runs.append((emb.cpu().numpy(), opt.accumulator.cpu().numpy()))
    assert np.array_equal(bits(runs[0][0]), bits(runs[1][0])) and np.array_equal(bits(runs[0][1]), bits(runs[1][1]))
    assert not np.array_equal(bits(runs[0][0]), bits(t))


# ------------------------------------------------------------------------------------------------ learning
N_REL_KG, N_ENT_KG, D_KG, B_KG, STEPS_KG, SCALE_KG, LR_KG = 8, 400, 64, 512, 300, 20.0, 0.1


def planted():
    """The planted workload: (train [2776-ish, 3], held out [300, 3], all triples), entity ids shifted behind the 8
    relation rows."""
    tri = XR.planted_kg(n_ent=N_ENT_KG, n_rel=N_REL_KG, dim=8, n_triples=6000, noise=0.05, seed=1).copy()
    tri[:, :2] += N_REL_KG
    test, train = tri[:300], np.unique(tri[300:], axis=0)
    return train.astype(I32), test.astype(I32), tri.astype(I32)


def mrr_host(table, test, all_tri, cand):
    """Filtered MRR, both sides, of an fp64 table with the project's tie rule (holE.py:434: ascending (loss, triple), so
    an equal loss with a smaller candidate id pops first); known triples other than the test triple are skipped."""
    fh = lambda x: SR._clip(x, 1.0)[0]
    rr = []
    for head, (fx, tr) in ((False, (0, 1)), (True, (1, 0))):
        known = {}
        for row in all_tri:
            known.setdefault((int(row[fx]), int(row[2])), set()).add(int(row[tr]))
        S = SR.query(fh(table[test[:, fx]]), fh(table[test[:, 2]]), head) @ fh(table[cand]).T
        for i, row in enumerate(test):
            j = int(np.nonzero(cand == row[tr])[0][0])
            before = (S[i] < S[i, j]) | ((S[i] == S[i, j]) & (cand < row[tr]))
            skip = np.isin(cand, list(known[(int(row[fx]), int(row[2]))] - {int(row[tr])}))
            rr.append(1.0 / (1 + int((before & ~skip).sum())))
    return float(np.mean(rr))


def mrr_gpu(emb, test, all_tri, cand):
    fil = [EV.link_prediction_ranks(emb, test.astype(np.int64), cand.astype(np.int64), known_triples=all_tri.astype(np.int64),
                                    side=side)[1] for side in ("tail", "head")]
    return float(np.mean(1.0 / np.concatenate(fil).astype(np.float64)))


def test_learning():
    """300 steps of SoftmaxTrainer on the planted workload reach the MRR of the same batches run through softmax_ref in
    fp64 (>= 0.40; within 0.03), and the hinge Trainer with AdaGrad after the same 300 steps stays below half of it."""
    train, test, all_tri = planted()
    N = N_REL_KG + N_ENT_KG
    cand = np.arange(N_REL_KG, N, dtype=I32)
    t0 = (np.random.default_rng(0).standard_normal((N, D_KG)) * np.sqrt(2.6 / (N + D_KG))).astype(F32)
    emb = dev(t0)
    tr = H.SoftmaxTrainer(emb, dev(train), dev(cand), B_KG, scale=SCALE_KG, learning_rate=LR_KG, seed=3,
                          initial_accumulator_value=A0)
    twin = H.SoftmaxTrainer(dev(t0), dev(train), dev(cand), B_KG, scale=SCALE_KG, learning_rate=LR_KG, seed=3)
    batches = [twin.next_batch().cpu().numpy() for _ in range(STEPS_KG)]
    loss = tr.run(STEPS_KG, keep_losses=True)
    torch.cuda.synchronize()
    assert loss.shape == (STEPS_KG, B_KG, 2) and tr.global_step == STEPS_KG and torch.isfinite(loss).all()
    assert len(np.unique(np.concatenate(batches[:len(train) // B_KG]), axis=0)) == len(train) // B_KG * B_KG   # no repeats in an epoch
    ref_t, ref_a = t0.astype(np.float64), np.full((N, D_KG), A0, np.float64)
    for b in batches:
        SR.step(ref_t, ref_a, b, cand, 1.0, SCALE_KG, LR_KG)
    ref_mrr, gpu_mrr = mrr_host(ref_t, test, all_tri, cand), mrr_gpu(emb, test, all_tri, cand)
    # the hinge objective, AdaGrad, the same number of steps and batch size: one type holds every entity
    id_to_type = np.where(np.arange(N) < N_REL_KG, -1, 0)
    tt = H.TypeTables.from_host(id_to_type, [0, N_ENT_KG], cand, padded_size=0)
    hemb = dev(t0)
    hinge = H.Trainer(hemb, dev(train), tt, B_KG, margin=0.2, learning_rate=LR_KG, seed=3, optimizer="adagrad",
                      initial_accumulator_value=A0)
    hinge.run(STEPS_KG)
    torch.cuda.synchronize()
    hinge_mrr = mrr_gpu(hemb, test, all_tri, cand)
    hinge.close()
    print("SOFTMAX learning: reference MRR %.4f, GPU MRR %.4f, hinge MRR %.4f" % (ref_mrr, gpu_mrr, hinge_mrr))
    assert ref_mrr >= 0.40
    assert abs(gpu_mrr - ref_mrr) <= 0.03
    assert hinge_mrr < 0.5 * ref_mrr


# ------------------------------------------------------------------------------------------------ the driver
def test_driver_objective_softmax(tmp_path):
    """train.py --objective softmax on the toy KG of tests/test_gpu_train_eval.py: an epoch is batch_count - 1 steps, no
    validation ticks (one log line says why), the checkpoint holds the accumulator and --resume_checkpoint restores both,
    --infer is what it was and ranks far above chance (0.04 over 120 candidates)."""
    from test_gpu_train_eval import _toy_kg
    from graphembeddings_amd import data as D
    from graphembeddings_amd import train as T
    dd = tmp_path / "data"
    dd.mkdir()
    data_dir, out = _toy_kg(dd), str(tmp_path / "run")
    argv = ["--data_dir", data_dir, "--output_dir", out, "--batch_size", "64", "--embedding_dim", "32", "--num_epochs", "30",
            "--learning_rate", "0.1", "--seed", "1", "--objective", "softmax", "--optimizer", "adagrad"]
    FLAGS = T.build_parser().parse_args(argv)
    data = D.init_data(data_dir)
    logs = []
    res = T.run_training(data, FLAGS, log=lambda *a: logs.append(" ".join(str(x) for x in a)))
    batch_count = data.triple_count // 64
    assert res["steps"] == 30 * (batch_count - 1) and np.isfinite(res["final_mean_softmax_loss"])
    assert any("no validation ticks" in l for l in logs) and not any("Validation Loss" in l for l in logs)
    emb, step, acc = T.load_checkpoint(out, with_accumulator=True)
    assert step == res["global_step"] and acc is not None and acc.shape == emb.shape and float(acc.min()) >= F32(0.1)
    assert float(acc[:data.relation_count].max()) > 0.1 and float(acc.max()) > 0.1
    with pytest.raises(Exception, match="already exists"):
        T.run_training(data, FLAGS, log=lambda *a: None)
    res2 = T.run_training(data, T.build_parser().parse_args(argv + ["--resume_checkpoint", "--num_epochs", "1"]),
                          log=lambda *a: None)
    assert res2["steps"] == batch_count - 1 and res2["global_step"] == res["global_step"] + res2["steps"]
    emb2, _, acc2 = T.load_checkpoint(out, with_accumulator=True)
    assert bool((acc2 >= acc).all()) and bool((acc2 > acc).any())          # the accumulator went on from the file's
    m = T.infer_triples(T.build_parser().parse_args(argv + ["--infer", "--infer_threshold", "1.0"]), log=lambda *a: None)
    print("SOFTMAX driver: filtered MRR %.4f after %d steps" % (m["filtered_mrr"], res["steps"] + res2["steps"]))
    assert m["recorded"] == m["sweeps"] == 80 and m["filtered_mrr"] > 0.15
