"""GPU: triple classification (graphembeddings_amd.classify over ge_threshold_fit / ge_threshold_classify) against the
numpy reference tests/classify_ref.py.  Every comparison is exact: the fit's outputs are integers or copies of input
floats, the decision is a comparison, and the resolved threshold is one fp64 midpoint rounded once."""
import json

import numpy as np
import pytest
import torch

from tests import classify_ref as R
from tests import transx_ref as XR

pytestmark = pytest.mark.gpu

I32, F32, U8 = np.int32, np.float32, np.uint8
FIELDS = ("thr_lo", "thr_hi", "best_correct", "n_pos", "n_neg")
SCORES = ("continuous", "four_values", "all_equal", "tie_runs", "nan_tail", "pos_inf")
LABELS = ("random", "all_pos", "all_neg", "separable", "inverted")


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")


def C():
    from graphembeddings_amd import classify
    return classify


def T():
    return C().FIT_TILE


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(I32) if a.dtype == F32 else a,
                                                                        b.view(I32) if b.dtype == F32 else b)


def check_accuracies(stats, conf, n):
    """Overall accuracy is one division of equal integers: exact.  Macro accuracy is a float64 mean of at most n_rel
    ratios in [0, 1], summed in another order on each side: each sum is within n_rel * 2^-53 of the true one."""
    acc, macro = R.accuracies(conf)
    assert stats["accuracy"] == acc and stats["n"] == n
    assert abs(stats["macro_accuracy"] - macro) <= len(conf) * 2.0 ** -52


def make_scores(kind, M, rng):
    s = rng.standard_normal(M).astype(F32)
    if kind == "four_values":
        s = rng.choice(np.array([-1.5, 0.25, 0.5, 3.0], F32), M)
    elif kind == "all_equal":
        s = np.full(M, 0.75, F32)
    elif kind == "nan_tail":
        s[rng.random(M) < 0.25] = np.nan
    elif kind == "pos_inf":
        s[rng.random(M) < 0.2] = np.inf
    return s


def make_labels(kind, score, rng):
    M = len(score)
    if kind == "random":
        return rng.integers(0, 2, M).astype(U8)
    if kind == "all_pos":
        return np.ones(M, U8)
    if kind == "all_neg":
        return np.zeros(M, U8)
    cut = np.nanmedian(score) if np.isfinite(score).any() else 0.0
    with np.errstate(invalid="ignore"):
        below = score <= cut                             # (a NaN is never below: it falls on the rejected side)
    return (below if kind == "separable" else ~below).astype(U8)


def make_segments(M, n_seg, rng):
    if n_seg == M:
        return rng.permutation(M).astype(I32)           # singletons
    return rng.integers(0, n_seg, M).astype(I32)


def tie_runs_across_tiles(score, seg):
    """On SORTED input: a run of equal scores laid across every tile boundary that falls inside a segment."""
    score = score.copy()
    for b in range(T(), len(score), T()):
        s = seg[b]
        lo, hi = b, b
        while lo > b - 3 and lo > 0 and seg[lo - 1] == s:
            lo -= 1
        while hi < b + 3 and hi < len(score) and seg[hi] == s:
            hi += 1
        score[lo:hi] = score[lo]                        # the smallest of the range: the order stays ascending
    return score


def sorted_case(score, seg, label, kind):
    o = R.sort_order(score, seg)
    score, seg, label = score[o], seg[o], label[o]
    if kind == "tie_runs":
        score = tie_runs_across_tiles(score, seg)
    return score, seg, label


def gpu_fit_raw(score, seg, label, n_seg):
    out = C().fit_raw(dev(score), dev(seg), dev(label), n_seg)
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_fit_raw(score, seg, label, n_seg, what):
    """ge_threshold_fit on the sorted arrays as given, at exactly this M: the five outputs bit-equal."""
    got, ref = gpu_fit_raw(score, seg, label, n_seg), R.fit(score, seg, label, n_seg)
    for k in FIELDS:
        assert same(got[k], ref[k]), (what, k, np.nonzero(got[k] != ref[k])[0][:5])
    return ref


def check_public_path(score, seg, label, n_seg, what):
    """fit_thresholds (its own sort, the global segment), resolve in both modes and fallbacks, classify on the
    UNSORTED input: all bit-equal to the reference."""
    cl = C()
    th = cl.fit_thresholds(dev(score), dev(seg), dev(label), n_seg)
    per, glob = R.fit(score, seg, label, n_seg), R.fit(score, np.zeros(len(score), I32), label, 1)
    for k in FIELDS:
        assert same(getattr(th, k).cpu().numpy(), per[k]), (what, k)
        assert same(getattr(th, "global_" + k).cpu().numpy(), glob[k]), (what, "global", k)
    for mode in ("mid", "lo"):
        for fb in ("global", "none"):
            thr = th.resolve(mode, fb)
            ref_thr = R.resolve(per, glob, mode, fb)
            assert same(thr.cpu().numpy(), ref_thr), (what, mode, fb)
            assert same(th.cpu().resolve(mode, fb).numpy(), ref_thr), (what, mode, fb, "cpu")
    thr = th.resolve()
    pred, stats = cl.classify(dev(score), dev(seg), thr, dev(label))
    rp, rc = R.classify(score, seg, thr.cpu().numpy(), n_seg, label)
    assert same(pred.cpu().numpy().astype(U8), rp), what
    assert same(stats["confusion"].numpy(), rc), what
    check_accuracies(stats, rc, len(score))
    # thr_lo reproduces the cut: the decisions it makes on the fitted scores are right best_correct times, per relation
    # (the midpoint does too unless the first rejected score is itself +inf, where "mid" is +inf by definition)
    _, lo_stats = cl.classify(dev(score), dev(seg), th.resolve("lo", "none"), dev(label))
    lo_conf = lo_stats["confusion"].numpy()
    assert np.array_equal(lo_conf[:, 0] + lo_conf[:, 2], per["best_correct"]), what


def sizes():
    t = C().FIT_TILE
    return [1, 63, 64, 65, t - 1, t, t + 1, 3 * t + 17, 200003]


SEG_KINDS = ("1", "2", "7", "1345", "M", "4M")


@pytest.mark.parametrize("skind", SCORES)
@pytest.mark.parametrize("seg_kind", SEG_KINDS)
@pytest.mark.parametrize("m_index", range(9))
def test_fit_and_classify_equal_the_reference(m_index, seg_kind, skind):
    """M in {1, 63, 64, 65, T-1, T, T+1, 3T+17, 200003} x n_seg in {1, 2, 7, 1345, M, 4M} x every score kind; every label
    kind below 10^5 elements, one label kind at 200003 (rotating, so that each meets every score kind and n_seg there)."""
    M = sizes()[m_index]
    n_seg = {"M": M, "4M": 4 * M}.get(seg_kind) or int(seg_kind)
    rng = np.random.default_rng(1000 * m_index + 10 * SEG_KINDS.index(seg_kind) + SCORES.index(skind))
    seg = make_segments(M, n_seg, rng)
    lkinds = LABELS if M < 100000 else (LABELS[(SCORES.index(skind) + SEG_KINDS.index(seg_kind)) % len(LABELS)],)
    for lkind in lkinds:
        score = make_scores(skind, M, rng)
        label = make_labels(lkind, score, rng)
        what = (M, n_seg, skind, lkind)
        check_fit_raw(*sorted_case(score, seg, label, skind), n_seg, what)
        if skind != "tie_runs":                         # (tie_runs edits the sorted arrays: it is a kernel-level case)
            check_public_path(score, seg, label, n_seg, what)


@pytest.mark.parametrize("lkind", LABELS)
def test_segment_boundary_on_a_tile_boundary(lkind):
    """Segments that end exactly where a tile ends, one that spans two whole tiles, and a tie run across each seam."""
    t = T()
    seg = np.concatenate([np.zeros(t, I32), np.full(2 * t, 1, I32), np.full(t, 3, I32), np.full(17, 4, I32)])
    rng = np.random.default_rng(5)
    for skind in SCORES:
        score = make_scores(skind, len(seg), rng)
        label = make_labels(lkind, score, rng)
        check_fit_raw(*sorted_case(score, seg, label, skind), 6, (skind, lkind))


@pytest.mark.parametrize("large", [False, True])
def test_one_segment_of_ninety_percent_beside_singletons(large):
    M = 200003 if large else 3 * T() + 17
    rng = np.random.default_rng(M)
    n_big = int(0.9 * M)
    n_seg = M - n_big + 1
    seg = np.concatenate([np.full(n_big, 3, I32), np.setdiff1d(np.arange(n_seg), [3]).astype(I32)])
    seg = seg[rng.permutation(M)]
    for skind, lkind in zip(SCORES, LABELS + ("random",)):
        score = make_scores(skind, M, rng)
        label = make_labels(lkind, score, rng)
        check_fit_raw(*sorted_case(score, seg, label, skind), n_seg, (skind, lkind))
        if skind != "tie_runs":
            check_public_path(score, seg, label, n_seg, (skind, lkind))


def test_segments_out_of_range_are_ignored_by_the_fit():
    rng = np.random.default_rng(9)
    M, n_seg = 5000, 7
    seg = rng.integers(-2, n_seg + 2, M).astype(I32)
    score = make_scores("nan_tail", M, rng)
    label = make_labels("random", score, rng)
    check_fit_raw(*sorted_case(score, seg, label, "nan_tail"), n_seg, "out of range")


def test_unsorted_input_returns_zero():
    """Random input that is NOT ordered: the numbers mean nothing, the call succeeds (no access out of bounds: the ABI
    guard file runs the same on guard-banded buffers)."""
    rng = np.random.default_rng(11)
    M, n_seg = 3 * T() + 17, 1345
    out = gpu_fit_raw(rng.standard_normal(M).astype(F32), rng.integers(-3, n_seg + 3, M).astype(I32),
                      rng.integers(0, 2, M).astype(U8), n_seg)
    torch.cuda.synchronize()
    assert all(len(out[k]) == n_seg for k in FIELDS)


def test_classify_unsorted_with_bad_segments_nans_and_no_labels():
    from graphembeddings_amd import _lib
    from graphembeddings_amd.hole import _stream
    rng = np.random.default_rng(13)
    M, n_seg = 70001, 1345
    seg = rng.integers(-5, n_seg + 5, M).astype(I32)
    seg[:4000] = 17                                     # whole waves of one segment beside mixed ones
    score = make_scores("nan_tail", M, rng)
    thr = rng.standard_normal(n_seg).astype(F32)
    thr[::50], thr[1::50], thr[2::50] = np.nan, np.inf, -np.inf
    label = rng.integers(0, 2, M).astype(U8)
    s, g, t, l = dev(score), dev(seg), dev(thr), dev(label)
    pred = torch.full((M,), 7, dtype=torch.uint8, device="cuda")
    conf = torch.full((n_seg, 4), -1, dtype=torch.int32, device="cuda")
    _lib.call("ge_threshold_classify", s.data_ptr(), g.data_ptr(), None, M, n_seg, t.data_ptr(), pred.data_ptr(), None, _stream())
    rp, _ = R.classify(score, seg, thr, n_seg)
    assert same(pred.cpu().numpy(), rp)
    pred.fill_(7)
    _lib.call("ge_threshold_classify", s.data_ptr(), g.data_ptr(), l.data_ptr(), M, n_seg, t.data_ptr(), pred.data_ptr(),
              conf.data_ptr(), _stream())
    rp, rc = R.classify(score, seg, thr, n_seg, label)
    assert same(pred.cpu().numpy(), rp) and same(conf.cpu().numpy(), rc)
    assert _lib.load().ge_threshold_classify(s.data_ptr(), g.data_ptr(), None, M, n_seg, t.data_ptr(), pred.data_ptr(),
                                             conf.data_ptr(), _stream()) == _lib.GE_EINVAL


@pytest.mark.parametrize("over", [0, 1])
def test_confusion_on_both_sides_of_the_lds_limit(over):
    """n_seg at and one past the largest table ge_threshold_classify counts in LDS, on unordered input in which one
    segment holds half of the elements, the last segment is used, and M is not a multiple of any chunk."""
    cl = C()
    n_seg = cl.CONFUSION_LDS_SEGMENTS + over
    rng = np.random.default_rng(19 + over)
    M = 3 * 8192 + 777
    seg = np.where(rng.random(M) < 0.5, 5, rng.integers(-3, n_seg + 3, M)).astype(I32)
    seg[-1], seg[0] = n_seg - 1, 0
    score = make_scores("nan_tail", M, rng)
    thr = rng.standard_normal(n_seg).astype(F32)
    label = rng.integers(0, 2, M).astype(U8)
    from graphembeddings_amd import _lib
    from graphembeddings_amd.hole import _stream
    s, g, t, l = dev(score), dev(seg), dev(thr), dev(label)
    pred = torch.full((M,), 7, dtype=torch.uint8, device="cuda")
    conf = torch.full((n_seg, 4), -1, dtype=torch.int32, device="cuda")
    _lib.call("ge_threshold_classify", s.data_ptr(), g.data_ptr(), l.data_ptr(), M, n_seg, t.data_ptr(), pred.data_ptr(),
              conf.data_ptr(), _stream())
    rp, rc = R.classify(score, seg, thr, n_seg, label)
    assert same(pred.cpu().numpy(), rp) and same(conf.cpu().numpy(), rc)


def test_two_runs_agree_bitwise():
    rng = np.random.default_rng(17)
    M, n_seg = 200003, 1345
    seg = make_segments(M, n_seg, rng)
    score = make_scores("four_values", M, rng)
    label = make_labels("random", score, rng)
    s, g, l = sorted_case(score, seg, label, "four_values")
    a, b = gpu_fit_raw(s, g, l, n_seg), gpu_fit_raw(s, g, l, n_seg)
    assert all(same(a[k], b[k]) for k in FIELDS)
    cl = C()
    thr = dev(R.resolve(a, R.fit(score, np.zeros(M, I32), label, 1)))
    p0, s0 = cl.classify(dev(score), dev(seg), thr, dev(label))
    p1, s1 = cl.classify(dev(score), dev(seg), thr, dev(label))
    assert torch.equal(p0, p1) and torch.equal(s0["confusion"], s1["confusion"])


def test_workspace_size_follows_the_tile():
    """FIT_TILE is the kernel's tile: the workspace grows by one tile's counters exactly when M passes a multiple."""
    from graphembeddings_amd import _lib
    f = _lib.load().ge_threshold_fit_workspace_bytes
    t = T()
    assert f(1, 1) == f(t, 1) > 0 and f(64 * t, 1) < f(64 * t + 1, 1) and f(1, 64) < f(1, 65)
    assert f(0, 1) == 0 and f(1, 0) == 0 and f(2 ** 31, 1) == 0 and f(2 ** 31 - 1, 1) > 0


# ------------------------------------------------------------------------------------ end to end on small tables
E_, R_ = 300, 5


@pytest.fixture(scope="module")
def kg():
    tri = XR.planted_kg(n_ent=E_, n_rel=R_, n_triples=3000, seed=1)
    n = len(tri)
    return {"train": tri[:int(0.8 * n)], "valid": tri[int(0.8 * n):int(0.9 * n)], "test": tri[int(0.9 * n):], "all": tri}


def translation_model(name):
    if name == "transr":
        from graphembeddings_amd import transr as TR
        return TR.TransR(E_, R_, 16, 8, seed=2)
    from graphembeddings_amd import transx as X
    return X.TransX(name, E_, R_, 16, seed=2)


def reference_result(score_fn, vtri, vlab, ttri, tlab, n_rel, mode="mid"):
    """classify_ref on the scores the model's own score call returns."""
    vs, ts = score_fn(vtri), score_fn(ttri)
    per, glob = R.fit(vs, vtri[:, 2], vlab, n_rel), R.fit(vs, np.zeros(len(vs), I32), vlab, 1)
    thr = R.resolve(per, glob, mode)
    pred, conf = R.classify(ts, ttri[:, 2], thr, n_rel, tlab)
    return per, glob, thr, conf


def check_against_reference(res, score_fn, vpos, tpos, n_rel, rel_offset=0):
    vneg, tneg = res["valid_neg"].cpu().numpy(), res["test_neg"].cpu().numpy()
    vtri, ttri = np.concatenate([vpos, vneg]).astype(I32), np.concatenate([tpos, tneg]).astype(I32)
    vlab = np.concatenate([np.ones(len(vpos), U8), np.zeros(len(vneg), U8)])
    tlab = np.concatenate([np.ones(len(tpos), U8), np.zeros(len(tneg), U8)])
    per, glob, thr, conf = reference_result(score_fn, vtri, vlab, ttri, tlab, n_rel)
    th = res["thresholds"]
    for k in FIELDS:
        assert same(getattr(th, k).cpu().numpy(), per[k]), k
        assert same(getattr(th, "global_" + k).cpu().numpy(), glob[k]), k
    assert same(res["thr"].cpu().numpy(), thr)
    assert same(res["confusion"].numpy(), conf)
    check_accuracies(res, conf, len(ttri))
    assert res["n_valid"] == len(vtri)


@pytest.mark.parametrize("name", ["transe", "transh", "transd", "transr"])
def test_translation_models_end_to_end(kg, name):
    from graphembeddings_amd import hole as H
    cl = C()
    m = translation_model(name)
    m.trainer(kg["train"], 256, seed=1).run(50)
    res = m.triple_classification(kg["valid"], kg["test"], known=kg["all"], seed=5)
    sampler = H.BernoulliSampler(kg["all"], R_, E_, ent_lo=0)
    for split, step in (("valid", cl.VALID_STEP), ("test", cl.TEST_STEP)):
        want = sampler.corrupt(dev(kg[split].astype(I32)), seed=5, step=step)
        assert torch.equal(res[split + "_neg"], want)
    assert cl.VALID_STEP != cl.TEST_STEP
    assert res["dropped_valid_neg"] == 0 and res["dropped_test_neg"] == 0
    score = lambda tri: m.score(dev(tri)).cpu().numpy()
    check_against_reference(res, score, kg["valid"], kg["test"], R_)
    # negatives handed in are used as they are
    again = m.triple_classification(kg["valid"], kg["test"], res["valid_neg"], res["test_neg"])
    assert again["accuracy"] == res["accuracy"] and same(again["thr"].cpu().numpy(), res["thr"].cpu().numpy())


def shared_table_kg(kg):
    """The planted KG in the shared-table layout: relations are rows [0, R), entity e is row R + e, four types."""
    sh = {k: np.stack([v[:, 0] + R_, v[:, 1] + R_, v[:, 2]], 1) for k, v in kg.items()}
    N = R_ + E_
    id_to_type = np.full(N, -1, I32)
    ent = np.arange(R_, N)
    id_to_type[ent] = ent % 4
    lists = [ent[ent % 4 == t] for t in range(4)]
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return sh, N, (id_to_type, offsets, np.concatenate(lists).astype(I32))


@pytest.mark.parametrize("name", ["complex", "hole", "hole_spectral"])
def test_shared_table_models_end_to_end(kg, name):
    from graphembeddings_amd import hole as H
    cl = C()
    sh, N, types = shared_table_kg(kg)
    tt = H.TypeTables.from_host(*types, padded_size=64)
    emb = H.init_embeddings(N, 32, seed=3)
    emb.mul_(8.0)                                       # rows outside the unit ball: the clip is part of the score
    res = cl.triple_classification((emb, R_, tt, name), sh["valid"], sh["test"], known=sh["all"], seed=7)
    known = {tuple(t) for t in sh["all"].tolist()}
    for split, step in (("valid", cl.VALID_STEP), ("test", cl.TEST_STEP)):
        drawn = H.corrupt_batch(tt, R_, dev(sh[split].astype(I32)), seed=7, step=step, mode=H.CORRUPT_ROW_COIN).cpu().numpy()
        keep = np.array([tuple(t) not in known and min(t) >= 0 for t in drawn.tolist()])
        assert np.array_equal(res[split + "_neg"].cpu().numpy(), drawn[keep])
        assert res[f"dropped_{split}_neg"] == int((~keep).sum())
    score = lambda tri: H.evaluate_triples(dev(tri), emb, model=name).view(-1).cpu().numpy()
    check_against_reference(res, score, sh["valid"], sh["test"], R_)


def test_value_errors_on_device_input():
    cl = C()
    s, r, l = dev(np.array([0.1, 0.2], F32)), dev(np.array([0, 1], I32)), dev(np.array([1, 0], U8))
    for bad in ((s, dev(np.array([0, 2], I32)), l), (s, r, dev(np.array([1, 2], U8))),
                (dev(np.array([-np.inf, 0.2], F32)), r, l), (s[:1], r, l), (s.double(), r, l)):
        with pytest.raises(ValueError):
            cl.fit_thresholds(*bad, 2)
    m = translation_model("transe")
    with pytest.raises(ValueError):
        m.triple_classification(np.array([[0, 1, R_]]), np.array([[0, 1, 0]]), known=np.array([[0, 1, 0]]))
    with pytest.raises(ValueError):
        m.triple_classification(np.array([[0, 1, 0]]), np.array([[0, 1, 0]]))          # no negatives and no known


# ------------------------------------------------------------------------------------ learning
def test_planted_kg_learns_to_classify():
    """The TransE training of test_gpu_transx.py::test_planted_kg_learns; the held-out 10 % split in half into valid and
    test.  Trained test accuracy above the untrained one and above 0.5 + 5 * 0.5 / sqrt(n): five binomial standard
    deviations of a coin over the n labelled test triples."""
    from graphembeddings_amd import transx as X
    tri = XR.planted_kg(seed=0)
    cut = int(0.9 * len(tri))
    train, held = tri[:cut], tri[cut:]
    valid, test = held[:len(held) // 2], held[len(held) // 2:]
    m = X.TransX("transe", 2000, 20, 32, l1=True, seed=0)
    run = lambda: m.triple_classification(valid, test, known=tri, seed=1)
    before = run()
    m.trainer(train, len(train) // 20, margin=1.0, learning_rate=0.01, seed=3).run(3000)
    after = run()
    n = after["n"]
    floor = 0.5 + 5 * 0.5 / np.sqrt(n)
    print(f"planted KG triple classification on {n} labelled test triples: untrained accuracy {before['accuracy']:.4f}, "
          f"trained {after['accuracy']:.4f} (macro {after['macro_accuracy']:.4f}); floor {floor:.4f}")
    assert n == 2 * len(test)
    assert after["accuracy"] > before["accuracy"] and after["accuracy"] > floor


# ------------------------------------------------------------------------------------ drivers
def _write(path, rows, count=None):
    with open(path, "w") as f:
        f.write(f"{len(rows) if count is None else count}\n")
        for r in rows:
            f.write(" ".join(str(int(x)) for x in r) + "\n")


def test_transx_driver_classifies(tmp_path, kg, capsys):
    from graphembeddings_amd import transx as X
    from graphembeddings_amd import transx_train as D
    cl = C()
    d = tmp_path / "data"
    d.mkdir()
    _write(str(d / "entity2id.txt"), [], E_)
    _write(str(d / "relation2id.txt"), [], R_)
    _write(str(d / "triple2id.txt"), kg["train"])
    _write(str(d / "test2id.txt"), kg["test"])
    _write(str(d / "valid2id.txt"), kg["valid"])
    out = tmp_path / "a"
    assert D.main(["--data_dir", str(d), "--nbatches", "5", "--output_dir", str(out), "--train_times", "2", "--model",
                   "transe", "--hidden_size", "16", "--test_file", str(d / "test2id.txt"), "--valid_file",
                   str(d / "valid2id.txt"), "--classify", "--classify_seed", "4"]) == 0
    assert "triple classification: accuracy" in capsys.readouterr().out
    rep = json.load(open(out / "transe_classify.json"))
    m = X.TransX("transe", E_, R_, 16)
    m.load_state_dict(torch.load(out / "transe.pt", map_location="cpu"))
    res = m.triple_classification(kg["valid"], kg["test"], known=np.concatenate([kg["train"], kg["valid"], kg["test"]]), seed=4)
    assert rep["accuracy"] == res["accuracy"] and rep["macro_accuracy"] == res["macro_accuracy"]
    assert rep["confusion"] == res["confusion"].tolist() and rep["n"] == res["n"]
    th, thr = cl.load_thresholds(str(out / "transe_thresholds.tsv"))
    assert same(thr.numpy(), res["thr"].cpu().numpy())
    for k in FIELDS:
        assert same(getattr(th, k).numpy(), getattr(res["thresholds"], k).cpu().numpy())
        assert same(getattr(th, "global_" + k).numpy(), getattr(res["thresholds"], "global_" + k).cpu().numpy())
    assert same(th.resolve().numpy(), thr.numpy())
    th.save(str(tmp_path / "again.tsv"))
    assert open(tmp_path / "again.tsv").read() == open(out / "transe_thresholds.tsv").read()
