"""Triple classification without a GPU: the numpy reference against hand-worked cases (and its vectorised fit against
its plain loop), Thresholds.resolve on CPU tensors, the host-side ValueErrors, the thresholds TSV and the drivers'
argument checks."""
import numpy as np
import pytest
import torch

import test_abi_workspace_host as W
from tests import classify_ref as R

# The size function of the fit joins the table test_abi_workspace_host.py checks (its
# test_every_size_function_is_listed reads CASES when it runs, after every module is collected): 0 for bad sizes,
# non-decreasing in M and n_seg across the fit's tile (2048) and the sizes of the other kernels, a multiple of 256.
W.CASES["ge_threshold_fit_workspace_bytes"] = (
    [sorted(W.SIZES + [2047, 2048, 2049, 6161, 2 ** 31 - 1]), sorted(W.SIZES + [1345, 2 ** 31 - 1])],
    [(0, 1), (-1, 1), (1, 0), (1, -1), (2 ** 31, 1)], True)

F32, I32 = np.float32, np.int32
INF = float("inf")


def C():
    from graphembeddings_amd import classify
    return classify


def seg_fit(score, label):
    lo, hi, best, n_pos, n_neg = R.fit_segment(np.asarray(score, F32), np.asarray(label))
    return float(lo), float(hi), best, n_pos, n_neg


# ------------------------------------------------------------------------------------ the reference, by hand
def test_reference_hand_worked_segments():
    # perfectly separable: accept the two positives
    assert seg_fit([0.1, 0.2, 0.7, 0.9], [1, 1, 0, 0]) == (F32(0.2), F32(0.7), 4, 2, 2)
    # one mistake either way: cuts 1 and 3 both get 3 right, the smaller cut wins
    assert seg_fit([0.1, 0.2, 0.3, 0.4], [1, 0, 1, 0]) == (F32(0.1), F32(0.2), 3, 2, 2)
    # p = 0: every positive sits above every negative, accepting nothing gets the 2 negatives right, as does accepting all
    # get the 2 positives right -- the tie goes to the smaller cut
    assert seg_fit([0.1, 0.2, 0.3, 0.4], [0, 0, 1, 1]) == (-INF, F32(0.1), 2, 2, 2)
    # p = m: all positive
    assert seg_fit([0.1, 0.2, 0.3], [1, 1, 1]) == (F32(0.3), INF, 3, 3, 0)
    # all negative
    assert seg_fit([0.1, 0.2, 0.3], [0, 0, 0]) == (-INF, F32(0.1), 3, 0, 3)
    # empty
    assert seg_fit([], []) == (-INF, INF, 0, 0, 0)
    # one element
    assert seg_fit([0.5], [1]) == (F32(0.5), INF, 1, 1, 0)
    assert seg_fit([0.5], [0]) == (-INF, F32(0.5), 1, 0, 1)


def test_reference_never_separates_equal_scores():
    # the only cuts are 0, 3 (after the run of 0.2) and 4: cut 3 gets pos 2 + neg 1 = 3 right, cut 0 gets 2, cut 4 gets 2
    assert seg_fit([0.2, 0.2, 0.2, 0.5], [1, 0, 1, 0]) == (F32(0.2), F32(0.5), 3, 2, 2)
    # all equal: accept all (2 positives) or nothing (1 negative)
    assert seg_fit([0.3, 0.3, 0.3], [1, 0, 1]) == (F32(0.3), INF, 2, 2, 1)
    assert seg_fit([0.3, 0.3, 0.3], [0, 1, 0]) == (-INF, F32(0.3), 2, 1, 2)
    # +inf is a score like any other; two of them are a tie
    assert seg_fit([0.1, INF, INF], [1, 1, 0]) == (F32(0.1), INF, 2, 2, 1)
    assert seg_fit([0.1, INF, INF], [1, 1, 1]) == (INF, INF, 3, 3, 0)


def test_reference_nan_tail_is_rejected_at_every_cut():
    nan = float("nan")
    # m_v = 2: the NaN positive can never be accepted; cut 2 = m_v has thr_hi = +inf
    assert seg_fit([0.1, 0.2, nan], [1, 1, 1]) == (F32(0.2), INF, 2, 3, 0)
    # a NaN negative counts as correct at every cut
    assert seg_fit([0.1, 0.2, nan, nan], [1, 0, 0, 0]) == (F32(0.1), F32(0.2), 4, 1, 3)
    # nothing but NaN: p = 0 = m_v
    assert seg_fit([nan, nan], [1, 0]) == (-INF, INF, 1, 1, 1)


def test_vectorised_fit_equals_the_plain_loop():
    rng = np.random.default_rng(0)
    for trial in range(200):
        M, n_seg = int(rng.integers(1, 80)), int(rng.integers(1, 9))
        seg = rng.integers(-1, n_seg + 1, M)
        score = (rng.choice(np.array([0.1, 0.2, 0.3, np.inf, np.nan, 0.5]), M) if trial % 2
                 else rng.standard_normal(M)).astype(F32)
        label = rng.integers(0, 2, M).astype(np.uint8)
        a, b = R.fit(score, seg, label, n_seg), R.fit_by_segment(score, seg, label, n_seg)
        for k in a:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(I32), b[k].view(I32)), (trial, k)


def test_reference_classify_and_accuracies():
    nan = float("nan")
    score = np.array([0.1, 0.5, 0.5, nan, 0.2, 0.9], F32)
    seg = np.array([0, 0, 1, 1, 2, -1])
    thr = np.array([0.3, 0.5], F32)
    label = np.array([1, 1, 0, 1, 1, 1])
    pred, conf = R.classify(score, seg, thr, 2, label)
    assert pred.tolist() == [1, 0, 1, 0, 0, 0]          # a NaN and a segment out of range are never accepted
    assert conf.tolist() == [[1, 0, 0, 1], [0, 1, 0, 1]]
    assert R.accuracies(conf) == (0.25, 0.25)
    assert R.classify(score, seg, thr, 2)[1] is None


# ------------------------------------------------------------------------------------ resolve
def thresholds(lo, hi, n_pos, n_neg, g=(0.25, 0.5)):
    t = lambda x, dt: torch.tensor(x, dtype=dt)
    n = len(lo)
    return C().Thresholds(t(lo, torch.float32), t(hi, torch.float32), t([0] * n, torch.int32), t(n_pos, torch.int32),
                          t(n_neg, torch.int32), t([g[0]], torch.float32), t([g[1]], torch.float32),
                          t([0], torch.int32), t([1], torch.int32), t([1], torch.int32))


def test_resolve_midpoint_infinite_ends_and_fallbacks():
    a = np.float32(0.3)
    b = np.nextafter(a, np.float32(1), dtype=np.float32)                 # adjacent floats: the midpoint rounds to one of them
    th = thresholds([0.5, float(a), -INF, 1.0, -INF, 0.5, 0.5], [1.0, float(b), 0.2, INF, INF, 0.75, 0.75],
                    [1, 1, 1, 1, 1, 0, 3], [1, 1, 1, 1, 1, 2, 0])
    mid = th.resolve("mid", "none").numpy()
    assert mid.dtype == F32 and mid[0] == F32(0.75)
    assert a <= mid[1] < b and mid[1] == a               # never >= hi: the cut stays where the fit put it
    assert mid[2] == -INF and mid[3] == INF and mid[4] == -INF
    assert mid[5] == mid[6] == F32(0.625)
    assert th.resolve("lo", "none").numpy().tolist() == [0.5, float(a), -INF, 1.0, -INF, 0.5, 0.5]
    g = th.resolve("mid", "global").numpy()
    assert g[5] == g[6] == F32(0.375) and np.array_equal(g[:5], mid[:5])  # no positives / no negatives: the global one
    assert th.resolve("lo", "global").numpy()[5] == F32(0.25)
    assert th.uses_global().tolist() == [False] * 5 + [True, True] and not th.uses_global("none").any()
    for bad in (("up", "global"), ("mid", "nearest")):
        with pytest.raises(ValueError):
            th.resolve(*bad)
    # the reference's resolve is the same function
    per = {"thr_lo": th.thr_lo.numpy(), "thr_hi": th.thr_hi.numpy(), "n_pos": th.n_pos.numpy(), "n_neg": th.n_neg.numpy()}
    glob = {"thr_lo": th.global_thr_lo.numpy(), "thr_hi": th.global_thr_hi.numpy()}
    for mode in ("mid", "lo"):
        for fb in ("global", "none"):
            assert np.array_equal(R.resolve(per, glob, mode, fb).view(I32), th.resolve(mode, fb).numpy().view(I32))


def test_resolve_midpoint_is_rounded_once_from_float64():
    lo, hi = np.float32(1.0), np.float32(1.0 + 3 * 2.0 ** -23)
    th = thresholds([float(lo)], [float(hi)], [1], [1])
    want = np.float32(0.5 * (np.float64(lo) + np.float64(hi)))           # 1 + 1.5 ulp -> ties-to-even: 1 + 2 ulp
    assert th.resolve().numpy()[0] == want == np.float32(1.0 + 2 * 2.0 ** -23)


# ------------------------------------------------------------------------------------ TSV
def test_thresholds_tsv_round_trip(tmp_path):
    cl = C()
    a = np.float32(0.1)
    th = thresholds([float(a), -INF, 1.0000001, 0.5], [float(np.nextafter(a, np.float32(1))), 0.2, INF, 0.75],
                    [4, 0, 2, 1], [3, 2, 0, 1], g=(0.30000001, 0.4))
    th.best_correct[:] = torch.tensor([7, 2, 2, 2], dtype=torch.int32)
    path = str(tmp_path / "thr.tsv")
    th.save(path)
    lines = open(path).read().splitlines()
    assert lines[0].split("\t") == list(cl.TSV_HEADER) and len(lines) == 6 and lines[-1].startswith("global\t")
    assert [l.split("\t")[-1] for l in lines[1:]] == ["own", "global", "global", "own", "global"]
    back, thr = cl.load_thresholds(path)
    for k, v in th.__dict__.items():
        assert getattr(back, k).dtype == v.dtype and torch.equal(getattr(back, k), v), k
    assert torch.equal(thr, th.resolve()) and torch.equal(back.resolve(), thr)
    back.save(str(tmp_path / "again.tsv"))
    assert open(tmp_path / "again.tsv").read() == open(path).read()
    (tmp_path / "bad.tsv").write_text("relation\tthr\n0\t1\n")
    with pytest.raises(ValueError):
        cl.load_thresholds(str(tmp_path / "bad.tsv"))


# ------------------------------------------------------------------------------------ errors before any GPU call
def test_product_path_needs_device_tensors():
    cl = C()
    s, r, l = torch.tensor([0.1, 0.2]), torch.tensor([0, 1], dtype=torch.int32), torch.tensor([1, 0], dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA"):
        cl.fit_thresholds(s, r, l, 2)
    with pytest.raises(RuntimeError, match="CUDA"):
        cl.classify(s, r, torch.tensor([0.5, 0.5]), l)


def test_model_and_triple_value_errors():
    cl = C()
    emb = torch.zeros(10, 4)
    with pytest.raises(ValueError):
        cl._as_model(object())
    with pytest.raises(ValueError):
        cl._as_model((emb, 3, None))                    # not the 4-tuple
    with pytest.raises(ValueError):
        cl._as_model(cl.TableModel(emb.cuda() if torch.cuda.is_available() else emb, 3, None, "transe"))
    tm = cl.TableModel(emb, 3, None, "complex")         # (the id checks run on the host, before the table is looked at)
    for bad in (np.array([[3, 4, 3]]), np.array([[2, 4, 0]]), np.array([[3, 10, 0]]), np.array([[3, 4]]),
                np.array([[3.0, 4.0, 0.0]])):
        with pytest.raises(ValueError):
            cl._triples_of(bad, "valid_pos", tm, "cpu")
    assert cl._triples_of(np.array([[3, 9, 2]]), "valid_pos", tm, "cpu").dtype == torch.int32

    class M:
        n_ent, n_rel = 5, 2
    for bad in (np.array([[0, 5, 0]]), np.array([[0, 1, 2]]), np.array([[-1, 1, 0]])):
        with pytest.raises(ValueError):
            cl._triples_of(bad, "test_pos", M(), "cpu")
    with pytest.raises(ValueError):
        cl.draw_negatives(M(), torch.zeros(1, 3, dtype=torch.int32), None, 0, 0)


def test_fit_workspace_size_function():
    W.test_size_function("ge_threshold_fit_workspace_bytes")


def test_library_version_and_symbols():
    from graphembeddings_amd import _lib
    lib = _lib.load()
    assert lib.ge_version() >= 400
    f = lib.ge_threshold_fit_workspace_bytes
    t = C().FIT_TILE
    assert f(1, 1) == f(t, 1) > 0 and f(64 * t, 1) < f(64 * t + 1, 1)   # FIT_TILE is the kernel's tile
    sizes = [f(m, n) for m in (1, t, t + 1, 10 ** 6, 2 ** 31 - 1) for n in (1, 64, 65, 10 ** 6)]
    assert all(f(m, n) <= f(m + 1, n) and f(m, n) <= f(m, n + 1) for m in (1, t - 1, t, 12345) for n in (1, 63, 64, 4000))
    assert min(sizes) > 0 and all(s % 256 == 0 for s in sizes)
    assert f(0, 1) == 0 and f(1, 0) == 0 and f(2 ** 31, 1) == 0
    # argument checks that launch nothing
    assert lib.ge_threshold_fit(None, None, None, 1, 1, None, None, None, None, None, None, 0, None) == _lib.GE_EINVAL
    assert lib.ge_threshold_classify(None, None, None, 1, 1, None, None, None, None) == _lib.GE_EINVAL


# ------------------------------------------------------------------------------------ drivers' argument checks
def test_translation_drivers_check_the_classify_flags(tmp_path):
    from graphembeddings_amd import transr_train, transx_train
    f = tmp_path / "x.txt"
    f.write_text("1\n0 1 0\n")
    for mod in (transx_train, transr_train):
        ok = mod.build_parser().parse_args(["--classify", "--test_file", str(f), "--valid_file", str(f), "--valid_neg_file",
                                            str(f), "--test_neg_file", str(f), "--classify_seed", "3"])
        mod.check_args(ok)
        assert ok.classify and ok.classify_seed == 3
        for argv in (["--classify"], ["--classify", "--test_file", str(f)], ["--classify", "--valid_file", str(f)],
                     ["--valid_file", str(f)], ["--test_file", str(f), "--valid_neg_file", str(f)],
                     ["--classify", "--test_file", str(f), "--valid_file", str(tmp_path / "missing.txt")],
                     ["--classify", "--test_file", str(f), "--valid_file", str(f), "--test_neg_file", str(tmp_path / "no.txt")],
                     ["--classify", "--test_file", str(f), "--valid_file", str(f), "--classify_seed", "-1"]):
            with pytest.raises(ValueError):
                mod.check_args(mod.build_parser().parse_args(argv))
        mod.check_args(mod.build_parser().parse_args([]))                # nothing asked: nothing to check


def test_train_driver_checks_the_classify_flags():
    from graphembeddings_amd import train as T
    base = ["--data_dir", "d", "--output_dir", "o"]
    parse = lambda extra: T.build_parser().parse_args(base + extra)
    T.check_classify_flags(parse([]))
    T.check_classify_flags(parse(["--infer", "--classify", "--classify_seed", "2"]))
    for extra, world in ((["--classify"], 1), (["--infer", "--classify", "--gpus", "2"], 1), (["--infer", "--classify"], 2),
                         (["--infer", "--classify", "--classify_seed", "-1"], 1)):
        with pytest.raises(SystemExit):
            T.check_classify_flags(parse(extra), world)
    with pytest.raises(SystemExit):
        T.main(base + ["--classify"])
