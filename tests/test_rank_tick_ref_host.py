"""Host: tests/rank_tick_ref.py -- the fp64 restatement of ge_rank_metrics and of the pocket rule -- against
evaluate.mrr_and_hits on the counted rows, and train.ticks_since_best (what --softmax_patience compares against) on
hand-made histories."""
import math

import numpy as np
import pytest

from graphembeddings_amd import evaluate as EV
from graphembeddings_amd import train as T
from tests import rank_tick_ref as RT

NAN = float("nan")


def counts(M, seed):
    rng = np.random.default_rng(seed)
    nb = rng.integers(0, 50, M).astype(np.int32)
    nk = np.minimum(rng.integers(0, 8, M), nb).astype(np.int32)
    return nb, nk


@pytest.mark.parametrize("M", [1, 2, 65, 1000])
def test_metrics_equal_mrr_and_hits_on_counted_rows(M):
    nb, nk = counts(M, M)
    tl = np.full(M, 0.25, np.float32)
    for bad_tl, bad_k in (((), ()), ((0,), ()), ((M - 1,), (M // 2,)), ((M // 2,), (0, M - 1))):
        nb2, nk2, tl2 = nb.copy(), nk.copy(), tl.copy()
        for i in bad_tl:
            nb2[i], nk2[i], tl2[i] = 0, 0, NAN
        for i in bad_k:
            nk2[i] = nb2[i] + 1 if i % 2 else -1
        ok = RT.counted_rows(nb2, nk2, tl2)
        bad = set(bad_tl) | set(bad_k)
        assert ok.sum() == M - len(bad) and not ok[sorted(bad)].any()
        m = RT.as_dict(RT.rank_metrics(nb2, nk2, tl2))
        if not ok.any():
            assert m["counted"] == 0 and all(math.isnan(m[k]) for k in RT.KEYS[:7])
            continue
        raw, fil = RT.ranks(nb2, nk2, tl2)
        assert np.array_equal(raw, 1 + nb2[ok].astype(np.int64)) and np.array_equal(fil, raw - nk2[ok])
        want = EV.mrr_and_hits(raw, fil)
        assert set(want) | {"counted"} == set(RT.KEYS) == set(EV.RankPocket.KEYS)
        assert RT.KEYS == EV.RankPocket.KEYS
        for k, v in want.items():
            assert m[k] == pytest.approx(v, rel=1e-14, abs=0), k
        assert m["counted"] == ok.sum()
    # without true losses only the counts decide
    assert RT.rank_metrics(nb, nk)[7] == M
    assert np.array_equal(RT.rank_metrics(nb, nk, None), RT.rank_metrics(nb, nk, tl), equal_nan=True)


def test_planted_ranks():
    nb = np.array([0, 5, 5, 5, 12, 12], np.int32)
    nk = np.array([0, 4, 3, 2, 3, 2], np.int32)             # filtered ranks 1, 2, 3, 4, 10, 11
    m = RT.as_dict(RT.rank_metrics(nb, nk))
    assert m["hits1"] == 100.0 / 6 and m["hits3"] == 50.0 and m["hits10"] == 500.0 / 6
    assert m["mean_filtered_pos"] == 31 / 6 and m["mean_raw_pos"] == (1 + 6 * 3 + 13 * 2) / 6
    assert m["filtered_mrr"] == pytest.approx((1 + 1 / 2 + 1 / 3 + 1 / 4 + 1 / 10 + 1 / 11) / 6, rel=1e-15)
    assert np.isnan(RT.rank_metrics(nb, nk, np.full(6, NAN))[:7]).all()


def test_pocket_rule():
    bests, imp = RT.pocket([0.2, 0.3, 0.3, 0.1, NAN, 0.4, 0.4])
    assert imp == [True, True, False, False, False, True, False]
    assert bests == [0.2, 0.3, 0.3, 0.3, 0.3, 0.4, 0.4]
    assert RT.pocket([0.0, NAN]) == ([0.0, 0.0], [False, False])          # best starts at 0: a zero is a tie
    assert RT.pocket([0.2, 0.3], best=0.25) == ([0.25, 0.3], [False, True])


def test_ticks_since_best():
    f = T.ticks_since_best
    assert f([]) == 0
    assert f([0.2]) == 0 and f([0.2, 0.3]) == 0
    assert f([0.3, 0.2]) == 1 and f([0.3, 0.2, 0.25]) == 2
    assert f([0.3, 0.3]) == 1 and f([0.3, 0.3, 0.3]) == 2                 # a tie does not reset the count
    assert f([0.3, NAN]) == 1 and f([NAN, NAN]) == 2 and f([0.3, NAN, 0.3]) == 2      # a NaN does not improve
    assert f([0.3, 0.2, 0.31]) == 0 and f([0.3, 0.2, 0.31, 0.31]) == 1
    assert f([0.0]) == 1                                                  # best starts at 0
    assert f([0.2, 0.3], best=0.5) == 2 and f([0.2, 0.6], best=0.5) == 0  # a resumed run starts from the file's best
    # it is the pocket rule replayed: the count since the last improving tick
    rng = np.random.default_rng(0)
    for _ in range(50):
        h = [float(x) if x < 0.9 else NAN for x in np.round(rng.random(12), 1)]
        imp = RT.pocket(h)[1]
        since = len(h) - 1 - max([i for i, b in enumerate(imp) if b], default=-1)
        assert f(h) == since


def test_tick_steps():
    assert T.tick_steps(10, 2) == {5, 10} and T.tick_steps(10, 1) == {10} and T.tick_steps(10, 3) == {4, 7, 10}
    assert T.tick_steps(3, 16) == {1, 2, 3} and T.tick_steps(1, 4) == {1}
    for n in (1, 7, 42, 1000):
        for t in (1, 2, 3, 16, 2000):
            s = T.tick_steps(n, t)
            assert max(s) == n and min(s) >= 1 and len(s) == min(n, t)
