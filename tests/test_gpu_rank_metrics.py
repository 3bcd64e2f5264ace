"""GPU: ge_rank_metrics on synthetic count vectors against tests/rank_tick_ref.py.

Bounds, both derived (rank_tick_ref.check_metrics).  Entries 2-7 equal float32(reference) exactly: the rank sums and the
hit counts are exact integers and each output is one correctly rounded double division, rounded once to float.  Entries 0
and 1 are within 2^-23 of float32(reference): a double sum of at most 2^24 terms <= 1 errs far below half a float ulp,
so the two can differ only by the final rounding, and an MRR is <= 1.

M in {1, 63, 64, 65, 1023, 1024, 1025, 100000}: one row, the wave (64) and the workgroup (1024) with their neighbours,
and many strides of the one workgroup."""
import numpy as np
import pytest
import torch

from graphembeddings_amd import _lib
from tests import rank_tick_ref as RT

pytestmark = pytest.mark.gpu

I32, F32 = np.int32, np.float32
NAN = float("nan")
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 100000]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def run(nb, nk, tl=None, best=None, poison=0.0):
    """(metrics [8] float32, best after, improved) of one call; best None: no decision is asked for."""
    out = torch.full((8,), poison, dtype=torch.float32, device="cuda")
    b = None if best is None else torch.full((), best, dtype=torch.float32, device="cuda")
    imp = torch.full((), 77, dtype=torch.int32, device="cuda")
    d_nb, d_nk, d_tl = dev(nb), dev(nk), None if tl is None else dev(tl)
    _lib.call("ge_rank_metrics", d_nb.data_ptr(), d_nk.data_ptr(), None if tl is None else d_tl.data_ptr(), len(nb),
              out.data_ptr(), None if b is None else b.data_ptr(), imp.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if b is None else float(b), int(imp)


def vectors(M, seed):
    """Counts with filtered ranks planted at exactly 1, 2, 3, 4, 10 and 11 (cyclically over the first rows), NaN true
    losses at the first, middle and last position, and rows that break n_known_before <= n_before."""
    rng = np.random.default_rng(seed)
    nb = rng.integers(0, 15000, M).astype(I32)
    nk = np.minimum(rng.integers(0, 40, M), nb).astype(I32)
    planted = np.array([1, 2, 3, 4, 10, 11])
    n = min(M, 60)
    fil = planted[np.arange(n) % 6]
    nk[:n] = rng.integers(0, 30, n)
    nb[:n] = fil - 1 + nk[:n]
    tl = rng.random(M).astype(F32)
    return nb, nk, tl


@pytest.mark.parametrize("M", SIZES)
def test_metrics(M):
    nb, nk, tl = vectors(M, M)
    ref = RT.rank_metrics(nb, nk, tl)
    got, _, imp = run(nb, nk, tl)
    RT.check_metrics(got, ref, "M=%d" % M)
    assert got[7] == M and imp == 0                                         # best NULL: no decision, improved = 0
    # without true losses the same rows count
    RT.check_metrics(run(nb, nk)[0], ref, "M=%d no true_loss" % M)
    # two calls agree bitwise, whatever the output held
    again = run(nb, nk, tl, poison=NAN)[0]
    assert np.array_equal(got.view(I32), again.view(I32))
    # NaN true losses at the first, middle and last position (with counts 0, as the sweeps report them): not rank 1
    nb2, nk2, tl2 = nb.copy(), nk.copy(), tl.copy()
    bad = sorted({0, M // 2, M - 1})
    nb2[bad], nk2[bad], tl2[bad] = 0, 0, NAN
    ref2 = RT.rank_metrics(nb2, nk2, tl2)
    got2 = run(nb2, nk2, tl2)[0]
    RT.check_metrics(got2, ref2, "M=%d NaN rows" % M)
    assert got2[7] == M - len(bad)
    # rows that break 0 <= n_known_before <= n_before do not count either
    nk3 = nk2.copy()
    broken = sorted({M // 3, (2 * M) // 3} - set(bad))
    if broken:
        nk3[broken[0]] = nb2[broken[0]] + 1
        nk3[broken[-1]] = -1 if len(broken) > 1 else nk3[broken[-1]]
    ref3 = RT.rank_metrics(nb2, nk3, tl2)
    got3 = run(nb2, nk3, tl2)[0]
    RT.check_metrics(got3, ref3, "M=%d broken rows" % M)
    assert got3[7] == M - len(bad) - len(broken) == ref3[7]


def test_planted_ranks_exactly():
    nb = np.array([0, 5, 5, 5, 12, 12], I32)
    nk = np.array([0, 4, 3, 2, 3, 2], I32)                  # filtered ranks 1, 2, 3, 4, 10, 11
    got = run(nb, nk)[0]
    RT.check_metrics(got, RT.rank_metrics(nb, nk), "planted")
    assert got[4] == F32(100.0 / 6) and got[5] == F32(50.0) and got[6] == F32(500.0 / 6) and got[2] == F32(31 / 6)
    assert got[3] == F32(45 / 6) and got[7] == 6


@pytest.mark.parametrize("M", [1, 65, 1025])
def test_all_nan(M):
    z = np.zeros(M, I32)
    got, best, imp = run(z, z, np.full(M, NAN, F32), best=0.0)
    assert np.isnan(got[:7]).all() and got[7] == 0
    assert imp == 0 and best == 0.0
    got, best, imp = run(z, z, np.full(M, NAN, F32), best=-1.0)             # a NaN never improves, whatever the best
    assert imp == 0 and best == -1.0


def test_pocket_sequence():
    """best / improved over rising, equal, falling and NaN metrics: one device scalar carried through the calls."""
    M = 200
    z = np.zeros(M, I32)
    ok = np.zeros(M, F32)

    def counts(rank):
        return np.full(M, rank - 1, I32)
    seq = [(counts(5), ok), (counts(4), ok), (counts(4), ok), (counts(2), ok), (counts(3), ok), (z, np.full(M, NAN, F32)),
           (counts(2), ok), (counts(1), ok), (counts(1), ok)]
    best = torch.zeros((), dtype=torch.float32, device="cuda")
    imp = torch.zeros((), dtype=torch.int32, device="cuda")
    out = torch.zeros(len(seq), 8, dtype=torch.float32, device="cuda")
    bests, imps = [], []
    for i, (nb, tl) in enumerate(seq):
        d_nb, d_nk, d_tl = dev(nb), dev(z), dev(tl)
        _lib.call("ge_rank_metrics", d_nb.data_ptr(), d_nk.data_ptr(), d_tl.data_ptr(), M, out.data_ptr() + 32 * i,
                  best.data_ptr(), imp.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        bests.append(float(best))
        imps.append(int(imp))
    mrrs = [float(x) for x in out[:, 0].cpu().numpy()]
    want_b, want_i = RT.pocket(mrrs)
    assert imps == [int(b) for b in want_i] == [1, 1, 0, 1, 0, 0, 0, 1, 0]
    assert bests == want_b
    assert mrrs[:5] == [float(F32(1 / 5)), 0.25, 0.25, 0.5, float(F32(1 / 3))] and np.isnan(mrrs[5])
