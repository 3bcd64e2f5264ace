"""Pins oracle/transx_oracle.py against the reference's OWN native code: oracle/_ref/init.so is
init.cpp compiled from where it lies in /root/reference (oracle/Makefile, make.sh:1 flags).  The
binary is run in a child process on generated ./data files; every batch must be bit-identical.
What the binary yields on those files is stored in tests/golden/transx_init_batches_v1.npz
(tests/golden/make_transx_golden.py), so the restatement is pinned wherever the binary was not built;
where it was, the binary is run as well and must still yield the stored batches."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import transx_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "init.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "transx_init_batches_v1.npz")
B, K = 64, 5

RUNNER = r"""
import ctypes, os, sys, numpy as np
so, work, B, K = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
os.chdir(work)
lib = ctypes.cdll.LoadLibrary(so)            # transE.py:9-10
lib.init()                                   # transE.py:62
out = []
arrs = [np.zeros(B, dtype=np.int32) for _ in range(6)]
addrs = [a.__array_interface__['data'][0] for a in arrs]   # transE.py:95-107
for _ in range(K):
    lib.getBatch(*[ctypes.c_void_p(x) for x in addrs], B, 0)   # transE.py:112
    out.append(np.stack(arrs).copy())
np.save(os.path.join(work, "batches.npy"), np.stack(out))
print(lib.getEntityTotal(), lib.getRelationTotal(), lib.getTripleTotal())
"""


def _make_kg(seed, E=60, R=5, T=400):
    rng = np.random.default_rng(seed)
    h = rng.integers(0, E, T)
    t = rng.integers(0, E, T)
    r = rng.integers(0, R, T)
    h[:30] = 7                                   # a head with many (r, t) pairs
    t[30:60] = 11
    tri = np.unique(np.stack([h, t, r], 1), axis=0)
    rng.shuffle(tri)
    # leave a few entities (incl. ids 0/1 and some >= 2) out of the head and/or tail role so the
    # memset(sizeof(pointer)) defect of init.cpp:94-95 changes left_mean/right_mean
    tri = tri[(tri[:, 0] != 0) & (tri[:, 1] != 1) & (tri[:, 0] != 20) & (tri[:, 1] != 21)]
    return tri.astype(np.int64), E, R


def run_reference_binary(work, tri, E, R):
    """init.so's first K batches of B on `tri`, [K, 6, B], and its (entity, relation, triple) totals."""
    data = work / "data"
    data.mkdir()
    (data / "relation2id.txt").write_text(f"{R}\n")
    (data / "entity2id.txt").write_text(f"{E}\n")
    with open(data / "triple2id.txt", "w") as f:
        f.write(f"{len(tri)}\n")
        for h, t, r in tri:
            f.write(f"{h} {t} {r}\n")              # init.cpp:70-73 reads h, t, r
    res = subprocess.run([sys.executable, "-c", RUNNER, REF_SO, str(work), str(B), str(K)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    return np.load(work / "batches.npy"), [int(x) for x in res.stdout.split()]


@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_equals_reference_binary(tmp_path, seed):
    tri, E, R = _make_kg(seed)
    g = np.load(GOLDEN)
    assert np.array_equal(g[f"seed{seed}/triples"], tri), "the generated graph is the one the batches were recorded on"
    ref = g[f"seed{seed}/batches"]                 # [K, 6, B]
    assert g[f"seed{seed}/totals"].tolist() == [E, R, len(tri)]
    if os.path.exists(REF_SO):
        got, totals = run_reference_binary(tmp_path, tri, E, R)
        assert totals == [E, R, len(tri)]
        assert np.array_equal(got, ref), "the reference binary no longer yields the stored batches"
    mine = TO.InitCppRestatement(tri, E, R, reproduce_defects=True)
    for k in range(K):
        got = np.stack(mine.getBatch(B))
        assert np.array_equal(got, ref[k]), f"batch {k}"
    # the corruption is filtered: a corrupted triple is never a known one, exactly one side changes
    known = {tuple(x) for x in tri}
    for k in range(K):
        ph, pt, pr, nh, nt, nr = ref[k]
        assert np.array_equal(pr, nr)
        assert ((ph != nh) ^ (pt != nt)).all()
        for b in range(B):
            assert (int(nh[b]), int(nt[b]), int(nr[b])) not in known
    # with the defects fixed the head/tail statistics differ on this graph (documented divergence)
    fixed = TO.InitCppRestatement(tri, E, R, reproduce_defects=False)
    assert not np.allclose(fixed.left_mean, mine.left_mean, equal_nan=True) or \
        not np.allclose(fixed.right_mean, mine.right_mean, equal_nan=True)


def test_parallel_sampler_semantics():
    tri, E, R = _make_kg(3, E=80, R=6, T=900)
    lo = 10                                        # entities live in rows [10, 90) of a shared table
    shifted = tri.copy()
    shifted[:, :2] += lo
    idx = TO.BernoulliIndex(shifted, lo, E, R)
    known = {tuple(x) for x in shifted}
    # fixed statistics equal the textbook tph / hpt
    for r in range(R):
        sub = shifted[shifted[:, 2] == r]
        tph = len(np.unique(sub, axis=0)) / len(np.unique(sub[:, 0]))
        hpt = len(np.unique(sub, axis=0)) / len(np.unique(sub[:, 1]))
        assert idx.tail_threshold[r] == pytest.approx(hpt / (hpt + tph) * 2**32, rel=1e-6)
    pos = shifted[np.random.default_rng(0).integers(0, len(shifted), 2000)].astype(np.int32)
    tails = 0
    for step in range(5):
        neg = TO.bernoulli_corrupt_batch(pos, idx, seed=5, step=step)
        ch = neg != pos
        assert not ch[:, 2].any() and (ch[:, 0] & ch[:, 1]).sum() == 0
        assert (ch.sum(1) == 1).all()              # filtered: the replacement is never the original
        for row in neg:
            assert tuple(int(v) for v in row) not in known
            assert lo <= row[0] < lo + E and lo <= row[1] < lo + E
        tails += ch[:, 1].sum()
    # side frequencies follow hpt/(hpt+tph) on average
    p = idx.tail_threshold[pos[:, 2]].astype(np.float64) / 2**32
    assert abs(tails / (5 * len(pos)) - p.mean()) < 0.03
    # the skip mapping is uniform over the free entities
    h, t, r = (int(v) for v in pos[0])
    same = np.tile(pos[:1], (20000, 1))
    neg = TO.bernoulli_corrupt_batch(same, idx, seed=1, step=0)
    repl = np.where(neg[:, 1] != t, neg[:, 1], neg[:, 0])
    counts = np.bincount(repl - lo, minlength=E)
    assert (counts > 0).sum() >= E - 40
