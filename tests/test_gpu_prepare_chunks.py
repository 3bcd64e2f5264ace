"""The native training loops across prepare-chunk boundaries.  The records of ge_train_max_chunk_steps(B, K) steps are
built per launch into one of two buffers, one chunk ahead on the handle's side stream or, without a handle, on the
caller's stream when a chunk is entered.  Which of the two it is, and where a call starts and stops inside a chunk, must
not reach the results: table, every step's losses and the negatives left in neg_ws are compared bit for bit between one
call with a handle, the same steps in calls of 7 on one handle, and one call without a handle."""
import numpy as np
import pytest
import torch

from graphembeddings_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU: the HIP path cannot be checked")
    from graphembeddings_amd import hole
    return hole


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _small(H):
    """2 relation rows + 64 entities in 4 types of 16, d = 8, B = 8, T = 5 B + 3: a pass is 5 batches (the last 3 rows
    never make a batch), so the batches wrap many times inside a chunk and across its end.  Heads and tails are distinct
    within a batch: an entity row collects at most 1 + 1 + 8 gradient slots in a step, a relation row at most 8 -- no row
    is split over work items, so every sum has a fixed order."""
    rng = np.random.default_rng(21)
    R, E, B, d = 2, 64, 8, 8
    T = 5 * B + 3
    blocks = [np.stack([R + rng.permutation(E)[:B], R + rng.permutation(E)[:B], rng.integers(0, R, B)], 1) for _ in range(6)]
    tri = np.concatenate(blocks)[:T].astype(np.int32)
    N = R + E
    id_to_type = np.concatenate([np.zeros(R), 1 + np.arange(E) // 16]).astype(np.int32)     # type 0: the relation rows
    offsets = np.array([0, R, R + 16, R + 32, R + 48, R + 64], np.int64)
    tt = H.TypeTables.from_host(id_to_type, offsets, np.arange(N, dtype=np.int32), padded_size=0)
    table = (rng.standard_normal((N, d)) * 0.3).astype(np.float32)
    return dict(B=B, d=d, N=N, T=T, tri=tri, tt=tt, table=table)


def _fb15k(H):
    """The FB15k id space and type tables with synthetic Zipfian triples, d = 8, B = 4096: full-size records (one tile of
    4096 pairs), relation rows and head entities with hundreds of slots a step."""
    from graphembeddings_amd import data as D
    fb = D.fb15k_shape()
    names, id_to_type, offsets, ids = fb.type_arrays()
    tt = H.TypeTables.from_host(id_to_type, offsets, ids, padded_size=1024)
    tri = D.synthetic_fb15k_triples(fb, n_triples=3 * 4096 + 100, seed=2)
    table = (np.random.default_rng(5).standard_normal((fb.entity_count, 8)) * 0.3).astype(np.float32)
    return dict(B=4096, d=8, N=fb.entity_count, T=len(tri), tri=tri, tt=tt, table=table)


def _drive(H, P, parts, lookahead, *, optimizer="sgd", log_loss=False, l2=0.0, deterministic=False):
    """Runs sum(parts) steps as one run() call per part; (table, accumulator, losses of every step, neg_ws after each call)."""
    emb = dev(P["table"])
    tr = H.Trainer(emb, dev(P["tri"]), P["tt"], P["B"], margin=1.0, learning_rate=0.1, decay_steps=50.0, seed=3,
                   lookahead=lookahead, optimizer=optimizer, deterministic=deterministic)
    if log_loss:
        tr.enable_log_loss(1, l2)
    assert (tr._pipe is not None) == lookahead
    losses, negs = [], []
    for n in parts:
        losses.append(tr.run(n, keep_losses=True).clone())
        negs.append(tr._neg.clone())
    torch.cuda.synchronize()
    acc = tr.accumulator
    tr.close()
    return emb, acc, torch.cat(losses), negs


def _three_ways(H, P, n, **kw):
    sevens = [7] * (n // 7) + ([n % 7] if n % 7 else [])
    one = _drive(H, P, [n], True, **kw)
    split = _drive(H, P, sevens, True, **kw)
    plain = _drive(H, P, [n], False, **kw)
    base = dev(P["table"])
    assert torch.isfinite(one[0]).all() and not torch.equal(one[0], base)
    assert (one[2] > 0).any(), "no active pair: the case checks nothing"
    for other in (split, plain):
        _same(one, other)
    return one, split, sevens


def _same(a, b):
    assert torch.equal(a[0], b[0]), "table"
    assert (a[1] is None and b[1] is None) or torch.equal(a[1], b[1]), "accumulator"
    assert torch.equal(a[2], b[2]), "losses"
    assert torch.equal(a[3][-1], b[3][-1]), "neg_ws"


def _chunk(B, negs=0):
    c = int(_lib.load().ge_train_max_chunk_steps(B, negs))
    assert c >= 1
    return c


@pytest.mark.parametrize("loop", ["hinge", "adagrad", "log_loss"])
def test_small_steps_across_two_chunk_boundaries(H, loop):
    P = _small(H)
    chunk = _chunk(P["B"], 1 if loop == "log_loss" else 0)
    n = 2 * chunk + 5
    kw = {"hinge": {}, "adagrad": {"optimizer": "adagrad"}, "log_loss": {"log_loss": True}}[loop]
    _three_ways(H, P, n, **kw)
    if loop == "log_loss":
        # With l2 > 0 the loop carries the dense decay as one scalar and multiplies it into the table when a call ends, so
        # where the calls end reaches the roundings by design: the split run above has l2 = 0 (no decay, nothing carried).
        # One call with and one without a handle end in the same place and are comparable with the decay on.
        _same(_drive(H, P, [n], True, log_loss=True, l2=0.01), _drive(H, P, [n], False, log_loss=True, l2=0.01))


def test_neg_ws_is_the_last_steps_record(H):
    """A ge_train_prepare_steps dump of steps 0 .. n-1 (one launch, no chunks): no row of this problem is split over work
    items, and the negatives a call leaves in neg_ws are the dump's for the call's last step -- for every call of the run
    split into sevens, whichever buffer and position in it that step's record had."""
    P = _small(H)
    B = P["B"]
    n = 2 * _chunk(B) + 5
    one, split, sevens = _three_ways(H, P, n)
    dump = H.prepare_steps(dev(P["tri"]), P["tt"], B, n, seed=3, direct=True)
    torch.cuda.synchronize()
    stride, n_sub, S, off_slot, off_sub, sub_stride, off_items, off_islots = H.prepared_layout(B)
    assert n_sub == 1 and dump.shape == (n, stride)
    rec = dump.cpu().numpy()
    for s in range(n):
        n_items = rec[s, off_sub]
        items = rec[s, off_sub + off_items: off_sub + off_items + 2 * n_items].reshape(-1, 2)
        assert ((items[:, 1] >> 30) & 1 == 0).all() and ((items[:, 1] & 0x3FFFFFFF) <= 16).all()
    assert np.array_equal(one[3][-1].cpu().numpy().ravel(), rec[n - 1, :3 * B])
    done = 0
    for part, neg in zip(sevens, split[3]):
        done += part
        assert np.array_equal(neg.cpu().numpy().ravel(), rec[done - 1, :3 * B]), done


def test_full_size_records_across_a_chunk_boundary(H):
    """B = 4096 on the FB15k-shaped type tables: records of full size (1.18 MB apart in the chunk buffers), the one-tile
    kernels, rows far beyond 16 slots -- reduced in a fixed order (GE_STEP_DETERMINISTIC), so the three runs are still
    bitwise comparable."""
    P = _fb15k(H)
    B = P["B"]
    stride, n_sub = H.prepared_layout(B)[:2]
    assert n_sub == 1 and stride * 4 > 1_000_000
    n = _chunk(B) + 3
    one, _, _ = _three_ways(H, P, n, deterministic=True)
    dump = H.prepare_steps(dev(P["tri"]), P["tt"], B, n, seed=3, direct=True)
    torch.cuda.synchronize()
    off_sub, off_items = H.prepared_layout(B)[4], H.prepared_layout(B)[6]
    last = dump[n - 1].cpu().numpy()
    items = last[off_sub + off_items: off_sub + off_items + 2 * last[off_sub]].reshape(-1, 2)
    assert ((items[:, 1] >> 30) & 1).any(), "no hot row: the fixed-order reduction is not exercised"
    assert np.array_equal(one[3][-1].cpu().numpy().ravel(), last[:3 * B])
