"""Host-side checks of tests/complex_shape_cases.py, so that tests/test_gpu_complex_shapes.py tests what it says: the
restated dispatch is the sources', the dims reach every key pick_shape can produce (and the runs every update-kernel
instantiation), the workloads hold what they are built for in every step of the replay, no pair sits near the hinge's
kink, and the recorded fp32-vs-fp64 gaps the bounds are made of are fresh.  `-s` prints the key and update-kernel map."""
import numpy as np
import pytest

import complex_shape_cases as SC

EVEN_DIMS = range(2, SC.MAX_DIM + 1, 2)
ALIGNMENTS = (4, 8, 16)


def test_mirrored_constants_and_dispatch_are_the_sources():
    c = SC.source_constants()
    assert (c["kWave"], c["kBlock"], c["kMaxBlocks"], c["kSub"], c["kItemCap"], c["kOneTileRowRegs"]) == (
        SC.K_WAVE, SC.K_BLOCK, SC.K_MAX_BLOCKS, SC.K_SUB, SC.K_ITEM_CAP, SC.K_ONE_TILE_ROW_REGS) == (64, 256, 2048, 4096, 16, 64)
    assert SC.source_dispatch() == SC.DISPATCH
    assert all(k == v * 1000 + l * 10 + n for k, (v, l, n) in SC.DISPATCH.items())
    assert SC.prep_layout(4096) == (1, False) and SC.prep_layout(SC.ORD_FROM_B) == (2, True)
    assert SC.prep_layout(2048, 1) == (1, False) and SC.prep_layout(2049, 1) == (2, False)
    assert [SC.one_tile_rows(r) for r in (1, 2, 4, 8, 16, 32, 64)] == [16, 16, 16, 8, 4, 2, 2]
    from graphembeddings_amd import _lib
    assert _lib.load().ge_max_dim() == SC.MAX_DIM


def test_every_key_has_both_ends_and_no_other_key_is_reachable():
    """Over every even d <= 1024 at alignments 4, 8 and 16: exactly twelve keys and GE_ENOTSUP; 4162 and 4322, which
    GE_DISPATCH_SHAPE lists, are reached by none.  DIMS holds the smallest and the largest d of each key."""
    by_key = {}
    for a in ALIGNMENTS:
        for d in EVEN_DIMS:
            by_key.setdefault(SC.shape_key(d, a), []).append((d, a))
    assert set(by_key) == set(SC.REACHABLE_KEYS) | {None} and len(SC.REACHABLE_KEYS) == 12
    assert set(SC.UNREACHABLE_KEYS) == set(SC.DISPATCH) - set(by_key) == {4162, 4322}
    assert set(SC.DIMS) == set(SC.REACHABLE_KEYS)
    print()
    for key in SC.REACHABLE_KEYS:
        vec, lpt, niter = SC.DISPATCH[key]
        aligned = [d for d, a in by_key[key] if a == 16]
        low, high = SC.DIMS[key]
        assert (low, high) == (min(aligned), max(aligned)) and SC.shape_key(low) == SC.shape_key(high) == key
        nlo, nhi = low // 2 // vec, high // 2 // vec
        assert nlo == (1 if lpt == 16 else lpt * niter // 2 + 1) and nhi <= lpt * niter
        assert nhi == lpt * niter or vec < 4                     # the high ends of VEC = 4 fill every lane
        upd = {e: "<%(vw)d, %(nj)d, RW %(rw)d>" % SC.apply_items_choice(d, 16, 1) for e, d in (("low", low), ("high", high))}
        print(f"key {key}: d {low} ({nlo} vectors) .. {high} ({nhi}); one-tile update kernel {upd['low']} .. {upd['high']}")
    print("keys 4162, 4322: unreachable")
    assert [d // 2 // SC.DISPATCH[SC.shape_key(d)][0] for d in SC.ONE_LIVE_LANE] == [65, 65, 65]
    # the refusals: the row's vectors (of the widest width k = d / 2 and the alignment allow) must fit 64 lanes x 2, so
    # aligned: d = 2 (mod 4) from 258 and d = 4 (mod 8) from 516; on a 4-byte boundary every d > 256; on an 8-byte one
    # also every d > 512
    refused = set(by_key[None])
    assert {d for d, a in refused if a == 16} == set(range(258, 1024, 4)) | set(range(516, 1024, 8))
    assert {d for d, a in refused if a == 4} == set(range(258, 1025, 2))
    assert {d for d, a in refused if a == 8} == set(range(258, 1024, 4)) | set(range(514, 1025, 2))
    for d, off in SC.REFUSED:
        assert (d, SC.alignment_of(off)) in refused and SC.route("complex", d, SC.alignment_of(off)) is None
    assert [SC.route("hole", d, SC.alignment_of(off)) for d, off in SC.REFUSED] == ["direct", None, "direct", None]
    assert [(d, off) for d, off in SC.REFUSED if SC.route("hole", d, SC.alignment_of(off))] == list(SC.HOLE_DIRECT)
    for d, off, key in SC.MISALIGNED:
        assert SC.shape_key(d, SC.alignment_of(off)) == key and off in (4, 8)


def test_runs_reach_every_update_kernel_instantiation():
    """Every apply_rows_kernel<VW, NJ, ., RW> (RW = 0: the multi-tile form) that a d the ComplEx-shaped kernels take
    reaches at some alignment is launched by a run, and so is every hot_rows_kernel<NJ>."""
    universe, hot = {}, {}
    for a in ALIGNMENTS:
        for d in EVEN_DIMS:
            if SC.pick_shape(d, a) is None:
                continue
            for n_sub in (1, 2):
                c = SC.apply_items_choice(d, a, n_sub)
                assert c["kernel"] == "apply_rows"
                universe.setdefault((c["vw"], c["nj"], c["rw"]), []).append((d, a))
            hot.setdefault(SC.apply_items_choice(d, a, 1, True)["hot_nj"], []).append(d)
    run, run_hot = {}, {}
    for test, workload, model, d, off, det in SC.LOOP_RUNS:
        n_sub, order = SC.prep_layout(SC.WORKLOADS[workload].B)
        assert (n_sub, order) == ((2, True) if workload == "two_tiles" else (1, False))
        c = SC.apply_items_choice(d, SC.alignment_of(off), n_sub, det)
        run.setdefault((c["vw"], c["nj"], c["rw"]), []).append((test, model, d, off))
        if det:
            run_hot.setdefault(c["hot_nj"], []).append(d)
    print()
    for k in sorted(set(universe) | set(run)):
        print("apply_rows_kernel<VW %d, NJ %d, RW %2d>: %4d (d, alignment) reach it; runs %s"
              % (*k, len(universe.get(k, ())), sorted({(t, d, o) for t, _, d, o in run.get(k, ())})[:4]))
    for k in sorted(hot):
        print("hot_rows_kernel<%d>: d %d .. %d; deterministic runs at d = %s" % (k, min(hot[k]), max(hot[k]), run_hot.get(k)))
    assert set(universe) <= set(run), sorted(set(universe) - set(run))
    # what the runs add: HolE on the direct kernels, at widths the ComplEx-shaped kernels refuse
    assert set(run) - set(universe) <= {(1, 8, 8)}
    assert set(hot) == set(run_hot) == {1, 2, 4, 8, 16}
    assert set(SC.GAPS) == set(SC.step_cases()) | set(SC.loop_cases())
    assert set(SC.LOGLOSS_D32) == set(SC.LOW)


def test_step_batch_is_what_it_claims():
    pos, neg = SC.step_batch()
    assert pos.shape == neg.shape == (SC.STEP_B, 3) and all(SC.STEP_B % g for g in (4, 2)) and SC.STEP_B == 67
    shared = (pos == neg).sum(1)
    assert {1, 2, 3} <= set(shared.tolist()) and (shared >= 1).all()
    s = SC.STEP_SHARES
    assert shared[s["all"]] == 3 and shared[s["r_only"]] == 1 and (pos[s["r_only"], :2] != neg[s["r_only"], :2]).all()
    assert shared[s["h_only"]] == 1 and shared[s["t_only"]] == 1 and pos[s["h_only"], 0] == neg[s["h_only"], 0]
    assert (pos[20:25] == pos[20]).all() and (neg[20:25] == neg[20]).all()
    assert ((pos[:, 2] < SC.STEP_REL) & (pos[:, :2] >= SC.STEP_REL).all(1)).all() and pos.max() < SC.STEP_N
    # no row with more than 16 slots: the table is held to the bar of a step without hot rows
    assert SC.slot_counts(pos, neg, SC.STEP_N).max() <= SC.K_ITEM_CAP
    for key in SC.step_cases():
        r = SC.step_replay(key[1], key[2])
        assert r.on[0].any() and not r.on[0].all(), key          # the hinge mask matters at every d


@pytest.mark.parametrize("name", ["small", "untyped", "two_tiles"])
def test_workloads_are_what_they_claim(name):
    w = SC.WORKLOADS[name]
    itt, offsets, ids, tri = SC.graph(name)
    bats, row_end = SC.batches(name)
    assert len(tri) == w.T and len(bats) == w.steps and [b[3] for b in bats][-1] == 0 and row_end == w.B   # the last batch wrapped
    assert (offsets[1] - offsets[0]) == 1 and ids[0] == w.n_rel                 # one type holds a single entity
    for pos, neg, gs, row in bats:
        ok = SC.valid_pairs(pos, neg, w.N)
        diff = (pos != neg)
        assert (diff.sum(1) <= 1).all() and not diff[:, 2].any()                # one entity replaced, or none
        same = ok & ~diff.any(1)
        counts = SC.slot_counts(pos, neg, w.N, ok)
        ent = counts[w.n_rel:]
        print(f"{name} step {gs}: {int((~ok).sum())} invalid pairs, {int(same.sum())} `same` pairs, "
              f"{int((ent == 1).sum())} of {int((ent > 0).sum())} entity rows with one slot, relation rows {counts[:w.n_rel].tolist()}")
        assert same.sum() >= 3
        assert (counts[:w.n_rel] > SC.K_ITEM_CAP).all()                         # every relation row: several items
        assert (ent == 1).sum() > 0.5 * (ent > 0).sum()                         # most entity rows: applied by the producer
        # a sole-slot row in each role of the four-row kernel: F (the kept entity), V (the replaced one), C (its replacement)
        col = np.where(diff[:, 0], 0, 1)
        i = np.arange(len(pos))
        sole = lambda r: ok & (counts[np.clip(r, 0, w.N - 1)] == 1)
        assert sole(pos[i, 1 - col]).any() and sole(pos[i, col]).any() and (sole(neg[i, col]) & diff.any(1)).any()
        if name == "untyped":
            assert 20 <= (~ok).sum() <= w.B // 4 and (neg[~ok] == -1).any(1).all()
        else:
            assert ok.all()
    n_sub, order = SC.prep_layout(w.B)
    if name == "two_tiles":
        assert (n_sub, order) == (2, True) and w.B - SC.K_SUB == 4              # the second tile is almost empty
        for lpt in (16, 32, 64):
            nwaves, per = SC.walk_geometry(w.B, lpt)
            assert nwaves * per >= w.B
            for pos, _, _, _ in bats:
                runs = np.bincount(pos[:, 2], minlength=w.n_rel)
                # every relation's run of the order is longer than what a workgroup's lane groups walk together: runs cross
                # the waves' stretches and the sums of several lane groups meet in the end-of-kernel merge
                assert (runs > (SC.K_BLOCK // SC.K_WAVE) * per).all(), (lpt, per, runs)
    else:
        assert (n_sub, order) == (1, False)


def test_no_pair_near_the_kink():
    """Every case, every step of the fp64 replay: no pair's pre-activation within 4 x the loss bound of 0, so the GPU
    tests compare every pair's loss, index and gradient and exclude nothing."""
    worst = np.inf
    for key in SC.step_cases() + SC.loop_cases():
        r = SC.step_replay(key[1], key[2]) if key[0] == "step" else SC.loop_replay(*key)
        assert r.kink > 4.0 * SC.bounds(key)[0], (key, r.kink)
        worst = min(worst, r.kink)
        share = float(np.mean([o.mean() for o in r.on]))
        assert 0.5 < share < 0.995, (key, share)                                # active and inactive pairs at every d
    print(f"closest pre-activation to the kink over all cases: {worst:.3g}")


@pytest.mark.parametrize("d", [d for d in SC.LOW if d > 2])         # (d = 2: one complex element, no row without it)
def test_a_dropped_tail_lane_would_show(d):
    """What the low ends are for: the last vector of a row belongs to the one lane past a power of two (at NITER = 2
    the only live lane of the second iteration).  A kernel that masked it out -- here: the fp64 oracle on a table
    without each row's last complex element -- moves the first step's losses by hundreds of times their bound, and one
    that counted the masked copies of it would move them as far the other way."""
    w = SC.WORKLOADS["small"]
    key = ("small", "complex", d)
    pos, neg, _, _ = SC.batches("small")[0][0]
    full = np.array(SC.table_of(w.N, d, SC.TABLE_SEEDS.get(key, 0), "complex"), np.float64)
    cut = full.copy()
    cut[:, [d // 2 - 1, d - 1]] = 0.0
    moved = np.abs(SC.O.evaluate_batch(pos, neg, full, SC.MARGIN) - SC.O.evaluate_batch(pos, neg, cut, SC.MARGIN)).max()
    print(f"d {d}: losses move by {moved:.3g} without the tail element, bound {SC.bounds(key)[0]:.3g}")
    assert moved > 100.0 * SC.bounds(key)[0]


@pytest.mark.parametrize("kind", ["step", "small", "two_tiles", "untyped"])
def test_recorded_gaps_are_fresh(kind):
    """The fp32 implementation against the fp64 oracle, recomputed: within a factor of two of the recorded gap (the C
    port's threads and torch's FFT may order sums otherwise), so never past the bound made of it."""
    for key in [k for k in SC.step_cases() + SC.loop_cases() if k[0] == kind]:
        fresh = SC.measure_step_gap(*key[1:]) if kind == "step" else SC.measure_loop_gap(*key)
        for f, rec, bound in zip(fresh, SC.GAPS[key], SC.bounds(key)):
            assert f / 2 <= rec <= f * 2 and SC.HEADROOM * f < 2 * bound, (key, fresh, SC.GAPS[key])
    assert SC.bounds(("step", "complex", 2)) == (SC.SCORE_TOL, SC.TABLE_TOL)
    assert SC.bounds(("small", "complex", 2)) == (SC.SCORE_TOL, SC.HOT_TABLE_TOL)


def test_recorded_logloss_d32_is_fresh():
    import logloss_cases as LC
    for d in SC.LOW:
        fresh = SC.measure_logloss_d32(d)
        assert fresh / 2 <= SC.LOGLOSS_D32[d] <= fresh * 2, (d, fresh)
        _, l64 = SC.logloss_replay(d)
        _, l32 = SC.logloss_replay(d, True)
        assert max(float(np.abs(a - b).max()) / LC.loss_tol(b) for a, b in zip(l32, l64)) < 0.1
    bats, _ = SC.batches("logloss")
    for pos, negs, gs, row in bats:
        counts = LC.slot_counts(LC.step_triples(pos, negs), SC.WORKLOADS["logloss"].N)
        assert (counts[:8] > SC.K_ITEM_CAP).all()
    assert SC.prep_layout(SC.LOGLOSS_B, SC.LOGLOSS_K) == (1, False) and bats[-1][3] == 0
