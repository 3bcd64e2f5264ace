#!/usr/bin/env python3
"""bench.py -- scored triples/s of the holE.py hot path on MI355X (BASELINE.json metric).

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR]
  (N>1 under a launcher: python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...;
   N>1 WITHOUT one: this file starts its own N ranks, graphembeddings_amd/launch.py, before anything touches the GPU)

A "step" is one pass of the hot path over one batch: type-safe corruption of B positives, fused
gather -> clip -> ComplEx score -> sigmoid -> hinge -> row gradients, sparse SGD scatter-add; it
scores 2B triples (B positives + B negatives).  Inputs (table, triples, type tables) are resident in
HBM before the timed region.  N=1 runs BASELINE config[1] (FB15k-shaped, d=200, B=4096, 1 neg/pos);
N>1 runs config[3] (1.2 M-entity synthetic, table row-sharded, RCCL all-to-all), B per GPU fixed
(weak scaling).  Rank 0 prints ONE JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHARDED_BATCH = 65536   # positives per GPU per step on the row-sharded path (config[3])
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s; ~6.3 TB/s achievable)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--workload", default="auto", choices=["auto", "fb15k", "synthetic"])
    ap.add_argument("--batch", type=int, default=None,
                    help="positives per GPU per step (default 4096 on 1 GPU = config[1]; 65536 per GPU on the sharded path)")
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--model", default="complex", choices=["complex", "hole"])
    ap.add_argument("--sharded", action="store_true", help="run the row-sharded (all-to-all) path even on 1 GPU")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-score-roofline", action="store_true")
    ap.add_argument("--no-hbm-roofline", action="store_true",
                    help="skip the HBM-bound leg of the train step (960 MB table, 65,536 pairs per step)")
    ap.add_argument("--no-rank-roofline", action="store_true",
                    help="skip the MFMA-bound leg (the link-prediction rank sweep at the FB15k test set's shape)")
    ap.add_argument("--no-extra-configs", action="store_true",
                    help="skip the legs for BASELINE configs 3 (HolE d=200 B=4096 step) and 5 (4096 x 256 x 200 1-vs-K contraction)")
    ap.add_argument("--no-scaling-base", action="store_true",
                    help="skip the 1-GPU run of the row-sharded config[3] workload that the N>1 lines are comparable to")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--partition", default="head", choices=["head", "random"],
                    help="N>1: which triples a rank trains -- those whose head row it owns (default), or a random share")
    ap.add_argument("--plan-group", action="store_true",
                    help="N>1: run the exchange planner's collectives on a second communicator (untested on hardware)")
    ap.add_argument("--overlap", action="store_true",
                    help="N>1, opt-in: fetch the rows of step s+1 that no rank touches in step s on a communication stream while "
                         "step s computes (bitwise the serial schedule's result; not yet run on RCCL)")
    ap.add_argument("--capacity", default=None,
                    help="N>1, opt-in: equal-split all-to-alls with this many rows per peer and step ('auto': 1.25 x the first "
                         "chunk's largest count) -- no split size is read back, the whole run is enqueued ahead of the device; "
                         "bitwise the exact schedule's result (gloo tests); not yet run on RCCL")
    ap.add_argument("--peer-mapped", action="store_true",
                    help="N>1 EXPERIMENT: map the other ranks' shards by IPC and read their rows in place instead of the row "
                         "all-to-all (two cross-rank barriers per step); rehearsed on one device only, needs peer access on hardware")
    ap.add_argument("--entities", type=int, default=1_200_000)
    ap.add_argument("--triples", type=int, default=30_000_000)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="1 GPU: after the timed steps, write what their last step computed (the step's hinge losses and "
                         "the updated table; a fixed sample of its rows if it would pass 32 MB) as DIR/<name>.npy, float32")
    return ap.parse_args()


def algorithmic_bytes(kernel: int, B: int, d: int) -> float:
    """fused train step = 72d+28 B per (pos,neg) pair, split over our launches as
    kernel 1 (gather+score+hinge+grad): 6 rows read + ids + loss = 24d+28; kernel 2 (scatter-add):
    read-modify-write of 6 rows = 48d; kernel 0 (sampler): 2 id triples + 1 type code."""
    per_pair = {0: 12 + 12 + 4 + 4, 1: 24 * d + 28, 2: 48 * d}[kernel]
    return float(per_pair) * B


KERNEL_NAMES = {0: "train_prepare_kernel", 1: "complex_hinge_grad_plan_kernel", 2: "apply_rows_kernel"}   # (round 4: the four-row / whole-row kernels at every batch size)


def pmc_traffic(kernel_name: str, tag: str):
    """HBM bytes per launch of `kernel_name` from the newest committed rocprofv3 PMC summary for this
    workload (profiles/*<tag>_pmc.json, produced by tools/profile_bench.sh: separate --pmc FETCH_SIZE /
    WRITE_SIZE passes, FETCH_SIZE doubled per the gfx950 correction).  None when no profile exists."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"*{tag}_pmc.json")))
    if not files:
        return None
    try:
        kern = json.load(open(files[-1])).get("kernels", {})
    except Exception:
        return None
    for name, v in kern.items():
        if kernel_name.split("<")[0] in name:
            return {"hbm_bytes_per_launch": v.get("hbm_bytes_corrected"), "source": os.path.basename(files[-1])}
    return None


def score_kernel_roofline(d, n_rows=1_200_018, n_triples=1 << 22, iters=10):
    """The kernel north_star sets the >=70 %-of-HBM target on: the fused gather + ComplEx score
    (ge_complex_score) at d=200, measured where it is HBM-bound -- a 960 MB table (> 256 MB Infinity
    Cache), uniformly random rows, 4 M triples per launch.  Algorithmic bytes 12d+16 per scored triple
    (SURVEY.md 8d).  Supplementary to `roofline` (which is the dominant kernel of the timed train step)."""
    import torch
    from graphembeddings_amd import hole as H
    g = torch.Generator(device="cuda").manual_seed(0)
    table = torch.randn(n_rows, d, device="cuda", generator=g) * 0.05
    tr = torch.randint(0, n_rows, (n_triples, 3), device="cuda", generator=g, dtype=torch.int32)
    for _ in range(2):
        H.evaluate_triples(tr, table)
    torch.cuda.synchronize()
    ev = H.Events(2)
    ev.record(0)
    for _ in range(iters):
        H.evaluate_triples(tr, table)
    ev.record(1)
    torch.cuda.synchronize()
    ms = ev.elapsed_ms(0, 1) / iters
    ev.close()
    alg = (12 * d + 16) * n_triples
    achieved = alg / (ms * 1e-3) / 1e9
    del table, tr
    return {"kernel": "complex_score_kernel", "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS,
            "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "kernel_ms": ms, "triples_per_launch": n_triples,
            "table_rows": n_rows, "table_mb": round(n_rows * d * 4 / 1e6, 1),
            "scored_triples_per_s": n_triples / (ms * 1e-3), "algorithmic_bytes_per_launch": alg}


def train_step_hbm_roofline(d, B=SHARDED_BATCH, n_entities=1_200_000, steps=48):
    """The whole train step where it is HBM-bound (the headline FB15k step is one round of waves on a 13 MB
    cache-resident table and cannot show bandwidth): ge_train_steps on the 1.2 M-row table (960 MB > the 256 MB
    Infinity Cache), Zipf(0.8) ids, B = 65,536 pairs per step.  Above B = 4096 the step's gradient slots are sorted
    across workgroups (csrc/ge_prep_big.hip), so every distinct row still gets ONE plain read-modify-write.
    Algorithmic bytes: 72d+28 per pair for the step, 24d+28 / 48d for its two kernels."""
    import torch
    from graphembeddings_amd import data as D
    from graphembeddings_amd import hole as H
    data, tri = D.synthetic_large(n_entities=n_entities, n_triples=max(8 * B, 2_000_000), seed=1234)
    names, id_to_type, offsets, ids = D.synthetic_large_type_arrays(data)
    tt = H.TypeTables.from_host(id_to_type, offsets, ids, padded_size=1024)
    dtri = torch.as_tensor(tri).cuda()
    emb = H.init_embeddings(data.entity_count, d, seed=0)
    tr = H.Trainer(emb, dtri, tt, B, margin=0.2, learning_rate=0.1, decay_steps=32.0 * (30_000_000 // B), seed=0)
    tr.run(steps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.run(steps)
    torch.cuda.synchronize()
    el = (time.perf_counter() - t0) / steps
    kern = {}
    for k, name in ((1, "complex_hinge_grad_plan_kernel"), (2, "apply_rows_kernel")):
        ev = H.Events(2 * steps)
        tr.run(steps, events=ev.handles, ev_kernel=k)
        torch.cuda.synchronize()
        kern[name] = float(np.median([ev.elapsed_ms(2 * i, 2 * i + 1) for i in range(steps)]))
        ev.close()
    loss = float(tr.last_loss.mean())
    tr.close()
    del emb, tr, dtri
    alg = {"step": (72 * d + 28) * B, "complex_hinge_grad_plan_kernel": (24 * d + 28) * B}
    traffic = {k: pmc_traffic(k, f"synthetic_d{d}_b{B}") for k in kern}
    # Two fractions, side by side.  `useful_bytes_frac`: SURVEY.md 8(d)'s ALGORITHMIC bytes of a step (72d+28 per pair: six
    # rows read, six read-modify-written) over the step's time -- credit for bytes the path does not move at all (a pair's
    # negative shares two rows with its positive, relation rows are summed in registers, sole-slot rows are updated by the
    # producing pair).  `achieved` / `frac`: the bytes the two kernels REALLY move per step (committed rocprofv3 PMC
    # summary of this very workload) over the step's time -- DRAM utilisation, the figure a roofline is about.
    moved = sum(t["hbm_bytes_per_launch"] for t in traffic.values() if t) if all(traffic.values()) else None
    return {"workload": f"synthetic {n_entities} entities, complex d={d}, batch={B}, native loop (ge_train_steps), 1 GPU",
            "bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s", "table_mb": round(data.entity_count * d * 4 / 1e6, 1),
            "ms_per_step": el * 1e3, "scored_triples_per_s": 2.0 * B / el,
            "achieved": (moved / el / 1e9) if moved else None, "frac": (moved / el / 1e9 / HBM_PEAK_GBS) if moved else None,
            "traffic": moved, "traffic_source": next((t["source"] for t in traffic.values() if t), None),
            "useful_bytes_per_step": alg["step"], "useful_GBs": alg["step"] / el / 1e9,
            "useful_bytes_frac": alg["step"] / el / 1e9 / HBM_PEAK_GBS,
            # per kernel: its time and its measured HBM traffic (committed PMC summary).  An algorithmic figure is given
            # for the gradient kernel only: the 48d of the update's read-modify-writes are mostly done inside it (sole-slot
            # rows) or merged before the apply kernel runs, so a per-kernel share of them would be arbitrary.
            "kernels": {k: dict({"kernel_ms": v, "traffic": traffic[k]["hbm_bytes_per_launch"] if traffic[k] else None,
                                 "traffic_source": traffic[k]["source"] if traffic[k] else None},
                                **({"measured_GBs": traffic[k]["hbm_bytes_per_launch"] / (v * 1e-3) / 1e9,
                                    "measured_frac": traffic[k]["hbm_bytes_per_launch"] / (v * 1e-3) / 1e9 / HBM_PEAK_GBS} if traffic[k] else {}),
                                **({"algorithmic_bytes_per_launch": alg[k], "useful_GBs": alg[k] / (v * 1e-3) / 1e9,
                                    "useful_bytes_frac": alg[k] / (v * 1e-3) / 1e9 / HBM_PEAK_GBS} if k in alg else {}))
                        for k, v in kern.items()},
            "final_mean_hinge": round(loss, 6)}


def rank_sweep_mfma_roofline(d, n_rows=59_071, n_entities=16_296, n_relations=1_345, iters=5):
    """The one MFMA-bound kernel on the path: the link-prediction sweep of holE.py:564-575 with the ranking of
    holE.py:427-472 as its epilogue (ge_rank_1vK_planes), at the FB15k test set's shape -- 59,071 (entity, relation)
    rows x 14,951 candidates, synthetic ids and table.  Split precision: three v_mfma_f32_32x32x16_f16 per 16-wide k
    block, so the flops it EXECUTES are 3 x 2 x rows x candidates x 16 ceil(d / 16); peak = the dense f16 MFMA rate."""
    import torch
    from graphembeddings_amd import hole as H
    g = torch.Generator(device="cpu").manual_seed(3)
    emb = H.init_embeddings(n_entities, d, seed=3) * 4.0
    cand = torch.arange(n_relations, n_entities, dtype=torch.int32).cuda()
    hr = torch.stack([torch.randint(n_relations, n_entities, (n_rows,), generator=g),
                      torch.randint(0, n_relations, (n_rows,), generator=g)], 1).int().cuda()
    tid = torch.randint(n_relations, n_entities, (n_rows,), generator=g).int().cuda()
    planes = H.RankPlanes(emb, cand)                    # once per evaluation, as evaluate.py does
    for _ in range(2):
        H.rank_candidates(emb, hr, tid, cand, planes=planes)
    ev = H.Events(2 * iters)
    for i in range(iters):
        ev.record(2 * i)
        nb, _ = H.rank_candidates(emb, hr, tid, cand, planes=planes)
        ev.record(2 * i + 1)
    torch.cuda.synchronize()
    ms = float(np.median([ev.elapsed_ms(2 * i, 2 * i + 1) for i in range(iters)]))
    ev.close()
    K = int(cand.numel())
    kpad = 16 * ((d + 15) // 16)
    split = planes.buffer is not None
    executed = (3 if split else 1) * 2.0 * n_rows * K * (kpad if split else d)
    peak = 2500.0 if split else 157.0                   # dense f16 / fp32 MFMA, MI355X_MICROARCH.md
    return {"workload": f"FB15k test-set shape: {n_rows} rows x {K} candidates, complex d={d}, ranks counted in the epilogue, candidate planes built once",
            "bound": "mfma", "kernel": "rank_f16_kernel" if split else "rank_pipe_kernel", "kernel_ms": ms,
            "achieved": executed / (ms * 1e-3) / 1e12, "peak": peak, "unit": "TFLOP/s",
            "frac": executed / (ms * 1e-3) / 1e12 / peak, "executed_flop_per_launch": executed,
            "fp32_equivalent_tflops": 2.0 * n_rows * K * d / (ms * 1e-3) / 1e12,
            "mean_rank": float(nb.float().mean()) + 1.0}


def config3_hole_step(d, B=4096, steps=400, warmup=64):
    """BASELINE config 3: FB15k-shaped, HolE (README.md:42: r . (h correlated with t)) d=200, batch 4096, 1 neg/pos, one GPU.
    The table is carried in the frequency domain for the whole run (what train.py does: ge_hole_to_spectral once, then
    the ComplEx-shaped pair of kernels with Hermitian weights), so a step is prepare (side stream) + gradient + update,
    like config 2's.  Reported: ms per step over `steps` steps in back-to-back native calls, scored triples/s, each
    kernel's own time (HIP events on its dispatch) and the dominant one's algorithmic bytes against the HBM peak."""
    import torch
    from graphembeddings_amd import data as D
    from graphembeddings_amd import hole as H
    fb = D.fb15k_shape()
    names, id_to_type, offsets, ids = fb.type_arrays()
    triples = D.synthetic_fb15k_triples(fb, n_triples=483142, seed=0)
    emb = H.init_embeddings(fb.entity_count, d, seed=0)
    tt = H.TypeTables.from_host(id_to_type, offsets, ids, padded_size=1024)
    dtri = torch.as_tensor(triples).cuda()
    tr = H.Trainer(emb, dtri, tt, B, margin=0.2, learning_rate=0.1, decay_steps=32.0 * (len(triples) // B), decay_rate=0.5,
                   model="hole", seed=0, spectral_resident=True)
    tr.reshuffle(torch.Generator(device="cuda").manual_seed(0))
    tr.run(warmup)
    torch.cuda.synchronize()
    call = 20                                             # steps per native call, as the driver's --steps
    t0 = time.perf_counter()
    for _ in range(steps // call):
        tr.run(call)
    torch.cuda.synchronize()
    el = (time.perf_counter() - t0) / (steps // call * call)
    kern = {}
    probe = 32
    for k, name in ((1, "complex_hinge_grad_plan_kernel<SPEC>"), (2, "apply_rows_kernel")):
        ev = H.Events(2 * probe)
        tr.run(probe, events=ev.handles, ev_kernel=k)
        torch.cuda.synchronize()
        kern[name] = float(np.median([ev.elapsed_ms(2 * i, 2 * i + 1) for i in range(probe)]))
        ev.close()
    loss = float(tr.last_loss.mean())
    tr.close()
    dom = max(kern, key=kern.get)
    alg = algorithmic_bytes(1 if "grad" in dom else 2, B, d)
    return {"workload": f"FB15k-shaped, HolE d={d} (table resident in the frequency domain), batch={B}, 1 neg/pos, 1 GPU",
            "ms_per_step": el * 1e3, "scored_triples_per_s": 2.0 * B / el, "steps": steps // call * call,
            "kernels_ms": {k: round(v, 5) for k, v in kern.items()}, "dominant_kernel": dom, "bound": "hbm",
            "algorithmic_bytes_per_launch": alg, "achieved": alg / (kern[dom] * 1e-3) / 1e9, "peak": HBM_PEAK_GBS,
            "unit": "GB/s", "frac": alg / (kern[dom] * 1e-3) / 1e9 / HBM_PEAK_GBS, "final_mean_hinge": round(loss, 6)}


def config5_score_1vK(d, B=4096, K=256, calls=400):
    """BASELINE config 5 at its own shape: FB15k-shaped table, 4096 (entity, relation) rows against 256 shared negatives
    as ONE (B x d) . (d x K) contraction on the matrix cores (ge_complex_score_1vK: clip scales, sigmoid and the [B,K]
    store in the epilogue).  us per call over `calls` back-to-back calls into a preallocated output, flop = 2 B K d."""
    import torch
    from graphembeddings_amd import _lib
    from graphembeddings_amd import hole as H
    N, R = 16296, 1345
    emb = H.init_embeddings(N, d, seed=0) * 4.0
    g = torch.Generator().manual_seed(0)
    hr = torch.stack([torch.randint(R, N, (B,), generator=g), torch.randint(0, R, (B,), generator=g)], 1).int().cuda()
    cand = torch.randint(R, N, (K,), generator=g).int().cuda()
    out = torch.empty(B, K, device="cuda")
    st = H._stream()

    def one():
        _lib.call("ge_complex_score_1vK", emb.data_ptr(), N, d, hr.data_ptr(), B, cand.data_ptr(), K, 1.0, 1, 0, out.data_ptr(), st)
    for _ in range(8):
        one()
    torch.cuda.synchronize()
    ev = H.Events(2)
    ev.record(0)
    for _ in range(calls):
        one()
    ev.record(1)
    torch.cuda.synchronize()
    us = ev.elapsed_ms(0, 1) / calls * 1e3
    ev.close()
    ref = H.evaluate_triples(torch.stack([hr[:64, 0], cand[:64], hr[:64, 1]], 1), emb)[:, 0]
    err = float((out[:64, :64].diagonal() - ref).abs().max())
    flop = 2.0 * B * K * d
    split = d % 8 == 0 and 56 <= d <= 224
    return {"workload": f"FB15k-shaped table, {B} (entity, relation) rows x {K} shared negatives, complex d={d}: one [B,d] x [d,K] contraction",
            "kernel": "score_1vK_f16_kernel (split precision: 3 f16 MFMAs per product, fp32-class accuracy)" if split else "score_1vK_tile_kernel (fp32 MFMA)",
            "us_per_call": us, "calls": calls, "scored_triples_per_s": B * K / (us * 1e-6), "flop_per_call": flop,
            "bound": "mfma (in practice launch + two dependent memory round trips: a 0.4 GFLOP problem)",
            "achieved": flop / (us * 1e-6) / 1e12, "peak": 157.3, "unit": "TFLOP/s (fp32-equivalent against the fp32 MFMA peak)",
            "frac": flop / (us * 1e-6) / 1e12 / 157.3, "max_abs_diff_vs_per_triple_kernel": err}


def cpu_baseline_fb15k(fb, type_arrays, d, B, seconds):
    """The oracle's C port (OpenMP) timed on this host on a bounded sample of the same workload:
    FB15k-shaped table, B positives per step, sampler + fused hinge step."""
    from oracle import c_oracle as CO
    from oracle import hole_oracle as O
    from graphembeddings_amd import data as D
    names, id_to_type, offsets, ids = type_arrays
    try:
        avail = len(os.sched_getaffinity(0))      # the cores this process may actually run on
    except AttributeError:
        avail = os.cpu_count() or 1
    table = O.init_table(fb.entity_count, d, seed=0)
    tri = D.synthetic_fb15k_triples(fb, n_triples=max(4 * B, 20000), seed=0)
    nb = len(tri) // B
    neg = CO.corrupt_batch(tri[:B], id_to_type, offsets, ids, 0, 0, 1024, 0)
    # thread count: the visible cores can exceed the container's CPU share (then a full-width OpenMP team
    # is slower than a narrow one), so time a few team sizes on 3 steps each and keep the fastest
    cap = max(1, min(CO.num_threads(), avail))
    cands = sorted({c for c in (cap, cap // 2, cap // 4, 32, 16, 8, 4, 1) if 1 <= c <= cap}, reverse=True)
    best = None
    for c in cands:
        CO.hinge_step(table, tri[:B], neg, 0.2, 0.1, threads=c)
        t = time.perf_counter()
        for _ in range(3):
            CO.hinge_step(table, tri[:B], neg, 0.2, 0.1, threads=c)
        t = (time.perf_counter() - t) / 3
        if best is None or t < best[0]:
            best = (t, c)
    threads = best[1]
    table = O.init_table(fb.entity_count, d, seed=0)
    CO.hinge_step(table, tri[:B], neg, 0.2, 0.1, threads=threads)   # warm-up at the chosen width
    t0 = time.perf_counter()
    steps = 0
    while time.perf_counter() - t0 < seconds and steps < 100000:
        pos = tri[(steps % nb) * B:(steps % nb + 1) * B]
        neg = CO.corrupt_batch(pos, id_to_type, offsets, ids, 0, steps + 1, 1024, 0)
        CO.hinge_step(table, pos, neg, 0.2, 0.1, threads=threads)
        steps += 1
    el = time.perf_counter() - t0
    # the reference's own per-batch host resample (holE.py:343-344), timed once for the record
    import random
    lists = [list(v) for v in fb.type_to_ids.values()]
    t1 = time.perf_counter()
    _ = [[random.choice(v) for _ in range(1024)] for v in lists]
    resample_s = time.perf_counter() - t1
    return {"value": 2.0 * B * steps / el, "unit": "scored triples/s", "cores": threads, "kind": "port",
            "sample": f"{steps} steps of B={B} (sampler + fused hinge SGD step, C/OpenMP oracle port, "
                      f"FB15k-shaped d={d}) in {el:.1f}s; {threads} of {avail} visible cores "
                      f"(fastest of team sizes {cands})",
            "reference_host_resample_s_per_step": round(resample_s, 3)}


DUMP_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """Write each device array as out_dir/<name>.npy in float32.  An array larger than its share of DUMP_BYTES is
    written as a fixed, seeded sample of its rows (sorted row ids), the same rows in every run of the same shape."""
    import torch
    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_BYTES // len(arrays)
    for name, t in arrays.items():
        a = t.detach().float()
        if a.numel() * 4 > share:
            row_bytes = max(1, a[0].numel()) * 4
            rows = np.sort(np.random.default_rng(0).choice(a.shape[0], share // row_bytes, replace=False))
            a = a[torch.as_tensor(rows, dtype=torch.int64, device=a.device)]
            name += "_sample"
        np.save(os.path.join(out_dir, f"{name}.npy"), a.cpu().numpy().astype(np.float32))


def run_single(args):
    import torch
    from graphembeddings_amd import data as D
    from graphembeddings_amd import hole as H
    torch.cuda.set_device(0)
    d, B, K, W = args.dim, args.batch, args.steps, args.warmup
    workload = "fb15k" if args.workload == "auto" else args.workload
    if workload == "fb15k":
        fb = D.fb15k_shape()
        arrays = fb.type_arrays()
        triples = D.synthetic_fb15k_triples(fb, n_triples=483142, seed=0)
        n_rows = fb.entity_count
        name = f"FB15k-shaped (16,296 rows, 815 types, 483,142 synthetic train triples), {args.model} d={d}, batch={B}, 1 neg/pos, fused gather+score+hinge+grad + scatter SGD"
    else:
        data, triples = D.synthetic_large(n_entities=args.entities, n_triples=args.triples, seed=1234)
        arrays = D.synthetic_large_type_arrays(data)
        fb = data
        n_rows = data.entity_count
        name = f"synthetic {args.entities} entities / {args.triples} triples, {args.model} d={d}, batch={B}, single GPU"
    names, id_to_type, offsets, ids = arrays
    emb = H.init_embeddings(n_rows, d, seed=0)
    tt = H.TypeTables.from_host(id_to_type, offsets, ids, padded_size=1024)
    dtri = torch.as_tensor(triples).cuda()
    batch_count = len(triples) // B
    # HolE: the table is transformed to the frequency domain once, here (untimed setup, like the upload),
    # and stays spectral for the run -- what train.py does; the steps are then ComplEx-shaped
    tr = H.Trainer(emb, dtri, tt, B, margin=0.2, learning_rate=0.1, decay_steps=32.0 * batch_count,
                   decay_rate=0.5, model=args.model, seed=0, spectral_resident=(args.model == "hole"))
    tr.reshuffle(torch.Generator(device="cuda").manual_seed(0))

    # warm-up (untimed) + pick the dominant kernel by timing each of the 3 launches with HIP events
    tr.run(W)
    torch.cuda.synchronize()
    probe = max(8, min(W, 64))
    ev = H.Events(2 * probe)
    avg = {}
    for kern in (1, 2):   # kernel 0 (prepare: sampler + LDS sort) runs on a side stream, off the critical path
        tr.run(probe, events=ev.handles, ev_kernel=kern)
        torch.cuda.synchronize()
        avg[kern] = sum(ev.elapsed_ms(2 * i, 2 * i + 1) for i in range(probe)) / probe
    ev.close()
    # the dominant kernel; the two launches of a step take the same time to within a few per cent at config[1], so a tie
    # (within 5 %) goes to the gradient kernel -- the one SURVEY.md 8(d)'s per-unit figure describes -- instead of to noise
    dom = max(avg, key=avg.get)
    if avg[1] >= 0.95 * avg[dom]:
        dom = 1
    kernel_names = dict(KERNEL_NAMES)
    if args.model == "hole":
        kernel_names[1] = "complex_hinge_grad_plan_kernel<SPEC>"   # same kernel template, Hermitian weights

    # timed region: ONE ge_train_steps call of exactly K steps, as the driver asks (`value` and `ms_per_step`).  It
    # continues the sequence, so its prepared records were built ahead on the side stream.  Before it, untimed:
    # `cold_call`, one K-step call right after a pipeline reset with its first prepare launch exposed, then one K-step
    # call with HIP events on the dominant kernel's dispatch in every 4th step (`kernel_ms`) -- events in every step
    # would add two barrier packets per step, and none ride in the timed call.
    EVERY = 4
    tr.invalidate()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.run(K)
    torch.cuda.synchronize()
    cold_el = time.perf_counter() - t0
    ev = H.Events(2 * ((K + EVERY - 1) // EVERY))
    handles = []
    for i in range(K):
        handles += ([ev.handles[2 * (i // EVERY)], ev.handles[2 * (i // EVERY) + 1]] if i % EVERY == 0 else [None, None])
    tr.run(K, events=handles, ev_kernel=dom)
    torch.cuda.synchronize()
    n_ev = len(ev.handles) // 2
    kern_ms = sum(ev.elapsed_ms(2 * i, 2 * i + 1) for i in range(n_ev)) / n_ev
    ev.close()
    t0 = time.perf_counter()
    loss = tr.run(K)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"loss": loss, "embeddings": tr.real_embeddings()})
    loss_mean = float(tr.last_loss.mean())
    assert np.isfinite(loss_mean), "training diverged / invalid ids"

    value = 2.0 * B * K / el
    alg = algorithmic_bytes(dom, B, d)
    achieved = alg / (kern_ms * 1e-3) / 1e9
    tag = f"{workload}_d{d}_b{B}" if args.model == "complex" else f"{workload}_{args.model}_d{d}_b{B}"
    traffic = pmc_traffic(kernel_names[dom], tag)
    out = {
        "metric": "scored triples/sec/GPU (d=200)", "value": value, "unit": "scored triples/s",
        "n_gpus": 1, "ranks_seen": 1, "backend": "none (one rank: no collective runs)",
        "steps": K, "warmup": W, "ms_per_step": el / K * 1e3, "higher_is_better": True,
        "timed_calls": 1, "timed_ms": el * 1e3,
        "cold_call": {"value": 2.0 * B * K / cold_el, "ms_per_step": cold_el / K * 1e3,
                      "note": "one K-step call right after a pipeline reset (first prepare launch exposed)"},
        "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": name, "batch_per_gpu": B, "embedding_dim": d, "table_rows": int(n_rows),
                   "table_mb": round(n_rows * d * 4 / 1e6, 1), "parallelism": "1 GPU",
                   "scored_triples_per_step": 2 * B, "final_mean_hinge": round(loss_mean, 6)},
        "roofline": {"bound": "hbm", "kernel": kernel_names[dom], "achieved": achieved, "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                     "traffic": traffic["hbm_bytes_per_launch"] if traffic else None,
                     "traffic_source": traffic["source"] if traffic else None,
                     "algorithmic_bytes_per_launch": alg, "kernel_ms": kern_ms,
                     "all_kernels_ms": {kernel_names[k]: round(v, 5) for k, v in avg.items()},
                     "step_algorithmic_bytes": (72 * d + 28) * B,
                     "step_achieved_GBs": (72 * d + 28) * B / (el / K) / 1e9},
    }
    if args.model == "hole":
        # what the frequency-domain representation costs when it is entered / left: one row-wise real DFT
        # of the whole table each way (paid once per training run by train.py, once per call by model 1)
        scratch = tr.real_embeddings().clone()
        torch.cuda.synchronize()
        ev2 = H.Events(2)
        ev2.record(0)
        for _ in range(5):
            H.hole_to_spectral(scratch)
            H.hole_from_spectral(scratch)
        ev2.record(1)
        torch.cuda.synchronize()
        out["config"]["hole_transform_pair_ms"] = ev2.elapsed_ms(0, 1) / 5
        ev2.close()
        del scratch
    if not args.no_score_roofline:
        out["score_kernel_roofline"] = score_kernel_roofline(d)
    if not args.no_hbm_roofline and args.workload == "auto" and args.model == "complex":
        try:
            out["train_step_hbm_roofline"] = train_step_hbm_roofline(d)
        except Exception as e:  # never lose the headline line to an auxiliary leg
            out["train_step_hbm_roofline"] = {"error": f"{type(e).__name__}: {e}"}
    if not args.no_rank_roofline and args.workload == "auto" and args.model == "complex":
        try:
            out["rank_sweep_mfma_roofline"] = rank_sweep_mfma_roofline(d)
        except Exception as e:  # never lose the headline line to an auxiliary leg
            out["rank_sweep_mfma_roofline"] = {"error": f"{type(e).__name__}: {e}"}
    if not args.no_extra_configs and args.workload == "auto" and args.model == "complex":
        for key, fn in (("config3_hole_step", config3_hole_step), ("config5_score_1vK", config5_score_1vK)):
            try:
                out[key] = fn(d)
            except Exception as e:  # never lose the headline line to an auxiliary leg
                out[key] = {"error": f"{type(e).__name__}: {e}"}
    if not args.no_cpu_baseline and workload == "fb15k":
        out["cpu_baseline"] = cpu_baseline_fb15k(fb, arrays, d, B, args.cpu_seconds)
    elif not args.no_cpu_baseline:
        out["cpu_baseline"] = None
    if not args.no_scaling_base and args.workload == "auto" and args.model == "complex":
        # The N>1 lines run BASELINE config[3] (960 MB table, row-sharded exchange) while this line is
        # config[1] (13 MB table, no exchange): report the 1-GPU value of the N>1 workload beside it so
        # weak-scaling efficiency can be read like for like (value(N) / (N * scaling_base.value)).
        import copy
        from graphembeddings_amd import sharded_bench
        a2 = copy.copy(args)
        a2.batch, a2.steps, a2.warmup = SHARDED_BATCH, 128, 64
        try:
            sb = sharded_bench.run(a2, emit=False)
            out["scaling_base"] = {"workload": sb["config"]["workload"], "batch_per_gpu": a2.batch, "value": sb["value"],
                                   "unit": sb["unit"], "ms_per_step": sb["ms_per_step"],
                                   "host_enqueue_ms_per_step": sb.get("host_enqueue_ms_per_step"), "n_gpus": 1,
                                   "note": "same code path and per-GPU batch as `bench.py --gpus N` for N>1"}
        except Exception as e:  # never lose the headline line to the auxiliary run
            out["scaling_base"] = {"error": f"{type(e).__name__}: {e}"}
    print(json.dumps(out))


def main():
    os.environ.setdefault("OMP_WAIT_POLICY", "passive")   # idle OpenMP workers of the CPU baseline must not spin
    args = parse()
    if args.dump_outputs and (args.gpus > 1 or args.sharded):
        print("bench.py: --dump-outputs is implemented for the 1-GPU path only", file=sys.stderr)
        sys.exit(2)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher around us: this process becomes the parent of N ranks.  It has not touched the GPU (nothing imported
        # so far initialises HIP; counting devices does not) and it never execs -- the ranks are ordinary children that
        # re-run this file with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set; rank 0 prints the line on our stdout.
        from graphembeddings_amd import launch
        try:
            rc = launch.spawn_ranks(args.gpus, sys.argv[1:], script=os.path.abspath(__file__))
        except (RuntimeError, ValueError) as e:
            print(json.dumps({"metric": "scored triples/sec/GPU (d=200)", "value": 0.0, "unit": "scored triples/s",
                              "n_gpus": args.gpus, "ranks_seen": 0, "error": f"{type(e).__name__}: {e}"}), flush=True)
            sys.exit(2)
        sys.exit(rc)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and args.gpus != world:
        print(f"bench.py: --gpus {args.gpus} but the launcher started {world} ranks", file=sys.stderr)
        sys.exit(2)
    sharded = args.gpus > 1 or world > 1 or args.sharded
    if args.batch is None:
        # config[3] names no batch size.  The exchange costs two all-to-alls of (distinct rows x d) per step
        # plus fixed latencies, so the per-GPU batch is chosen large (measured on one GPU through the same
        # path: 219 / 266 / 291 / 312 M scored triples/s at 16k / 32k / 64k / 128k); it is the same for
        # every N (weak scaling)
        args.batch = SHARDED_BATCH if sharded else 4096
    if sharded:
        from graphembeddings_amd import sharded_bench
        try:
            sharded_bench.run(args)
        except Exception as e:  # leave a diagnosable line for the driver, then fail loudly
            import traceback
            traceback.print_exc()
            if int(os.environ.get("RANK", "0")) == 0:
                print(json.dumps({"metric": "scored triples/sec/GPU (d=200)", "value": 0.0, "unit": "scored triples/s",
                                  "n_gpus": world, "error": f"{type(e).__name__}: {e}"}), flush=True)
            sys.exit(1)
        return
    run_single(args)


if __name__ == "__main__":
    main()
