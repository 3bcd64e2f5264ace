"""What a validation tick of the translation models costs (evaluate.TranslationPocket) at FB15k shape: E = 14,951,
R = 1,345, V = 50,000 validation rows with tools/transx_bench.py's Zipf relation column, the filter train + valid;
TransE / TransH / TransD at d = 100, TransR at 100 x 100, RotatE at d = 200, all L1, AdaGrad state where the model has it.

    python tools/translation_tick_bench.py [--calls 5] [--models transe,transh,transd,transr,rotate] [--rows 50000] [--out F]

Per model, one JSON line:
  tick_ms        one tick(): both sides' rank sweeps, ge_rank_metrics, ge_copy_if (the flag decides on the device; the
                 timed ticks are ties, so the copy kernel launches and returns at the flag)
  ranks_ms       the same two rank_counts calls alone, into the same buffers
                 (tick and ranks alternate in one process; each figure is the median of --calls, device events)
  copy_if_ms     ge_copy_if with the flag set over the model's whole state (one launch), and
  torch_copy_ms  torch.Tensor.copy_ of the same buffers (one launch a buffer); each the median of --calls batches of 10
  state_mb       the bytes of that state
The sweeps are evaluate.translation_ranks' own; there is no reference to beat.  The numbers are a record, not a gate."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphembeddings_amd import _lib  # noqa: E402
from graphembeddings_amd import evaluate as EV  # noqa: E402
from graphembeddings_amd import rotate as RO  # noqa: E402
from graphembeddings_amd import transr as TRm  # noqa: E402
from graphembeddings_amd import transx as X  # noqa: E402

E, R, D, T = 14951, 1345, 100, 483142


def fb15k_like(n_valid, seed=0):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, R + 1) ** 1.1
    r = rng.choice(R, size=T + n_valid, p=w / w.sum())
    tri = np.unique(np.stack([rng.integers(0, E, T + n_valid), rng.integers(0, E, T + n_valid), r], 1), axis=0)
    rng.shuffle(tri)
    return tri[:-n_valid], tri[-n_valid:]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternated(fns, calls):
    """Median ms of each function, the functions taking turns."""
    ts = [[] for _ in fns]
    for _ in range(calls):
        for k, fn in enumerate(fns):
            ts[k].append(event_ms(fn))
    return [float(np.median(t)) for t in ts]


def make(name):
    if name == "transr":
        return TRm.TransR(E, R, D, D, l1=True, seed=0)
    m = RO.RotatE(E, R, 2 * D, l1=True, seed=0) if name == "rotate" else X.TransX(name, E, R, D, l1=True, seed=0)
    m.enable_adagrad(0.1)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--models", default="transe,transh,transd,transr,rotate")
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("translation_tick_bench needs an MI355X: there is no CPU path")
    train, valid = fb15k_like(a.rows)
    known = np.concatenate([train, valid], 0)
    idx = {s: EV.KnownIndex(known, max(E, R), s, "cuda") for s in ("tail", "head")}
    S = lambda: torch.cuda.current_stream().cuda_stream
    lines = []
    for name in a.models.split(","):
        m = make(name)
        vp = EV.TranslationPocket(m, valid, idx)
        V = vp.V

        def tick():
            vp.tick(0)
            vp._pending.clear()                             # (timing only: the history slot is reused)

        def ranks():
            for k, side in enumerate(("tail", "head")):
                for (lo, hi), (off, rc) in zip(vp._chunks, vp._cells[side]):
                    m.rank_counts(vp.triples[lo:hi], cand_is_head=(side == "head"), known_off=off, known_rc=rc,
                                  out=(vp.n_before[k * V + lo:k * V + hi], vp.n_known_before[k * V + lo:k * V + hi],
                                       vp.true_dist[k * V + lo:k * V + hi]), workspace=vp._ws)

        tick()                                              # warm-up; this tick improves on 0 and fills the pocket
        ranks()
        torch.cuda.synchronize()
        tick_ms, ranks_ms = alternated([tick, ranks], a.calls)
        state = m._pocket_tensors()
        names = list(state)
        one = torch.ones(1, dtype=torch.int32, device="cuda")
        args = _lib.copy_if_args([state[n].data_ptr() for n in names], [vp.pocket[n].data_ptr() for n in names],
                                 [state[n].numel() for n in names])

        def gated():
            for _ in range(10):
                _lib.call("ge_copy_if", one.data_ptr(), *args, S())

        def plain():
            for _ in range(10):
                for n in names:
                    vp.pocket[n].copy_(state[n])

        gated()
        plain()
        torch.cuda.synchronize()
        copy_if_ms, torch_copy_ms = (t / 10 for t in alternated([gated, plain], a.calls))
        assert all(torch.equal(vp.pocket[n], state[n]) for n in names)
        line = {"model": name, "E": E, "R": R, "d": 2 * D if name == "rotate" else D, "l1": True, "validation_rows": V,
                "tick_ms": round(tick_ms, 3), "ranks_ms": round(ranks_ms, 3), "tick_minus_ranks_ms": round(tick_ms - ranks_ms, 3),
                "state_buffers": len(names), "state_mb": round(sum(4 * state[n].numel() for n in names) / 1e6, 2),
                "copy_if_ms": round(copy_if_ms, 4), "torch_copy_ms": round(torch_copy_ms, 4), "calls": a.calls}
        print(json.dumps(line))
        sys.stdout.flush()
        lines.append(line)
        del m, vp, state
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
