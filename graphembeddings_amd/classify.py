"""Triple classification: is (h, r, t) true?  Per-relation decision thresholds fitted from labelled validation
triples (ge_threshold_fit), and the decision with its confusion counts (ge_threshold_classify), for all six models.

Every model scores "lower is more plausible" -- the distance D of TransX.score / TransR.score, E = sigmoid(score) of
hole.evaluate_triples -- so one rule serves them: a triple is predicted true iff score <= thr[relation]; a NaN score
is never accepted.  This is the fitted form of the reference's inference gate (holE.py:438 accepts a prediction when
min_loss < --infer_threshold, one global number the user has to guess).

The fit (include/ge_hip.h): per relation, over the labelled scores sorted ascending with NaN last, the cut p that
maximises  #positives in [0,p) + #negatives in [p,m), equal scores never separated, ties to the smallest p; thr_lo
is the last accepted score (-inf: none), thr_hi the first rejected one (+inf: none).  `Thresholds.resolve` turns the
pair into one number.  There is no CPU path for the fit or the decision; `resolve` is tensor arithmetic and runs
wherever its tensors live.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from . import hole as H

FIT_TILE = 2048         # elements per workgroup of ge_threshold_fit (GE_THRESHOLD_FIT_TILE in include/ge_hip.h)
CONFUSION_LDS_SEGMENTS = 2048   # up to here ge_threshold_classify counts the confusion table in LDS first (kHistMax / 4)
MODES = ("mid", "lo")
FALLBACKS = ("global", "none")
TSV_HEADER = ("relation", "thr", "thr_lo", "thr_hi", "n_pos", "n_neg", "valid_correct", "source")
_FIELDS = ("thr_lo", "thr_hi", "best_correct", "n_pos", "n_neg")


def _resolve_pair(lo: torch.Tensor, hi: torch.Tensor, mode: str) -> torch.Tensor:
    if mode == "lo":
        return lo.clone()
    mid = (0.5 * (lo.double() + hi.double())).float()
    mid = torch.where(mid >= hi, lo, mid)               # adjacent floats: the midpoint rounds up to hi
    mid = torch.where(torch.isposinf(hi), hi, mid)
    return torch.where(torch.isneginf(lo), lo, mid)


@dataclass
class Thresholds:
    """The fit's outputs per relation ([n_rel] tensors) and for the one global segment "all triples" ([1] tensors,
    global_*).  thr_lo / thr_hi float32, the counts int32."""
    thr_lo: torch.Tensor
    thr_hi: torch.Tensor
    best_correct: torch.Tensor
    n_pos: torch.Tensor
    n_neg: torch.Tensor
    global_thr_lo: torch.Tensor
    global_thr_hi: torch.Tensor
    global_best_correct: torch.Tensor
    global_n_pos: torch.Tensor
    global_n_neg: torch.Tensor

    @property
    def n_rel(self) -> int:
        return int(self.thr_lo.numel())

    def uses_global(self, fallback: str = "global") -> torch.Tensor:
        """bool [n_rel]: the relations that take the global threshold (no positive or no negative to fit on)."""
        if fallback not in FALLBACKS:
            raise ValueError(f"fallback must be one of {FALLBACKS}, got {fallback!r}")
        degenerate = (self.n_pos == 0) | (self.n_neg == 0)
        return degenerate if fallback == "global" else torch.zeros_like(degenerate)

    def resolve(self, mode: str = "mid", fallback: str = "global") -> torch.Tensor:
        """One threshold per relation, float32 [n_rel].  "lo": thr_lo.  "mid": float32(0.5 * (float64(lo) +
        float64(hi))), replaced by lo when that rounds to >= hi; an infinite end wins (-inf first).  A relation with
        n_pos == 0 or n_neg == 0 takes the global threshold, resolved the same way (fallback="none": its own)."""
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        own = _resolve_pair(self.thr_lo, self.thr_hi, mode)
        glob = _resolve_pair(self.global_thr_lo, self.global_thr_hi, mode)
        return torch.where(self.uses_global(fallback), glob.expand_as(own), own)

    def cpu(self) -> "Thresholds":
        return Thresholds(**{k: v.cpu() for k, v in self.__dict__.items()})

    def save(self, path: str, mode: str = "mid", fallback: str = "global") -> None:
        """TSV: relation, thr, thr_lo, thr_hi, n_pos, n_neg, valid_correct, source (own | global); the last row is the
        global segment (relation `global`).  Floats are written with nine significant digits: float32 exactly."""
        t = self.cpu()
        thr, src = t.resolve(mode, fallback), t.uses_global(fallback)
        g = _resolve_pair(t.global_thr_lo, t.global_thr_hi, mode)
        f = lambda x: "%.9g" % float(x)
        with open(path, "w") as out:
            out.write("\t".join(TSV_HEADER) + "\n")
            for r in range(t.n_rel):
                out.write("\t".join([str(r), f(thr[r]), f(t.thr_lo[r]), f(t.thr_hi[r]), str(int(t.n_pos[r])),
                                     str(int(t.n_neg[r])), str(int(t.best_correct[r])),
                                     "global" if bool(src[r]) else "own"]) + "\n")
            out.write("\t".join(["global", f(g[0]), f(t.global_thr_lo[0]), f(t.global_thr_hi[0]),
                                 str(int(t.global_n_pos[0])), str(int(t.global_n_neg[0])),
                                 str(int(t.global_best_correct[0])), "global"]) + "\n")


def load_thresholds(path: str):
    """(Thresholds on the CPU, thr float32 [n_rel] as saved) of a file Thresholds.save wrote."""
    with open(path) as f:
        rows = [line.rstrip("\n").split("\t") for line in f if line.strip()]
    if not rows or tuple(rows[0]) != TSV_HEADER:
        raise ValueError(f"{path}: not a thresholds file (header {rows[0] if rows else None})")
    body = rows[1:]
    if len(body) < 2 or body[-1][0] != "global" or any(len(r) != len(TSV_HEADER) for r in body):
        raise ValueError(f"{path}: expected one row per relation and a final `global` row of {len(TSV_HEADER)} columns")
    if [r[0] for r in body[:-1]] != [str(i) for i in range(len(body) - 1)]:
        raise ValueError(f"{path}: relation rows must be numbered 0 .. n_rel - 1 in order")
    fl = lambda rs, c: torch.tensor([float(r[c]) for r in rs], dtype=torch.float64).float()
    it = lambda rs, c: torch.tensor([int(r[c]) for r in rs], dtype=torch.int32)
    rel, g = body[:-1], body[-1:]
    t = Thresholds(fl(rel, 2), fl(rel, 3), it(rel, 6), it(rel, 4), it(rel, 5),
                   fl(g, 2), fl(g, 3), it(g, 6), it(g, 4), it(g, 5))
    return t, fl(rel, 1)


def _vector(t, name: str, M: Optional[int] = None) -> torch.Tensor:
    H._need_cuda(t, name)
    if t.dim() != 1 or (M is not None and t.shape[0] != M):
        raise ValueError(f"{name} must be a 1-D tensor" + (f" of {M} elements" if M is not None else ""))
    return t


def _checked(scores, relations, labels, n_rel: int):
    """(score float32, relation int32, label uint8 or None) contiguous device vectors, or ValueError."""
    s = _vector(scores, "scores")
    if s.dtype != torch.float32:
        raise ValueError("scores must be float32")
    M = s.shape[0]
    r = _vector(relations, "relations", M)
    if r.dtype not in (torch.int32, torch.int64):
        raise ValueError("relations must be int32 or int64")
    if n_rel < 1 or n_rel >= 2 ** 31 - 1:
        raise ValueError(f"n_rel must lie in [1, 2^31 - 2], got {n_rel}")
    if M and (int(r.min()) < 0 or int(r.max()) >= n_rel):
        raise ValueError(f"relations hold an id outside [0, {n_rel})")
    if M and bool(torch.isneginf(s).any()):
        raise ValueError("scores hold -inf: no threshold can reject it")
    lab = None
    if labels is not None:
        lab = _vector(labels, "labels", M)
        if lab.dtype.is_floating_point or lab.dtype.is_complex:
            raise ValueError("labels must be integers (0 or 1) or bool")
        if M and lab.dtype != torch.bool and (int(lab.min()) < 0 or int(lab.max()) > 1):
            raise ValueError("labels must be 0 or 1")
        lab = lab.to(torch.uint8).contiguous()
    return s.contiguous(), r.to(torch.int32).contiguous(), lab


def _sort_key(score: torch.Tensor, seg: torch.Tensor) -> torch.Tensor:
    """int64 key whose ascending order is (seg, score ascending, NaN last): seg << 32 | the float's bits made monotone."""
    bits = score.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    mono = torch.where(bits >= 0x80000000, 0xFFFFFFFF - bits, bits + 0x80000000)
    mono = torch.where(torch.isnan(score), torch.full_like(mono, 0xFFFFFFFF), mono)
    return (seg.to(torch.int64) << 32) | mono


def fit_raw(score: torch.Tensor, seg: torch.Tensor, label: torch.Tensor, n_seg: int) -> Dict[str, torch.Tensor]:
    """ge_threshold_fit on device vectors that are ALREADY ordered by (seg, score ascending, NaN last): the five
    [n_seg] outputs by name."""
    M, dev = score.shape[0], score.device
    lib = _lib.load()
    need = int(lib.ge_threshold_fit_workspace_bytes(M, n_seg))
    if need == 0:
        raise ValueError(f"ge_threshold_fit takes 1 <= M <= 2^31 - 1 and n_seg >= 1, got M = {M}, n_seg = {n_seg}")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = {k: torch.empty(n_seg, dtype=torch.float32 if k.startswith("thr") else torch.int32, device=dev) for k in _FIELDS}
    _lib.call("ge_threshold_fit", score.data_ptr(), seg.data_ptr(), label.data_ptr(), M, n_seg,
              *(out[k].data_ptr() for k in _FIELDS), ws.data_ptr(), ws.numel(), H._stream())
    return out


def fit_thresholds(scores: torch.Tensor, relations: torch.Tensor, labels: torch.Tensor, n_rel: int) -> Thresholds:
    """Fit one threshold per relation and the global one from labelled scores (device vectors of one length M >= 1;
    labels 0 / 1).  One sort and one ge_threshold_fit call: every element is entered twice, once under its relation
    and once under segment n_rel, "all triples".  Ids, labels outside {0, 1} and -inf scores raise ValueError."""
    n_rel = int(n_rel)
    if labels is None:
        raise ValueError("labels are required")
    s, r, lab = _checked(scores, relations, labels, n_rel)
    M = s.shape[0]
    if M < 1 or 2 * M > 2 ** 31 - 1:
        raise ValueError(f"fit_thresholds takes 1 <= M < 2^30 labelled scores, got {M}")
    seg2 = torch.cat([r, torch.full_like(r, n_rel)])
    order = torch.sort(_sort_key(torch.cat([s, s]), seg2)).indices
    src = order % M
    out = fit_raw(s[src].contiguous(), seg2[order].contiguous(), lab[src].contiguous(), n_rel + 1)
    return Thresholds(*(out[k][:n_rel] for k in _FIELDS), *(out[k][n_rel:] for k in _FIELDS))


def classify(scores: torch.Tensor, relations: torch.Tensor, thr: torch.Tensor, labels: Optional[torch.Tensor] = None):
    """pred bool [M] = scores <= thr[relations] (False for a NaN).  With labels (0 / 1): (pred, stats), stats =
    {"accuracy", "macro_accuracy" (mean over the relations that have triples here), "confusion" (int32 [n_rel, 4] =
    tp, fp, tn, fn, on the CPU), "n"}."""
    H._need_cuda(thr, "thr")
    if thr.dim() != 1 or thr.dtype != torch.float32 or thr.numel() < 1:
        raise ValueError("thr must be a float32 [n_rel] tensor")
    n_rel = int(thr.numel())
    s, r, lab = _checked(scores, relations, labels, n_rel)
    M, dev = s.shape[0], s.device
    pred = torch.empty(M, dtype=torch.uint8, device=dev)
    conf = torch.empty(n_rel, 4, dtype=torch.int32, device=dev) if lab is not None else None
    thr = thr.contiguous()
    _lib.call("ge_threshold_classify", s.data_ptr(), r.data_ptr(), None if lab is None else lab.data_ptr(), M, n_rel,
              thr.data_ptr(), pred.data_ptr(), None if conf is None else conf.data_ptr(), H._stream())
    if lab is None:
        return pred.bool()
    return pred.bool(), confusion_stats(conf.cpu())


def confusion_stats(conf: torch.Tensor) -> Dict[str, object]:
    c = conf.to(torch.int64)
    tot, right = c.sum(1), c[:, 0] + c[:, 2]
    have = tot > 0
    n = int(tot.sum())
    return {"accuracy": float(right.sum()) / n if n else 0.0,
            "macro_accuracy": float((right[have].double() / tot[have].double()).mean()) if bool(have.any()) else 0.0,
            "confusion": conf, "n": n}


@dataclass
class TableModel:
    """A ComplEx / HolE table for triple_classification: the shared table (relations are rows [0, relation_count)),
    hole.TypeTables for the type-safe sampler, and the score: "complex", "hole" or "hole_spectral"."""
    embeddings: torch.Tensor
    relation_count: int
    type_tables: Optional[H.TypeTables] = None
    model: str = "complex"


def _as_model(model):
    if isinstance(model, (tuple, list)):
        if len(model) != 4:
            raise ValueError("a table model is (embeddings, relation_count, type_tables, model name)")
        model = TableModel(*model)
    if isinstance(model, TableModel):
        if model.model not in ("complex", "hole", "hole_spectral"):
            raise ValueError(f"model must be complex, hole or hole_spectral, got {model.model!r}")
        H._table(model.embeddings)
        if not 1 <= int(model.relation_count) < model.embeddings.shape[0]:
            raise ValueError("relation_count must lie in [1, table rows)")
    elif not (hasattr(model, "score") and hasattr(model, "n_ent") and hasattr(model, "n_rel")):
        raise ValueError("model must be a TransX / TransR model or a TableModel")
    return model


def _triples_of(x, name: str, model, dev) -> Optional[torch.Tensor]:
    """[n,3] (h, t, r) int32 device rows, ids checked against the model on the host."""
    if x is None:
        return None
    a = np.asarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x)
    if a.ndim != 2 or a.shape[1] != 3 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name} must be an integer [n, 3] (head, tail, relation) array")
    a = a.astype(np.int64)
    if len(a):
        if isinstance(model, TableModel):
            R, N = int(model.relation_count), int(model.embeddings.shape[0])
            ok = a[:, :2].min() >= R and a[:, :2].max() < N and a[:, 2].min() >= 0 and a[:, 2].max() < R
        else:
            ok = (a[:, :2].min() >= 0 and a[:, :2].max() < model.n_ent and a[:, 2].min() >= 0
                  and a[:, 2].max() < model.n_rel)
        if not ok:
            raise ValueError(f"{name} holds an id outside the model's tables")
    return torch.as_tensor(a.astype(np.int32)).to(dev).contiguous()


def _scores(model, tri: torch.Tensor) -> torch.Tensor:
    if isinstance(model, TableModel):
        return H.evaluate_triples(tri, model.embeddings, model=model.model).view(-1)
    return model.score(tri)


def draw_negatives(model, pos: torch.Tensor, known, seed: int, step: int):
    """One negative per positive from the model's own sampler at Philox (seed, step); (negatives, dropped count).
    Translation models: the filtered Bernoulli sampler over `known` (never a known triple).  ComplEx / HolE: the
    type-safe hole.corrupt_batch with a coin per row; a draw that is in `known`, or has no replacement (an entity of
    unknown type), is dropped."""
    if known is None:
        raise ValueError("drawing negatives needs the known triples")
    kn = np.asarray(known.cpu().numpy() if isinstance(known, torch.Tensor) else known, dtype=np.int64).reshape(-1, 3)
    if isinstance(model, TableModel):
        if model.type_tables is None:
            raise ValueError("drawing negatives for a table model needs its type tables")
        neg = H.corrupt_batch(model.type_tables, int(model.relation_count), pos, seed=seed, step=step,
                              mode=H.CORRUPT_ROW_COIN)
        N = int(model.embeddings.shape[0])
        pack = lambda t: (t[:, 0].to(torch.int64) * N + t[:, 1].to(torch.int64)) * N + t[:, 2].to(torch.int64)
        kkey = torch.as_tensor((kn[:, 0] * N + kn[:, 1]) * N + kn[:, 2]).to(pos.device)
        keep = (neg.min(1).values >= 0) & ~torch.isin(pack(neg), kkey)
        return neg[keep].contiguous(), int((~keep).sum())
    sampler = H.BernoulliSampler(kn, model.n_rel, model.n_ent, device=pos.device, ent_lo=0)
    return sampler.corrupt(pos, seed=seed, step=step), 0


VALID_STEP, TEST_STEP = 0, 1            # the Philox steps of the two draws


def triple_classification(model, valid_pos, test_pos, valid_neg=None, test_neg=None, known=None, seed: int = 0,
                          mode: str = "mid", fallback: str = "global") -> Dict[str, object]:
    """Fit per-relation thresholds on the validation split and classify the test split.

    model: a TransX / TransR model, or a TableModel (or the tuple (embeddings, relation_count, type_tables, name)) for
    ComplEx / HolE.  *_pos / *_neg: [n,3] (h, t, r) rows.  Missing negatives are drawn one per positive by
    draw_negatives (valid at Philox step 0, test at step 1 of `seed`) and need `known`.
    Returns accuracy, macro_accuracy, confusion, n (test); valid_accuracy, n_valid; dropped_valid_neg,
    dropped_test_neg; thresholds (Thresholds), thr (the resolved float32 [n_rel]); valid_neg, test_neg (device rows)."""
    model = _as_model(model)
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    table = isinstance(model, TableModel)
    dev = model.embeddings.device if table else model.tables["ent"].device
    n_rel = int(model.relation_count) if table else int(model.n_rel)
    splits, dropped = {}, {}
    for name, pos, neg, step in (("valid", valid_pos, valid_neg, VALID_STEP), ("test", test_pos, test_neg, TEST_STEP)):
        p = _triples_of(pos, f"{name}_pos", model, dev)
        if p is None or p.shape[0] == 0:
            raise ValueError(f"{name}_pos must hold at least one triple")
        n, dropped[name] = _triples_of(neg, f"{name}_neg", model, dev), 0
        if n is None:
            n, dropped[name] = draw_negatives(model, p, known, int(seed), step)
        tri = torch.cat([p, n], 0)
        lab = torch.cat([torch.ones(p.shape[0], dtype=torch.uint8, device=dev),
                         torch.zeros(n.shape[0], dtype=torch.uint8, device=dev)])
        splits[name] = (tri, lab, n)
    vtri, vlab, vneg = splits["valid"]
    ttri, tlab, tneg = splits["test"]
    th = fit_thresholds(_scores(model, vtri), vtri[:, 2], vlab, n_rel)
    thr = th.resolve(mode, fallback)
    _, vstats = classify(_scores(model, vtri), vtri[:, 2], thr, vlab)
    _, stats = classify(_scores(model, ttri), ttri[:, 2], thr, tlab)
    return {"accuracy": stats["accuracy"], "macro_accuracy": stats["macro_accuracy"], "confusion": stats["confusion"],
            "n": stats["n"], "valid_accuracy": vstats["accuracy"], "n_valid": vstats["n"],
            "dropped_valid_neg": dropped["valid"], "dropped_test_neg": dropped["test"], "thresholds": th, "thr": thr,
            "valid_neg": vneg, "test_neg": tneg, "mode": mode, "seed": int(seed)}


def report(res: Dict[str, object]) -> Dict[str, object]:
    """The JSON form of a triple_classification result."""
    out = {k: res[k] for k in ("accuracy", "macro_accuracy", "n", "valid_accuracy", "n_valid", "dropped_valid_neg",
                               "dropped_test_neg", "mode", "seed")}
    out["confusion"] = [[int(x) for x in row] for row in res["confusion"].tolist()]
    out["relations_on_global_threshold"] = int(res["thresholds"].uses_global().sum())
    return out


def summary_line(res: Dict[str, object]) -> str:
    return ("triple classification: accuracy {accuracy:.4f} (macro {macro_accuracy:.4f}) on {n} test triples; "
            "validation accuracy {valid_accuracy:.4f} on {n_valid}".format(**res))


def write_results(res: Dict[str, object], json_path: str, tsv_path: str) -> None:
    """<model>_classify.json and <model>_thresholds.tsv of the drivers."""
    import json
    with open(json_path, "w") as f:
        json.dump(report(res), f, indent=1, sort_keys=True)
    res["thresholds"].save(tsv_path, mode=res["mode"])
