"""TransE / TransH / TransD (transE.py, transH.py, transD.py) on the MI355X: tables, batch scoring, the
margin-hinge SGD step and the native multi-step loop of include/ge_hip.h's ge_transx_* entry points.

Reference semantics: separate `ent [E,d]` / `rel [R,d]` tables (TransH adds `normal_vector [R,d]`, TransD adds
`ent_transfer [E,d]` and `rel_transfer [R,d]`), every table xavier_initializer(uniform=False) for its own shape,
D = sum |h_p + r - t_p| (L1) or sum (h_p + r - t_p)^2, loss = sum_batch max(D+ - D- + margin, 0), plain SGD
(tf.train.GradientDescentOptimizer) on every table, or TF1's AdagradOptimizer in its place (enable_adagrad,
adagrad_step, trainer(optimizer="adagrad")).  There is no CPU path: every call runs a HIP kernel.

The self-adversarial negative-sampling loss of Sun et al. 2019 (adv_loss / adv_step / adv_adagrad_step,
trainer(loss="self_adversarial"); ge_transx_adv_*): K negatives per positive, all on one side of it, weighted by a
softmax over their own scores that is not differentiated.  What it shares with RotatE (the batch checks, the
hyperparameter checks, AdvTrainer) lives here, parametrised by the model's PREFIX; rotate.py re-exports it.
"""
from __future__ import annotations

import math
import os
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .hole import BernoulliSampler, _need_cuda, _stream, init_embeddings

MODELS = {"transe": 0, "transh": 1, "transd": 2}
# the extra tables of each model, in the order they are stored
EXTRA_TABLES = {"transe": (), "transh": ("normal_vector",), "transd": ("ent_transfer", "rel_transfer")}
MAX_NEGATIVES = 1024            # ge_rotate_adv_max_negatives() and ge_transx_adv_max_negatives()
LOSSES = ("hinge", "self_adversarial")


def _count(path: str) -> int:
    """The leading count of a *2id.txt file, read the way init.cpp:53-62 reads it (one `%d`, the rest unread)."""
    with open(path) as f:
        tok = f.read().split(maxsplit=1)
    if not tok:
        raise ValueError(f"{path}: empty file, expected a leading count")
    try:
        n = int(tok[0])
    except ValueError:
        raise ValueError(f"{path}: leading count {tok[0]!r} is not an integer") from None
    if n <= 0:
        raise ValueError(f"{path}: count {n} must be positive")
    return n


def ids_outside(tri: np.ndarray, n_ent: int, n_rel: int) -> Optional[str]:
    """"entity" or "relation" when an id of the [n,3] (h, t, r) rows lies outside [0, n_ent) / [0, n_rel), else None."""
    if len(tri) and (tri[:, :2].min() < 0 or tri[:, :2].max() >= n_ent):
        return "entity"
    if len(tri) and (tri[:, 2].min() < 0 or tri[:, 2].max() >= n_rel):
        return "relation"
    return None


def read_kg(data_dir: str):
    """(entity_total, relation_total, triples int32 [T,3] as (h, t, r)) from relation2id.txt, entity2id.txt and
    triple2id.txt (init.cpp:47-86).  Each file begins with its count; the triples follow as `h t r` rows and are
    read until the input ends, as init.cpp's `while (fscanf(...) == 1)` does.  Where init.cpp would read garbage or
    write past its buffers (a partial last triple, more triples than declared, an id out of range) this raises."""
    R = _count(os.path.join(data_dir, "relation2id.txt"))
    E = _count(os.path.join(data_dir, "entity2id.txt"))
    return E, R, read_triples(os.path.join(data_dir, "triple2id.txt"), E, R)


def read_triples(path: str, n_ent: int, n_rel: int) -> np.ndarray:
    """int32 [T,3] (h, t, r) rows of one *2id.txt triple file (triple2id.txt, or a test / valid split in the same
    format): a leading count, then `h t r` rows until the input ends, with read_kg's checks."""
    E, R = n_ent, n_rel
    with open(path) as f:
        tok = f.read().split()
    if not tok:
        raise ValueError(f"{path}: empty file, expected a leading count")
    try:
        vals = np.array([int(x) for x in tok], dtype=np.int64)
    except ValueError as e:
        raise ValueError(f"{path}: non-integer token ({e})") from None
    declared, body = int(vals[0]), vals[1:]
    if body.size % 3:
        raise ValueError(f"{path}: {body.size} ids after the count is not a whole number of (h, t, r) triples")
    tri = body.reshape(-1, 3)
    if len(tri) == 0:
        raise ValueError(f"{path}: no triples")
    if len(tri) > declared:
        raise ValueError(f"{path}: {len(tri)} triples but the file declares {declared}")
    bad = ids_outside(tri, E, R)
    if bad:
        raise ValueError(f"{path}: {bad} id outside [0, {E if bad == 'entity' else R})")
    return tri.astype(np.int32)




def topk_max_k() -> int:
    """Largest k the fused top-k of the translation models (ge_transx_topk / ge_transr_topk) takes."""
    return int(_lib.load().ge_transx_topk_max_k())


def _pairs(t: torch.Tensor, name: str) -> torch.Tensor:
    _need_cuda(t, name)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} must have shape [B, 3] (head, tail, relation)")
    return t.to(torch.int32).contiguous()


class Trainer:
    """The reference's training loop (getBatch + train_step, transE.py:109-115) as one native call per run():
    each step draws `batch_size` positives uniformly with replacement from `triples` and corrupts each with the
    filtered Bernoulli rule (ent_lo = 0), then takes the model's step.  Step s of the run uses the Philox counter
    (seed, s): ge_transx_draw_batch(.., seed, s, ..) reproduces any step's batch.  `optimizer` ("sgd", or "adagrad"
    for a TransX model: _Model.trainer sets it) selects the step; the draws are the same."""
    optimizer = "sgd"

    def __init__(self, model: TransX, triples, batch_size: int, *, margin: float = 1.0, learning_rate: float = 0.001,
                 seed: int = 0):
        tri = np.asarray(triples.cpu().numpy() if isinstance(triples, torch.Tensor) else triples, dtype=np.int64)
        if tri.ndim != 2 or tri.shape[1] != 3 or len(tri) == 0:
            raise ValueError("triples must be a non-empty [T, 3] (h, t, r) array")
        if ids_outside(tri, model.n_ent, model.n_rel):
            raise ValueError("triples hold an id outside the model's tables")
        if batch_size <= 0:
            raise ValueError("batch_size must be positive")
        dev = model.tables["ent"].device
        self.model, self.B, self.margin, self.lr, self.seed = model, int(batch_size), float(margin), float(learning_rate), int(seed)
        self.triples = torch.as_tensor(tri.astype(np.int32)).to(dev).contiguous()
        self.sampler = BernoulliSampler(tri, model.n_rel, model.n_ent, device=dev, ent_lo=0)
        self.step_count = 0

    def _sampler_args(self):
        """The triples and sampler arguments of a *_train_steps call, from `triples` to `tail_threshold`."""
        s = self.sampler
        return (self.triples.data_ptr(), self.triples.shape[0], s.bh_key.data_ptr(), s.bh_ent.data_ptr(),
                s.bt_key.data_ptr(), s.bt_ent.data_ptr(), s.n_known, s.tail_threshold.data_ptr())

    def draw(self, step: int):
        """The (pos, neg) batch the loop uses at `step`."""
        pos = torch.empty(self.B, 3, dtype=torch.int32, device=self.triples.device)
        neg = torch.empty_like(pos)
        a = self._sampler_args()                        # ge_transx_draw_batch takes B after (triples, T)
        _lib.call("ge_transx_draw_batch", *a[:2], self.B, *a[2:], self.sampler.n_rel, self.sampler.n_ent,
                  self.seed & (2**64 - 1), int(step) & (2**64 - 1), pos.data_ptr(), neg.data_ptr(), _stream())
        return pos, neg

    def run(self, n: int) -> torch.Tensor:
        """n steps in one call (the model's _train_steps); returns the [n] per-step batch losses (device)."""
        losses = torch.empty(max(int(n), 0), dtype=torch.float32, device=self.triples.device)
        if n <= 0:
            return losses
        self.model._train_steps(self, int(n), losses, self.model.workspace(self.B))
        self.step_count += int(n)
        return losses


def check_adv_hyperparameters(negatives, adversarial_temperature, margin) -> None:
    """K in [1, MAX_NEGATIVES], alpha finite and >= 0, margin finite: ValueError otherwise (no device work)."""
    if isinstance(negatives, bool) or not isinstance(negatives, (int, np.integer)) or not 1 <= negatives <= MAX_NEGATIVES:
        raise ValueError(f"negatives must be an integer in [1, {MAX_NEGATIVES}], got {negatives!r}")
    alpha = float(adversarial_temperature)
    if not math.isfinite(alpha) or alpha < 0:
        raise ValueError(f"adversarial_temperature must be finite and >= 0, got {adversarial_temperature!r}")
    if not math.isfinite(float(margin)):
        raise ValueError(f"margin must be finite, got {margin!r}")


class AdvTrainer(Trainer):
    """The native loop of the self-adversarial loss: the Trainer's positives and sides for the same seed, K filtered
    negatives per positive (ge_rotate_adv_draw_batch, which reads no table and serves every model), one
    <PREFIX>_adv_train_steps[_adagrad] call per run().  Its workspace depends on K as well as on B and is cached here,
    not in the model."""

    def __init__(self, model, triples, batch_size: int, *, negatives: int, adversarial_temperature: float,
                 margin: float = 1.0, learning_rate: float = 0.001, seed: int = 0):
        check_adv_hyperparameters(negatives, adversarial_temperature, margin)
        super().__init__(model, triples, batch_size, margin=margin, learning_rate=learning_rate, seed=seed)
        self.K, self.alpha = int(negatives), float(adversarial_temperature)
        self._ws = None

    def workspace(self) -> torch.Tensor:
        if self._ws is None:
            self._ws = self.model._adv_workspace(self.B, self.K)
        return self._ws

    def draw(self, step: int):
        """The (pos [B,3], side [B], neg_ent [B,K]) batch the loop uses at `step`."""
        dev = self.triples.device
        pos = torch.empty(self.B, 3, dtype=torch.int32, device=dev)
        side = torch.empty(self.B, dtype=torch.int32, device=dev)
        neg_ent = torch.empty(self.B, self.K, dtype=torch.int32, device=dev)
        a = self._sampler_args()
        _lib.call("ge_rotate_adv_draw_batch", *a[:2], self.B, *a[2:], self.sampler.n_rel, self.sampler.n_ent,
                  self.seed & (2**64 - 1), int(step) & (2**64 - 1), self.K, pos.data_ptr(), side.data_ptr(),
                  neg_ent.data_ptr(), _stream())
        return pos, side, neg_ent

    def run(self, n: int) -> torch.Tensor:
        """n steps in one native call; returns the [n] per-step batch losses (device)."""
        losses = torch.empty(max(int(n), 0), dtype=torch.float32, device=self.triples.device)
        if n <= 0:
            return losses
        m, ws = self.model, self.workspace()
        ada = self.optimizer == "adagrad"
        _lib.call(m.PREFIX + ("_adv_train_steps_adagrad" if ada else "_adv_train_steps"),
                  *(m._adagrad_ptrs() if ada else m._ptrs()), *self._sampler_args(), self.seed & (2**64 - 1),
                  self.step_count, int(n), self.B, self.K, self.margin, self.alpha, self.lr, losses.data_ptr(),
                  ws.data_ptr(), ws.numel(), _stream())
        self.step_count += int(n)
        return losses


class _Model:
    """What TransX and TransR share: named tables, the cached step workspace, scoring, ranks, top-k prediction, the
    Trainer and the state-dict checks.  A subclass sets PREFIX (its ge_* entry points), _trainer and _state_tensors(), and supplies
    _ptrs() (the table arguments every entry takes), _ws_bytes(kind, B, *extra) and _train_steps(trainer, n, losses, ws)."""
    PREFIX = ""
    _trainer = Trainer

    def _init_tables(self, shapes, seed: Optional[int], device) -> None:
        """One table per (name, shape), drawn with seed base + k for the k-th (None: unseeded)."""
        base = None if seed is None else int(seed)
        self.tables: Dict[str, torch.Tensor] = {
            name: init_embeddings(*shape, device=device, seed=None if base is None else base + k)
            for k, (name, shape) in enumerate(shapes)}
        self._ws: Optional[torch.Tensor] = None
        self._ws_B = -1
        self._loss = torch.empty(1, dtype=torch.float32, device=self.tables["ent"].device)

    def workspace(self, B: int) -> torch.Tensor:
        if self._ws is None or self._ws_B != B:
            nbytes = self._ws_bytes("step", int(B))
            if nbytes == 0:
                raise RuntimeError(f"{self.PREFIX}_step_workspace_bytes failed")
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.tables["ent"].device)
            self._ws_B = B
        return self._ws

    def score(self, triples: torch.Tensor) -> torch.Tensor:
        """D of every (h, t, r) row, [B] fp32 (NaN where an id is out of range)."""
        tb = _pairs(triples, "triples")
        out = torch.empty(tb.shape[0], dtype=torch.float32, device=tb.device)
        _lib.call(self.PREFIX + "_score", *self._ptrs(), tb.data_ptr(), tb.shape[0], out.data_ptr(), _stream())
        return out

    def _step_batch(self, pos: torch.Tensor, neg: torch.Tensor):
        """(pos, neg, workspace) of one step, the pairs checked."""
        pb, nb = _pairs(pos, "pos"), _pairs(neg, "neg")
        if pb.shape != nb.shape or pb.shape[0] == 0:
            raise ValueError("pos and neg must be non-empty and of the same shape")
        return pb, nb, self.workspace(pb.shape[0])

    def _sets_args(self, B: int, row_set, mask):
        """(row_set pointer, mask pointer, n_sets) of a masked sweep over every entity, the tensors checked; () without
        sets.  mask: int32 / uint32-as-int32 [n_sets, ge_candidate_mask_words(n_ent)], row_set: int32 [B] (-1:
        unrestricted), both on the device and kept alive by the caller's frame."""
        if row_set is None and mask is None:
            return ()
        if row_set is None or mask is None:
            raise ValueError("row_set and mask come together")
        _need_cuda(row_set, "row_set")
        _need_cuda(mask, "mask")
        words = int(_lib.load().ge_candidate_mask_words(self.n_ent))
        if mask.dtype != torch.int32 or mask.dim() != 2 or mask.shape[0] < 1 or mask.shape[1] != words or not mask.is_contiguous():
            raise ValueError(f"mask must be a contiguous int32 [n_sets, {words}] tensor (sets built for arange(n_ent))")
        if row_set.dtype != torch.int32 or row_set.dim() != 1 or row_set.numel() != B or not row_set.is_contiguous():
            raise ValueError(f"row_set must be a contiguous int32 [{B}] tensor")
        return (row_set.data_ptr(), mask.data_ptr(), int(mask.shape[0]))

    def rank_counts(self, triples: torch.Tensor, cand_is_head: bool = False, known_off: torch.Tensor = None,
                    known_rc: torch.Tensor = None, return_scores: bool = False, row_set: torch.Tensor = None,
                    mask: torch.Tensor = None, out=None, workspace: torch.Tensor = None):
        """ge_transx_rank / ge_transr_rank on the [B,3] rows as given: (n_before, n_known_before, true_dist) device
        tensors, plus the [B, n_ent] distances with return_scores (tests).  known_off / known_rc: ge_known_cells'
        lists for these rows with pos_of = the identity (None: unfiltered).  Rows with an id out of range get -1
        counts.  row_set / mask (int32 [B]; int32 [n_sets, words], CandidateSets.mask for arange(n_ent)): only the
        entities admissible in the row's set are counted (ge_transx_rank_masked / ge_transr_rank_masked, which store no
        distances: not with return_scores); a set index outside [-1, n_sets) gives the row -1 counts.
        out = (n_before, n_known_before, true_dist): contiguous int32 / int32 / float32 [B] device tensors (views of a
        caller's buffers) to write and return instead of new ones; workspace: a uint8 device tensor of at least the
        rank workspace's size for B rows, used instead of a new one.  With both (int32 contiguous rows, no
        return_scores) the call allocates nothing."""
        tb = _pairs(triples, "triples")
        B, dev = tb.shape[0], tb.device
        sets = self._sets_args(B, row_set, mask)
        if sets and return_scores:
            raise ValueError("the masked rank sweep stores no distances: return_scores needs row_set = mask = None")
        ws_bytes = self._ws_bytes("rank", max(B, 1))
        if (known_off is None) != (known_rc is None):
            raise ValueError("known_off and known_rc come together")
        if ws_bytes == 0:
            raise RuntimeError(f"{self.PREFIX}_rank_workspace_bytes failed")
        if out is None:
            nb = torch.empty(B, dtype=torch.int32, device=dev)
            nk = torch.empty(B, dtype=torch.int32, device=dev)
            td = torch.empty(B, dtype=torch.float32, device=dev)
        else:
            nb, nk, td = out
            for t, dt, name in ((nb, torch.int32, "n_before"), (nk, torch.int32, "n_known_before"), (td, torch.float32, "true_dist")):
                _need_cuda(t, "out " + name)
                if t.dtype != dt or t.dim() != 1 or t.numel() != B or not t.is_contiguous():
                    raise ValueError(f"out {name} must be a contiguous {dt} [{B}] tensor")
        sc = torch.empty(B, self.n_ent, dtype=torch.float32, device=dev) if return_scores else None
        if workspace is None:
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        else:
            ws = workspace
            _need_cuda(ws, "workspace")
            if ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < ws_bytes:
                raise ValueError(f"workspace must be a contiguous uint8 tensor of at least {ws_bytes} bytes")
        p = lambda t: None if t is None else t.data_ptr()
        if sets:
            _lib.call(self.PREFIX + "_rank_masked", *self._ptrs(), tb.data_ptr(), B, int(bool(cand_is_head)),
                      p(known_off), p(known_rc), *sets, nb.data_ptr(), nk.data_ptr(), td.data_ptr(), ws.data_ptr(),
                      ws.numel(), _stream())
            return nb, nk, td
        _lib.call(self.PREFIX + "_rank", *self._ptrs(), tb.data_ptr(), B, int(bool(cand_is_head)), p(known_off),
                  p(known_rc), nb.data_ptr(), nk.data_ptr(), td.data_ptr(), p(sc), ws.data_ptr(), ws.numel(), _stream())
        return (nb, nk, td, sc) if return_scores else (nb, nk, td)

    def topk_candidates(self, queries: torch.Tensor, k: int, cand_is_head: bool = False, known_off: torch.Tensor = None,
                        known_rc: torch.Tensor = None, row_set: torch.Tensor = None, mask: torch.Tensor = None):
        """ge_transx_topk / ge_transr_topk on the [B,2] (fixed, relation) rows as given: (ids int32 [B,k], dist fp32
        [B,k]) device tensors, the first k entities in ascending (D, id), D the rank sweep's own distance.  known_off /
        known_rc: ge_known_cells' lists for these rows with pos_of = the identity (None: unfiltered); known cells are
        skipped.  Padding -1 / +inf; a row with an id out of range or a NaN distance is -1 / NaN.  row_set / mask (as
        rank_counts): only entities admissible in the row's set are returned (ge_transx_topk_masked /
        ge_transr_topk_masked); an empty set gives a row of -1 / +inf, a set index outside [-1, n_sets) -1 / NaN."""
        _need_cuda(queries, "queries")
        qb = queries.to(torch.int32).contiguous()
        if qb.dim() != 2 or qb.shape[1] != 2:
            raise ValueError("queries must have shape [B, 2] (fixed entity, relation)")
        k = int(k)
        if not 1 <= k <= topk_max_k():
            raise ValueError(f"k must lie in [1, {topk_max_k()}], got {k}")
        if (known_off is None) != (known_rc is None):
            raise ValueError("known_off and known_rc come together")
        B, dev = qb.shape[0], qb.device
        sets = self._sets_args(B, row_set, mask)
        ids = torch.empty(B, k, dtype=torch.int32, device=dev)
        dist = torch.empty(B, k, dtype=torch.float32, device=dev)
        if B == 0:
            return ids, dist
        nbytes = self._ws_bytes("topk", B, k)
        if nbytes == 0:
            raise RuntimeError(f"{self.PREFIX}_topk_workspace_bytes failed")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        p = lambda t: None if t is None else t.data_ptr()
        _lib.call(self.PREFIX + ("_topk_masked" if sets else "_topk"), *self._ptrs(), qb.data_ptr(), B,
                  int(bool(cand_is_head)), p(known_off), p(known_rc), *sets, k, ids.data_ptr(), dist.data_ptr(),
                  ws.data_ptr(), ws.numel(), _stream())
        return ids, dist

    def relation_rank_counts(self, triples: torch.Tensor, known_off: torch.Tensor = None, known_rc: torch.Tensor = None,
                             return_scores: bool = False):
        """ge_transx_relation_rank / ge_transr_relation_rank on the [B,3] (h, t, r) rows as given: every relation c is
        a candidate with D_c = D(h, t, c).  Returns (n_before, n_known_before, true_dist) device tensors, plus the
        [B, n_rel] distances with return_scores.  known_off / known_rc: ge_known_cells' lists for these rows (fixed = h,
        rel = t against a KnownIndex(side="relation")) with pos_of = the identity over [0, n_rel) (None: unfiltered).
        Rows with an id out of range get -1 counts and a NaN distance."""
        tb = _pairs(triples, "triples")
        B, dev = tb.shape[0], tb.device
        if (known_off is None) != (known_rc is None):
            raise ValueError("known_off and known_rc come together")
        ws_bytes = self._ws_bytes("relation_rank", max(B, 1))
        if ws_bytes == 0:
            raise RuntimeError(f"{self.PREFIX}_relation_rank_workspace_bytes failed")
        nb = torch.empty(B, dtype=torch.int32, device=dev)
        nk = torch.empty(B, dtype=torch.int32, device=dev)
        td = torch.empty(B, dtype=torch.float32, device=dev)
        sc = torch.empty((B, self.n_rel) if return_scores else (0,), dtype=torch.float32, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        p = lambda t: None if t is None else t.data_ptr()
        _lib.call(self.PREFIX + "_relation_rank", *self._ptrs(), tb.data_ptr(), B, p(known_off), p(known_rc),
                  nb.data_ptr(), nk.data_ptr(), td.data_ptr(), sc.data_ptr() if return_scores else None, ws.data_ptr(),
                  ws.numel(), _stream())
        return (nb, nk, td, sc) if return_scores else (nb, nk, td)

    def relation_ranks(self, test, known=None, batch: int = None):
        """(raw, filtered) int64 rank arrays of the test triples' relations over every relation:
        evaluate.translation_relation_ranks."""
        from .evaluate import translation_relation_ranks
        return translation_relation_ranks(self, test, known, batch=batch)

    def predict_relations(self, pairs, k: int, known=None, batch: int = None):
        """Top-k relation prediction for (h, t) pairs: evaluate.predict_translation_relations."""
        from .evaluate import predict_translation_relations
        return predict_translation_relations(self, pairs, k, known, batch=batch)

    def predict(self, queries, k: int, known=None, side: str = "tail", batch: int = None, fused: bool = None,
                candidate_sets=None, row_sets=None):
        """Top-k tail (or head) prediction over every entity, or with candidate_sets over each row's set:
        evaluate.predict_translation."""
        from .evaluate import predict_translation
        return predict_translation(self, queries, k, known, side=side, batch=batch, fused=fused,
                                   candidate_sets=candidate_sets, row_sets=row_sets)

    def ranks(self, test, known=None, side: str = "tail", batch: int = None, candidate_sets=None, row_sets=None,
              return_admissible: bool = False):
        """(raw, filtered) int64 rank arrays of the test triples over every entity, or with candidate_sets over each
        row's set: evaluate.translation_ranks."""
        from .evaluate import translation_ranks
        return translation_ranks(self, test, known, side=side, batch=batch, candidate_sets=candidate_sets,
                                 row_sets=row_sets, return_admissible=return_admissible)

    def triple_classification(self, valid_pos, test_pos, valid_neg=None, test_neg=None, known=None, seed: int = 0,
                              mode: str = "mid"):
        """Per-relation thresholds fitted on the validation split, the test split classified:
        classify.triple_classification."""
        from .classify import triple_classification
        return triple_classification(self, valid_pos, test_pos, valid_neg, test_neg, known=known, seed=seed, mode=mode)

    def trainer(self, triples, batch_size: int, *, loss: str = "hinge", negatives: Optional[int] = None,
                adversarial_temperature: Optional[float] = None, margin: float = 1.0, learning_rate: float = 0.001,
                seed: int = 0, optimizer: str = "sgd", initial_accumulator_value: float = 0.1) -> Trainer:
        """The model's native loop.  optimizer="sgd" (the default) is the model's own step: plain SGD for TransX and
        RotatE, Adam for TransR.  optimizer="adagrad" (not TransR) enables AdaGrad with initial_accumulator_value unless
        the model already has accumulators, which are kept; its run(n) is one <PREFIX>_train_steps_adagrad call.
        loss="hinge" (the default): one negative per positive under the margin hinge.  loss="self_adversarial" (TransX
        and RotatE): an AdvTrainer with `negatives` = K per positive (default 64) and `adversarial_temperature` = alpha
        (default 1.0); margin is gamma.  Either optimizer."""
        if loss not in LOSSES:
            raise ValueError(f"loss must be one of {LOSSES}, got {loss!r}")
        if loss == "hinge":
            if negatives is not None or adversarial_temperature is not None:
                raise ValueError("negatives and adversarial_temperature need loss='self_adversarial'")
            if optimizer not in ("sgd", "adagrad"):
                raise ValueError(f"optimizer must be 'sgd' or 'adagrad', got {optimizer!r}")
            if optimizer == "adagrad":
                self._trainer_adagrad(initial_accumulator_value)
            tr = self._trainer(self, triples, batch_size, margin=margin, learning_rate=learning_rate, seed=seed)
            tr.optimizer = optimizer
            return tr
        if not isinstance(self, _AdvLoss):
            raise ValueError(f"{type(self).__name__} has no self-adversarial step: loss must be 'hinge'")
        K = 64 if negatives is None else negatives
        alpha = 1.0 if adversarial_temperature is None else adversarial_temperature
        check_adv_hyperparameters(K, alpha, margin)
        if optimizer not in ("sgd", "adagrad"):
            raise ValueError(f"optimizer must be 'sgd' or 'adagrad', got {optimizer!r}")
        if optimizer == "adagrad":
            self._trainer_adagrad(initial_accumulator_value)
        tr = AdvTrainer(self, triples, batch_size, negatives=K, adversarial_temperature=alpha, margin=margin,
                        learning_rate=learning_rate, seed=seed)
        tr.optimizer = optimizer
        return tr

    def _trainer_adagrad(self, initial_accumulator_value: float) -> None:
        raise ValueError(f"{type(self).__name__} has no AdaGrad step: TransR trains with Adam, which optimizer='sgd' "
                         "(the default) leaves in place")

    def _state_tensors(self) -> Dict[str, torch.Tensor]:
        return self.tables

    def _pocket_tensors(self) -> Dict[str, torch.Tensor]:
        """Every device tensor of the training state, under its state_dict name: what a validation pocket
        (evaluate.TranslationPocket) copies on an improving tick -- the tables, and adagrad_<table> per accumulator."""
        acc = getattr(self, "accumulators", None) or {}
        return {**self.tables, **{"adagrad_" + k: v for k, v in acc.items()}}

    def _pocket_scalars(self) -> Dict[str, object]:
        """The host attributes that belong to that state (recorded per tick, set again by the pocket's restore())."""
        return {}

    def _check_candidate_sets(self) -> None:
        """Raises where the model's sweeps take no candidate sets."""

    def _check_state(self, state: Dict[str, object], keys, what: str) -> None:
        """The sizes in `keys` and the shape of every tensor, checked before anything is copied."""
        for key in keys:
            if state[key] != getattr(self, key):
                raise ValueError(f"state_dict {key}={state[key]!r} does not match this model's {getattr(self, key)!r}")
        for name, t in self._state_tensors().items():
            src = state[name]
            if tuple(src.shape) != tuple(t.shape):
                raise ValueError(f"state_dict {what} {name} has shape {tuple(src.shape)}, expected {tuple(t.shape)}")

    def _copy_state(self, state: Dict[str, object]) -> None:
        self.l1 = bool(state.get("l1", self.l1))
        for name, t in self._state_tensors().items():
            t.copy_(state[name].to(device=t.device, dtype=torch.float32))


class _AdvLoss:
    """The self-adversarial negative-sampling loss of a model whose PREFIX has <PREFIX>_adv_* entry points (TransX,
    RotatE): per-row losses and the two single steps.  The model supplies _ptrs(), _adagrad_ptrs() and
    _adv_ws_bytes(B, K); trainer(loss="self_adversarial") is _Model's."""
    _adv_ws = None                                       # ((B, K), workspace) of the last adv_step / adv_adagrad_step

    def _adv_workspace(self, B: int, K: int) -> torch.Tensor:
        nbytes = self._adv_ws_bytes(int(B), int(K))
        if nbytes == 0:
            raise RuntimeError(f"{self.PREFIX}_adv_step_workspace_bytes failed")
        return torch.empty(nbytes, dtype=torch.uint8, device=self.tables["ent"].device)

    def _adv_step_workspace(self, B: int, K: int) -> torch.Tensor:
        """The single steps' workspace, kept while (B, K) stays (as _Model.workspace keeps the hinge step's by B)."""
        if self._adv_ws is None or self._adv_ws[0] != (B, K):
            self._adv_ws = ((B, K), self._adv_workspace(B, K))
        return self._adv_ws[1]

    @staticmethod
    def _adv_batch(pos, side, neg_ent, margin, alpha):
        """(pos, side, neg_ent) as contiguous int32 device tensors; shapes, dtypes, K and the two hyperparameters are
        checked first, on the host.  An int64 value that int32 does not hold is clamped to [-1, 2^31 - 1] before the
        cast, so that it stays what it was: out of range (an empty slot, an invalid row), never wrapped into a valid id."""
        for name, t in (("pos", pos), ("side", side), ("neg_ent", neg_ent)):
            if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"{name} must be an int32 or int64 tensor")
        if pos.dim() != 2 or pos.shape[1] != 3 or pos.shape[0] == 0:
            raise ValueError("pos must have shape [B, 3] (head, tail, relation) with B >= 1")
        B = pos.shape[0]
        if side.dim() != 1 or side.shape[0] != B:
            raise ValueError("side must have shape [B]")
        if neg_ent.dim() != 2 or neg_ent.shape[0] != B:
            raise ValueError("neg_ent must have shape [B, K]")
        check_adv_hyperparameters(int(neg_ent.shape[1]), alpha, margin)
        out = []
        for name, t in (("pos", pos), ("side", side), ("neg_ent", neg_ent)):
            _need_cuda(t, name)
            out.append((t.clamp(-1, 2**31 - 1) if t.dtype == torch.int64 else t).to(torch.int32).contiguous())
        return out

    def adv_loss(self, pos: torch.Tensor, side: torch.Tensor, neg_ent: torch.Tensor, margin: float,
                 alpha: float) -> torch.Tensor:
        """The [B] per-row self-adversarial losses (NaN for a row with a positive id out of range or a side outside
        {0, 1}); a slot of neg_ent outside [0, n_ent) is empty."""
        pb, sb, nb = self._adv_batch(pos, side, neg_ent, margin, alpha)
        out = torch.empty(pb.shape[0], dtype=torch.float32, device=pb.device)
        _lib.call(self.PREFIX + "_adv_loss", *self._ptrs(), pb.data_ptr(), sb.data_ptr(), nb.data_ptr(), pb.shape[0],
                  nb.shape[1], float(margin), float(alpha), out.data_ptr(), _stream())
        return out

    def _adv_step(self, entry, ptrs, pos, side, neg_ent, margin, alpha, lr):
        pb, sb, nb = self._adv_batch(pos, side, neg_ent, margin, alpha)
        ws = self._adv_step_workspace(pb.shape[0], nb.shape[1])
        _lib.call(entry, *ptrs(), pb.data_ptr(), sb.data_ptr(), nb.data_ptr(), pb.shape[0], nb.shape[1], float(margin),
                  float(alpha), float(lr), self._loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        return self._loss[0].clone()

    def adv_step(self, pos, side, neg_ent, margin: float, alpha: float, lr: float) -> torch.Tensor:
        """One SGD step on the summed self-adversarial loss; returns that batch loss (device scalar, before the step)."""
        return self._adv_step(self.PREFIX + "_adv_step", self._ptrs, pos, side, neg_ent, margin, alpha, lr)

    def adv_adagrad_step(self, pos, side, neg_ent, margin: float, alpha: float, lr: float) -> torch.Tensor:
        """The same step with AdaGrad's update (enable_adagrad() first)."""
        self._adagrad_ptrs()
        return self._adv_step(self.PREFIX + "_adv_adagrad_step", self._adagrad_ptrs, pos, side, neg_ent, margin, alpha, lr)


class TransX(_AdvLoss, _Model):
    """The tables of one translation model.  `model` in {"transe", "transh", "transd"}; `l1` selects the L1
    distance (the reference's L1_flag), else the squared L2 one."""
    PREFIX = "ge_transx"

    def __init__(self, model: str, n_ent: int, n_rel: int, d: int, l1: bool = True, seed: Optional[int] = 0,
                 device="cuda"):
        model = model.lower()
        if model not in MODELS:
            raise ValueError(f"model must be one of {sorted(MODELS)}, got {model!r}")
        if n_ent <= 0 or n_rel <= 0:
            raise ValueError("n_ent and n_rel must be positive")
        if not 1 <= d <= 1024:
            raise ValueError(f"d must lie in [1, 1024], got {d}")
        self.model, self.n_ent, self.n_rel, self.d, self.l1 = model, int(n_ent), int(n_rel), int(d), bool(l1)
        rows = {"ent": n_ent, "rel": n_rel, "normal_vector": n_rel, "ent_transfer": n_ent, "rel_transfer": n_rel}
        self._init_tables([(name, (rows[name], d)) for name in ("ent", "rel") + EXTRA_TABLES[model]], seed, device)

    # the pointer arguments every ge_transx_* entry takes
    def _ptrs(self):
        t = self.tables
        p = lambda name: t[name].data_ptr() if name in t else None
        return (MODELS[self.model], int(self.l1), p("ent"), self.n_ent, p("rel"), self.n_rel, p("normal_vector"),
                p("ent_transfer"), p("rel_transfer"), self.d)

    def _ws_bytes(self, kind: str, B: int, *extra) -> int:
        lead = (MODELS[self.model],) if kind in ("rank", "topk", "relation_rank") else ()
        return getattr(_lib.load(), f"ge_transx_{kind}_workspace_bytes")(*lead, self.n_ent, self.n_rel, self.d, B, *extra)

    def _adv_ws_bytes(self, B: int, K: int) -> int:
        return _lib.load().ge_transx_adv_step_workspace_bytes(MODELS[self.model], self.n_ent, self.n_rel, self.d, B, K)

    def step(self, pos: torch.Tensor, neg: torch.Tensor, lr: float, margin: float) -> torch.Tensor:
        """One SGD step on sum max(D(pos) - D(neg) + margin, 0); returns that batch loss (device scalar, before
        the step).  neg must keep pos's relation column (as getBatch's negatives do)."""
        pb, nb, ws = self._step_batch(pos, neg)
        _lib.call("ge_transx_hinge_step", *self._ptrs(), pb.data_ptr(), nb.data_ptr(), pb.shape[0], float(margin),
                  float(lr), self._loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        return self._loss[0].clone()

    # --- AdaGrad (ge_transx_adagrad_step / ge_transx_train_steps_adagrad): one accumulator per table
    accumulators: Optional[Dict[str, torch.Tensor]] = None
    adagrad_init: Optional[float] = None

    def enable_adagrad(self, initial_accumulator_value: float = 0.1) -> None:
        """Create (or refill) `accumulators`: one fp32 tensor per table under the table's name, filled with
        initial_accumulator_value, TF1's AdagradOptimizer(lr, initial_accumulator_value) slots."""
        a0 = float(initial_accumulator_value)
        if not a0 > 0:
            raise ValueError(f"initial_accumulator_value must be positive, got {initial_accumulator_value}")
        self.accumulators = {k: torch.full_like(v, a0) for k, v in self.tables.items()}
        self.adagrad_init = a0

    def _trainer_adagrad(self, initial_accumulator_value: float) -> None:
        if not float(initial_accumulator_value) > 0:
            raise ValueError(f"initial_accumulator_value must be positive, got {initial_accumulator_value}")
        if self.accumulators is None:
            self.enable_adagrad(initial_accumulator_value)

    def _adagrad_ptrs(self):
        """_ptrs() with the five accumulator arguments in front of d, as the two AdaGrad entry points take them."""
        if self.accumulators is None:
            raise RuntimeError("AdaGrad is not enabled: call enable_adagrad() first")
        a = self.accumulators
        p = lambda name: a[name].data_ptr() if name in a else None
        base = self._ptrs()
        return (*base[:-1], p("ent"), p("rel"), p("normal_vector"), p("ent_transfer"), p("rel_transfer"), base[-1])

    def adagrad_step(self, pos: torch.Tensor, neg: torch.Tensor, lr: float, margin: float) -> torch.Tensor:
        """One AdaGrad step on sum max(D(pos) - D(neg) + margin, 0): per row an active pair names, s = its summed
        gradient, accumulator += s * s, row -= lr * s / sqrt(accumulator).  Returns the batch loss as step() does."""
        ptrs = self._adagrad_ptrs()
        pb, nb, ws = self._step_batch(pos, neg)
        _lib.call("ge_transx_adagrad_step", *ptrs, pb.data_ptr(), nb.data_ptr(), pb.shape[0], float(margin), float(lr),
                  self._loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        return self._loss[0].clone()

    def _train_steps(self, tr: Trainer, n: int, losses: torch.Tensor, ws: torch.Tensor) -> None:
        ada = tr.optimizer == "adagrad"
        _lib.call("ge_transx_train_steps_adagrad" if ada else "ge_transx_train_steps",
                  *(self._adagrad_ptrs() if ada else self._ptrs()), *tr._sampler_args(), tr.seed & (2**64 - 1),
                  tr.step_count, n, tr.B, tr.margin, tr.lr, losses.data_ptr(), ws.data_ptr(), ws.numel(), _stream())

    def state_dict(self) -> Dict[str, object]:
        state = {"model": self.model, "l1": self.l1, "n_ent": self.n_ent, "n_rel": self.n_rel, "d": self.d,
                 **{k: v.detach().cpu().clone() for k, v in self.tables.items()}}
        if self.accumulators is not None:                # adagrad_init and one adagrad_<table> per table
            state["adagrad_init"] = self.adagrad_init
            state.update({"adagrad_" + k: v.detach().cpu().clone() for k, v in self.accumulators.items()})
        return state

    def load_state_dict(self, state: Dict[str, object]) -> None:
        """Every shape is checked before anything is copied.  A state with accumulators enables AdaGrad and restores
        them; one without, loaded into a model with AdaGrad enabled, refills the accumulators with its adagrad_init."""
        self._check_state(state, ("model", "n_ent", "n_rel", "d"), "table")
        has = "adagrad_init" in state
        if has:
            a0 = float(state["adagrad_init"])
            if not a0 > 0:
                raise ValueError(f"state_dict adagrad_init={a0} must be positive")
            for name, t in self.tables.items():
                if "adagrad_" + name not in state:
                    raise ValueError(f"state_dict has adagrad_init but no adagrad_{name}")
                src = state["adagrad_" + name]
                if tuple(src.shape) != tuple(t.shape):
                    raise ValueError(f"state_dict accumulator adagrad_{name} has shape {tuple(src.shape)}, "
                                     f"expected {tuple(t.shape)}")
        self._copy_state(state)
        if has:
            if self.accumulators is None:
                self.enable_adagrad(a0)
            self.adagrad_init = a0
            for name, acc in self.accumulators.items():
                acc.copy_(state["adagrad_" + name].to(device=acc.device, dtype=torch.float32))
        elif self.accumulators is not None:
            self.enable_adagrad(self.adagrad_init)
