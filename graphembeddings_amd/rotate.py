"""RotatE (Sun et al., ICLR 2019) on the MI355X: the translation model in the complex plane, t ~ h o r with |r_j| = 1.
Tables, batch scoring, the margin-hinge step and the paper's self-adversarial negative-sampling step (SGD and AdaGrad
each), their native multi-step loops and link-prediction ranks of include/ge_hip.h's ge_rotate_* entry points.

`ent [E,d]` (d even, a row [Re (d/2) | Im (d/2)], xavier_initializer(uniform=False) like every other model's tables)
and `rel [R,d/2]` of PHASES in radians, uniform in [-pi, pi) at the start and unconstrained after it: never wrapped,
never normalised.  D = sum_j |h_j e^{i theta_j} - t_j| (l1, the paper's norm) or sum_j |.|^2; loss = sum_batch
max(D+ - D- + margin, 0); plain SGD or TF1's AdaGrad rule on both tables, as for TransX.  There is no CPU path: every
call runs a HIP kernel.

The self-adversarial loss (adv_loss / adv_step / adv_adagrad_step, trainer(loss="self_adversarial")): K negatives per
positive, all on one side of it (side 0: tails replaced, 1: heads), weighted by a softmax over their own scores that is
not differentiated: loss_i = softplus(D+ - margin) + sum_j softmax_j(-alpha D-_j) softplus(margin - D-_j), summed over
the batch.  The loop draws the K negatives filtered (never a known completion), with the hinge loop's positives and
sides for the same seed.

Not provided for this model (each raises NotImplementedError naming the operation): top-k prediction, candidate sets,
relation prediction; nor multi-GPU training.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import _lib
from .hole import _stream
# the same *2id.txt readers; the self-adversarial loss's shared host side (MAX_NEGATIVES = ge_rotate_adv_max_negatives())
from .transx import (LOSSES, MAX_NEGATIVES, AdvTrainer, Trainer, TransX, _AdvLoss, _Model,  # noqa: F401
                     check_adv_hyperparameters, read_kg, read_triples)

MAX_DIM = 1024


def _out_of_scope(what: str):
    return NotImplementedError(f"RotatE has no {what}: the ge_rotate_* entry points score, train and rank over every entity")


class RotatE(_AdvLoss, _Model):
    """The two tables of one RotatE model.  `l1` selects the sum of complex moduli (the paper's norm), else the sum of
    their squares."""
    PREFIX = "ge_rotate"

    def __init__(self, n_ent: int, n_rel: int, d: int, l1: bool = True, seed: Optional[int] = 0, device="cuda"):
        if n_ent <= 0 or n_rel <= 0:
            raise ValueError("n_ent and n_rel must be positive")
        if not 2 <= d <= MAX_DIM or d % 2:
            raise ValueError(f"d must be even and lie in [2, {MAX_DIM}], got {d}")
        self.n_ent, self.n_rel, self.d, self.l1 = int(n_ent), int(n_rel), int(d), bool(l1)
        self._init_tables([("ent", (n_ent, d))], seed, device)
        dev = self.tables["ent"].device
        gen = torch.Generator(device=dev)
        if seed is not None:
            gen.manual_seed(int(seed) + 1)
        else:
            gen.seed()                                   # (a fresh Generator starts from torch's fixed default seed)
        u = torch.rand(n_rel, d // 2, dtype=torch.float32, device=dev, generator=gen)      # [0, 1)
        self.tables["rel"] = ((u * 2.0 - 1.0) * math.pi).contiguous()

    # the table arguments every ge_rotate_* entry takes
    def _ptrs(self):
        t = self.tables
        return (int(self.l1), t["ent"].data_ptr(), self.n_ent, t["rel"].data_ptr(), self.n_rel, self.d)

    def _ws_bytes(self, kind: str, B: int, *extra) -> int:
        if kind not in ("step", "rank"):
            raise _out_of_scope({"topk": "top-k prediction", "relation_rank": "relation prediction"}.get(kind, kind))
        return getattr(_lib.load(), f"ge_rotate_{kind}_workspace_bytes")(self.n_ent, self.n_rel, self.d, B)

    def step(self, pos: torch.Tensor, neg: torch.Tensor, lr: float, margin: float) -> torch.Tensor:
        """One SGD step on sum max(D(pos) - D(neg) + margin, 0); returns that batch loss (device scalar, before the
        step).  neg must keep pos's relation column."""
        pb, nb, ws = self._step_batch(pos, neg)
        _lib.call("ge_rotate_hinge_step", *self._ptrs(), pb.data_ptr(), nb.data_ptr(), pb.shape[0], float(margin),
                  float(lr), self._loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        return self._loss[0].clone()

    # --- AdaGrad (ge_rotate_adagrad_step / ge_rotate_train_steps_adagrad): one accumulator per table, as TransX
    accumulators: Optional[Dict[str, torch.Tensor]] = None
    adagrad_init: Optional[float] = None
    enable_adagrad = TransX.enable_adagrad
    _trainer_adagrad = TransX._trainer_adagrad

    def _adagrad_ptrs(self):
        """_ptrs() with the two accumulator arguments in front of d."""
        if self.accumulators is None:
            raise RuntimeError("AdaGrad is not enabled: call enable_adagrad() first")
        a, base = self.accumulators, self._ptrs()
        return (*base[:-1], a["ent"].data_ptr(), a["rel"].data_ptr(), base[-1])

    def adagrad_step(self, pos: torch.Tensor, neg: torch.Tensor, lr: float, margin: float) -> torch.Tensor:
        """One AdaGrad step on the same loss: per row an active pair names, s = its summed gradient,
        accumulator += s * s, row -= lr * s / sqrt(accumulator).  Returns the batch loss as step() does."""
        ptrs = self._adagrad_ptrs()
        pb, nb, ws = self._step_batch(pos, neg)
        _lib.call("ge_rotate_adagrad_step", *ptrs, pb.data_ptr(), nb.data_ptr(), pb.shape[0], float(margin), float(lr),
                  self._loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        return self._loss[0].clone()

    def _train_steps(self, tr: Trainer, n: int, losses: torch.Tensor, ws: torch.Tensor) -> None:
        ada = tr.optimizer == "adagrad"
        _lib.call("ge_rotate_train_steps_adagrad" if ada else "ge_rotate_train_steps",
                  *(self._adagrad_ptrs() if ada else self._ptrs()), *tr._sampler_args(), tr.seed & (2**64 - 1),
                  tr.step_count, n, tr.B, tr.margin, tr.lr, losses.data_ptr(), ws.data_ptr(), ws.numel(), _stream())

    # --- the self-adversarial negative-sampling loss (ge_rotate_adv_*): transx._AdvLoss's methods, _Model.trainer
    def _adv_ws_bytes(self, B: int, K: int) -> int:
        return _lib.load().ge_rotate_adv_step_workspace_bytes(self.n_ent, self.n_rel, self.d, B, K)

    # --- what this model does not have
    def rank_counts(self, triples: torch.Tensor, cand_is_head: bool = False, known_off: torch.Tensor = None,
                    known_rc: torch.Tensor = None, return_scores: bool = False, row_set: torch.Tensor = None,
                    mask: torch.Tensor = None, out=None, workspace: torch.Tensor = None):
        """ge_rotate_rank on the [B,3] rows as given: _Model.rank_counts without candidate sets."""
        if row_set is not None or mask is not None:
            raise _out_of_scope("candidate sets")
        return super().rank_counts(triples, cand_is_head, known_off, known_rc, return_scores, out=out, workspace=workspace)

    def _check_candidate_sets(self) -> None:
        raise _out_of_scope("candidate sets")

    def ranks(self, test, known=None, side: str = "tail", batch: int = None, candidate_sets=None, row_sets=None,
              return_admissible: bool = False):
        """(raw, filtered) int64 rank arrays of the test triples over every entity: evaluate.translation_ranks."""
        if candidate_sets is not None or row_sets is not None or return_admissible:
            raise _out_of_scope("candidate sets")
        return super().ranks(test, known, side=side, batch=batch)

    def topk_candidates(self, *args, **kw):
        raise _out_of_scope("top-k prediction")

    def predict(self, *args, **kw):
        raise _out_of_scope("top-k prediction")

    def relation_rank_counts(self, *args, **kw):
        raise _out_of_scope("relation prediction")

    def relation_ranks(self, *args, **kw):
        raise _out_of_scope("relation prediction")

    def predict_relations(self, *args, **kw):
        raise _out_of_scope("relation prediction")

    # --- state: the keys of TransX, "model" = "rotate"
    def state_dict(self) -> Dict[str, object]:
        state = {"model": "rotate", "l1": self.l1, "n_ent": self.n_ent, "n_rel": self.n_rel, "d": self.d,
                 **{k: v.detach().cpu().clone() for k, v in self.tables.items()}}
        if self.accumulators is not None:                # adagrad_init and one adagrad_<table> per table
            state["adagrad_init"] = self.adagrad_init
            state.update({"adagrad_" + k: v.detach().cpu().clone() for k, v in self.accumulators.items()})
        return state

    model = "rotate"                                     # what _check_state compares the state's "model" with
    load_state_dict = TransX.load_state_dict
