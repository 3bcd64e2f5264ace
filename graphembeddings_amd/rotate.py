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

import numpy as np
import torch

from . import _lib
from .hole import _need_cuda, _stream
from .transx import Trainer, TransX, _Model, read_kg, read_triples  # noqa: F401  (the same *2id.txt readers)

MAX_DIM = 1024
MAX_NEGATIVES = 1024            # ge_rotate_adv_max_negatives()
LOSSES = ("hinge", "self_adversarial")


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
    negatives per positive (ge_rotate_adv_draw_batch), one ge_rotate_adv_train_steps[_adagrad] call per run().  Its
    workspace depends on K as well as on B and is cached here, not in the model."""

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
        _lib.call("ge_rotate_adv_train_steps_adagrad" if ada else "ge_rotate_adv_train_steps",
                  *(m._adagrad_ptrs() if ada else m._ptrs()), *self._sampler_args(), self.seed & (2**64 - 1),
                  self.step_count, int(n), self.B, self.K, self.margin, self.alpha, self.lr, losses.data_ptr(),
                  ws.data_ptr(), ws.numel(), _stream())
        self.step_count += int(n)
        return losses


def _out_of_scope(what: str):
    return NotImplementedError(f"RotatE has no {what}: the ge_rotate_* entry points score, train and rank over every entity")


class RotatE(_Model):
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

    # --- the self-adversarial negative-sampling loss (ge_rotate_adv_*)
    _adv_ws = None                                       # ((B, K), workspace) of the last adv_step / adv_adagrad_step

    def _adv_workspace(self, B: int, K: int) -> torch.Tensor:
        nbytes = _lib.load().ge_rotate_adv_step_workspace_bytes(self.n_ent, self.n_rel, self.d, int(B), int(K))
        if nbytes == 0:
            raise RuntimeError("ge_rotate_adv_step_workspace_bytes failed")
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
        _lib.call("ge_rotate_adv_loss", *self._ptrs(), pb.data_ptr(), sb.data_ptr(), nb.data_ptr(), pb.shape[0],
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
        return self._adv_step("ge_rotate_adv_step", self._ptrs, pos, side, neg_ent, margin, alpha, lr)

    def adv_adagrad_step(self, pos, side, neg_ent, margin: float, alpha: float, lr: float) -> torch.Tensor:
        """The same step with AdaGrad's update (enable_adagrad() first)."""
        self._adagrad_ptrs()
        return self._adv_step("ge_rotate_adv_adagrad_step", self._adagrad_ptrs, pos, side, neg_ent, margin, alpha, lr)

    def trainer(self, triples, batch_size: int, *, loss: str = "hinge", negatives: Optional[int] = None,
                adversarial_temperature: Optional[float] = None, margin: float = 1.0, learning_rate: float = 0.001,
                seed: int = 0, optimizer: str = "sgd", initial_accumulator_value: float = 0.1) -> Trainer:
        """loss="hinge" (the default): _Model.trainer's loop, one negative per positive.  loss="self_adversarial": an
        AdvTrainer with `negatives` = K per positive (default 64) and `adversarial_temperature` = alpha (default 1.0);
        margin is gamma.  Either optimizer."""
        if loss not in LOSSES:
            raise ValueError(f"loss must be one of {LOSSES}, got {loss!r}")
        if loss == "hinge":
            if negatives is not None or adversarial_temperature is not None:
                raise ValueError("negatives and adversarial_temperature need loss='self_adversarial'")
            return super().trainer(triples, batch_size, margin=margin, learning_rate=learning_rate, seed=seed,
                                   optimizer=optimizer, initial_accumulator_value=initial_accumulator_value)
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

    # --- what this model does not have
    def rank_counts(self, triples: torch.Tensor, cand_is_head: bool = False, known_off: torch.Tensor = None,
                    known_rc: torch.Tensor = None, return_scores: bool = False, row_set: torch.Tensor = None,
                    mask: torch.Tensor = None):
        """ge_rotate_rank on the [B,3] rows as given: _Model.rank_counts without candidate sets."""
        if row_set is not None or mask is not None:
            raise _out_of_scope("candidate sets")
        return super().rank_counts(triples, cand_is_head, known_off, known_rc, return_scores)

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
