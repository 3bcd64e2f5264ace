"""TransR (transR.py) on the MI355X: tables, Adam state, batch scoring, the margin-hinge Adam step and the native
multi-step loop of include/ge_hip.h's ge_transr_* entry points.

Reference semantics: `ent [E,dim_e]`, `rel [R,dim_r]` and `rel_matrix [R,dim_e*dim_r]` (row r read as [dim_r][dim_e]
is M_r), each xavier_initializer(uniform=False) for its own shape; u = M_r h + r - M_r t, D = sum |u| (L1) or
sum u^2; loss = sum_batch max(D+ - D- + margin, 0); tf.train.AdamOptimizer(0.001) on every table, whose m and v
decay on every row at every step.  There is no CPU path: every call runs a HIP kernel.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _lib
from . import transx as X
from .hole import _stream
from .transx import _Model, read_kg, read_triples  # noqa: F401  (the same *2id.txt readers)

TABLES = ("ent", "rel", "rel_matrix")
MAX_DIM = 256
# tf.train.AdamOptimizer's defaults
BETA1, BETA2, EPSILON = 0.9, 0.999, 1e-8


def check_adam(lr: float, b1: float, b2: float, eps: float) -> None:
    if not lr > 0:
        raise ValueError(f"learning rate must be positive, got {lr}")
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"beta1 and beta2 must lie in [0, 1), got {b1}, {b2}")
    if not eps >= 0:
        raise ValueError(f"epsilon must be non-negative, got {eps}")


class Trainer(X.Trainer):
    """transR.py's training loop (getBatch + train_step): transx.Trainer with one Adam step per draw.  The Adam step
    count lives in the model: run(n) advances model.t by n."""

    def __init__(self, model: TransR, triples, batch_size: int, *, margin: float = 1.0, learning_rate: float = 0.001,
                 seed: int = 0, b1: float = BETA1, b2: float = BETA2, eps: float = EPSILON):
        check_adam(learning_rate, b1, b2, eps)
        super().__init__(model, triples, batch_size, margin=margin, learning_rate=learning_rate, seed=seed)
        self.b1, self.b2, self.eps = float(b1), float(b2), float(eps)

    def run(self, n: int) -> torch.Tensor:
        losses = super().run(n)
        self.model.t += losses.numel()
        return losses


class TransR(_Model):
    """The tables and Adam state of one TransR model.  `l1` selects the L1 distance (the reference's L1_flag),
    else the squared L2 one.  m and v are flat [ent | rel | rel_matrix] buffers; t counts the steps taken."""
    PREFIX = "ge_transr"
    _trainer = Trainer

    def __init__(self, n_ent: int, n_rel: int, dim_e: int = 100, dim_r: int = 100, l1: bool = True,
                 seed: Optional[int] = 0, device="cuda"):
        if n_ent <= 0 or n_rel <= 0:
            raise ValueError("n_ent and n_rel must be positive")
        for name, d in (("dim_e", dim_e), ("dim_r", dim_r)):
            if not 1 <= d <= MAX_DIM:
                raise ValueError(f"{name} must lie in [1, {MAX_DIM}], got {d}")
        self.n_ent, self.n_rel, self.dim_e, self.dim_r, self.l1 = int(n_ent), int(n_rel), int(dim_e), int(dim_r), bool(l1)
        self._init_tables(zip(TABLES, ((n_ent, dim_e), (n_rel, dim_r), (n_rel, dim_e * dim_r))), seed, device)
        n, dev = sum(t.numel() for t in self.tables.values()), self.tables["ent"].device
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        self.t = 0

    def _ptrs(self):
        t = self.tables
        return (int(self.l1), t["ent"].data_ptr(), self.n_ent, t["rel"].data_ptr(), t["rel_matrix"].data_ptr(),
                self.n_rel, self.dim_e, self.dim_r)

    def _ws_bytes(self, kind: str, B: int, *extra) -> int:
        return getattr(_lib.load(), f"ge_transr_{kind}_workspace_bytes")(self.n_ent, self.n_rel, self.dim_e,
                                                                          self.dim_r, B, *extra)

    def moments(self, name: str):
        """(m, v) of one table, as views shaped like it."""
        off = 0
        for k in TABLES:
            n = self.tables[k].numel()
            if k == name:
                shape = self.tables[k].shape
                return self.m[off:off + n].view(shape), self.v[off:off + n].view(shape)
            off += n
        raise KeyError(name)

    def step(self, pos: torch.Tensor, neg: torch.Tensor, margin: float, lr: float = 0.001, b1: float = BETA1,
             b2: float = BETA2, eps: float = EPSILON) -> torch.Tensor:
        """One Adam step (t -> t + 1) on sum max(D(pos) - D(neg) + margin, 0); returns that batch loss (device
        scalar, before the step).  neg must keep pos's relation column (as getBatch's negatives do)."""
        check_adam(lr, b1, b2, eps)
        pb, nb, ws = self._step_batch(pos, neg)
        _lib.call("ge_transr_adam_step", *self._ptrs(), self.m.data_ptr(), self.v.data_ptr(), pb.data_ptr(),
                  nb.data_ptr(), pb.shape[0], float(margin), float(lr), float(b1), float(b2), float(eps), self.t + 1,
                  self._loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        self.t += 1
        return self._loss[0].clone()

    def _train_steps(self, tr: Trainer, n: int, losses: torch.Tensor, ws: torch.Tensor) -> None:
        _lib.call("ge_transr_train_steps", *self._ptrs(), self.m.data_ptr(), self.v.data_ptr(), *tr._sampler_args(),
                  tr.seed & (2**64 - 1), tr.step_count, n, tr.B, tr.margin, tr.lr, tr.b1, tr.b2, tr.eps, self.t + 1,
                  losses.data_ptr(), ws.data_ptr(), ws.numel(), _stream())

    def _state_tensors(self) -> Dict[str, torch.Tensor]:
        return {**self.tables, "m": self.m, "v": self.v}

    def _pocket_tensors(self) -> Dict[str, torch.Tensor]:
        return self._state_tensors()                     # the tables and Adam's flat m and v

    def _pocket_scalars(self) -> Dict[str, object]:
        return {"t": self.t}                             # Adam's step count goes with m and v

    def state_dict(self) -> Dict[str, object]:
        return {"model": "transr", "l1": self.l1, "n_ent": self.n_ent, "n_rel": self.n_rel, "dim_e": self.dim_e,
                "dim_r": self.dim_r, "t": self.t, "m": self.m.detach().cpu().clone(), "v": self.v.detach().cpu().clone(),
                **{k: v.detach().cpu().clone() for k, v in self.tables.items()}}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        if state.get("model") != "transr":
            raise ValueError(f"state_dict is of model {state.get('model')!r}, not 'transr'")
        self._check_state(state, ("n_ent", "n_rel", "dim_e", "dim_r"), "tensor")
        t = int(state["t"])
        if t < 0:
            raise ValueError(f"state_dict t={t} is negative")
        self._copy_state(state)
        self.t = t
