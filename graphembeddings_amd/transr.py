"""TransR (transR.py) on the MI355X: tables, Adam state, batch scoring, the margin-hinge Adam step and the native
multi-step loop of include/ge_hip.h's ge_transr_* entry points.

Reference semantics: `ent [E,dim_e]`, `rel [R,dim_r]` and `rel_matrix [R,dim_e*dim_r]` (row r read as [dim_r][dim_e]
is M_r), each xavier_initializer(uniform=False) for its own shape; u = M_r h + r - M_r t, D = sum |u| (L1) or
sum u^2; loss = sum_batch max(D+ - D- + margin, 0); tf.train.AdamOptimizer(0.001) on every table, whose m and v
decay on every row at every step.  There is no CPU path: every call runs a HIP kernel.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .hole import BernoulliSampler, _stream, init_embeddings
from .transx import _pairs, _rank_call, read_kg, read_triples  # noqa: F401  (the same *2id.txt readers)

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


class TransR:
    """The tables and Adam state of one TransR model.  `l1` selects the L1 distance (the reference's L1_flag),
    else the squared L2 one.  m and v are flat [ent | rel | rel_matrix] buffers; t counts the steps taken."""

    def __init__(self, n_ent: int, n_rel: int, dim_e: int = 100, dim_r: int = 100, l1: bool = True,
                 seed: Optional[int] = 0, device="cuda"):
        if n_ent <= 0 or n_rel <= 0:
            raise ValueError("n_ent and n_rel must be positive")
        for name, d in (("dim_e", dim_e), ("dim_r", dim_r)):
            if not 1 <= d <= MAX_DIM:
                raise ValueError(f"{name} must lie in [1, {MAX_DIM}], got {d}")
        self.n_ent, self.n_rel, self.dim_e, self.dim_r, self.l1 = int(n_ent), int(n_rel), int(dim_e), int(dim_r), bool(l1)
        base = None if seed is None else int(seed)
        shapes = {"ent": (n_ent, dim_e), "rel": (n_rel, dim_r), "rel_matrix": (n_rel, dim_e * dim_r)}
        self.tables: Dict[str, torch.Tensor] = {}
        for k, name in enumerate(TABLES):
            self.tables[name] = init_embeddings(*shapes[name], device=device, seed=None if base is None else base + k)
        dev = self.tables["ent"].device
        n = sum(t.numel() for t in self.tables.values())
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        self.t = 0
        self._ws: Optional[torch.Tensor] = None
        self._ws_B = -1
        self._loss = torch.empty(1, dtype=torch.float32, device=dev)

    def _ptrs(self):
        t = self.tables
        return (int(self.l1), t["ent"].data_ptr(), self.n_ent, t["rel"].data_ptr(), t["rel_matrix"].data_ptr(),
                self.n_rel, self.dim_e, self.dim_r)

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

    def workspace(self, B: int) -> torch.Tensor:
        if self._ws is None or self._ws_B != B:
            nbytes = _lib.load().ge_transr_step_workspace_bytes(self.n_ent, self.n_rel, self.dim_e, self.dim_r, int(B))
            if nbytes == 0:
                raise RuntimeError("ge_transr_step_workspace_bytes failed")
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.tables["ent"].device)
            self._ws_B = B
        return self._ws

    def score(self, triples: torch.Tensor) -> torch.Tensor:
        """D of every (h, t, r) row, [B] fp32 (NaN where an id is out of range)."""
        tb = _pairs(triples, "triples")
        out = torch.empty(tb.shape[0], dtype=torch.float32, device=tb.device)
        _lib.call("ge_transr_score", *self._ptrs(), tb.data_ptr(), tb.shape[0], out.data_ptr(), _stream())
        return out

    def step(self, pos: torch.Tensor, neg: torch.Tensor, margin: float, lr: float = 0.001, b1: float = BETA1,
             b2: float = BETA2, eps: float = EPSILON) -> torch.Tensor:
        """One Adam step (t -> t + 1) on sum max(D(pos) - D(neg) + margin, 0); returns that batch loss (device
        scalar, before the step).  neg must keep pos's relation column (as getBatch's negatives do)."""
        check_adam(lr, b1, b2, eps)
        pb, nb = _pairs(pos, "pos"), _pairs(neg, "neg")
        if pb.shape != nb.shape or pb.shape[0] == 0:
            raise ValueError("pos and neg must be non-empty and of the same shape")
        ws = self.workspace(pb.shape[0])
        _lib.call("ge_transr_adam_step", *self._ptrs(), self.m.data_ptr(), self.v.data_ptr(), pb.data_ptr(),
                  nb.data_ptr(), pb.shape[0], float(margin), float(lr), float(b1), float(b2), float(eps), self.t + 1,
                  self._loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        self.t += 1
        return self._loss[0].clone()

    def rank_counts(self, triples: torch.Tensor, cand_is_head: bool = False, known_off: torch.Tensor = None,
                    known_rc: torch.Tensor = None, return_scores: bool = False):
        """ge_transr_rank on the [B,3] rows as given: as TransX.rank_counts."""
        tb = _pairs(triples, "triples")
        return _rank_call("ge_transr_rank", self._ptrs(), _lib.load().ge_transr_rank_workspace_bytes(
            self.n_ent, self.n_rel, self.dim_e, self.dim_r, max(tb.shape[0], 1)), self.n_ent, tb, cand_is_head,
            known_off, known_rc, return_scores)

    def ranks(self, test, known=None, side: str = "tail", batch: int = None):
        """(raw, filtered) int64 rank arrays of the test triples over every entity: evaluate.translation_ranks."""
        from .evaluate import translation_ranks
        return translation_ranks(self, test, known, side=side, batch=batch)

    def state_dict(self) -> Dict[str, object]:
        return {"model": "transr", "l1": self.l1, "n_ent": self.n_ent, "n_rel": self.n_rel, "dim_e": self.dim_e,
                "dim_r": self.dim_r, "t": self.t, "m": self.m.detach().cpu().clone(), "v": self.v.detach().cpu().clone(),
                **{k: v.detach().cpu().clone() for k, v in self.tables.items()}}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        if state.get("model") != "transr":
            raise ValueError(f"state_dict is of model {state.get('model')!r}, not 'transr'")
        for key in ("n_ent", "n_rel", "dim_e", "dim_r"):
            if state[key] != getattr(self, key):
                raise ValueError(f"state_dict {key}={state[key]!r} does not match this model's {getattr(self, key)!r}")
        for name, t in list(self.tables.items()) + [("m", self.m), ("v", self.v)]:
            src = state[name]
            if tuple(src.shape) != tuple(t.shape):
                raise ValueError(f"state_dict tensor {name} has shape {tuple(src.shape)}, expected {tuple(t.shape)}")
        t = int(state["t"])
        if t < 0:
            raise ValueError(f"state_dict t={t} is negative")
        self.l1 = bool(state.get("l1", self.l1))
        for name, dst in list(self.tables.items()) + [("m", self.m), ("v", self.v)]:
            dst.copy_(state[name].to(device=dst.device, dtype=torch.float32))
        self.t = t

    def trainer(self, triples, batch_size: int, *, margin: float = 1.0, learning_rate: float = 0.001,
                seed: int = 0) -> "Trainer":
        return Trainer(self, triples, batch_size, margin=margin, learning_rate=learning_rate, seed=seed)


class Trainer:
    """transR.py's training loop (getBatch + train_step) as one native call per run(): each step draws
    `batch_size` positives uniformly with replacement from `triples`, corrupts each with the filtered Bernoulli
    rule (ent_lo = 0) and takes one Adam step.  Step s of the trainer uses the Philox counter (seed, s):
    ge_transx_draw_batch(.., seed, s, ..) reproduces any step's batch.  The Adam step count lives in the model."""

    def __init__(self, model: TransR, triples, batch_size: int, *, margin: float = 1.0, learning_rate: float = 0.001,
                 seed: int = 0, b1: float = BETA1, b2: float = BETA2, eps: float = EPSILON):
        tri = np.asarray(triples.cpu().numpy() if isinstance(triples, torch.Tensor) else triples, dtype=np.int64)
        if tri.ndim != 2 or tri.shape[1] != 3 or len(tri) == 0:
            raise ValueError("triples must be a non-empty [T, 3] (h, t, r) array")
        if tri[:, :2].min() < 0 or tri[:, :2].max() >= model.n_ent or tri[:, 2].min() < 0 or tri[:, 2].max() >= model.n_rel:
            raise ValueError("triples hold an id outside the model's tables")
        if batch_size <= 0:
            raise ValueError("batch_size must be positive")
        check_adam(learning_rate, b1, b2, eps)
        dev = model.tables["ent"].device
        self.model, self.B, self.margin, self.lr, self.seed = model, int(batch_size), float(margin), float(learning_rate), int(seed)
        self.b1, self.b2, self.eps = float(b1), float(b2), float(eps)
        self.triples = torch.as_tensor(tri.astype(np.int32)).to(dev).contiguous()
        self.sampler = BernoulliSampler(tri, model.n_rel, model.n_ent, device=dev, ent_lo=0)
        self.step_count = 0

    def draw(self, step: int):
        """The (pos, neg) batch the loop uses at `step`."""
        s = self.sampler
        pos = torch.empty(self.B, 3, dtype=torch.int32, device=self.triples.device)
        neg = torch.empty_like(pos)
        _lib.call("ge_transx_draw_batch", self.triples.data_ptr(), self.triples.shape[0], self.B, s.bh_key.data_ptr(),
                  s.bh_ent.data_ptr(), s.bt_key.data_ptr(), s.bt_ent.data_ptr(), s.n_known, s.tail_threshold.data_ptr(),
                  s.n_rel, s.n_ent, self.seed & (2**64 - 1), int(step) & (2**64 - 1), pos.data_ptr(), neg.data_ptr(),
                  _stream())
        return pos, neg

    def run(self, n: int) -> torch.Tensor:
        """n steps in one call; returns the [n] per-step batch losses (device)."""
        m, s = self.model, self.sampler
        losses = torch.empty(max(int(n), 0), dtype=torch.float32, device=self.triples.device)
        if n <= 0:
            return losses
        ws = m.workspace(self.B)
        _lib.call("ge_transr_train_steps", *m._ptrs(), m.m.data_ptr(), m.v.data_ptr(), self.triples.data_ptr(),
                  self.triples.shape[0], s.bh_key.data_ptr(), s.bh_ent.data_ptr(), s.bt_key.data_ptr(),
                  s.bt_ent.data_ptr(), s.n_known, s.tail_threshold.data_ptr(), self.seed & (2**64 - 1), self.step_count,
                  int(n), self.B, self.margin, self.lr, self.b1, self.b2, self.eps, m.t + 1, losses.data_ptr(),
                  ws.data_ptr(), ws.numel(), _stream())
        self.step_count += int(n)
        m.t += int(n)
        return losses
