"""Host-side mirror of the holE.py operator interface for the hot path, on libge_hip.so.

Same names, argument meaning and orientation as the reference functions (cited per function);
tensors are PyTorch-ROCm CUDA tensors instead of TF graph nodes, and every call enqueues hand-written
HIP kernels on torch's current stream through the C ABI of include/ge_hip.h.  PyTorch is plumbing
here (device memory, streams); there is no torch / CPU compute fallback.

Orientation reminder: E(h,t,r) = sigmoid(score) is a LOSS -- lower is more
plausible; the hinge max(E(pos) - E(neg) + margin, 0) pushes positive scores down.
"""
from __future__ import annotations

import types
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib

MODEL_COMPLEX, MODEL_HOLE, MODEL_HOLE_SPECTRAL, MODEL_HOLE_DIRECT = 0, 1, 2, 3
STEP_DETERMINISTIC = 0x100      # GE_STEP_DETERMINISTIC: OR-ed into the model code of ge_train_steps
_MODELS = {"complex": MODEL_COMPLEX, "hole": MODEL_HOLE, "hole_spectral": MODEL_HOLE_SPECTRAL,
           "hole_direct": MODEL_HOLE_DIRECT, 0: 0, 1: 1, 2: 2, 3: 3}

CORRUPT_BATCH_COIN, CORRUPT_ROW_COIN, CORRUPT_HEADS, CORRUPT_TAILS = 0, 1, 2, 3


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need_cuda(t: torch.Tensor, name: str):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA (ROCm) tensor: graphembeddings_amd has no CPU path")


def _table(embeddings: torch.Tensor):
    _need_cuda(embeddings, "embeddings")
    if embeddings.dtype != torch.float32 or embeddings.dim() != 2 or not embeddings.is_contiguous():
        raise ValueError("embeddings must be a contiguous float32 [entity_count, embedding_dim] tensor")
    return embeddings


def _triples(t: torch.Tensor, name="triple_batch") -> torch.Tensor:
    """[B,3] (head, tail, relation) (holE.py:181-185). int64 accepted (holE.py:547) and narrowed."""
    _need_cuda(t, name)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} must have shape [B, 3] (head, tail, relation)")
    if t.dtype != torch.int32:
        t = t.to(torch.int32)
    return t.contiguous()


def init_embeddings(entity_count: int, embedding_dim: int, device="cuda", seed: Optional[int] = None):
    """The `embeddings` variable of holE.py:263-264: xavier_initializer(uniform=False) =
    truncated normal (re-drawn beyond 2 sigma) with stddev sqrt(2.6 / (entity_count + dim)), drawn on the
    device (a 960 MB table is not built on the host and copied)."""
    dev = torch.device(device)
    gen = torch.Generator(device=dev)
    if seed is not None:
        gen.manual_seed(seed)
    std = float(np.sqrt(2.6 / (entity_count + embedding_dim)))
    t = torch.empty(entity_count, embedding_dim, dtype=torch.float32, device=dev)
    torch.nn.init.trunc_normal_(t, mean=0.0, std=std, a=-2 * std, b=2 * std, generator=gen)
    return t


def evaluate_triples(triple_batch: torch.Tensor, embeddings: torch.Tensor, label=None, *,
                     model="complex", max_norm: float = 1.0, apply_sigmoid: bool = True,
                     l2_regularization: float = 0.1) -> torch.Tensor:
    """holE.py:179-202 as [B,1].  label=None (hinge / inference branch): sigmoid(sum_k Re(h_k r_k conj(t_k))).
    label=+1 / -1 (the --log_loss branch, holE.py:194-196; FLAGS.l2_regularization becomes a keyword):
    log(1 + exp(-label * score)) + l2_regularization * l2_loss(embeddings), ComplEx score only.
    model="hole" gives the README.md:42 HolE score instead ("hole_spectral": on a spectral table)."""
    emb = _table(embeddings)
    tb = _triples(triple_batch)
    out = torch.empty(tb.shape[0], dtype=torch.float32, device=emb.device)
    if label is not None:
        if _MODELS[model] != MODEL_COMPLEX:
            raise NotImplementedError("the log-loss branch is defined for the ComplEx score (holE.py:191-196)")
        ws = torch.empty(256, dtype=torch.uint8, device=emb.device)
        _lib.call("ge_complex_logloss", emb.data_ptr(), emb.shape[0], emb.shape[1], tb.data_ptr(), tb.shape[0],
                  float(label), float(l2_regularization), max_norm, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        return out.view(-1, 1)
    fn = {MODEL_COMPLEX: "ge_complex_score", MODEL_HOLE: "ge_hole_score", MODEL_HOLE_DIRECT: "ge_hole_score",
          MODEL_HOLE_SPECTRAL: "ge_hole_spectral_score"}[_MODELS[model]]
    _lib.call(fn, emb.data_ptr(), emb.shape[0], emb.shape[1], tb.data_ptr(), tb.shape[0],
              max_norm, int(apply_sigmoid), out.data_ptr(), _stream())
    return out.view(-1, 1)


def hole_to_spectral(embeddings: torch.Tensor) -> torch.Tensor:
    """In place: every row of a HolE table -> its packed half spectrum (ge_hole_to_spectral).  On the
    result, model="hole_spectral" scores / trains README.md:42's HolE without any transform."""
    emb = _table(embeddings)
    _lib.call("ge_hole_to_spectral", emb.data_ptr(), emb.shape[0], emb.shape[1], _stream())
    return emb


def hole_from_spectral(embeddings: torch.Tensor) -> torch.Tensor:
    """In place inverse of hole_to_spectral."""
    emb = _table(embeddings)
    _lib.call("ge_hole_from_spectral", emb.data_ptr(), emb.shape[0], emb.shape[1], _stream())
    return emb


@dataclass
class TypeTables:
    """Device form of the two corruption tables of holE.py:267-277.

    id_to_type : int32 [entity_count] type code per table row (-1 unknown -> '?' default, holE.py:39)
    type_offsets / type_ids : CSR of type code -> ids (the full lists of data.type_to_ids; the
    per-batch padded_size subsample of holE.py:343-347 is drawn inside the kernel).
    """
    id_to_type: torch.Tensor
    type_offsets: torch.Tensor
    type_ids: torch.Tensor
    padded_size: int = 1024

    @staticmethod
    def from_host(id_to_type, type_offsets, type_ids, padded_size=1024, device="cuda") -> "TypeTables":
        return TypeTables(
            torch.as_tensor(np.ascontiguousarray(id_to_type, dtype=np.int32)).to(device),
            torch.as_tensor(np.ascontiguousarray(type_offsets, dtype=np.int64)).to(device),
            torch.as_tensor(np.ascontiguousarray(type_ids, dtype=np.int32)).to(device),
            int(padded_size))

    @property
    def n_types(self) -> int:
        return int(self.type_offsets.numel()) - 1

    def abi(self):
        """The tables as the C ABI takes them: (id_to_type, type_offsets, n_types, type_ids), pointers as integers."""
        return self.id_to_type.data_ptr(), self.type_offsets.data_ptr(), self.n_types, self.type_ids.data_ptr()


def corrupt_batch(type_tables: TypeTables, relation_count: int, triples: torch.Tensor, *, seed: int = 0,
                  step: int = 0, mode: int = CORRUPT_BATCH_COIN) -> torch.Tensor:
    """holE.py:152-153 (-> corrupt_entities 136-140 -> corrupt_heads/tails 97-133): type-safe
    corruption, [B,3] int32.  relation_count is unused, as in the reference (relation corruption is
    commented out, holE.py:154-158).  (seed, step) key the counter-based random stream."""
    tb = _triples(triples, "triples")
    _need_cuda(type_tables.id_to_type, "type tables")
    neg = torch.empty_like(tb)
    id_to_type, *rest = type_tables.abi()
    _lib.call("ge_corrupt_batch", tb.data_ptr(), tb.shape[0], id_to_type, type_tables.id_to_type.numel(), *rest,
              int(seed) & (2**64 - 1), int(step) & (2**64 - 1), type_tables.padded_size, int(mode), neg.data_ptr(), _stream())
    return neg


def hinge_loss(pos: torch.Tensor, neg: torch.Tensor, embeddings: torch.Tensor, *, margin: float = 0.2,
               model="complex", max_norm: float = 1.0, return_sigmoids: bool = False):
    """max(E(pos) - E(neg) + margin, 0) as [B,1] (holE.py:231) for given negatives."""
    emb = _table(embeddings)
    p, n = _triples(pos, "pos"), _triples(neg, "neg")
    if p.shape != n.shape:
        raise ValueError("pos and neg must have the same shape")
    B = p.shape[0]
    loss = torch.empty(B, dtype=torch.float32, device=emb.device)
    sig = torch.empty(2 * B, dtype=torch.float32, device=emb.device) if return_sigmoids else None
    _lib.call("ge_hinge_loss", emb.data_ptr(), emb.shape[0], emb.shape[1], p.data_ptr(), n.data_ptr(), B,
              margin, max_norm, _MODELS[model], loss.data_ptr(), sig.data_ptr() if sig is not None else None,
              _stream())
    if return_sigmoids:
        return loss.view(-1, 1), sig[:B].view(-1, 1), sig[B:].view(-1, 1)
    return loss.view(-1, 1)


def evaluate_batch(triple_batch: torch.Tensor, embeddings: torch.Tensor, type_to_ids_table: TypeTables,
                   id_to_type_table=None, relation_count: int = 0, *, margin: float = 0.2,
                   model="complex", seed: int = 0, step: int = 0, mode: int = CORRUPT_BATCH_COIN,
                   max_norm: float = 1.0) -> torch.Tensor:
    """holE.py:205-234 (hinge branch): corrupt the batch type-safely, score both, return the hinge
    [B,1].  The reference passes two hash tables; here both live in one TypeTables object
    (`id_to_type_table` is accepted and ignored)."""
    neg = corrupt_batch(type_to_ids_table, relation_count, triple_batch, seed=seed, step=step, mode=mode)
    return hinge_loss(triple_batch, neg, embeddings, margin=margin, model=model, max_norm=max_norm)


def inverse_time_decay(learning_rate: float, global_step: int, decay_steps: float, decay_rate: float) -> float:
    """tf.train.inverse_time_decay as called at holE.py:292-294 (no staircase)."""
    return learning_rate / (1.0 + decay_rate * (float(global_step) / float(decay_steps)))


class HingeSGD:
    """GradientDescentOptimizer(lr).minimize(loss) of holE.py:296 for the hinge of holE.py:231,
    fused on the GPU: gradient of SUM_i loss_i, then ScatterSub with duplicates accumulating.
    Owns the scratch workspace the C ABI needs."""

    def __init__(self, embeddings: torch.Tensor, batch_size: int, *, margin: float = 0.2,
                 model="complex", max_norm: float = 1.0):
        self.embeddings = _table(embeddings)
        self.margin, self.max_norm = float(margin), float(max_norm)
        self.model = _MODELS[model]
        self._ws = None
        self._turn = 0
        self._reserve(batch_size)

    # The gradient rows are written by one kernel and read by the next on other XCDs; rewriting a buffer whose
    # lines still sit in another XCD's L2 is the slow path (profiles/r01_xcd_locality_probe.txt), so small
    # workspaces are rotated (4 regions, the same trick as ge_train_steps); large ones evict themselves.
    _RING, _RING_MAX_BYTES = 4, 48 << 20

    def _reserve(self, B: int):
        need = max(_lib.load().ge_hinge_step_workspace_bytes(B, self.embeddings.shape[1]), 256)
        if self._ws is None or self._ws.shape[1] < need:
            ring = self._RING if need <= self._RING_MAX_BYTES else 1
            self._ws = torch.empty(ring, (need + 255) // 256 * 256, dtype=torch.uint8, device=self.embeddings.device)

    def step(self, pos: torch.Tensor, neg: torch.Tensor, lr: float) -> torch.Tensor:
        """One training step in place on the table; returns the per-pair hinge [B,1]."""
        emb = self.embeddings
        p, n = _triples(pos, "pos"), _triples(neg, "neg")
        if p.shape != n.shape:
            raise ValueError("pos and neg must have the same shape")
        B = p.shape[0]
        self._reserve(B)
        loss = torch.empty(B, dtype=torch.float32, device=emb.device)
        ws = self._ws[self._turn % self._ws.shape[0]]
        self._turn += 1
        if self.model == MODEL_HOLE_SPECTRAL:    # the two halves of the step through their own entry points
            gi = ws[:24 * B].view(torch.int32)
            off = (24 * B + 255) // 256 * 256
            gv = ws[off:off + 24 * B * emb.shape[1]].view(torch.float32).view(6 * B, emb.shape[1])
            _lib.call("ge_hinge_grad", emb.data_ptr(), emb.shape[0], emb.shape[1], p.data_ptr(), n.data_ptr(), B,
                      self.margin, float(lr), self.max_norm, self.model, loss.data_ptr(), gi.data_ptr(), gv.data_ptr(),
                      _stream())
            _lib.call("ge_scatter_add_rows", emb.data_ptr(), emb.shape[0], emb.shape[1], gi.data_ptr(), gv.data_ptr(),
                      6 * B, _stream())
            return loss.view(-1, 1)
        fn = "ge_complex_hinge_step" if self.model == MODEL_COMPLEX else "ge_hole_hinge_step"
        _lib.call(fn, emb.data_ptr(), emb.shape[0], emb.shape[1], p.data_ptr(), n.data_ptr(), B,
                  self.margin, float(lr), self.max_norm, loss.data_ptr(), ws.data_ptr(),
                  ws.numel(), _stream())
        return loss.view(-1, 1)


class LogLossSGD:
    """The --log_loss branch (holE.py:194-196, 206-220): logistic loss over the positives (label +1)
    and `negative_ratio` corrupted batches (label -1) plus l2_regularization * l2_loss(whole table),
    minimised by plain SGD on the SUM of the loss vector (holE.py:296)."""

    def __init__(self, embeddings: torch.Tensor, l2_regularization: float = 0.1, max_norm: float = 1.0):
        self.embeddings = _table(embeddings)
        self.l2, self.max_norm = float(l2_regularization), float(max_norm)
        self._ws = None

    def step(self, pos: torch.Tensor, negs, lr: float) -> torch.Tensor:
        """pos [B,3]; negs: [K,B,3] tensor or list of K [B,3] tensors.  Returns the loss vector
        [(1+K)*B, 1] in the reference's concat order (holE.py:220)."""
        emb = self.embeddings
        p = _triples(pos, "pos")
        if isinstance(negs, (list, tuple)):
            negs = torch.stack([_triples(n, "neg") for n in negs], 0)
        negs = negs.to(torch.int32).reshape(-1, 3)
        tri = torch.cat([p, negs], 0).contiguous()
        M, B = tri.shape[0], p.shape[0]
        labels = torch.ones(M, dtype=torch.float32, device=emb.device)
        labels[B:] = -1.0
        need = _lib.load().ge_logloss_step_workspace_bytes(M, emb.shape[1])
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=emb.device)
        loss = torch.empty(M, dtype=torch.float32, device=emb.device)
        _lib.call("ge_complex_logloss_step", emb.data_ptr(), emb.shape[0], emb.shape[1], tri.data_ptr(),
                  labels.data_ptr(), M, float(lr), self.l2, self.max_norm, loss.data_ptr(), self._ws.data_ptr(),
                  self._ws.numel(), _stream())
        return loss.view(-1, 1)


def hinge_grad(rows: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor, lr: float, *, margin=0.2,
               model="complex", max_norm=1.0):
    """First half of the step (ge_hinge_grad): returns (loss [B], grad_idx [6B] int32, grad_val [6B,d])
    with grad_val already multiplied by -lr.  `rows` may be a staging buffer of fetched rows."""
    rows = _table(rows)
    p, n = _triples(pos, "pos"), _triples(neg, "neg")
    B, d = p.shape[0], rows.shape[1]
    loss = torch.empty(B, dtype=torch.float32, device=rows.device)
    gi = torch.empty(6 * B, dtype=torch.int32, device=rows.device)
    gv = torch.empty(6 * B, d, dtype=torch.float32, device=rows.device)
    _lib.call("ge_hinge_grad", rows.data_ptr(), rows.shape[0], d, p.data_ptr(), n.data_ptr(), B, margin,
              float(lr), max_norm, _MODELS[model], loss.data_ptr(), gi.data_ptr(), gv.data_ptr(), _stream())
    return loss, gi, gv


def scatter_add_rows(table: torch.Tensor, idx: torch.Tensor, val: torch.Tensor) -> None:
    """table[idx[i]] += val[i] for idx[i] >= 0 (ScatterSub with the sign folded into val)."""
    table = _table(table)
    _need_cuda(idx, "idx"); _need_cuda(val, "val")
    idx = idx.to(torch.int32).contiguous()
    val = val.to(torch.float32).contiguous()
    if val.shape != (idx.numel(), table.shape[1]):
        raise ValueError("val must be [len(idx), embedding_dim]")
    _lib.call("ge_scatter_add_rows", table.data_ptr(), table.shape[0], table.shape[1], idx.data_ptr(),
              val.data_ptr(), idx.numel(), _stream())


def _accumulator(accumulator: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    _need_cuda(accumulator, "accumulator")
    if accumulator.dtype != torch.float32 or accumulator.shape != table.shape or not accumulator.is_contiguous():
        raise ValueError("accumulator must be a contiguous float32 tensor of the table's shape")
    return accumulator


def adagrad_rows(table: torch.Tensor, accumulator: torch.Tensor, idx: torch.Tensor, val: torch.Tensor, lr: float) -> None:
    """The AdaGrad counterpart of scatter_add_rows (ge_adagrad_rows; AdagradOptimizer at holE.py:296): `val` holds MINUS
    the gradient rows.  Per row named by idx >= 0: s = sum of its val rows, accumulator[row] += s*s,
    table[row] += lr * s / sqrt(accumulator[row]).  Rows not named are not touched."""
    table = _table(table)
    acc = _accumulator(accumulator, table)
    _need_cuda(idx, "idx"); _need_cuda(val, "val")
    idx = idx.to(torch.int32).contiguous()
    val = val.to(torch.float32).contiguous()
    if val.shape != (idx.numel(), table.shape[1]):
        raise ValueError("val must be [len(idx), embedding_dim]")
    # a row's occurrences consecutive and in their original order: the stable argsort, empty slots last
    key = torch.where(idx < 0, torch.full_like(idx, table.shape[0]), idx)
    perm = torch.argsort(key, stable=True).to(torch.int32)
    _lib.call("ge_adagrad_rows", table.data_ptr(), acc.data_ptr(), table.shape[0], table.shape[1], idx.data_ptr(),
              val.data_ptr(), perm.data_ptr(), idx.numel(), float(lr), _stream())


class HingeAdaGrad:
    """AdagradOptimizer(lr, initial_accumulator_value).minimize(loss) in place of the GradientDescentOptimizer of
    holE.py:296 for the hinge of holE.py:231: ge_hinge_grad at lr = 1 (minus the gradient of SUM_i loss_i as
    IndexedSlices), duplicates summed per row, then the AdaGrad update of every row named.  Owns `.accumulator`."""

    def __init__(self, embeddings: torch.Tensor, batch_size: int, *, margin: float = 0.2, model="complex",
                 max_norm: float = 1.0, initial_accumulator_value: float = 0.1):
        if not initial_accumulator_value > 0:
            raise ValueError("initial_accumulator_value must be positive")
        self.embeddings = _table(embeddings)
        if _MODELS[model] == MODEL_HOLE_SPECTRAL:
            raise ValueError("AdaGrad is elementwise: it does not commute with the DFT of a spectral HolE table")
        self.margin, self.max_norm, self.model = float(margin), float(max_norm), model
        self.accumulator = torch.full_like(self.embeddings, float(initial_accumulator_value))

    def step(self, pos: torch.Tensor, neg: torch.Tensor, lr: float) -> torch.Tensor:
        """One training step in place on the table and the accumulator; returns the per-pair hinge [B,1]."""
        loss, gi, gv = hinge_grad(self.embeddings, pos, neg, 1.0, margin=self.margin, model=self.model,
                                  max_norm=self.max_norm)
        adagrad_rows(self.embeddings, self.accumulator, gi, gv, lr)
        return loss.view(-1, 1)


def _softmax_args(embeddings, fixed_and_relation, true_ids, candidates, scale, max_norm, side, who):
    """The host checks of the softmax calls: (emb, hr [B,2] int32, true ids [B] int32, candidates [K] int32, side code)."""
    emb = _table(embeddings)
    for name, t in (("fixed_and_relation", fixed_and_relation), ("true_ids", true_ids), ("candidates", candidates)):
        _need_cuda(t, name)
    if side not in ("tail", "head"):
        raise ValueError(f"{who}: side must be 'tail' or 'head'")
    if not (scale > 0 and np.isfinite(scale)):
        raise ValueError(f"{who}: scale must be positive and finite")
    if not max_norm > 0:
        raise ValueError(f"{who}: max_norm must be positive")
    hr = fixed_and_relation.to(torch.int32).contiguous()
    tid = true_ids.to(torch.int32).contiguous().view(-1)
    cand = candidates.to(torch.int32).contiguous().view(-1)
    if hr.dim() != 2 or hr.shape[1] != 2 or tid.numel() != hr.shape[0]:
        raise ValueError(f"{who}: fixed_and_relation must be [B,2] (entity, relation) and true_ids [B]")
    if hr.shape[0] < 1 or cand.numel() < 1:
        raise ValueError(f"{who}: at least one query row and one candidate")
    d = emb.shape[1]
    if d % 8 != 0 or d < 8 or d > rank_max_dim():
        raise ValueError(f"{who}: embedding_dim must be a multiple of 8 in 8 ... {rank_max_dim()}")
    return emb, hr, tid, cand, int(side == "head")


def softmax_workspace(embeddings: torch.Tensor, B: int, K: int) -> torch.Tensor:
    """A workspace for softmax_loss / softmax_grad at this shape (ge_softmax_workspace_bytes)."""
    need = _lib.load().ge_softmax_workspace_bytes(B, K, embeddings.shape[1])
    return torch.empty(max(need, 256), dtype=torch.uint8, device=embeddings.device)


def softmax_masked_workspace(embeddings: torch.Tensor, B: int, K: int) -> torch.Tensor:
    """A workspace for softmax_loss / softmax_grad with candidate_sets at this shape (ge_softmax_masked_workspace_bytes)."""
    need = _lib.load().ge_softmax_masked_workspace_bytes(B, K, embeddings.shape[1])
    return torch.empty(max(need, 256), dtype=torch.uint8, device=embeddings.device)


def softmax_loss(embeddings: torch.Tensor, fixed_and_relation: torch.Tensor, true_ids: torch.Tensor,
                 candidates: torch.Tensor, *, scale: float, max_norm: float = 1.0, side: str = "tail",
                 workspace: Optional[torch.Tensor] = None, candidate_sets=None, row_sets=None) -> torch.Tensor:
    """The 1-vs-all objective (ge_softmax_loss): loss_i = logsumexp_j(-scale * s_ij) - (-scale * s_i,true) over all
    `candidates` (distinct ids), s the ComplEx score of score_candidates without the sigmoid.  side="tail": row i is
    (head_i, relation_i) and the candidates are tails; "head": (tail_i, relation_i), candidates are heads.  NaN for a row
    with an id outside the table or whose true id is not a candidate.  ComplEx only.
    candidate_sets (an evaluate.CandidateSets built for these very `candidates` and this side) / row_sets ([B], default
    the row's relation id; -1: unrestricted): ge_softmax_masked_loss -- row i's softmax runs over the candidates its set
    admits, and a row whose true candidate is inadmissible is NaN too.  The workspace is then softmax_masked_workspace's."""
    emb, hr, tid, cand, head = _softmax_args(embeddings, fixed_and_relation, true_ids, candidates, scale, max_norm, side,
                                             "softmax_loss")
    B, K = hr.shape[0], cand.numel()
    sets, _rs = _sets_args(candidate_sets, row_sets, hr, cand, "softmax_loss")
    loss = torch.empty(B, dtype=torch.float32, device=emb.device)
    if sets:
        ws = workspace if workspace is not None else softmax_masked_workspace(emb, B, K)
        _lib.call("ge_softmax_masked_loss", emb.data_ptr(), emb.shape[0], emb.shape[1], hr.data_ptr(), B, tid.data_ptr(),
                  cand.data_ptr(), K, float(max_norm), float(scale), MODEL_COMPLEX, head, loss.data_ptr(), ws.data_ptr(),
                  ws.numel(), *sets, _stream())
        return loss
    ws = workspace if workspace is not None else softmax_workspace(emb, B, K)
    _lib.call("ge_softmax_loss", emb.data_ptr(), emb.shape[0], emb.shape[1], hr.data_ptr(), B, tid.data_ptr(), cand.data_ptr(),
              K, float(max_norm), float(scale), MODEL_COMPLEX, head, loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return loss


def softmax_grad(embeddings: torch.Tensor, fixed_and_relation: torch.Tensor, true_ids: torch.Tensor,
                 candidates: torch.Tensor, lr: float, *, scale: float, max_norm: float = 1.0, side: str = "tail",
                 workspace: Optional[torch.Tensor] = None, out=None, candidate_sets=None, row_sets=None):
    """The counterpart of hinge_grad for the 1-vs-all objective (ge_softmax_grad): (loss [B], grad_idx [K + 2B] int32,
    grad_val [K + 2B, d]) with grad_val = -lr * the gradient of SUM_i loss_i.  Slot j < K is candidates[j], slots K + 2i
    and K + 2i + 1 the fixed entity and the relation of row i; -1 and a zero row for an empty slot.  out: (grad_idx,
    grad_val) views to write into.
    candidate_sets / row_sets (as softmax_loss takes them): ge_softmax_masked_grad, same slots; a candidate that no valid
    row admits keeps its id and gets an exact zero row."""
    emb, hr, tid, cand, head = _softmax_args(embeddings, fixed_and_relation, true_ids, candidates, scale, max_norm, side,
                                             "softmax_grad")
    B, K, d = hr.shape[0], cand.numel(), emb.shape[1]
    R = K + 2 * B
    sets, _rs = _sets_args(candidate_sets, row_sets, hr, cand, "softmax_grad")
    if workspace is not None:
        ws = workspace
    else:
        ws = softmax_masked_workspace(emb, B, K) if sets else softmax_workspace(emb, B, K)
    loss = torch.empty(B, dtype=torch.float32, device=emb.device)
    if out is None:
        gi = torch.empty(R, dtype=torch.int32, device=emb.device)
        gv = torch.empty(R, d, dtype=torch.float32, device=emb.device)
    else:
        gi, gv = out
        if gi.dtype != torch.int32 or gv.dtype != torch.float32 or gi.numel() != R or tuple(gv.shape) != (R, d) \
                or not gi.is_contiguous() or not gv.is_contiguous():
            raise ValueError("softmax_grad: out must be (int32 [K + 2B], float32 [K + 2B, d]), contiguous")
    if sets:
        _lib.call("ge_softmax_masked_grad", emb.data_ptr(), emb.shape[0], d, hr.data_ptr(), B, tid.data_ptr(), cand.data_ptr(),
                  K, float(max_norm), float(scale), float(lr), MODEL_COMPLEX, head, loss.data_ptr(), gi.data_ptr(),
                  gv.data_ptr(), ws.data_ptr(), ws.numel(), *sets, _stream())
        return loss, gi, gv
    _lib.call("ge_softmax_grad", emb.data_ptr(), emb.shape[0], d, hr.data_ptr(), B, tid.data_ptr(), cand.data_ptr(), K,
              float(max_norm), float(scale), float(lr), MODEL_COMPLEX, head, loss.data_ptr(), gi.data_ptr(), gv.data_ptr(),
              ws.data_ptr(), ws.numel(), _stream())
    return loss, gi, gv


class SoftmaxAdaGrad:
    """AdagradOptimizer(lr, initial_accumulator_value) on the 1-vs-all objective, both sides of every triple against ONE
    snapshot of the table: two ge_softmax_grad calls at lr = 1 (tails, then heads) into one slices buffer of
    2 (K + 2B) slots, one stable argsort, one ge_adagrad_rows -- an entity that is a candidate, a tail and a head in the
    same step gets one update from its summed gradient.  Owns `.accumulator`; workspace and slices are reserved once.

    candidate_sets={"tail": sets, "head": sets} (evaluate.CandidateSets built for `candidates`, one per side): the
    type-constrained objective (ge_softmax_masked_grad).  The step then orders the batch rows by set id (a stable sort) before
    the two gradient calls, so that the rows of a 64-row tile share sets and the tile pairs nobody admits are skipped;
    the losses come back in the caller's order."""

    def __init__(self, embeddings: torch.Tensor, candidates: torch.Tensor, batch_size: int, *, scale: float,
                 max_norm: float = 1.0, initial_accumulator_value: float = 0.1, candidate_sets=None):
        if not initial_accumulator_value > 0:
            raise ValueError("initial_accumulator_value must be positive")
        self.embeddings = _table(embeddings)
        _need_cuda(candidates, "candidates")
        self.candidates = candidates.to(torch.int32).contiguous().view(-1)
        self.B, self.scale, self.max_norm = int(batch_size), float(scale), float(max_norm)
        if self.B < 1 or self.candidates.numel() < 1:
            raise ValueError("SoftmaxAdaGrad: at least one row a batch and one candidate")
        dev, d = self.embeddings.device, self.embeddings.shape[1]
        self.accumulator = torch.full_like(self.embeddings, float(initial_accumulator_value))
        R = self.candidates.numel() + 2 * self.B
        self.candidate_sets, self._sets = candidate_sets, {}
        if candidate_sets is not None:
            if not isinstance(candidate_sets, dict) or any(s not in candidate_sets for s in ("tail", "head")):
                raise ValueError("SoftmaxAdaGrad: candidate_sets must be a dict with a CandidateSets per side ('tail', 'head')")
            # checked against the candidates once, here: the step's calls then see the optimizer's own tensor
            for side in ("tail", "head"):
                cs = candidate_sets[side]
                _sets_args(cs, None, torch.zeros(1, 2, dtype=torch.int32, device=dev), self.candidates, "SoftmaxAdaGrad")
                self._sets[side] = types.SimpleNamespace(mask=cs.mask, n_sets=int(cs.n_sets), cand=self.candidates)
            self._ws = softmax_masked_workspace(self.embeddings, self.B, self.candidates.numel())
        else:
            self._ws = softmax_workspace(self.embeddings, self.B, self.candidates.numel())
        self._gi = torch.empty(2 * R, dtype=torch.int32, device=dev)
        self._gv = torch.empty(2 * R, d, dtype=torch.float32, device=dev)

    def step(self, triples: torch.Tensor, lr: float, row_sets=None) -> torch.Tensor:
        """One step in place on the table and the accumulator for triples [B,3] (head, tail, relation); returns the
        per-row losses [B,2] (tail side, head side).  row_sets ([B], with candidate_sets only; default the rows' relation
        ids): the set of each row, the same on both sides."""
        emb = self.embeddings
        tri = _triples(triples, "triples")
        if tri.shape[0] != self.B:
            raise ValueError("SoftmaxAdaGrad.step: triples must be [batch_size, 3]")
        R = self.candidates.numel() + 2 * self.B
        order, rs = None, None
        if self.candidate_sets is None:
            if row_sets is not None:
                raise ValueError("SoftmaxAdaGrad.step: row_sets without candidate_sets")
        else:
            rs = tri[:, 2] if row_sets is None else torch.as_tensor(row_sets).to(tri.device)
            if rs.dim() != 1 or rs.numel() != self.B or rs.dtype.is_floating_point:
                raise ValueError("SoftmaxAdaGrad.step: row_sets must be [B] integers")
            order = torch.argsort(rs, stable=True)
            tri, rs = tri[order].contiguous(), rs[order].contiguous()
        losses = []
        for s, (fixed, true, side) in enumerate(((0, 1, "tail"), (1, 0, "head"))):
            hr = tri[:, [fixed, 2]].contiguous()
            sets = self._sets.get(side)
            loss, _, _ = softmax_grad(emb, hr, tri[:, true].contiguous(), self.candidates, 1.0, scale=self.scale,
                                      max_norm=self.max_norm, side=side, workspace=self._ws,
                                      out=(self._gi[s * R:(s + 1) * R], self._gv[s * R:(s + 1) * R]),
                                      candidate_sets=sets, row_sets=rs)
            if order is not None:
                loss = torch.empty_like(loss).index_copy_(0, order, loss)
            losses.append(loss)
        # a row's occurrences consecutive and in slot order: the stable argsort, empty slots last (adagrad_rows)
        key = torch.where(self._gi < 0, torch.full_like(self._gi, emb.shape[0]), self._gi)
        perm = torch.argsort(key, stable=True).to(torch.int32)
        _lib.call("ge_adagrad_rows", emb.data_ptr(), _accumulator(self.accumulator, emb).data_ptr(), emb.shape[0],
                  emb.shape[1], self._gi.data_ptr(), self._gv.data_ptr(), perm.data_ptr(), 2 * R, float(lr), _stream())
        return torch.stack(losses, 1)


class QueryLabels:
    """The rows of the multi-label objective for one side: the distinct queries (fixed, relation) of `triples` and, per
    query, the candidate POSITIONS of all its known answers, as a CSR on the device.
    queries [Q,2] int32, label_off [Q + 1] int64, label_pos [sum n_i] int32 (ascending and distinct within a query)."""

    def __init__(self, queries: torch.Tensor, label_off: torch.Tensor, label_pos: torch.Tensor, side: str):
        self.queries, self.label_off, self.label_pos, self.side = queries, label_off, label_pos, side
        self.counts = label_off[1:] - label_off[:-1]

    def __len__(self) -> int:
        return self.queries.shape[0]

    @classmethod
    def from_triples(cls, triples: torch.Tensor, candidates: torch.Tensor, side: str) -> "QueryLabels":
        """side="tail": the queries are (head, relation) and the answers tails; "head": (tail, relation), answers heads.
        `candidates` are distinct ids; a triple whose answer is none of them is refused."""
        if side not in ("tail", "head"):
            raise ValueError("QueryLabels: side must be 'tail' or 'head'")
        tri = _triples(triples, "triples").to(torch.int64)
        _need_cuda(candidates, "candidates")
        cand = candidates.to(torch.int64).view(-1)
        K = cand.numel()
        if tri.shape[0] < 1 or K < 1:
            raise ValueError("QueryLabels: at least one triple and one candidate")
        if int(tri.min()) < 0 or int(cand.min()) < 0:
            raise ValueError("QueryLabels: negative ids")
        fixed, answer, rel = tri[:, 0 if side == "tail" else 1], tri[:, 1 if side == "tail" else 0], tri[:, 2]
        where = torch.full((int(max(cand.max(), answer.max())) + 1,), -1, dtype=torch.int64, device=tri.device)
        where[cand] = torch.arange(K, device=tri.device)
        if int((where >= 0).sum()) != K:
            raise ValueError("QueryLabels: candidates must be distinct")
        pos = where[answer]
        if bool((pos < 0).any()):
            raise ValueError("QueryLabels: a triple's answer is not among the candidates")
        n_rel = int(rel.max()) + 1
        # one key per (query, position), sorted and distinct: the queries in (fixed, relation) order, each one's positions ascending
        pair = torch.unique((fixed * n_rel + rel) * K + pos)
        qkey, counts = torch.unique_consecutive(torch.div(pair, K, rounding_mode="floor"), return_counts=True)
        off = torch.zeros(qkey.numel() + 1, dtype=torch.int64, device=tri.device)
        off[1:] = torch.cumsum(counts, 0)
        queries = torch.stack([torch.div(qkey, n_rel, rounding_mode="floor"), qkey % n_rel], 1).to(torch.int32)
        return cls(queries.contiguous(), off, (pair % K).to(torch.int32).contiguous(), side)

    def take(self, rows: torch.Tensor):
        """(hr [b,2] int32, label_off [b + 1] int32, label_pos [L] int32) of the queries `rows` (indices on the device), in
        that order.  The host waits once, for L."""
        rows = rows.to(torch.int64).view(-1)
        n = self.counts[rows]
        off = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=rows.device)
        off[1:] = torch.cumsum(n, 0)
        L = int(off[-1])
        src = torch.repeat_interleave(self.label_off[rows] - off[:-1], n, output_size=L) + torch.arange(L, device=rows.device)
        return self.queries[rows].contiguous(), off.to(torch.int32), self.label_pos[src].contiguous()


def _labels_args(fixed_and_relation, label_off, label_pos, who):
    for name, t in (("fixed_and_relation", fixed_and_relation), ("label_off", label_off), ("label_pos", label_pos)):
        _need_cuda(t, name)
    off = label_off.to(torch.int32).contiguous().view(-1)
    pos = label_pos.to(torch.int32).contiguous().view(-1)
    if off.numel() != fixed_and_relation.shape[0] + 1:
        raise ValueError(f"{who}: label_off must be [B + 1]")
    return off, pos


def softmax_labels_workspace(embeddings: torch.Tensor, B: int, K: int, L: int) -> torch.Tensor:
    """A workspace for softmax_labels_loss / softmax_labels_grad at this shape (ge_softmax_labels_workspace_bytes)."""
    need = _lib.load().ge_softmax_labels_workspace_bytes(B, K, embeddings.shape[1], L)
    return torch.empty(max(need, 256), dtype=torch.uint8, device=embeddings.device)


def softmax_labels_loss(embeddings: torch.Tensor, fixed_and_relation: torch.Tensor, label_off: torch.Tensor,
                        label_pos: torch.Tensor, candidates: torch.Tensor, *, scale: float, max_norm: float = 1.0,
                        side: str = "tail", workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The multi-label (K-vs-all) objective (ge_softmax_labels_loss): row i is a query (fixed, relation) whose labels are the
    candidate positions label_pos[label_off[i] : label_off[i + 1]], n_i of them, and
    loss_i = logsumexp_j(-scale * s_ij) - mean over the labels of (-scale * s_i,l).  NaN for a row with an id outside the
    table, without labels, or with a label that is no position of a candidate in the table.  ComplEx only."""
    off, pos = _labels_args(fixed_and_relation, label_off, label_pos, "softmax_labels_loss")
    # (the offsets behind the first stand in for the true ids of the shared checks: one per row)
    emb, hr, _, cand, head = _softmax_args(embeddings, fixed_and_relation, off[1:], candidates, scale, max_norm, side,
                                           "softmax_labels_loss")
    B, K, L = hr.shape[0], cand.numel(), pos.numel()
    ws = workspace if workspace is not None else softmax_labels_workspace(emb, B, K, L)
    loss = torch.empty(B, dtype=torch.float32, device=emb.device)
    _lib.call("ge_softmax_labels_loss", emb.data_ptr(), emb.shape[0], emb.shape[1], hr.data_ptr(), B, off.data_ptr(),
              pos.data_ptr() if L else off.data_ptr(), L, cand.data_ptr(), K, float(max_norm), float(scale), MODEL_COMPLEX,
              head, loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return loss


def softmax_labels_grad(embeddings: torch.Tensor, fixed_and_relation: torch.Tensor, label_off: torch.Tensor,
                        label_pos: torch.Tensor, candidates: torch.Tensor, lr: float, *, scale: float, max_norm: float = 1.0,
                        side: str = "tail", workspace: Optional[torch.Tensor] = None, out=None):
    """The gradients of softmax_labels_loss (ge_softmax_labels_grad): (loss [B], grad_idx [K + 2B + L] int32, grad_val
    [K + 2B + L, d]) with grad_val = -lr * the gradient of SUM_i loss_i.  Slot j < K is candidates[j] with the softmax term of
    its gradient, slots K + 2i and K + 2i + 1 the fixed entity and the relation of row i, slot K + 2B + x the candidate of
    label entry x with the label term of its gradient; -1 and a zero row for an empty slot.  The slices of one table row
    sum to its gradient.  out: (grad_idx, grad_val) views to write into."""
    off, pos = _labels_args(fixed_and_relation, label_off, label_pos, "softmax_labels_grad")
    # (the offsets behind the first stand in for the true ids of the shared checks: one per row)
    emb, hr, _, cand, head = _softmax_args(embeddings, fixed_and_relation, off[1:], candidates, scale, max_norm, side,
                                           "softmax_labels_grad")
    B, K, L, d = hr.shape[0], cand.numel(), pos.numel(), emb.shape[1]
    R = K + 2 * B + L
    ws = workspace if workspace is not None else softmax_labels_workspace(emb, B, K, L)
    loss = torch.empty(B, dtype=torch.float32, device=emb.device)
    if out is None:
        gi = torch.empty(R, dtype=torch.int32, device=emb.device)
        gv = torch.empty(R, d, dtype=torch.float32, device=emb.device)
    else:
        gi, gv = out
        if gi.dtype != torch.int32 or gv.dtype != torch.float32 or gi.numel() != R or tuple(gv.shape) != (R, d) \
                or not gi.is_contiguous() or not gv.is_contiguous():
            raise ValueError("softmax_labels_grad: out must be (int32 [K + 2B + L], float32 [K + 2B + L, d]), contiguous")
    _lib.call("ge_softmax_labels_grad", emb.data_ptr(), emb.shape[0], d, hr.data_ptr(), B, off.data_ptr(),
              pos.data_ptr() if L else off.data_ptr(), L, cand.data_ptr(), K, float(max_norm), float(scale), float(lr),
              MODEL_COMPLEX, head, loss.data_ptr(), gi.data_ptr(), gv.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return loss, gi, gv


class LabelSoftmaxAdaGrad:
    """SoftmaxAdaGrad on the multi-label objective: per step a batch of tail-side queries and one of head-side queries,
    each (hr [b,2], label_off [b + 1], label_pos [L]) as QueryLabels.take gives them, with b <= batch_size and
    L <= max_labels a side (a side may be None: no rows).  Two ge_softmax_labels_grad calls at lr = 1 (tails, then heads)
    against ONE snapshot of the table into one slices buffer, one stable argsort, one ge_adagrad_rows.  Owns
    `.accumulator`; workspace and slices are reserved once, for the largest step."""

    def __init__(self, embeddings: torch.Tensor, candidates: torch.Tensor, batch_size: int, max_labels: int, *, scale: float,
                 max_norm: float = 1.0, initial_accumulator_value: float = 0.1):
        if not initial_accumulator_value > 0:
            raise ValueError("initial_accumulator_value must be positive")
        self.embeddings = _table(embeddings)
        _need_cuda(candidates, "candidates")
        self.candidates = candidates.to(torch.int32).contiguous().view(-1)
        self.B, self.L, self.scale, self.max_norm = int(batch_size), int(max_labels), float(scale), float(max_norm)
        if self.B < 1 or self.L < 1 or self.candidates.numel() < 1:
            raise ValueError("LabelSoftmaxAdaGrad: at least one row a batch, one label and one candidate")
        dev, d = self.embeddings.device, self.embeddings.shape[1]
        self.accumulator = torch.full_like(self.embeddings, float(initial_accumulator_value))
        R = self.candidates.numel() + 2 * self.B + self.L
        self._ws = softmax_labels_workspace(self.embeddings, self.B, self.candidates.numel(), self.L)
        self._gi = torch.empty(2 * R, dtype=torch.int32, device=dev)
        self._gv = torch.empty(2 * R, d, dtype=torch.float32, device=dev)

    def step(self, tail_batch, head_batch, lr: float):
        """One step in place on the table and the accumulator; returns (tail losses [b_tail] or None, head losses [b_head]
        or None)."""
        emb, K = self.embeddings, self.candidates.numel()
        at, losses = 0, []
        for batch, side in ((tail_batch, "tail"), (head_batch, "head")):
            if batch is None or batch[0].shape[0] == 0:
                losses.append(None)
                continue
            hr, off, pos = batch
            b, L = hr.shape[0], pos.numel()
            if b > self.B or L > self.L:
                raise ValueError("LabelSoftmaxAdaGrad.step: more rows than batch_size or more labels than max_labels")
            R = K + 2 * b + L
            loss, _, _ = softmax_labels_grad(emb, hr, off, pos, self.candidates, 1.0, scale=self.scale, max_norm=self.max_norm,
                                             side=side, workspace=self._ws, out=(self._gi[at:at + R], self._gv[at:at + R]))
            losses.append(loss)
            at += R
        if at == 0:
            raise ValueError("LabelSoftmaxAdaGrad.step: no rows on either side")
        gi = self._gi[:at]
        # a row's occurrences consecutive and in slot order: the stable argsort, empty slots last (adagrad_rows)
        key = torch.where(gi < 0, torch.full_like(gi, emb.shape[0]), gi)
        perm = torch.argsort(key, stable=True).to(torch.int32)
        _lib.call("ge_adagrad_rows", emb.data_ptr(), _accumulator(self.accumulator, emb).data_ptr(), emb.shape[0],
                  emb.shape[1], gi.data_ptr(), self._gv.data_ptr(), perm.data_ptr(), at, float(lr), _stream())
        return tuple(losses)


def softmax_sampled_workspace(embeddings: torch.Tensor, B: int, K: int) -> torch.Tensor:
    """A workspace for softmax_sampled_loss / softmax_sampled_grad at this shape (ge_softmax_sampled_workspace_bytes)."""
    need = _lib.load().ge_softmax_sampled_workspace_bytes(B, K, embeddings.shape[1])
    return torch.empty(max(need, 256), dtype=torch.uint8, device=embeddings.device)


def softmax_sampled_loss(embeddings: torch.Tensor, fixed_and_relation: torch.Tensor, true_ids: torch.Tensor,
                         candidates: torch.Tensor, *, scale: float, max_norm: float = 1.0, side: str = "tail",
                         workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sampled softmax with shared negatives (ge_softmax_sampled_loss): softmax_loss over `candidates` that need not hold
    the true entity and may repeat.  The true entity has a logit of its own and every slot that holds it is left out of
    the row's softmax: loss_i = log(exp(z_i,true) + sum_{j: cand_j != true_i} exp(z_ij)) - z_i,true.  NaN for a row with an
    id outside the table.  ComplEx only."""
    emb, hr, tid, cand, head = _softmax_args(embeddings, fixed_and_relation, true_ids, candidates, scale, max_norm, side,
                                             "softmax_sampled_loss")
    B, K = hr.shape[0], cand.numel()
    ws = workspace if workspace is not None else softmax_sampled_workspace(emb, B, K)
    loss = torch.empty(B, dtype=torch.float32, device=emb.device)
    _lib.call("ge_softmax_sampled_loss", emb.data_ptr(), emb.shape[0], emb.shape[1], hr.data_ptr(), B, tid.data_ptr(),
              cand.data_ptr(), K, float(max_norm), float(scale), MODEL_COMPLEX, head, loss.data_ptr(), ws.data_ptr(),
              ws.numel(), _stream())
    return loss


def softmax_sampled_grad(embeddings: torch.Tensor, fixed_and_relation: torch.Tensor, true_ids: torch.Tensor,
                         candidates: torch.Tensor, lr: float, *, scale: float, max_norm: float = 1.0, side: str = "tail",
                         workspace: Optional[torch.Tensor] = None, out=None):
    """The gradients of softmax_sampled_loss (ge_softmax_sampled_grad): (loss [B], grad_idx [K + 3B] int32, grad_val
    [K + 3B, d]) with grad_val = -lr * the gradient of SUM_i loss_i.  Slot j < K is candidates[j]; slots K + 3i, K + 3i + 1
    and K + 3i + 2 the fixed entity, the relation and the true entity of row i; -1 and a zero row for an empty slot.
    out: (grad_idx, grad_val) views to write into."""
    emb, hr, tid, cand, head = _softmax_args(embeddings, fixed_and_relation, true_ids, candidates, scale, max_norm, side,
                                             "softmax_sampled_grad")
    B, K, d = hr.shape[0], cand.numel(), emb.shape[1]
    R = K + 3 * B
    ws = workspace if workspace is not None else softmax_sampled_workspace(emb, B, K)
    loss = torch.empty(B, dtype=torch.float32, device=emb.device)
    if out is None:
        gi = torch.empty(R, dtype=torch.int32, device=emb.device)
        gv = torch.empty(R, d, dtype=torch.float32, device=emb.device)
    else:
        gi, gv = out
        if gi.dtype != torch.int32 or gv.dtype != torch.float32 or gi.numel() != R or tuple(gv.shape) != (R, d) \
                or not gi.is_contiguous() or not gv.is_contiguous():
            raise ValueError("softmax_sampled_grad: out must be (int32 [K + 3B], float32 [K + 3B, d]), contiguous")
    _lib.call("ge_softmax_sampled_grad", emb.data_ptr(), emb.shape[0], d, hr.data_ptr(), B, tid.data_ptr(), cand.data_ptr(), K,
              float(max_norm), float(scale), float(lr), MODEL_COMPLEX, head, loss.data_ptr(), gi.data_ptr(), gv.data_ptr(),
              ws.data_ptr(), ws.numel(), _stream())
    return loss, gi, gv


class SampledSoftmaxAdaGrad:
    """SoftmaxAdaGrad on the sampled objective: per step `n_samples` candidates, shared by all rows and both sides.  Two
    ge_softmax_sampled_grad calls at lr = 1 (tails, then heads) against the same candidates and ONE snapshot of the table
    into one slices buffer of 2 (n_samples + 3B) slots, one stable argsort, one ge_adagrad_rows.  Owns `.accumulator`;
    workspace and slices are reserved once."""

    def __init__(self, embeddings: torch.Tensor, batch_size: int, n_samples: int, *, scale: float, max_norm: float = 1.0,
                 initial_accumulator_value: float = 0.1):
        if not initial_accumulator_value > 0:
            raise ValueError("initial_accumulator_value must be positive")
        self.embeddings = _table(embeddings)
        self.B, self.K, self.scale, self.max_norm = int(batch_size), int(n_samples), float(scale), float(max_norm)
        if self.B < 1 or self.K < 1:
            raise ValueError("SampledSoftmaxAdaGrad: at least one row a batch and one sample")
        dev, d = self.embeddings.device, self.embeddings.shape[1]
        self.accumulator = torch.full_like(self.embeddings, float(initial_accumulator_value))
        R = self.K + 3 * self.B
        self._ws = softmax_sampled_workspace(self.embeddings, self.B, self.K)
        self._gi = torch.empty(2 * R, dtype=torch.int32, device=dev)
        self._gv = torch.empty(2 * R, d, dtype=torch.float32, device=dev)

    def step(self, triples: torch.Tensor, candidates: torch.Tensor, lr: float) -> torch.Tensor:
        """One step in place on the table and the accumulator for triples [B,3] (head, tail, relation) against
        candidates [n_samples]; returns the per-row losses [B,2] (tail side, head side)."""
        emb = self.embeddings
        tri = _triples(triples, "triples")
        if tri.shape[0] != self.B:
            raise ValueError("SampledSoftmaxAdaGrad.step: triples must be [batch_size, 3]")
        _need_cuda(candidates, "candidates")
        cand = candidates.to(torch.int32).contiguous().view(-1)
        if cand.numel() != self.K:
            raise ValueError("SampledSoftmaxAdaGrad.step: candidates must be [n_samples]")
        R = self.K + 3 * self.B
        losses = []
        for s, (fixed, true, side) in enumerate(((0, 1, "tail"), (1, 0, "head"))):
            hr = tri[:, [fixed, 2]].contiguous()
            loss, _, _ = softmax_sampled_grad(emb, hr, tri[:, true].contiguous(), cand, 1.0, scale=self.scale,
                                              max_norm=self.max_norm, side=side, workspace=self._ws,
                                              out=(self._gi[s * R:(s + 1) * R], self._gv[s * R:(s + 1) * R]))
            losses.append(loss)
        # a row's occurrences consecutive and in slot order: the stable argsort, empty slots last (adagrad_rows)
        key = torch.where(self._gi < 0, torch.full_like(self._gi, emb.shape[0]), self._gi)
        perm = torch.argsort(key, stable=True).to(torch.int32)
        _lib.call("ge_adagrad_rows", emb.data_ptr(), _accumulator(self.accumulator, emb).data_ptr(), emb.shape[0],
                  emb.shape[1], self._gi.data_ptr(), self._gv.data_ptr(), perm.data_ptr(), 2 * R, float(lr), _stream())
        return torch.stack(losses, 1)


class SoftmaxTrainer:
    """The training loop of the 1-vs-all objective: per step a batch of `triples` [T,3] (head, tail, relation) drawn on
    the device -- without replacement within an epoch, every epoch a new permutation from a generator seeded with
    `seed` --, lr from inverse_time_decay as in Trainer, one SoftmaxAdaGrad.step.  A Python loop: a step is milliseconds
    of GPU work, which the host's few launches per step stay ahead of.

    n_samples: the sampled objective (SampledSoftmaxAdaGrad).  `candidates` is then the pool: every step draws
    pool[randint(len(pool), n_samples)], with replacement, one draw for both sides, from a second generator seeded with
    seed + 1 -- so the batches are the ones drawn without sampling.

    candidate_sets ({"tail": sets, "head": sets}, without n_samples): passed through to SoftmaxAdaGrad; every row's set is
    its relation id.

    labels="all" (without n_samples or candidate_sets): the multi-label objective (LabelSoftmaxAdaGrad).  The rows are the
    distinct QUERIES of both sides (QueryLabels.from_triples, built once), each with all its answers in `triples` as
    labels.  An epoch is one permutation of all Q_tail + Q_head queries from the seeded generator; a step takes the next
    batch_size of them and splits them by side (a side without rows is skipped); the last short batch is dropped.  The
    step's losses come back as one [batch_size] tensor, tail-side rows first."""

    def __init__(self, embeddings: torch.Tensor, triples: torch.Tensor, candidates: torch.Tensor, batch_size: int, *,
                 scale: float, learning_rate: float = 0.1, learning_decay_steps: float = 0.0,
                 learning_decay_rate: float = 0.5, seed: int = 0, max_norm: float = 1.0,
                 initial_accumulator_value: float = 0.1, n_samples: Optional[int] = None, candidate_sets=None,
                 labels: str = "one"):
        self.n_samples = None if n_samples is None else int(n_samples)
        if self.n_samples is not None and candidate_sets is not None:
            raise ValueError("SoftmaxTrainer: candidate_sets belong to the 1-vs-all objective (drop n_samples)")
        if labels not in ("one", "all"):
            raise ValueError("SoftmaxTrainer: labels must be 'one' or 'all'")
        self.labels = labels
        if labels == "all":
            if self.n_samples is not None or candidate_sets is not None:
                raise ValueError("SoftmaxTrainer: labels='all' runs over all candidates (drop n_samples and candidate_sets)")
            tri = _triples(triples, "triples")
            self.queries = {s: QueryLabels.from_triples(tri, candidates, s) for s in ("tail", "head")}
            self.Q = len(self.queries["tail"]) + len(self.queries["head"])
            if self.Q < int(batch_size):
                raise ValueError("fewer queries than batch_size (no short batches)")
            # the most labels batch_size rows of one side can have
            most = max(int(torch.sort(q.counts, descending=True).values[:int(batch_size)].sum()) for q in self.queries.values())
            self.opt = LabelSoftmaxAdaGrad(embeddings, candidates, batch_size, most, scale=scale, max_norm=max_norm,
                                           initial_accumulator_value=initial_accumulator_value)
        elif self.n_samples is None:
            self.opt = SoftmaxAdaGrad(embeddings, candidates, batch_size, scale=scale, max_norm=max_norm,
                                      initial_accumulator_value=initial_accumulator_value, candidate_sets=candidate_sets)
        else:
            _need_cuda(candidates, "candidates")
            self.pool = candidates.to(torch.int32).contiguous().view(-1)
            if self.pool.numel() < 1:
                raise ValueError("SoftmaxTrainer: an empty candidate pool")
            self.opt = SampledSoftmaxAdaGrad(embeddings, batch_size, self.n_samples, scale=scale, max_norm=max_norm,
                                             initial_accumulator_value=initial_accumulator_value)
            self._cand_gen = torch.Generator(device=self.opt.embeddings.device)
            self._cand_gen.manual_seed(int(seed) + 1)
        self.embeddings = self.opt.embeddings
        self.triples = _triples(triples, "triples")
        self.B = int(batch_size)
        if self.triples.shape[0] < self.B:
            raise ValueError("fewer triples than batch_size (no short batches)")
        self.lr0, self.decay_steps, self.decay_rate = float(learning_rate), float(learning_decay_steps), float(learning_decay_rate)
        self.global_step = 0
        self._gen = torch.Generator(device=self.embeddings.device)
        self._gen.manual_seed(int(seed))
        self._perm, self._row = None, 0

    @property
    def accumulator(self) -> torch.Tensor:
        return self.opt.accumulator

    @accumulator.setter
    def accumulator(self, value: torch.Tensor):
        self.opt.accumulator = _accumulator(value, self.embeddings)

    def learning_rate(self, step=None) -> float:
        s = self.global_step if step is None else step
        return inverse_time_decay(self.lr0, s, self.decay_steps, self.decay_rate) if self.decay_steps > 0 else self.lr0

    def next_batch(self) -> torch.Tensor:
        """The next [B,3] batch of the epoch order (a new permutation when fewer than B rows are left)."""
        T = self.triples.shape[0]
        if self._perm is None or self._row + self.B > T:
            self._perm = torch.randperm(T, device=self.triples.device, generator=self._gen)
            self._row = 0
        rows = self._perm[self._row:self._row + self.B]
        self._row += self.B
        return self.triples[rows].contiguous()

    def next_queries(self):
        """labels="all": the next step's (tail batch or None, head batch or None), each as QueryLabels.take gives it."""
        if self.labels != "all":
            raise ValueError("SoftmaxTrainer.next_queries: built with labels='one', the rows are triples")
        if self._perm is None or self._row + self.B > self.Q:
            self._perm = torch.randperm(self.Q, device=self.embeddings.device, generator=self._gen)
            self._row = 0
        rows = self._perm[self._row:self._row + self.B]
        self._row += self.B
        n_tail = len(self.queries["tail"])
        is_tail = rows < n_tail
        t, h = rows[is_tail], rows[~is_tail] - n_tail
        return (self.queries["tail"].take(t) if t.numel() else None, self.queries["head"].take(h) if h.numel() else None)

    def next_candidates(self) -> torch.Tensor:
        """The next step's [n_samples] candidates: a uniform draw from the pool, with replacement."""
        if self.n_samples is None:
            raise ValueError("SoftmaxTrainer.next_candidates: built without n_samples, every candidate is used")
        at = torch.randint(self.pool.numel(), (self.n_samples,), device=self.pool.device, generator=self._cand_gen)
        return self.pool[at]

    def run(self, n_steps: int, keep_losses: bool = False) -> torch.Tensor:
        """n_steps steps on the current stream; the losses [n_steps, B, 2] if keep_losses, else the last step's [B,2]
        (labels="all": [n_steps, B] and [B])."""
        kept, loss = [], None
        for _ in range(n_steps):
            if self.labels == "all":
                loss = torch.cat([l for l in self.opt.step(*self.next_queries(), self.learning_rate()) if l is not None])
            elif self.n_samples is None:
                loss = self.opt.step(self.next_batch(), self.learning_rate())
            else:
                loss = self.opt.step(self.next_batch(), self.next_candidates(), self.learning_rate())
            self.global_step += 1
            if keep_losses:
                kept.append(loss)
        return torch.stack(kept, 0) if keep_losses else loss


def gather_rows(table: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """out[i] = table[idx[i]] (zeros where idx[i] < 0)."""
    table = _table(table)
    _need_cuda(idx, "idx")
    idx = idx.to(torch.int32).contiguous()
    out = torch.empty(idx.numel(), table.shape[1], dtype=torch.float32, device=table.device)
    _lib.call("ge_gather_rows", table.data_ptr(), table.shape[0], table.shape[1], idx.data_ptr(),
              idx.numel(), out.data_ptr(), _stream())
    return out


def score_candidates(embeddings: torch.Tensor, fixed_and_relation: torch.Tensor, candidates: torch.Tensor, *,
                     cand_is_head: bool = False, max_norm: float = 1.0, apply_sigmoid: bool = True) -> torch.Tensor:
    """The candidate sweep of holE.py:564-569 in one call: E for every (fixed_i, cand_j, rel_i)
    (or (cand_j, fixed_i, rel_i) with cand_is_head) as [B,K]; fp32-MFMA GEMM on the GPU."""
    emb = _table(embeddings)
    _need_cuda(fixed_and_relation, "fixed_and_relation"); _need_cuda(candidates, "candidates")
    hr = fixed_and_relation.to(torch.int32).contiguous()
    cand = candidates.to(torch.int32).contiguous().view(-1)
    if hr.dim() != 2 or hr.shape[1] != 2:
        raise ValueError("fixed_and_relation must be [B,2] (entity, relation)")
    out = torch.empty(hr.shape[0], cand.numel(), dtype=torch.float32, device=emb.device)
    _lib.call("ge_complex_score_1vK", emb.data_ptr(), emb.shape[0], emb.shape[1], hr.data_ptr(), hr.shape[0],
              cand.data_ptr(), cand.numel(), max_norm, int(apply_sigmoid), int(cand_is_head), out.data_ptr(),
              _stream())
    return out


def rank_max_dim() -> int:
    return int(_lib.load().ge_rank_max_dim())


def split_sweep_ok(d: int, max_norm: float) -> bool:
    """The split-precision sweep (the F16 of csrc/ge_sweep_route.h, f16_sweep_ok there) takes this embedding_dim and
    max_norm: what the planes, the fused top-k and the main road of the rank sweep need."""
    return d % 8 == 0 and 56 <= d <= 288 and max_norm <= 8.0


def rank_fused_ok(d: int, max_norm: float) -> bool:
    """Some kernel of route_rank (csrc/ge_sweep_route.h) ranks this embedding_dim and max_norm: a multiple of 8 that
    the fp32 kernels hold (kRankMaxDimF32 = 232 there) or the split-precision sweep takes."""
    return d % 8 == 0 and (0 < d <= 232 or split_sweep_ok(d, max_norm))


def _sweep_model(model, who: str, hint: str = "") -> int:
    """The model code of a sweep of csrc/ge_sweep_route.h: ComplEx, or HolE on a spectral table."""
    if model not in ("complex", "hole_spectral"):
        raise ValueError(f"{who}: model must be 'complex' or 'hole_spectral'{hint}")
    return _MODELS[model]


_TRANSFORM_FIRST = " (transform a real HolE table first)"


def _known_ok(known_off, known_rc, B=None, K=None):
    """The known-true lists of a sweep come together; with (B, K) their shape is checked too.  Returns their pointers."""
    if (known_off is None) != (known_rc is None):
        raise ValueError("known_off and known_rc come together")
    if known_off is None:
        return None, None
    if B is not None:
        n_tiles = ((B + 127) // 128) * ((K + 127) // 128)
        if known_off.dtype != torch.int32 or known_off.numel() != n_tiles + 1 or known_rc.dtype != torch.int16:
            raise ValueError("known_off must be int32 [tiles+1], known_rc int16 (row%128 << 7 | col%128)")
    return known_off.data_ptr(), known_rc.data_ptr()


def _planes_ptr(planes, emb, cand, K, max_norm, model, who):
    """(candidates, planes pointer) of a sweep given `planes`: the RankPlanes' own candidate tensor and buffer once they
    are known to be built for this (table, candidate list, max_norm, model); (cand, None) without planes."""
    if planes is None or planes.buffer is None:
        return cand, None
    same = planes.key == (emb.data_ptr(), emb.shape[0], emb.shape[1], planes.cand.data_ptr(), K, float(max_norm), model)
    if same and cand.data_ptr() != planes.cand.data_ptr():      # another tensor: compare the ids (one synchronisation)
        same = bool(torch.equal(planes.cand, cand))
    if not same:
        raise ValueError(f"{who}: `planes` were built for another table / candidate list / max_norm / model")
    return planes.cand, planes.buffer.data_ptr()


def candidate_mask_words(K: int) -> int:
    """Words per set of a candidate mask over K candidates (ge_candidate_mask_words): 4 per 128-candidate tile."""
    return 0 if K <= 0 else 4 * ((int(K) + 127) // 128)


def _sets_args(candidate_sets, row_sets, hr, cand, who):
    """() without candidate sets, else (row_set pointer, mask pointer, n_sets) of a masked sweep -- after the host checks:
    the mask's shape, that it was built for this candidate list, the row sets' length and range (one synchronisation).
    candidate_sets: anything with .mask (int32 [n_sets, candidate_mask_words(K)], CUDA), .n_sets and .cand (the int32
    candidate ids it was built for): evaluate.CandidateSets.  row_sets default: each row's relation id."""
    if candidate_sets is None:
        if row_sets is not None:
            raise ValueError(f"{who}: row_sets without candidate_sets")
        return (), None
    cs, B, K = candidate_sets, hr.shape[0], cand.numel()
    mask = cs.mask
    if (not isinstance(mask, torch.Tensor) or not mask.is_cuda or mask.dtype != torch.int32 or not mask.is_contiguous()
            or tuple(mask.shape) != (int(cs.n_sets), candidate_mask_words(K)) or cs.n_sets < 1):
        raise ValueError(f"{who}: candidate_sets.mask must be a contiguous CUDA int32 [n_sets, {candidate_mask_words(K)}] "
                         f"tensor for these {K} candidates")
    if cs.cand.numel() != K or (cs.cand.data_ptr() != cand.data_ptr() and not bool(torch.equal(cs.cand.to(cand.device), cand))):
        raise ValueError(f"{who}: candidate_sets were built for another candidate list")
    rs = hr[:, 1] if row_sets is None else torch.as_tensor(row_sets).to(hr.device)
    if rs.dim() != 1 or rs.numel() != B or rs.dtype.is_floating_point:
        raise ValueError(f"{who}: row_sets must be [B] integers")
    if B and bool(((rs < -1) | (rs >= cs.n_sets)).any()):
        raise ValueError(f"{who}: a row's set index is outside [-1, {cs.n_sets})")
    rs = rs.to(torch.int32).contiguous()
    return (rs.data_ptr(), mask.data_ptr(), int(cs.n_sets)), rs     # (rs: kept alive by the caller until the launch)


class RankPlanes:
    """The candidates of a ranking sweep as the split-precision kernel reads them (ge_rank_planes: fp16 high halves and
    remainders of row * clip scale * 2^8 per 64-candidate tile, plus the entity -> position map), built ONCE for all the
    batches -- tails and heads -- ranked against the same (table, candidates, max_norm, model).  `buffer` is None when
    embedding_dim has no split-precision sweep (rank_candidates then ignores it).  Rebuild after the table changes."""

    def __init__(self, embeddings: torch.Tensor, candidates: torch.Tensor, *, max_norm: float = 1.0, model: str = "complex"):
        code = _sweep_model(model, "RankPlanes")
        emb = _table(embeddings)
        _need_cuda(candidates, "candidates")
        self.cand = candidates.to(torch.int32).contiguous().view(-1)
        self.key = (emb.data_ptr(), emb.shape[0], emb.shape[1], self.cand.data_ptr(), self.cand.numel(), float(max_norm), model)
        nbytes = int(_lib.load().ge_rank_planes_bytes(emb.shape[0], emb.shape[1], self.cand.numel())) if split_sweep_ok(emb.shape[1], max_norm) else 0
        self.buffer = None
        if nbytes > 0:
            self.buffer = torch.empty(nbytes, dtype=torch.uint8, device=emb.device)     # (the allocator aligns to 256 bytes and more)
            _lib.call("ge_rank_planes", emb.data_ptr(), emb.shape[0], emb.shape[1], self.cand.data_ptr(), self.cand.numel(),
                      max_norm, code, self.buffer.data_ptr(), _stream())


def rank_candidates(embeddings: torch.Tensor, fixed_and_relation: torch.Tensor, true_ids: torch.Tensor,
                    candidates: torch.Tensor, *, known_off: Optional[torch.Tensor] = None,
                    known_rc: Optional[torch.Tensor] = None, cand_is_head: bool = False, max_norm: float = 1.0,
                    return_true_loss: bool = False, return_scores: bool = False, model: str = "complex",
                    planes: Optional[RankPlanes] = None, candidate_sets=None, row_sets=None):
    """The candidate sweep of holE.py:564-569 with the ranking of holE.py:427-472 as its epilogue
    (ge_complex_rank_1vK): per test row the number of candidates that pop from the reference's heap before the
    true one (n_before; raw rank = 1 + n_before) and how many of those are known-true (n_known_before; filtered
    rank = raw - n_known_before).  No [B,K] score matrix exists unless return_scores asks for it (tests).
    known_off / known_rc: the per-(128 rows x 128 candidates)-tile lists of known-true cells (evaluate.py).
    model: "complex", or "hole_spectral" for a table held in the frequency domain (hole_to_spectral).
    planes: RankPlanes(embeddings, candidates, ...) built once for many calls (otherwise the kernel rebuilds them).
    candidate_sets (evaluate.CandidateSets) / row_sets ([B], default the row's relation id; -1: unrestricted): only the
    candidates admissible in the row's set are counted (ge_rank_1vK_masked); losses and true_loss are unchanged.  The
    split-precision range only (split_sweep_ok), otherwise GeError (GE_ENOTSUP); bad sets raise ValueError."""
    code = _sweep_model(model, "rank_candidates", _TRANSFORM_FIRST)
    emb = _table(embeddings)
    for name, t in (("fixed_and_relation", fixed_and_relation), ("true_ids", true_ids), ("candidates", candidates)):
        _need_cuda(t, name)
    hr = fixed_and_relation.to(torch.int32).contiguous()
    tid = true_ids.to(torch.int32).contiguous().view(-1)
    cand = candidates.to(torch.int32).contiguous().view(-1)
    B, K = hr.shape[0], cand.numel()
    if hr.dim() != 2 or hr.shape[1] != 2 or tid.numel() != B:
        raise ValueError("fixed_and_relation must be [B,2] (entity, relation) and true_ids [B]")
    n_before = torch.empty(B, dtype=torch.int32, device=emb.device)
    n_known = torch.empty(B, dtype=torch.int32, device=emb.device)
    tl = torch.empty(B, dtype=torch.float32, device=emb.device) if return_true_loss else None
    sc = torch.empty(B, K, dtype=torch.float32, device=emb.device) if return_scores else None
    known = _known_ok(known_off, known_rc, B, K)
    cand, pl = _planes_ptr(planes, emb, cand, K, max_norm, model, "rank_candidates")
    sets, _rs = _sets_args(candidate_sets, row_sets, hr, cand, "rank_candidates")
    _lib.call("ge_rank_1vK_masked" if sets else "ge_rank_1vK_planes", emb.data_ptr(), emb.shape[0], emb.shape[1],
              hr.data_ptr(), B, tid.data_ptr(),
              cand.data_ptr(), K, max_norm, code, int(cand_is_head), *known, n_before.data_ptr(), n_known.data_ptr(),
              tl.data_ptr() if tl is not None else None, sc.data_ptr() if sc is not None else None, pl, *sets, _stream())
    out = (n_before, n_known)
    if return_true_loss:
        out += (tl,)
    if return_scores:
        out += (sc,)
    return out


def rank_candidates_vs_loss(embeddings: torch.Tensor, fixed_and_relation: torch.Tensor, ref_ids: torch.Tensor,
                            ref_losses: torch.Tensor, candidates: torch.Tensor, *, known_off: Optional[torch.Tensor] = None,
                            known_rc: Optional[torch.Tensor] = None, cand_is_head: bool = False, max_norm: float = 1.0,
                            model: str = "complex", planes: Optional[RankPlanes] = None):
    """The sweep of rank_candidates against GIVEN losses (ge_rank_1vK_vs_loss): per row how many of `candidates` pop from
    the reference's heap (holE.py:427-472: ascending loss, ties by id) before a triple of loss ref_losses[i] and id
    ref_ids[i] -- which need not be among them -- and how many of those are known-true.  What a rank of a row-sharded
    evaluation computes over its own candidates (the counts add across ranks), and what the reference's is_confident
    gate (holE.py:436-438) reduces to: min_loss < threshold  <=>  n_before(threshold, id = INT32_MIN) > 0."""
    code = _sweep_model(model, "rank_candidates_vs_loss")
    emb = _table(embeddings)
    for name, t in (("fixed_and_relation", fixed_and_relation), ("ref_ids", ref_ids), ("ref_losses", ref_losses),
                    ("candidates", candidates)):
        _need_cuda(t, name)
    hr = fixed_and_relation.to(torch.int32).contiguous()
    rid = ref_ids.to(torch.int32).contiguous().view(-1)
    rl = ref_losses.to(torch.float32).contiguous().view(-1)
    cand = candidates.to(torch.int32).contiguous().view(-1)
    B, K = hr.shape[0], cand.numel()
    if hr.dim() != 2 or hr.shape[1] != 2 or rid.numel() != B or rl.numel() != B:
        raise ValueError("fixed_and_relation must be [B,2] (entity, relation), ref_ids and ref_losses [B]")
    known = _known_ok(known_off, known_rc)
    cand, pl = _planes_ptr(planes, emb, cand, K, max_norm, model, "rank_candidates_vs_loss")
    n_before = torch.empty(B, dtype=torch.int32, device=emb.device)
    n_known = torch.empty(B, dtype=torch.int32, device=emb.device)
    _lib.call("ge_rank_1vK_vs_loss", emb.data_ptr(), emb.shape[0], emb.shape[1], hr.data_ptr(), B, rid.data_ptr(),
              rl.data_ptr(), cand.data_ptr(), K, max_norm, code, int(cand_is_head), *known, n_before.data_ptr(),
              n_known.data_ptr(), pl, _stream())
    return n_before, n_known


def topk_max_k() -> int:
    """Largest k the fused top-k sweep (ge_topk_1vK_planes) takes."""
    return int(_lib.load().ge_topk_max_k())


def topk_candidates(embeddings: torch.Tensor, fixed_and_relation: torch.Tensor, candidates: torch.Tensor, k: int, *,
                    known_off: Optional[torch.Tensor] = None, known_rc: Optional[torch.Tensor] = None,
                    cand_is_head: bool = False, max_norm: float = 1.0, model: str = "complex",
                    planes: Optional[RankPlanes] = None, candidate_sets=None, row_sets=None):
    """The first k pops of the reference's heap (holE.py:427-469: ascending loss, ties by entity id) per query row
    (fixed entity, relation) among `candidates`, on the split-precision sweep (ge_topk_1vK_planes) -- no [B,K] matrix.
    With known_off / known_rc (as rank_candidates takes them) known-true candidates are skipped.  Returns
    (ids int32 [B,k], losses float32 [B,k]); a row with fewer eligible candidates is padded with -1 / +inf, a row whose
    ids are out of range is -1 / NaN.  The losses are bit-equal to rank_candidates(..., return_scores=True)'s.
    embedding_dim % 8 == 0 in 56 ... 288, max_norm <= 8, 1 <= k <= topk_max_k(); otherwise GeError (GE_ENOTSUP).
    candidate_sets / row_sets (as rank_candidates takes them): the first k pops that are admissible in the row's set and
    not known (ge_topk_1vK_masked); an empty set gives a row of -1 / +inf."""
    code = _sweep_model(model, "topk_candidates", _TRANSFORM_FIRST)
    emb = _table(embeddings)
    for name, t in (("fixed_and_relation", fixed_and_relation), ("candidates", candidates)):
        _need_cuda(t, name)
    hr = fixed_and_relation.to(torch.int32).contiguous()
    cand = candidates.to(torch.int32).contiguous().view(-1)
    if hr.dim() != 2 or hr.shape[1] != 2:
        raise ValueError("fixed_and_relation must be [B,2] (entity, relation)")
    B, K, N = hr.shape[0], cand.numel(), emb.shape[0]
    k = int(k)
    if k < 1:
        raise ValueError("k must be >= 1")
    if K < 1:
        raise ValueError("candidates must not be empty")
    if bool(((cand < 0) | (cand >= N)).any()):
        raise ValueError("a candidate id is outside the table")
    if torch.unique(cand).numel() != K:
        raise ValueError("candidates must be distinct")
    if B and bool(((hr < 0) | (hr >= N)).any()):
        raise ValueError("a fixed entity or relation id is outside the table")
    known = _known_ok(known_off, known_rc, B, K)
    cand, pl = _planes_ptr(planes, emb, cand, K, max_norm, model, "topk_candidates")
    sets, _rs = _sets_args(candidate_sets, row_sets, hr, cand, "topk_candidates")
    ids = torch.empty(B, k, dtype=torch.int32, device=emb.device)
    losses = torch.empty(B, k, dtype=torch.float32, device=emb.device)
    if B == 0:
        return ids, losses
    nbytes = int(_lib.load().ge_topk_workspace_bytes(B, K, k))
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=emb.device)
    _lib.call("ge_topk_1vK_masked" if sets else "ge_topk_1vK_planes", emb.data_ptr(), N, emb.shape[1], hr.data_ptr(), B,
              cand.data_ptr(), K, max_norm, code, int(cand_is_head), *known, k, ids.data_ptr(), losses.data_ptr(), pl,
              ws.data_ptr(), ws.numel(), *sets, _stream())
    return ids, losses


def confident_rows(embeddings: torch.Tensor, fixed_and_relation: torch.Tensor, candidates: torch.Tensor, infer_threshold: float,
                   **kw) -> torch.Tensor:
    """is_confident of holE.py:436-438 for every row of a sweep: min over the candidates of the loss < infer_threshold,
    as a bool tensor [B] -- one more sweep, counting the candidates below the threshold (no [B,K] matrix)."""
    B = fixed_and_relation.shape[0]
    dev = embeddings.device
    thr = torch.full((B,), float(infer_threshold), dtype=torch.float32, device=dev)
    lowest = torch.full((B,), -2 ** 31, dtype=torch.int32, device=dev)        # no candidate id is smaller: strict "<" only
    n_before, _ = rank_candidates_vs_loss(embeddings, fixed_and_relation, lowest, thr, candidates, **kw)
    return n_before > 0


class ValidationPocket:
    """The validation ticks of the training loop (holE.py:299-304, 351-360) without a host round trip per tick
    (ge_validation_tick): each tick draws a validation batch on the device, corrupts it, takes the mean hinge into
    `hist`, and -- the reference's "pocket" -- copies the table into `pocket` iff that mean is the best so far.
    The host calls read() when it wants the numbers (one synchronisation for all ticks since the last read)."""

    def __init__(self, embeddings: torch.Tensor, validation_triples: torch.Tensor, type_tables: "TypeTables",
                 batch_size: int, *, margin: float = 0.2, model="complex", max_norm: float = 1.0, seed: int = 0,
                 mode: int = CORRUPT_BATCH_COIN, keep_table: bool = True, capacity: int = 4096, log_loss=None):
        """log_loss = (negative_ratio, l2_regularization): the tick evaluates the --log_loss objective instead of the hinge
        (ge_validation_tick_logloss; ComplEx score)."""
        self.emb = _table(embeddings)
        _need_cuda(validation_triples, "validation_triples")
        self.valid = validation_triples.to(torch.int32).contiguous()
        if self.valid.dim() != 2 or self.valid.shape[1] != 3 or self.valid.shape[0] == 0:
            raise ValueError("validation_triples must be [V,3] with V > 0")
        self.tt, self.B = type_tables, int(batch_size)
        self.margin, self.max_norm, self.model = float(margin), float(max_norm), _MODELS[model]
        self.seed, self.mode = int(seed), int(mode)
        dev = self.emb.device
        self.best = torch.full((), 2.0, dtype=torch.float32, device=dev)     # holE.py:336 pocket_loss = 2.
        self.pocket = torch.empty_like(self.emb) if keep_table else None
        self.hist = torch.zeros(int(capacity), dtype=torch.float32, device=dev)
        self.log_loss = None if log_loss is None else (int(log_loss[0]), float(log_loss[1]))
        if self.log_loss is not None and self.model != MODEL_COMPLEX:
            raise NotImplementedError("--log_loss is defined for the ComplEx score (holE.py:191-196)")
        need = (_lib.load().ge_validation_workspace_bytes(self.B) if self.log_loss is None
                else _lib.load().ge_validation_logloss_workspace_bytes(self.B, self.log_loss[0]))
        self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        self._steps = []        # global step of each tick since the last read()

    def tick(self, counter: int, global_step: int) -> None:
        if len(self._steps) >= self.hist.numel():
            raise RuntimeError("ValidationPocket: read() the pending ticks first (capacity %d)" % self.hist.numel())
        tt, i = self.tt, len(self._steps)
        head = (self.emb.data_ptr(), self.emb.shape[0], self.emb.shape[1], self.valid.data_ptr(), self.valid.shape[0], self.B,
                *tt.abi(), self.seed & (2**64 - 1), int(counter) & (2**64 - 1), tt.padded_size, self.mode)
        tail = (self.max_norm,) + (() if self.log_loss is not None else (self.model,)) + (
            self._ws.data_ptr(), self._ws.numel(), self.hist.data_ptr() + 4 * i, self.best.data_ptr(),
            self.pocket.data_ptr() if self.pocket is not None else None, _stream())
        if self.log_loss is not None:
            _lib.call("ge_validation_tick_logloss", *head, *self.log_loss, *tail)
        else:
            _lib.call("ge_validation_tick", *head, self.margin, *tail)
        self._steps.append(int(global_step))

    def read(self):
        """[(global_step, mean validation hinge)] of the ticks since the last read, in order (synchronises)."""
        n = len(self._steps)
        if n == 0:
            return []
        vals = self.hist[:n].cpu().tolist()
        out = list(zip(self._steps, vals))
        self._steps = []
        return out


def _i32(t: torch.Tensor, name: str) -> torch.Tensor:
    _need_cuda(t, name)
    if t.dtype != torch.int32 or not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous int32")
    return t


# ---------------------------------------------------------------- the row-sharded step (csrc/ge_shard.hip)
def shard_plan(pos: torch.Tensor, neg: torch.Tensor, n_rows: int, world: int, rank: int, peer_mapped: bool = False):
    """ge_shard_plan for S steps: pos, neg [S,B,3] int32 global ids -> (records [S,W], pos_src [S,B,3], neg_src [S,B],
    req_row [S,cap], counts [S,world]) -- see include/ge_hip.h."""
    _i32(pos, "pos"), _i32(neg, "neg")
    S, B = int(pos.shape[0]), int(pos.shape[1])
    lay = prepared_layout(B)
    dev = pos.device
    records = torch.empty(S, lay[0], dtype=torch.int32, device=dev)
    pos_src = torch.empty(S, B, 3, dtype=torch.int32, device=dev)
    neg_src = torch.empty(S, B, dtype=torch.int32, device=dev)
    req_row = torch.empty(S, 4 * lay[1] * lay[2], dtype=torch.int32, device=dev)
    counts = torch.empty(S, world, dtype=torch.int32, device=dev)
    need = int(_lib.load().ge_shard_plan_workspace_bytes(B, S))
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    _lib.call("ge_shard_plan", pos.data_ptr(), neg.data_ptr(), S, B, int(n_rows), int(world), int(rank), records.data_ptr(),
              pos_src.data_ptr(), neg_src.data_ptr(), req_row.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
              int(bool(peer_mapped)), _stream())
    return records, pos_src, neg_src, req_row, counts


def shard_grad(shard: torch.Tensor, staged, pos_src, neg_src, record, B: int, n_rows: int, world: int, lr: float,
               margin: float, model, max_norm: float, grad_idx: torch.Tensor, grad_val: torch.Tensor, gsum,
               peer_shards=None) -> torch.Tensor:
    """ge_shard_grad: one step's fused gather/score/hinge/grad on the shard (in place) + the staged rows; returns loss [B].
    peer_shards (experiment): the `world` shards as tensors mapped into this process -- the other owners' rows are
    then read in place and `staged` is None (the plan must have been built with peer_mapped=True)."""
    import ctypes as C
    shard = _table(shard)
    n_staged = (0 if gsum is None else int(gsum.shape[0])) if peer_shards is not None else (0 if staged is None else int(staged.shape[0]))
    loss = torch.empty(B, dtype=torch.float32, device=shard.device)
    peers = None
    if peer_shards is not None:
        peers = (C.c_void_p * len(peer_shards))(*[t.data_ptr() for t in peer_shards])
    _lib.call("ge_shard_grad", shard.data_ptr(), shard.shape[0], shard.shape[1],
              staged.data_ptr() if (peers is None and n_staged) else None,
              n_staged, pos_src.data_ptr(), neg_src.data_ptr(), record.data_ptr(), int(B), int(n_rows), int(world),
              float(margin), float(lr), float(max_norm), _MODELS[model], loss.data_ptr(), grad_idx.data_ptr(),
              grad_val.data_ptr(), gsum.data_ptr() if n_staged else None, peers, _stream())
    return loss


def shard_apply(shard: torch.Tensor, record, B: int, n_rows: int, world: int, grad_idx, grad_val, gsum) -> None:
    """ge_shard_apply: own rows updated in place, staged rows' gradient sums into gsum."""
    shard = _table(shard)
    _lib.call("ge_shard_apply", shard.data_ptr(), shard.shape[0], shard.shape[1], record.data_ptr(), int(B), int(n_rows),
              int(world), grad_idx.data_ptr(), grad_val.data_ptr(), gsum.data_ptr() if gsum is not None and gsum.numel() else None,
              _stream())


def shard_owner_plan(req_all: torch.Tensor, req_start, rows_local: int):
    """ge_shard_owner_plan: (records [S,W], cap) for the chunk's received request lists; req_start: host list [S+1]."""
    S = len(req_start) - 1
    cap = max([req_start[i + 1] - req_start[i] for i in range(S)] + [0])
    dev = req_all.device
    lib = _lib.load()
    words = int(lib.ge_shard_owner_record_words(cap))
    records = torch.empty(S, max(words, 1), dtype=torch.int32, device=dev)
    if cap:
        rs = torch.tensor(req_start, dtype=torch.int64).to(dev, non_blocking=False)
        ws = torch.empty(max(int(lib.ge_shard_owner_workspace_bytes(cap, S)), 256), dtype=torch.uint8, device=dev)
        _lib.call("ge_shard_owner_plan", _i32(req_all, "req_all").data_ptr(), rs.data_ptr(), S, cap, int(rows_local),
                  records.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return records, cap


def shard_owner_apply(shard: torch.Tensor, oplan, s: int, recv: torch.Tensor) -> None:
    records, cap = oplan
    if cap == 0 or recv.shape[0] == 0:
        return
    shard = _table(shard)
    _lib.call("ge_shard_owner_apply", shard.data_ptr(), shard.shape[0], shard.shape[1], records[s].data_ptr(), int(cap),
              recv.data_ptr(), _stream())


class Trainer:
    """The inner loop of run_training (holE.py:340-362, minus validation) enqueued natively by
    ge_train_steps: per step a batch of the device-resident shuffled triple array, type-safe
    negatives, lr from inverse_time_decay, one fused hinge SGD step.  No host work per step."""

    def __init__(self, embeddings: torch.Tensor, triples: torch.Tensor, type_tables: TypeTables,
                 batch_size: int, *, margin: float = 0.2, learning_rate: float = 0.1,
                 decay_steps: float = 0.0, decay_rate: float = 0.5, model="complex", max_norm: float = 1.0,
                 seed: int = 0, corrupt_mode: int = CORRUPT_BATCH_COIN, prepared: bool = True,
                 lookahead: bool = True, spectral_resident: bool = False, deterministic: bool = False,
                 optimizer: str = "sgd", initial_accumulator_value: float = 0.1):
        # optimizer="adagrad": AdagradOptimizer in place of the GradientDescentOptimizer of holE.py:296 -- run() enqueues
        # ge_train_steps_adagrad (prepared path only; no float atomics, so bitwise reproducible) and `accumulator` holds
        # the [N,d] sum of squared gradients, filled with initial_accumulator_value
        if optimizer not in ("sgd", "adagrad"):
            raise ValueError("optimizer must be 'sgd' or 'adagrad'")
        self.optimizer, self.accumulator = optimizer, None
        if optimizer == "adagrad":
            if spectral_resident or _MODELS[model] == MODEL_HOLE_SPECTRAL:
                raise ValueError("AdaGrad is elementwise: it does not commute with the DFT, the table stays real "
                                 "(spectral_resident=False)")
            if not prepared:
                raise ValueError("the AdaGrad loop runs on the prepared path only")
            if not initial_accumulator_value > 0:
                raise ValueError("initial_accumulator_value must be positive")
        # deterministic (GE_STEP_DETERMINISTIC): rows with more than 16 gradient slots in a step are reduced in a fixed
        # order instead of by float atomics -- every row bitwise reproducible run to run; one more launch per step
        self.deterministic = bool(deterministic)
        self.embeddings = _table(embeddings)
        self.triples = _triples(triples, "triples")
        if self.triples.shape[0] < batch_size:
            raise ValueError("fewer triples than batch_size (the reference never yields a short batch)")
        self.tt = type_tables
        self.B = int(batch_size)
        self.margin, self.lr0 = float(margin), float(learning_rate)
        self.decay_steps, self.decay_rate = float(decay_steps), float(decay_rate)
        self.model, self.max_norm, self.seed, self.mode = _MODELS[model], float(max_norm), int(seed), int(corrupt_mode)
        self.global_step = 0
        self.row = 0
        dev = self.embeddings.device
        # model="hole" hands ge_train_steps the real-valued table: every run() transforms it to the frequency
        # domain and back (two O(N d^2) passes per call).  spectral_resident=True transforms ONCE, here, keeps
        # `embeddings` spectral between calls (score it with model="hole_spectral") and to_real() undoes it.
        self.spectral = False
        if spectral_resident:
            if self.model != MODEL_HOLE or (self.embeddings.shape[1] & 1):
                raise ValueError("spectral_resident needs model='hole' and an even embedding_dim")
            hole_to_spectral(self.embeddings)
            self.model, self.spectral = MODEL_HOLE_SPECTRAL, True
        # prepared=False: only the single-step workspace -> ge_train_steps takes its fallback branch
        # (per-step sampler launch + float-atomic scatter); lookahead=False: no pipeline handle, the
        # prepare launches go to the caller's stream and nothing survives between run() calls
        lib = _lib.load()
        d = self.embeddings.shape[1]
        need = lib.ge_train_workspace_bytes(self.B, d) if prepared else lib.ge_hinge_step_workspace_bytes(self.B, d)
        self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        self._neg = torch.empty(self.B, 3, dtype=torch.int32, device=dev)
        self.last_loss = torch.zeros(self.B, dtype=torch.float32, device=dev)
        if optimizer == "adagrad":
            self.accumulator = torch.full_like(self.embeddings, float(initial_accumulator_value))
        # the prepared-steps pipeline (side stream + look-ahead records that survive between run() calls)
        self._pipe = None
        if prepared and lookahead:
            import ctypes as C
            h = C.c_void_p()
            with torch.cuda.device(dev):
                _lib.call("ge_train_pipeline_create", C.byref(h))
            self._pipe = h.value

    def close(self):
        """Release the pipeline handle (waits for its side stream)."""
        if getattr(self, "_pipe", None):
            _lib.load().ge_train_pipeline_destroy(self._pipe)
            self._pipe = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def to_real(self):
        """Leave the resident-spectral mode: `embeddings` becomes the real-valued HolE table again."""
        if self.spectral:
            hole_from_spectral(self.embeddings)
            self.model, self.spectral = MODEL_HOLE, False

    def real_embeddings(self) -> torch.Tensor:
        """A real-valued copy of the table (checkpoints, evaluation), whatever domain it is held in."""
        return hole_from_spectral(self.embeddings.clone()) if self.spectral else self.embeddings

    def invalidate(self):
        """Forget the records prepared ahead (call after changing `triples` or the type tables in place)."""
        if self._pipe:
            _lib.call("ge_train_pipeline_reset", self._pipe)

    def learning_rate(self, step=None) -> float:
        s = self.global_step if step is None else step
        return inverse_time_decay(self.lr0, s, self.decay_steps, self.decay_rate) if self.decay_steps > 0 else self.lr0

    def prepare_reshuffle(self, generator=None):
        """Draw the NEXT pass order now, on a side stream, beside the steps of the current pass (a device randperm is a
        30-launch radix sort: ~0.35 ms, a fifth of a 116-step FB15k epoch at B = 4096 when it sits between two epochs);
        the next reshuffle() call adopts it.  Same generator, same draw order as reshuffle(generator): identical orders."""
        dev = self.triples.device
        if getattr(self, "_shuffle_stream", None) is None:
            self._shuffle_stream = torch.cuda.Stream(device=dev)
        side, cur = self._shuffle_stream, torch.cuda.current_stream(dev)
        side.wait_stream(cur)                                  # `triples` as it is now (an order is a permutation of it)
        with torch.cuda.stream(side):
            perm = torch.randperm(self.triples.shape[0], device=dev, generator=generator)
            nxt = self.triples[perm].contiguous()
            ready = torch.cuda.Event()
            ready.record(side)
        self.triples.record_stream(side)
        self._next_order = (nxt, ready)

    def reshuffle(self, generator=None):
        """New pass order (the shuffle queue of holE.py:281-283), done on the device -- the one prepare_reshuffle() drew
        ahead, if there is one."""
        ahead, self._next_order = getattr(self, "_next_order", None), None
        if ahead is not None:
            nxt, ready = ahead
            cur = torch.cuda.current_stream(nxt.device)
            cur.wait_event(ready)
            nxt.record_stream(cur)
            self.triples = nxt
        else:
            perm = torch.randperm(self.triples.shape[0], device=self.triples.device, generator=generator)
            self.triples = self.triples[perm].contiguous()
        self.row = 0
        self.invalidate()     # the allocator may hand the new order the address of an older one

    def enable_log_loss(self, negative_ratio: int = 1, l2_regularization: float = 0.1):
        """Switch the native loop to the --log_loss objective (holE.py:194-196, 206-220): run() then enqueues
        ge_train_steps_logloss -- negatives of all `negative_ratio` corrupted batches drawn in the prepare launch,
        row-sorted update, the dense L2 decay carried as one scalar.  last_loss becomes [(1+K)*B]."""
        if self.model != MODEL_COMPLEX:
            raise NotImplementedError("--log_loss is defined for the ComplEx score (holE.py:191-196)")
        if self.optimizer == "adagrad":
            raise ValueError("AdaGrad is not available for --log_loss: its dense L2 term makes every row's gradient non-zero")
        self.K, self.l2 = int(negative_ratio), float(l2_regularization)
        dev = self.embeddings.device
        need = _lib.load().ge_train_logloss_workspace_bytes(self.B, self.K, self.embeddings.shape[1])
        self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        self._neg = torch.empty(self.K, self.B, 3, dtype=torch.int32, device=dev)
        self.last_loss = torch.zeros((1 + self.K) * self.B, dtype=torch.float32, device=dev)
        self.invalidate()
        return self

    def _source(self, n_steps: int):
        """The step sequence and its sampler as both loops take them, up to `mode`."""
        return (self.triples.data_ptr(), self.triples.shape[0], self.row, self.B, n_steps, *self.tt.abi(),
                self.seed & (2**64 - 1), self.global_step, self.tt.padded_size, self.mode)

    def _advance(self, n_steps: int):
        """Mirror the C loops' row bookkeeping (step_row of csrc/ge_prep.h) and step count."""
        T, row = self.triples.shape[0], self.row % self.triples.shape[0]
        for _ in range(n_steps):
            if row + self.B > T:
                row = 0
            row += self.B
        self.row = row
        self.global_step += n_steps

    def run(self, n_steps: int, *, keep_losses: bool = False, events=None, ev_kernel: int = 2):
        """Enqueue n_steps training steps on the current stream; returns the loss tensor
        ([n_steps,B] if keep_losses else the last step's [B]; with enable_log_loss (1+K)*B per step)."""
        import ctypes as C
        emb = self.embeddings
        K = getattr(self, "K", 0)
        M = (1 + K) * self.B
        loss = torch.empty(n_steps * M, dtype=torch.float32, device=emb.device) if keep_losses else self.last_loss
        table = (emb.data_ptr(), emb.shape[0], emb.shape[1])
        rates = (self.lr0, self.decay_steps, self.decay_rate, self.max_norm)
        out = (loss.data_ptr(), int(keep_losses), self._neg.data_ptr(), self._ws.data_ptr(), self._ws.numel())
        if self.optimizer == "adagrad":
            if events is not None:
                raise ValueError("events= times the kernels of the SGD loop; the AdaGrad loop takes none")
            _lib.call("ge_train_steps_adagrad", emb.data_ptr(), _accumulator(self.accumulator, emb).data_ptr(), *table[1:],
                      *self._source(n_steps), self.margin, *rates, self.model, *out, self._pipe, _stream())
        elif K:
            _lib.call("ge_train_steps_logloss", *table, *self._source(n_steps), K, self.l2, *rates, *out, self._pipe, _stream())
        else:
            evp = None
            if events is not None:
                assert len(events) == 2 * n_steps
                evp = (C.c_void_p * len(events))(*events)
            _lib.call("ge_train_steps", *table, *self._source(n_steps), self.margin, *rates,
                      self.model | (STEP_DETERMINISTIC if self.deterministic else 0), *out, evp, int(ev_kernel), self._pipe,
                      _stream())
        self._advance(n_steps)
        return loss.view(n_steps, M) if keep_losses else loss


def prepared_layout(batch_size: int):
    """Word offsets of a prepared step record (ge_train_prepared_layout): (words per step, sub-batches,
    pairs per sub-batch, slot_item offset, first sub-batch offset, words per sub-batch, items offset,
    islots offset)."""
    import ctypes as C
    out = (C.c_int64 * 8)()
    _lib.call("ge_train_prepared_layout", int(batch_size), out)
    return tuple(int(v) for v in out)


def prepare_steps(triples: torch.Tensor, type_tables: TypeTables, batch_size: int, n_steps: int, *, first_row: int = 0,
                  seed: int = 0, global_step: int = 0, mode: int = CORRUPT_BATCH_COIN, direct: bool = False) -> torch.Tensor:
    """The prepare launch of ge_train_steps on its own (ge_train_prepare_steps): negatives plus the
    row-sorted work items of `n_steps` consecutive steps as an int32 [n_steps, words] tensor."""
    tb = _triples(triples, "triples")
    lay = prepared_layout(batch_size)
    nbytes = int(_lib.load().ge_train_prepare_bytes(int(batch_size), int(n_steps)))   # records + (B > 4096) sort scratch
    buf = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=tb.device)
    out = buf[:n_steps * lay[0]].view(n_steps, lay[0])
    id_to_type, *rest = type_tables.abi()
    _lib.call("ge_train_prepare_steps", tb.data_ptr(), tb.shape[0], int(first_row), int(batch_size), int(n_steps),
              id_to_type, type_tables.id_to_type.numel(), *rest, int(seed) & (2**64 - 1), int(global_step),
              type_tables.padded_size, int(mode), int(bool(direct)), buf.data_ptr(), buf.numel() * 4, _stream())
    return out


class Events:
    """hipEvent_t handles from the C ABI (ge_event_*), recorded on the launch stream."""

    def __init__(self, n: int):
        import ctypes as C
        self.handles = []
        for _ in range(n):
            h = C.c_void_p()
            _lib.call("ge_event_create", C.byref(h))
            self.handles.append(h.value)

    def record(self, i: int):
        _lib.call("ge_event_record", self.handles[i], _stream())

    def elapsed_ms(self, i: int, j: int) -> float:
        import ctypes as C
        ms = C.c_float()
        _lib.call("ge_event_elapsed_ms", self.handles[i], self.handles[j], C.byref(ms))
        return float(ms.value)

    def close(self):
        for h in self.handles:
            _lib.load().ge_event_destroy(h)
        self.handles = []


class BernoulliSampler:
    """Filtered Bernoulli negative sampler: the GPU form of the reference's native init.so
    (init.cpp:159-246) for tables that share relation and entity rows (holE.py layout: entities are
    rows [relation_count, entity_count)).  Known triples -> two sorted device indexes + per-relation
    tail-corruption thresholds from tails-per-head / heads-per-tail (init.cpp:107-127, defects fixed)."""

    def __init__(self, known_triples: np.ndarray, relation_count: int, entity_count: int, device="cuda", *,
                 ent_lo: Optional[int] = None):
        """entity_count counts table rows; entities are rows [ent_lo, entity_count).  ent_lo defaults to
        relation_count (the shared holE.py table); ent_lo=0 serves a separate entity table (the TransX models)."""
        tri = np.unique(np.asarray(known_triples, dtype=np.int64), axis=0)
        R = int(relation_count)
        lo = R if ent_lo is None else int(ent_lo)
        self.n_rel, self.ent_lo, self.n_ent = R, lo, int(entity_count) - lo
        bh = tri[np.lexsort((tri[:, 1], tri[:, 2], tri[:, 0]))]
        bt = tri[np.lexsort((tri[:, 0], tri[:, 2], tri[:, 1]))]
        freq = np.bincount(tri[:, 2], minlength=R).astype(np.float64)
        n_hr = np.bincount(np.unique(tri[:, [0, 2]], axis=0)[:, 1], minlength=R).astype(np.float64)
        n_tr = np.bincount(np.unique(tri[:, [1, 2]], axis=0)[:, 1], minlength=R).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            tph = np.where(n_hr > 0, freq / n_hr, 1.0)
            hpt = np.where(n_tr > 0, freq / n_tr, 1.0)
        thr = np.minimum(np.floor(hpt / (hpt + tph) * 4294967296.0), 4294967295.0).astype(np.uint32)
        to = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a.astype(dt))).to(device)
        self.bh_key, self.bh_ent = to(bh[:, 0] * R + bh[:, 2], np.int64), to(bh[:, 1], np.int32)
        self.bt_key, self.bt_ent = to(bt[:, 1] * R + bt[:, 2], np.int64), to(bt[:, 0], np.int32)
        self.tail_threshold = torch.as_tensor(thr.view(np.int32)).to(device)   # bit pattern of the uint32s
        self.n_known = int(len(tri))

    def corrupt(self, triples: torch.Tensor, *, seed: int = 0, step: int = 0) -> torch.Tensor:
        tb = _triples(triples, "triples")
        neg = torch.empty_like(tb)
        _lib.call("ge_bernoulli_corrupt_batch", tb.data_ptr(), tb.shape[0], self.bh_key.data_ptr(),
                  self.bh_ent.data_ptr(), self.bt_key.data_ptr(), self.bt_ent.data_ptr(), self.n_known,
                  self.tail_threshold.data_ptr(), self.n_rel, self.ent_lo, self.n_ent,
                  int(seed) & (2**64 - 1), int(step) & (2**64 - 1), neg.data_ptr(), _stream())
        return neg
