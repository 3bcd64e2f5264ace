"""Nearest-neighbour entity search (the third use of the embeddings the reference names, README.md:23-29: "search for
associated entities using k-nearest neighbors"; its demo lists, README.md:58-108, are cosine neighbours).

For query rows q and candidate rows c of a float32 table, used as stored:
    u_x = x / |x| (0 for a zero row),  cos = u_q . u_c
    cosine     D = max(0, 1 - cos)
    euclidean  D = sqrt(max(0, |q|^2 + |c|^2 - 2 |q| |c| cos))
and per query the first k candidates in ascending (D, table row id).

Routes, chosen from embedding_dim and k (no switch):
  * fused (d <= 288, k <= 128): ge_neighbor_topk selects the lists inside the split-precision sweep; no [n, K] matrix;
  * stored (d <= 288, k > 128): ge_neighbor_dists' distances in chunks of at most 1024 rows, sorted on the device by
    evaluate._topk_of_losses.  Where both apply they return the same arrays;
  * torch (d > 288, or more candidates than the sweep addresses): normalised rows, an fp32 matmul, the same distance
    expressions and the same sort -- within rounding of the kernels, not bitwise.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib
from .evaluate import _topk_of_losses
from .hole import _need_cuda, _stream

METRICS = {"cosine": 0, "euclidean": 1}     # GE_METRIC_COSINE / GE_METRIC_EUCLIDEAN
MAX_K = 128                                  # ge_neighbor_max_k()
MAX_DIM = 288                                # ge_neighbor_max_dim()
STORED_ROWS = 1024                           # rows per chunk of the stored and torch routes
FUSED_BATCH = 16384                          # default rows per ge_neighbor_topk call (its workspace grows with them)
_MAX_CELLS = 1 << 28                         # a stored chunk's [rows, K] matrix stays below 1 GiB


def _check_table(table) -> tuple:
    if not isinstance(table, torch.Tensor):
        raise ValueError("table must be a torch float32 [N, d] tensor")
    if table.dtype != torch.float32 or table.dim() != 2 or table.shape[0] < 1 or table.shape[1] < 1:
        raise ValueError(f"table must be a float32 [N, d] tensor with N, d >= 1, got {table.dtype} {tuple(table.shape)}")
    if not table.is_contiguous():
        raise ValueError("table must be contiguous")
    return int(table.shape[0]), int(table.shape[1])


def _ids(x, n: int, name: str, distinct: bool = False) -> np.ndarray:
    """Row ids as a host int64 array, checked: one dimension, integers, inside [0, n), distinct if asked."""
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if a.dtype == bool or not np.issubdtype(a.dtype, np.integer):
        if a.size == 0:
            a = a.astype(np.int64)
        else:
            raise ValueError(f"{name} must be integer row ids, got dtype {a.dtype}")
    if a.ndim != 1:
        raise ValueError(f"{name} must be one-dimensional, got shape {a.shape}")
    a = a.astype(np.int64)
    if a.size and (a.min() < 0 or a.max() >= n):
        raise ValueError(f"{name} must lie in [0, {n}): got {int(a.min())} ... {int(a.max())}")
    if distinct and np.unique(a).size != a.size:
        raise ValueError(f"{name} must be distinct")
    return a


def _candidates(candidates, n: int) -> np.ndarray:
    cand = np.arange(n, dtype=np.int64) if candidates is None else _ids(candidates, n, "candidates", distinct=True)
    if cand.size == 0:
        raise ValueError("candidates must not be empty")
    if cand.size > np.iinfo(np.int32).max:
        raise ValueError("more than 2^31 - 1 candidates")
    return cand


class NeighborPlanes:
    """The candidates of a nearest-neighbour search as the sweep reads them (ge_neighbor_planes: unit rows * 2^8 as fp16
    high halves and remainders, and the rows' norms), built once per (table, candidate list) for any number of
    nearest() calls.  `buffer` is None when the sweep does not apply (embedding_dim > 288, or more candidates than it
    addresses): nearest() then takes the torch route.  Rebuild after the table changes."""

    def __init__(self, table: torch.Tensor, candidates=None):
        n, d = _check_table(table)
        cand = _candidates(candidates, n)
        _need_cuda(table, "table")
        self.key = (table.data_ptr(), n, d)
        self.cand_np = cand
        self.cand64 = torch.as_tensor(cand).to(table.device)
        self.cand = self.cand64.to(torch.int32).contiguous()
        self.buffer = None
        nbytes = int(_lib.load().ge_neighbor_planes_bytes(cand.size, d)) if d <= MAX_DIM else 0
        if nbytes > 0:
            self.buffer = torch.empty(nbytes, dtype=torch.uint8, device=table.device)   # (256-byte aligned)
            _lib.call("ge_neighbor_planes", table.data_ptr(), n, d, self.cand.data_ptr(), cand.size,
                      self.buffer.data_ptr(), _stream())


def _check_k(k) -> int:
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError(f"k must be an integer >= 1, got {k!r}")
    return int(k)


def route(d: int, k: int) -> str:
    """The route nearest() takes for embedding_dim d and k (when the candidates fit the sweep)."""
    if d > MAX_DIM:
        return "torch"
    return "fused" if k <= MAX_K else "stored"


def _self_cells(q: np.ndarray, cand: np.ndarray, n: int, dev):
    """(row, column) of every query's own row among the candidates -- the cells exclude_self removes."""
    pos = np.full(n, -1, dtype=np.int64)
    pos[cand] = np.arange(cand.size)
    col = pos[q]
    rows = np.nonzero(col >= 0)[0]
    return torch.as_tensor(rows).to(dev), torch.as_tensor(col[rows]).to(dev)


def _distances_torch(cq: torch.Tensor, nq: torch.Tensor, nc: torch.Tensor, metric: int) -> torch.Tensor:
    """The kernels' distance expressions on a [b, K] cos matrix (fp32)."""
    if metric == 0:
        return (1.0 - cq).clamp_min(0.0)
    s = (nq * nq)[:, None] + (nc * nc)[None, :] - ((2.0 * nq)[:, None] * nc[None, :]) * cq
    return s.clamp_min(0.0).sqrt()


@torch.no_grad()
def nearest(table: torch.Tensor, queries, k: int, *, candidates=None, metric: str = "cosine", exclude_self: bool = True,
            planes: Optional[NeighborPlanes] = None, batch: Optional[int] = None):
    """The k nearest candidates of every query row: (ids int64 [n, k], dist float32 [n, k]) numpy arrays in the queries'
    order, ascending (D, row id).  candidates: row ids (distinct; None = every row).  exclude_self: a query's own row
    is not its neighbour (a duplicate row is).  Padding -1 / +inf when fewer candidates are eligible; a query that meets
    a NaN distance at an eligible candidate gets -1 / NaN.  planes: NeighborPlanes(table, candidates) shared between
    calls.  batch: queries per fused call (default 16384).
    Ids, shapes and dtypes are checked on the host before any GPU call (ValueError)."""
    n_rows, d = _check_table(table)
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}, got {metric!r}")
    k = _check_k(k)
    q = _ids(queries, n_rows, "queries")
    if planes is not None:
        if not isinstance(planes, NeighborPlanes):
            raise ValueError("planes must be a NeighborPlanes")
        if candidates is not None and not np.array_equal(_candidates(candidates, n_rows), planes.cand_np):
            raise ValueError("planes were built for another candidate list")
        if planes.key != (table.data_ptr(), n_rows, d):
            raise ValueError("planes were built for another table")
        cand = planes.cand_np
    else:
        cand = _candidates(candidates, n_rows)
    if batch is not None and (isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or
                              not 1 <= batch <= (1 << 28)):
        raise ValueError(f"batch must be an integer in [1, 2^28], got {batch!r}")
    _need_cuda(table, "table")
    m = METRICS[metric]
    n, K, dev = q.size, cand.size, table.device
    if n == 0:
        return np.zeros((0, k), dtype=np.int64), np.zeros((0, k), dtype=np.float32)
    how = route(d, k)
    if how != "torch":
        if planes is None:
            planes = NeighborPlanes(table, cand)
        if planes.buffer is None:       # more candidates than the sweep addresses
            how = "torch"
    if planes is not None:
        cand64 = planes.cand64
    else:
        cand64 = torch.as_tensor(cand).to(dev)
    qd = torch.as_tensor(q.astype(np.int32)).to(dev)
    ids_all, dist_all = [], []
    if how == "fused":
        b0 = min(n, int(batch or FUSED_BATCH))
        ws = torch.empty(int(_lib.load().ge_neighbor_workspace_bytes(b0, K, k)), dtype=torch.uint8, device=dev)
        for s in range(0, n, b0):
            qb = qd[s:s + b0]
            b = qb.numel()
            oid = torch.empty((b, k), dtype=torch.int32, device=dev)
            od = torch.empty((b, k), dtype=torch.float32, device=dev)
            _lib.call("ge_neighbor_topk", table.data_ptr(), n_rows, d, qb.data_ptr(), b, planes.cand.data_ptr(), K, k, m,
                      int(bool(exclude_self)), planes.buffer.data_ptr(), oid.data_ptr(), od.data_ptr(), ws.data_ptr(),
                      ws.numel(), _stream())
            ids_all.append(oid.to(torch.int64).cpu().numpy())
            dist_all.append(od.cpu().numpy())
    else:
        rows = max(1, min(STORED_ROWS, _MAX_CELLS // K))
        if how == "torch":
            norms = torch.linalg.vector_norm(table, dim=1)
            inv = torch.where(norms == 0, torch.zeros_like(norms), 1.0 / norms)
            uc = table[cand64] * inv[cand64, None]
            nc = norms[cand64]
        for s in range(0, n, rows):
            qb = qd[s:s + rows]
            b = qb.numel()
            if how == "stored":
                L = torch.empty((b, K), dtype=torch.float32, device=dev)
                _lib.call("ge_neighbor_dists", table.data_ptr(), n_rows, d, qb.data_ptr(), b, planes.cand.data_ptr(), K, m,
                          planes.buffer.data_ptr(), L.data_ptr(), _stream())
            else:
                ql = qb.long()
                cq = torch.matmul(table[ql] * inv[ql, None], uc.t())
                L = _distances_torch(cq, norms[ql], nc, m)
            known = _self_cells(q[s:s + b], cand, n_rows, dev) if exclude_self else None
            ids, vals = _topk_of_losses(L, cand64, k, known)
            ids_all.append(ids.cpu().numpy())
            dist_all.append(vals.cpu().numpy())
    return np.concatenate(ids_all).astype(np.int64), np.concatenate(dist_all).astype(np.float32)


def neighbor_lines(query_ids, ids, dists, names=None) -> list:
    """TSV lines of a neighbour list, one per (query, position), positions from 1, padding (-1) left out:
    with names (a dict id -> name, missing ids by number) `query  query_name  position  neighbor  neighbor_name
    distance`, without `query  position  neighbor  distance`; distances as %.9g (float32 round trip)."""
    out = []
    for qi, row_id, row_d in zip(query_ids, ids, dists):
        qi = int(qi)
        for j, (c, v) in enumerate(zip(row_id, row_d)):
            c = int(c)
            if c < 0:
                continue
            if names is None:
                out.append("%d\t%d\t%d\t%.9g\n" % (qi, j + 1, c, float(v)))
            else:
                out.append("%d\t%s\t%d\t%d\t%s\t%.9g\n" % (qi, names.get(qi, str(qi)), j + 1, c, names.get(c, str(c)),
                                                          float(v)))
    return out


def write_neighbors(path: str, table: torch.Tensor, queries, k: int, *, candidates=None, metric: str = "cosine",
                    names=None) -> int:
    """nearest(table, queries, k, candidates, metric, exclude_self=True) as neighbor_lines into `path` (truncated);
    returns the number of lines."""
    q = _ids(queries, _check_table(table)[0], "queries")
    ids, dist = nearest(table, q, k, candidates=candidates, metric=metric, exclude_self=True)
    lines = neighbor_lines(q, ids, dist, names)
    with open(path, "w") as f:
        f.writelines(lines)
    return len(lines)
