"""Link-prediction ranking and MRR / Hits@n (holE.py:427-490), with the candidate sweep on the GPU.

Orientation: E = sigmoid(score) is a loss, candidates are ranked ASCENDING by it (min-heap pop order,
holE.py:446-447); ties are broken by the (head, tail, relation) tuple (holE.py:434).
raw_rank counts every popped candidate; filtered_rank skips candidates that are known-true
train/valid triples (holE.py:454-463); ranks are recorded for tails in the test set
(holE.py:464-466).  The reference evaluator is wired to Diffbot-specific candidates
(holE.py:534-541); here the same ranking semantics run 1-vs-all over a candidate list through
ge_complex_score_1vK (fp32-MFMA GEMM), for tails and -- as FB15k protocols need -- heads.
"""
from __future__ import annotations

from collections import defaultdict

import numpy as np
import torch

from . import hole as H
from .transx import ids_outside


def mrr_and_hits(raw_ranks, filtered_ranks) -> dict:
    """The summary numbers of holE.py:475-490 from rank arrays: reciprocal-rank means, mean ranks and the
    share of filtered ranks within 1 / 3 / 10 (percent)."""
    raw = np.asarray(raw_ranks, dtype=np.float64)
    fil = np.asarray(filtered_ranks, dtype=np.float64)
    pct = lambda n: 100.0 * float(np.count_nonzero(fil <= n)) / max(1, fil.size)
    return {"raw_mrr": float((1.0 / raw).mean()), "mean_raw_pos": float(raw.mean()),
            "filtered_mrr": float((1.0 / fil).mean()), "mean_filtered_pos": float(fil.mean()),
            "hits1": pct(1), "hits3": pct(3), "hits10": pct(10)}


class KnownIndex:
    """Known-true triples as a device-side sorted index: key = fixed entity * n_rows + relation -> the entities
    that complete a known triple (tails for side="tail", heads for "head").  side="relation": key = head * n_rows +
    tail -> the relations that link the pair (n_rows must hold every entity and relation id); cells(h, t, pos_of,
    n_rel) then lists the known relations of (h, ?, t) rows."""

    def __init__(self, known_triples, n_rows: int, side: str, device):
        self.n_rows = int(n_rows)
        if known_triples is None or len(known_triples) == 0:
            self.key = torch.empty(0, dtype=torch.int64, device=device)
            self.ent = torch.empty(0, dtype=torch.int64, device=device)
            return
        k = torch.as_tensor(np.asarray(known_triples, dtype=np.int64)).to(device)
        if side == "relation":              # (head, tail) -> relation
            fixed, second, other = k[:, 0], k[:, 1], k[:, 2]
        else:
            fixed, other = (k[:, 0], k[:, 1]) if side == "tail" else (k[:, 1], k[:, 0])
            second = k[:, 2]
        # a set, like the reference's dict of sets (holE.py:413-422), sorted by (fixed, relation, other)
        if self.n_rows ** 3 < 2 ** 63:      # one radix sort of the triple packed into an int64
            packed = torch.unique_consecutive(torch.sort((fixed * self.n_rows + second) * self.n_rows + other)[0])
            self.key, self.ent = (packed // self.n_rows).contiguous(), (packed % self.n_rows).contiguous()
        else:
            pairs = torch.unique(torch.stack([fixed * self.n_rows + second, other], 1), dim=0)
            self.key, self.ent = pairs[:, 0].contiguous(), pairs[:, 1].contiguous()

    def cells(self, fixed: torch.Tensor, rel: torch.Tensor, pos_of: torch.Tensor, n_cand: int):
        """(row, candidate position) of every known-true candidate of the query rows, as the per-tile lists
        ge_complex_rank_1vK takes: (known_off int32 [tiles+1], known_rc int16) -- ge_known_cells: a counting pass, the total
        read back (the call's one synchronisation), a filling pass."""
        B = fixed.numel()
        dev = fixed.device
        if dev.type != "cuda" or pos_of.dtype != torch.int64 or not pos_of.is_cuda:
            raise ValueError("KnownIndex.cells runs on the GPU (ge_known_cells): CUDA tensors, pos_of int64")
        n_tiles = ((B + 127) // 128) * ((n_cand + 127) // 128)
        off = torch.empty(n_tiles + 1, dtype=torch.int32, device=dev)
        scratch = torch.empty(max(n_tiles, 1), dtype=torch.int32, device=dev)
        fixed, rel = fixed.to(torch.int64).contiguous(), rel.to(torch.int64).contiguous()
        args = (self.key.data_ptr(), self.ent.data_ptr(), self.key.numel(), fixed.data_ptr(), rel.data_ptr(), B,
                pos_of.data_ptr(), self.n_rows, n_cand, scratch.data_ptr(), off.data_ptr())
        H._lib.call("ge_known_cells", 0, *args, None, H._stream())
        total = int(off[-1])
        rc = torch.empty(max(total, 1), dtype=torch.int16, device=dev)
        if total:
            H._lib.call("ge_known_cells", 1, *args, rc.data_ptr(), H._stream())
        else:
            rc.zero_()
        return off, rc


class CandidateSets:
    """Per-relation candidate sets of a sweep over `candidates` (the type-constrained, domain / range protocol; the
    reference's InferenceCandidates, holE.py:493-499, 535-541, gives each group of relations its own tail candidates and
    leaves "get candidate tail type from training triples" as a TODO, holE.py:533): set s admits a subset of the
    candidate list, and a query row is ranked against / predicts from the set named by its row set (default: its
    relation id).
      mask     int32 [n_sets, 4 * ceil(K / 128)] on the device: bit c & 31 of word c >> 5 = the candidate at position c
      n_sets, counts (int64 [n_sets] numpy: admissible candidates per set), cand (the int32 device candidate ids)
    The host part of each builder -- cell lists, allow bitmaps -- is plain numpy (the static methods); the mask itself is
    built on the device (ge_candidate_mask_from_cells / ge_candidate_mask_from_classes)."""

    def __init__(self, cand: torch.Tensor, mask: torch.Tensor, counts: np.ndarray):
        self.cand, self.mask = cand, mask
        self.n_sets = int(mask.shape[0])
        self.counts = np.asarray(counts, dtype=np.int64)

    # ---- host parts
    @staticmethod
    def _candidates(candidates) -> np.ndarray:
        c = np.asarray(candidates.cpu() if isinstance(candidates, torch.Tensor) else candidates, dtype=np.int64).reshape(-1)
        if c.size == 0 or c.min() < 0 or np.unique(c).size != c.size:
            raise ValueError("candidates must be distinct non-negative ids")
        return c

    @staticmethod
    def positions_of(candidates: np.ndarray, ids: np.ndarray) -> np.ndarray:
        """Position of every id in the candidate list (-1: not a candidate)."""
        ids = np.asarray(ids, dtype=np.int64)
        order = np.argsort(candidates, kind="stable")
        j = np.searchsorted(candidates[order], ids)
        j = np.minimum(j, candidates.size - 1)
        pos = order[j]
        return np.where(candidates[pos] == ids, pos, -1)

    @staticmethod
    def cells_from_lists(candidates, lists: dict, n_sets: int = None):
        """(cells int32 [M,2] = distinct (set, candidate position) pairs, n_sets) of explicit lists {set: entity ids}.
        An id that is no candidate, or a set index outside [0, n_sets), is a ValueError."""
        cand = CandidateSets._candidates(candidates)
        keys = [int(k) for k in lists.keys()]
        if n_sets is None:
            n_sets = max(keys) + 1 if keys else 1
        if n_sets < 1 or any(k < 0 or k >= n_sets for k in keys):
            raise ValueError("a set index is outside [0, n_sets)")
        parts = []
        for k, ids in lists.items():
            pos = CandidateSets.positions_of(cand, np.asarray(list(ids), dtype=np.int64).reshape(-1))
            if (pos < 0).any():
                raise ValueError(f"set {k} lists an id that is not a candidate")
            parts.append(np.stack([np.full(pos.size, int(k), dtype=np.int64), pos], 1))
        cells = np.unique(np.concatenate(parts, 0), axis=0) if parts else np.zeros((0, 2), dtype=np.int64)
        return cells.astype(np.int32).reshape(-1, 2), int(n_sets)

    @staticmethod
    def _side_columns(triples, relation_count: int, side: str):
        if side not in ("tail", "head"):
            raise ValueError("side must be 'tail' or 'head'")
        t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
        if relation_count < 1 or (t.size and (t[:, 2].min() < 0 or t[:, 2].max() >= relation_count)):
            raise ValueError("a triple's relation is outside [0, relation_count)")
        return t[:, 2], t[:, 1 if side == "tail" else 0]

    @staticmethod
    def cells_from_observed(candidates, triples, relation_count: int, side: str) -> np.ndarray:
        """cells int32 [M,2]: set r = the candidates seen on `side` of relation r in `triples` ([n,3] head, tail, relation);
        entities that are no candidates are dropped."""
        cand = CandidateSets._candidates(candidates)
        rel, ent = CandidateSets._side_columns(triples, relation_count, side)
        pos = CandidateSets.positions_of(cand, ent)
        keep = pos >= 0
        cells = np.unique(np.stack([rel[keep], pos[keep]], 1), axis=0) if keep.any() else np.zeros((0, 2), dtype=np.int64)
        return cells.astype(np.int32).reshape(-1, 2)

    @staticmethod
    def type_codes(id_to_type, n_rows: int = None) -> np.ndarray:
        """int32 type code per table row (-1: no type) from an integer array, or from a dict id -> type name."""
        if isinstance(id_to_type, dict):
            n = (max(id_to_type) + 1 if id_to_type else 0) if n_rows is None else int(n_rows)
            names = {ty: i for i, ty in enumerate(sorted(set(id_to_type.values()), key=str))}
            codes = np.full(n, -1, dtype=np.int32)
            for idx, ty in id_to_type.items():
                if 0 <= idx < n:
                    codes[idx] = names[ty]
            return codes
        codes = np.asarray(id_to_type)
        if codes.ndim != 1 or codes.dtype.kind not in "iu":
            raise ValueError("id_to_type must be a 1-d integer array of type codes (or a dict id -> type)")
        return codes.astype(np.int32)

    @staticmethod
    def allow_from_types(id_to_type, triples, relation_count: int, side: str):
        """(codes int32 [n_rows], allow uint32 [relation_count, ceil(n_class / 32)], n_class): bit t of allow[r] = some
        triple of relation r has an entity of type t on `side` (untyped entities, code < 0, allow nothing)."""
        codes = CandidateSets.type_codes(id_to_type)
        rel, ent = CandidateSets._side_columns(triples, relation_count, side)
        if ent.size and (ent.min() < 0 or ent.max() >= codes.size):
            raise ValueError("a triple's entity has no entry in id_to_type")
        n_class = max(1, int(codes.max()) + 1 if codes.size else 1)
        allow = np.zeros((relation_count, (n_class + 31) // 32), dtype=np.uint32)
        ty = codes[ent].astype(np.int64)
        keep = ty >= 0
        pairs = np.unique(np.stack([rel[keep], ty[keep]], 1), axis=0) if keep.any() else np.zeros((0, 2), dtype=np.int64)
        np.bitwise_or.at(allow, (pairs[:, 0], pairs[:, 1] >> 5), (np.uint32(1) << (pairs[:, 1] & 31).astype(np.uint32)))
        return codes, allow, n_class

    # ---- builders
    @classmethod
    def _from_cells(cls, candidates, cells: np.ndarray, n_sets: int, device) -> "CandidateSets":
        cand = torch.as_tensor(cls._candidates(candidates).astype(np.int32)).to(device)
        K = cand.numel()
        mask = torch.empty(n_sets, H.candidate_mask_words(K), dtype=torch.int32, device=device)
        c = torch.as_tensor(np.ascontiguousarray(cells, dtype=np.int32)).to(device)
        H._lib.call("ge_candidate_mask_from_cells", c.data_ptr(), c.shape[0], n_sets, K, mask.data_ptr(), H._stream())
        counts = np.bincount(cells[:, 0], minlength=n_sets) if len(cells) else np.zeros(n_sets, dtype=np.int64)
        return cls(cand, mask, counts)

    @classmethod
    def from_lists(cls, candidates, lists: dict, n_sets: int = None, device="cuda") -> "CandidateSets":
        """Explicit lists {set: entity ids} (the reference's per-group candidate lists, holE.py:495)."""
        cells, n_sets = cls.cells_from_lists(candidates, lists, n_sets)
        return cls._from_cells(candidates, cells, n_sets, device)

    @classmethod
    def from_observed(cls, candidates, triples, relation_count: int, side: str, device="cuda") -> "CandidateSets":
        """Set r = the candidates seen on `side` ("tail" / "head") of relation r in `triples`."""
        return cls._from_cells(candidates, cls.cells_from_observed(candidates, triples, relation_count, side),
                               int(relation_count), device)

    @classmethod
    def from_types(cls, candidates, id_to_type, triples, relation_count: int, side: str, device="cuda") -> "CandidateSets":
        """Set r = every candidate whose type was seen on `side` of relation r in `triples` (the reference's TODO,
        holE.py:533).  id_to_type: int type code per table row (HolEData.type_arrays()[1]; -1: none), or a dict."""
        cand_np = cls._candidates(candidates)
        codes, allow, n_class = cls.allow_from_types(id_to_type, triples, relation_count, side)
        if cand_np.max() >= codes.size:
            raise ValueError("a candidate has no entry in id_to_type")
        cand_class = codes[cand_np]
        cand = torch.as_tensor(cand_np.astype(np.int32)).to(device)
        K = cand.numel()
        mask = torch.empty(int(relation_count), H.candidate_mask_words(K), dtype=torch.int32, device=device)
        cc = torch.as_tensor(np.ascontiguousarray(cand_class, dtype=np.int32)).to(device)
        al = torch.as_tensor(allow.view(np.int32)).to(device)
        H._lib.call("ge_candidate_mask_from_classes", cc.data_ptr(), K, al.data_ptr(), int(relation_count), n_class,
                    mask.data_ptr(), H._stream())
        hist = np.bincount(cand_class[cand_class >= 0], minlength=n_class).astype(np.int64)
        bits = (allow[:, np.arange(n_class) >> 5] >> (np.arange(n_class) & 31).astype(np.uint32)) & 1
        return cls(cand, mask, bits.astype(np.int64) @ hist)

    # ---- what the host-side paths read
    def _check(self, cand: torch.Tensor, who: str):
        if self.cand.numel() != cand.numel() or not bool(torch.equal(self.cand.to(cand.device), cand.to(torch.int32))):
            raise ValueError(f"{who}: candidate_sets were built for another candidate list")

    def row_sets(self, row_sets, default: torch.Tensor, who: str) -> torch.Tensor:
        """int64 device row sets of a chunk (default: the rows' relation ids), range-checked."""
        rs = default if row_sets is None else torch.as_tensor(np.asarray(row_sets, dtype=np.int64)).to(default.device)
        if rs.dim() != 1 or rs.numel() != default.numel():
            raise ValueError(f"{who}: row_sets must have one entry per row")
        if rs.numel() and bool(((rs < -1) | (rs >= self.n_sets)).any()):
            raise ValueError(f"{who}: a row's set index is outside [-1, {self.n_sets})")
        return rs.to(torch.int64)

    def admissible(self, rs: torch.Tensor, pos: torch.Tensor = None) -> torch.Tensor:
        """bool [b, K] (pos None), or bool [b] for candidate position pos[i] of row i: admissible in row set rs[i]."""
        rows = self.mask[rs.clamp(min=0)]
        if pos is None:
            p = torch.arange(self.cand.numel(), device=rows.device)
            bits = (rows[:, p >> 5] >> (p & 31).to(torch.int32)) & 1
            return (bits != 0) | (rs < 0).view(-1, 1)
        bits = (rows.gather(1, (pos >> 5).view(-1, 1)).view(-1) >> (pos & 31).to(torch.int32)) & 1
        return (bits != 0) | (rs < 0)


@torch.no_grad()
def link_prediction_ranks(embeddings: torch.Tensor, test_triples: np.ndarray, candidates: np.ndarray,
                          known_triples: np.ndarray = None, side: str = "tail", batch: int = None,
                          max_norm: float = 1.0, fused: bool = None, model: str = "complex", planes=None,
                          infer_threshold: float = None, return_confident: bool = False, candidate_sets=None,
                          row_sets=None, return_admissible: bool = False):
    """Raw and filtered rank of every test triple's true entity among `candidates`, with the
    semantics of holE.py:446-469.  side="tail": candidates replace the tail; "head": the head.
    known_triples: an [n,3] array, or a KnownIndex built for this side (evaluate_fb15k_style keeps the two it builds).
    Returns (raw_ranks, filtered_ranks) int64 arrays.  The true entity must be a candidate.
    fused (default: whenever the kernel supports embedding_dim): the ranks are counted in the candidate
    GEMM's epilogue (ge_complex_rank_1vK) and no [B,K] score matrix is materialised; otherwise the scores
    of ge_complex_score_1vK are ranked with tensor ops.
    model: "complex"; "hole" (README.md:42 on a real-valued table: a copy is taken to the frequency domain once,
    where HolE is the ComplEx-shaped form the sweep computes) or "hole_spectral" (table already there).  HolE
    needs the fused sweep.
    planes: H.RankPlanes of (embeddings, candidates) shared between calls (tails then heads: evaluate_fb15k_style); built
    here otherwise -- once for all the batches of the call.
    infer_threshold: the reference's gate (holE.py:436-438, flag holE.py:616): a sweep is `is_confident` when the lowest
    loss among its candidates is below the threshold, and ONLY confident sweeps record their positions (holE.py:464-466)
    -- the returned arrays then hold the confident rows' ranks only (return_confident=True adds the bool mask over all
    test rows).  None: every row is recorded (the reference with a threshold above every loss).
    candidate_sets (CandidateSets built for `candidates` and this side) / row_sets ([n], default each row's relation id;
    -1: unrestricted): every rank counts only the candidates admissible in the row's set; the true entity need not be one
    of them (return_admissible=True adds the bool array "true entity admissible in its set").  On the split-precision
    sweep this is the masked kernel; elsewhere (fused=False, other embedding_dims) the same ranks come from stored losses
    in chunks of 1024 rows.  Not combined with infer_threshold."""
    assert side in ("tail", "head")
    if candidate_sets is None and (row_sets is not None or return_admissible):
        raise ValueError("row_sets / return_admissible need candidate_sets")
    if candidate_sets is not None and infer_threshold is not None:
        raise ValueError("candidate_sets with infer_threshold is not implemented")
    if model not in ("complex", "hole", "hole_spectral"):
        raise ValueError(f"unknown model {model!r}")
    dev = embeddings.device
    d = embeddings.shape[1]
    can_fuse = H.rank_fused_ok(d, max_norm)
    if fused is None:
        fused = can_fuse
    if model != "complex":
        if not (fused and can_fuse):
            raise ValueError("HolE link prediction needs the fused sweep: embedding_dim a multiple of 8, <= %d" % H.rank_max_dim())
        if model == "hole":
            embeddings = H.hole_to_spectral(embeddings.detach().clone())
        model = "hole_spectral"
    test = np.asarray(test_triples, dtype=np.int64)
    cand = torch.as_tensor(np.asarray(candidates, dtype=np.int32)).to(dev)
    cand64 = cand.to(torch.int64)
    # position of every row id in the candidate list (-1: not a candidate)
    pos_of = torch.full((embeddings.shape[0],), -1, dtype=torch.int64, device=dev)
    pos_of[cand64] = torch.arange(cand.numel(), device=dev)
    index = known_triples if isinstance(known_triples, KnownIndex) else KnownIndex(known_triples, embeddings.shape[0], side, dev)
    if batch is None:
        # test rows per call: the stored-scores path holds a [batch, K] fp32 matrix; the fused sweep holds nothing
        # per row, and longer calls amortise its per-row-block set-up (the whole FB15k test set is one call)
        batch = 1 << 17 if fused else 16384
    # candidate sets: the masked sweep where the split-precision kernel runs, stored losses elsewhere
    in_kernel = fused and (candidate_sets is None or H.split_sweep_ok(d, max_norm))
    if candidate_sets is not None:
        candidate_sets._check(cand, "link_prediction_ranks")
        if row_sets is not None and len(row_sets) != len(test):
            raise ValueError("row_sets must have one entry per test triple")
        if not in_kernel:
            batch = min(batch, 1024)
    raw_all, fil_all, conf_all, adm_all = [], [], [], []
    fixed_col, true_col = (0, 1) if side == "tail" else (1, 0)
    if fused and planes is None:
        planes = H.RankPlanes(embeddings, cand, max_norm=max_norm, model=model)
    if planes is not None:
        # the planes' own id tensor is handed to the kernel: it has to BE this candidate list (pos_of and the known cells
        # below are built from the caller's), not merely as long
        if planes.cand.numel() != cand.numel() or not bool(torch.equal(planes.cand.to(dev), cand)):
            raise ValueError("`planes` were built for another candidate list")
        cand = planes.cand
    for s in range(0, len(test), batch):
        chunk = torch.as_tensor(test[s:s + batch]).to(dev)
        fixed, rel, true_id = chunk[:, fixed_col], chunk[:, 2], chunk[:, true_col]
        hr = torch.stack([fixed, rel], 1).to(torch.int32)
        tpos = pos_of[true_id]
        if (tpos < 0).any():
            raise ValueError("a test triple's true entity is not in the candidate list")
        off, rc = index.cells(fixed, rel, pos_of, cand.numel())
        rs = None
        if candidate_sets is not None:
            rs = candidate_sets.row_sets(None if row_sets is None else row_sets[s:s + batch], rel, "link_prediction_ranks")
            adm_all.append(candidate_sets.admissible(rs, tpos).cpu().numpy())
        if in_kernel:
            n_before, n_known = H.rank_candidates(embeddings, hr, true_id, cand, known_off=off, known_rc=rc,
                                                  cand_is_head=(side == "head"), max_norm=max_norm, model=model, planes=planes,
                                                  candidate_sets=candidate_sets, row_sets=rs)
            raw = n_before.to(torch.int64) + 1
            fil = raw - n_known.to(torch.int64)
        else:
            if fused:                                # (candidate sets off the split-precision range: the sweep's own losses)
                scores = H.rank_candidates(embeddings, hr, true_id, cand, cand_is_head=(side == "head"), max_norm=max_norm,
                                           return_scores=True, model=model, planes=planes)[-1]
            else:
                scores = H.score_candidates(embeddings, hr, cand, cand_is_head=(side == "head"), max_norm=max_norm)
            s_true = scores.gather(1, tpos.view(-1, 1))
            # ascending by (loss, triple tuple): among equal losses the smaller entity id pops first
            before = (scores < s_true) | ((scores == s_true) & (cand64.view(1, -1) < true_id.view(-1, 1)))
            if rs is not None:
                before &= candidate_sets.admissible(rs)
            raw = before.sum(1) + 1
            # filtered: known-true candidates popped before the target do not advance the rank
            n_ct = (cand.numel() + 127) // 128
            tiles = torch.repeat_interleave(torch.arange(off.numel() - 1, device=dev), (off[1:] - off[:-1]).to(torch.int64))
            rcv = rc[:tiles.numel()].to(torch.int64)
            rows_t = (tiles // n_ct) * 128 + rcv // 128
            cols_t = (tiles % n_ct) * 128 + rcv % 128
            skipped = torch.zeros(chunk.shape[0], dtype=torch.int64, device=dev)
            if rows_t.numel():
                skipped.index_add_(0, rows_t, before[rows_t, cols_t].to(torch.int64))
            fil = raw - skipped
        if infer_threshold is not None:
            # is_confident: the sweep's lowest loss is below the threshold <=> some candidate ranks before a loss equal to it
            if fused:
                conf = H.confident_rows(embeddings, hr, cand, infer_threshold, cand_is_head=(side == "head"), max_norm=max_norm,
                                        model=model, planes=planes)
            else:
                conf = scores.min(dim=1).values < infer_threshold
            raw, fil = raw[conf], fil[conf]
            conf_all.append(conf.cpu().numpy())
        raw_all.append(raw.cpu().numpy())
        fil_all.append(fil.cpu().numpy())
    out = (np.concatenate(raw_all), np.concatenate(fil_all))
    if return_confident:
        out += (np.concatenate(conf_all) if conf_all else np.ones(len(test), dtype=bool),)
    if return_admissible:
        out += (np.concatenate(adm_all) if adm_all else np.zeros(0, dtype=bool),)
    return out


def constrained_sets(data, kind: str, candidates=None, device="cuda"):
    """(known, {side: CandidateSets}) of the type-constrained protocol: the sets of both sides over `candidates` (default
    the entity rows in id order) -- kind "types": every entity whose type was seen on that side of the relation;
    "observed": the entities seen there -- built from train + valid (`known`, the evaluation's filter too).  What
    evaluate_constrained ranks against and what train.py --softmax_candidate_sets trains against."""
    if kind not in ("types", "observed"):
        raise ValueError("kind must be 'types' or 'observed'")
    R, N = data.relation_count, data.entity_count
    cand = np.arange(R, N, dtype=np.int32) if candidates is None else np.asarray(candidates, dtype=np.int32)
    parts = [a for a in (data.triples, data.validation_triples) if a is not None]
    if not parts:
        raise ValueError("candidate sets are built from the train / valid triples: none found")
    known = np.concatenate(parts, 0)
    id_to_type = data.type_arrays()[1] if kind == "types" else None
    sets = {}
    for side in ("tail", "head"):
        sets[side] = (CandidateSets.from_types(cand, id_to_type, known, R, side, device=device) if kind == "types"
                      else CandidateSets.from_observed(cand, known, R, side, device=device))
    return known, sets


def evaluate_constrained(embeddings: torch.Tensor, data, kind: str, model: str = "complex", verbose: bool = True):
    """Type-constrained link prediction over data.test_array, both sides: each row is ranked against its relation's
    candidate set -- kind "types": every entity whose type was seen on that side of the relation; "observed": the
    entities seen there -- built from train + valid, which are also the filter.  Returns (block, {side: CandidateSets}):
    block = {"mrr_and_hits": ..., "admissible_true": share of rows whose true entity is in its set, "mean_set_size":
    the mean over the ranked rows of their set's size}."""
    if kind not in ("types", "observed"):
        raise ValueError("kind must be 'types' or 'observed'")
    R, N = data.relation_count, data.entity_count
    cand = np.arange(R, N, dtype=np.int32)
    known, sets = constrained_sets(data, kind, device=embeddings.device)
    if model == "hole":
        embeddings, model = H.hole_to_spectral(embeddings.detach().clone()), "hole_spectral"
    dev = embeddings.device
    planes = H.RankPlanes(embeddings, torch.as_tensor(cand).to(dev), model=model) if H.rank_fused_ok(embeddings.shape[1], 1.0) else None
    raw, fil, adm, size = [], [], [], []
    test = np.asarray(data.test_array, dtype=np.int64)
    for side in ("tail", "head"):
        cs = sets[side]
        r, f, a = link_prediction_ranks(embeddings, test, cand, known, side, model=model, planes=planes, candidate_sets=cs,
                                        return_admissible=True)
        raw.append(r); fil.append(f); adm.append(a); size.append(cs.counts[test[:, 2]])
    raw, fil, adm, size = (np.concatenate(x) for x in (raw, fil, adm, size))
    block = {"mrr_and_hits": mrr_and_hits(raw, fil), "admissible_true": float(adm.mean()) if adm.size else float("nan"),
             "mean_set_size": float(size.mean()) if size.size else float("nan")}
    if verbose:
        print("constrained: ({kind} sets) raw MRR {raw_mrr:.6f}; filtered MRR {filtered_mrr:.6f} (mean rank "
              "{mean_filtered_pos:.1f}); hits@1/3/10 {hits1:.2f} / {hits3:.2f} / {hits10:.2f} %; ".format(kind=kind, **block["mrr_and_hits"])
              + "true entity admissible {:.2f} %; mean set size {:.1f}".format(100.0 * block["admissible_true"], block["mean_set_size"]))
    return block, sets


def evaluate_fb15k_style(embeddings: torch.Tensor, data, both_sides: bool = True, batch: int = None,
                         verbose: bool = True, model: str = "complex", infer_threshold: float = None) -> dict:
    """Filtered link prediction over all entities (rows >= relation_count) for
    data.test_array, filtering train+valid triples as the reference does (holE.py:413-422).
    infer_threshold: the reference's is_confident gate (holE.py:436-438); the summary then covers the confident sweeps
    only and carries their number (`recorded` of `sweeps`)."""
    R, N = data.relation_count, data.entity_count
    cand = np.arange(R, N, dtype=np.int32)
    parts = [a for a in (data.triples, data.validation_triples) if a is not None]
    known = np.concatenate(parts, 0) if parts else None
    if model == "hole":                      # one transform for both sides
        embeddings, model = H.hole_to_spectral(embeddings.detach().clone()), "hole_spectral"
    d = embeddings.shape[1]
    planes = None                            # the candidates' fp16 planes: one build for tails and heads
    if H.rank_fused_ok(d, 1.0):              # (max_norm: the default of the calls below)
        planes = H.RankPlanes(embeddings, torch.as_tensor(cand).to(embeddings.device), model=model)
    # the known-triple indexes (a sort each) are kept on `data`: the train / valid splits do not change between the
    # evaluations of a training run
    cache = data.__dict__.setdefault("_known_index_cache", {}) if hasattr(data, "__dict__") else {}
    def known_index(side):
        # keyed on the IDENTITY of the split arrays (kept alive by `data`) as well as their length: a data object whose
        # train / valid triples are replaced by others of the same count must not reuse the old filter
        key = (side, str(embeddings.device), N, 0 if known is None else len(known), tuple(id(a) for a in parts))
        if key not in cache:
            cache[key] = KnownIndex(known, N, side, embeddings.device)
        return cache[key]
    raw_t, fil_t = link_prediction_ranks(embeddings, data.test_array, cand, known_index("tail"), "tail", batch, model=model,
                                         planes=planes, infer_threshold=infer_threshold)
    raw, fil = [raw_t], [fil_t]
    if both_sides:
        raw_h, fil_h = link_prediction_ranks(embeddings, data.test_array, cand, known_index("head"), "head", batch, model=model,
                                             planes=planes, infer_threshold=infer_threshold)
        raw.append(raw_h); fil.append(fil_h)
    raw, fil = np.concatenate(raw), np.concatenate(fil)
    sweeps = len(data.test_array) * (2 if both_sides else 1)
    if raw.size == 0:      # no sweep was confident: the reference would take the mean of nothing (holE.py:477)
        out = {k: float("nan") for k in ("raw_mrr", "mean_raw_pos", "filtered_mrr", "mean_filtered_pos", "hits1", "hits3", "hits10")}
    else:
        out = mrr_and_hits(raw, fil)
    out["recorded"], out["sweeps"] = int(raw.size), int(sweeps)
    if verbose and infer_threshold is not None:
        print(f"is_confident (lowest loss < {infer_threshold}): {raw.size} of {sweeps} sweeps recorded")
    if verbose:
        print("raw MRR {raw_mrr:.6f} (mean rank {mean_raw_pos:.1f}); filtered MRR {filtered_mrr:.6f} "
              "(mean rank {mean_filtered_pos:.1f}); hits@1/3/10 {hits1:.2f} / {hits3:.2f} / {hits10:.2f} %".format(**out))
    return out


class RankPocket:
    """Validation ticks on the evaluation's own metric without a host round trip per tick (ge_rank_validation_tick): each
    tick rebuilds the candidates' planes from the table as it is now, ranks every validation triple's tail and head among
    `candidates` (filtered by known_triples; with candidate_sets = {"tail": CandidateSets, "head": CandidateSets} each
    row against its relation's set, the constrained protocol of evaluate_constrained), takes the summary of mrr_and_hits
    into `hist`, and copies the table into `pocket` -- and `accumulator` into `pocket_accumulator` -- iff the filtered
    MRR is the best so far (`best`, a device scalar that starts at 0; a tie keeps the first).  The constructor does all
    that does not depend on the table; tick() enqueues one native call; read() synchronises once for all pending ticks.
    ValueError on the host: an empty validation set, a true entity that is no candidate, candidate sets outside the
    masked sweep's embedding_dim range, a relation without a set."""

    KEYS = ("filtered_mrr", "raw_mrr", "mean_filtered_pos", "mean_raw_pos", "hits1", "hits3", "hits10", "counted")

    def __init__(self, embeddings: torch.Tensor, validation_triples, candidates, known_triples=None, *, accumulator=None,
                 candidate_sets=None, max_norm: float = 1.0, keep_table: bool = True, capacity: int = 4096,
                 model: str = "complex"):
        self.model = H._sweep_model(model, "RankPocket", H._TRANSFORM_FIRST)
        self.emb = emb = H._table(embeddings)
        dev, (N, d) = emb.device, emb.shape
        self.max_norm = float(max_norm)
        valid = np.asarray(validation_triples.cpu() if isinstance(validation_triples, torch.Tensor) else validation_triples,
                           dtype=np.int64).reshape(-1, 3)
        if len(valid) == 0:
            raise ValueError("RankPocket: the validation set is empty")
        cand_np = CandidateSets._candidates(candidates)
        if cand_np.max() >= N:
            raise ValueError("RankPocket: a candidate id is outside the table")
        if valid.min() < 0 or valid.max() >= N:
            raise ValueError("RankPocket: a validation triple holds an id outside the table")
        if (CandidateSets.positions_of(cand_np, valid[:, :2].reshape(-1)) < 0).any():
            raise ValueError("a validation triple's true entity is not in the candidate list")
        self.V, self.K = len(valid), cand_np.size
        self.cand = torch.as_tensor(cand_np.astype(np.int32)).to(dev)
        self.sets = None
        if candidate_sets is not None:
            if not H.split_sweep_ok(d, self.max_norm):
                raise ValueError("RankPocket: candidate sets need the masked sweep: embedding_dim % 8 == 0 in 56 ... 288, "
                                 "max_norm <= 8")
            tail, head = candidate_sets["tail"], candidate_sets["head"]
            for cs in (tail, head):
                cs._check(self.cand, "RankPocket")
            if tail.n_sets != head.n_sets:
                raise ValueError("RankPocket: the tail and head candidate sets must hold the same number of sets")
            if valid[:, 2].max() >= tail.n_sets:
                raise ValueError("RankPocket: a validation relation has no candidate set")
            self.sets = (tail, head)
        q = torch.as_tensor(valid).to(dev)
        self.hr = torch.cat([q[:, [0, 2]], q[:, [1, 2]]], 0).to(torch.int32).contiguous()
        self.true_id = torch.cat([q[:, 1], q[:, 0]]).to(torch.int32).contiguous()
        self.row_set = torch.cat([q[:, 2], q[:, 2]]).to(torch.int32).contiguous() if self.sets else None
        self.known = (None, None, None, None)
        if known_triples is not None and len(known_triples):
            pos_of = torch.full((N,), -1, dtype=torch.int64, device=dev)
            pos_of[self.cand.to(torch.int64)] = torch.arange(self.K, device=dev)
            cells = []
            for side, col in (("tail", 0), ("head", 1)):
                index = known_triples[side] if isinstance(known_triples, dict) else KnownIndex(known_triples, N, side, dev)
                cells += list(index.cells(q[:, col], q[:, 2], pos_of, self.K))
            self.known = tuple(cells)
        lib = H._lib.load()
        nbytes = int(lib.ge_rank_planes_bytes(N, d, self.K)) if H.split_sweep_ok(d, self.max_norm) else 0
        self.planes = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        self._ws = torch.empty(max(int(lib.ge_rank_tick_workspace_bytes(self.V)), 256), dtype=torch.uint8, device=dev)
        self.hist = torch.zeros(int(capacity), 8, dtype=torch.float32, device=dev)
        self.best = torch.zeros((), dtype=torch.float32, device=dev)
        self.accumulator = None
        if accumulator is not None:
            H._need_cuda(accumulator, "accumulator")
            if accumulator.shape != emb.shape or accumulator.dtype != torch.float32 or not accumulator.is_contiguous():
                raise ValueError("RankPocket: accumulator must be a contiguous float32 tensor of the table's shape")
            self.accumulator = accumulator
        self.pocket = torch.empty_like(emb) if keep_table else None
        self.pocket_accumulator = torch.empty_like(accumulator) if keep_table and accumulator is not None else None
        self._steps = []        # global step of each tick since the last read()

    def tick(self, global_step: int) -> None:
        if len(self._steps) >= self.hist.shape[0]:
            raise RuntimeError("RankPocket: read() the pending ticks first (capacity %d)" % self.hist.shape[0])
        ptr = lambda t: None if t is None else t.data_ptr()
        sets = (ptr(self.row_set), self.sets[0].mask.data_ptr(), self.sets[1].mask.data_ptr(), self.sets[0].n_sets) \
            if self.sets else (None, None, None, 0)
        emb = self.emb
        H._lib.call("ge_rank_validation_tick", emb.data_ptr(), emb.shape[0], emb.shape[1], self.hr.data_ptr(),
                    self.true_id.data_ptr(), self.V, self.cand.data_ptr(), self.K, self.max_norm, self.model,
                    *[ptr(t) for t in self.known], ptr(self.planes), *sets, ptr(self.accumulator),
                    self.hist.data_ptr() + 32 * len(self._steps), self.best.data_ptr(), ptr(self.pocket),
                    ptr(self.pocket_accumulator), self._ws.data_ptr(), self._ws.numel(), H._stream())
        self._steps.append(int(global_step))

    def read(self):
        """[(global_step, metrics)] of the ticks since the last read, in order (synchronises): the keys of mrr_and_hits
        plus `counted`, the number of rows that had a rank."""
        n = len(self._steps)
        if n == 0:
            return []
        rows = self.hist[:n].cpu().tolist()
        out = []
        for step, row in zip(self._steps, rows):
            m = dict(zip(self.KEYS, row))
            m["counted"] = int(m["counted"])
            out.append((step, m))
        self._steps = []
        return out


# ------------------------------------------------------------------ top-k prediction
def _known_cells_rc(off: torch.Tensor, rc: torch.Tensor, n_cand: int):
    """(rows, columns) int64 of the per-tile known-cell lists of KnownIndex.cells."""
    dev = off.device
    n_ct = (n_cand + 127) // 128
    tiles = torch.repeat_interleave(torch.arange(off.numel() - 1, device=dev), (off[1:] - off[:-1]).to(torch.int64))
    rcv = rc[:tiles.numel()].to(torch.int64)
    return (tiles // n_ct) * 128 + rcv // 128, (tiles % n_ct) * 128 + rcv % 128


def _topk_of_losses(losses: torch.Tensor, cand64: torch.Tensor, k: int, known=None):
    """The first k pops of the reference's heap from a [b, K] loss matrix: a stable sort by loss of the candidates in id
    order, i.e. ascending (loss, id).  Known cells are skipped; padding -1 / +inf, rows with NaN losses -1 / NaN."""
    L = losses.clone()
    if known is not None and known[0].numel():
        L[known[0], known[1]] = float("inf")
    by_id = torch.argsort(cand64)
    vals, order = torch.sort(L[:, by_id], dim=1, stable=True)
    kk = min(k, L.shape[1])
    vals, ids = vals[:, :kk].contiguous(), cand64[by_id][order[:, :kk]]
    if kk < k:
        vals = torch.cat([vals, torch.full((L.shape[0], k - kk), float("inf"), device=L.device)], 1)
        ids = torch.cat([ids, torch.full((L.shape[0], k - kk), -1, dtype=torch.int64, device=L.device)], 1)
    ids[vals == float("inf")] = -1
    bad = torch.isnan(L).any(1)
    vals[bad] = float("nan")
    ids[bad] = -1
    return ids, vals


@torch.no_grad()
def predict_links(embeddings: torch.Tensor, queries, candidates, k: int, known_triples=None, side: str = "tail",
                  model: str = "complex", batch: int = None, fused: bool = None, planes=None, max_norm: float = 1.0,
                  candidate_sets=None, row_sets=None):
    """Top-k link prediction: for every query (fixed entity, relation) the first k pops of the reference's heap
    (holE.py:427-469) over `candidates` -- ascending loss E = sigmoid(score), ties by entity id.  side="tail" predicts
    (fixed, ?, relation), "head" (?, fixed, relation).  known_triples (an [n,3] array or a KnownIndex for this side):
    known-true candidates are skipped, as the reference's filtered ranks skip them.
    Returns (ids int64 [n,k], losses float32 [n,k]) numpy arrays, rows in the queries' order; a row with fewer eligible
    candidates is padded with -1 / +inf.
    fused (default: whenever embedding_dim has the split-precision sweep, % 8 == 0 in 56 ... 288): the list is selected
    inside the candidate sweep (hole.topk_candidates) and no [n, K] matrix exists; k > hole.topk_max_k() takes the same
    sweep's losses (rank_candidates' scores) in chunks of 1024 rows, sorted on the device.  fused=False: the losses of
    score_candidates, sorted the same way in chunks of 1024 rows.
    model: "complex", "hole" (a real-valued HolE table: a copy is transformed once) or "hole_spectral"; HolE needs the
    fused sweep.  planes: hole.RankPlanes of (embeddings, candidates) shared between calls.  The copy model="hole" makes
    is new on every call, so planes cannot be built for it: with HolE and planes, transform the table once
    (hole.hole_to_spectral), build the planes with model="hole_spectral" and pass that table and model here.
    candidate_sets (CandidateSets for `candidates` and this side) / row_sets ([n], default each query's relation id; -1:
    unrestricted): only candidates admissible in the row's set are returned -- inside the masked sweep, or by masking the
    stored losses on the two fallback paths."""
    assert side in ("tail", "head")
    if candidate_sets is None and row_sets is not None:
        raise ValueError("row_sets need candidate_sets")
    if model not in ("complex", "hole", "hole_spectral"):
        raise ValueError(f"unknown model {model!r}")
    k = int(k)
    if k < 1:
        raise ValueError("k must be >= 1")
    dev = embeddings.device
    N, d = embeddings.shape
    can_fuse = H.split_sweep_ok(d, max_norm)
    if fused is None:
        fused = can_fuse
    if fused and not can_fuse:
        raise ValueError("the fused top-k needs embedding_dim % 8 == 0 in 56 ... 288 and max_norm <= 8")
    if model != "complex":
        if not fused:
            raise ValueError("HolE prediction needs the fused sweep: embedding_dim % 8 == 0 in 56 ... 288")
        if model == "hole":
            if planes is not None:
                raise ValueError("planes with model='hole': build them for a hole_to_spectral table and pass that "
                                 "table with model='hole_spectral'")
            embeddings = H.hole_to_spectral(embeddings.detach().clone())
        model = "hole_spectral"
    q = np.asarray(queries, dtype=np.int64).reshape(-1, 2)
    cand_np = np.asarray(candidates, dtype=np.int64).reshape(-1)
    if cand_np.size == 0:
        raise ValueError("candidates must not be empty")
    if cand_np.min() < 0 or cand_np.max() >= N or np.unique(cand_np).size != cand_np.size:
        raise ValueError("candidates must be distinct table rows")
    if q.size and (q.min() < 0 or q.max() >= N):
        raise ValueError("a query id is outside the table")
    cand = torch.as_tensor(cand_np.astype(np.int32)).to(dev)
    cand64 = cand.to(torch.int64)
    K = cand.numel()
    pos_of = torch.full((N,), -1, dtype=torch.int64, device=dev)
    pos_of[cand64] = torch.arange(K, device=dev)
    index = None
    if known_triples is not None:
        index = known_triples if isinstance(known_triples, KnownIndex) else KnownIndex(known_triples, N, side, dev)
    if fused and planes is None:
        planes = H.RankPlanes(embeddings, cand, max_norm=max_norm, model=model)
    if planes is not None:
        if planes.cand.numel() != K or not bool(torch.equal(planes.cand.to(dev), cand)):
            raise ValueError("`planes` were built for another candidate list")
        cand = planes.cand
    in_kernel = fused and k <= H.topk_max_k()
    if candidate_sets is not None:
        candidate_sets._check(cand, "predict_links")
        if row_sets is not None and len(row_sets) != len(q):
            raise ValueError("row_sets must have one entry per query")
    if batch is None:
        batch = 1 << 17 if in_kernel else 1024
    if not in_kernel:
        batch = min(batch, 1024)                 # a [batch, K] loss matrix exists per chunk
    ids_all, loss_all = [], []
    for s0 in range(0, len(q), batch):
        chunk = torch.as_tensor(q[s0:s0 + batch]).to(dev)
        fixed, rel = chunk[:, 0], chunk[:, 1]
        hr = torch.stack([fixed, rel], 1).to(torch.int32)
        off = rc = None
        if index is not None:
            off, rc = index.cells(fixed, rel, pos_of, K)
        rs = None
        if candidate_sets is not None:
            rs = candidate_sets.row_sets(None if row_sets is None else row_sets[s0:s0 + batch], rel, "predict_links")
        if in_kernel:
            ids, losses = H.topk_candidates(embeddings, hr, cand, k, known_off=off, known_rc=rc, cand_is_head=(side == "head"),
                                            max_norm=max_norm, model=model, planes=planes, candidate_sets=candidate_sets,
                                            row_sets=rs)
            ids = ids.to(torch.int64)
        else:
            if fused:                            # the fused sweep's own losses (MODE 1 of the rank kernel)
                tid = cand[:1].expand(hr.shape[0]).contiguous()
                losses = H.rank_candidates(embeddings, hr, tid, cand, cand_is_head=(side == "head"), max_norm=max_norm,
                                           return_scores=True, model=model, planes=planes)[-1]
            else:
                losses = H.score_candidates(embeddings, hr, cand, cand_is_head=(side == "head"), max_norm=max_norm)
            if rs is not None:                   # (every query id is in range: no NaN row to keep apart)
                losses = torch.where(candidate_sets.admissible(rs), losses, torch.full_like(losses, float("inf")))
            ids, losses = _topk_of_losses(losses, cand64, k, _known_cells_rc(off, rc, K) if off is not None else None)
        ids_all.append(ids.cpu().numpy())
        loss_all.append(losses.cpu().numpy())
    if not ids_all:
        return np.zeros((0, k), dtype=np.int64), np.zeros((0, k), dtype=np.float32)
    return np.concatenate(ids_all).astype(np.int64), np.concatenate(loss_all).astype(np.float32)


def inference_lines(head: int, relation: int, pop_ids, pop_losses, in_sample_set) -> list:
    """The lines of the reference's inference_results.tsv (holE.py:451-453) for one query's pops, in pop order:
    'loss, head, tail, relation, in_sample' with in_sample = the tail completes a known (train / valid) triple."""
    return ['{:.6f}\t{}\t{}\t{}\t{}\n'.format(float(l), int(head), int(t), int(relation), int(t) in in_sample_set)
            for t, l in zip(pop_ids, pop_losses)]


@torch.no_grad()
def predict_inference_results(embeddings: torch.Tensor, data, predict_k: int, infer_threshold: float, path: str,
                              model: str = "complex", log=print, candidate_sets=None) -> dict:
    """The prediction output of the reference's --infer (holE.py:427-469) for the distinct (head, relation) pairs of the
    test triples, in order of first appearance, over every entity row: for each query whose lowest loss is below
    infer_threshold (is_confident, holE.py:436-438), every pop up to and including the predict_k-th filtered pop --
    known-true (train / valid) pops interleaved with in_sample = True -- as the reference's lines, written to `path`
    (truncated first; the reference appends to ./inference_results.tsv).
    Exact: the filtered top-k gives the k-th filtered pop; its raw position m (rank_candidates_vs_loss, or the stored
    scores off the fused range) gives the raw top-m that holds every line.
    candidate_sets (CandidateSets over the entity rows, tail side; set = the query's relation): every pop, the gate's
    lowest loss included, is taken among the tails admissible for the relation; a relation with an empty set writes
    nothing."""
    R, N = data.relation_count, data.entity_count
    cand = np.arange(R, N, dtype=np.int64)
    test = np.asarray(data.test_array, dtype=np.int64)
    hr_all = test[:, [0, 2]]
    _, first = np.unique(hr_all, axis=0, return_index=True)
    queries = hr_all[np.sort(first)]
    parts = [a for a in (data.triples, data.validation_triples) if a is not None]
    known = np.concatenate(parts, 0) if parts else None
    if model == "hole":
        embeddings, model = H.hole_to_spectral(embeddings.detach().clone()), "hole_spectral"
    dev = embeddings.device
    fused = H.split_sweep_ok(embeddings.shape[1], 1.0)
    planes = H.RankPlanes(embeddings, torch.as_tensor(cand).to(dev), model=model) if fused else None
    kw = dict(model=model, fused=fused, planes=planes, candidate_sets=candidate_sets)
    cs = candidate_sets
    K = int(predict_k)
    fid, floss = predict_links(embeddings, queries, cand, K, known_triples=KnownIndex(known, N, "tail", dev), **kw)
    # m = raw position of the K-th filtered pop (every pop when fewer than K candidates are eligible)
    m = np.full(len(queries), len(cand), dtype=np.int64) if cs is None else cs.counts[queries[:, 1]].astype(np.int64)
    rows = np.nonzero(fid[:, K - 1] >= 0)[0]
    if rows.size:
        hr = torch.as_tensor(queries[rows]).to(dev).to(torch.int32)
        ref_id = torch.as_tensor(fid[rows, K - 1]).to(dev)
        ref_loss = torch.as_tensor(floss[rows, K - 1]).to(dev)
        if fused and cs is not None:
            # (the K-th filtered pop is a candidate: ranking it as the true entity of the masked sweep counts the admissible
            # pops before it, its own loss recomputed by the same sweep)
            nb, _ = H.rank_candidates(embeddings, hr, ref_id, planes.cand, model=model, planes=planes, candidate_sets=cs)
            m[rows] = nb.cpu().numpy().astype(np.int64) + 1
        elif fused:
            nb, _ = H.rank_candidates_vs_loss(embeddings, hr, ref_id, ref_loss, planes.cand, model=model, planes=planes)
            m[rows] = nb.cpu().numpy().astype(np.int64) + 1
        else:
            c64 = torch.as_tensor(cand).to(dev)
            for s0 in range(0, rows.size, 1024):
                sc = H.score_candidates(embeddings, hr[s0:s0 + 1024], c64)
                rl, ri = ref_loss[s0:s0 + 1024, None], ref_id[s0:s0 + 1024, None]
                before = (sc < rl) | ((sc == rl) & (c64[None, :] < ri))
                if cs is not None:
                    before &= cs.admissible(hr[s0:s0 + 1024, 1].to(torch.int64))
                m[rows[s0:s0 + 1024]] = (before.sum(1) + 1).cpu().numpy()
    # the raw pops: rows sorted by m and cut into chunks, each predicted with its own longest m -- up to 16384 rows
    # while that fits the fused kernel, 1024 rows (the fallback's [rows, K] losses) beyond it
    raw_id = [None] * len(queries)
    raw_loss = [None] * len(queries)
    order = np.argsort(m, kind="stable")
    for i in order[m[order] == 0]:                           # (an empty set: no pop at all)
        raw_id[i], raw_loss[i] = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32)
    order = order[m[order] > 0]
    kmax = H.topk_max_k()
    s0 = 0
    while s0 < order.size:
        rows_c = 1 << 14 if m[order[s0]] <= kmax else 1024
        chunk = order[s0:s0 + rows_c]
        if m[chunk[-1]] > kmax and m[chunk[0]] <= kmax:      # (the fused chunk ends where m passes kmax)
            chunk = chunk[m[chunk] <= kmax]
        ids, ls = predict_links(embeddings, queries[chunk], cand, int(m[chunk[-1]]), **kw)
        for j, i in enumerate(chunk):
            raw_id[i], raw_loss[i] = ids[j, :m[i]], ls[j, :m[i]]
        s0 += chunk.size
    n_conf = n_lines = 0
    with open(path, "w") as out:
        for i, (h, r) in enumerate(queries):
            if len(raw_loss[i]) == 0 or not raw_loss[i][0] < infer_threshold:       # is_confident: the lowest loss of the sweep (holE.py:438)
                continue
            n_conf += 1
            lines = inference_lines(h, r, raw_id[i], raw_loss[i], data.true_triples[int(h)][int(r)])
            out.writelines(lines)
            n_lines += len(lines)
    log(f"top-{K} prediction: {len(queries)} queries, {n_conf} confident (lowest loss < {infer_threshold}), "
        f"{n_lines} lines written to {path}")
    return {"queries": int(len(queries)), "confident": int(n_conf), "lines": int(n_lines)}


# ------------------------------------------------------------------ translation models (TransE / H / D, TransR)
def _translation_test(model, test) -> np.ndarray:
    """The test rows as int64 [n,3] (h, t, r), ids checked against the model's tables on the host."""
    t = np.asarray(test.cpu().numpy() if isinstance(test, torch.Tensor) else test)
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("test triples must have shape [n, 3] (head, tail, relation)")
    if t.size and not np.issubdtype(t.dtype, np.integer):
        raise ValueError("test triples must be integer ids")
    t = t.astype(np.int64)
    if ids_outside(t, model.n_ent, model.n_rel):
        raise ValueError(f"a test triple holds an id outside [0, {model.n_ent}) entities / [0, {model.n_rel}) relations")
    return t


def _translation_sweep_setup(model, rel, known, side: str):
    """What a translation-model sweep over every entity needs, for translation_ranks and predict_translation: the
    rows' order (a stable sort by relation: rows of one relation share the sweep's projection work), the KnownIndex of
    `known` (an [n,3] array, None, or a KnownIndex with n_rows = max(n_ent, n_rel)) and pos_of (every entity is a
    candidate at its own id)."""
    if side not in ("tail", "head"):
        raise ValueError(f"side must be 'tail' or 'head', got {side!r}")
    dev = model.tables["ent"].device
    E = model.n_ent
    n_rows = max(E, model.n_rel)
    index = known if isinstance(known, KnownIndex) else KnownIndex(known, n_rows, side, dev)
    if index.n_rows != n_rows:
        raise ValueError(f"the KnownIndex has n_rows={index.n_rows}, expected max(n_ent, n_rel) = {n_rows}")
    order = np.argsort(np.asarray(rel), kind="stable")
    pos_of = torch.arange(n_rows, dtype=torch.int64, device=dev)
    pos_of[E:] = -1
    return order, index, pos_of


def _translation_sets(model, candidate_sets, row_sets, n_rows: int, who: str):
    """The host checks of a translation-model sweep's candidate sets, before any device work: built for arange(n_ent),
    one row set per row, every index in [-1, n_sets).  Returns row_sets as an int64 numpy array, or None (the default:
    each row's relation id)."""
    if not isinstance(candidate_sets, CandidateSets):
        raise ValueError(f"{who}: candidate_sets must be a CandidateSets")
    if candidate_sets.cand.numel() != model.n_ent:
        raise ValueError(f"{who}: candidate_sets were built for another candidate list (need arange(n_ent))")
    if row_sets is None:
        if candidate_sets.n_sets < model.n_rel:
            raise ValueError(f"{who}: the default row set is the relation id, but candidate_sets holds "
                             f"{candidate_sets.n_sets} sets for {model.n_rel} relations")
        return None
    rs = np.asarray(row_sets.cpu().numpy() if isinstance(row_sets, torch.Tensor) else row_sets)
    if rs.ndim != 1 or rs.shape[0] != n_rows:
        raise ValueError(f"{who}: row_sets must have one entry per row")
    if rs.size and not np.issubdtype(rs.dtype, np.integer):
        raise ValueError(f"{who}: row_sets must be integer set indices")
    rs = rs.astype(np.int64)
    if rs.size and (rs.min() < -1 or rs.max() >= candidate_sets.n_sets):
        raise ValueError(f"{who}: a row's set index is outside [-1, {candidate_sets.n_sets})")
    return rs


@torch.no_grad()
def translation_ranks(model, test, known=None, side: str = "tail", batch: int = None, candidate_sets=None,
                      row_sets=None, return_admissible: bool = False):
    """Raw and filtered rank of every test triple's true entity among ALL entities for a TransX or TransR model
    (int64 arrays, in test order).  side="tail": every entity replaces the tail; "head": the head.  Order: ascending
    by (D, entity id), as link_prediction_ranks.  known: an [n,3] array of triples to filter, or a KnownIndex built
    for this side with n_rows = max(n_ent, n_rel) (None: filtered == raw).  The rows are grouped by relation for the
    sweep (a stable sort on the host) and the ranks returned in the caller's order; a row's ranks do not depend on
    the grouping.  batch: rows per native call (default 131072).
    candidate_sets (CandidateSets built for arange(n_ent) and this side) / row_sets ([n], default each row's relation
    id; -1: unrestricted): every rank counts only the entities admissible in the row's set, inside the masked sweep
    (rank_counts with row_set / mask), which computes a distance for those entities alone.  The true entity need not be
    admissible; return_admissible=True adds the bool array "true entity admissible in its set"."""
    if side not in ("tail", "head"):
        raise ValueError(f"side must be 'tail' or 'head', got {side!r}")
    if candidate_sets is None and (row_sets is not None or return_admissible):
        raise ValueError("row_sets / return_admissible need candidate_sets")
    test = _translation_test(model, test)
    rs_all = None
    if candidate_sets is not None:
        rs_all = _translation_sets(model, candidate_sets, row_sets, len(test), "translation_ranks")
        if rs_all is None:
            rs_all = test[:, 2]
    order, index, pos_of = _translation_sweep_setup(model, test[:, 2], known, side)
    E, dev = model.n_ent, model.tables["ent"].device
    if candidate_sets is not None:
        candidate_sets._check(torch.arange(E, dtype=torch.int32, device=dev), "translation_ranks")
    if batch is None:
        batch = 1 << 17
    if batch <= 0:
        raise ValueError("batch must be positive")
    raw = np.empty(len(test), dtype=np.int64)
    fil = np.empty(len(test), dtype=np.int64)
    adm = np.empty(len(test), dtype=bool)
    if len(test) == 0:
        return (raw, fil, adm) if return_admissible else (raw, fil)
    fixed_col, true_col = (0, 1) if side == "tail" else (1, 0)
    for s in range(0, len(test), batch):
        idx = order[s:s + batch]
        chunk = torch.as_tensor(test[idx]).to(dev)
        off, rc = index.cells(chunk[:, fixed_col], chunk[:, 2], pos_of, E)
        sets = {}
        if candidate_sets is not None:
            rs = torch.as_tensor(rs_all[idx]).to(dev)
            sets = {"row_set": rs.to(torch.int32).contiguous(), "mask": candidate_sets.mask}
            adm[idx] = candidate_sets.admissible(rs, chunk[:, true_col]).cpu().numpy()
        nb, nk, _ = model.rank_counts(chunk, cand_is_head=(side == "head"), known_off=off, known_rc=rc, **sets)
        nb, nk = nb.cpu().numpy().astype(np.int64), nk.cpu().numpy().astype(np.int64)
        if (nb < 0).any() or (nk < 0).any():
            raise ValueError("a test triple holds an id outside the model's tables")
        raw[idx] = nb + 1
        fil[idx] = nb + 1 - nk
    return (raw, fil, adm) if return_admissible else (raw, fil)


def evaluate_translation(model, test, known=None, both_sides: bool = True, batch: int = None, verbose: bool = False,
                         relations: bool = False, candidate_sets=None) -> dict:
    """Filtered link prediction of a TransX / TransR model over all entities: mrr_and_hits of the tail ranks (and the
    head ranks with both_sides) plus `sweeps`, and per side `tail` / `head` dicts of the same numbers.  known: the
    triples to filter (the Bordes et al. setting filters train + valid + test).  relations: add a `relation` dict, the
    same numbers for the relation ranks (translation_relation_ranks); the other entries do not change.
    candidate_sets: {"tail": CandidateSets, "head": CandidateSets} built for arange(n_ent) (row set = relation id) adds a
    `constrained` dict -- mrr_and_hits of the type-constrained ranks over the evaluated sides, `admissible_true` (the
    share of rows whose true entity is in its set) and `mean_set_size` (over the rows); the other entries do not
    change."""
    n_rows = max(model.n_ent, model.n_rel)
    dev = model.tables["ent"].device
    sides = ("tail", "head") if both_sides else ("tail",)
    if candidate_sets is not None and (not isinstance(candidate_sets, dict) or any(s not in candidate_sets for s in sides)):
        raise ValueError("candidate_sets must be a dict with a CandidateSets per evaluated side ('tail', 'head')")
    per, raw_all, fil_all = {}, [], []
    c_raw, c_fil, c_adm, c_size = [], [], [], []
    for side in sides:
        idx = KnownIndex(None if known is None else np.asarray(known, dtype=np.int64), n_rows, side, dev)
        raw, fil = translation_ranks(model, test, idx, side=side, batch=batch)
        per[side] = mrr_and_hits(raw, fil)
        raw_all.append(raw); fil_all.append(fil)
        if candidate_sets is not None:
            r, f, a = translation_ranks(model, test, idx, side=side, batch=batch, candidate_sets=candidate_sets[side],
                                        return_admissible=True)
            c_raw.append(r); c_fil.append(f); c_adm.append(a)
            c_size.append(candidate_sets[side].counts[_translation_test(model, test)[:, 2]])
    out = mrr_and_hits(np.concatenate(raw_all), np.concatenate(fil_all))
    out["sweeps"] = int(sum(r.size for r in raw_all))
    if relations:
        per["relation"] = mrr_and_hits(*translation_relation_ranks(model, test, known, batch=batch))
    out.update(per)
    if candidate_sets is not None:
        con = mrr_and_hits(np.concatenate(c_raw), np.concatenate(c_fil))
        adm, size = np.concatenate(c_adm), np.concatenate(c_size)
        con["admissible_true"] = float(adm.mean()) if adm.size else 0.0
        con["mean_set_size"] = float(size.mean()) if size.size else 0.0
        out["constrained"] = con
    if verbose:
        for name, m in list(per.items()) + [("both", out)]:
            print(f"{name}: raw MRR {m['raw_mrr']:.6f} (mean rank {m['mean_raw_pos']:.1f}); filtered MRR "
                  f"{m['filtered_mrr']:.6f} (mean rank {m['mean_filtered_pos']:.1f}); hits@1/3/10 "
                  f"{m['hits1']:.2f} / {m['hits3']:.2f} / {m['hits10']:.2f} %")
        if candidate_sets is not None:
            print(constrained_line(out["constrained"]))
    return out


def constrained_line(m: dict) -> str:
    """The `constrained:` line of evaluate_translation's constrained block."""
    return (f"constrained: raw MRR {m['raw_mrr']:.6f}; filtered MRR {m['filtered_mrr']:.6f} (mean rank "
            f"{m['mean_filtered_pos']:.1f}); hits@1/3/10 {m['hits1']:.2f} / {m['hits3']:.2f} / {m['hits10']:.2f} %; true "
            f"entity admissible {100.0 * m['admissible_true']:.2f} %; mean set size {m['mean_set_size']:.1f}")


class TranslationPocket:
    """RankPocket for a TransX, TransR or RotatE model: validation ticks on the filtered MRR of translation_ranks over
    both sides, without a host decision per tick.  tick() enqueues the model's rank sweeps of the validation rows' tails
    and heads into fixed buffers, ge_rank_metrics over the 2V rows into `hist`, `best` (a device scalar that starts at
    0; a tie keeps the first best, a NaN never improves) and `improved`, and one ge_copy_if on that flag: `pocket`
    {name: tensor} <- the model's _pocket_tensors() (the tables, adagrad_<table> per accumulator, TransR's m and v).
    The model's host scalars of that state (TransR.t) are recorded per tick; restore() puts the best tick's tensors and
    scalars back.  The constructor does all that does not depend on the tables; tick() neither synchronises nor
    allocates; read() synchronises once for all pending ticks.
    known: the triples to filter ([n,3], None: filtered == raw) or {"tail": KnownIndex, "head": KnownIndex} built with
    n_rows = max(n_ent, n_rel).  rows=n: only the first n rows of np.random.default_rng(seed).permutation(len(valid))
    are ranked (`row_index`, in the order they are swept).  candidate_sets = {"tail": CandidateSets, "head":
    CandidateSets} for arange(n_ent): every row against its relation's set, the `constrained` ranks of
    evaluate_translation (not RotatE).  keep_state=False: no pocket and no copy.  batch: rows per native call.
    ValueError on the host: an empty validation set, ids outside the tables, rows < 1, a KnownIndex of the wrong n_rows."""

    KEYS = RankPocket.KEYS

    def __init__(self, model, validation_triples, known=None, *, rows: int = None, seed: int = 0, candidate_sets=None,
                 keep_state: bool = True, capacity: int = 4096, batch: int = None):
        valid = _translation_test(model, validation_triples)
        if len(valid) == 0:
            raise ValueError("TranslationPocket: the validation set is empty")
        index = np.arange(len(valid))
        if rows is not None:
            if rows < 1:
                raise ValueError(f"TranslationPocket: rows must be >= 1, got {rows}")
            index = np.random.default_rng(seed).permutation(len(valid))[:rows]
        if batch is None:
            batch = 1 << 17
        if batch <= 0 or capacity < 1:
            raise ValueError("TranslationPocket: batch and capacity must be positive")
        if 2 * len(index) > 1 << 24:
            raise ValueError("TranslationPocket: more than 2^23 validation rows (ge_rank_metrics counts 2^24); use rows=")
        self.sets = None
        if candidate_sets is not None:
            model._check_candidate_sets()
            if not isinstance(candidate_sets, dict) or any(s not in candidate_sets for s in ("tail", "head")):
                raise ValueError("candidate_sets must be a dict with a CandidateSets per side ('tail', 'head')")
            for side in ("tail", "head"):
                _translation_sets(model, candidate_sets[side], None, len(index), "TranslationPocket")
            self.sets = candidate_sets
        self.model, dev, E = model, model.tables["ent"].device, model.n_ent
        self.row_index = index[np.argsort(valid[index, 2], kind="stable")]      # grouped by relation, as translation_ranks
        valid = valid[self.row_index]
        self.V = V = len(valid)
        self.triples = torch.as_tensor(valid).to(dev).to(torch.int32).contiguous()
        self.row_set = self.triples[:, 2].contiguous() if self.sets else None
        if self.sets:
            for side in ("tail", "head"):
                self.sets[side]._check(torch.arange(E, dtype=torch.int32, device=dev), "TranslationPocket")
        self._chunks = [(s, min(s + int(batch), V)) for s in range(0, V, int(batch))]
        q = self.triples.to(torch.int64)
        self._cells = {}
        for side, col in (("tail", 0), ("head", 1)):
            _, ki, pos_of = _translation_sweep_setup(model, valid[:, 2], known[side] if isinstance(known, dict) else known, side)
            self._cells[side] = [ki.cells(q[a:b, col], q[a:b, 2], pos_of, E) for a, b in self._chunks]
        self.n_before = torch.empty(2 * V, dtype=torch.int32, device=dev)
        self.n_known_before = torch.empty(2 * V, dtype=torch.int32, device=dev)
        self.true_dist = torch.empty(2 * V, dtype=torch.float32, device=dev)
        nbytes = model._ws_bytes("rank", min(int(batch), V))
        if nbytes == 0:
            raise RuntimeError(f"{model.PREFIX}_rank_workspace_bytes failed")
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.hist = torch.zeros(int(capacity), 8, dtype=torch.float32, device=dev)
        self.improved = torch.zeros(int(capacity), dtype=torch.int32, device=dev)
        self.best = torch.zeros((), dtype=torch.float32, device=dev)
        self._shapes = {k: tuple(t.shape) for k, t in model._pocket_tensors().items()}
        self.pocket = {k: torch.empty_like(t) for k, t in model._pocket_tensors().items()} if keep_state else None
        self._pending = []      # (global step, host scalars) of each tick since the last read()
        self._best = None       # ... of the best tick read so far

    def tick(self, global_step: int) -> None:
        i = len(self._pending)
        if i >= self.hist.shape[0]:
            raise RuntimeError("TranslationPocket: read() the pending ticks first (capacity %d)" % self.hist.shape[0])
        m, V = self.model, self.V
        state = m._pocket_tensors()
        if {k: tuple(t.shape) for k, t in state.items()} != self._shapes:
            raise RuntimeError("TranslationPocket: the model's state tensors are no longer the constructor's (%s, now %s): "
                               "build the pocket after enable_adagrad() / trainer()" % (sorted(self._shapes), sorted(state)))
        for k, side in enumerate(("tail", "head")):
            for (a, b), (off, rc) in zip(self._chunks, self._cells[side]):
                sets = {"row_set": self.row_set[a:b], "mask": self.sets[side].mask} if self.sets else {}
                lo, hi = k * V + a, k * V + b
                m.rank_counts(self.triples[a:b], cand_is_head=(side == "head"), known_off=off, known_rc=rc, **sets,
                              out=(self.n_before[lo:hi], self.n_known_before[lo:hi], self.true_dist[lo:hi]), workspace=self._ws)
        flag = self.improved.data_ptr() + 4 * i
        H._lib.call("ge_rank_metrics", self.n_before.data_ptr(), self.n_known_before.data_ptr(), self.true_dist.data_ptr(),
                    2 * V, self.hist.data_ptr() + 32 * i, self.best.data_ptr(), flag, H._stream())
        if self.pocket is not None:
            names = list(state)
            H._lib.call("ge_copy_if", flag, *H._lib.copy_if_args([state[n].data_ptr() for n in names],
                                                                 [self.pocket[n].data_ptr() for n in names],
                                                                 [state[n].numel() for n in names]), H._stream())
        self._pending.append((int(global_step), m._pocket_scalars()))

    def read(self):
        """[(global_step, metrics)] of the ticks since the last read, in order (synchronises): RankPocket.KEYS plus
        `improved`, whether the tick's filtered MRR became `best` (and its state the pocket)."""
        n = len(self._pending)
        if n == 0:
            return []
        rows, flags = self.hist[:n].cpu().tolist(), self.improved[:n].cpu().tolist()
        out = []
        for (step, scalars), row, flag in zip(self._pending, rows, flags):
            mt = dict(zip(self.KEYS, row))
            mt["counted"] = int(mt["counted"])
            mt["improved"] = bool(flag)
            if flag:
                self._best = (step, scalars)
            out.append((step, mt))
        self._pending = []
        return out

    @torch.no_grad()
    def restore(self):
        """pocket -> model: the best tick's tensors and host scalars (reads the pending ticks first).  Returns that
        tick's global_step; None, and nothing is written, if no tick improved on 0 or keep_state is False."""
        self.read()
        if self._best is None or self.pocket is None:
            return None
        step, scalars = self._best
        state = self.model._pocket_tensors()
        if {k: tuple(t.shape) for k, t in state.items()} != self._shapes:
            raise RuntimeError("TranslationPocket: the model's state tensors are no longer the constructor's")
        for name, t in state.items():
            t.copy_(self.pocket[name])
        for name, value in scalars.items():
            setattr(self.model, name, value)
        return step


def _translation_queries(model, queries) -> np.ndarray:
    """The query rows as int64 [n,2] (fixed entity, relation), ids checked against the model's tables on the host."""
    q = np.asarray(queries.cpu().numpy() if isinstance(queries, torch.Tensor) else queries)
    if q.size == 0:
        return np.zeros((0, 2), dtype=np.int64)
    if q.ndim != 2 or q.shape[1] != 2:
        raise ValueError("queries must have shape [n, 2] (fixed entity, relation)")
    if not np.issubdtype(q.dtype, np.integer):
        raise ValueError("queries must be integer ids")
    q = q.astype(np.int64)
    if q[:, 0].min() < 0 or q[:, 0].max() >= model.n_ent or q[:, 1].min() < 0 or q[:, 1].max() >= model.n_rel:
        raise ValueError(f"a query holds an id outside [0, {model.n_ent}) entities / [0, {model.n_rel}) relations")
    return q


@torch.no_grad()
def predict_translation(model, queries, k: int, known=None, side: str = "tail", batch: int = None, fused: bool = None,
                        candidate_sets=None, row_sets=None):
    """Top-k link prediction of a TransX / TransR model over ALL entities: for every query (fixed f, relation r) the
    first k entities c in ascending (D, c), D = D(f, c, r) (side="tail") or D(c, f, r) ("head") -- the rank sweep's own
    distance, so the filtered rank (translation_ranks, same `known`) of the j-th candidate is j + 1.  known: an [m,3]
    array or a KnownIndex with n_rows = max(n_ent, n_rel); known-true candidates are skipped.
    Returns (ids int64 [n,k], dist float32 [n,k]) numpy arrays in the queries' order; padding -1 / +inf (+inf distances
    are padding too); a row with a NaN distance at a candidate that is not known is -1 / NaN.
    The rows are grouped by relation for the sweep.  fused (default: k <= transx.topk_max_k()): the list is selected
    inside the sweep (topk_candidates), no [n, n_ent] matrix exists.  k > max_k or fused=False: the rank sweep's stored
    distances (rank_counts(return_scores=True)) in chunks of <= 1024 rows, sorted stably on the device -- the same
    arrays where both routes apply.  batch: rows per native call.
    candidate_sets (CandidateSets built for arange(n_ent) and this side) / row_sets ([n], default each query's relation
    id; -1: unrestricted): only entities admissible in the row's set are returned -- inside the masked sweep
    (topk_candidates with row_set / mask), or on the stored-distance route by treating the inadmissible entities as
    known cells."""
    from .transx import topk_max_k
    k = int(k)
    if k < 1:
        raise ValueError("k must be >= 1")
    if side not in ("tail", "head"):
        raise ValueError(f"side must be 'tail' or 'head', got {side!r}")
    if candidate_sets is None and row_sets is not None:
        raise ValueError("row_sets need candidate_sets")
    q = _translation_queries(model, queries)
    rs_all = None
    if candidate_sets is not None:
        rs_all = _translation_sets(model, candidate_sets, row_sets, len(q), "predict_translation")
        if rs_all is None:
            rs_all = q[:, 1]
    order, index, pos_of = _translation_sweep_setup(model, q[:, 1], known, side)
    E, dev = model.n_ent, model.tables["ent"].device
    if candidate_sets is not None:
        candidate_sets._check(torch.arange(E, dtype=torch.int32, device=dev), "predict_translation")
    in_kernel = fused is not False and k <= topk_max_k()
    if batch is None:
        batch = 1 << 15 if in_kernel else 1024
    if batch <= 0:
        raise ValueError("batch must be positive")
    if not in_kernel:
        batch = min(batch, 1024)                 # a [batch, n_ent] distance matrix exists per chunk
    ids_out = np.empty((len(q), k), dtype=np.int64)
    dist_out = np.empty((len(q), k), dtype=np.float32)
    filtered = index.key.numel() > 0
    head = side == "head"
    for s0 in range(0, len(q), batch):
        idx = order[s0:s0 + batch]
        chunk = torch.as_tensor(q[idx]).to(dev)
        off = rc = None
        if filtered:
            off, rc = index.cells(chunk[:, 0], chunk[:, 1], pos_of, E)
        rs = None if candidate_sets is None else torch.as_tensor(rs_all[idx]).to(dev)
        if in_kernel:
            sets = {} if rs is None else {"row_set": rs.to(torch.int32).contiguous(), "mask": candidate_sets.mask}
            ids, dist = model.topk_candidates(chunk, k, cand_is_head=head, known_off=off, known_rc=rc, **sets)
        else:
            # rows (f, any valid target, r): the target's counts are discarded, the distances are the row's
            zero = torch.zeros_like(chunk[:, 0])
            tri = torch.stack([zero, chunk[:, 0], chunk[:, 1]] if head else [chunk[:, 0], zero, chunk[:, 1]], 1)
            dist_all = model.rank_counts(tri, cand_is_head=head, return_scores=True)[-1]
            cells = _known_cells_rc(off, rc, E) if off is not None else None
            if rs is not None:                   # the inadmissible entities join the known cells
                out_r, out_c = torch.nonzero(~candidate_sets.admissible(rs), as_tuple=True)
                cells = (out_r, out_c) if cells is None else (torch.cat([cells[0], out_r]), torch.cat([cells[1], out_c]))
            ids, dist = _topk_of_losses(dist_all, torch.arange(E, device=dev), k, cells)
        ids_out[idx] = ids.to(torch.int64).cpu().numpy()
        dist_out[idx] = dist.cpu().numpy()
    return ids_out, dist_out


# ------------------------------------------------------------------ relation prediction (h, ?, t)
def _relation_sweep_setup(model, known):
    """The KnownIndex(side="relation") of `known` (an [n,3] array, None, or such an index with n_rows =
    max(n_ent, n_rel)) and pos_of (every relation is a candidate at its own id)."""
    dev = model.tables["ent"].device
    n_rows = max(model.n_ent, model.n_rel)
    index = known if isinstance(known, KnownIndex) else KnownIndex(known, n_rows, "relation", dev)
    if index.n_rows != n_rows:
        raise ValueError(f"the KnownIndex has n_rows={index.n_rows}, expected max(n_ent, n_rel) = {n_rows}")
    pos_of = torch.arange(n_rows, dtype=torch.int64, device=dev)
    pos_of[model.n_rel:] = -1
    return index, pos_of


@torch.no_grad()
def translation_relation_ranks(model, test, known=None, batch: int = None):
    """Raw and filtered rank of every test triple's relation among ALL relations for a TransX or TransR model (int64
    arrays, in test order): the candidates c replace the relation, D_c = D(h, t, c), order ascending by (D, relation
    id).  known: an [n,3] array of triples to filter, or a KnownIndex(side="relation") with n_rows = max(n_ent, n_rel)
    (None: filtered == raw).  batch: rows per native call (default 131072)."""
    test = _translation_test(model, test)
    index, pos_of = _relation_sweep_setup(model, known)
    dev = model.tables["ent"].device
    if batch is None:
        batch = 1 << 17
    if batch <= 0:
        raise ValueError("batch must be positive")
    raw = np.empty(len(test), dtype=np.int64)
    fil = np.empty(len(test), dtype=np.int64)
    filtered = index.key.numel() > 0
    for s in range(0, len(test), batch):
        chunk = torch.as_tensor(test[s:s + batch]).to(dev)
        off = rc = None
        if filtered:
            off, rc = index.cells(chunk[:, 0], chunk[:, 1], pos_of, model.n_rel)
        nb, nk, _ = model.relation_rank_counts(chunk, known_off=off, known_rc=rc)
        nb, nk = nb.cpu().numpy().astype(np.int64), nk.cpu().numpy().astype(np.int64)
        if (nb < 0).any() or (nk < 0).any():
            raise ValueError("a test triple holds an id outside the model's tables")
        raw[s:s + batch] = nb + 1
        fil[s:s + batch] = nb + 1 - nk
    return raw, fil


def _entity_pairs(n_ent: int, pairs) -> np.ndarray:
    """The (h, t) rows as int64 [n,2], ids checked against [0, n_ent) on the host."""
    q = np.asarray(pairs.cpu().numpy() if isinstance(pairs, torch.Tensor) else pairs)
    if q.size == 0:
        return np.zeros((0, 2), dtype=np.int64)
    if q.ndim != 2 or q.shape[1] != 2:
        raise ValueError("pairs must have shape [n, 2] (head, tail)")
    if not np.issubdtype(q.dtype, np.integer):
        raise ValueError("pairs must be integer ids")
    q = q.astype(np.int64)
    if q.min() < 0 or q.max() >= n_ent:
        raise ValueError(f"a pair holds an id outside [0, {n_ent}) entities")
    return q


@torch.no_grad()
def predict_translation_relations(model, pairs, k: int, known=None, batch: int = None):
    """Top-k relation prediction of a TransX / TransR model: for every pair (h, t) the first k relations c in ascending
    (D, c), D = D(h, t, c) -- the relation sweep's own stored distance, so the filtered rank
    (translation_relation_ranks, same `known`) of the j-th entry is j + 1.  known: an [m,3] array or a
    KnownIndex(side="relation") with n_rows = max(n_ent, n_rel); known relations of the pair are skipped.
    Returns (ids int64 [n,k], dist float32 [n,k]) numpy arrays in the pairs' order; padding -1 / +inf.  The stored
    distances (relation_rank_counts(return_scores=True)) are sorted stably on the device in chunks of <= 1024 rows
    (batch: rows per chunk, at most 1024)."""
    k = int(k)
    if k < 1:
        raise ValueError("k must be >= 1")
    q = _entity_pairs(model.n_ent, pairs)
    index, pos_of = _relation_sweep_setup(model, known)
    R, dev = model.n_rel, model.tables["ent"].device
    if batch is None:
        batch = 1024
    if batch <= 0:
        raise ValueError("batch must be positive")
    batch = min(batch, 1024)                     # a [batch, n_rel] distance matrix is sorted per chunk
    ids_out = np.empty((len(q), k), dtype=np.int64)
    dist_out = np.empty((len(q), k), dtype=np.float32)
    filtered = index.key.numel() > 0
    for s0 in range(0, len(q), batch):
        chunk = torch.as_tensor(q[s0:s0 + batch]).to(dev)
        cells = None
        if filtered:
            cells = _known_cells_rc(*index.cells(chunk[:, 0], chunk[:, 1], pos_of, R), R)
        # rows (h, t, any valid relation): the target's counts are discarded, the distances are the row's
        tri = torch.cat([chunk, torch.zeros_like(chunk[:, :1])], 1)
        dist_all = model.relation_rank_counts(tri, return_scores=True)[-1]
        ids, dist = _topk_of_losses(dist_all, torch.arange(R, device=dev), k, cells)
        ids_out[s0:s0 + batch] = ids.to(torch.int64).cpu().numpy()
        dist_out[s0:s0 + batch] = dist.cpu().numpy()
    return ids_out, dist_out


def translation_relation_lines(pairs, ids, dist, test_triples) -> list:
    """The lines of a driver's <name>_predict_relations.tsv: per returned relation, in order,
    'head, tail, position (1-based), relation, distance (%.9g: round-trips fp32), in_test' with in_test = 1 when
    (head, tail, relation) is a test triple.  Padding (id -1) is not written."""
    tset = {tuple(int(x) for x in t) for t in np.asarray(test_triples, dtype=np.int64).reshape(-1, 3)}
    lines = []
    for (h, t), row_ids, row_d in zip(np.asarray(pairs, dtype=np.int64), np.asarray(ids), np.asarray(dist)):
        for j, (c, D) in enumerate(zip(row_ids, row_d)):
            if c >= 0:
                lines.append("%d\t%d\t%d\t%d\t%.9g\t%d\n" % (h, t, j + 1, c, float(D), (int(h), int(t), int(c)) in tset))
    return lines


def write_translation_relation_predictions(model, test, known, k: int, path: str) -> int:
    """The driver's top-k relation file: for the distinct (h, t) pairs of the test triples, in order of first
    appearance, the k best relations filtered by `known`; returns the number of lines."""
    test = np.asarray(test, dtype=np.int64).reshape(-1, 3)
    pairs = distinct_pairs(test[:, :2])
    ids, dist = predict_translation_relations(model, pairs, k, known)
    lines = translation_relation_lines(pairs, ids, dist, test)
    with open(path, "w") as out:
        out.writelines(lines)
    return len(lines)


def _relation_as_head(triples):
    """(h, t, r) rows as (r, t, h): ComplEx's Re sum h r conj(t) and HolE's sum_{k,i} r_k h_i t_{i+k} are symmetric
    under h <-> r, so the relation of (h, ?, t) is the head of (?, t, h) in the same table."""
    if triples is None or isinstance(triples, KnownIndex):
        return triples
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    return t[:, [2, 1, 0]]


def relation_ranks(embeddings: torch.Tensor, test, relation_count: int, known_triples=None, model: str = "complex", **kw):
    """Raw and filtered rank of every test triple's relation among the relation rows [0, relation_count) of a ComplEx
    or HolE table: link_prediction_ranks' head-side sweep on the triples with head and relation exchanged (the scores
    are symmetric under h <-> r).  known_triples: an [n,3] (h, t, r) array, or a KnownIndex(side="head") built from
    triples exchanged the same way.  Further keywords go to link_prediction_ranks."""
    return link_prediction_ranks(embeddings, _relation_as_head(test), np.arange(int(relation_count), dtype=np.int32),
                                 _relation_as_head(known_triples), side="head", model=model, **kw)


def predict_relations(embeddings: torch.Tensor, pairs, relation_count: int, k: int, known_triples=None,
                      model: str = "complex", **kw):
    """Top-k relation prediction of a ComplEx or HolE table for (h, t) pairs: predict_links' head-side sweep over the
    relation rows [0, relation_count) with the query (fixed = t, relation = h).  Returns (ids int64 [n,k], losses
    float32 [n,k]); known relations of the pair are skipped; padding -1 / +inf."""
    q = _entity_pairs(embeddings.shape[0], pairs)
    return predict_links(embeddings, q[:, [1, 0]], np.arange(int(relation_count), dtype=np.int64), k,
                         _relation_as_head(known_triples), side="head", model=model, **kw)


def distinct_pairs(a) -> np.ndarray:
    """The distinct rows of an [n,2] array, in order of first appearance."""
    a = np.asarray(a, dtype=np.int64).reshape(-1, 2)
    if len(a) == 0:
        return a
    _, first = np.unique(a, axis=0, return_index=True)
    return a[np.sort(first)]


def translation_predict_lines(side: str, queries, ids, dist, test_triples) -> list:
    """The lines of a driver's <name>_predict.tsv for one side: per returned candidate, in order,
    'side, fixed, relation, position (1-based), entity, distance (%.9g: round-trips fp32), in_test' with in_test = 1
    when the completed triple is a test triple.  Padding (id -1) is not written."""
    tset = {tuple(int(x) for x in t) for t in np.asarray(test_triples, dtype=np.int64).reshape(-1, 3)}
    lines = []
    for (f, r), row_ids, row_d in zip(np.asarray(queries, dtype=np.int64), np.asarray(ids), np.asarray(dist)):
        for j, (c, D) in enumerate(zip(row_ids, row_d)):
            if c < 0:
                continue
            tri = (int(f), int(c), int(r)) if side == "tail" else (int(c), int(f), int(r))
            lines.append("%s\t%d\t%d\t%d\t%d\t%.9g\t%d\n" % (side, f, r, j + 1, c, float(D), tri in tset))
    return lines


def write_translation_predictions(model, test, known, k: int, path: str, candidate_sets: dict = None) -> int:
    """The driver's top-k prediction file: tails for the distinct (h, r) pairs of the test triples, then heads for the
    distinct (t, r) pairs, each in order of first appearance, filtered by `known`; returns the number of lines.
    candidate_sets ({"tail": CandidateSets, "head": CandidateSets}): each side predicts from its relation's set only."""
    test = np.asarray(test, dtype=np.int64).reshape(-1, 3)
    n = 0
    with open(path, "w") as out:
        for side, cols in (("tail", [0, 2]), ("head", [1, 2])):
            queries = distinct_pairs(test[:, cols])
            ids, dist = predict_translation(model, queries, k, known, side=side,
                                            candidate_sets=None if candidate_sets is None else candidate_sets[side])
            lines = translation_predict_lines(side, queries, ids, dist, test)
            out.writelines(lines)
            n += len(lines)
    return n
