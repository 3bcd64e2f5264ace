"""Restatement, in numpy, of what the translation models' masked sweeps (ge_transx_rank_masked, ge_transr_rank_masked,
ge_transx_topk_masked, ge_transr_topk_masked) return, as a function of the distances the UNMASKED rank sweep stores in
scores_out: the oracle of tests/test_gpu_translation_candidate_sets.py and tests/test_gpu_abi_guard_translation_masked.py,
itself checked on a hand-written example in tests/test_translation_candidate_sets_host.py.  Not product code.

Candidate position = entity id.  adm: bool [n_sets, E]; row_set: int [B], -1 = unrestricted, any other value outside
[0, n_sets) = a bad row; known: bool [B, E] or None."""
import numpy as np

I32, I64, U32, F32 = np.int32, np.int64, np.uint32, np.float32


def words(K):
    """ge_candidate_mask_words: four words per 128-candidate tile."""
    return 4 * ((K + 127) // 128)


def pack(bits, n_words=None, pad=False):
    """uint32 [n_sets, n_words] of a bool [n_sets, K]: bit c & 31 of word c >> 5.  pad: the bits at positions >= K set
    (the sweeps must ignore them)."""
    bits = np.asarray(bits, dtype=bool)
    n_words = words(bits.shape[1]) if n_words is None else n_words
    full = np.full((bits.shape[0], n_words * 32), bool(pad))
    full[:, :bits.shape[1]] = bits
    return np.packbits(full, axis=1, bitorder="little").view(U32).reshape(bits.shape[0], n_words)


def bad_rows(row_set, n_sets):
    rs = np.asarray(row_set, dtype=I64)
    return (rs < -1) | (rs >= n_sets)


def admitted(adm, row_set):
    """bool [B, E]: entity c is admissible for row i (an unrestricted row admits everything, a bad row nothing)."""
    adm = np.asarray(adm, dtype=bool)
    rs = np.asarray(row_set, dtype=I64)
    rows = adm[np.clip(rs, 0, adm.shape[0] - 1)]
    rows[rs == -1] = True
    rows[bad_rows(rs, adm.shape[0])] = False
    return rows


def masked_counts(sc, true_id, adm, row_set, known=None):
    """(n_before, n_known_before int32 [B], bad bool [B]): the admissible c with (D_c, c) below (D_true, true) and those
    of them that are known; a bad row has -1 / -1 (and a NaN true_dist, which the caller checks with `bad`)."""
    sc = np.asarray(sc, dtype=F32)
    B, E = sc.shape
    true_id = np.asarray(true_id, dtype=I64)
    dt = sc[np.arange(B), true_id][:, None]
    before = (sc < dt) | ((sc == dt) & (np.arange(E)[None, :] < true_id[:, None]))
    rows = admitted(adm, row_set)
    nb = (before & rows).sum(1).astype(I32)
    nk = (before & rows & known).sum(1).astype(I32) if known is not None else np.zeros(B, I32)
    bad = bad_rows(row_set, np.asarray(adm).shape[0])
    nb[bad], nk[bad] = -1, -1
    return nb, nk, bad


def masked_topk(sc, k, adm, row_set, known=None):
    """(ids int32 [B, k], dist float32 [B, k]): the first k entities in ascending (D, c) that are admissible and not
    known; padding -1 / +inf (a +inf distance is padding too); -1 / NaN for a bad row and for a row with a NaN distance
    at an entity that is admissible and not known."""
    sc = np.asarray(sc, dtype=F32)
    B, E = sc.shape
    rows = admitted(adm, row_set)
    if known is not None:
        rows &= ~np.asarray(known, dtype=bool)
    bad = bad_rows(row_set, np.asarray(adm).shape[0])
    ids = np.full((B, k), -1, I32)
    dist = np.full((B, k), np.inf, F32)
    for b in range(B):
        c = np.nonzero(rows[b])[0]
        D = sc[b, c]
        if bad[b] or np.isnan(D).any():
            dist[b] = np.nan
            continue
        keep = D < np.inf
        c, D = c[keep], D[keep]
        o = np.lexsort((c, D))[:k]
        ids[b, :o.size], dist[b, :o.size] = c[o], D[o]
    return ids, dist


def cells_from_mask(mask):
    """ge_known_cells' lists of a [B, E] bool mask (pos_of = the identity): (known_off int32, known_rc uint16)."""
    B, K = mask.shape
    n_rt, n_ct = (B + 127) // 128, (K + 127) // 128
    off, rc = [0], []
    for rt in range(n_rt):
        for ct in range(n_ct):
            r, c = np.nonzero(mask[rt * 128:(rt + 1) * 128, ct * 128:(ct + 1) * 128])
            rc.append(((r << 7) | c).astype(np.uint16))
            off.append(off[-1] + len(r))
    rc = np.concatenate(rc) if rc else np.zeros(0, np.uint16)
    return np.asarray(off, I32), (rc if len(rc) else np.zeros(1, np.uint16))
