"""The workloads of tests/test_gpu_update_onetile.py and of tools/dev/onetile_bits.py, which records their fixtures:
five one-tile training steps (B = 4096, d = 200) whose table and losses are hashed.  Test infrastructure only.

A pair is hinge-active (live) when its loss is positive.  Rows are clipped to norm 1 and scores pass a sigmoid, so a
fresh table leaves EVERY pair live at margin 0.2; the deterministic cases therefore run WARM deterministic steps first
(the oracle's C port on the host: 61 % of the pairs live after 600 steps for ComplEx, 44 % for HolE), and the default-mode
workload, which cannot be trained without growing rows of more than 16 slots, has margin 0.0 beside the two others
(sigma(pos) > sigma(neg) in about half the pairs of any table)."""
import hashlib

import numpy as np

B, D_EMB, STEPS = 4096, 200, 5
WARM = 600
MARGINS = (0.2, 5.0)
PLAIN_MARGINS = (0.0, 0.2, 5.0)
MODELS = ("complex", "hole")
ITEM_CAP = 16


def sha(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)
    return hashlib.sha256(a.tobytes()).hexdigest()


def det_key(model, margin):
    return f"det/{model}/margin{margin}"


def plain_key(model, margin):
    return f"plain/{model}/margin{margin}"


def live_share(loss):
    """share of hinge-active pairs in each step of a [steps, B] loss tensor"""
    return [float(v) for v in (loss > 0).float().mean(1).cpu()]


def run_det(model, margin):
    """Trainer(deterministic=True) on the FB15k-shaped headline workload: hot rows (> 16 slots) reduced in fixed order.
    WARM steps, then the STEPS hashed ones.  Returns (hashes, share of live pairs in each hashed step)."""
    import torch
    from graphembeddings_amd import data as D, hole as H
    fb = D.fb15k_shape()
    names, id_to_type, offsets, ids = fb.type_arrays()
    tt = H.TypeTables.from_host(id_to_type, offsets, ids, padded_size=1024)
    tri = torch.as_tensor(D.synthetic_fb15k_triples(fb, n_triples=483142, seed=0)).cuda()
    emb = H.init_embeddings(fb.entity_count, D_EMB, seed=0)
    tr = H.Trainer(emb, tri, tt, B, margin=margin, learning_rate=0.1, decay_steps=32.0 * 117, seed=0, model=model,
                   spectral_resident=(model == "hole"), deterministic=True)
    tr.run(WARM)
    loss = tr.run(STEPS, keep_losses=True)
    torch.cuda.synchronize()
    out = {"table": sha(tr.embeddings), "losses": sha(loss)}
    tr.close()
    return out, live_share(loss)


N_REL, N_ENT = 460, 50_000


def no_hot_row_triples(seed=7):
    """STEPS batches of B pairs in which no table row collects more than 16 gradient slots: relation j is in
    2 + j % 15 pairs of every batch (2 ... 16: a relation row holds one slot per pair of its relation), heads and tails
    are uniform over 50,000 entities.  Returns (HolEData, triples [STEPS * B, 3] as head, tail, relation)."""
    from graphembeddings_amd import data as D
    data, tri = D.synthetic_large(n_entities=N_ENT, n_relations=N_REL, n_types=12, n_triples=STEPS * B, seed=seed, zipf_s=0.0)
    rel = np.repeat(np.arange(N_REL), 2 + np.arange(N_REL) % 15)
    assert len(rel) >= B
    rel = rel[:B]
    rng = np.random.default_rng(seed)
    tri = tri.copy()
    for s in range(STEPS):
        tri[s * B:(s + 1) * B, 2] = rng.permutation(rel)
    return data, tri


def slots_per_row(pos, neg, n_rows):
    """Gradient slots each table row collects in one step (tests/prep_model.py: the three rows of the positive triple and
    the one row in which the negative differs)."""
    cnt = np.bincount(pos.reshape(-1), minlength=n_rows)
    diff = pos != neg
    has = diff.any(1)
    c = diff.argmax(1)
    cnt += np.bincount(neg[np.arange(len(neg)), c][has], minlength=n_rows)
    return cnt


def run_plain(model, margin):
    """Default mode (float atomics on hot rows) on the workload without a hot row.  One step per call, so that every
    step's negatives can be read back.  Returns (hashes, slots per row of each step, share of live pairs of each step)."""
    import torch
    from graphembeddings_amd import data as D, hole as H
    data, tri = no_hot_row_triples()
    names, id_to_type, offsets, ids = D.synthetic_large_type_arrays(data)
    tt = H.TypeTables.from_host(id_to_type, offsets, ids, padded_size=1024)
    emb = H.init_embeddings(data.entity_count, D_EMB, seed=1)
    tr = H.Trainer(emb, torch.as_tensor(tri).cuda(), tt, B, margin=margin, learning_rate=0.1, decay_steps=32.0 * 117, seed=3,
                   model=model, spectral_resident=(model == "hole"))
    losses, counts = [], []
    for s in range(STEPS):
        losses.append(tr.run(1, keep_losses=True).clone())
        torch.cuda.synchronize()
        counts.append(slots_per_row(tri[s * B:(s + 1) * B].astype(np.int64), tr._neg.cpu().numpy().astype(np.int64),
                                    data.entity_count))
    loss = torch.cat(losses)
    out = {"table": sha(tr.embeddings), "losses": sha(loss)}
    tr.close()
    return out, counts, live_share(loss)
