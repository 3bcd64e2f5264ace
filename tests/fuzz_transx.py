"""Randomised check of the TransE / TransH / TransD kernels (ge_transx_score, ge_transx_hinge_step and the native
loop ge_transx_train_steps) against the fp64 restatement tests/transx_ref.py: model, norm, d in 1 ... 1024, ragged
B up to 40 k, E from 2 to 300 k, R from 1 to 1,345 with a Zipf relation column, and margins that leave all, none or
some pairs active.  Each table element is held to 5e-6 + 2^-20 * lr * (sum of |terms| reaching it, as
transx_ref.hinge_grads(magnitude=True) bounds them) + 2^-23 * |element|, the loss to
5e-6 relative, scores to 1e-5 relative + 1e-7.  Not collected by pytest: `python tests/fuzz_transx.py [n_cases] [seed]`
on a GPU box."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODELS = ("transe", "transh", "transd")
EDGE_D = (1, 3, 4, 8, 9, 31, 32, 33, 36, 64, 65, 100, 128, 132, 200, 256, 1023, 1024)
MAX_ED = 12_000_000          # entity rows x d: the reference builds several dense fp64 copies of each table
MAX_BD = 4_000_000           # pairs x d: and several fp64 [B, d] arrays per pass


def _log_uniform(rng, lo, hi):
    return int(np.exp(rng.uniform(np.log(lo), np.log(hi + 1))))


def _close(model, l1, before, after, loss, pos, neg, lr, margin, TR):
    """(worst err / bound over the tables, max abs err, loss rel err) of one step."""
    new, rloss = TR.sgd_step(model, before, pos, neg, lr, margin, l1)
    mags = TR.hinge_grads(model, before, pos, neg, margin, l1, magnitude=True)[1]
    ratio, err_max = 0.0, 0.0
    for k in new:
        err = np.abs(after[k] - new[k])
        # the last term is the rounding of the stored element itself: rows grow to ~1e4 at a few entities
        ratio = max(ratio, float((err / (5e-6 + 2.0 ** -20 * lr * mags[k] + 2.0 ** -23 * np.abs(new[k]))).max()))
        err_max = max(err_max, float(err.max()))
    return ratio, err_max, abs(loss - rloss) / max(1.0, abs(rloss))


def main():
    import torch
    from graphembeddings_amd import transx as X
    from tests import transx_ref as TR

    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
    host = lambda m: {k: v.cpu().numpy().astype(np.float64) for k, v in m.tables.items()}
    dev = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int32)).cuda()
    worst = dict.fromkeys(("score_ratio", "step_ratio", "step_abs", "loss_rel", "loop_ratio", "loop_abs"), 0.0)
    fails = []
    for case in range(n_cases):
        model = MODELS[int(rng.integers(0, 3))]
        l1 = bool(rng.integers(0, 2))
        d = int(rng.choice(EDGE_D)) if rng.random() < 0.5 else int(rng.integers(1, 1025))
        E, R, B = _log_uniform(rng, 2, 300_000), _log_uniform(rng, 1, 1345), _log_uniform(rng, 1, 40_000)
        d = max(1, min(d, MAX_ED // E, MAX_BD // B))
        lr = float(rng.choice([0.001, 0.01, 0.05]))
        m = X.TransX(model, E, R, d, l1=l1, seed=int(rng.integers(0, 2**31)))
        tabs = host(m)
        rel = (rng.zipf(1.3, B) - 1) % R
        pos = np.stack([rng.integers(0, E, B), rng.integers(0, E, B), rel], 1)
        neg = pos.copy()
        neg[np.arange(B), rng.integers(0, 2, B)] = rng.integers(0, E, B)
        # score
        got = m.score(dev(pos)).cpu().numpy().astype(np.float64)
        dp = TR.score(model, tabs, pos, l1)
        score_ratio = float((np.abs(got - dp) / (1e-5 * np.abs(dp) + 1e-7)).max())
        # step, with a margin that leaves all, none or about half of the pairs active
        dn = TR.score(model, tabs, neg, l1)
        mode = ("all", "none", "some")[int(rng.integers(0, 3))]
        margin = float({"all": dn.max() - dp.min() + 1.0, "none": dn.min() - dp.max() - 1.0,
                        "some": np.median(dn - dp)}[mode])
        z = dp - dn + margin
        near = np.abs(z) <= 1e-4 * (dp + dn + abs(margin) + 1e-3)  # fp32 may decide these either way: neg = pos
        neg[near] = pos[near]
        n_active = int(TR.active_mask(model, tabs, pos, neg, margin, l1).sum())
        loss = float(m.step(dev(pos), dev(neg), lr, margin))
        step_ratio, step_abs, loss_rel = _close(model, l1, tabs, host(m), loss, pos, neg, lr, margin, TR)
        # a short native loop on a random triple list.  It must equal its own draws through single steps bitwise,
        # and each of those steps is held to fp64 from its own pre-step tables (errors compound across steps on
        # rows of thousands of slots, so a run is not compared with a fp64 run).
        T = min(max(E, 8), 3000)
        tri = np.unique(np.stack([rng.integers(0, E, T), rng.integers(0, E, T), (rng.zipf(1.3, T) - 1) % R], 1), axis=0)
        Bl = min(B, 4000)
        single = X.TransX(model, E, R, d, l1=l1, seed=0)
        for k, v in m.tables.items():
            single.tables[k].copy_(v)
        tr = m.trainer(tri, Bl, margin=margin, learning_rate=lr, seed=case)
        # lr over the hottest row's slots: with thousands of slots on one row three steps at the step's lr diverge
        p, n = (x.cpu().numpy() for x in tr.draw(0))
        ids = np.concatenate([p[:, 0], p[:, 1], n[:, 0], n[:, 1]])
        hot = max(np.bincount(ids[ids >= 0]).max(), np.bincount(p[:, 2]).max())
        tr.lr = lr_loop = min(lr, 0.5 / hot)
        losses = tr.run(3).cpu().numpy()
        loop_ratio, loop_abs, loop_loss, ambiguous, bitwise = 0.0, 0.0, 0.0, 0, True
        for s in range(3):
            pd, nd = tr.draw(s)
            before = host(single)
            ls = float(single.step(pd, nd, lr_loop, margin))
            bitwise = bitwise and ls == losses[s]
            p, n = pd.cpu().numpy(), nd.cpu().numpy()
            # a (fixed entity, relation) with no free entity left draws -1 (ge_bernoulli_dev.h): the step skips it
            ok = (n[:, :2] >= 0).all(1)
            p, n = p[ok], n[ok]
            dps, dns = TR.score(model, before, p, l1), TR.score(model, before, n, l1)
            # a pair with z within fp32 rounding of 0 may go either way: such a run is reported, not judged
            ambiguous += int((np.abs(dps - dns + margin) <= 1e-5 * (dps + dns + abs(margin) + 1e-3)).sum())
            r_, a_, l_ = _close(model, l1, before, host(single), ls, p, n, lr_loop, margin, TR)
            loop_ratio, loop_abs, loop_loss = max(loop_ratio, r_), max(loop_abs, a_), max(loop_loss, l_)
        bitwise = bitwise and all(torch.equal(v, single.tables[k]) for k, v in m.tables.items())
        rec = {"case": case, "model": model, "l1": l1, "d": d, "E": E, "R": R, "B": B, "lr": lr, "mode": mode,
               "active": n_active, "score_err_over_bound": score_ratio, "step_err_over_bound": step_ratio,
               "step_abs": step_abs, "loss_rel": loss_rel, "loop_B": Bl, "loop_lr": lr_loop,
               "loop_err_over_bound": loop_ratio, "loop_abs": loop_abs, "loop_loss_rel": float(loop_loss),
               "loop_ambiguous_pairs": ambiguous, "loop_equals_single_steps": bitwise}
        print(json.dumps(rec), flush=True)
        for k, v in (("score_ratio", score_ratio), ("step_ratio", step_ratio), ("step_abs", step_abs),
                     ("loss_rel", loss_rel), ("loop_ratio", loop_ratio), ("loop_abs", loop_abs)):
            if not (ambiguous and k.startswith("loop")):
                worst[k] = max(worst[k], v)
        if not (score_ratio <= 1.0 and step_ratio <= 1.0 and loss_rel <= 5e-6
                and bitwise and (ambiguous or (loop_ratio <= 1.0 and loop_loss <= 5e-6))):
            fails.append(rec)
        del m, single, tr
        torch.cuda.empty_cache()
    print(json.dumps({"cases": n_cases, "worst": worst, "failed": fails}))
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
