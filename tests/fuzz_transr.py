"""Randomised check of the TransR kernels (ge_transr_score, ge_transr_adam_step) against the fp64 restatement
tests/transr_ref.py: norm, dim_e and dim_r in 1 ... 256 (square or not), ragged B up to 20 k, E from 2 to 100 k, R
from 1 to 1,345 with a Zipf relation column (or every pair on one relation), and margins that leave all, none or
some pairs active.  One Adam step at t = 1 from zero moments, so m = (1 - b1) g: each element of g is held to
(dim_e + dim_r + 2 B) 2^-22 * (sum of |terms| reaching it, transr_ref.hinge_grads(magnitude=True)), scores to
(dim_e + dim_r + 8) 2^-22 (4 x for L2) of their terms, the loss to 1e-5 relative.  A case with a pair whose z, or
an L1 component of u, lies within rounding of 0 is reported, not judged.  Not collected by pytest:
`python tests/fuzz_transr.py [n_cases] [seed]` on a GPU box."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EDGE_D = (1, 2, 3, 4, 7, 8, 15, 16, 17, 32, 33, 64, 100, 127, 128, 200, 255, 256)
MAX_MAT = 40_000_000         # R x dim_e x dim_r: the reference holds several fp64 copies


def _log_uniform(rng, lo, hi):
    return int(np.exp(rng.uniform(np.log(lo), np.log(hi + 1))))


def main():
    import torch
    from graphembeddings_amd import transr as XR
    from tests import transr_ref as RR

    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    eps32 = 2.0 ** -23
    worst = {"score_ratio": 0.0, "grad_ratio": 0.0, "loss_rel": 0.0}
    fails = []
    for case in range(n_cases):
        dim_e, dim_r = int(rng.choice(EDGE_D)), int(rng.choice(EDGE_D))
        l1 = bool(rng.integers(0, 2))
        R = _log_uniform(rng, 1, 1345)
        while R * dim_e * dim_r > MAX_MAT:
            R = max(1, R // 2)
        E = max(2, _log_uniform(rng, 2, 100_000) if rng.random() < 0.5 else _log_uniform(rng, 2, 3000))
        B = _log_uniform(rng, 1, 20_000 if dim_e * dim_r <= 4096 else 3000)
        hot = int(rng.integers(0, R)) if rng.random() < 0.2 else None
        pos, neg = RR.skewed_batch(rng, E, R, B, hot=hot)
        m = XR.TransR(E, R, dim_e, dim_r, l1=l1, seed=case)
        tabs = {k: v.cpu().numpy().astype(np.float64) for k, v in m.tables.items()}
        d = RR.score(tabs, pos, l1) - RR.score(tabs, neg, l1)
        mode = rng.choice(["some", "all", "none"])
        margin = {"some": float(np.median(-d)) if B else 1.0, "all": float(-d.min() + 1.0),
                  "none": float(-d.max() - 1.0)}[mode]
        pd, nd = (torch.as_tensor(x).cuda() for x in (pos, neg))
        got = m.score(pd).cpu().numpy().astype(np.float64)
        ref, mag = RR.score(tabs, pos, l1), RR.score_magnitude(tabs, pos, l1)
        score_ratio = float((np.abs(got - ref) / ((2 if l1 else 4) * (dim_e + dim_r + 8) * 2 * eps32 * mag + 1e-30)).max())
        loss = float(m.step(pd, nd, margin))
        rloss, g = RR.hinge_grads(tabs, pos, neg, margin, l1)
        _, gm = RR.hinge_grads(tabs, pos, neg, margin, l1, magnitude=True)
        z = d + margin
        ua = np.concatenate([RR.residual(tabs, pos), RR.residual(tabs, neg)])
        ua_mag = np.concatenate([RR.residual_magnitude(tabs, t) for t in (pos, neg)])
        zmag = RR.score_magnitude(tabs, pos, l1) + RR.score_magnitude(tabs, neg, l1) + abs(margin)
        ambiguous = int((np.abs(z) <= (dim_e + dim_r + 8) * 4 * eps32 * zmag).sum())
        if l1:
            ambiguous += int((np.abs(ua) <= (dim_e + 8) * 2 * eps32 * (ua_mag + 1e-30)).sum())
        ratio = 0.0
        for k, (mk, _) in ((k, m.moments(k)) for k in m.tables):
            gk = mk.cpu().numpy().astype(np.float64) / (1.0 - np.float32(0.9))
            bound = (dim_e + dim_r + 2 * B) * 2 * eps32 * gm[k] + 4 * eps32 * np.abs(g[k]) + 1e-30
            ratio = max(ratio, float((np.abs(gk - g[k]) / bound).max()))
        loss_rel = abs(loss - rloss) / max(1.0, abs(rloss))
        rec = {"case": case, "l1": l1, "dim_e": dim_e, "dim_r": dim_r, "E": E, "R": R, "B": B, "hot": hot,
               "mode": str(mode), "active": int((z >= 0).sum()), "ambiguous": ambiguous,
               "score_err_over_bound": score_ratio, "grad_err_over_bound": ratio, "loss_rel": loss_rel}
        print(json.dumps(rec), flush=True)
        worst["score_ratio"] = max(worst["score_ratio"], score_ratio)
        if not ambiguous:
            worst["grad_ratio"] = max(worst["grad_ratio"], ratio)
            worst["loss_rel"] = max(worst["loss_rel"], loss_rel)
        if score_ratio > 1.0 or (not ambiguous and (ratio > 1.0 or loss_rel > 1e-5)):
            fails.append(rec)
        del m
        torch.cuda.empty_cache()
    print(json.dumps({"cases": n_cases, "worst": worst, "failed": fails}))
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
