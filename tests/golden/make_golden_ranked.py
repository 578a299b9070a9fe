#!/usr/bin/env python3
"""Generate ``ranked.npz`` FROM THE REFERENCE ITSELF: the ``samp_scores`` its own ``choose_step_test`` returns.

    python tests/golden/make_golden_ranked.py

Like make_golden.py it runs only where the reference tree is mounted.  It rebuilds the yelp_small, single_rel and five_rel
cases with make_golden's graph builder, seeds and batch, wraps ``RL.choose_step_test`` and records, per relation of the
test-mode forward: ``sample_list`` and the score distances the reference kept for every centre (float32, flattened, with
offsets).  Data only.  Running it twice gives identical bytes (no timestamps: ``np.savez``, arrays in a fixed order).
"""
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
_argv, sys.argv = sys.argv, sys.argv[:1]       # (make_golden reads its output directory from argv at import)
import make_golden as MG  # noqa: E402
sys.argv = _argv
RL = MG.RL

OUT = sys.argv[1] if len(sys.argv) > 1 else HERE
CASES = {      # name -> make_golden.pcgnn_case's arguments (its __main__ block)
    "yelp_small": dict(seed=3, n=1500, f=32, rel_deg=(2.5, 9, 28), pos_rate=0.145, emb=64, batch=256, rho=0.5),
    "single_rel": dict(seed=9, n=800, f=32, rel_deg=(12,), pos_rate=0.12, emb=32, batch=100, rho=0.5),
    "five_rel": dict(seed=37, n=700, f=16, rel_deg=(3, 6, 10, 5, 16), pos_rate=0.14, emb=48, batch=90, rho=0.5),
}


def ranked_case(seed, n, f, rel_deg, pos_rate, emb, batch, rho, alpha=2.0):
    X, labels, rels, homo = MG.synth_graph(seed, n, f, rel_deg, pos_rate, False)
    rs = np.random.RandomState(seed + 1)
    idx_train = sorted(rs.choice(n, size=int(0.4 * n), replace=False).tolist())
    y_train = labels[np.array(idx_train)]
    train_pos = [v for v in idx_train if labels[v] == 1]
    random.seed(seed)
    picked = MG.pick_step(idx_train, y_train, homo, size=2 * len(train_pos))
    nodes = (picked[:batch - 8] + [7, 11, 12, 13, 14, 15] + picked[:2])[:batch]
    blab = labels[np.array(nodes)]
    model = MG.build_model(X, rels, train_pos, emb, rho, alpha, seed)

    calls = []
    orig = RL.choose_step_test

    def wrap(center_scores, neigh_scores, neighs_list, sample_list):
        out = orig(center_scores, neigh_scores, neighs_list, sample_list)
        calls.append(([int(k) for k in sample_list], [list(map(float, s)) for s in out[1]], [sorted(s) for s in out[0]]))
        return out

    RL.choose_step_test = wrap
    try:
        model.forward(nodes, torch.LongTensor(blab), False)
    finally:
        RL.choose_step_test = orig
    assert len(calls) == len(rels)
    out = {"nodes": np.array(nodes, dtype=np.int64)}
    for r, (samples, scores, sets) in enumerate(calls):
        off = np.zeros(len(scores) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(s) for s in scores])
        out[f"sample_list{r}"] = np.array(samples, dtype=np.int64)
        out[f"score_off{r}"] = off
        # (the reference's .tolist() widened float32 distances to Python floats: back to float32 is exact)
        out[f"scores{r}"] = np.array([x for s in scores for x in s], dtype=np.float64).astype(np.float32)
        out[f"set_len{r}"] = np.array([len(s) for s in sets], dtype=np.int64)
    return out


if __name__ == "__main__":
    out = {}
    for name, kw in CASES.items():
        for k, v in ranked_case(**kw).items():
            out[f"{name}_{k}"] = v
    path = os.path.join(OUT, "ranked.npz")
    np.savez(path, **{k: out[k] for k in sorted(out)})
    print(f"ranked.npz: {os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays")
