#!/usr/bin/env python3
"""Generate ``ranked_train.npz`` FROM THE REFERENCE ITSELF: the ``samp_score_diff`` its own ``choose_step_neighs`` returns.

    python tests/golden/make_golden_ranked_train.py

A sibling of make_golden_ranked.py, and like it it runs only where the reference tree is mounted.  It rebuilds the yelp_small,
single_rel and five_rel cases with make_golden's graph builder, seeds and batch, wraps ``RL.choose_step_neighs`` and records, for
rho 0.2, 0.5 and 2.0 and per relation of the train-mode forward: ``sample_list``, the score distances the reference kept for
every centre - the neighbour part followed by a positive centre's minority part - (float32, flattened, with offsets) and the set
sizes; per case the batch labels, and the centre and minority scores the reference ranked with.  Data only.  The zip members
carry a fixed date, so running it twice gives identical bytes.  It asserts that no minority cut falls on a tie.
"""
import math
import os
import random
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
_argv, sys.argv = sys.argv, sys.argv[:1]       # (make_golden reads its output directory from argv at import)
import make_golden as MG  # noqa: E402
sys.argv = _argv
RL = MG.RL

OUT = sys.argv[1] if len(sys.argv) > 1 else HERE
RHOS = (0.2, 0.5, 2.0)
CASES = {      # name -> make_golden.pcgnn_case's arguments (its __main__ block)
    "yelp_small": dict(seed=3, n=1500, f=32, rel_deg=(2.5, 9, 28), pos_rate=0.145, emb=64, batch=256),
    "single_rel": dict(seed=9, n=800, f=32, rel_deg=(12,), pos_rate=0.12, emb=32, batch=100),
    "five_rel": dict(seed=37, n=700, f=16, rel_deg=(3, 6, 10, 5, 16), pos_rate=0.14, emb=48, batch=90),
}


def ranked_train_case(seed, n, f, rel_deg, pos_rate, emb, batch, alpha=2.0):
    X, labels, rels, homo = MG.synth_graph(seed, n, f, rel_deg, pos_rate, False)
    rs = np.random.RandomState(seed + 1)
    idx_train = sorted(rs.choice(n, size=int(0.4 * n), replace=False).tolist())
    y_train = labels[np.array(idx_train)]
    train_pos = [v for v in idx_train if labels[v] == 1]
    random.seed(seed)
    picked = MG.pick_step(idx_train, y_train, homo, size=2 * len(train_pos))
    nodes = (picked[:batch - 8] + [7, 11, 12, 13, 14, 15] + picked[:2])[:batch]
    blab = labels[np.array(nodes)]
    out = {"nodes": np.array(nodes, dtype=np.int64), "labels": blab.astype(np.int64),
           "train_pos": np.array(train_pos, dtype=np.int64)}
    min_gap = math.inf
    for rho in RHOS:
        model = MG.build_model(X, rels, train_pos, emb, rho, alpha, seed)
        calls = []
        orig = RL.choose_step_neighs

        def wrap(center_scores, center_labels, neigh_scores, neighs_list, minor_scores, minor_list, sample_list, sample_rate):
            res = orig(center_scores, center_labels, neigh_scores, neighs_list, minor_scores, minor_list, sample_list, sample_rate)
            assert list(minor_list) == train_pos and sample_rate == rho
            calls.append(([int(k) for k in sample_list], [list(map(float, s)) for s in res[1]], [len(s) for s in res[0]],
                          center_scores.detach()[:, 0].numpy().copy(), minor_scores.detach()[:, 0].numpy().copy(),
                          [int(v) for v in center_labels]))
            return res

        RL.choose_step_neighs = wrap
        try:
            model.forward(nodes, torch.LongTensor(blab), True)
        finally:
            RL.choose_step_neighs = orig
        assert len(calls) == len(rels)
        for r, (samples, scores, set_len, cen, minor, lab) in enumerate(calls):
            assert lab == blab.tolist()
            for key, val in (("center_scores", cen.astype(np.float32)), ("minor_scores", minor.astype(np.float32)),
                             (f"sample_list{r}", np.array(samples, dtype=np.int64))):
                assert key not in out or np.array_equal(out[key], val)        # (one table, one model: the same in every call)
                out[key] = val
            for b, k in enumerate(samples):                                   # no minority cut on a tie
                m = int(k * rho)
                if lab[b] == 1 and 0 < m < len(minor):
                    d = torch.sort(torch.abs(torch.tensor(cen[b]) - torch.from_numpy(minor))).values
                    min_gap = min(min_gap, float(d[m] - d[m - 1]))
            off = np.zeros(len(scores) + 1, dtype=np.int64)
            off[1:] = np.cumsum([len(s) for s in scores])
            tag = f"rho{rho}_"
            out[tag + f"score_off{r}"] = off
            # (the reference's .tolist() widened float32 distances to Python floats: back to float32 is exact)
            out[tag + f"scores{r}"] = np.array([x for s in scores for x in s], dtype=np.float64).astype(np.float32)
            out[tag + f"set_len{r}"] = np.array(set_len, dtype=np.int64)
    assert min_gap > 0, "a minority cut falls on a tie - pick another seed"
    out["min_minor_gap"] = np.float64(min_gap)
    return out


def save_fixed(path, arrays):
    """np.savez's format with a fixed member date: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as fh:
                np.lib.format.write_array(fh, np.asanyarray(arrays[k]), allow_pickle=False)


if __name__ == "__main__":
    out = {}
    for name, kw in CASES.items():
        for k, v in ranked_train_case(**kw).items():
            out[f"{name}_{k}"] = v
        print(f"{name}: smallest gap at a minority cut = {float(out[name + '_min_minor_gap']):.3e}")
    path = os.path.join(OUT, "ranked_train.npz")
    save_fixed(path, out)
    print(f"ranked_train.npz: {os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays")
