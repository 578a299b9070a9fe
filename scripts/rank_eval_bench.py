"""Wall clock of the ranking metrics' stage after ``infer``, three ways, on the same probabilities.

    python scripts/rank_eval_bench.py [--reps 5] [--only yelp,powerlaw] [--ks 100,1000]

Per set, after a warm-up, the median of --reps passes (synchronised at both ends) of the stage that turns the device-resident
class probabilities [n, 2] into average precision, G-mean and precision / recall at every k:
  (a) host:   copy [n, 2] to the host, then utils.host_ranking (average_precision, precision_recall_at_k, conf_gmean);
  (b) device: utils.device_ranking (pcg_pr_counts + pcg_topk_alerts, one small copy, the host statements);
  (c) torch:  a torch-on-device restatement with the same tie rule - torch.sort(p1, descending=True, stable=True), a gather of
              the labels, a cumulative sum, unique_consecutive - and a copy of its points.
The script asserts (a) == (b) in value and reports, for every pair of ways, whether the gap between their medians exceeds the
slower way's own max - min over the repetitions.  One JSON line per set.  Sets: yelp_like(0) held-out ids and whole graph,
power_law(2 M, 40 M) whole graph."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def torch_ranking(prob, lab, ks, U):
    """(c): the same integers from torch's stable sort, then the same host statements"""
    n = prob.shape[0]
    p1 = prob[:, 1] + 0.0
    srt, order = torch.sort(p1, descending=True, stable=True)
    y = (lab[order] != 0).to(torch.int64)
    hits = torch.cumsum(y, 0)
    _, counts = torch.unique_consecutive(srt, return_counts=True)
    last = torch.cumsum(counts, 0) - 1                                  # the last row of every score group
    tp_all = hits[last]
    keep = torch.ones_like(tp_all, dtype=torch.bool)
    keep[1:] = tp_all[1:] > tp_all[:-1]                                 # groups that hold a positive: recall changes
    keep[0] = tp_all[0] > 0
    pred = prob[:, 1] > prob[:, 0]
    conf = torch.stack([((~pred) & (lab == 0)).sum(), (pred & (lab == 0)).sum(), ((~pred) & (lab != 0)).sum(), (pred & (lab != 0)).sum()])
    at = torch.tensor([min(k, n) - 1 for k in ks], dtype=torch.int64, device=prob.device)
    words = torch.cat([conf, hits[at], tp_all[keep], (last + 1)[keep]]).cpu().numpy()
    tn, fp, fn, tp = (int(v) for v in words[:4])
    G = (len(words) - 4 - len(ks)) // 2
    pts = words[4 + len(ks):]
    m = U.ranking_from_counts([tp, fp, fn, tn, tp + fn, tn + fp, G, 0], pts[:G], pts[G:])
    hk = {min(k, n): int(h) for k, h in zip(ks, words[4:4 + len(ks)])}
    prec, rec = U._rates_at_k(lambda ke: hk[ke], ks, n, m["n_pos"])
    return {"average_precision": m["average_precision"], "gmean": m["gmean"], "precision_at": prec, "recall_at": rec,
            "n_pos": m["n_pos"], "n_points": m["n_points"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="yelp,powerlaw")
    ap.add_argument("--ks", default="100,1000")
    args = ap.parse_args()
    import pcgnn_amd  # noqa: F401
    from pcgnn_amd import synth, utils as U
    from pcgnn_amd.handler import PCGNNTrainer
    dev = torch.device("cuda", 0)
    only = args.only.split(",")
    ks = tuple(int(k) for k in args.ks.split(","))
    cases = []
    if "yelp" in only:
        cases.append(("yelp", lambda: synth.yelp_like(0), 1024, ["held_out", "whole"], 3))
    if "powerlaw" in only:
        cases.append(("powerlaw_2m", lambda: synth.power_law(2_000_000, 40_000_000, 0), 4096, ["whole"], 1))
    for name, make, B, sets, epochs in cases:
        t0 = time.time()
        w = make()
        tr = PCGNNTrainer(w, dict(engine="graph", batch_size=B, seed=0), dev)
        for _ in range(epochs):
            tr.run_epoch_one_graph()
        fz = tr.fused
        print(f"# {name}: built in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
        for which in sets:
            ids = np.arange(w.n)
            if which == "held_out":
                ids = ids[~np.isin(ids, w.idx_train)]
            labels = np.asarray(w.labels)[ids]
            lab_dev = torch.from_numpy(labels.astype(np.int32)).to(dev)
            n1 = int(labels.sum())
            with torch.no_grad():
                prob = torch.sigmoid(fz.infer(torch.as_tensor(ids, dtype=torch.int32, device=dev))).float()
            ways = {"host": lambda: U.host_ranking(labels, prob.cpu().numpy(), ks),
                    "device": lambda: U.device_ranking(prob, lab_dev, ks, cap=n1),
                    "torch": lambda: torch_ranking(prob, lab_dev, ks, U)}
            rows = {k: [] for k in ways}
            for rep in range(args.reps + 1):                            # (pass 0 is the warm-up)
                res = {}
                for k, fn in ways.items():
                    ms, res[k] = wall(fn)
                    if rep:
                        rows[k].append(ms)
                assert res["host"] == res["device"], (res["host"], res["device"])
                torch_same = res["torch"] == res["host"]
            med = {k: float(np.median(v)) for k, v in rows.items()}
            spread = {k: float(max(v) - min(v)) for k, v in rows.items()}
            gaps = {}
            for a, b in (("host", "device"), ("torch", "device"), ("host", "torch")):
                slow = a if med[a] >= med[b] else b
                gaps[f"{a}_vs_{b}"] = dict(faster=b if slow == a else a, gap_ms=round(abs(med[a] - med[b]), 4),
                                           exceeds_slower_spread=abs(med[a] - med[b]) > spread[slow])
            m = res["device"]
            print(json.dumps(dict(workload=name, set=which, n=len(ids), n_pos=n1, n_points=m["n_points"], ks=list(ks),
                                  host_ms=round(med["host"], 4), device_ms=round(med["device"], 4), torch_ms=round(med["torch"], 4),
                                  host_spread_ms=round(spread["host"], 4), device_spread_ms=round(spread["device"], 4),
                                  torch_spread_ms=round(spread["torch"], 4), gaps=gaps, host_equals_device=True,
                                  torch_equals_host=bool(torch_same), average_precision=m["average_precision"], gmean=m["gmean"],
                                  precision_at={str(k): v for k, v in m["precision_at"].items()})), flush=True)
        del tr, fz
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
