"""Event-timed evaluation passes: the per-batch predict loop (what utils.test ran before FusedPCGNN.infer existed, restated
here at the bench batch sizes) against one FusedPCGNN.infer call, on the same engine and the same ids.

    python scripts/infer_bench.py [--reps 5] [--big] [--only yelp,amazon,powerlaw]

Sets: yelp_like(0) held-out ids (the labelled ids not in idx_train - the reference splits them into validation and test) and
the whole graph; amazon_like(0) held-out ids and whole graph; power_law(2 M, 40 M) whole graph; --big: power_law(10 M, 200 M)
whole graph.  One JSON line per set: ms per pass (median of --reps, after one warm-up pass each) and nodes/s, both ways."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def old_pass(fz, ids_dev, B):
    out = []
    for s in range(0, ids_dev.numel(), B):
        out.append(torch.sigmoid(fz.predict(ids_dev[s:s + B], None, False)[0]))
    prob = torch.cat(out)
    fz.check()
    return prob


def new_pass(fz, ids_dev, B):
    prob = torch.sigmoid(fz.infer(ids_dev))
    fz.check()
    return prob


def timed(fn, reps):
    fn()                                                   # warm-up (workspaces, kernel attributes)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--big", action="store_true", help="also power_law(10 M, 200 M), whole graph")
    ap.add_argument("--only", default="yelp,amazon,powerlaw")
    args = ap.parse_args()
    import pcgnn_amd  # noqa: F401
    from pcgnn_amd import synth
    from pcgnn_amd.handler import PCGNNTrainer
    dev = torch.device("cuda", 0)
    cases = []
    only = args.only.split(",")
    if "yelp" in only:
        cases.append(("yelp", lambda: synth.yelp_like(0), 1024, 0, ["held_out", "whole"]))
    if "amazon" in only:
        cases.append(("amazon", lambda: synth.amazon_like(0), 256, 3305, ["held_out", "whole"]))
    if "powerlaw" in only:
        cases.append(("powerlaw_2m", lambda: synth.power_law(2_000_000, 40_000_000, 0), 4096, 0, ["whole"]))
    if args.big:
        cases.append(("powerlaw_10m", lambda: synth.power_law(10_000_000, 200_000_000, 0), 4096, 0, ["whole"]))
    for name, make, B, first, sets in cases:
        t0 = time.time()
        w = make()
        tr = PCGNNTrainer(w, dict(engine="graph", batch_size=B, seed=0), dev)
        tr.run_epoch_one_graph()                            # (trained parameters; the engine as a training run leaves it)
        fz = tr.fused
        print(f"# {name}: built in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
        for which in sets:
            ids = np.arange(first, w.n)
            if which == "held_out":
                ids = ids[~np.isin(ids, w.idx_train)]
            else:
                ids = np.arange(w.n)
            ids_dev = torch.as_tensor(ids, dtype=torch.int32, device=dev)
            old_ms, old = timed(lambda: old_pass(fz, ids_dev, B), args.reps)
            new_ms, new = timed(lambda: new_pass(fz, ids_dev, B), args.reps)
            n = len(ids)
            print(json.dumps(dict(workload=name, set=which, n=n, batch=B, old_ms=round(old_ms, 4), new_ms=round(new_ms, 4),
                                  old_nodes_per_s=n / old_ms * 1e3, new_nodes_per_s=n / new_ms * 1e3,
                                  speedup=round(old_ms / new_ms, 3), bit_identical=bool(torch.equal(old, new)))), flush=True)
        del tr, fz
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
