"""Event-timed partitioned inference at world size 1 over RCCL: DistributedPCGNN.infer against FusedPCGNN.infer on the same
graph, the same parameters and the same ids.  At world size 1 the halo is empty: what differs is the id translation of the
gather and the per-chunk exchange (a hash-table reset + two all-to-alls that are copies).

    python scripts/dist_infer_bench.py [--reps 5] [--only yelp,powerlaw]

Sets: yelp_like(0) held-out ids (labelled ids not in idx_train) and the whole graph; power_law(2 M, 40 M) whole graph.  One
JSON line per set: ms per pass (median of --reps after one warm-up pass each), the ratio and whether the logits are bitwise
equal.  N > 1 over RCCL is not measured here (no multi-GPU node); gloo rehearsals are correctness checks, not timings."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    fn()                                                   # warm-up (workspaces, plans, kernel attributes)
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
    ap.add_argument("--only", default="yelp,powerlaw")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29517")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    import pcgnn_amd  # noqa: F401
    from pcgnn_amd import synth
    from pcgnn_amd.dist import DistributedPCGNN
    from pcgnn_amd.handler import PCGNNTrainer
    only = args.only.split(",")
    cases = []
    if "yelp" in only:
        cases.append(("yelp", lambda: synth.yelp_like(0), 1024, ["held_out", "whole"]))
    if "powerlaw" in only:
        cases.append(("powerlaw_2m", lambda: synth.power_law(2_000_000, 40_000_000, 0), 4096, ["whole"]))
    try:
        for name, make, B, sets in cases:
            t0 = time.time()
            w = make()
            cfg = dict(emb_size=64, rho=0.5, alpha=2.0, lr=0.01, weight_decay=0.001, batch_size=B, seed=0)
            d = DistributedPCGNN(w, cfg, dev, window=2)
            ids = d.pick_epoch(2 * B, 0)
            d.train_window(ids, d.labels_of(ids))          # (moved parameters, an update pending)
            d.flush()
            fz = PCGNNTrainer(w, dict(engine="graph", batch_size=B, seed=0), dev).fused
            fz.theta.copy_(d.theta)
            fz.params_changed()
            print(f"# {name}: built in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
            for which in sets:
                if which == "held_out":
                    gid = np.arange(w.n)
                    gid = gid[~np.isin(gid, w.idx_train)]
                    local = gid                             # (world size 1: local rows are global ids)
                else:
                    gid, local = np.arange(w.n), None
                gid_dev = torch.as_tensor(gid, dtype=torch.int32, device=dev)
                loc_dev = None if local is None else torch.as_tensor(local, dtype=torch.int32, device=dev)
                f_ms, f_out = timed(lambda: fz.infer(gid_dev), args.reps)
                d_ms, d_out = timed(lambda: d.infer(loc_dev), args.reps)
                n = len(gid)
                print(json.dumps(dict(workload=name, set=which, n=n, fused_ms=round(f_ms, 4), dist_ms=round(d_ms, 4),
                                      ratio=round(d_ms / f_ms, 3), fused_nodes_per_s=n / f_ms * 1e3, dist_nodes_per_s=n / d_ms * 1e3,
                                      bit_identical=bool(torch.equal(f_out, d_out)))), flush=True)
            d.close()
            del d, fz
            torch.cuda.empty_cache()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
