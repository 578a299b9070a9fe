"""Event-timed training of the GraphSAGE / GCN baselines: the autograd loop (``model.loss`` -> backward -> torch.optim.Adam per
batch, what ModelHandler runs by default) against ``BaselineEngine.train_epoch`` / ``train_step`` (pcg_baseline_train), on the same
graph, the same ids and the same starting weights.

    python scripts/baseline_train_bench.py [--reps 5] [--only yelp,powerlaw]

Workloads: yelp_like(0) as a homo graph (the union of its relations) at batch 1024, E = 64; a power-law graph of 2 M nodes / 40 M
edges built as ONE relation at batch 4096.  Models: SAGE and GCN as ModelHandler builds them.  One epoch is the workload's
idx_train in one seeded shuffle (the last batch partial), one step its first full batch.  One JSON line per (workload, model): ms
per epoch and per step as the median of --reps after one warm-up each, with max - min, both ways; whether the gap exceeds the
old path's own max - min; and the largest difference between the two paths' weights after the timed epochs' first one (the same
steps, float32 apart)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.baseline_infer_bench import build, homo_union      # noqa: E402

LR, WD = 0.01, 0.001


def timed(fn, reps):
    fn()                                                   # warm-up (workspaces, kernel attributes, rocBLAS)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(max(ms) - min(ms))


def autograd_epoch(model, opt, ids_host, labels_dev, batch):
    for b0 in range(0, len(ids_host), batch):
        nodes = ids_host[b0:b0 + batch]
        opt.zero_grad()
        loss = model.loss(nodes, labels_dev[torch.as_tensor(nodes, device=labels_dev.device)].long())
        loss.backward()
        opt.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="yelp,powerlaw")
    ap.add_argument("--emb", type=int, default=64)
    args = ap.parse_args()
    import pcgnn_amd as P
    from pcgnn_amd import graphsage as GS, synth
    dev = torch.device("cuda", 0)
    cases = []
    only = args.only.split(",")
    if "yelp" in only:
        cases.append(("yelp_homo", lambda: synth.yelp_like(0), 1024))
    if "powerlaw" in only:
        cases.append(("powerlaw_2m_homo", lambda: synth.make_workload("powerlaw-2m-homo", 2_000_000, 32, [40_000_000], 0.01, 0, 1.1,
                                                                      max_share=1e-4), 4096))
    for name, make, batch in cases:
        t0 = time.time()
        w = make()
        csr = homo_union(w.n, w.csr)
        g = P.DeviceGraph(w.X, [csr], [], dev)
        print(f"# {name}: {w.n} nodes, {int(csr[1].shape[0])} CSR entries, max degree {g.max_degree}, built in {time.time() - t0:.1f} s",
              file=sys.stderr, flush=True)
        labels_dev = torch.from_numpy(np.asarray(w.labels).astype(np.int32)).to(dev)
        ids_host = [int(v) for v in np.random.RandomState(0).permutation(np.asarray(w.idx_train))]
        ids_dev = torch.as_tensor(ids_host, dtype=torch.int32, device=dev)
        lab_ids = labels_dev[ids_dev.long()]
        n = len(ids_host)
        for mname in ("SAGE", "GCN"):
            old, new = build(GS, mname, g, g.feat_dim, args.emb), build(GS, mname, g, g.feat_dim, args.emb)
            opt = torch.optim.Adam(old.parameters(), lr=LR, weight_decay=WD)
            new.configure_optimizer(LR, WD)
            # the same steps on both sides first: one epoch each from the same weights
            autograd_epoch(old, opt, ids_host, labels_dev, batch)
            new.train_epoch(ids_dev, lab_ids, batch)
            new.check()
            diff = max(float((a.detach() - b.detach()).abs().max()) for a, b in ((old.enc.weight, new.enc.weight), (old.weight, new.weight)))
            old_ms, old_spread = timed(lambda: autograd_epoch(old, opt, ids_host, labels_dev, batch), args.reps)
            new_ms, new_spread = timed(lambda: new.train_epoch(ids_dev, lab_ids, batch), args.reps)
            old_step, old_step_spread = timed(lambda: autograd_epoch(old, opt, ids_host[:batch], labels_dev, batch), args.reps)
            new_step, new_step_spread = timed(lambda: new.train_step(ids_dev[:batch], lab_ids[:batch]), args.reps)
            new.check()
            row = dict(workload=name, model=mname, n_train=n, batch=batch, emb=args.emb, n_batches=(n + batch - 1) // batch,
                       autograd_epoch_ms=round(old_ms, 4), autograd_epoch_max_minus_min=round(old_spread, 4),
                       train_epoch_ms=round(new_ms, 4), train_epoch_max_minus_min=round(new_spread, 4),
                       epoch_speedup=round(old_ms / new_ms, 3), epoch_gap_exceeds_autograd_spread=bool(old_ms - new_ms > old_spread),
                       autograd_step_ms=round(old_step, 4), autograd_step_max_minus_min=round(old_step_spread, 4),
                       train_step_ms=round(new_step, 4), train_step_max_minus_min=round(new_step_spread, 4),
                       step_speedup=round(old_step / new_step, 3), step_gap_exceeds_autograd_spread=bool(old_step - new_step > old_step_spread),
                       max_abs_weight_diff_after_one_epoch=diff)
            print(json.dumps(row), flush=True)
            del old, new, opt
        del g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
