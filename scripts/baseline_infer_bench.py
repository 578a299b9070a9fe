"""Event-timed evaluation passes of the GraphSAGE / GCN baselines: the per-batch ``to_prob`` loop at batch 1024 (what
utils.predict_proba runs by default) against one ``infer`` call (baseline.BaselineEngine), on the same model and the same ids.

    python scripts/baseline_infer_bench.py [--reps 5] [--only yelp,powerlaw] [--infer-only]

Sets: yelp_like(0) as a homo graph (the union of its relations) - held-out ids (the labelled ids not in idx_train) and the whole
graph; a power-law graph of 2 M nodes / 40 M edges built as ONE relation - whole graph.  Models: SAGE and GCN as ModelHandler
builds them.  One JSON line per (set, model): ms per pass as the median of --reps after one warm-up pass each, with max - min,
both ways, and the largest probability difference between the two.  For the 2 M graph also the aggregate's algorithmic bytes
(edges x feat_stride x 4, plus the CSR: 8 bytes per indptr entry read twice, 4 per index) over the time of the whole ``infer``
call, as a fraction of the 8 TB/s HBM peak - a floor for the aggregate's own share, whose kernel time is in a kernel trace
(--infer-only runs nothing but ``infer`` calls: the run to put under ``rocprofv3 --kernel-trace --stats``)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8e12
BATCH = 1024


def homo_union(n, csrs):
    """the union graph of the relations, as the reference's homo pickle holds it (handler.py does the same)"""
    if len(csrs) == 1:
        return csrs[0]
    keys = np.unique(np.concatenate([np.repeat(np.arange(n, dtype=np.int64), np.diff(ip)) * n + ix for ip, ix in csrs]))
    rows = keys // n
    hp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=hp[1:])
    return hp, (keys - rows * n).astype(np.int32)


def build(GS, name, graph, F, E):
    torch.manual_seed(0)
    if name == "SAGE":
        enc = GS.Encoder(None, F, E, graph, GS.MeanAggregator(None, cuda=True), gcn=True, cuda=True)
        return GS.GraphSage(2, enc).to(graph.device)
    enc = GS.GCNEncoder(None, F, E, graph, GS.GCNAggregator(None, cuda=True), cuda=True)
    return GS.GCN(2, enc).to(graph.device)


def loop_pass(model, ids_host):
    with torch.no_grad():
        return torch.cat([model.to_prob(ids_host[s:s + BATCH].tolist(), None, train_flag=False)[0]
                          for s in range(0, len(ids_host), BATCH)])


def infer_pass(model, ids_dev):
    with torch.no_grad():
        return torch.sigmoid(model.infer(ids_dev))


def timed(fn, reps):
    fn()                                                   # warm-up (workspaces, kernel attributes, rocBLAS)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(max(ms) - min(ms)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="yelp,powerlaw")
    ap.add_argument("--emb", type=int, default=64)
    ap.add_argument("--infer-only", action="store_true", help="only the infer calls (for a kernel trace)")
    args = ap.parse_args()
    import pcgnn_amd as P
    from pcgnn_amd import graphsage as GS, synth
    dev = torch.device("cuda", 0)
    cases = []
    only = args.only.split(",")
    if "yelp" in only:
        cases.append(("yelp_homo", lambda: synth.yelp_like(0), ["held_out", "whole"]))
    if "powerlaw" in only:
        cases.append(("powerlaw_2m_homo", lambda: synth.make_workload("powerlaw-2m-homo", 2_000_000, 32, [40_000_000], 0.01, 0, 1.1,
                                                                      max_share=1e-4), ["whole"]))
    for name, make, sets in cases:
        t0 = time.time()
        w = make()
        csr = homo_union(w.n, w.csr)
        g = P.DeviceGraph(w.X, [csr], [], dev)
        edges = int(csr[1].shape[0])
        print(f"# {name}: {w.n} nodes, {edges} CSR entries, max degree {g.max_degree}, built in {time.time() - t0:.1f} s",
              file=sys.stderr, flush=True)
        for which in sets:
            ids = np.arange(w.n)
            if which == "held_out":
                ids = ids[~np.isin(ids, w.idx_train)]
            ids_dev = torch.as_tensor(ids, dtype=torch.int32, device=dev)
            n = len(ids)
            for mname in ("SAGE", "GCN"):
                model = build(GS, mname, g, g.feat_dim, args.emb)
                new_ms, new_spread, new = timed(lambda: infer_pass(model, ids_dev), args.reps)
                row = dict(workload=name, set=which, model=mname, n=n, emb=args.emb, infer_ms=round(new_ms, 4),
                           infer_max_minus_min=round(new_spread, 4), infer_nodes_per_s=n / new_ms * 1e3)
                if not args.infer_only:
                    old_ms, old_spread, old = timed(lambda: loop_pass(model, ids), args.reps)
                    row.update(batch=BATCH, loop_ms=round(old_ms, 4), loop_max_minus_min=round(old_spread, 4),
                               loop_nodes_per_s=n / old_ms * 1e3, speedup=round(old_ms / new_ms, 3),
                               gap_exceeds_loop_spread=bool(old_ms - new_ms > old_spread),
                               max_abs_prob_diff=float((old - new).abs().max()))
                if which == "whole":
                    nbytes = edges * g.feat_stride * 4 + edges * 4 + 2 * 8 * n
                    row.update(agg_algorithmic_bytes=nbytes, agg_bytes_over_infer_time_of_hbm_peak=nbytes / (new_ms * 1e-3) / HBM_PEAK)
                print(json.dumps(row), flush=True)
                del model
        del g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
