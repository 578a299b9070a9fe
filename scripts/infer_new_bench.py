"""Scoring unseen nodes: FusedPCGNN.infer_new against what a user had before it - rebuild the DeviceGraph with the new rows
appended, then FusedPCGNN.infer(ids) on the grown graph.

    python scripts/infer_new_bench.py [--reps 7] [--only yelp,powerlaw] [--sizes 1,256,4096,65536] [--one-warm NQ]

Per graph (yelp_like(0); power_law(2 M, 40 M)) and query size nq: the query nodes are generated behind the graph (random
features; ~the graph's mean degree of edges each, to random nodes of the whole id range, symmetrised, self-loops).  Timed, wall
clock with a device synchronise at both ends, one warm-up call, median of --reps passes (51 where a call takes under 5 ms):
    (a) infer(ids of the nq nodes) on the GROWN graph (+ `build_ms`: constructing the grown DeviceGraph, once)
    (b) infer_new cold (reuse_scores=False: the base table is scored)
    (c) infer_new warm (the cached base scores)
and, power-law only, (c) against a 200 K-node base graph with the same query degree profile.  The script asserts that (a),
(b) and (c) return identical bits, then checks
    (c) <= (a);   (b) <= (a) + spread(a)   [spread = (a)'s max - min over the passes];
    nq <= 4096 on the 2 M graph:  |(c) - (c on the 200 K base)| <= spread(a)
and prints one JSON line per (graph, nq) with the numbers and which conditions hold (a failed condition is reported, and the
exit status is 1 at the end).  --one-warm NQ: nothing but one cold and then ONE warm infer_new call, for a kernel trace
(rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o y -- python scripts/infer_new_bench.py --only yelp --one-warm 256);
--trace-summary DIR/.../y_kernel_trace.csv then lists the warm call's kernels and their sum."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def grow(w, nq, seed, avg_deg):
    """(X_full, csrs_full): the workload's graph + nq generated nodes behind it (the generators' recipe)"""
    from pcgnn_amd.synth import _csr_from_pairs
    rs = np.random.RandomState(seed)
    n = w.n
    nf = n + nq
    Xf = np.concatenate([w.X, rs.randn(nq, w.X.shape[1]).astype(np.float32)])
    out = []
    for (indptr, idx), deg in zip(w.csr, avg_deg):
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
        m = max(int(nq * deg), 1)
        src = rs.randint(n, nf, size=m).astype(np.int64)
        dst = rs.randint(0, nf, size=m).astype(np.int64)
        out.append(_csr_from_pairs(nf, np.concatenate([rows, src]), np.concatenate([idx.astype(np.int64), dst])))
    return Xf, out


def query_rows(Xf, full_csr, N):
    return Xf[N:], [(ip[N:] - ip[N], ix[ip[N]:]) for ip, ix in full_csr]


FAST_MS, FAST_REPS = 5.0, 51


def wall(fn, reps):
    """median and max - min (ms) of `reps` synchronised wall-clock passes after a warm-up; a call that takes under FAST_MS is
    host-noise sized, so it gets FAST_REPS passes instead"""
    fn()                                                   # warm-up (workspaces, kernel attributes, uploads)
    ms = []
    out = None
    while len(ms) < reps:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        if len(ms) == reps and reps < FAST_REPS and float(np.median(ms)) < FAST_MS:
            reps = FAST_REPS
    return float(np.median(ms)), float(max(ms) - min(ms)), out


def engine_on(w, graph, X, dev, theta=None):
    """a FusedPCGNN over `graph` with the workload's model shape (and the given parameters)"""
    import torch.nn as nn
    from pcgnn_amd.fused import FusedPCGNN
    from pcgnn_amd.layers import InterAgg, IntraAgg
    from pcgnn_amd.model import PCALayer
    f = graph.feat_dim
    torch.manual_seed(0)
    feats = nn.Embedding(X.shape[0], f)
    feats.weight = nn.Parameter(torch.from_numpy(X), requires_grad=False)
    intras = [IntraAgg(feats, f, 64, w.train_pos, 0.5, cuda=True) for _ in w.csr]
    inter = InterAgg(feats, f, 64, w.train_pos, graph, intras, cuda=True)
    fz = FusedPCGNN(PCALayer(2, inter, 2.0).to(dev), 0.01, 0.001, max_batch=256)
    if theta is not None:
        fz.theta.copy_(theta)
        fz.params_changed()
    return fz


def summarise_trace(path):
    """the kernels of the WARM call from the kernel trace (csv) of a --one-warm run: that run makes two identical calls (cold,
    then warm), so the warm call's launches are the second half of the trace's pcg:: kernels, in start order"""
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "pcg::" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert rows and len(rows) % 2 == 0, f"{len(rows)} pcg:: launches: not two identical calls"
    warm = rows[len(rows) // 2:]
    total = 0
    for r in warm:
        ns = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        total += ns
        print(f"{ns / 1e3:9.2f} us  {r['Kernel_Name'][:100]}")
    span = int(warm[-1]["End_Timestamp"]) - int(warm[0]["Start_Timestamp"])
    print(f"{total / 1e3:9.2f} us  sum of the warm call's {len(warm)} kernels;  {span / 1e3:.2f} us from the first one's start to the last one's end")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-summary", default=None, help="a *_kernel_trace.csv of a --one-warm run: print the warm call's kernels")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="yelp,powerlaw")
    ap.add_argument("--sizes", default="1,256,4096,65536")
    ap.add_argument("--one-warm", type=int, default=0)
    args = ap.parse_args()
    if args.trace_summary:
        summarise_trace(args.trace_summary)
        return 0
    assert args.reps >= 5
    import pcgnn_amd  # noqa: F401
    from pcgnn_amd import synth
    from pcgnn_amd.graph import DeviceGraph, QueryBatch
    dev = torch.device("cuda", 0)
    sizes = [int(s) for s in args.sizes.split(",")]
    only = args.only.split(",")
    cases = []
    if "yelp" in only:
        cases.append(("yelp", lambda: synth.yelp_like(0), None))
    if "powerlaw" in only:
        cases.append(("powerlaw_2m", lambda: synth.power_law(2_000_000, 40_000_000, 0), lambda: synth.power_law(200_000, 4_000_000, 0)))
    failed = False
    for name, make, make_small in cases:
        w = make()
        N = w.n
        avg_deg = [float(np.diff(ip).mean()) / 2 for ip, _ in w.csr]        # (each generated edge is stored twice)
        base_graph = DeviceGraph(w.X, w.csr, w.train_pos, dev)
        base = engine_on(w, base_graph, w.X, dev)
        small = None
        if make_small is not None and not args.one_warm:
            ws = make_small()
            small = engine_on(ws, DeviceGraph(ws.X, ws.csr, ws.train_pos, dev), ws.X, dev, base.theta)
        print(f"# {name}: N {N}, mean degrees {[round(2 * d, 1) for d in avg_deg]}", file=sys.stderr, flush=True)
        if args.one_warm:
            Xf, full_csr = grow(w, args.one_warm, 1, avg_deg)
            q = QueryBatch(*query_rows(Xf, full_csr, N), base_graph).to(dev, base_graph)
            base.infer_new(q, reuse_scores=False)
            base.infer_new(q)
            assert not base._new_scored_base
            torch.cuda.synchronize()
            return 0
        for nq in sizes:
            Xf, full_csr = grow(w, nq, nq, avg_deg)
            Xq, q_pairs = query_rows(Xf, full_csr, N)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            full_graph = DeviceGraph(Xf, full_csr, w.train_pos, dev)        # what a user had to do first, every time
            torch.cuda.synchronize()
            build_ms = (time.perf_counter() - t0) * 1e3
            full = engine_on(w, full_graph, Xf, dev, base.theta)
            ids = torch.arange(N, N + nq, dtype=torch.int32, device=dev)
            q = QueryBatch(Xq, q_pairs, base_graph).to(dev, base_graph)
            a_ms, a_spread, a_out = wall(lambda: full.infer(ids), args.reps)
            b_ms, _, b_out = wall(lambda: base.infer_new(q, reuse_scores=False), args.reps)
            c_ms, _, c_out = wall(lambda: base.infer_new(q), args.reps)
            assert not base._new_scored_base
            assert torch.equal(a_out, b_out) and torch.equal(a_out, c_out), "infer_new differs from infer on the grown graph"
            rec = dict(workload=name, n_base=N, nq=nq, build_ms=round(build_ms, 3), infer_full_ms=round(a_ms, 4),
                       infer_full_spread_ms=round(a_spread, 4), infer_new_cold_ms=round(b_ms, 4), infer_new_warm_ms=round(c_ms, 4),
                       bit_identical=True, warm_le_full=c_ms <= a_ms, cold_le_full_plus_spread=b_ms <= a_ms + a_spread)
            if small is not None and nq <= 4096:
                # the same query rows against a 200 K base: neighbour ids folded into its id range (degrees unchanged up to the
                # few duplicates the fold creates)
                Ns = small.g.n_nodes
                pairs_s = [(ip, np.where(ix >= N, ix - N + Ns, ix % Ns)) for ip, ix in q_pairs]
                qs = QueryBatch(Xq, pairs_s, small.g).to(dev, small.g)
                s_ms, _, _ = wall(lambda: small.infer_new(qs), args.reps)
                rec.update(infer_new_warm_200k_ms=round(s_ms, 4), warm_flat_in_n=abs(c_ms - s_ms) <= a_spread)
            failed = failed or not all(v for k, v in rec.items() if isinstance(v, bool))
            print(json.dumps(rec), flush=True)
            del full, full_graph, q
            torch.cuda.empty_cache()
        del base, base_graph, small
        torch.cuda.empty_cache()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
