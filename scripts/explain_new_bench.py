"""Explaining unseen nodes: FusedPCGNN.attribute_new(neighbours=True) against what a user had before it - rebuild the DeviceGraph
with the new rows appended, then FusedPCGNN.attribute(ids, neighbours=True) on the grown graph.

    python scripts/explain_new_bench.py [--reps 7] [--only yelp,powerlaw] [--sizes 1,256,4096] [--one-warm NQ]

Per graph (yelp_like(0); power_law(2 M, 40 M)) and query size nq the query nodes are generated behind the graph as
scripts/infer_new_bench.py generates them (its helpers are imported).  Timed, wall clock with a device synchronise at both ends,
one warm-up call, median of --reps passes (51 where a call takes under 5 ms: infer_new_bench.py's `wall`, imported):
    (a) attribute(ids of the nq nodes, neighbours=True) on the GROWN graph (+ `build_ms`: constructing the grown DeviceGraph, once -
        its own column, not part of (a))
    (b) attribute_new(neighbours=True) cold (reuse_scores=False: the base table is scored)
    (c) attribute_new(neighbours=True) warm (the cached base scores)
    (d) infer_new warm, for scale
The script asserts that (a), (b) and (c) return identical bits (logits, d_self, d_agg, self_contrib, rel_contrib, the lists'
offsets, ids and distances, neigh_contrib), then checks
    (a) - (c) > spread(a)   [spread = (a)'s max - min over the passes];   (b) <= (a) + spread(a)
and prints one JSON line per (graph, nq) with the numbers and which conditions hold (a failed condition is reported, and the exit
status is 1 at the end).  --one-warm NQ: nothing but one cold and then ONE warm attribute_new(neighbours=True) call, for a kernel
trace (rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o y -- python scripts/explain_new_bench.py --only yelp
--one-warm 256); `python scripts/infer_new_bench.py --trace-summary DIR/.../y_kernel_trace.csv` lists the warm call's kernels."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from infer_new_bench import engine_on, grow, query_rows, wall  # noqa: E402

KEYS = ("logits", "d_self", "d_agg", "self_contrib", "rel_contrib", "neigh_contrib")


def same_bits(a, b):
    view = lambda t: t.contiguous().view(torch.int32)
    return (all(torch.equal(view(getattr(a, k)), view(getattr(b, k))) for k in KEYS)
            and torch.equal(a.chosen.flat_offsets, b.chosen.flat_offsets) and torch.equal(a.chosen.ids, b.chosen.ids)
            and torch.equal(view(a.chosen.dist), view(b.chosen.dist)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="yelp,powerlaw")
    ap.add_argument("--sizes", default="1,256,4096")
    ap.add_argument("--one-warm", type=int, default=0)
    args = ap.parse_args()
    assert args.reps >= 5
    import pcgnn_amd  # noqa: F401
    from pcgnn_amd import synth
    from pcgnn_amd.graph import DeviceGraph, QueryBatch
    dev = torch.device("cuda", 0)
    sizes = [int(s) for s in args.sizes.split(",")]
    only = args.only.split(",")
    cases = []
    if "yelp" in only:
        cases.append(("yelp", lambda: synth.yelp_like(0)))
    if "powerlaw" in only:
        cases.append(("powerlaw_2m", lambda: synth.power_law(2_000_000, 40_000_000, 0)))
    failed = False
    for name, make in cases:
        w = make()
        N = w.n
        avg_deg = [float(np.diff(ip).mean()) / 2 for ip, _ in w.csr]        # (each generated edge is stored twice)
        base_graph = DeviceGraph(w.X, w.csr, w.train_pos, dev)
        base = engine_on(w, base_graph, w.X, dev)
        print(f"# {name}: N {N}, mean degrees {[round(2 * d, 1) for d in avg_deg]}", file=sys.stderr, flush=True)
        if args.one_warm:
            Xf, full_csr = grow(w, args.one_warm, 1, avg_deg)
            q = QueryBatch(*query_rows(Xf, full_csr, N), base_graph).to(dev, base_graph)
            base.attribute_new(q, neighbours=True, reuse_scores=False)
            base.attribute_new(q, neighbours=True)
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
            a_ms, a_spread, a_out = wall(lambda: full.attribute(ids, neighbours=True), args.reps)
            b_ms, b_spread, b_out = wall(lambda: base.attribute_new(q, neighbours=True, reuse_scores=False), args.reps)
            assert base._new_scored_base
            c_ms, c_spread, c_out = wall(lambda: base.attribute_new(q, neighbours=True), args.reps)
            assert not base._new_scored_base
            d_ms, _, d_out = wall(lambda: base.infer_new(q), args.reps)
            assert same_bits(a_out, b_out) and same_bits(a_out, c_out), "attribute_new differs from attribute on the grown graph"
            assert torch.equal(d_out.view(torch.int32), c_out.logits.view(torch.int32)), "attribute_new's logits are not infer_new's"
            rec = dict(workload=name, n_base=N, nq=nq, list_entries=int(a_out.chosen.ids.numel()), build_ms=round(build_ms, 3),
                       attribute_full_ms=round(a_ms, 4), attribute_full_spread_ms=round(a_spread, 4),
                       attribute_new_cold_ms=round(b_ms, 4), attribute_new_cold_spread_ms=round(b_spread, 4),
                       attribute_new_warm_ms=round(c_ms, 4), attribute_new_warm_spread_ms=round(c_spread, 4),
                       infer_new_warm_ms=round(d_ms, 4),
                       bit_identical=True, warm_below_full_by_more_than_spread=a_ms - c_ms > a_spread,
                       cold_le_full_plus_spread=b_ms <= a_ms + a_spread)
            failed = failed or not all(v for k, v in rec.items() if isinstance(v, bool))
            print(json.dumps(rec), flush=True)
            del full, full_graph, q, a_out, b_out, c_out
            torch.cuda.empty_cache()
        del base, base_graph
        torch.cuda.empty_cache()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
