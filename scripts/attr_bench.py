"""Event-timed attribution passes: one FusedPCGNN.infer call (the closest operation the engine had before ``attribute``) against
``attribute`` and ``attribute(neighbours=True)`` on the same engine and the same ids, and pcg_attr_neighbours on its own
(``ops.neighbour_contrib`` over the lists and d_agg of the pass before) with its algorithmic bytes per second: entries x (row
bytes + 8: the id read and the value written) + d_agg.

    python scripts/attr_bench.py [--reps 5] [--only yelp,amazon,powerlaw]

Sets: yelp_like(0) held-out ids and the whole graph; amazon_like(0) held-out ids; power_law(2 M, 40 M) whole graph.  One JSON
line per set: ms per pass (median of --reps, after one warm-up pass each)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
    ap.add_argument("--only", default="yelp,amazon,powerlaw")
    args = ap.parse_args()
    import pcgnn_amd  # noqa: F401
    from pcgnn_amd import ops, synth
    from pcgnn_amd.handler import PCGNNTrainer
    dev = torch.device("cuda", 0)
    cases = []
    only = args.only.split(",")
    if "yelp" in only:
        cases.append(("yelp", lambda: synth.yelp_like(0), 1024, 0, ["held_out", "whole"]))
    if "amazon" in only:
        cases.append(("amazon", lambda: synth.amazon_like(0), 256, 3305, ["held_out"]))
    if "powerlaw" in only:
        cases.append(("powerlaw_2m", lambda: synth.power_law(2_000_000, 40_000_000, 0), 4096, 0, ["whole"]))
    for name, make, B, first, sets in cases:
        t0 = time.time()
        w = make()
        tr = PCGNNTrainer(w, dict(engine="graph", batch_size=B, seed=0), dev)
        tr.run_epoch_one_graph()                            # (trained parameters; the engine as a training run leaves it)
        fz = tr.fused
        print(f"# {name}: built in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
        for which in sets:
            ids = np.arange(first, w.n)
            ids = ids[~np.isin(ids, w.idx_train)] if which == "held_out" else np.arange(w.n)
            ids_dev = torch.as_tensor(ids, dtype=torch.int32, device=dev)
            infer_ms, logits = timed(lambda: fz.infer(ids_dev), args.reps)
            attr_ms, res = timed(lambda: fz.attribute(ids_dev), args.reps)
            chosen_ms, _ = timed(lambda: fz.chosen(ids_dev), args.reps)
            full_ms, full = timed(lambda: fz.attribute(ids_dev, neighbours=True), args.reps)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            out = torch.empty_like(full.neigh_contrib)
            neigh_ms, _ = timed(lambda: ops.neighbour_contrib(fz.g, full.chosen, full.d_agg, status=status, out=out), args.reps)
            entries, n = int(full.chosen.ids.numel()), len(ids)
            nbytes = entries * (4 * fz.g.feat_stride + 8) + 4 * full.d_agg.numel()
            resid = full.completeness_residual()
            finite = torch.isfinite(resid)
            print(json.dumps(dict(workload=name, set=which, n=n, entries=entries, infer_ms=round(infer_ms, 4), attribute_ms=round(attr_ms, 4),
                                  attribute_over_infer=round(attr_ms / infer_ms, 3), chosen_ms=round(chosen_ms, 4),
                                  attribute_neighbours_ms=round(full_ms, 4), neigh_kernel_ms=round(neigh_ms, 4),
                                  neigh_gbytes_per_s=round(nbytes / neigh_ms / 1e6, 1),
                                  logits_bit_identical=bool(torch.equal(res.logits.view(torch.int32), logits.view(torch.int32))),
                                  neigh_bit_identical=bool(torch.equal(out.view(torch.int32), full.neigh_contrib.view(torch.int32))), status=int(status.item()),
                                  max_abs_residual=float(resid[finite].abs().max()), nan_rows=int((~finite).sum()))), flush=True)
            del res, full, out
        del tr, fz
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
