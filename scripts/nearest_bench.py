"""Embeddings and nearest labelled examples: what FusedPCGNN.embed costs beside infer, and FusedPCGNN.nearest's search
(pcg_topk_similar) against the eager expression torch.topk(score(Q, bank), k) on the same embeddings.

    python scripts/nearest_bench.py [--reps 7] [--only yelp,powerlaw] [--k 8]

Per graph (yelp_like(0); power_law(2 M, 40 M)), every node of the graph as the query set, the graph's training positives as the
bank.  Timed as scripts/infer_new_bench.py times (its `wall`, imported): wall clock with a device synchronise at both ends, one
warm-up call, the median and the max - min of --reps passes (51 where a call takes under 5 ms).
    infer(ids) | embed(ids) | embed(ids, relations=True)   - the difference is the n*E (+ n*R*E) float stores; recorded, not
                                                              asserted
    topk_similar(Q, bank, k, metric) for cosine, dot, l2     - with its throughput against the two bounds of the kernel:
                                                              2 n M E flops (f32 MFMA), (n E + M E) * 4 bytes read once
    torch.topk(score(Q, bank), k)                            - only where the [n, M] matrix fits (--eager-max-bytes, default
                                                              8 GiB): the yelp-like graph
The script asserts that embed's logits are infer's bits and, where the eager expression runs, that both searches return the
same positions on rows without near-ties (a row whose eager k-th and (k+1)-th scores differ by less than 1e-5 of the row's
largest is not compared: the two paths round differently).  `faster_than_eager` is reported only as a comparison with the eager
path's own spread: true when eager - ours > eager's max - min.  One JSON line per (graph, measurement)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from infer_new_bench import engine_on, wall  # noqa: E402


def eager_scores(Q, bank, metric):
    dot = Q @ bank.t()
    if metric == "dot":
        return dot
    qn2, cn2 = (Q * Q).sum(1), (bank * bank).sum(1)
    if metric == "l2":
        return torch.clamp(2 * dot - qn2[:, None] - cn2[None, :], max=0)
    den = qn2.sqrt()[:, None] * cn2.sqrt()[None, :]
    return torch.where(den > 0, dot / den, torch.zeros_like(dot))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="yelp,powerlaw")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--eager-max-bytes", type=int, default=8 << 30)
    args = ap.parse_args()
    assert args.reps >= 5
    import pcgnn_amd  # noqa: F401
    from pcgnn_amd import ops, synth
    from pcgnn_amd.graph import DeviceGraph
    dev = torch.device("cuda", 0)
    only = args.only.split(",")
    cases = []
    if "yelp" in only:
        cases.append(("yelp", lambda: synth.yelp_like(0)))
    if "powerlaw" in only:
        cases.append(("powerlaw_2m", lambda: synth.power_law(2_000_000, 40_000_000, 0)))
    k = args.k
    for name, make in cases:
        w = make()
        g = DeviceGraph(w.X, w.csr, w.train_pos, dev)
        fz = engine_on(w, g, w.X, dev)
        n, E, R = w.n, fz.E, g.R
        i_ms, i_spread, logits = wall(lambda: fz.infer(None), args.reps)
        e_ms, e_spread, _ = wall(lambda: fz.embed(None), args.reps)
        el_ms, el_spread, out = wall(lambda: fz.embed(None, want_logits=True), args.reps)
        assert torch.equal(out[1].view(torch.int32), logits.view(torch.int32)), "embed's logits are not infer's"
        del out
        r_ms, r_spread, out = wall(lambda: fz.embed(None, relations=True), args.reps)
        del out
        print(json.dumps(dict(workload=name, what="embed_vs_infer", n=n, emb=E, n_rel=R, infer_ms=round(i_ms, 3),
                              infer_spread_ms=round(i_spread, 3), embed_ms=round(e_ms, 3), embed_spread_ms=round(e_spread, 3),
                              embed_logits_ms=round(el_ms, 3), embed_logits_spread_ms=round(el_spread, 3),
                              embed_relations_ms=round(r_ms, 3), embed_relations_spread_ms=round(r_spread, 3),
                              embed_over_infer=round(e_ms / i_ms, 4), embed_relations_over_infer=round(r_ms / i_ms, 4))), flush=True)
        Q = fz.embed(None)
        among = torch.as_tensor(np.asarray(w.train_pos), dtype=torch.int32, device=dev)
        bank = fz.embed(among)
        M = int(bank.shape[0])
        fits = 2 * 4 * n * M <= args.eager_max_bytes                     # (the scores and one temporary)
        for metric in ("cosine", "dot", "l2"):
            t_ms, t_spread, (pos, score) = wall(lambda: ops.topk_similar(Q, bank, k, metric), args.reps)
            rec = dict(workload=name, what="topk_similar", metric=metric, n=n, M=M, emb=E, k=k, ms=round(t_ms, 3),
                       spread_ms=round(t_spread, 3), tflops=round(2.0 * n * M * E / (t_ms * 1e-3) / 1e12, 3),
                       flop_bound="2 n M E", bytes_once=4 * (n + M) * E,
                       gbps_of_bytes_once=round(4.0 * (n + M) * E / (t_ms * 1e-3) / 1e9, 3))
            if fits:
                g_ms, g_spread, (ev, ei) = wall(lambda: torch.topk(eager_scores(Q, bank, metric), min(k + 1, M), dim=1), args.reps)
                if M > k:
                    clear = (ev[:, k - 1] - ev[:, k]) > 1e-5 * ev.abs().max(1).values.clamp(min=1e-30)
                    gaps = (ev[:, :k - 1] - ev[:, 1:k]) > 1e-5 * ev.abs().max(1).values.clamp(min=1e-30)[:, None]
                    clear = clear & gaps.all(1)
                    assert torch.equal(pos[clear].long(), ei[clear, :k]), f"{metric}: positions differ from torch.topk"
                    rec["rows_compared"] = int(clear.sum())
                rec.update(eager_ms=round(g_ms, 3), eager_spread_ms=round(g_spread, 3),
                           faster_than_eager=bool(g_ms - t_ms > g_spread))
                del ev, ei
            else:
                rec["eager"] = f"not run: the [n, M] matrix is {4 * n * M / 2 ** 30:.1f} GiB"
            print(json.dumps(rec), flush=True)
        n_ms, n_spread, _ = wall(lambda: fz.nearest(None, k=k), max(args.reps // 2, 5) if n > 500_000 else args.reps)
        print(json.dumps(dict(workload=name, what="nearest_whole_graph", n=n, M=M, k=k, ms=round(n_ms, 3),
                              spread_ms=round(n_spread, 3))), flush=True)
        del fz, g, Q, bank
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
