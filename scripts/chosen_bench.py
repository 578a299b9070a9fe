"""Wall-clock selection reports: what a user had before FusedPCGNN.chosen existed against one FusedPCGNN.chosen call, on the
same engine and the same ids, producing the same arrays.

    python scripts/chosen_bench.py [--reps 7] [--only yelp,powerlaw]

(a) old: the ops.chosen_sets / read_batch_lists way, batch by batch at the bench batch size - one score pass, then per batch a
    test-mode select into a workspace, the batch's offsets / lengths / list copied to the host, and there the distances
    (float32 |c - s|) and a stable sort of every ranked row into the (offsets, ids, dist) arrays.  The host part is vectorised
    numpy (one lexsort per batch), not the helpers' per-row Python sets: the strongest form of what was possible.  Its result is
    on the host.
(b) new: FusedPCGNN.chosen(ids).  Its result is on the device; ``new_to_host_ms`` adds the copy of ids and dist to the host.
Sets: yelp_like(0) held-out ids and whole graph; power_law(2 M, 40 M) whole graph.  Wall clock (time.perf_counter), synchronised
at both ends, one warm-up pass each, --reps timed passes (default 7): median, min, max.  The two results are compared inside the
script (np.array_equal on offsets, ids and the distances' bits) and the script asserts (b) <= (a) by more than (a)'s own
max - min.  One JSON line per set."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def old_pass(fz, ids, B):
    """-> (flat offsets [R * n + 1], ids int32, dist float32) on the host"""
    from pcgnn_amd import ops
    g, dev = fz.g, fz.dev
    R, n = g.R, len(ids)
    thr = fz.thresholds
    fz.flush()
    s0 = ops.score_table(g, fz.w_clf, fz.b_clf)
    s0h = s0.cpu().numpy()
    caps = ops.sel_capacity(g, ids, None, thr, 0.0, False)                      # [R, n]
    off = ops.rank_offsets(caps)
    out_ids = np.empty(int(off[-1]), dtype=np.int32)
    out_dist = np.empty(int(off[-1]), dtype=np.float32)
    deg = np.stack([g.deg_host[r][ids] for r in range(R)]).astype(np.int64)
    ranked = deg > np.ceil(deg * np.asarray(thr, dtype=np.float64)[:, None]).astype(np.int64) + 1
    ids_dev = torch.as_tensor(ids, dtype=torch.int32, device=dev)
    cap_max = max(int(caps[:, s:s + B].sum()) for s in range(0, n, B))
    wss = {}
    for s in range(0, n, B):
        b = min(B, n - s)
        ws = wss.get(b)
        if ws is None:
            ws = wss[b] = (ops.ChooseWorkspace(g, b, list_capacity=max(cap_max, 1)), torch.empty(R * b, dtype=torch.int32, device=dev))
        ws, cnt = ws
        ops.choose_select(g, ids_dev[s:s + b], None, s0, None, thr, 0.0, False, ws, cnt)
        rows = R * b
        torch.cuda.synchronize(dev)
        ws.check()
        begin = ws.view(0, torch.int64, rows + 1).cpu().numpy()
        length = ws.view(1, torch.int32, rows).cpu().numpy().astype(np.int64)
        lst = ws.view(2, torch.int32, max(int(begin[-1]), 1)).cpu().numpy()[:int(begin[-1])]
        assert np.array_equal(length, caps[:, s:s + b].reshape(-1)) and np.array_equal(np.diff(begin), length)
        row_of = np.repeat(np.arange(rows), length)
        cen = np.tile(s0h[ids[s:s + b]], R)
        dist = np.abs(cen[row_of] - s0h[lst]).astype(np.float32)
        key = np.where(ranked[:, s:s + b].reshape(-1)[row_of], dist, np.float32(0))    # keep-all rows stay in list order
        order = np.lexsort((key, row_of))                                        # stable: ties by list position
        for r in range(R):                                                       # relation r of the batch: contiguous both sides
            lo, hi = int(begin[r * b]), int(begin[(r + 1) * b])
            o = int(off[r * n + s])
            out_ids[o:o + hi - lo] = lst[order[lo:hi]]
            out_dist[o:o + hi - lo] = dist[order[lo:hi]]
    return off, out_ids, out_dist


def timed(fn, reps, dev):
    fn()                                                   # warm-up (workspaces, kernel attributes)
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="yelp,powerlaw")
    args = ap.parse_args()
    import pcgnn_amd  # noqa: F401
    from pcgnn_amd import synth
    from pcgnn_amd.handler import PCGNNTrainer
    dev = torch.device("cuda", 0)
    cases = []
    only = args.only.split(",")
    if "yelp" in only:
        cases.append(("yelp", lambda: synth.yelp_like(0), 1024, ["held_out", "whole"]))
    if "powerlaw" in only:
        cases.append(("powerlaw_2m", lambda: synth.power_law(2_000_000, 40_000_000, 0), 4096, ["whole"]))
    for name, make, B, sets in cases:
        t0 = time.time()
        w = make()
        tr = PCGNNTrainer(w, dict(engine="graph", batch_size=B, seed=0), dev)
        tr.run_epoch_one_graph()                            # (trained parameters; the engine as a training run leaves it)
        fz = tr.fused
        print(f"# {name}: built in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
        for which in sets:
            ids = np.arange(w.n)
            if which == "held_out":
                ids = ids[~np.isin(ids, w.idx_train)]
            old_ms, old = timed(lambda: old_pass(fz, ids, B), args.reps, dev)
            new_ms, new = timed(lambda: fz.chosen(ids), args.reps, dev)
            host_ms, _ = timed(lambda: (lambda c: (c.ids.cpu(), c.dist.cpu()))(fz.chosen(ids)), args.reps, dev)
            same = (np.array_equal(old[0], new.host_offsets()) and np.array_equal(old[1], new.ids.cpu().numpy())
                    and np.array_equal(old[2].view(np.uint32), new.dist.cpu().numpy().view(np.uint32)))
            spread = max(old_ms) - min(old_ms)
            res = dict(workload=name, set=which, n=len(ids), entries=int(old[0][-1]), batch=B, reps=args.reps,
                       old_ms=round(float(np.median(old_ms)), 3), old_min=round(min(old_ms), 3), old_max=round(max(old_ms), 3),
                       new_ms=round(float(np.median(new_ms)), 3), new_min=round(min(new_ms), 3), new_max=round(max(new_ms), 3),
                       new_to_host_ms=round(float(np.median(host_ms)), 3), old_spread_ms=round(spread, 3),
                       speedup=round(float(np.median(old_ms) / np.median(new_ms)), 2), identical=bool(same))
            print(json.dumps(res), flush=True)
            assert same, "the two ways disagree"
            assert np.median(new_ms) <= np.median(old_ms) - spread, "chosen() is not faster than the per-batch way beyond its spread"
        del tr, fz
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
