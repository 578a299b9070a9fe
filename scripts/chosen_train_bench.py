"""Wall-clock train-mode selection reports: what a user had before FusedPCGNN.chosen(train_flag=True) existed against one such
call, on the same engine, the same ids and labels, producing the same arrays.

    python scripts/chosen_train_bench.py [--reps 7] [--only yelp,powerlaw]

(a) old: batch by batch at the bench batch size - one score pass and one sort of the train positives, then per batch a TRAIN-mode
    select into a workspace, the batch's offsets / lengths / list copied to the host (a row's kept neighbours are the head of
    its list), and there the neighbour distances (float32 |c - s|) and a stable sort of every ranked row; the sorted keys copied
    to the host once, and there per positive centre its window of the sorted train positives, their distances and a stable
    sort by (distance, position in train_pos).  The host part is vectorised numpy per batch and a short Python loop over the
    positive centres: the strongest form of what was possible.  Its result is on the host.
(b) new: FusedPCGNN.chosen(ids, labels=labels, train_flag=True).  Its result is on the device.
(c) FusedPCGNN.chosen(ids), test mode: (b) - (c) is what the minority part costs.
Sets: the train ids of yelp_like(0) and of power_law(2 M, 40 M).  Wall clock (time.perf_counter), synchronised at both ends,
one warm-up pass each, --reps timed passes (default 7): median, min, max.  (a) and (b) are compared inside the script
(np.array_equal on offsets, ids and the distances' bits, both parts) and the script asserts (b) <= (a) by more than (a)'s own
max - min.  One JSON line per set."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def from_orderable(k):
    k = k.astype(np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def old_pass(fz, ids, labels, B):
    """-> (flat offsets, ids, dist, minority flat offsets, ids, dist) on the host"""
    from pcgnn_amd import ops
    g, dev = fz.g, fz.dev
    R, n, P = g.R, len(ids), g.n_pos
    thr, rho = fz.thresholds, fz.rho
    fz.flush()
    s0 = ops.score_table(g, fz.w_clf, fz.b_clf)
    keys = ops.pos_sort(g, s0) if P else None
    s0h = s0.cpu().numpy()
    kept = ops.sel_capacity(g, ids, None, thr, 0.0, False)                      # [R, n]: the neighbour part
    minor = ops.minority_counts(g, ids, labels, thr, rho)                       # [R, n]
    caps = kept + minor
    off, moff = ops.rank_offsets(kept), ops.rank_offsets(minor)
    out_ids = np.empty(int(off[-1]), dtype=np.int32)
    out_dist = np.empty(int(off[-1]), dtype=np.float32)
    deg = np.stack([g.deg_host[r][ids] for r in range(R)]).astype(np.int64)
    ranked = deg > np.ceil(deg * np.asarray(thr, dtype=np.float64)[:, None]).astype(np.int64) + 1
    ids_dev = torch.as_tensor(ids, dtype=torch.int32, device=dev)
    lab_dev = torch.as_tensor(labels, dtype=torch.int32, device=dev)
    cap_max = max(int(caps[:, s:s + B].sum()) for s in range(0, n, B))
    wss = {}
    for s in range(0, n, B):
        b = min(B, n - s)
        ws = wss.get(b)
        if ws is None:
            ws = wss[b] = (ops.ChooseWorkspace(g, b, list_capacity=max(cap_max, 1)), torch.empty(R * b, dtype=torch.int32, device=dev))
        ws, cnt = ws
        ops.choose_select(g, ids_dev[s:s + b], lab_dev[s:s + b], s0, keys, thr, rho, True, ws, cnt)
        rows = R * b
        torch.cuda.synchronize(dev)
        ws.check()
        begin = ws.view(0, torch.int64, rows + 1).cpu().numpy()
        lst = ws.view(2, torch.int32, max(int(begin[-1]), 1)).cpu().numpy()
        length = kept[:, s:s + b].reshape(-1)                                    # the head of a row's list: its kept neighbours
        start = np.zeros(rows + 1, dtype=np.int64)
        np.cumsum(length, out=start[1:])
        row_of = np.repeat(np.arange(rows), length)
        ent = lst[begin[row_of] + (np.arange(int(start[-1])) - start[row_of])]
        cen = np.tile(s0h[ids[s:s + b]], R)
        dist = np.abs(cen[row_of] - s0h[ent]).astype(np.float32)
        key = np.where(ranked[:, s:s + b].reshape(-1)[row_of], dist, np.float32(0))    # keep-all rows stay in list order
        order = np.lexsort((key, row_of))                                        # stable: ties by list position
        for r in range(R):
            lo, hi = int(start[r * b]), int(start[(r + 1) * b])
            o = int(off[r * n + s])
            out_ids[o:o + hi - lo] = ent[order[lo:hi]]
            out_dist[o:o + hi - lo] = dist[order[lo:hi]]
    # the minority part: per positive centre its window of the sorted train positives
    m_ids = np.empty(int(moff[-1]), dtype=np.int32)
    m_dist = np.empty(int(moff[-1]), dtype=np.float32)
    if P and int(moff[-1]):
        kh = keys[:P].cpu().numpy().view(np.uint64)
        ss, pp = from_orderable(kh >> np.uint64(32)), (kh & np.uint64(0xFFFFFFFF)).astype(np.int64)
        tp = np.asarray(g.train_pos_host, dtype=np.int64)
        M = minor.max(0)
        cen = s0h[ids]
        pcs = np.searchsorted(ss, cen, side="left")
        for i in np.flatnonzero(M > 0).tolist():
            c, pc, mm = cen[i], int(pcs[i]), int(M[i])
            a, e = max(pc - mm, 0), min(pc + mm, P)
            while a > 0 and a < pc and abs(c - ss[a - 1]) == abs(c - ss[a]):     # a tie at an end of the window: its whole run
                a -= 1
            while e < P and e > pc and abs(c - ss[e]) == abs(c - ss[e - 1]):
                e += 1
            d = np.abs(c - ss[a:e]).astype(np.float32)
            order = np.lexsort((pp[a:e], d))[:mm]
            wid, wd = tp[pp[a:e][order]].astype(np.int32), d[order]
            for r in range(R):
                mr, o = int(minor[r, i]), int(moff[r * n + i])
                m_ids[o:o + mr] = wid[:mr]
                m_dist[o:o + mr] = wd[:mr]
    return off, out_ids, out_dist, moff, m_ids, m_dist


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
        cases.append(("yelp", lambda: synth.yelp_like(0), 1024))
    if "powerlaw" in only:
        cases.append(("powerlaw_2m", lambda: synth.power_law(2_000_000, 40_000_000, 0), 4096))
    for name, make, B in cases:
        t0 = time.time()
        w = make()
        tr = PCGNNTrainer(w, dict(engine="graph", batch_size=B, seed=0), dev)
        tr.run_epoch_one_graph()                            # (trained parameters; the engine as a training run leaves it)
        fz = tr.fused
        print(f"# {name}: built in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
        ids = np.asarray(w.idx_train, dtype=np.int64)
        labels = np.asarray(w.labels)[ids]
        old_ms, old = timed(lambda: old_pass(fz, ids, labels, B), args.reps, dev)
        new_ms, new = timed(lambda: fz.chosen(ids, labels=labels, train_flag=True), args.reps, dev)
        test_ms, _ = timed(lambda: fz.chosen(ids), args.reps, dev)
        bits = lambda x: x.view(np.uint32)
        same = (np.array_equal(old[0], new.host_offsets()) and np.array_equal(old[1], new.ids.cpu().numpy())
                and np.array_equal(bits(old[2]), bits(new.dist.cpu().numpy()))
                and np.array_equal(old[3], new.minor_host_offsets()) and np.array_equal(old[4], new.minor_ids.cpu().numpy())
                and np.array_equal(bits(old[5]), bits(new.minor_dist.cpu().numpy())))
        spread = max(old_ms) - min(old_ms)
        med = lambda x: round(float(np.median(x)), 3)
        res = dict(workload=name, set="train", n=len(ids), positives=int((labels == 1).sum()), n_pos=fz.g.n_pos,
                   entries=int(old[0][-1]), minority_entries=int(old[3][-1]), batch=B, reps=args.reps,
                   old_ms=med(old_ms), old_min=round(min(old_ms), 3), old_max=round(max(old_ms), 3),
                   train_ms=med(new_ms), train_min=round(min(new_ms), 3), train_max=round(max(new_ms), 3),
                   test_ms=med(test_ms), test_min=round(min(test_ms), 3), test_max=round(max(test_ms), 3),
                   minority_ms=round(med(new_ms) - med(test_ms), 3), old_spread_ms=round(spread, 3),
                   speedup=round(float(np.median(old_ms) / np.median(new_ms)), 2), identical=bool(same))
        print(json.dumps(res), flush=True)
        assert same, "the two ways disagree"
        assert np.median(new_ms) <= np.median(old_ms) - spread, "chosen(train_flag=True) is not faster than the per-batch way beyond its spread"
        del tr, fz
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
