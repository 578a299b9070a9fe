"""Wall clock of the stage after ``alerts`` that turns the alert list into cases, two ways, on the same list.

    python scripts/cases_bench.py [--reps 5] [--only yelp,powerlaw] [--ks 100,1000,65536]

Per workload and k, after a warm-up, the median of --reps passes (synchronised at both ends) of
  (a) host:   today's route - copy the alert ids to the host, slice their CSR rows off the device tensors (one gather per
              relation, copied to the host), map the neighbours to slots, scipy connected_components on the induced, symmetrised
              slot graph, number the components by their lowest slot;
  (b) device: ops.group_members (pcg_alert_cases) and its one read of the header.
The script asserts that (a)'s numbering equals (b)'s ``case_of`` and reports whether the gap between the medians exceeds the
old route's own max - min over the repetitions.  One JSON line per (workload, k).  Workloads: yelp_like(0) and
power_law(2 M, 40 M), every node ranked."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def host_cases(g, ids_dev):
    """(a) -> case_of [k] int32 (-1 for padding), numbered by ascending lowest slot"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    ids = ids_dev.cpu().numpy()
    k = ids.size
    slots = np.nonzero(ids >= 0)[0]
    nodes = ids[slots].astype(np.int64)
    uniq, first = np.unique(nodes, return_index=True)                    # a node's first slot (np.unique: the first occurrence)
    first_slot = slots[first]
    v = torch.from_numpy(nodes).to(ids_dev.device)
    rows, cols = [slots], [first_slot[np.searchsorted(uniq, nodes)]]      # the same node twice
    for r in range(g.R):
        beg, end = g.indptr[r][v], g.indptr[r][v + 1]
        cnt = end - beg
        total = int(cnt.sum().item())
        if total == 0:
            continue
        owner = torch.repeat_interleave(torch.arange(v.numel(), device=v.device), cnt)
        at = torch.arange(total, device=v.device) - (torch.cumsum(cnt, 0) - cnt)[owner] + beg[owner]
        nb = g.indices[r][at].cpu().numpy().astype(np.int64)
        src = slots[owner.cpu().numpy()]
        where = np.minimum(np.searchsorted(uniq, nb), uniq.size - 1)
        keep = (uniq[where] == nb) & (nb != ids[src])
        rows.append(src[keep])
        cols.append(first_slot[where[keep]])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    a = sp.coo_matrix((np.ones(rows.size, dtype=np.int8), (rows, cols)), shape=(k, k)).tocsr()
    _, lab = connected_components(a + a.T, directed=False)
    lab = lab[slots]
    _, head_at = np.unique(lab, return_index=True)                       # number by ascending lowest slot
    number = np.empty(lab.max() + 1 if lab.size else 0, dtype=np.int64)
    order = np.argsort(head_at, kind="stable")
    number[np.unique(lab)[order]] = np.arange(order.size)
    case_of = np.full(k, -1, dtype=np.int32)
    case_of[slots] = number[lab]
    return case_of


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="yelp,powerlaw")
    ap.add_argument("--ks", default="100,1000,65536")
    args = ap.parse_args()
    import pcgnn_amd  # noqa: F401
    from pcgnn_amd import ops, synth
    from pcgnn_amd.handler import PCGNNTrainer
    dev = torch.device("cuda", 0)
    only = args.only.split(",")
    cases = []
    if "yelp" in only:
        cases.append(("yelp", lambda: synth.yelp_like(0), 1024, 3))
    if "powerlaw" in only:
        cases.append(("powerlaw_2m", lambda: synth.power_law(2_000_000, 40_000_000, 0), 4096, 1))
    for name, make, B, epochs in cases:
        t0 = time.time()
        w = make()
        tr = PCGNNTrainer(w, dict(engine="graph", batch_size=B, seed=0), dev)
        for _ in range(epochs):
            tr.run_epoch_one_graph()
        fz = tr.fused
        print(f"# {name}: built in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
        for k in (int(x) for x in args.ks.split(",")):
            al = fz.alerts(k=k)
            ids_host = al.ids.cpu().numpy()
            deg = sum(np.asarray(d)[ids_host[ids_host >= 0]].astype(np.int64) for d in fz.g.deg_host)
            ways = {"host": lambda: host_cases(fz.g, al.ids), "device": lambda: ops.group_members(fz.g, al.ids, alerts=al)}
            rows = {key: [] for key in ways}
            for rep in range(args.reps + 1):                            # (pass 0 is the warm-up)
                res = {}
                for key, fn in ways.items():
                    ms, res[key] = wall(fn)
                    if rep:
                        rows[key].append(ms)
                assert np.array_equal(res["host"], res["device"].case_of.cpu().numpy()), "the two routes disagree"
            cl = res["device"]
            med = {key: float(np.median(v)) for key, v in rows.items()}
            spread = {key: float(max(v) - min(v)) for key, v in rows.items()}
            gap = abs(med["host"] - med["device"])
            sizes = cl.size().cpu().numpy()
            print(json.dumps(dict(workload=name, n=w.n, k=k, member_degree_sum=int(deg.sum()), n_cases=cl.n_cases,
                                  largest_case=int(sizes.max()) if sizes.size else 0, links=int(cl.links.sum().item()),
                                  host_ms=round(med["host"], 4), device_ms=round(med["device"], 4),
                                  host_spread_ms=round(spread["host"], 4), device_spread_ms=round(spread["device"], 4),
                                  faster="device" if med["device"] < med["host"] else "host", gap_ms=round(gap, 4),
                                  gap_exceeds_host_spread=gap > spread["host"], routes_agree=True)), flush=True)
        del tr, fz
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
