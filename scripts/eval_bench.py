"""Wall-clock evaluation passes, host metrics against device-side counts, on the same engine and the same ids.

    python scripts/eval_bench.py [--reps 5] [--big] [--only yelp,powerlaw]

Per set, after a warm-up, the median of --reps passes of
  (a) utils.test as it runs by default: infer -> sigmoid -> copy [n, 2] to the host -> numpy metrics (binary_metrics, roc_auc),
  (b) utils.test(on_device=True): infer -> sigmoid -> pcg_eval_counts -> copy 8 + 2 T words -> metrics_from_counts,
each split into "logits" (FusedPCGNN.infer, synchronised at both ends) and "metrics" (everything after it, wall clock to the
returned floats; for (b) also HIP events around the stage).  get_best_f1's sweep is timed on its own for (a) - (b)'s counts
hold it already.  The script asserts that both ways return identical values and that (b)'s metrics stage is shorter than the
infer stage of the same run.  One JSON line per set.  Sets: yelp_like(0) held-out ids and whole graph, power_law(2 M, 40 M)
whole graph; --big: power_law(10 M, 200 M) whole graph."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--big", action="store_true", help="also power_law(10 M, 200 M), whole graph")
    ap.add_argument("--only", default="yelp,powerlaw")
    args = ap.parse_args()
    import pcgnn_amd  # noqa: F401
    from pcgnn_amd import synth, utils as U
    from pcgnn_amd.handler import PCGNNTrainer
    dev = torch.device("cuda", 0)
    only = args.only.split(",")
    cases = []
    if "yelp" in only:
        cases.append(("yelp", lambda: synth.yelp_like(0), 1024, ["held_out", "whole"], 3))
    if "powerlaw" in only:
        cases.append(("powerlaw_2m", lambda: synth.power_law(2_000_000, 40_000_000, 0), 4096, ["whole"], 1))
    if args.big:
        cases.append(("powerlaw_10m", lambda: synth.power_law(10_000_000, 200_000_000, 0), 4096, ["whole"], 1))
    ok = True
    for name, make, B, sets, epochs in cases:
        t0 = time.time()
        w = make()
        tr = PCGNNTrainer(w, dict(engine="graph", batch_size=B, seed=0), dev)
        for _ in range(epochs):
            tr.run_epoch_one_graph()
        fz = tr.fused
        print(f"# {name}: built in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
        for which in sets:
            ids = np.arange(w.n)
            if which == "held_out":
                ids = ids[~np.isin(ids, w.idx_train)]
            labels = np.asarray(w.labels)[ids]
            lab_dev = torch.from_numpy(labels.astype(np.int32)).to(dev)
            ids_dev = torch.as_tensor(ids, dtype=torch.int32, device=dev)

            def host_metrics(logits):
                prob = torch.sigmoid(logits).float().cpu().numpy()
                return U.binary_metrics(labels, prob.argmax(axis=1), prob[:, 1]), prob

            def device_metrics(logits):
                return U.device_metrics(torch.sigmoid(logits).float(), lab_dev)

            rows = {k: [] for k in ("infer", "host", "sweep", "device", "device_events", "test_host", "test_device")}
            for rep in range(args.reps + 1):                            # (pass 0 is the warm-up)
                ms_infer, logits = wall(lambda: fz.infer(ids_dev))
                ms_host, (m_host, prob) = wall(lambda: host_metrics(logits))
                ms_sweep, best = wall(lambda: U.get_best_f1(labels, prob[:, 1]))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                m_dev = device_metrics(logits)
                e1.record()
                torch.cuda.synchronize()
                ms_dev = (time.perf_counter() - t0) * 1e3
                ms_test_host, r_host = wall(lambda: U.test(ids, labels, fz, B, print_line=False))
                ms_test_dev, r_dev = wall(lambda: U.test(ids, labels, fz, B, print_line=False, on_device=True))
                same = all(m_dev[k] == v for k, v in m_host.items()) and (m_dev["best_f1"], m_dev["best_threshold"]) == best \
                    and r_host == r_dev
                assert same, (m_host, best, m_dev, r_host, r_dev)
                if rep:
                    for k, v in zip(rows, (ms_infer, ms_host, ms_sweep, ms_dev, e0.elapsed_time(e1), ms_test_host, ms_test_dev)):
                        rows[k].append(v)
            med = {k: float(np.median(v)) for k, v in rows.items()}
            shorter = med["device"] < med["infer"]
            ok &= shorter
            print(json.dumps(dict(workload=name, set=which, n=len(ids), n_pos=int(labels.sum()), infer_ms=round(med["infer"], 4),
                                  host_metrics_ms=round(med["host"], 4), host_best_f1_ms=round(med["sweep"], 4),
                                  device_metrics_ms=round(med["device"], 4), device_metrics_gpu_ms=round(med["device_events"], 4),
                                  test_host_ms=round(med["test_host"], 4), test_on_device_ms=round(med["test_device"], 4),
                                  identical_values=True, device_metrics_shorter_than_infer=shorter, auc=m_dev["auc"])), flush=True)
        del tr, fz
        torch.cuda.empty_cache()
    assert ok, "a workload's device metrics stage is not shorter than its infer stage"


if __name__ == "__main__":
    main()
