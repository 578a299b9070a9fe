"""Event-timed training steps with a CUSTOM loss: what it cost before the fused path took caller-supplied loss gradients, and what
it costs now.  The loss is the class-weighted focal loss (gamma 2) on the gnn logits + lambda_1 * CE on the label-aware logits,
the optimizer Adam with the trainer's lr and weight decay; eager steps on full batches of the epoch's picks.

    (a) engine="torch": HIP selection, then the dense tail, the loss, the backward and torch.optim.Adam as eager torch ops
    (b) engine="fused": FusedPCGNN.forward -> loss -> backward (pcg_dense_vjp + pcg_wgrad) -> optimizer_step(torch.optim.Adam)
    (c) engine="fused": FusedPCGNN.train_step_custom (the same loss, the engine's own Adam)
    (d) engine="fused": FusedPCGNN.train_step (the built-in loss) - the floor

    python scripts/custom_loss_bench.py [--steps 40] [--reps 7] [--only yelp,powerlaw]

A run is --steps consecutive steps between two device events (one synchronise at its end); the variants alternate inside every
repetition, after one warm-up run each.  One JSON line per workload: per variant the median ms per step over --reps runs and
the spread (max - min), and whether (b) and (c) beat (a) by more than (a)'s own spread."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GAMMA, WEIGHT = 2.0, (0.25, 0.75)


def focal_loss(lambda_1):
    weights = {}                                             # (device, dtype) -> the class weights there: no copy per step

    def loss(gnn, center, labels):
        y = labels.long()
        logp = Fn.log_softmax(gnn, dim=1).gather(1, y[:, None])[:, 0]
        key = (gnn.device, gnn.dtype)
        if key not in weights:
            weights[key] = torch.tensor(WEIGHT, dtype=gnn.dtype, device=gnn.device)
        w = weights[key][y]
        return (-(w * (1.0 - logp.exp()) ** GAMMA * logp).sum() + lambda_1 * Fn.cross_entropy(center, y, reduction="sum")) / y.numel()
    return loss


def run_ms(step, batches, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for s in range(steps):
        step(*batches[s % len(batches)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="yelp,powerlaw")
    args = ap.parse_args()
    import pcgnn_amd  # noqa: F401
    from pcgnn_amd import synth
    from pcgnn_amd.handler import PCGNNTrainer
    assert torch.cuda.is_available(), "a timing needs the GPU"
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
        cfg = dict(batch_size=B, seed=0)
        lam = 2.0                                            # DEFAULTS["alpha"]
        loss_fn = focal_loss(lam)
        ta = PCGNNTrainer(w, dict(engine="torch", **cfg), dev)
        adam = lambda ps: torch.optim.Adam(ps, lr=ta.cfg["lr"], weight_decay=ta.cfg["weight_decay"])
        tb = PCGNNTrainer(w, dict(engine="fused", **cfg), dev, loss_fn=loss_fn, optimizer=adam)
        tc = PCGNNTrainer(w, dict(engine="fused", **cfg), dev, loss_fn=loss_fn)
        td = PCGNNTrainer(w, dict(engine="fused", **cfg), dev)
        ids = ta.start_epoch(0)
        batches = [(ids[lo:lo + B].contiguous(), ta.labels_i32[ids[lo:lo + B].long()]) for lo in range(0, ids.numel() - B + 1, B)]
        assert batches, f"{name}: the epoch's picks do not fill one batch of {B}"
        print(f"# {name}: built in {time.time() - t0:.1f} s, {len(batches)} full batches of {B}", file=sys.stderr, flush=True)

        def step_a(b, lab):
            ta.opt.zero_grad(set_to_none=True)
            loss_fn(*ta.model(b, lab.long()), lab).backward()
            ta.opt.step()

        variants = {"a_torch_engine": step_a, "b_forward_backward_optimizer": lambda b, lab: tb.step(b),
                    "c_train_step_custom": lambda b, lab: tc.step(b), "d_train_step_builtin": lambda b, lab: td.step(b)}
        ms = {k: [] for k in variants}
        for k, fn in variants.items():                       # warm-up: workspaces, kernel attributes, the optimizers' state
            run_ms(fn, batches, max(len(batches), 4))
        for _ in range(args.reps):
            for k, fn in variants.items():
                ms[k].append(run_ms(fn, batches, args.steps))
        for t in (tb, tc, td):
            t.fused.flush()
            t.fused.check()
        torch.cuda.synchronize()
        out = dict(workload=name, batch=B, steps_per_run=args.steps, reps=args.reps)
        for k, v in ms.items():
            out[k] = dict(median_ms=round(float(np.median(v)), 4), spread_ms=round(float(max(v) - min(v)), 4))
        a = out["a_torch_engine"]
        for k in ("b_forward_backward_optimizer", "c_train_step_custom"):
            out[k]["speedup_over_a"] = round(a["median_ms"] / out[k]["median_ms"], 2)
            out[k]["beats_a_by_more_than_its_spread"] = bool(a["median_ms"] - out[k]["median_ms"] > a["spread_ms"])
        print(json.dumps(out), flush=True)
        del ta, tb, tc, td
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
