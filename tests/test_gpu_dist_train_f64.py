"""The partitioned engine's training steps (pc-gnn_amd/dist.py, DistributedPCGNN) against float64 and torch.optim.Adam, every
step of two windows.  Run with ``pytest -m gpu`` on an MI355X; all ranks share GPU 0, collectives staged through the host (gloo).

Cases (tests/adam_ref.py: DistCase): a 6000-node three-relation graph, model shapes (32, 64, 3) and (25, 128, 3), per-rank batch
129 (eight full 16-row tiles and one row), a window of 3 * 129 + 17 centres per rank - steps of 129, 129, 129 and 17, the short
one behind longer ones in the same activations, aggregates, plans and workspace - and a second window of 129 + 17, so that an
update rides across a window boundary; then both windows once more (twelve steps), because the first use of a step's graph runs
a warm-up step that applies the waiting update itself: only in the second round does every step of the captured path - the
17-row tails, whose scores 2a compares, included - replay with a gradient waiting.  World sizes 1 (launch by launch, and through
the captured per-step graphs) and 2 (graphs).

Two engines per rank from the same seed.  A runs the windows as the product does (train_window: every update rides in the next
step's front launch; one flush() at the very end).  B flushes after every step and keeps theta_k, m_k, v_k, the step counter,
and the step's all-reduced gradient, logits, row losses and ReLU masks.

  2a  A and B end bit-identical (theta, m, v, step counter = the number of steps: the warm-up before a graph capture is not
      counted); at the end of each window the scores A's last front launch computed equal pcg_score_table with the classifier of
      B's theta before that step, bit for bit, on every row A holds.  Whether that front launch found a gradient waiting - and so
      RECOMPUTED the label classifier from its snapshot and the gradient (csrc/choose.hip: front_dist_kernel's "same statement
      of the arithmetic") instead of reading the snapshot - is read from the device word before every front launch of A and
      asserted: every step of the second round in every mode and world, and every step but the first launch by launch.
  2b  every step of B: the device's float32 theta_k, m_k, v_k, the all-reduced gradient and t = k + 1 through adam_ref in
      float64; theta_{k+1}, m_{k+1}, v_{k+1} within the tolerances of test_adam_step_matches_torch_adam (theta atol lr * 2e-5;
      m rtol 1e-5 atol 2e-7; v rtol 5e-5 atol 1e-12).  Entries whose float64 |g + wd theta| is below 2^-16 of the larger term are
      left out of theta's comparison (the float32 sum has no correct digit there): at most 1e-3 of the parameters, asserted.
  2c  every step of B: the global batch (all ranks' ids, labels, masks, in rank order) through dense_ref in float64 at theta_k,
      the chosen sets from the single-GPU kernels on the whole graph with theta_k's classifier (tests/test_dist_gpu.py holds
      the partitioned lists equal to those).  The all-reduced gradient per parameter, the gradient recovered from B's first
      moments, this rank's logits and the loss - sum over the ranks of row_loss[:B].sum(), times 1 / (B * world): row_loss holds
      the rows' UNSCALED loss terms (csrc/dense.h) - each within e_kernel <= 8 * e_f32 + 2^-20 of float64, e_f32 the same
      reference in float32 (through float32 torch.optim.Adam for the recovered gradient): the rule of test_gpu_grad_f64.py, not
      fitted to this code.  ReLU kinks as there (at most 1e-4 of the activations ambiguous, no mask wrong outside that band).
  2d  world 2: every rank ends with the same theta, m, v, bit for bit.

What the planted mistakes - Adam's t off by one, decoupled decay, a stale classifier state, the loss scaled by 1 / B, a row
counted twice - do to theta, and that the reference alone keeps the caps on these seeds: tests/test_adam_ref_host.py.

Measured on an MI355X (profiles/r13/dist_train_f64_ratios.txt): the maximum over the twelve steps, the tensors and the ranks.
2b: the worst error as a fraction of its tolerance, and the largest share of entries left out; 2c: `ratio` = e_kernel / e_f32
over the entries with e_f32 >= 2^-24, `of bound` = e_kernel / (8 * e_f32 + 2^-20):

    shape (F, E, R)  world  steps run         | 2b theta  m      v      left out | 2c ratio  of bound
    (32, 64, 3)      1      launch by launch  | 0.467     0.045  0.260  0        | 5.27      0.26
    (32, 64, 3)      1      per-step graphs   | 0.467     0.045  0.260  0        | 5.27      0.26
    (32, 64, 3)      2      per-step graphs   | 0.457     0.036  0.261  0        | 2.55      0.27
    (25, 128, 3)     1      launch by launch  | 0.453     0.050  0.261  0        | 3.97      0.23
    (25, 128, 3)     1      per-step graphs   | 0.453     0.050  0.261  0        | 3.97      0.23
    (25, 128, 3)     2      per-step graphs   | 0.456     0.031  0.261  0        | 2.96      0.22

2a and 2d held bit for bit in every case; the classifier was recomputed inside the compared front launch in both windows of the
second round in every mode and world (launch by launch in the first round too).  The largest 2c ratios are gradients recovered
from the first moment (5.27: the label classifier's two biases at a 17-row step, e_kernel 4.1e-7); every e_kernel is below 1e-6.
v's quarter of its tolerance is the float32 constant 1 - 0.999f against 0.001 (1.3e-5 relative, rtol 5e-5).  No bug was found.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import adam_ref as A
from tests import dense_ref as D
from tests.grad_check import Tally, by_name, check_first_moment, dist_views
from tests.util import PARAM_KEYS

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _state(d):
    torch.cuda.synchronize()
    return dict(theta=d.theta.clone(), m=d.m.clone(), v=d.v.clone(), t=int(d.step_counter.item()))


def _gathered(world, t):
    """a CPU tensor of every rank, in rank order"""
    out = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(out, t)
    return out


def _run_mode(c, rank, world, use_graphs, g_full, problems):
    """both engines through the windows in one mode; returns the figures.  Nothing is asserted before the last collective: what
    fails goes into `problems` (a rank that raised early would leave the others inside a collective)."""
    from pcgnn_amd import ops
    from pcgnn_amd.dist import DistributedPCGNN
    dev = torch.device("cuda", 0)
    F, E, R = c.shape
    tag = f"{c.shape} world {world} rank {rank} graphs {int(use_graphs)}"
    a = DistributedPCGNN(c.w, c.cfg, dev, stage_host=True, window=4)
    b = DistributedPCGNN(c.w, c.cfg, dev, stage_host=True, window=4)
    part, views = b.part, dist_views(b)
    if (part.lo, part.hi) != (c.parts[rank].lo, c.parts[rank].hi) or a.collectives_in_graph or a.window_graphs:
        problems.append(f"{tag}: partition {(part.lo, part.hi)} / graph modes are not the case's")
    for k, v in by_name(views, b.theta).items():
        if not torch.equal(v.cpu(), c.params()[k]):
            problems.append(f"{tag}: DistCase does not restate the engine's initial {k}")
    if not torch.equal(a.theta, b.theta):
        problems.append(f"{tag}: the two engines start from different parameters")
    o3, o4 = (int(b.lib.pcg_dense_param_offset(F, E, R, wch, 0)) for wch in (3, 4))

    def scores(theta):
        """the single-GPU score pass on the whole graph with theta's label classifier"""
        return ops.score_table(g_full, theta[o3:o3 + 2 * F].view(2, F), theta[o4:o4 + 2])

    windows = []
    for win in range(len(A.WINDOWS)):
        ids_w = torch.from_numpy(c.centres(rank, win).astype(np.int32)).to(dev)
        lab_w = b.labels_of(ids_w)
        if not torch.equal(lab_w.cpu().long(), torch.from_numpy(c.labels[c.centres(rank, win) + part.lo])):
            problems.append(f"{tag}: window {win}: the engine's labels are not the case's")
        windows.append((ids_w, lab_w))

    # ---- B: a flush after every step; the state before and after, and what the step left ----
    states, recs = [_state(b)], []
    for k, (win, b0, B) in enumerate(A.STEPS):
        ids_w, lab_w = windows[win]
        if b0 == 0:
            b.begin_window(ids_w)
        ids, lab = ids_w[b0:b0 + B], lab_w[b0:b0 + B]
        b.train_step(ids, lab, use_graphs=use_graphs)
        torch.cuda.synchronize()
        recs.append(dict(grad=b.grad.clone(), logits=b.logits[:B].clone(), row_loss=b.row_loss[:B].clone(),
                         masks=D.device_masks(b.acts, F, E, R, B), ids=(ids.long() + part.lo).cpu(), lab=lab.long().cpu()))
        b.flush()
        states.append(_state(b))

    # ---- A: the windows as the product runs them; 2a ----
    # `waiting`: the "a gradient is waiting" word as every step's front launch of A found it (read just before the launch by
    # launch step, or just before the step's graph replay - behind the warm-up of a graph's first use, which applies the
    # waiting update itself and leaves the replay nothing to recompute)
    waiting = []
    hook = "_replay_step" if use_graphs else "_seg_step"
    inner = getattr(a, hook)

    def spied(*args, **kwargs):
        waiting.append(int(a.opt_flag.item()))
        return inner(*args, **kwargs)
    setattr(a, hook, spied)
    done = 0
    for rnd in range(A.ROUNDS):
        for win, (ids_w, lab_w) in enumerate(windows):
            a.train_window(ids_w, lab_w, use_graphs=use_graphs)
            torch.cuda.synchronize()
            done += sum(1 for s in A.STEPS[:len(A.STEPS) // A.ROUNDS] if s[0] == win)
            # the window's last front launch scored with the classifier after update number done - 1: recomputed for itself
            # from the snapshot and the waiting gradient if it found one waiting (every step of the second round must)
            held = a.row_gid[a.row_gid >= 0].long()
            want = scores(states[done - 1]["theta"])
            same = torch.equal(a.s0_full[held], want[held])
            rode = len(waiting) == done and waiting[-1] == 1
            print(f"{tag} 2a round {rnd} window {win}: {held.numel()} held rows, scores of the "
                  f"{'RECOMPUTED classifier' if rode else 'snapshot (nothing was waiting)'} "
                  f"{'equal' if same else 'DIFFER in ' + str(int((a.s0_full[held] != want[held]).sum())) + ' rows'}")
            if not same:
                problems.append(f"{tag}: round {rnd} window {win}: the front launch's scores differ from the classifier of theta_{done - 1}")
            if int(a.step_counter.item()) != done:
                problems.append(f"{tag}: step counter {int(a.step_counter.item())} after {done} steps of A")
    setattr(a, hook, inner)
    first = len(A.STEPS) // A.ROUNDS
    print(f"{tag} 2a: gradient waiting at each of A's front launches: {waiting}")
    if len(waiting) != len(A.STEPS) or waiting[first:] != [1] * (len(A.STEPS) - first) or (not use_graphs and waiting[1:first] != [1] * (first - 1)):
        problems.append(f"{tag}: some front launch that should have found a gradient waiting did not (2a would compare nothing): {waiting}")
    a.flush()
    end = _state(a)
    for name in ("theta", "m", "v"):
        if not torch.equal(end[name], states[-1][name]):
            diff = int((end[name] != states[-1][name]).sum())
            problems.append(f"{tag}: riding and flushed engines end with different {name} ({diff} entries)")
    print(f"{tag} 2a: step counters A {end['t']} B {states[-1]['t']} ({len(A.STEPS)} steps)")
    if end["t"] != len(A.STEPS) or states[-1]["t"] != len(A.STEPS):
        problems.append(f"{tag}: step counters {end['t']} / {states[-1]['t']} after {len(A.STEPS)} steps")

    # ---- 2b, 2c: every step of B ----
    fig2b = dict(theta=0.0, m=0.0, v=0.0, excluded=0.0)
    tally = Tally(tag)
    for k, (win, b0, B) in enumerate(A.STEPS):
        s0, s1, rec = states[k], states[k + 1], recs[k]
        if s1["t"] != k + 1:
            problems.append(f"{tag}: step counter {s1['t']} after step {k}")
        fig = A.adam_figures((s1["theta"], s1["m"], s1["v"]), s0["theta"], s0["m"], s0["v"], rec["grad"], k + 1, c.lr, c.betas,
                             c.eps, c.wd)
        print(f"{tag} 2b step {k} (B {B}): of tolerance: theta {fig['theta']:.3f}  m {fig['m']:.3f}  v {fig['v']:.3f}  "
              f"left out {fig['excluded']:.2e} (cap {A.CANCEL_CAP:.0e})")
        if max(fig["theta"], fig["m"], fig["v"]) > 1.0 or fig["excluded"] > A.CANCEL_CAP:
            problems.append(f"{tag}: 2b step {k}: {fig}")
        fig2b = {n: max(fig2b[n], fig[n]) for n in fig2b}

        gb_ids, gb_lab = A.global_batch(_gathered(world, rec["ids"]), _gathered(world, rec["lab"]))
        if not (np.array_equal(gb_ids, c.step_batch(k)[0]) and np.array_equal(gb_lab, c.step_batch(k)[1])):
            problems.append(f"{tag}: step {k}: the gathered global batch is not the case's")
        every = [None] * world
        dist.all_gather_object(every, rec["masks"])
        masks = [torch.cat([every[r][j] for r in range(world)]) for j in range(R + 1)]
        s_k = scores(s0["theta"])
        sets, _, _ = ops.chosen_sets(g_full, torch.from_numpy(gb_ids.astype(np.int32)).to(dev),
                                     torch.from_numpy(gb_lab.astype(np.int32)).to(dev), s_k, ops.pos_sort(g_full, s_k),
                                     [0.5] * R, c.rho, True)
        params = {n: v.detach().cpu().clone() for n, v in by_name(views, s0["theta"]).items()}
        r64, r32, share, wrong = D.reference_pair(c, gb_ids, gb_lab, sets, params=params, dev_masks=masks)
        print(f"{tag} 2c step {k} (B {B}): {share:.2e} of the activations ambiguous (cap {D.AMBIGUOUS_CAP:.0e}), {wrong} masks wrong")
        if share > D.AMBIGUOUS_CAP:
            problems.append(f"{tag}: step {k}: {share:.2e} of the activations are ambiguous - change the seed")
        if wrong:
            problems.append(f"{tag}: step {k}: {wrong} ReLU masks differ from the float64 sign outside the ambiguous band")
        grad = by_name(views, rec["grad"])
        for n in PARAM_KEYS(R):
            tally.check(f"step {k} B={B} all-reduced grad {n}", grad[n], r64["grads"][n], r32["grads"][n])
        check_first_moment(tally, c, views, f"step {k} B={B} first-moment", s1["m"], s0["theta"], r64, r32,
                           state=None if k == 0 else (s0["m"], s0["v"]))
        rows = slice(rank * B, (rank + 1) * B)
        tally.check(f"step {k} B={B} logits", rec["logits"], r64["logits"][rows], r32["logits"][rows])
        # row_loss: the rows' loss terms, unscaled; the step's loss is their sum over the ranks times the documented 1 / (B * world)
        total = rec["row_loss"].double().sum().cpu().reshape(1)
        dist.all_reduce(total)
        tally.check(f"step {k} B={B} loss", total[0] / (B * world), r64["loss"], r32["loss"])

    # ---- 2d ----
    for name in ("theta", "m", "v"):
        every = _gathered(world, end[name].cpu())
        if not all(torch.equal(every[0], t) for t in every[1:]):
            problems.append(f"{tag}: the ranks end with different {name}")
    for d in (a, b):
        d.check()
    print(f"RATIO {tag}: ratio {tally.ratio:.2f}  of bound {tally.of_bound:.2f}")
    for miss in tally.misses:
        problems.append(f"{tag}: 2c {miss}")
    return dict(graphs=int(use_graphs), ratio=tally.ratio, of_bound=tally.of_bound, **fig2b)


def _worker(rank, world, shape, modes, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import pcgnn_amd
        c = A.DistCase(shape, world)
        g_full = pcgnn_amd.DeviceGraph(c.X, c.csr, c.train_pos, torch.device("cuda", 0))
        problems, figures = [], []
        for use_graphs in modes:
            figures.append(_run_mode(c, rank, world, use_graphs, g_full, problems))
        q.put((rank, "ok" if not problems else "\n".join(problems), figures))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc(), []))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", A.WORLDS)
@pytest.mark.parametrize("shape", list(A.CASES))
def test_partitioned_steps_against_float64_and_adam(shape, world):
    """world 1: once launch by launch, once through the per-step graphs; world 2: through the graphs (the product's default)"""
    import queue
    import time
    modes = (False, True) if world == 1 else (True,)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, shape, modes, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res, deadline = [], time.time() + 600
    try:
        while len(res) < len(procs):                          # (a worker that died without a result ends the wait)
            try:
                res.append(q.get(timeout=5))
            except queue.Empty:
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                assert not dead and time.time() < deadline, f"workers ended without a result: exit codes {dead}"
            if res and res[-1][1] != "ok" and not res[-1][2]:     # (a rank that raised: the others may be inside a collective)
                break
    finally:
        for p in procs:
            p.join(timeout=5 if len(res) < len(procs) else 60)
            if p.is_alive():
                p.kill()
    for rank, msg, figures in sorted(res, key=lambda r: r[0]):
        for f in figures:
            print(f"FIGURES {shape} world {world} rank {rank} graphs {f['graphs']}: 2b of tolerance theta {f['theta']:.3f} m {f['m']:.3f} "
                  f"v {f['v']:.3f} left out {f['excluded']:.2e} | 2c ratio {f['ratio']:.2f} of bound {f['of_bound']:.2f}")
    for rank, msg, _ in res:
        assert msg == "ok", f"rank {rank}: {msg}"
    assert len(res) == len(procs)
