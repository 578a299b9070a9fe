"""Diagnostic: in-kernel stamps of the select half of ONE fused launch (dense tiles of t || select of t + 1) in the middle of a
pipelined sequence of four YelpChi-like steps run launch by launch.  PROBE_AHEAD=0: pcg_dense_select_train (the select half sorts
its keys itself); 1 (default): pcg_dense_select_ahead (keys sorted a launch earlier, the classifier two batches ahead).
Prints when the in-kernel sort publishes, when positive rows leave their wait, when the rows and the classifier step end."""
import sys, os, ctypes as C, torch, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pcgnn_amd import synth, _lib
from pcgnn_amd.handler import PCGNNTrainer
B = int(os.environ.get("PROBE_B", "1024"))
ahead = os.environ.get("PROBE_AHEAD", "1") != "0"
w = synth.yelp_like(0)
tr = PCGNNTrainer(w, dict(engine="graph", batch_size=B), torch.device("cuda", 0))
fz = tr.fused; g = fz.g; lib = _lib.load()
fz.clf_ahead = ahead
tr.start_epoch_staged(1)
steps = [(fz._ep_ids[lo:lo + Bb], fz._ep_lab[lo:lo + Bb], Bb, fz._ep_plan(i)) for i, (lo, Bb) in enumerate(fz._ep_batches)][:4]
assert fz._pipelines([(0, s[2]) for s in steps]) and fz._ahead(steps) == ahead
rows = g.R * B
stamps = torch.zeros(rows + 2, 8, dtype=torch.int64, device="cuda")
name = "pcg_dense_select_ahead" if ahead else "pcg_dense_select_train"
real = getattr(lib, name)
calls = {"n": 0, "on": False}
def wrapped(*a):                       # stamps for the SECOND fused launch of the sequence only (batch 1's tiles || batch 2's select)
    calls["n"] += 1
    hit = calls["on"] and calls["n"] == 2
    if hit: lib.pcg_debug_set_stamps(C.c_void_p(stamps.data_ptr()))
    rc = real(*a)
    if hit: lib.pcg_debug_set_stamps(None)
    return rc
setattr(lib, name, wrapped)
for it in range(3):
    calls["n"], calls["on"] = 0, it == 2
    fz._theta_written()
    fz._enqueue_pipelined(steps)
    fz.flush()
    torch.cuda.synchronize()
setattr(lib, name, real)
fz.check()
extra = stamps[rows].cpu().numpy().astype(np.float64) * 0.01
raw = stamps[:rows].cpu().numpy()
raw[:, 0] &= (1 << 54) - 1
st = raw.astype(np.float64) * 0.01
ids, lab = steps[2][0], steps[2][1]
deg = np.stack([g.deg_host[r][ids.cpu().numpy()] for r in range(g.R)]).reshape(-1)
pos = np.tile(lab.cpu().numpy() == 1, g.R)
ran = st[:, 0] > 0
t0 = st[ran, 0].min()
print("schedule:", "classifier two batches ahead, keys sorted a launch earlier" if ahead else "in-kernel sort", "| rows with stamps", int(ran.sum()), "of", rows)
if not ahead:
    print("   sort workgroup 0 started at %.2f, the LAST key group was published at %.2f us (after the first row start)" % tuple(extra[4:6] - t0))
if extra[3] > 0:
    print("   the label classifier's step: from %.2f to %.2f us" % tuple(extra[2:4] - t0))
wt = st[:, 7][ran & pos & (st[:, 7] > 0)] - t0
if wt.size:
    print("   positive rows left the wait for the sorted keys at: min %.2f p10 %.2f p50 %.2f p90 %.2f max %.2f us" % (
        wt.min(), np.percentile(wt, 10), np.percentile(wt, 50), np.percentile(wt, 90), wt.max()))
end = st[ran, 6] - t0
print("row end times (us): p50 %.1f p90 %.1f p99 %.1f max %.1f" % (np.percentile(end, 50), np.percentile(end, 90), np.percentile(end, 99), end.max()))
for what, msk in (("positive", pos), ("negative", ~pos)):
    for lo, hi, tier in ((0, 512, "single-wave"), (512, 1 << 30, "workgroup")):
        sel = ran & msk & (deg > lo) & (deg <= hi)
        if sel.any():
            print(f"   {what} {tier} rows: {int(sel.sum())}, start max {st[sel, 0].max() - t0:.1f}, end max {st[sel, 6].max() - t0:.1f}, time in the row mean {np.mean(st[sel, 6] - st[sel, 0]):.2f} max {np.max(st[sel, 6] - st[sel, 0]):.2f} us")
# the positive single-wave rows' phases: stamps 0 start, 1 distance keys, 2 k-th value, 3 kept ids, 7 the tail begins on the window
# (behind its wait / with the staged search's loads under way), 4 window known, 5 picks written, 6 end
sel = ran & pos & (deg <= 512) & (st[:, 7] > 0) & (st[:, 4] > 0)
if sel.any():
    ph = [("keys 0-1", 0, 1), ("k-th 1-2", 1, 2), ("kept 2-3", 2, 3), ("to tail 3-7", 3, 7), ("window 7-4", 7, 4), ("picks 4-5", 4, 5),
          ("end 5-6", 5, 6)]
    print(f"   positive single-wave rows with a tail ({int(sel.sum())}), mean us per phase: " +
          ", ".join(f"{n} {np.mean(st[sel, b] - st[sel, a]):.2f}" for n, a, b in ph))
order = np.flatnonzero(ran)[np.argsort(-(st[ran, 6] - t0))][:6]
print("last rows to finish: row deg positive | start | end")
for rr in order:
    print(f"  {rr:5d} {deg[rr]:5d} {int(pos[rr])} | {st[rr, 0] - t0:6.1f} | {st[rr, 6] - t0:6.2f}")
