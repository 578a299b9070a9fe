"""The pipelined training step (FusedPCGNN.pipeline, pcg_dense_select_train): a sequence of steps run as
select(0), then per step gather(t) and ONE launch of [dense tiles of t || select of t + 1] leaves bit for bit what the
three-launch steps leave - parameters, Adam moments, the step counter, the stepped label classifier, the last batch's row losses
and a mid-group batch's selection lists - and no in-kernel wait times out."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def _pair(w, B, **cfg):
    from pcgnn_amd.handler import PCGNNTrainer
    a = PCGNNTrainer(w, dict(engine="graph", batch_size=B, seed=5, **cfg), dev())
    b = PCGNNTrainer(w, dict(engine="graph", batch_size=B, seed=5, **cfg), dev())
    a.fused.pipeline, b.fused.pipeline = True, False
    b.fused.theta.copy_(a.fused.theta)
    b.fused.params_changed()
    return a, b


def _run_and_compare(w, B, expect_pipelined, ahead=None, **cfg):
    """ahead: the engine's clf_ahead switch (None: its default for the graph); cfg: further trainer settings (emb_size)"""
    a, b = _pair(w, B, **cfg)
    nb = a.batches_per_epoch()
    assert a.pick_size % B != 0, "the last batch of every epoch must be partial"
    assert (a.fused._pipe_blocks > 0) == expect_pipelined
    if ahead is not None:
        a.fused.clf_ahead = b.fused.clf_ahead = ahead
        # (switched on, the two-epoch group below must take the schedule: the select halves' presorted instantiation)
        assert not ahead or a.fused._ahead([(None, None, B, 0)] * (2 * nb))
    mid = nb // 2
    lists = []
    for t in (a, b):
        t.run_epoch_one_graph(n_epochs=2)                    # a group of two epochs (partial last batches) ...
        t.run_epoch_one_graph(flush=False)                   # ... and one more, its last update left pending
        t.fused.flush()
        # a group cut short: batches 0 .. mid as one graph launch, so that the lists of batch `mid` are the last ones selected
        t.run_epoch_one_graph(flush=False, n_steps=mid + 1)
        lists.append(t.fused.read_batch_lists(mid))
        t.fused.flush()
    torch.cuda.synchronize()
    for t in (a, b):
        t.fused.check()                                      # (no sync time-out, no overflow)
    for name in ("theta", "m", "v", "step_counter", "clf_next", "row_loss"):
        assert torch.equal(getattr(a.fused, name), getattr(b.fused, name)), f"{name} ({w.name}, batch {B})"
    assert int(a.fused.step_counter[0]) == 3 * nb + mid + 1
    assert len(lists[0]) == len(lists[1])
    for r, (sa, sb) in enumerate(zip(*lists)):
        assert len(sa) == len(sb)
        for x, y in zip(sa, sb):
            assert np.array_equal(np.asarray(x), np.asarray(y)), f"relation {r}"
    assert torch.equal(a.fused.last_counts, b.fused.last_counts)


def test_pipelined_equals_three_launches_mini():
    from pcgnn_amd import synth
    w = synth.make_workload("mini", 6000, 32, (4000, 30000, 90000), 0.12, seed=3)
    _run_and_compare(w, 256, True)


# The instantiations of the fused launch that the tests of this file, tests/test_gpu_clf_ahead.py and
# tests/test_gpu_launch_sequences.py do not launch (tests/test_edge_shapes_host.py works out which, and that these cases reach
# them): (feature width, emb_size, the classifier two batches ahead).  emb 128 at the two fixed widths, the two run-time-shape
# kernels (F 30: weights in LDS, F 64: weights streamed) with the select half sorting its keys (False) and finding them sorted
# (True: the presorted instantiation), and the presorted fixed kernel of F 25 at emb 64.
OTHER_SHAPES = [(F, E, ahead) for F, E in [(32, 128), (25, 128), (30, 64), (64, 64)] for ahead in (False, True)] + [(25, 64, True)]
MINI = dict(n=6000, rel_edges=(4000, 30000, 90000), pos_rate=0.12, seed=3, B=256)


@pytest.mark.parametrize("feat,emb,ahead", OTHER_SHAPES)
def test_pipelined_equals_three_launches_other_shapes(feat, emb, ahead):
    from pcgnn_amd import synth
    w = synth.make_workload("mini", MINI["n"], feat, MINI["rel_edges"], MINI["pos_rate"], seed=MINI["seed"])
    _run_and_compare(w, MINI["B"], True, ahead=ahead, emb_size=emb)


# (batch 2048: 128 tiles, the largest batch the fused launch takes - and two classifier workgroups, whose last one counts the step)
@pytest.mark.parametrize("wname,B", [("yelp", 1024), ("yelp", 2048), ("amazon", 256)])
def test_pipelined_equals_three_launches_full_size(wname, B):
    from pcgnn_amd import synth
    w = synth.yelp_like(0) if wname == "yelp" else synth.amazon_like(0)
    _run_and_compare(w, B, True)


def test_above_threshold_falls_back():
    """A batch of more than 128 tiles keeps the three-launch step (the fused launch would leave the selection too few CUs)."""
    from pcgnn_amd import synth
    w = synth.make_workload("mini", 50000, 32, (30000, 200000, 600000), 0.12, seed=3)
    _run_and_compare(w, 2064, False)


def test_pipelined_with_a_tight_list_capacity():
    """The selection list a fused launch's select half writes for a SHORT last batch and the partial sums its dense tiles read for
    the full batch before it share the data part: with a list capacity just above what the batches need (not the graph's worst
    case) the pipelined engine still leaves what the three-launch engine leaves, and nothing overflows."""
    from pcgnn_amd import synth
    from pcgnn_amd import _lib
    w = synth.make_workload("mini", 6000, 32, (4000, 30000, 90000), 0.12, seed=3)
    B = 256
    # the batches three single-epoch groups run (the same sampler seed in every engine): what their lists need
    probe, _ = _pair(w, B)
    lib = _lib.load()
    fz = probe.fused
    degs = [np.diff(ip) for ip, _ in w.csr]
    need = 0
    for _ in range(3):
        probe.run_epoch_one_graph()
        n = probe.pick_size
        ids = fz._ep_ids[:n].cpu().numpy()
        lab = fz._ep_lab[:n].cpu().numpy()
        for lo, Bb in fz._ep_batches:
            tot = 0
            for r in range(len(w.csr)):
                for i in range(lo, lo + Bb):
                    tot += lib.pcg_sel_capacity_row(int(degs[r][ids[i]]), float(fz.thresholds[r]), float(fz.rho[r]),
                                                    int(lab[i] == 1), fz.g.n_pos, 0)
            need = max(need, tot)
    assert probe.pick_size % B < B // 2, "the last batch must be shorter than half a batch"
    a, b = _pair(w, B, list_capacity=need + 1)
    assert a.fused.list_capacity == need + 1 and a.fused._pipe_blocks > 0
    for t in (a, b):
        for _ in range(3):
            t.run_epoch_one_graph()
    torch.cuda.synchronize()
    for t in (a, b):
        t.fused.check()
    for name in ("theta", "m", "v", "step_counter", "clf_next", "row_loss"):
        assert torch.equal(getattr(a.fused, name), getattr(b.fused, name)), name
    assert torch.equal(a.fused.theta, probe.fused.theta), "the list capacity changes nothing the step computes"
