"""The pipelined step with the label classifier two batches ahead (FusedPCGNN.clf_ahead, pcg_dense_select_ahead, pcg_clf_step):
whatever sequence of steps runs, the engine is left bit for bit as the same engine with the switch off leaves it - parameters,
Adam moments, the step counter, the stepped classifier, the last batch's row losses and counts, the score table and the train-pos
keys the next step would start from - and no status bit is raised.

The graph is small (6000 nodes, F 32, three relations, batch 128) but has what the fused launch's select half can go wrong on with
keys sorted a launch earlier: positive centres of more than 512 neighbours in the last relation (workgroup rows: the window
search on the group's last wave), positive single-wave rows, 280 train positives (not a multiple of 64: a partial key group for
the sort riders), a last batch of 40 rows (less than half a batch)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 128
N_IDS = 6 * B + 40          # seven batches, the last one short
NAMES = ("theta", "m", "v", "step_counter", "clf_next", "row_loss")


def dev():
    return torch.device("cuda", 0)


def _workload(with_pos=True):
    from pcgnn_amd import synth
    w = synth.make_workload("mini", 6000, 32, (4000, 30000, 90000), 0.12, seed=3)
    rs = np.random.RandomState(11)
    # a dozen train positives become hubs of the last relation: 600 more neighbours each
    hubs = rs.choice(np.asarray(w.train_pos), size=12, replace=False)
    indptr, idx = w.csr[2]
    src = np.repeat(np.arange(w.n, dtype=np.int64), np.diff(indptr))
    dst = idx.astype(np.int64)
    hs = np.repeat(hubs.astype(np.int64), 600)
    hd = np.concatenate([rs.choice(w.n, size=600, replace=False) for _ in hubs]).astype(np.int64)
    w.csr[2] = synth._csr_from_pairs(w.n, np.concatenate([src, hs]), np.concatenate([dst, hd]))
    w.homo_deg = synth._homo_degree(w.n, w.csr)
    if len(w.train_pos) % 64 == 0:                       # (the key groups must end in a partial one)
        w.train_pos = w.train_pos[:-1]
    # the staged ids: every batch has hub positives, ordinary positives and ordinary training nodes
    ids = []
    pos = np.asarray(w.train_pos)
    for b in range(-(-N_IDS // B)):
        nb = min(B, N_IDS - b * B)
        part = np.concatenate([rs.choice(hubs, size=3, replace=False), rs.choice(pos, size=min(30, nb - 3)),
                               rs.choice(w.idx_train, size=max(nb - 33, 0))])
        ids.append(rs.permutation(part)[:nb])
    ids = np.concatenate(ids).astype(np.int32)
    deg2 = np.diff(w.csr[2][0])
    assert deg2[hubs].min() > 512 and all(np.isin(ids[b * B:(b + 1) * B], hubs).any() for b in range(7))
    assert len(w.train_pos) % 64 != 0 and N_IDS % B < B // 2
    if not with_pos:
        w.train_pos = []
    return w, ids


_CACHE = {}


def workload(with_pos=True):
    if with_pos not in _CACHE:
        _CACHE[with_pos] = _workload(with_pos)
    return _CACHE[with_pos]


def _engine(w, ahead, list_capacity=None):
    import torch.nn as nn
    from pcgnn_amd.graph import DeviceGraph
    from pcgnn_amd.layers import InterAgg, IntraAgg
    from pcgnn_amd.model import PCALayer
    from pcgnn_amd.fused import FusedPCGNN
    torch.manual_seed(5)
    g = DeviceGraph(w.X, w.csr, w.train_pos, dev())
    f = w.X.shape[1]
    feats = nn.Embedding(w.n, f)
    feats.weight = nn.Parameter(torch.from_numpy(w.X), requires_grad=False)
    intras = [IntraAgg(feats, f, 64, w.train_pos, 0.5, cuda=True) for _ in w.csr]
    inter = InterAgg(feats, f, 64, w.train_pos, g, intras, cuda=True)
    model = PCALayer(2, inter, 2.0).to(dev())
    return FusedPCGNN(model, 0.01, 0.001, max_batch=B, list_capacity=list_capacity, pipeline=True, clf_ahead=ahead)


def _pair(with_pos=True, list_capacity=None):
    w, ids = workload(with_pos)
    a, b = _engine(w, True, list_capacity), _engine(w, False, list_capacity)
    b.theta.copy_(a.theta)
    b.params_changed()
    ids_d = torch.from_numpy(ids).to(dev())
    lab_d = torch.from_numpy(w.labels[ids].astype(np.int32)).to(dev())
    for fz in (a, b):
        fz.begin_epoch(ids_d, lab_d, B)
    steps = [(None, None, Bb, 0) for _, Bb in a._ep_batches]
    assert a._ahead(steps) and not b._ahead(steps), "the switch must decide the schedule of this shape"
    return a, b


def _same(a, b, what):
    torch.cuda.synchronize()
    for fz in (a, b):
        fz.check()                                           # (no overflow, no time-out)
    for name in NAMES:
        assert torch.equal(getattr(a, name), getattr(b, name)), f"{name} ({what})"
    assert torch.equal(a.last_counts, b.last_counts), f"last counts ({what})"
    # what the next step starts from: the scores and the sorted / raw keys of the classifier the sequence left
    assert a._fresh == b._fresh
    assert torch.equal(a.s0, b.s0), f"s0 ({what})"
    P = a.g.n_pos
    if P:
        cap = a.keys.numel() // 2
        assert torch.equal(a.keys[:P], b.keys[:P]) and torch.equal(a.keys[cap:cap + P], b.keys[cap:cap + P]), f"keys ({what})"


@pytest.mark.parametrize("n_steps", [1, 2, 3, 4, 7])
def test_sequence_lengths(n_steps):
    """prologue and epilogue meet (3, 4), shorter sequences keep the parent's schedule (1, 2), 7 ends in the 40-row batch"""
    a, b = _pair()
    for fz in (a, b):
        fz.epoch_run(n_steps=n_steps, flush=False)
    _same(a, b, f"{n_steps} steps, update pending")
    assert int(a.step_counter[0]) == n_steps
    for fz in (a, b):
        fz.flush()
    _same(a, b, f"{n_steps} steps, flushed")


def test_no_train_positives():
    a, b = _pair(with_pos=False)
    assert a.g.n_pos == 0
    for fz in (a, b):
        fz.epoch_run(flush=True)
    _same(a, b, "no train positives")


def test_two_groups_back_to_back_then_infer():
    a, b = _pair()
    for fz in (a, b):
        fz.epoch_run(flush=False)
        fz.epoch_run(n_steps=5, flush=False)                 # (the first gather launch applies the first group's last update)
    _same(a, b, "two groups")
    la, lb = a.infer(), b.infer()                            # (flushes; reads theta alone)
    assert torch.equal(la, lb)
    _same(a, b, "two groups, after infer")


def test_group_tail_as_eager_timed_step():
    """the benchmark's bracketed pattern: r - 1 steps as one graph, the r-th kernel by kernel (three launches)"""
    a, b = _pair()
    for fz in (a, b):
        fz._prof = []
        fz.epoch_run(n_steps=6, flush=False)
        fz.epoch_step_timed(6, eager=True, flush=False)
        fz.flush()
        fz._prof = None
    _same(a, b, "6 steps + eager tail")
    assert int(a.step_counter[0]) == 7


def test_graph_replay_equals_eager():
    a, b = _pair()
    a.epoch_run(flush=True)                                  # captured, replayed
    a.epoch_run(n_steps=4, flush=True)
    for n in (7, 4):                                         # the same launches one by one, the switch on as well
        steps = [(b._ep_ids[lo:lo + Bb], b._ep_lab[lo:lo + Bb], Bb, b._ep_plan(i)) for i, (lo, Bb) in enumerate(b._ep_batches)][:n]
        b.clf_ahead = True
        b._theta_written()
        b._enqueue_pipelined(steps)
        b.flush()
    _same(a, b, "graph replay against eager launches")


def test_tight_list_capacity():
    """a list capacity just above the batches' need: the short last batch's list and the partial sums of the batch before it
    share the data part"""
    from pcgnn_amd import _lib
    lib = _lib.load()
    w, ids = workload()
    probe = _engine(w, True)
    degs = [np.diff(ip) for ip, _ in w.csr]
    need = 0
    for lo in range(0, N_IDS, B):
        tot = 0
        for r in range(len(w.csr)):
            for i in ids[lo:lo + B]:
                tot += lib.pcg_sel_capacity_row(int(degs[r][i]), float(probe.thresholds[r]), float(probe.rho[r]),
                                                int(w.labels[i] == 1), probe.g.n_pos, 0)
        need = max(need, tot)
    a, b = _pair(list_capacity=need + 1)
    assert a.list_capacity == need + 1
    for fz in (a, b):
        fz.epoch_run(flush=True)
    _same(a, b, "tight list capacity")
