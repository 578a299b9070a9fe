"""Train-mode chosen lists: pcg_rank_minority / ops.rank_minority / ops.choose_ranked(labels=...) / FusedPCGNN.chosen(train_flag=True)
/ layers.choose_step_neighs.  The oracle is tests/ranked_train_ref.py (pinned to the reference's own samp_score_diff by
test_ranked_train_ref_golden.py), fed the very scores the device used - so every comparison is exact: np.array_equal on ids and
on the distances' bit patterns.  No tolerance anywhere."""
import math
import os

import numpy as np
import pytest
import torch

from tests.ranked_train_ref import (compare_train_with_golden, golden_scores, golden_train_rows, minority_tail,
                                    ranked_train_ref)
from tests.util import GOLDEN, GoldenCase, build_model, synth_graph

pytestmark = pytest.mark.gpu

RANK_SLICE = 2048          # rank.hip: candidates of one slice; 64: the wave tier's limit
GOLDEN_CASES = ["yelp_small", "single_rel", "five_rel"]
FILL_ID, FILL_DIST = -7, -1.0


def dev():
    return torch.device("cuda", 0)


# ---- the kernel alone ---------------------------------------------------------------------------------------------------------
class Positives:
    """a graph that is nothing but P training positives (pcg_rank_minority reads no CSR), their scores and sorted keys"""

    def __init__(self, P, R, scores, seed=0):
        import pcgnn_amd as PK
        from pcgnn_amd import ops
        rs = np.random.RandomState(seed)
        self.P, self.R, self.N = P, R, P + 3
        self.train_pos = rs.permutation(self.N)[:P].astype(np.int64)
        empty = (np.zeros(self.N + 1, np.int64), np.zeros(0, np.int32))
        self.g = PK.DeviceGraph(np.zeros((self.N, 4), np.float32), [empty] * R, self.train_pos.tolist(), dev())
        self.s0 = np.zeros(self.N, np.float32)
        self.s0[self.train_pos] = scores
        self.pos_scores = torch.from_numpy(np.asarray(scores, dtype=np.float32))
        self.s0_dev = torch.from_numpy(self.s0).to(dev())
        self.keys = ops.pos_sort(self.g, self.s0_dev)
        self.sorted = np.sort(np.asarray(scores, dtype=np.float32))

    def run(self, centers, extents, nodes=None, guard=64):
        """centers float32 [n] (None: s0[nodes]), extents int [R, n] -> (flat offsets, ids, dist, status) with guard words"""
        from pcgnn_amd import ops
        extents = np.asarray(extents, dtype=np.int64).reshape(self.R, -1)
        n = extents.shape[1]
        off = ops.rank_offsets(extents)
        total = int(off[-1])
        ids = torch.full((total + 2 * guard,), FILL_ID, dtype=torch.int32, device=dev())
        dist = torch.full((total + 2 * guard,), FILL_DIST, dtype=torch.float32, device=dev())
        status = torch.zeros(1, dtype=torch.int32, device=dev())
        nd = torch.from_numpy(np.zeros(n, np.int32) if nodes is None else np.asarray(nodes, dtype=np.int32)).to(dev())
        cen = None if centers is None else torch.from_numpy(np.asarray(centers, dtype=np.float32)).to(dev())
        ops.rank_minority(self.g, nd, self.s0_dev, self.keys, torch.from_numpy(off).to(dev()), ids[guard:guard + total],
                          dist[guard:guard + total], status, center_s0=cen)
        st = int(status.item())
        ids, dist = ids.cpu().numpy(), dist.cpu().numpy()
        for buf, fill in ((ids, FILL_ID), (dist, FILL_DIST)):
            assert (buf[:guard] == fill).all() and (buf[guard + total:] == fill).all(), "a write outside the arrays"
        return off, ids[guard:guard + total], dist[guard:guard + total], st

    def check(self, centers, extents, what=""):
        extents = np.asarray(extents, dtype=np.int64).reshape(self.R, -1)
        off, ids, dist, st = self.run(centers, extents)
        assert st == 0, what
        n = extents.shape[1]
        for i in range(n):
            pos, d = minority_tail(torch.tensor(np.float32(centers[i])), self.pos_scores, int(extents[:, i].max()))
            for r in range(self.R):
                lo, m = int(off[r * n + i]), int(extents[r, i])
                assert np.array_equal(ids[lo:lo + m], self.train_pos[pos[:m]].astype(np.int32)), (what, self.P, r, i, m)
                assert np.array_equal(dist[lo:lo + m].view(np.uint32), d[:m].view(np.uint32)), (what, self.P, r, i, m)


# the wave tier's limit (64 candidates = m 32 on both sides) and RANK_SLICE's (2048 candidates = m 1024), one above and below
# each; two slices exactly and one more; several slices; everything but one; everything
M_LIST = [0, 1, 2, 31, 32, 33, 1023, 1024, 1025, 2048, 2049, 5000]


def placements(ss, m):
    """centre scores against the sorted scores ss: below every key, above every key, exactly on a key, between two keys in the
    middle, and within m of either end (the window is cut by the end of the array)"""
    P = len(ss)
    lo, hi = min(m // 2, P - 1), max(P - 1 - m // 2, 0)
    mid = lambda j: np.float32((float(ss[j]) + float(ss[min(j + 1, P - 1)])) / 2)
    return [np.float32(ss[0] - 1), np.float32(ss[-1] + 1), ss[P // 2], mid(P // 2), mid(lo), ss[lo], mid(hi), ss[hi]]


@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 1000, 12000])
def test_kernel_alone(P):
    pz = Positives(P, 1, np.random.RandomState(20 + P).randn(P).astype(np.float32), seed=P)
    centers, extents = [], []
    for m in sorted({m for m in M_LIST + [P - 1, P] if 0 <= m <= P}):
        for c in placements(pz.sorted, m):
            centers.append(c)
            extents.append(m)
    pz.check(np.array(centers, np.float32), [extents])
    # the centre's own score from the table (no center_s0): node = a training positive, distance 0 first
    off, ids, dist, st = pz.run(None, [[min(3, P)]], nodes=[int(pz.train_pos[0])])
    assert st == 0 and ids[0] == pz.train_pos[0] and dist[0] == 0.0
    pos, d = minority_tail(pz.pos_scores[0], pz.pos_scores, min(3, P))
    assert np.array_equal(ids, pz.train_pos[pos].astype(np.int32)) and np.array_equal(dist.view(np.uint32), d.view(np.uint32))


def test_kernel_relations_share_one_ranking():
    """R = 3, a different extent per row: every row is the prefix of its centre's ranking"""
    P = 3000
    pz = Positives(P, 3, np.random.RandomState(31).randn(P).astype(np.float32), seed=1)
    ext = np.array([[0, 5, 70], [2049, 1, 64], [33, 33, 0], [P, 0, 1], [0, 0, 0], [1, 1025, 2], [64, 65, 3000]]).T   # [3, n]
    cen = np.random.RandomState(32).randn(ext.shape[1]).astype(np.float32)
    cen[1] = pz.sorted[7]
    pz.check(cen, ext)
    assert ext.shape == (3, 7)


def test_kernel_rejects_an_extent_above_P():
    """an extent of P + 1: PCG_ST_RANK_MISMATCH, the row keeps its fill, its neighbours are written"""
    from pcgnn_amd import _lib
    from pcgnn_amd.fused import FusedPCGNN
    for P, good in ((65, 40), (3000, 1500)):
        pz = Positives(P, 1, np.random.RandomState(33).randn(P).astype(np.float32), seed=2)
        cen = np.array([0.1, -0.2, 0.3], np.float32)
        ext = [[good, P + 1, good]]
        off, ids, dist, st = pz.run(cen, ext)
        assert st == _lib.PCG_ST_RANK_MISMATCH
        with pytest.raises(_lib.PcgnnLibraryError, match="rank_minority"):
            FusedPCGNN._raise_status(st)
        assert (ids[off[1]:off[2]] == FILL_ID).all() and (dist[off[1]:off[2]] == FILL_DIST).all()
        for i in (0, 2):
            pos, d = minority_tail(torch.tensor(cen[i]), pz.pos_scores, good)
            assert np.array_equal(ids[off[i]:off[i + 1]], pz.train_pos[pos].astype(np.int32))
            assert np.array_equal(dist[off[i]:off[i + 1]].view(np.uint32), d.view(np.uint32))


def test_kernel_empty_calls_enqueue_nothing():
    from pcgnn_amd import ops
    pz = Positives(5, 2, np.arange(5, dtype=np.float32), seed=3)
    off, ids, dist, st = pz.run(np.zeros(0, np.float32), np.zeros((2, 0), np.int64))
    assert st == 0 and ids.size == 0 and off.tolist() == [0]
    import pcgnn_amd as PK
    empty = (np.zeros(9, np.int64), np.zeros(0, np.int32))
    g0 = PK.DeviceGraph(np.zeros((8, 4), np.float32), [empty], [], dev())            # no training positives
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    z64 = torch.zeros(3, dtype=torch.int64, device=dev())
    out_i, out_d = torch.full((1,), FILL_ID, dtype=torch.int32, device=dev()), torch.full((1,), FILL_DIST, device=dev())
    ops.rank_minority(g0, torch.zeros(2, dtype=torch.int32, device=dev()), torch.zeros(8, device=dev()),
                      torch.zeros(8, dtype=torch.int64, device=dev()), z64, out_i, out_d, status)
    assert int(status.item()) == 0 and int(out_i.item()) == FILL_ID


# ---- ties -----------------------------------------------------------------------------------------------------------------------
def test_ties_quantised_scores():
    """scores in eighths, P = 1000: every cut and most ranks tie - also across the centre (c - a == b - c exactly)"""
    P = 1000
    pz = Positives(P, 1, (np.random.RandomState(40).randint(0, 8, size=P) / 8.0).astype(np.float32), seed=4)
    centers, extents = [], []
    for c in (0.0, 0.125, 0.5, 0.875, 0.0625, 0.4375, 0.8125, -1.0, 2.0, 0.3):
        for m in (1, 2, 31, 32, 33, 64, 65, 125, 126, 500, 999, 1000):
            centers.append(c)
            extents.append(m)
    pz.check(np.array(centers, np.float32), [extents])
    assert abs(np.float32(0.4375) - np.float32(0.375)) == abs(np.float32(0.4375) - np.float32(0.5))


def test_ties_all_scores_equal():
    """one run of P equal distances: the first m by train_pos position"""
    P = 300
    pz = Positives(P, 1, np.full(P, 0.25, np.float32), seed=5)
    ms = [0, 1, 63, 64, 65, 299, 300]
    for c in (0.25, -3.0, 7.5):
        off, ids, dist, st = pz.run(np.full(len(ms), c, np.float32), [ms])
        assert st == 0
        for i, m in enumerate(ms):
            assert np.array_equal(ids[off[i]:off[i + 1]], pz.train_pos[:m].astype(np.int32)), (c, m)
            assert (dist[off[i]:off[i + 1]] == abs(np.float32(c) - np.float32(0.25))).all()
    pz.check(np.full(len(ms), 0.5, np.float32), [ms])


# ---- a synthetic three-relation graph ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synth():
    X, labels, csrs = synth_graph(1, 3000, 32, (3, 10, 40), 0.15)
    rs = np.random.RandomState(2)
    idx_train = np.sort(rs.choice(3000, size=1200, replace=False))
    train_pos = [int(v) for v in idx_train if labels[v] == 1]
    return X, labels, csrs, train_pos, idx_train


def assert_same_train(ch, ref, what=""):
    """a train-mode ChosenLists against ranked_train_ref's two triples: exact"""
    (off, ids, dist), (moff, mids, mdist) = ref
    assert ch.has_minority, what
    assert np.array_equal(ch.offsets.cpu().numpy(), off) and np.array_equal(ch.minor_offsets.cpu().numpy(), moff), what
    assert np.array_equal(ch.ids.cpu().numpy(), ids) and np.array_equal(ch.minor_ids.cpu().numpy(), mids), what
    assert np.array_equal(ch.dist.cpu().numpy().view(np.uint32), dist.view(np.uint32)), what
    assert np.array_equal(ch.minor_dist.cpu().numpy().view(np.uint32), mdist.view(np.uint32)), what


@pytest.mark.parametrize("scores", ["random", "quantised"])
@pytest.mark.parametrize("rho", [0.5, 2.0])
def test_against_the_training_selection(synth, rho, scores):
    """neighbour ids | minority ids == the set the training step's select kernel chose, on every row - the tie rule too"""
    import pcgnn_amd as PK
    from pcgnn_amd import ops
    X, labels, csrs, train_pos, idx_train = synth
    g = PK.DeviceGraph(X, csrs, train_pos, dev())
    rs = np.random.RandomState(50)
    s0h = rs.randn(3000).astype(np.float32) if scores == "random" else (rs.randint(0, 8, size=3000) / 8.0).astype(np.float32)
    nodes = np.concatenate([rs.choice(idx_train, size=300), [7], train_pos[:20]])
    lab = labels[nodes].astype(np.int32)
    assert lab.sum() > 20 and (lab == 0).sum() > 100
    thr = [0.5, 0.5, 0.5]
    s0 = torch.from_numpy(s0h).to(dev())
    keys = ops.pos_sort(g, s0)
    ch = ops.choose_ranked(g, nodes, s0, thr, labels=lab, rho=rho, pos_keys=keys)
    assert_same_train(ch, ranked_train_ref(csrs, nodes, lab, s0h, thr, rho, train_pos))
    nd, lb = torch.from_numpy(nodes.astype(np.int32)).to(dev()), torch.from_numpy(lab).to(dev())
    sets, _, cnt = ops.chosen_sets(g, nd, lb, s0, keys, thr, rho, True)
    cnt = cnt.cpu().numpy().reshape(3, -1)
    for r in range(3):
        got, got_scores = ch.to_reference(r)
        assert got == sets[r]
        assert [len(s) for s in got] == cnt[r].tolist()
        # the reference lists a pick that is also a kept neighbour twice in its distances, once in its set
        assert all(len(sc) >= len(s) for sc, s in zip(got_scores, got))
    # without keys the call sorts them itself; without labels it is the test-mode call, unchanged
    ch2 = ops.choose_ranked(g, nodes, s0, thr, labels=lab, rho=[rho] * 3)
    assert torch.equal(ch2.minor_ids, ch.minor_ids) and torch.equal(ch2.minor_dist, ch.minor_dist)
    ch3 = ops.choose_ranked(g, nodes, s0, thr)
    assert not ch3.has_minority and torch.equal(ch3.ids, ch.ids) and torch.equal(ch3.dist, ch.dist)
    assert torch.equal(ch3.flat_offsets, ch.flat_offsets)


# ---- the engine -------------------------------------------------------------------------------------------------------------------
def engine(X, csrs, train_pos, emb, rho, seed=0):
    import pcgnn_amd as PK
    from pcgnn_amd.fused import FusedPCGNN
    n, f = X.shape
    torch.manual_seed(seed)
    g = PK.DeviceGraph(X, csrs, train_pos, dev())
    feats = torch.nn.Embedding(n, f)
    feats.weight = torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(X)), requires_grad=False)
    intras = [PK.IntraAgg(feats, f, emb, train_pos, rho, cuda=True) for _ in csrs]
    inter = PK.InterAgg(feats, f, emb, train_pos, g, intras, cuda=True)
    return FusedPCGNN(PK.PCALayer(2, inter, 2.0).cuda(), 0.01, 0.001, max_batch=256)


def engine_ref(fz, csrs, ids, labels, train_pos):
    """the oracle on the scores the engine's last chosen call used"""
    return ranked_train_ref(csrs, ids, labels, fz._inf["s0"][:fz.g.n_nodes].cpu().numpy(), fz.thresholds, fz.rho, train_pos)


@pytest.fixture(scope="module")
def fused(synth):
    X, _, csrs, train_pos, _ = synth
    return engine(X, csrs, train_pos, 64, 0.5)


def test_engine_whole_graph_chunks_and_duplicates(fused, synth):
    _, labels, csrs, train_pos, _ = synth
    ch = fused.chosen(labels=labels, train_flag=True)                      # every node
    assert_same_train(ch, engine_ref(fused, csrs, np.arange(3000), labels, train_pos))
    assert ch.minor_offsets.shape == (3, 3001) and ch.minor_ids.dtype == torch.int32 and ch.minor_dist.dtype == torch.float32
    assert int(ch.minor_flat_offsets[-1]) > 0
    rs = np.random.RandomState(60)
    ids = np.concatenate([rs.randint(0, 3000, size=500), [7, 7, train_pos[0], train_pos[0], 2999, 0, 7]])
    rs.shuffle(ids)
    lab = labels[ids]
    want = engine_ref(fused, csrs, ids, lab, train_pos)
    whole = fused.chosen(ids, labels=lab, train_flag=True)
    assert_same_train(whole, want, "duplicates in ids")
    chunked = fused.chosen(torch.from_numpy(ids).to(dev()), chunk=64, labels=torch.from_numpy(lab).to(dev()), train_flag=True)
    assert_same_train(chunked, want, "chunk = 64")
    # the neighbour part is the test-mode call's
    test_mode = fused.chosen(ids)
    assert not test_mode.has_minority
    assert torch.equal(test_mode.ids, whole.ids) and torch.equal(test_mode.dist, whole.dist)
    assert torch.equal(test_mode.flat_offsets, whole.flat_offsets)
    # views and diagnostics
    (off, _, _), (moff, mids, mdist) = want
    b = int(np.argmax(np.diff(moff[2])))                                   # the longest minority row of relation 2
    i, d = whole.minor_row(2, b)
    assert np.array_equal(i.cpu().numpy(), mids[moff[2, b]:moff[2, b + 1]]) and i.numel() > 0
    assert np.array_equal(d.cpu().numpy(), mdist[moff[2, b]:moff[2, b + 1]])
    md, mdm = whole.mean_dist().cpu().numpy(), whole.mean_dist(include_minority=True).cpu().numpy()
    neg = lab == 0
    assert np.array_equal(md[:, neg], mdm[:, neg], equal_nan=True) and not np.array_equal(md[:, ~neg], mdm[:, ~neg], equal_nan=True)


def test_engine_argument_checks(fused, synth):
    _, labels, _, _, _ = synth
    with pytest.raises(ValueError):
        fused.chosen([1, 2, 3], train_flag=True)
    with pytest.raises(ValueError):
        fused.chosen([1, 2, 3], labels=[0, 1], train_flag=True)
    with pytest.raises(ValueError):
        fused.chosen([1, 2, 3], labels=[0, 1, 2], train_flag=True)
    with pytest.raises(ValueError):
        fused.chosen(labels=labels[:-1], train_flag=True)
    ch = fused.chosen(np.zeros(0, np.int64), labels=np.zeros(0, np.int64), train_flag=True)
    assert ch.has_minority and ch.minor_offsets.shape == (3, 1) and ch.minor_ids.numel() == 0


def test_explain_nodes_train(fused, synth):
    from pcgnn_amd import utils as U
    _, labels, csrs, train_pos, _ = synth
    ids = np.array([5, 7, 11, train_pos[3]])
    ch, prob = U.explain_nodes(fused, ids, labels=labels[ids])
    assert_same_train(ch, engine_ref(fused, csrs, ids, labels[ids], train_pos))
    assert torch.equal(prob, torch.sigmoid(fused.infer(ids)).float())
    assert not U.explain_nodes(fused, ids)[0].has_minority


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_engine_golden_graphs(name):
    import pcgnn_amd as PK
    from pcgnn_amd.fused import FusedPCGNN
    c = GoldenCase(name)
    g = PK.DeviceGraph(c.X, c.csr, c.train_pos, dev())
    fz = FusedPCGNN(build_model(PK, c, 0.5, graph=g), c.lr, c.wd, max_batch=256)
    ids, lab = np.asarray(c.nodes), c.batch_labels
    ch = fz.chosen(ids, labels=lab, train_flag=True)
    ref = engine_ref(fz, c.csr, ids, lab, c.train_pos)
    assert_same_train(ch, ref)
    assert_same_train(fz.chosen(ids, chunk=64, labels=lab, train_flag=True), ref, "chunk = 64")
    # its sets are the reference's own train-mode selection (the device's scores rank these tie-free cuts as the reference's do)
    for r in range(c.R):
        assert ch.to_reference(r)[0] == c.sel("rho0.5_train", r)


def test_engine_no_train_positives_and_rho_zero(synth):
    X, labels, csrs, train_pos, _ = synth
    ids = np.arange(0, 3000, 7)
    for tp, rho in (([], 0.5), (train_pos, 0.0)):
        fz = engine(X, csrs, tp, 32, rho, seed=2)
        ch = fz.chosen(ids, labels=labels[ids], train_flag=True)
        assert ch.has_minority and ch.minor_ids.numel() == 0 and int(ch.minor_flat_offsets.abs().sum()) == 0
        assert_same_train(ch, engine_ref(fz, csrs, ids, labels[ids], tp))
        assert ch.to_reference(1)[0] == fz.chosen(ids).to_reference(1)[0]


def test_training_state_is_left_alone(synth):
    """train_step, chosen(train_flag=True), train_step == train_step, train_step on a twin that never called chosen"""
    X, labels, csrs, train_pos, _ = synth
    a, b = (engine(X, csrs, train_pos, 64, 0.5, seed=1) for _ in range(2))
    b.theta.copy_(a.theta)
    b.params_changed()
    ids = torch.as_tensor(np.random.RandomState(12).randint(0, 3000, size=256), dtype=torch.int32, device=dev())
    lab = torch.as_tensor(labels[ids.cpu().numpy()].astype(np.int32), device=dev())
    for t in (a, b):
        t.train_step(ids, lab)
    keys, s0 = a.keys.clone(), a.s0.clone()
    sub = np.arange(0, 3000, 3)
    ch = a.chosen(sub, labels=labels[sub], train_flag=True)
    b.flush()
    torch.cuda.synchronize()
    assert torch.equal(a.keys, keys) and torch.equal(a.s0, s0) and a._inf["pos_keys"].data_ptr() != a.keys.data_ptr()
    assert_same_train(ch, engine_ref(a, csrs, sub, labels[sub], train_pos))
    for t in (a, b):
        t.train_step(ids, lab)
        t.flush()
    torch.cuda.synchronize()
    for name in ("theta", "m", "v", "step_counter"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    a.check()


# ---- the reference's own numbers and names ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ranked_train_npz():
    return np.load(os.path.join(GOLDEN, "ranked_train.npz"))


@pytest.mark.parametrize("rho", [0.2, 0.5, 2.0])
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_golden_choose_ranked_train(ranked_train_npz, name, rho):
    import pcgnn_amd as PK
    from pcgnn_amd import ops
    c = GoldenCase(name)
    g = PK.DeviceGraph(c.X, c.csr, c.train_pos, dev())
    s0, center = golden_scores(ranked_train_npz, c)
    thr = [0.5] * c.R
    ch = ops.choose_ranked(g, np.asarray(c.nodes), torch.from_numpy(s0).to(dev()), thr,
                           center_s0=torch.from_numpy(center).to(dev()), labels=c.batch_labels, rho=rho)
    neigh = tuple(t.cpu().numpy() for t in ch)
    minor = (ch.minor_offsets.cpu().numpy(), ch.minor_ids.cpu().numpy(), ch.minor_dist.cpu().numpy())
    compare_train_with_golden(ranked_train_npz, c, rho, neigh, minor, thr)


def reference_call_args(c, r, z):
    """choose_step_neighs' arguments as the reference's InterAgg forms them (layers.py:246-262) from the golden scores"""
    s0, center = golden_scores(z, c)
    scores = torch.from_numpy(np.stack([s0, np.zeros_like(s0)], 1))
    adj = c.adj(r)
    neighs_list = [list(adj[int(v)]) for v in c.nodes]
    center_scores = torch.from_numpy(np.stack([center, np.zeros_like(center)], 1))
    neigh_scores = [scores[torch.as_tensor(l)].view(-1, 2) for l in neighs_list]
    minor_scores = scores[torch.as_tensor(c.train_pos)]
    sample_list = z[f"{c.name}_sample_list{r}"].tolist()
    return center_scores, torch.from_numpy(c.batch_labels), neigh_scores, neighs_list, minor_scores, list(c.train_pos), sample_list


def check_reference_shape(c, r, rho, z, args, sets, scores):
    """(samp_neighs, samp_scores) against the reference's: a keep-all row's neighbour part in the caller's list order, a ranked
    row's ascending, the minority tail after it - every row bit for bit"""
    cs, lab, ns, nl, ms, ml, sl = args
    want = golden_train_rows(z, c.name, rho, r)
    have_sets = f"rho{rho}_train_sel_off0" in c.z.files
    want_sets = c.sel(f"rho{rho}_train", r) if have_sets else None
    assert len(sets) == len(scores) == len(c.nodes)
    for b in range(len(c.nodes)):
        assert isinstance(sets[b], set) and isinstance(scores[b], list)
        assert len(sets[b]) == int(z[f"{c.name}_rho{rho}_set_len{r}"][b])
        if have_sets:
            assert sets[b] == want_sets[b]
        got = np.asarray(scores[b], dtype=np.float64).astype(np.float32)
        deg = len(nl[b])
        if deg > sl[b] + 1:
            assert np.array_equal(got.view(np.uint32), want[b].view(np.uint32)), (c.name, rho, r, b)
        else:       # (the reference's list order here is its own set-iteration order: compare with the caller's, and the tail)
            assert scores[b][:deg] == torch.abs(cs[b, 0] - ns[b][:, 0]).tolist(), (c.name, rho, r, b)
            assert np.array_equal(got[deg:].view(np.uint32), want[b][deg:].view(np.uint32)), (c.name, rho, r, b)
            assert np.array_equal(np.sort(got[:deg]).view(np.uint32), np.sort(want[b][:deg]).view(np.uint32))


@pytest.mark.parametrize("name,rho", [("yelp_small", 0.2), ("yelp_small", 2.0), ("single_rel", 0.5), ("five_rel", 0.5), ("five_rel", 2.0)])
def test_reference_name_choose_step_neighs(ranked_train_npz, name, rho):
    from pcgnn_amd import layers
    c = GoldenCase(name)
    for r in range(c.R):
        args = reference_call_args(c, r, ranked_train_npz)
        before = [list(l) for l in args[3]]
        sets, scores = layers.choose_step_neighs(*args, rho)
        assert args[3] == before, "the caller's lists are left alone"
        check_reference_shape(c, r, rho, ranked_train_npz, args, sets, scores)


def test_reference_name_intra_agg_forward_train(ranked_train_npz):
    import pcgnn_amd as PK
    c = GoldenCase("single_rel")
    feats = torch.nn.Embedding(c.n, c.f)
    feats.weight = torch.nn.Parameter(torch.from_numpy(c.X), requires_grad=False)
    agg = PK.IntraAgg(feats, c.f, c.emb, c.train_pos, 0.5, cuda=True).to(dev())
    args = reference_call_args(c, 0, ranked_train_npz)
    cs, lab, ns, nl, ms, ml, sl = args
    out0, none = agg(c.nodes, lab, nl, cs, ns, ms, sl, True)
    assert none is None                                                   # as before, unless asked for
    agg.train_samp_scores = True
    out1, samp_scores = agg(c.nodes, lab, nl, cs, ns, ms, sl, True)
    assert torch.equal(out0, out1), "the first value is unchanged"
    sets = [set(s) for s in c.sel("rho0.5_train", 0)]
    check_reference_shape(c, 0, 0.5, ranked_train_npz, args, sets, samp_scores)
    out2, test_scores = agg(c.nodes, lab, nl, cs, ns, ms, sl, False)      # the test-mode path does not change
    assert out2.shape == out1.shape and len(test_scores) == len(c.nodes)
    assert all(len(t) <= len(s) for t, s in zip(test_scores, samp_scores))
