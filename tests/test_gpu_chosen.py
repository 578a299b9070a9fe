"""FusedPCGNN.chosen / ops.choose_ranked / pcg_rank_lists: the chosen neighbours in the reference's order with their distances.
The oracle is tests/ranked_ref.py (pinned to the reference's own samp_scores by test_ranked_ref_golden.py), fed the very scores
the device used - so every comparison is exact: np.array_equal on ids and on the distances' bit patterns."""
import math
import os

import numpy as np
import pytest
import torch

from tests.ranked_ref import compare_with_golden, ranked_ref
from tests.util import GOLDEN, GoldenCase, csr_to_adj, synth_graph

pytestmark = pytest.mark.gpu

RANK_SLICE = 2048          # rank.hip: the one-workgroup limit (keys of one slice)
GOLDEN_CASES = ["yelp_small", "single_rel", "five_rel"]


def dev():
    return torch.device("cuda", 0)


def assert_same(ch, ref, what=""):
    """a ChosenLists against ranked_ref's (offsets, ids, dist): exact"""
    off, ids, dist = ref
    assert np.array_equal(ch.offsets.cpu().numpy(), off), what
    assert np.array_equal(ch.ids.cpu().numpy(), ids), what
    assert np.array_equal(ch.dist.cpu().numpy().view(np.uint32), dist.view(np.uint32)), what


# ---- explicit rows at every boundary --------------------------------------------------------------------------------------
# threshold 0.5: degrees 0 .. 3 keep everything, 4 is the first ranked row (k = 2); kept counts 63 / 64 / 65 around the wave
# tier's limit; RANK_SLICE - 1 / exact / + 1 around the one-workgroup limit; two slices exactly, three slices; a hub of 30 000
# (15 000 kept = eight slices; beyond the select kernel's LDS key capacity: its long-row launch)
DEGS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 33, 63, 64, 65, 126, 128, 130, 512, 513, 1024, 2 * RANK_SLICE - 2, 2 * RANK_SLICE,
        2 * RANK_SLICE + 2, 4 * RANK_SLICE, 10000, 4097, 30000]
N_EXPLICIT = 32768


@pytest.fixture(scope="module")
def explicit():
    import pcgnn_amd as P
    rs = np.random.RandomState(11)
    indptr = np.zeros(N_EXPLICIT + 1, dtype=np.int64)
    indptr[1:len(DEGS) + 1] = np.cumsum(DEGS)
    indptr[len(DEGS) + 1:] = indptr[len(DEGS)]
    idx = np.concatenate([np.sort(rs.choice(N_EXPLICIT, size=d, replace=False)) for d in DEGS]).astype(np.int32)
    X = rs.randn(N_EXPLICIT, 8).astype(np.float32)
    csr = [(indptr, idx)]
    g = P.DeviceGraph(X, csr, [], dev())
    assert g.max_degree == 30000
    nodes = np.arange(len(DEGS))
    return g, csr, nodes, rs.randn(N_EXPLICIT).astype(np.float32)


def test_rows_at_every_boundary(explicit):
    from pcgnn_amd import ops
    g, csr, nodes, s0 = explicit
    kept = [d if not d > math.ceil(d * 0.5) + 1 else math.ceil(d * 0.5) for d in DEGS]
    for want in (0, 1, 2, 3, 63, 64, 65, RANK_SLICE - 1, RANK_SLICE, RANK_SLICE + 1, 2 * RANK_SLICE, 5000, 15000):
        assert want in kept
    ch = ops.choose_ranked(g, nodes, torch.from_numpy(s0).to(dev()), [0.5])
    ref = ranked_ref(csr, nodes, s0, [0.5])
    assert np.diff(ref[0][0]).tolist() == kept
    assert_same(ch, ref)
    # the same rows in another order, a centre twice, explicit centre scores
    perm = np.random.RandomState(3).permutation(len(DEGS)).tolist() + [len(DEGS) - 1, 4]
    cen = np.random.RandomState(4).randn(len(perm)).astype(np.float32)
    ch = ops.choose_ranked(g, np.array(perm), torch.from_numpy(s0).to(dev()), [0.5], center_s0=torch.from_numpy(cen).to(dev()))
    assert_same(ch, ranked_ref(csr, perm, s0, [0.5], center=cen))


def test_exact_ties(explicit):
    """scores quantised to 8 values: every cut and most ranks are ties - order by list position"""
    from pcgnn_amd import ops
    g, csr, nodes, _ = explicit
    s0 = (np.random.RandomState(5).randint(0, 8, size=N_EXPLICIT) / 8.0).astype(np.float32)
    ch = ops.choose_ranked(g, nodes, torch.from_numpy(s0).to(dev()), [0.5])
    ref = ranked_ref(csr, nodes, s0, [0.5])
    assert len(np.unique(ref[2])) <= 8
    assert_same(ch, ref)


@pytest.mark.parametrize("thr", [0.2, 1.0])
def test_thresholds_explicit(explicit, thr):
    """0.2: other cuts; 1.0: every row keeps everything (list order, the hub over fifteen slices)"""
    from pcgnn_amd import ops
    g, csr, nodes, s0 = explicit
    ch = ops.choose_ranked(g, nodes, torch.from_numpy(s0).to(dev()), [thr])
    ref = ranked_ref(csr, nodes, s0, [thr])
    if thr == 1.0:
        assert np.diff(ref[0][0]).tolist() == DEGS
    assert_same(ch, ref)


# ---- a synthetic three-relation graph ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synth():
    X, labels, csrs = synth_graph(1, 3000, 32, (3, 10, 40), 0.15)
    rs = np.random.RandomState(2)
    idx_train = np.sort(rs.choice(3000, size=1200, replace=False))
    train_pos = [int(v) for v in idx_train if labels[v] == 1]
    return X, labels, csrs, train_pos


def test_per_relation_thresholds(synth):
    import pcgnn_amd as P
    from pcgnn_amd import ops
    X, _, csrs, train_pos = synth
    g = P.DeviceGraph(X, csrs, train_pos, dev())
    s0 = np.random.RandomState(6).randn(3000).astype(np.float32)
    nodes = np.random.RandomState(7).randint(0, 3000, size=700)
    thr = [0.2, 0.5, 1.0]
    ch = ops.choose_ranked(g, nodes, torch.from_numpy(s0).to(dev()), thr)
    assert_same(ch, ranked_ref(csrs, nodes, s0, thr))


def engine(X, csrs, train_pos, emb, thresholds, seed=0):
    import pcgnn_amd as P
    from pcgnn_amd.fused import FusedPCGNN
    n, f = X.shape
    torch.manual_seed(seed)
    g = P.DeviceGraph(X, csrs, train_pos, dev())
    feats = torch.nn.Embedding(n, f)
    feats.weight = torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(X)), requires_grad=False)
    intras = [P.IntraAgg(feats, f, emb, train_pos, 0.5, cuda=True) for _ in csrs]
    inter = P.InterAgg(feats, f, emb, train_pos, g, intras, cuda=True)
    inter.thresholds = list(thresholds)
    return FusedPCGNN(P.PCALayer(2, inter, 2.0).cuda(), 0.01, 0.001, max_batch=256)


@pytest.fixture(scope="module")
def fused(synth):
    X, _, csrs, train_pos = synth
    return engine(X, csrs, train_pos, 64, [0.5, 0.5, 0.5])


def engine_ref(fz, csrs, ids):
    """ranked_ref on the scores the engine's last chosen / infer call used"""
    return ranked_ref(csrs, ids, fz._inf["s0"].cpu().numpy(), fz.thresholds)


def test_chosen_whole_graph(fused, synth):
    _, _, csrs, _ = synth
    ch = fused.chosen()
    ref = engine_ref(fused, csrs, np.arange(3000))
    assert_same(ch, ref)
    assert ch.offsets.shape == (3, 3001) and ch.ids.dtype == torch.int32 and ch.dist.dtype == torch.float32
    # the views, the per-relation diagnostic and the reference's return shape
    off, ids, dist = ref
    i, d = ch.row(2, 7)
    assert np.array_equal(i.cpu().numpy(), ids[off[2, 7]:off[2, 8]]) and np.array_equal(d.cpu().numpy(), dist[off[2, 7]:off[2, 8]])
    md = ch.mean_dist().cpu().numpy()
    want = np.array([[dist[off[r, b]:off[r, b + 1]].astype(np.float64).mean() for b in range(3000)] for r in range(3)])
    np.testing.assert_allclose(md, want, rtol=1e-6)
    sets, scores = ch.to_reference(1)
    assert len(sets) == len(scores) == 3000
    assert sets[7] == set(ids[off[1, 7]:off[1, 8]].tolist()) and scores[7] == dist[off[1, 7]:off[1, 8]].tolist()
    # the scores are the ones infer selects by
    fused.infer(np.arange(10))
    assert_same(ch, engine_ref(fused, csrs, np.arange(3000)))


@pytest.mark.parametrize("kind", ["tensor", "numpy", "list"])
def test_chosen_subset_with_duplicates(fused, synth, kind):
    _, _, csrs, _ = synth
    rs = np.random.RandomState(8)
    ids = np.concatenate([rs.randint(0, 3000, size=500), [7, 7, 2999, 0, 7]])
    rs.shuffle(ids)
    arg = torch.from_numpy(ids).to(dev()) if kind == "tensor" else (ids if kind == "numpy" else ids.tolist())
    assert_same(fused.chosen(arg), engine_ref(fused, csrs, ids))


def test_chosen_chunks(fused, synth):
    _, _, csrs, _ = synth
    ids = np.random.RandomState(9).randint(0, 3000, size=1000)
    want = engine_ref(fused, csrs, ids)                    # (the parameters do not change: the scores of the last call)
    assert_same(fused.chosen(ids, chunk=130), want, "many chunks, a tail of 90")
    assert_same(fused.chosen(ids[:40], chunk=1), engine_ref(fused, csrs, ids[:40]), "chunk = 1")
    assert_same(fused.chosen(ids, chunk=1000), want)
    assert_same(fused.chosen(ids), want)


def test_chosen_empty_and_range(fused):
    ch = fused.chosen(np.zeros(0, np.int64))
    assert ch.offsets.shape == (3, 1) and ch.ids.numel() == 0 and ch.dist.numel() == 0
    assert ch.mean_dist().shape == (3, 0)
    with pytest.raises(ValueError):
        fused.chosen([0, 3000])
    with pytest.raises(ValueError):
        fused.chosen([-1])


def test_chosen_sets_equal_chosen_sets(fused, synth):
    from pcgnn_amd import ops
    ids = np.random.RandomState(10).randint(0, 3000, size=300)
    ch = fused.chosen(ids)
    idt = torch.from_numpy(ids.astype(np.int32)).to(dev())
    sets, _, _ = ops.chosen_sets(fused.g, idt, None, fused._inf["s0"], None, fused.thresholds, fused.rho, False)
    for r in range(3):
        got, _ = ch.to_reference(r)
        assert got == sets[r]


def test_explain_nodes(fused):
    from pcgnn_amd import utils as U
    ids = [5, 7, 11]
    ch, prob = U.explain_nodes(fused, ids)
    assert ch.n == 3 and torch.equal(prob, torch.sigmoid(fused.infer(ids)).float())


# ---- the training engine is left alone ------------------------------------------------------------------------------------
def test_training_engine_untouched():
    """a group, chosen, two more groups == a group, flush, two more groups - bit for bit; no re-capture, no re-allocation"""
    from pcgnn_amd import synth as S
    from pcgnn_amd.handler import PCGNNTrainer
    w = S.make_workload("mini", 6000, 32, (4000, 30000, 90000), 0.12, seed=3)
    mk = lambda: PCGNNTrainer(w, dict(engine="graph", seed=5, batch_size=256), dev())
    a, b = mk(), mk()
    b.fused.theta.copy_(a.fused.theta)
    b.fused.params_changed()
    for t in (a, b):
        t.run_epoch_one_graph(n_epochs=2)
    maxB, graphs, fresh = a.fused.maxB, dict(a.fused._ep_graphs), a.fused._fresh
    s0, keys = a.fused.s0.clone(), a.fused.keys.clone() if hasattr(a.fused, "keys") else None
    ch = a.fused.chosen(np.arange(0, 6000, 7), chunk=130)
    a.fused.chosen()
    b.fused.flush()
    torch.cuda.synchronize()
    assert a.fused._fresh == fresh and torch.equal(a.fused.s0, s0)
    if keys is not None:
        assert torch.equal(a.fused.keys, keys)
    assert_same(ch, ranked_ref(w.csr, np.arange(0, 6000, 7), a.fused._inf["s0"].cpu().numpy(), a.fused.thresholds))
    for t in (a, b):
        for _ in range(2):
            t.run_epoch_one_graph(n_epochs=2)
    torch.cuda.synchronize()
    for name in ("theta", "m", "v", "step_counter", "clf_next"):
        assert torch.equal(getattr(a.fused, name), getattr(b.fused, name)), name
    assert a.fused.maxB == maxB
    assert set(a.fused._ep_graphs) == set(graphs) and len(b.fused._ep_graphs) == len(graphs)
    assert all(a.fused._ep_graphs[k] is gr for k, gr in graphs.items())
    a.fused.check()


def test_train_step_parameters_unchanged_by_chosen(synth):
    """train_step, chosen, train_step == train_step, train_step"""
    X, labels, csrs, train_pos = synth
    a, b = (engine(X, csrs, train_pos, 64, [0.5, 0.5, 0.5], seed=1) for _ in range(2))
    b.theta.copy_(a.theta)
    b.params_changed()
    ids = torch.as_tensor(np.random.RandomState(12).randint(0, 3000, size=256), dtype=torch.int32, device=dev())
    lab = torch.as_tensor(labels[ids.cpu().numpy()].astype(np.int32), device=dev())
    for t in (a, b):
        t.train_step(ids, lab)
    a.chosen(np.arange(100))
    for t in (a, b):
        t.train_step(ids, lab)
        t.flush()
    torch.cuda.synchronize()
    for name in ("theta", "m", "v", "step_counter"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


# ---- the reference's own numbers --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ranked_npz():
    return np.load(os.path.join(GOLDEN, "ranked.npz"))


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_golden_choose_ranked(ranked_npz, name):
    import pcgnn_amd as P
    from pcgnn_amd import ops
    c = GoldenCase(name)
    g = P.DeviceGraph(c.X, c.csr, c.train_pos, dev())
    s0 = np.ascontiguousarray(c.z["table_scores"][:, 0])
    thr = [0.5] * c.R
    ch = ops.choose_ranked(g, np.asarray(c.nodes), torch.from_numpy(s0).to(dev()), thr)
    off, ids, dist = (t.cpu().numpy() for t in ch)
    compare_with_golden(ranked_npz, c, off, ids, dist, thr)
    # on every row dist[j] == |c - s[ids[j]]|
    st = torch.from_numpy(s0)
    B = len(c.nodes)
    cen = st[torch.as_tensor(c.nodes)].repeat(c.R)                                  # row r * B + b
    per_entry = torch.repeat_interleave(cen, torch.from_numpy(np.diff(ch.host_offsets())))
    want = torch.abs(per_entry - st[torch.from_numpy(ids.astype(np.int64))]).numpy()
    assert np.array_equal(dist.view(np.uint32), want.view(np.uint32))
    assert off.shape == (c.R, B + 1)


def reference_call_args(c, r, ranked_npz):
    """choose_step_test's arguments as the reference's InterAgg forms them (layers.py:246-262) from the golden score table"""
    scores = torch.from_numpy(np.ascontiguousarray(c.z["table_scores"]))
    adj = c.adj(r)
    neighs_list = [list(adj[int(v)]) for v in c.nodes]
    center_scores = scores[torch.as_tensor(c.nodes)]
    neigh_scores = [scores[torch.as_tensor(l)].view(-1, 2) for l in neighs_list]
    sample_list = ranked_npz[f"{c.name}_sample_list{r}"].tolist()
    return center_scores, neigh_scores, neighs_list, sample_list


def check_reference_shape(c, r, ranked_npz, sets, scores):
    off, flat = ranked_npz[f"{c.name}_score_off{r}"], ranked_npz[f"{c.name}_scores{r}"]
    want_sets = c.sel("test", r)
    indptr, _ = c.csr[r]
    assert len(sets) == len(scores) == len(c.nodes)
    for b, v in enumerate(c.nodes):
        want = flat[off[b]:off[b + 1]]
        got = np.asarray(scores[b], dtype=np.float64).astype(np.float32)
        deg = int(indptr[v + 1] - indptr[v])
        assert isinstance(sets[b], set) and isinstance(scores[b], list)
        assert sets[b] == want_sets[b]
        if deg > math.ceil(deg * 0.5) + 1:
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (c.name, r, b)
        else:
            assert np.array_equal(np.sort(got).view(np.uint32), np.sort(want).view(np.uint32)), (c.name, r, b)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_reference_name_choose_step_test(ranked_npz, name):
    from pcgnn_amd import layers
    c = GoldenCase(name)
    for r in range(c.R):
        args = reference_call_args(c, r, ranked_npz)
        sets, scores = layers.choose_step_test(*args)
        check_reference_shape(c, r, ranked_npz, sets, scores)
        # a keep-all row comes back in the caller's list order, as the reference returns it
        cs, ns, nl, sl = args
        for b in range(len(nl)):
            if not len(nl[b]) > sl[b] + 1:
                want = torch.abs(cs[b, 0] - ns[b][:, 0]).tolist()
                assert scores[b] == want, (name, r, b)


def test_reference_name_intra_agg_forward(ranked_npz):
    import pcgnn_amd as P
    c = GoldenCase("single_rel")
    feats = torch.nn.Embedding(c.n, c.f)
    feats.weight = torch.nn.Parameter(torch.from_numpy(c.X), requires_grad=False)
    agg = P.IntraAgg(feats, c.f, c.emb, c.train_pos, 0.5, cuda=True).to(dev())    # (the attribute `cuda` shadows Module.cuda, as in the reference)
    cs, ns, nl, sl = reference_call_args(c, 0, ranked_npz)
    pos_scores = torch.from_numpy(np.ascontiguousarray(c.z["table_scores"]))[torch.as_tensor(c.train_pos)]
    out, samp_scores = agg(c.nodes, torch.from_numpy(c.batch_labels), nl, cs, ns, pos_scores, sl, False)
    assert out.shape == (len(c.nodes), c.emb)
    check_reference_shape(c, 0, ranked_npz, c.sel("test", 0), samp_scores)
    out_t, none = agg(c.nodes, torch.from_numpy(c.batch_labels), nl, cs, ns, pos_scores, sl, True)
    assert none is None and out_t.shape == out.shape


# ---- the status word ------------------------------------------------------------------------------------------------------------
def test_rank_mismatch_is_reported_and_nothing_leaves_an_extent(explicit):
    """an extent one short for one row (through the argument only): the bit is set, the row is not written, every other row
    is, and the guard words around the output stay intact"""
    from pcgnn_amd import _lib, ops
    from pcgnn_amd.fused import FusedPCGNN
    g, csr, nodes, s0h = explicit
    s0 = torch.from_numpy(s0h).to(dev())
    idt = torch.from_numpy(nodes.astype(np.int32)).to(dev())
    B = len(nodes)
    caps = ops.sel_capacity(g, nodes, None, [0.5], 0.0, False)
    assert caps.shape == (1, B)
    ws = ops.ChooseWorkspace(g, B, list_capacity=int(caps.sum()))
    cnt = torch.empty(B, dtype=torch.int32, device=dev())
    ops.choose_select(g, idt, None, s0, None, [0.5], 0.0, False, ws, cnt)
    ref_off, ref_ids, ref_dist = ranked_ref(csr, nodes, s0h, [0.5])
    GUARD = 64
    for short in (DEGS.index(5), DEGS.index(130), DEGS.index(10000)):          # a wave row, a one-workgroup row, a sliced row
        bad = caps.copy()
        bad[0, short] -= 1
        off = ops.rank_offsets(bad)
        total = int(off[-1])
        ids_buf = torch.full((total + 2 * GUARD,), -7, dtype=torch.int32, device=dev())
        dist_buf = torch.full((total + 2 * GUARD,), -1.0, dtype=torch.float32, device=dev())
        ops.rank_lists(g, idt, s0, ws, torch.from_numpy(off).to(dev()), ids_buf[GUARD:GUARD + total], dist_buf[GUARD:GUARD + total])
        st = int(ws.status.item())
        ws.status.zero_()
        assert st == _lib.PCG_ST_RANK_MISMATCH
        with pytest.raises(_lib.PcgnnLibraryError, match="rank_lists"):
            FusedPCGNN._raise_status(st)
        ids, dist = ids_buf.cpu().numpy(), dist_buf.cpu().numpy()
        for buf, fill in ((ids, -7), (dist, -1.0)):
            assert (buf[:GUARD] == fill).all() and (buf[GUARD + total:] == fill).all()
        for b in range(B):
            lo, hi = GUARD + int(off[b]), GUARD + int(off[b + 1])
            if b == short:
                assert (ids[lo:hi] == -7).all() and (dist[lo:hi] == -1.0).all()
            else:
                assert np.array_equal(ids[lo:hi], ref_ids[ref_off[0, b]:ref_off[0, b + 1]])
                assert np.array_equal(dist[lo:hi].view(np.uint32), ref_dist[ref_off[0, b]:ref_off[0, b + 1]].view(np.uint32))
    ws.check()
