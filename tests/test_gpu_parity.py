"""GPU parity tests: the HIP path (through the C ABI) against the oracle and the
golden vectors captured from the reference.  Run with ``pytest -m gpu`` on an MI355X.

Bars: chosen index sets bit-exact (given the same class-0 scores); floats within
the tolerance written at each assert (north_star: logits within 1e-4 fp32).
"""
import math
import os

import numpy as np
import pytest
import torch

from oracle import pcgnn_oracle as O
from tests import dense_ref as D
from tests.util import GOLDEN, PARAM_KEYS, GoldenCase, build_model, csr_to_adj, synth_graph

pytestmark = pytest.mark.gpu

CASES = ["yelp_small", "amazon_small", "single_rel", "yelp_emb128", "feat100", "five_rel"]   # emb128 / feat100 / five_rel: dense_step_kernel<false>
LOGIT_TOL = 1e-4     # north_star tolerance for logits
FEAT_TOL = 2e-5      # aggregated features / activations


@pytest.fixture(scope="module")
def P():
    import pcgnn_amd
    from pcgnn_amd import ops  # noqa: F401  (fails loudly if the .so is missing)
    return pcgnn_amd


@pytest.fixture(scope="module", params=CASES)
def case(request):
    return GoldenCase(request.param)


def dev():
    return torch.device("cuda", 0)


def graph_of(P, c):
    return P.DeviceGraph(c.X, c.csr, c.train_pos, dev())


# ---------------------------------------------------------------------------
def test_library_loaded(P):
    from pcgnn_amd import _lib
    assert _lib.load().pcg_version().startswith(b"pcgnn_hip gfx950")


def test_score_table_and_rows(P, case):
    c, ops = case, P.ops
    g = graph_of(P, c)
    W = c.params()["inter1.label_clf.weight"].cuda()
    b = c.params()["inter1.label_clf.bias"].cuda()
    s0 = ops.score_table(g, W, b)
    ref = c.z["table_scores"]
    np.testing.assert_allclose(s0.cpu().numpy(), ref[:, 0], rtol=0, atol=2e-6)
    ids = torch.arange(c.n, dtype=torch.int32, device=dev())
    both = ops.score_rows(g, W, b, ids)
    assert torch.equal(both[:, 0], s0), "score_rows column 0 must be bit-identical to score_table"
    np.testing.assert_allclose(both.cpu().numpy(), ref, rtol=0, atol=2e-6)
    # partial range leaves the rest untouched
    out = torch.full((c.n,), 7.0, device=dev())
    ops.score_table(g, W, b, out=out, row_begin=10, row_end=20)
    assert torch.equal(out[10:20], s0[10:20]) and float(out[:10].min()) == 7.0 and float(out[20:].max()) == 7.0


def test_pos_sort(P, case):
    c, ops = case, P.ops
    g = graph_of(P, c)
    s0 = torch.from_numpy(c.z["table_scores"][:, 0].copy()).cuda()
    keys = ops.pos_sort(g, s0).cpu().numpy().view(np.uint64)
    n = len(c.train_pos)
    assert np.all(keys[n:len(keys) // 2] == np.uint64(0xFFFFFFFFFFFFFFFF))     # (the second half of the buffer is scratch)
    pos = (keys[:n] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    sc = c.z["table_scores"][np.array(c.train_pos), 0]
    order = np.lexsort((np.arange(n), sc))       # by score, then position
    assert np.array_equal(pos, order)


def test_chosen_sets_bit_exact_golden(P, case):
    """Feed the reference's own class-0 scores: the chosen sets must be identical."""
    c, ops = case, P.ops
    g = graph_of(P, c)
    s0 = torch.from_numpy(c.z["table_scores"][:, 0].copy()).cuda()
    keys = ops.pos_sort(g, s0)
    nodes = torch.tensor(c.nodes, dtype=torch.int32, device=dev())
    labels = torch.from_numpy(c.batch_labels.astype(np.int32)).cuda()
    X = torch.from_numpy(c.X)
    for rho in c.rhos:
        sets, agg, cnt = ops.chosen_sets(g, nodes, labels, s0, keys, [0.5] * c.R, rho, True)
        for r in range(c.R):
            want = c.sel(f"rho{rho}_train", r)
            assert sets[r] == want, f"{c.name} rho={rho} rel={r}"
            assert cnt[r].cpu().tolist() == [len(s) for s in want]
            np.testing.assert_allclose(agg[r].cpu().numpy(), O.sparse_aggregate(want, X).numpy(), rtol=0, atol=FEAT_TOL)
    sets, agg, cnt = ops.chosen_sets(g, nodes, None, s0, None, [0.5] * c.R, 0.5, False)
    for r in range(c.R):
        assert sets[r] == c.sel("test", r)


def test_forward_matches_reference(P, case):
    c = case
    for rho in c.rhos:
        m = build_model(P, c, rho)
        logits, cs = m.forward(c.nodes, torch.from_numpy(c.batch_labels).cuda(), True)
        key = f"rho{rho}_train"
        got_sets = m.inter1.chosen_sets(c.nodes, c.batch_labels, True)
        for r in range(c.R):
            assert got_sets[r] == c.sel(key, r)
        np.testing.assert_allclose(logits.detach().cpu().numpy(), c.z[key + "_logits"], rtol=0, atol=LOGIT_TOL)
        np.testing.assert_allclose(cs.detach().cpu().numpy(), c.z[key + "_center_scores"], rtol=0, atol=1e-5)
    m = build_model(P, c, c.rhos[0])
    gp, _ = m.to_prob(c.nodes, c.batch_labels, train_flag=False)
    np.testing.assert_allclose(gp.detach().cpu().numpy(), c.z["test_gnn_prob"], rtol=0, atol=LOGIT_TOL)
    comb, _ = m.inter1(c.nodes, c.batch_labels, False)
    assert tuple(comb.shape) == (c.emb, len(c.nodes))
    np.testing.assert_allclose(comb.detach().cpu().numpy(), c.z["test_combined"], rtol=0, atol=FEAT_TOL)


def test_loss_grads_adam_match_reference(P, case):
    c = case
    rho = c.rhos[0]
    tag = f"rho{rho}"
    m = build_model(P, c, rho)
    opt = torch.optim.Adam(filter(lambda p: p.requires_grad, m.parameters()), lr=c.lr, weight_decay=c.wd)
    opt.zero_grad()
    loss = m.loss(c.nodes, torch.from_numpy(c.batch_labels).cuda())
    loss.backward()
    assert abs(loss.item() - float(c.z[tag + "_loss"])) < LOGIT_TOL
    named = dict(m.named_parameters())
    for k in PARAM_KEYS(c.R):
        np.testing.assert_allclose(named[k].grad.cpu().numpy(), c.z[f"{tag}_grad_{k}"], rtol=0, atol=2e-5, err_msg=k)
    opt.step()
    sd = m.state_dict()
    for k in PARAM_KEYS(c.R):
        np.testing.assert_allclose(sd[k].cpu().numpy(), c.z[f"{tag}_step_{k}"], rtol=0, atol=c.lr * 5e-2, err_msg=k)
    # state-dict names of the reference, incl. the frozen feature table copies
    keys = set(sd.keys())
    assert {"weight", "inter1.weight", "inter1.features.weight", "inter1.label_clf.weight",
            "inter1.label_clf.bias", "inter1.intra_agg1.weight", "inter1.intra_agg1.features.weight"} <= keys


def test_pick_golden(P, case):
    c, ops = case, P.ops
    idx_train = c.z["idx_train"]
    y = c.labels[idx_train]
    indptr, _ = c.homo_csr
    deg = np.diff(indptr)[idx_train]
    lf = (y.sum() - len(y)) * y + len(y)
    cum = np.cumsum(deg / lf)
    out = ops.pick(torch.from_numpy(cum).cuda(), torch.from_numpy(idx_train.astype(np.int32)).cuda(),
                   len(c.z["pick_uniforms"]), uniforms=torch.from_numpy(c.z["pick_uniforms"]).cuda())
    assert out.cpu().tolist() == c.z["pick_out"].tolist()


def test_pick_shuffled_is_a_shuffle_of_pick(P):
    """pcg_pick_shuffled = pcg_pick's draws of the same (seed, epoch) in a random order, with their labels; the
    device epoch counter advances by one per call."""
    ops = P.ops
    rs = np.random.RandomState(3)
    n_nodes, n_train = 50000, 18000
    idx_train = np.sort(rs.choice(n_nodes, size=n_train, replace=False)).astype(np.int32)
    labels = (rs.rand(n_nodes) < 0.15).astype(np.int32)
    cum = torch.from_numpy(np.cumsum(rs.randint(1, 50, size=n_train) / 7.0)).cuda()
    idx_d, lab_d = torch.from_numpy(idx_train).cuda(), torch.from_numpy(labels).cuda()
    counter = torch.zeros(2, dtype=torch.int64, device=dev())
    orders = []
    for k in (1, 63, 5346, 20000):
        out_ids = torch.full((k,), -1, dtype=torch.int32, device=dev())
        out_lab = torch.full((k,), -1, dtype=torch.int32, device=dev())
        e0 = int(counter[0].item())
        ops.pick_shuffled(cum, idx_d, k, 11, 100, out_ids, lab_d, out_lab, counter, bump=True)
        ref = ops.pick(cum, idx_d, k, None, 11, 100 + e0)
        assert int(counter[0].item()) == e0 + 1 and int(counter[1].item()) == 0
        a, b = out_ids.cpu().numpy(), ref.cpu().numpy()
        assert np.array_equal(np.sort(a), np.sort(b))                      # same draws ...
        assert np.array_equal(out_lab.cpu().numpy(), labels[a])            # ... with their labels
        if k > 1000:
            assert not np.array_equal(a, b)                                # ... in another order
            orders.append(a)
    # a different epoch gives different draws
    out2 = torch.empty(5346, dtype=torch.int32, device=dev())
    ops.pick_shuffled(cum, idx_d, 5346, 11, 100, out2, None, None, counter, bump=False)
    assert not np.array_equal(np.sort(out2.cpu().numpy()), np.sort(orders[0]))


def test_kat(P):
    z = np.load(os.path.join(GOLDEN, "kat.npz"))
    ops = P.ops
    # KAT 1: centre node 0 (score 0) with neighbours 10..14
    n = 40
    X = np.random.RandomState(0).randn(n, 8).astype(np.float32)
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = 5
    g = P.DeviceGraph(X, [(indptr, np.array([10, 11, 12, 13, 14], dtype=np.int32))], [], dev())
    s0 = torch.zeros(n, device=dev())
    s0[10:15] = torch.tensor(z["kat1_s0"], dtype=torch.float32, device=dev())
    sets, _, _ = ops.chosen_sets(g, torch.tensor([0], dtype=torch.int32, device=dev()), None, s0, None, [0.5], 0.5, False)
    assert sorted(sets[0][0]) == z["kat1_out"].tolist()
    # KAT 2: positive centre (score 1.0), single neighbour 20, train_pos [20,31,32,33]
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = 1
    g = P.DeviceGraph(X, [(indptr, np.array([20], dtype=np.int32))], [20, 31, 32, 33], dev())
    s0 = torch.zeros(n, device=dev())
    s0[0] = 1.0
    s0[torch.tensor([20, 31, 32, 33], device=dev())] = torch.tensor(z["kat2_pos_s0"], dtype=torch.float32, device=dev())
    # the neighbour's own score in the KAT is 0.4 but node 20 is also a train-pos with score 1.5;
    # keep-all applies (deg 1), so only the minority part matters
    keys = ops.pos_sort(g, s0)
    for rho in (0.2, 0.5, 0.8, 2.0, 3.5):
        sets, _, _ = ops.chosen_sets(g, torch.tensor([0], dtype=torch.int32, device=dev()),
                                     torch.tensor([1], dtype=torch.int32, device=dev()), s0, keys, [0.5], rho, True)
        assert sorted(sets[0][0]) == z[f"kat2_out_rho{rho}"].tolist(), rho
    # KAT 3: keep-all table
    for deg, kept in zip(z["kat3_deg"].tolist(), z["kat3_kept"].tolist()):
        indptr = np.zeros(n + 1, dtype=np.int64)
        indptr[1:] = deg
        g = P.DeviceGraph(X, [(indptr, np.arange(20, 20 + deg, dtype=np.int32))], [], dev())
        s0 = torch.zeros(n, device=dev())
        s0[20:20 + deg] = torch.linspace(0.1, 1.0, deg).to(dev())
        _, _, cnt = ops.chosen_sets(g, torch.tensor([0], dtype=torch.int32, device=dev()), None, s0, None, [0.5], 0.5,
                                    False)
        assert int(cnt[0, 0]) == kept


# ---------------------------------------------------------------------------
# seeded synthetic graphs against the oracle (same device scores => bit-exact sets)
# ---------------------------------------------------------------------------
def oracle_sets(csr, n, nodes, labels, s0, train_pos, thr, rho, train):
    s0 = torch.from_numpy(s0)
    indptr, idx = csr
    lists = [idx[indptr[v]:indptr[v + 1]].tolist() for v in nodes]
    nscore = [s0[torch.as_tensor(l, dtype=torch.long)] for l in lists]
    return O.choose_sets(s0[torch.as_tensor(nodes, dtype=torch.long)], labels, lists, nscore, list(train_pos),
                         s0[torch.as_tensor(list(train_pos), dtype=torch.long)], thr, rho, train)


def hub_graph(seed, n, hub_degs, base_deg=6.0, feat=32):
    """Graph with explicit hub rows (node i gets hub_degs[i] neighbours) to drive the
    4-wave / 16-wave tiers (deg > 512 / > 4096), the global-scratch path (deg > 8192) and multi-chunk gathers."""
    X, labels, csrs = synth_graph(seed, n, feat, (base_deg,), 0.1, hub=False)
    indptr, idx = csrs[0]
    rs = np.random.RandomState(seed + 1)
    rows = [idx[indptr[v]:indptr[v + 1]] for v in range(n)]
    for v, d in enumerate(hub_degs):
        rows[v] = np.unique(np.concatenate([rs.choice(n, size=d, replace=False).astype(np.int32), [v]]))
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=indptr[1:])
    return X, labels, (indptr, np.concatenate(rows).astype(np.int32))


@pytest.mark.parametrize("quantize", [False, True])
def test_hub_rows_block_and_scratch_paths(P, quantize):
    ops = P.ops
    n = 120000
    # (> 10240: the long-row launch, keys in ITS LDS up to 32768 neighbours - 30000 / 20480 / 10241 / 32768 -, beyond that in global
    #  scratch: 70000 as a positive centre keeps 35000 ids, more than that LDS holds - they go to the list region -, 40000 as a
    #  negative one, 32769 on the boundary)
    hub_degs = [30000, 13000, 8193, 8192, 8191, 6000, 4097, 4096, 4095, 2500, 513, 512, 511, 257, 256, 255, 65, 64, 63, 20480, 10241,
                10240, 40000, 70000, 32769, 32768]
    X, labels, csr = hub_graph(11, n, hub_degs)
    if quantize:   # many exact distance ties: the positional tie-break must match the oracle
        X = np.round(X * 2) / 2
    train_pos = np.flatnonzero(labels[: n // 2] == 1)[:3000].tolist()
    g = P.DeviceGraph(X, [csr], train_pos, dev())
    W = torch.randn(2, 32, generator=torch.Generator().manual_seed(1)).cuda() * (0.25 if quantize else 1.0)
    if quantize:
        W = torch.round(W * 4) / 4
    b = torch.zeros(2).cuda()
    s0 = ops.score_table(g, W, b)
    keys = ops.pos_sort(g, s0)
    nodes = list(range(len(hub_degs))) + [0, 1, 777, 778]
    lab = ([1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1, 0, 1, 0] * 3)[:len(nodes)]
    assert lab[22] == 0 and lab[23] == 1          # (40000: a negative centre, 70000: a positive one)
    for rho in (0.5, 2.0):
        sets, agg, cnt = ops.chosen_sets(g, torch.tensor(nodes, dtype=torch.int32, device=dev()),
                                         torch.tensor(lab, dtype=torch.int32, device=dev()), s0, keys, [0.5], rho, True)
        want = oracle_sets(csr, n, nodes, lab, s0.cpu().numpy(), train_pos, 0.5, rho, True)
        for bidx in range(len(nodes)):
            assert sets[0][bidx] == want[bidx], f"row {bidx} (deg {len(csr[1][csr[0][nodes[bidx]]:csr[0][nodes[bidx]+1]])}) rho {rho}"
        np.testing.assert_allclose(agg[0].cpu().numpy(), O.sparse_aggregate(want, torch.from_numpy(X)).numpy(),
                                   rtol=0, atol=5e-5)
    sets, _, _ = ops.chosen_sets(g, torch.tensor(nodes, dtype=torch.int32, device=dev()), None, s0, None, [0.5], 0.5, False)
    want = oracle_sets(csr, n, nodes, None, s0.cpu().numpy(), train_pos, 0.5, 0.5, False)
    assert sets[0] == want
    # threshold 1.0: k = deg, so every row keeps ALL its neighbours (deg <= k + 1) - a positive centre longer than the LDS key
    # capacity then keeps deg > 10240 ids, not k: they must go to the list region, not into the 10240-word LDS buffer
    sets, _, _ = ops.chosen_sets(g, torch.tensor(nodes, dtype=torch.int32, device=dev()),
                                 torch.tensor(lab, dtype=torch.int32, device=dev()), s0, keys, [1.0], 0.5, True)
    want = oracle_sets(csr, n, nodes, lab, s0.cpu().numpy(), train_pos, 1.0, 0.5, True)
    assert sets[0] == want


def test_halo_table_full_is_reported_promptly(P):
    """pcg_halo_collect with a hash table far too small for the window's distinct remote neighbours: every probe sequence is
    bounded, the kernel stops walking once the table is reported full, and overflow bit 1 is set - a capacity error, not a
    pseudo-hang of O(ids x slots) probes."""
    import ctypes as C
    import time
    from pcgnn_amd import _lib
    lib = _lib.load()
    ops = P.ops
    n = 40000
    X, labels, csrs = synth_graph(3, n, 32, (300.0,), 0.1, hub=False)
    g = P.DeviceGraph(X, csrs, [], dev())
    lo, hi = 0, 64                                      # this "rank" owns 64 nodes: nearly every neighbour is remote
    centres = torch.arange(64, dtype=torch.int32, device=dev())
    halo_cap = 128                                      # the window needs ~15 000 rows
    slots = int(lib.pcg_halo_table_slots(halo_cap))
    assert slots == 1024
    table = torch.empty(2 * slots, dtype=torch.int32, device=dev())
    counts = torch.zeros(131, dtype=torch.int32, device=dev())
    uniq = torch.empty(halo_cap, dtype=torch.int32, device=dev())
    bounds = torch.tensor([0, 64, n], dtype=torch.int32, device=dev())
    empty = torch.zeros(1, dtype=torch.int32, device=dev())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _lib.check(lib.pcg_halo_collect(g.desc_ref(), ops._p(centres), 64, lo, hi, 64, ops._p(empty), 0, ops._p(bounds), 2, ops._p(table),
                                    slots, ops._p(counts), ops._p(uniq), halo_cap, 64, halo_cap, 0, ops._stream(dev())),
               "pcg_halo_collect")
    torch.cuda.synchronize()
    assert time.perf_counter() - t0 < 5.0
    flags = int(counts[128].item())
    assert flags & 1, "the table-full bit"
    distinct = len(set(csrs[0][1][csrs[0][0][0]:csrs[0][0][64]].tolist()) - set(range(64)))
    assert distinct > 20 * halo_cap, "the test must over-subscribe the table by far"
    # the same window with room: no flag, and every distinct remote neighbour got a slot
    halo_cap = 32768
    slots = int(lib.pcg_halo_table_slots(halo_cap))
    table = torch.empty(2 * slots, dtype=torch.int32, device=dev())
    counts.zero_()
    uniq = torch.empty(halo_cap, dtype=torch.int32, device=dev())
    _lib.check(lib.pcg_halo_collect(g.desc_ref(), ops._p(centres), 64, lo, hi, 64, ops._p(empty), 0, ops._p(bounds), 2, ops._p(table),
                                    slots, ops._p(counts), ops._p(uniq), halo_cap, 64, halo_cap, 0, ops._stream(dev())),
               "pcg_halo_collect")
    torch.cuda.synchronize()
    assert int(counts[128].item()) == 0 and int(counts[1].item()) == distinct
    got = uniq.cpu().numpy()
    assert len(set(got[got >= 0].tolist())) == distinct


@pytest.mark.parametrize("feat", [10, 25, 32, 64, 100, 166, 400])
def test_feature_widths(P, feat):
    ops = P.ops
    n = 3000
    X, labels, csrs = synth_graph(21, n, feat, (4, 20), 0.1)
    train_pos = np.flatnonzero(labels == 1)[:200].tolist()
    g = P.DeviceGraph(X, csrs, train_pos, dev())
    W = torch.randn(2, feat, generator=torch.Generator().manual_seed(2)).cuda()
    b = torch.randn(2, generator=torch.Generator().manual_seed(3)).cuda()
    s0 = ops.score_table(g, W, b)
    ref = torch.nn.functional.linear(torch.from_numpy(X), W.cpu(), b.cpu())[:, 0]
    np.testing.assert_allclose(s0.cpu().numpy(), ref.numpy(), rtol=0, atol=1e-4)
    keys = ops.pos_sort(g, s0)
    rs = np.random.RandomState(5)
    nodes = rs.randint(0, n, size=97).tolist()
    lab = labels[np.array(nodes)].tolist()
    sets, agg, cnt = ops.chosen_sets(g, torch.tensor(nodes, dtype=torch.int32, device=dev()),
                                     torch.tensor(lab, dtype=torch.int32, device=dev()), s0, keys, [0.5, 0.5], 0.8, True)
    for r in range(2):
        want = oracle_sets(csrs[r], n, nodes, lab, s0.cpu().numpy(), train_pos, 0.5, 0.8, True)
        assert sets[r] == want
        np.testing.assert_allclose(agg[r].cpu().numpy(), O.sparse_aggregate(want, torch.from_numpy(X)).numpy(),
                                   rtol=0, atol=FEAT_TOL)
    got = ops.gather_rows(g, torch.tensor(nodes, dtype=torch.int32, device=dev()))
    assert np.array_equal(got.cpu().numpy(), X[np.array(nodes)])


def test_edge_cases(P):
    ops = P.ops
    n = 500
    X, labels, csrs = synth_graph(31, n, 32, (6,), 0.2)
    train_pos = np.flatnonzero(labels == 1).tolist()
    g = P.DeviceGraph(X, csrs, train_pos, dev())
    W = torch.randn(2, 32, generator=torch.Generator().manual_seed(4)).cuda()
    b = torch.zeros(2).cuda()
    s0 = ops.score_table(g, W, b)
    keys = ops.pos_sort(g, s0)
    # empty batch
    agg, cnt = ops.choose_aggregate(g, torch.zeros(0, dtype=torch.int32, device=dev()),
                                    torch.zeros(0, dtype=torch.int32, device=dev()), s0, keys, [0.5], 0.5, True)
    assert agg.shape == (1, 0, 32)
    # single node, duplicates, rho = 0 (no over-sampling), rho huge (all train-pos)
    for nodes, rho in (([3], 0.5), ([5, 5, 5, 9, 5], 0.5), ([1, 2, 3, 4], 0.0), ([1, 2, 3, 4], 1e6)):
        lab = [1] * len(nodes)
        sets, agg, cnt = ops.chosen_sets(g, torch.tensor(nodes, dtype=torch.int32, device=dev()),
                                         torch.tensor(lab, dtype=torch.int32, device=dev()), s0, keys, [0.5], rho, True)
        want = oracle_sets(csrs[0], n, nodes, lab, s0.cpu().numpy(), train_pos, 0.5, rho, True)
        assert sets[0] == want
        np.testing.assert_allclose(agg[0].cpu().numpy(), O.sparse_aggregate(want, torch.from_numpy(X)).numpy(),
                                   rtol=0, atol=FEAT_TOL)
    # thresholds other than 0.5 (BASELINE config 5 sweeps; layers.py:193 fixes 0.5)
    nodes = list(range(40))
    for thr in (0.2, 0.8, 1.0):
        sets, _, _ = ops.chosen_sets(g, torch.tensor(nodes, dtype=torch.int32, device=dev()), None, s0, None, [thr], 0.5, False)
        assert sets[0] == oracle_sets(csrs[0], n, nodes, None, s0.cpu().numpy(), train_pos, thr, 0.5, False)
    # no training positives at all
    g0 = P.DeviceGraph(X, csrs, [], dev())
    sets, _, _ = ops.chosen_sets(g0, torch.tensor(nodes, dtype=torch.int32, device=dev()),
                                 torch.ones(40, dtype=torch.int32, device=dev()), s0, None, [0.5], 0.5, True)
    assert sets[0] == oracle_sets(csrs[0], n, nodes, [1] * 40, s0.cpu().numpy(), [], 0.5, 0.5, True)


def test_segment_mean_and_graphsage_aggregators(P, case):
    c, ops = case, P.ops
    g = P.DeviceGraph(c.X, [c.homo_csr], [], dev())
    sub = c.z["s1_nodes"].tolist()
    indptr, idx = c.homo_csr
    begin = torch.from_numpy(indptr[np.array(sub)]).cuda()
    count = torch.from_numpy(np.diff(indptr)[np.array(sub)].astype(np.int32)).cuda()
    idx_d = torch.from_numpy(idx).cuda()
    got = ops.segment_mean(g, begin, count, idx_d, 0)
    np.testing.assert_allclose(got.cpu().numpy(), c.z["s1_mean"], rtol=0, atol=FEAT_TOL)
    # GCN: union self, / sqrt(count); SAGE gcn=True: union self, / count - through the fused kernel (threshold 1 => keep all)
    s0 = torch.zeros(c.n, device=dev())
    nodes = torch.tensor(sub, dtype=torch.int32, device=dev())
    agg, _ = ops.choose_aggregate(g, nodes, None, s0, None, [1.0], 0.0, False, norm=1, add_self=True)
    np.testing.assert_allclose(agg[0].cpu().numpy(), c.z["s1_gcn"], rtol=0, atol=FEAT_TOL)
    agg, _ = ops.choose_aggregate(g, nodes, None, s0, None, [1.0], 0.0, False, norm=0, add_self=True)
    np.testing.assert_allclose(agg[0].cpu().numpy(), c.z["s1_mean_gcn"], rtol=0, atol=FEAT_TOL)


def test_intra_agg_reference_signature(P, case):
    """IntraAgg.forward called the way the reference's InterAgg calls it (layers.py:268)."""
    c = case
    rho = c.rhos[0]
    m = build_model(P, c, rho)
    table = torch.from_numpy(c.z["table_scores"].copy())
    adj = c.adj(0)
    lists = [sorted(adj[v]) for v in c.nodes]
    nscores = [table[torch.as_tensor(l)] for l in lists]
    samples = [math.ceil(len(l) * 0.5) for l in lists]
    center = table[torch.as_tensor(c.nodes)]
    pos_scores = table[torch.as_tensor(c.train_pos)]
    feats, _ = m.inter1.intra_agg1.forward(c.nodes, c.batch_labels, lists, center, nscores, pos_scores, samples, False)
    np.testing.assert_allclose(feats.detach().cpu().numpy(), c.z["test_feats0"], rtol=0, atol=FEAT_TOL)


@pytest.mark.parametrize("n_pos", [1, 63, 64, 65, 4096, 8192, 8193, 16384, 16385, 40000, 65536, 65537])
def test_pos_sort_sizes(P, n_pos):
    """rank sort (<= 16384, tiles of 8192) and chunk-sort + merge-rank (> 16384) paths, incl. duplicate scores."""
    ops = P.ops
    n = 80000
    rs = np.random.RandomState(n_pos)
    X = np.zeros((n, 4), np.float32)
    indptr = np.arange(n + 1, dtype=np.int64)
    g = P.DeviceGraph(X, [(indptr, np.arange(n, dtype=np.int32))], rs.choice(n, size=n_pos, replace=False).tolist(), dev())
    s0h = np.round(rs.randn(n).astype(np.float32), 2)          # many equal scores, both signs, +-0
    s0h[rs.randint(0, n, 50)] = -0.0
    keys = ops.pos_sort(g, torch.from_numpy(s0h).cuda()).cpu().numpy().view(np.uint64)
    pos = (keys[:n_pos] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    sc = s0h[g.train_pos_host]
    # order: by score (with -0.0 < +0.0 as the orderable bit pattern has it), then by position
    bits = sc.view(np.uint32).astype(np.int64)
    ordk = np.where(bits & 0x80000000, (~bits) & 0xFFFFFFFF, bits | 0x80000000)
    assert np.array_equal(pos, np.lexsort((np.arange(n_pos), ordk)))
    cap = 4096
    while cap < n_pos:
        cap *= 2
    assert np.all(keys[n_pos:cap] == np.uint64(0xFFFFFFFFFFFFFFFF))


@pytest.mark.parametrize("n_pos", [16385, 40000, 65537, 131072])
def test_pos_sort_one_launch(P, n_pos):
    """The one-launch bucket sort over raw keys (16384 < n_pos <= 131072: what a training step's gather launch is followed by):
    the same order as pcg_pos_sort's four launches, all-ones padding, nothing reported - on scores with many duplicates (the keys
    stay unique through their positions), on a constant score (every key in a single run of equal scores: the splitters fall
    inside it) and on a sorted-descending one."""
    from pcgnn_amd import _lib
    ops, lib = P.ops, _lib.load()
    n = n_pos + 1000
    rs = np.random.RandomState(n_pos)
    X = np.zeros((n, 4), np.float32)
    indptr = np.arange(n + 1, dtype=np.int64)
    g = P.DeviceGraph(X, [(indptr, np.arange(n, dtype=np.int32))], rs.choice(n, size=n_pos, replace=False).tolist(), dev())
    assert lib.pcg_pos_sort_one_launch(n_pos) == 1 and lib.pcg_pos_sort_one_launch(16384) == 0
    cap = int(lib.pcg_pos_sort_capacity(n_pos)) // 2
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    for kind in ("duplicates", "constant", "descending"):
        if kind == "duplicates":
            s0h = np.round(rs.randn(n).astype(np.float32), 2)
            s0h[rs.randint(0, n, 50)] = -0.0
        elif kind == "constant":
            s0h = np.full(n, 0.25, np.float32)
        else:
            s0h = -np.arange(n, dtype=np.float32)
        s0 = torch.from_numpy(s0h).cuda()
        want = ops.pos_sort(g, s0).clone()                       # the four-launch sort; its scratch half holds other things
        keys = torch.zeros_like(want)
        # raw keys: whatever order the sorted ones are shuffled into (unique 64-bit keys: the sort's input is just that)
        perm = torch.from_numpy(rs.permutation(n_pos)).cuda()
        keys[cap:cap + n_pos] = want[:n_pos][perm]
        _lib.check(lib.pcg_pos_sort_raw(g.desc_ref(), ops._p(keys), ops._p(status), ops._stream(dev())), "pcg_pos_sort_raw")
        torch.cuda.synchronize()
        assert torch.equal(keys[:cap], want[:cap]), kind
        assert int(status.item()) == 0, kind


# ---------------------------------------------------------------------------
# fused dense step + Adam (hand-written MFMA kernels) and the hipGraph-captured step
# ---------------------------------------------------------------------------
def fused_of(P, c, rho, **kw):
    from pcgnn_amd.fused import FusedPCGNN
    m = build_model(P, c, rho, graph=graph_of(P, c))
    return m, FusedPCGNN(m, c.lr, c.wd, max_batch=len(c.nodes), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1024, 1500, 4096, 9000])
def test_label_classifier_step_of_its_own(P, case, B):
    """The label classifier is stepped by the select launch (one workgroup per <= 1024 rows of the batch, the gradients of
    several summed by the last one in): after two steps - batches with repeated centres - its parameters and Adam state
    track torch autograd + torch.optim.Adam; the other parameters too (their update is the deferred one)."""
    c = case
    rho = c.rhos[0]
    rs = np.random.RandomState(B)
    nodes = rs.randint(0, len(c.labels), size=B)
    ids = torch.from_numpy(nodes.astype(np.int32)).cuda()
    lab = torch.from_numpy(c.labels[nodes].astype(np.int32)).cuda()
    m1, f1 = fused_of(P, c, rho)
    m3 = build_model(P, c, rho, graph=graph_of(P, c))
    opt = torch.optim.Adam([p for p in m3.parameters() if p.requires_grad], lr=c.lr, weight_decay=c.wd)
    for step in range(2):
        sl = slice(0, None) if step == 0 else slice(B // 3, None)
        f1.train_step(ids[sl], lab[sl], defer=True)
        opt.zero_grad()
        m3.loss(ids[sl], lab[sl].long()).backward()
        opt.step()
    f1.flush()
    torch.cuda.synchronize()
    f1.check()
    sd1, sd3 = m1.state_dict(), m3.state_dict()
    for k in PARAM_KEYS(c.R):
        a, b = sd1[k].cpu().numpy(), sd3[k].cpu().numpy()
        # (Adam's first steps move every parameter by ~lr whatever the gradient's size: a wrong gradient sum - a slice of the
        #  batch missing, say - shows as differences of the order of lr everywhere; rounding differences of the sums do not)
        np.testing.assert_allclose(a, b, rtol=0, atol=c.lr * 0.25, err_msg=k)
        assert np.mean(np.abs(a - b)) < c.lr * 5e-3, k


def test_fused_forward_grads_adam_golden(P, case):
    c = case
    rho = c.rhos[0]
    tag = f"rho{rho}"
    m, fz = fused_of(P, c, rho)
    ids = torch.tensor(c.nodes, dtype=torch.int32, device=dev())
    lab = torch.from_numpy(c.batch_labels.astype(np.int32)).cuda()
    # inference and training forward
    lg, cs, comb = fz.predict(ids, None, False, want_combined=True)
    np.testing.assert_allclose(torch.sigmoid(lg).cpu().numpy(), c.z["test_gnn_prob"], rtol=0, atol=LOGIT_TOL)
    np.testing.assert_allclose(comb.cpu().numpy().T, c.z["test_combined"], rtol=0, atol=FEAT_TOL)
    lg, cs = fz.predict(ids, lab, True)
    np.testing.assert_allclose(lg.cpu().numpy(), c.z[f"{tag}_train_logits"], rtol=0, atol=LOGIT_TOL)
    np.testing.assert_allclose(cs.cpu().numpy(), c.z[f"{tag}_train_center_scores"], rtol=0, atol=1e-5)
    # gradients of every parameter
    # (both ways the engine forms them: the training step's - transposed activations, weight gradients as GEMMs over the batch -
    #  and the data-parallel paths' per-tile slabs summed in tile order)
    by_via = {}
    for via in ("slabs", "acts"):
        grads = by_via[via] = fz.gradients(ids, lab, via=via)
        assert abs(float(fz.last_loss()) - float(c.z[tag + "_loss"])) < LOGIT_TOL
        for k in PARAM_KEYS(c.R):
            np.testing.assert_allclose(grads[k].cpu().numpy(), c.z[f"{tag}_grad_{k}"], rtol=0, atol=2e-5, err_msg=f"{k} via {via}")
    # ... and against float64 (tests/dense_ref.py: the golden sets; the engine's own ReLU masks where f32 and f64 may differ)
    r64, r32, _, wrong = D.reference_pair(c, c.nodes, c.batch_labels, [c.sel(f"{tag}_train", r) for r in range(c.R)],
                                          dev_masks=D.device_masks(fz.acts, c.f, c.emb, c.R, len(c.nodes)))
    assert wrong == 0
    for via, k in [(via, k) for via in by_via for k in PARAM_KEYS(c.R)]:
        assert D.rel_err(by_via[via][k], r64["grads"][k]) <= D.tolerance(D.rel_err(r32["grads"][k], r64["grads"][k])), f"{k} via {via}"
    # one Adam step: where the reference's own gradient is well away from zero the first update is -lr * g'/(|g'| + eps)
    # with g' = g + wd * p (coupled decay) - elementwise tight there; loose where |g'| ~ the gradient tolerance
    p0 = {k: v.clone() for k, v in c.params().items()}
    fz.train_step(ids, lab)
    sd = m.state_dict()
    for k in PARAM_KEYS(c.R):
        got, want = sd[k].cpu().numpy(), c.z[f"{tag}_step_{k}"]
        gp = c.z[f"{tag}_grad_{k}"] + c.wd * p0[k].numpy()
        firm = np.abs(gp) > 2e-3
        np.testing.assert_allclose(got[firm], want[firm], rtol=0, atol=c.lr * 2e-2, err_msg=k)
        # elsewhere: the first update is -lr * g' / (|g'| + eps); a gradient off by dg (<= the 2e-5 tolerance above) moves it by at
        # most lr * dg / (|g'| + eps), and never by more than 2 * lr (a sign flip at |g'| ~ dg)
        bound = np.minimum(c.lr * 4e-5 / (np.abs(gp) + 1e-8), 2.001 * c.lr) + c.lr * 1e-3
        assert (np.abs(got - want) <= bound).all(), k
        # ... and against torch.optim.Adam applied to the KERNEL's own gradient: tight for every element
        t = torch.nn.Parameter(p0[k].clone())
        t.grad = grads[k].cpu().clone()
        torch.optim.Adam([t], lr=c.lr, weight_decay=c.wd).step()
        np.testing.assert_allclose(got, t.detach().numpy(), rtol=0, atol=c.lr * 2e-4, err_msg=k + " (torch Adam on the kernel's gradient)")
    assert int(fz.step_counter.item()) == 1


def test_fused_graph_equals_eager_and_torch(P, case):
    """Five steps: hipGraph replay == eager fused launches bit for bit; both track the
    torch-autograd + torch.optim.Adam path."""
    c = case
    rho = c.rhos[0]
    ids = torch.tensor(c.nodes, dtype=torch.int32, device=dev())
    lab = torch.from_numpy(c.batch_labels.astype(np.int32)).cuda()
    m1, f1 = fused_of(P, c, rho)
    m2, f2 = fused_of(P, c, rho)
    m3 = build_model(P, c, rho, graph=graph_of(P, c))
    opt = torch.optim.Adam([p for p in m3.parameters() if p.requires_grad], lr=c.lr, weight_decay=c.wd)
    half = len(c.nodes) // 2
    for step in range(5):
        sl = slice(0, None) if step % 2 == 0 else slice(0, half)     # two batch sizes -> two graphs
        f1.train_step(ids[sl], lab[sl])
        f2.train_step_graph(ids[sl], lab[sl])
        opt.zero_grad()
        m3.loss(ids[sl], lab[sl].long()).backward()
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(f1.theta, f2.theta), "graph replay must reproduce the eager fused step exactly"
    sd1, sd3 = m1.state_dict(), m3.state_dict()
    for k in PARAM_KEYS(c.R):
        a, b = sd1[k].cpu().numpy(), sd3[k].cpu().numpy()
        np.testing.assert_allclose(a, b, rtol=0, atol=c.lr * 0.25, err_msg=k)
        assert np.mean(np.abs(a - b)) < c.lr * 5e-3, k      # on average the two trajectories stay together
    assert abs(float(f1.last_loss()) - float(f2.last_loss())) == 0.0


def test_adam_step_matches_torch_adam(P):
    """pcg_adam_step alone against torch.optim.Adam (coupled weight decay, bias correction) on the same gradient
    sequence: six steps, the gradient of every step handed over as 1..37 partial slabs (model_handler.py:124,153)."""
    from pcgnn_amd import _lib
    lib, ops = _lib.load(), P.ops
    n = 26818
    gen = torch.Generator().manual_seed(12)
    p0 = torch.randn(n, generator=gen) * 0.1
    for lr, wd, b1, b2, eps in ((0.01, 0.001, 0.9, 0.999, 1e-8), (0.005, 0.0, 0.8, 0.99, 1e-6), (0.02, 0.05, 0.9, 0.999, 1e-8)):
        ref = torch.nn.Parameter(p0.clone().cuda())
        opt = torch.optim.Adam([ref], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
        theta = p0.clone().cuda()
        m, v = torch.zeros_like(theta), torch.zeros_like(theta)
        counter = torch.zeros(1, dtype=torch.int32, device=dev())
        grad_out = torch.empty_like(theta)
        for step, n_slabs in enumerate((1, 2, 5, 16, 37, 64)):
            slabs = (torch.randn(n_slabs, n, generator=gen) * (10.0 ** -(step % 3))).cuda()
            if step == 3:
                slabs[:, ::7] = 0.0                     # exact zeros: the update is then pure weight decay / momentum
            counter += 1
            _lib.check(lib.pcg_adam_step(ops._p(theta), ops._p(m), ops._p(v), ops._p(slabs), n_slabs, n, ops._p(counter),
                                         _lib.AdamHyper(lr, b1, b2, eps, wd), ops._p(grad_out), 1, ops._stream(dev())), "pcg_adam_step")
            g = slabs.double().sum(0).float()
            np.testing.assert_allclose(grad_out.cpu().numpy(), g.cpu().numpy(), rtol=2e-6, atol=1e-6 * n_slabs)
            ref.grad = grad_out.clone()                 # the same summed gradient, so only the update rule is compared
            opt.step()
            np.testing.assert_allclose(theta.cpu().numpy(), ref.detach().cpu().numpy(), rtol=0, atol=lr * 2e-5,
                                       err_msg=f"step {step} lr {lr} wd {wd}")
        st = opt.state[ref]
        np.testing.assert_allclose(m.cpu().numpy(), st["exp_avg"].cpu().numpy(), rtol=1e-5, atol=2e-7)    # (sums that cancel)
        np.testing.assert_allclose(v.cpu().numpy(), st["exp_avg_sq"].cpu().numpy(), rtol=5e-5, atol=1e-12)


# ---------------------------------------------------------------------------
# GraphSAGE / GCN baselines and the evaluation loop on the same kernels
# ---------------------------------------------------------------------------
def test_graphsage_gcn_models_golden(P, case):
    from pcgnn_amd import graphsage as GS
    c = case
    feats = torch.nn.Embedding(c.n, c.f)
    feats.weight = torch.nn.Parameter(torch.from_numpy(c.X.copy()), requires_grad=False)
    homo = c.adj(None)
    sub = c.z["s1_nodes"].tolist()
    # Encoder(gcn=True) over a MeanAggregator with its own gcn=False - exactly what the fixture generator built
    enc = GS.Encoder(feats, c.f, c.emb, homo, GS.MeanAggregator(feats, cuda=True), gcn=True, cuda=True).to("cuda")
    with torch.no_grad():
        enc.weight.copy_(torch.from_numpy(c.z["s1_sage_enc_w"]))
    np.testing.assert_allclose(enc(sub).detach().cpu().numpy(), c.z["s1_sage_enc"], rtol=0, atol=FEAT_TOL)
    genc = GS.GCNEncoder(feats, c.f, c.emb, homo, GS.GCNAggregator(feats, cuda=True), cuda=True).to("cuda")
    with torch.no_grad():
        genc.weight.copy_(torch.from_numpy(c.z["s1_gcn_enc_w"]))
    np.testing.assert_allclose(genc(sub).detach().cpu().numpy(), c.z["s1_gcn_enc"], rtol=0, atol=5e-5)
    # aggregators with explicit neighbour sets (reference call shape) incl. the gcn self-union
    neighs = [homo[int(v)] for v in sub]
    magg = GS.MeanAggregator(feats, cuda=True, gcn=True)
    magg._dev = dev()
    magg.adj_lists = None
    got = magg.forward(sub, neighs)
    np.testing.assert_allclose(got.cpu().numpy(), c.z["s1_mean_gcn"], rtol=0, atol=FEAT_TOL)
    # full models train: loss decreases over a few Adam steps
    labels = c.labels[np.array(sub)]
    torch.manual_seed(0)                      # the classifier heads are randomly initialised
    for model in (GS.GCN(2, genc).to("cuda"), GS.GraphSage(2, enc).to("cuda")):
        opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=0.05)
        losses = []
        for _ in range(30):
            opt.zero_grad()
            loss = model.loss(sub, torch.from_numpy(labels).cuda())
            loss.backward()
            opt.step()
            losses.append(loss.item())
        assert np.isfinite(losses).all() and min(losses[1:]) < losses[0]
        prob, _ = model.to_prob(sub, labels, train_flag=False)
        assert tuple(prob.shape) == (len(sub), 2)


def test_graphsage_random_fanout_golden(P, case):
    """MeanAggregator.forward(..., num_sample=k) (graphsage.py:70-74) against the reference's output under the same seed."""
    import random
    from pcgnn_amd import graphsage as GS
    c = case
    feats = torch.nn.Embedding(c.n, c.f)
    feats.weight = torch.nn.Parameter(torch.from_numpy(c.X.copy()), requires_grad=False)
    homo = c.adj(None)
    sub = c.z["s1_nodes"].tolist()
    k, seed = int(c.z["s1_fanout_k"]), int(c.z["s1_fanout_seed"])
    for gcn, key in ((False, "s1_fanout_mean"), (True, "s1_fanout_mean_gcn")):
        agg = GS.MeanAggregator(feats, cuda=True, gcn=gcn)
        agg._dev = dev()
        random.seed(seed)
        fsets = [set(sorted(homo[int(v)])) for v in sub]
        got = agg.forward(sub, fsets, num_sample=k)
        np.testing.assert_allclose(got.cpu().numpy(), c.z[key], rtol=0, atol=FEAT_TOL)


def test_eval_loop_matches_reference_probabilities(P, case):
    """utils.test mirror (utils.py:280-333): batched inference -> metrics, torch path and fused path."""
    from pcgnn_amd import utils as U
    from pcgnn_amd.fused import FusedPCGNN
    c = case
    prob = c.z["test_gnn_prob"]
    want = U.binary_metrics(c.batch_labels, prob.argmax(1), prob[:, 1])
    m = build_model(P, c, c.rhos[0], graph=graph_of(P, c))
    auc, recall, f1m, prec = U.test(np.array(c.nodes), c.batch_labels, m, batch_size=50, print_line=False)
    assert abs(auc - want["auc"]) < 1e-6 and abs(f1m - want["f1_macro"]) < 1e-6
    assert abs(recall - want["recall"]) < 1e-6 and abs(prec - want["precision"]) < 1e-6
    fz = FusedPCGNN(m, c.lr, c.wd, max_batch=64)
    auc2, recall2, f1m2, prec2 = U.test(np.array(c.nodes), c.batch_labels, fz, batch_size=64, print_line=False)
    assert abs(auc2 - want["auc"]) < 1e-6 and abs(f1m2 - want["f1_macro"]) < 1e-6
    # the "(f1)" evaluation (utils(f1).py:280-350): validation picks the threshold, the test split applies it
    _, thr_want = U.get_best_f1(c.batch_labels, prob[:, 1])
    auc3, _, f1m3, _, thr = U.test_f1(np.array(c.nodes), c.batch_labels, fz, batch_size=64, flag="valid")
    preds = (prob[:, 1] > thr_want).astype(np.int64)
    f1m_want = 0.5 * (U._prf(c.batch_labels, preds, 1)[2] + U._prf(c.batch_labels, preds, 0)[2])
    assert abs(thr - thr_want) < 1e-12 and abs(auc3 - want["auc"]) < 1e-6 and abs(f1m3 - f1m_want) < 1e-6
    assert U.test_f1(np.array(c.nodes), c.batch_labels, m, batch_size=50, flag="test", valid_thresh=thr)[4] is None


# ---------------------------------------------------------------------------
# BASELINE-size workload (configs[1]: YelpChi-shaped graph, batch 1024): size-independent properties
# ---------------------------------------------------------------------------
def _full_size_workload(name):
    from pcgnn_amd import synth
    if name == "yelp":
        return synth.yelp_like(0), 1024
    if name == "yelp_e128":      # BASELINE configs[2]'s shape on one GPU: emb 128, batch 4096 (the dense kernel that streams its weights, 256 tiles)
        return synth.yelp_like(0), 4096
    if name == "amazon":
        return synth.amazon_like(0), 256
    # power-law: 200 K nodes / 4 M edges, the most popular node capped at 0.5 % of a relation's endpoints, so that rows of
    # every degree tier (<= 128, <= 512, <= 4096, > 4096, > 12288 -> global scratch) occur
    return synth.power_law(200_000, 4_000_000, 0, max_share=5e-3), 4096


@pytest.mark.parametrize("wname,rho", [("yelp", 0.5), ("yelp_e128", 0.5), ("amazon", 0.2), ("amazon", 0.5), ("amazon", 0.8), ("powerlaw", 0.5)])
def test_full_size_properties(P, wname, rho):
    """BASELINE-size workloads (configs[1]: YelpChi-shaped batch 1024; configs[4]: Amazon-shaped batch 256, rho sweep;
    configs[3] shape: power-law, batch 4096): properties that hold at any size - idempotence, the selection lists are
    sets, kept neighbours an ascending subset of the row, the count law, every mean recomputed in float64 from the
    materialised lists - plus the oracle's chosen sets on a strided sample of rows, plus a few training epochs."""
    from pcgnn_amd.handler import PCGNNTrainer
    ops = P.ops
    w, B = _full_size_workload(wname)
    emb = 128 if wname == "yelp_e128" else 64
    tr = PCGNNTrainer(w, dict(engine="fused", batch_size=B, rho=rho, emb_size=emb), dev())
    g, fz = tr.graph, tr.fused
    ids = tr.sampler.pick(B, 0)          # B label-balanced, degree-biased draws with replacement (utils.py:274-278)
    assert ids.numel() == B
    if wname == "powerlaw":       # make sure the longest rows of every relation are in the batch
        top = np.unique(np.concatenate([np.argsort(np.diff(ip))[-3:] for ip, _ in w.csr])).astype(np.int32)
        ids[:len(top)] = torch.from_numpy(top).to(ids.device)
    lab = tr.labels_i32[ids.long()]
    s0 = ops.score_table(g, fz.w_clf, fz.b_clf)
    keys = ops.pos_sort(g, s0)
    R = g.R
    ids_h, lab_h = ids.cpu().numpy(), lab.cpu().numpy()
    s0_h = s0.cpu().numpy()
    tp = set(w.train_pos)
    if wname == "powerlaw":
        degs = np.concatenate([np.diff(ip)[ids_h] for ip, _ in w.csr])
        assert (degs <= 128).any() and ((degs > 128) & (degs <= 512)).any() and ((degs > 512) & (degs <= 4096)).any() \
            and (degs > 4096).any() and (degs > 12288).any(), "every degree tier must be exercised"
    for train in (False, True):
        ws = ops.ChooseWorkspace(g, B)
        agg, cnt = ops.choose_aggregate(g, ids, lab if train else None, s0, keys if train else None, [0.5] * R, rho, train, ws=ws)
        agg2, cnt2 = ops.choose_aggregate(g, ids, lab if train else None, s0, keys if train else None, [0.5] * R, rho, train, ws=ws)
        torch.cuda.synchronize()
        ws.check()
        assert torch.equal(agg, agg2) and torch.equal(cnt, cnt2), "idempotent and run-to-run bitwise reproducible"
        begin = ws.view(0, torch.int64, R * B + 1).cpu().numpy()
        length = ws.view(1, torch.int32, R * B).cpu().numpy()
        lst = ws.view(2, torch.int32, int(begin[-1])).cpu().numpy()
        cnt_h = cnt.cpu().numpy()
        agg_h = agg.cpu().numpy()
        stride = 7 if B <= 1024 else 29
        for r in range(R):
            indptr, idx = w.csr[r]
            deg = np.diff(indptr)[ids_h]
            k = np.ceil(deg * 0.5).astype(np.int64)
            kept = np.where(deg > k + 1, k, deg)
            probe = sorted(set(range(0, B, stride)) | set(range(8)))       # strided rows + the forced hub rows
            for b in probe:
                row = r * B + b
                seg = lst[begin[row]:begin[row] + length[row]]
                chosen = seg[seg >= 0]
                assert len(chosen) == cnt_h[r, b] and len(set(chosen.tolist())) == len(chosen), "a set: no duplicates"
                nb = idx[indptr[ids_h[b]]:indptr[ids_h[b] + 1]]
                first = chosen[:kept[b]]
                assert np.all(np.diff(first) > 0) and np.isin(first, nb).all(), "kept neighbours: ascending subset of the row"
                extra = chosen[kept[b]:]
                if not train or lab_h[b] != 1:
                    assert len(extra) == 0 and cnt_h[r, b] == kept[b]
                else:
                    m = min(int(k[b] * rho), len(w.train_pos))
                    assert len(extra) <= m and all(int(e) in tp for e in extra) and not np.isin(extra, first).any()
                ref = w.X[chosen].astype(np.float64).mean(0)
                np.testing.assert_allclose(agg_h[r, b], ref, rtol=0, atol=2e-5)
            # the oracle's sets (same device scores => bit-exact) on the probed rows
            want = oracle_sets(w.csr[r], w.n, [int(ids_h[b]) for b in probe], [int(lab_h[b]) for b in probe] if train else None,
                               s0_h, w.train_pos, 0.5, rho, train)
            for b, ws_ in zip(probe, want):
                row = r * B + b
                seg = lst[begin[row]:begin[row] + length[row]]
                assert set(seg[seg >= 0].tolist()) == ws_, f"{wname} rel {r} row {b} (deg {deg[b]}) train={train}"
        # test mode count law over ALL rows at once
        if not train:
            for r in range(R):
                deg = np.diff(w.csr[r][0])[ids_h]
                k = np.ceil(deg * 0.5).astype(np.int64)
                assert np.array_equal(cnt_h[r], np.where(deg > k + 1, k, deg))
    # a few training epochs through the hipGraph engine: finite loss that goes down
    tr2 = PCGNNTrainer(w, dict(engine="graph", batch_size=B, rho=rho, emb_size=emb), dev())
    theta0 = tr2.fused.theta.clone()
    losses = []
    for e in range(4):
        tr2.train_epoch(e)
        losses.append(float(tr2.fused.last_loss()))
    assert all(np.isfinite(losses)) and not torch.equal(theta0, tr2.fused.theta)
    if wname == "yelp_e128":     # a training step's gradients against torch autograd on the same aggregates (the E = 128 dense kernel at 256 tiles)
        fz2 = tr2.fused
        ids2 = tr2.sampler.pick(B, 7)
        lab2 = tr2.labels_i32[ids2.long()]
        grads = fz2.gradients(ids2, lab2)
        agg = fz2.agg.view(-1)[:g.R * B * g.feat_dim].view(g.R, B, g.feat_dim).clone()
        cnt = fz2.cnt.view(-1)[:g.R * B].view(g.R, B)
        # rows of several gather chunks: their means are finished inside the dense kernel - recompute them from the lists' counts
        # is not possible here without the lists, so compare on the torch side with the engine's own forward (predict, train mode)
        lg, cs, comb = fz2.predict(ids2, lab2, True, want_combined=True)
        Wc = fz2.views["weight"].detach().clone().requires_grad_(True)
        logits_t = comb.detach() @ Wc.t()
        loss_t = torch.nn.functional.cross_entropy(logits_t, lab2.long())
        loss_t.backward()
        np.testing.assert_allclose(lg.cpu().numpy(), logits_t.detach().cpu().numpy(), rtol=0, atol=1e-4)
        # d loss / d W_cls from the combined embeddings: the engine's gradient of the classifier weight (alpha-term excluded: it
        # does not reach W_cls)
        np.testing.assert_allclose(grads["weight"].cpu().numpy(), Wc.grad.cpu().numpy(), rtol=0, atol=2e-5)
    if wname in ("yelp", "yelp_e128"):          # (the Amazon-like features are row-normalised to ~1/F: four epochs of three batches barely move the loss)
        assert losses[-1] < losses[0]


def test_epoch_as_one_graph_equals_step_by_step(P):
    """A whole epoch as ONE graph launch (sampler + every batch, PCGNNTrainer.run_epoch_one_graph) leaves bit for bit the
    parameters, Adam moments and epoch counter that the same epochs run launch by launch leave (staged sampler, then
    FusedPCGNN.train_step per batch) - over three epochs, the last batch of each partial."""
    from pcgnn_amd import synth
    from pcgnn_amd.handler import PCGNNTrainer
    w = synth.make_workload("mini", 6000, 32, (4000, 30000, 90000), 0.12, seed=3)
    cfg = dict(engine="graph", batch_size=256, seed=5)
    a, b, c, d, e, f, h, i = (PCGNNTrainer(w, cfg, dev()) for _ in range(8))
    for t in (b, c, d, e, f, h, i):
        t.fused.theta.copy_(a.fused.theta)
        t.fused.params_changed()
    nb = a.batches_per_epoch()
    assert a.pick_size % a.batch_size != 0 and nb >= 3
    for ep in range(3):
        a.run_epoch_one_graph()
        d.run_epoch_one_graph(flush=False)      # the last batch's update left to the next epoch's first launch (bench.py)
        # ... and with the NEXT epoch's sampler and plans on a parallel branch of this epoch's graph (two buffer sets); the second
        # epoch is taken batch by batch from the set the first one prepared
        if ep == 1:
            assert e.fused._cur_ready
            e.start_epoch_staged()
            assert not e.fused._cur_ready
            for k in range(nb):
                e.fused.epoch_step(k, defer=True)
        else:
            e.run_epoch_one_graph(flush=False, prefetch=True)
        # ... or enqueued by the host on a second stream beside this epoch's graph
        f.run_epoch_one_graph(flush=False, prefetch="stream")
        # an event-bracketed epoch as bench.py runs it: the first batch kernel by kernel, the REST of the epoch one graph launch
        h.start_epoch_staged()
        h.fused.epoch_step_timed(0)
        h.fused.epoch_run(first_step=1, flush=False)
        # a run's last, partial epoch as one graph launch (sampler + plans + its first two batches), the rest batch by batch
        i.run_epoch_one_graph(flush=False, n_steps=2)
        for k in range(2, nb):
            i.fused.epoch_step(k, defer=True)
        ids = b.start_epoch_staged()
        for k in range(nb):
            sl = slice(k * b.batch_size, min((k + 1) * b.batch_size, b.pick_size))
            b.fused.train_step(ids[sl], b.fused._ep_lab[sl])
        # the same epoch as one graph replay per batch with the Adam update deferred inside the epoch (what bench.py does for
        # batches that are not part of a whole-epoch replay), the first batch of the second epoch launched kernel by kernel
        c.start_epoch_staged()
        for k in range(nb):
            if ep == 1 and k == 0:
                c.fused.epoch_step_timed(k)
            else:
                c.fused.epoch_step(k, defer=True)
    for t in (d, e, f, h, i):
        t.fused.flush()
    torch.cuda.synchronize()
    assert int(a._epoch_dev[0]) == int(b._epoch_dev[0]) == int(c._epoch_dev[0]) == int(d._epoch_dev[0]) == 3
    assert int(e._epoch_dev[0]) == 4 and e.fused._cur_ready        # (the fourth epoch is sampled and planned already)
    assert int(f._epoch_dev[0]) == 4 and f.fused._cur_ready
    assert torch.equal(a.fused._ep_ids[:a.pick_size], b.fused._ep_ids[:b.pick_size])
    assert torch.equal(a.fused._ep_ids[:a.pick_size], c.fused._ep_ids[:c.pick_size])
    for name in ("theta", "m", "v", "step_counter"):
        assert torch.equal(getattr(a.fused, name), getattr(b.fused, name)), name
        assert torch.equal(getattr(a.fused, name), getattr(c.fused, name)), name + " (per-batch graphs, deferred Adam)"
        assert torch.equal(getattr(a.fused, name), getattr(d.fused, name)), name + " (epoch graphs without the end-of-epoch flush)"
        assert torch.equal(getattr(a.fused, name), getattr(e.fused, name)), name + " (next epoch's sampler + plans on a parallel branch)"
        assert torch.equal(getattr(a.fused, name), getattr(f.fused, name)), name + " (next epoch's sampler + plans on a second stream)"
        assert torch.equal(getattr(a.fused, name), getattr(h.fused, name)), name + " (first batch eager, the rest of the epoch one graph)"
        assert torch.equal(getattr(a.fused, name), getattr(i.fused, name)), name + " (a partial epoch as one graph, the rest batch by batch)"
    assert torch.isfinite(a.fused.theta).all() and not torch.equal(a.fused.theta, torch.zeros_like(a.fused.theta))


def test_keys_sorted_a_launch_early_equal_the_in_kernel_sort(P, monkeypatch):
    """At batch sizes whose dense launch leaves CUs idle the dense launch sorts the NEXT step's train-pos keys and the select
    launch is told so (it sorts nothing, no row waits, a positive hub row's window search runs on one wave beside the others'
    key pass).  Same lists, same aggregates, same everything as the in-kernel sort (PCG_PRESORT=0), bit for bit: three epochs
    as graph launches + single steps with another batch size, on a graph with hub rows of a few thousand neighbours (workgroup
    rows of positive centres: the overlapped window search) and on the YelpChi-shaped one."""
    from pcgnn_amd import synth
    from pcgnn_amd.handler import PCGNNTrainer
    for w, B in ((synth.make_workload("hubs", 30000, 32, (20000, 150000, 900000), 0.15, seed=4, skew=1.2, max_share=5e-3), 512),
                 (synth.yelp_like(0), 1024)):
        engines = []
        for presort in ("1", "0"):
            monkeypatch.setenv("PCG_PRESORT", presort)
            t = PCGNNTrainer(w, dict(engine="graph", batch_size=B, seed=5), dev())
            assert t.fused.presort == (presort == "1")
            engines.append(t)
        a, b = engines
        b.fused.theta.copy_(a.fused.theta)
        b.fused.params_changed()
        if B == 512:
            deg = np.concatenate([np.diff(ip)[w.train_pos] for ip, _ in w.csr])
            assert (deg > 512).any(), "positive centres with workgroup rows must exist"
        for t in (a, b):
            for _ in range(3):
                t.run_epoch_one_graph()
            ids = t.sampler.pick(B // 2 + 7, 99)
            t.fused.train_step(ids, t.labels_i32[ids.long()])
            t.fused.train_step(ids[:100], t.labels_i32[ids[:100].long()], defer=True)
            t.fused.flush()
        torch.cuda.synchronize()
        for t in (a, b):
            t.fused.check()
        for name in ("theta", "m", "v", "step_counter", "clf_next"):
            assert torch.equal(getattr(a.fused, name), getattr(b.fused, name)), f"{name} ({w.name})"
        assert torch.equal(a.fused.agg, b.fused.agg) and torch.equal(a.fused.cnt, b.fused.cnt)


def test_epoch_groups_equal_epochs_one_by_one(P):
    """Several epochs sampled, planned and replayed TOGETHER (one sampler launch, one plan launch, one graph launch for the
    group: PCGNNTrainer.run_epoch_one_graph(n_epochs=K), what bench.py times) leave bit for bit what the same epochs leave one
    by one: the same picks in the same order, parameters, Adam moments, step and epoch counters - as one group of four, as two
    groups of two, as bench.py's event-bracketed group (first batch kernel by kernel, the rest one graph) and as a group cut
    short inside its third epoch.  Every epoch's last batch is the shorter one."""
    from pcgnn_amd import synth
    from pcgnn_amd.handler import PCGNNTrainer
    w = synth.make_workload("mini", 6000, 32, (4000, 30000, 90000), 0.12, seed=3)
    cfg = dict(engine="graph", batch_size=256, seed=5)
    a, b, c, d, e, f = (PCGNNTrainer(w, cfg, dev()) for _ in range(6))
    for t in (b, c, d, e, f):
        t.fused.theta.copy_(a.fused.theta)
        t.fused.params_changed()
    nb, n = a.batches_per_epoch(), a.pick_size
    assert n % a.batch_size != 0 and nb >= 3
    ids_a = []
    for _ in range(4):
        assert a.run_epoch_one_graph() == n
        ids_a.append(a.fused._ep_ids[:n].clone())
    assert b.run_epoch_one_graph(n_epochs=4) == 4 * n
    assert torch.equal(b.fused._ep_ids[:4 * n], torch.cat(ids_a)), "a group's picks are its epochs' picks, epoch by epoch"
    assert len(b.fused._ep_batches) == 4 * nb and b.fused._ep_batches[nb - 1][1] == n - (nb - 1) * a.batch_size
    c.start_epoch_staged(4)
    c.fused.epoch_step_timed(0)
    c.fused.epoch_run(first_step=1)
    d.run_epoch_one_graph(flush=False, n_epochs=2)
    d.run_epoch_one_graph(n_epochs=2)
    torch.cuda.synchronize()
    for t in (a, b, c, d):
        t.fused.check()
        assert int(t._epoch_dev[0]) == 4
    for name in ("theta", "m", "v", "step_counter"):
        assert torch.equal(getattr(a.fused, name), getattr(b.fused, name)), name + " (one group of four epochs)"
        assert torch.equal(getattr(a.fused, name), getattr(c.fused, name)), name + " (bracketed group)"
        assert torch.equal(getattr(a.fused, name), getattr(d.fused, name)), name + " (two groups of two)"
    # a group cut short inside its third epoch == two epochs and the first two batches of a third
    r = 2 * nb + 2
    assert e.run_epoch_one_graph(n_steps=r, n_epochs=4) == 2 * n + 2 * a.batch_size
    f.run_epoch_one_graph(flush=False)
    f.run_epoch_one_graph(flush=False)
    f.run_epoch_one_graph(n_steps=2)
    torch.cuda.synchronize()
    assert int(e._epoch_dev[0]) == 4 and int(f._epoch_dev[0]) == 3      # (the group's four epochs were sampled; three were begun)
    for name in ("theta", "m", "v", "step_counter"):
        assert torch.equal(getattr(e.fused, name), getattr(f.fused, name)), name + " (a group cut short)"
    assert int(e.fused.step_counter.item()) == r


def test_large_batch_two_pass_plan(P):
    """rows > 4096 take the two-launch, multi-workgroup plan: same result as the oracle / the small-batch path."""
    ops = P.ops
    n = 20000
    X, labels, csrs = synth_graph(41, n, 32, (3, 12), 0.12)
    train_pos = np.flatnonzero(labels == 1)[:900].tolist()
    g = P.DeviceGraph(X, csrs, train_pos, dev())
    W = torch.randn(2, 32, generator=torch.Generator().manual_seed(6)).cuda()
    s0 = ops.score_table(g, W, torch.zeros(2).cuda())
    keys = ops.pos_sort(g, s0)
    rs = np.random.RandomState(7)
    B = 5000                                         # 2 relations x 5000 = 10000 rows -> 3 plan blocks
    nodes = rs.randint(0, n, size=B)
    lab = labels[nodes]
    ids_d, lab_d = torch.from_numpy(nodes.astype(np.int32)).cuda(), torch.from_numpy(lab.astype(np.int32)).cuda()
    agg, cnt = ops.choose_aggregate(g, ids_d, lab_d, s0, keys, [0.5, 0.5], 0.5, True)
    # the same centres in small batches (single-block plan) must give bitwise the same rows
    for lo in (0, 1234, 4000):
        sl = slice(lo, lo + 700)
        agg_s, cnt_s = ops.choose_aggregate(g, ids_d[sl].contiguous(), lab_d[sl].contiguous(), s0, keys, [0.5, 0.5], 0.5, True)
        assert torch.equal(agg[:, sl], agg_s) and torch.equal(cnt[:, sl], cnt_s)
    sets, _, _ = ops.chosen_sets(g, ids_d, lab_d, s0, keys, [0.5, 0.5], 0.5, True)
    probe = list(range(0, B, 97))
    want = oracle_sets(csrs[1], n, nodes[probe].tolist(), lab[probe].tolist(), s0.cpu().numpy(), train_pos, 0.5, 0.5, True)
    assert [sets[1][b] for b in probe] == want


@pytest.mark.parametrize("B,train", [(23, True), (700, True), (5000, True), (300, False)])
def test_step_front_equals_separate_calls(P, B, train):
    """pcg_step_front (score pass + plan pass 1 | sort + plan pass 2) followed by the *_planned entry points gives
    bit for bit what pcg_score_table + pcg_pos_sort + pcg_choose_aggregate give: scores, sorted keys, row offsets,
    list entries, counts and aggregated rows."""
    ops = P.ops
    n = 30000
    hub_degs = [13000, 7000, 5000, 600, 300, 100, 3, 1]
    X, labels, csr = hub_graph(5, n, hub_degs)
    _, _, csrs2 = synth_graph(43, n, 32, (4,), 0.1)
    csrs = [csr, csrs2[0]]
    train_pos = np.flatnonzero(labels == 1)[:1500].tolist()
    g = P.DeviceGraph(X, csrs, train_pos, dev())
    gen = torch.Generator().manual_seed(8)
    W, b = torch.randn(2, 32, generator=gen).cuda(), torch.randn(2, generator=gen).cuda()
    rs = np.random.RandomState(B)
    nodes = np.concatenate([np.arange(len(hub_degs)), rs.randint(0, n, size=B - len(hub_degs))]).astype(np.int32)
    ids = torch.from_numpy(nodes).cuda()
    lab = torch.from_numpy(labels[nodes].astype(np.int32)).cuda() if train else None
    thr, rho = [0.5, 0.7], [0.5, 1.5]
    # separate calls
    s0_a = ops.score_table(g, W, b)
    keys_a = ops.pos_sort(g, s0_a) if train else None
    ws_a = ops.ChooseWorkspace(g, B)
    agg_a, cnt_a = ops.choose_aggregate(g, ids, lab, s0_a, keys_a, thr, rho, train, ws=ws_a)
    # front + planned
    s0_b = torch.full_like(s0_a, float("nan"))
    keys_b = torch.zeros_like(keys_a) if train else None
    ws_b = ops.ChooseWorkspace(g, B)
    kb = ops.step_front(g, W, b, s0_b, keys_b, ids, lab, thr, rho, train, ws_b)
    agg_b, cnt_b = ops.choose_aggregate(g, ids, lab, s0_b, kb, thr, rho, train, ws=ws_b, planned=True)
    torch.cuda.synchronize()
    ws_a.check(); ws_b.check()
    assert torch.equal(s0_a, s0_b)
    if train:
        half = keys_a.numel() // 2                      # (the second half of the buffer is scratch)
        assert torch.equal(keys_a[:half], keys_b[:half])
    assert torch.equal(cnt_a, cnt_b)
    assert torch.equal(agg_a.view(torch.int32), agg_b.view(torch.int32))          # bitwise, NaN-safe
    rows = g.R * B
    begin_a, begin_b = ws_a.view(0, torch.int64, rows + 1), ws_b.view(0, torch.int64, rows + 1)
    assert torch.equal(begin_a, begin_b)
    total = int(begin_a[-1])
    assert torch.equal(ws_a.view(1, torch.int32, rows), ws_b.view(1, torch.int32, rows))
    assert torch.equal(ws_a.view(2, torch.int32, total), ws_b.view(2, torch.int32, total))
    # an empty batch still refreshes scores and keys
    s0_c = torch.zeros_like(s0_a)
    empty = torch.zeros(0, dtype=torch.int32, device=dev())
    ops.step_front(g, W, b, s0_c, keys_b, empty, empty if train else None, thr, rho, train, ops.ChooseWorkspace(g, 0))
    assert torch.equal(s0_a, s0_c)


# (8192 / 8193: the last size whose LDS search index takes every 16th key and the first that takes every 32nd; 16384: the last size
#  sorted inside the select kernel)
@pytest.mark.parametrize("B,n_pos", [(300, 1500), (700, 5000), (64, 40), (64, 8192), (64, 8193), (64, 16384)])
def test_epoch_plans_and_in_kernel_sort_equal_separate_calls(P, B, n_pos):
    """pcg_plan_batches (every batch of an "epoch" planned in one launch, one plan slot each, ONE shared data part) +
    pcg_step_scores_train (scores and UNSORTED train-pos keys in one launch) + pcg_choose_gather_planned(sync_words) (the
    select kernel sorts the keys itself, rows with minority picks wait for it) give bit for bit what pcg_score_table +
    pcg_pos_sort + pcg_choose_aggregate give batch by batch: scores, sorted keys, row offsets, list entries, counts, and the
    aggregated rows of every single-chunk row."""
    import ctypes as C
    from pcgnn_amd import _lib
    lib = _lib.load()
    ops = P.ops
    _p = ops._p
    n = 30000
    hub_degs = [9000, 7000, 5000, 600, 300, 100, 3, 1]
    X, labels, csr = hub_graph(5, n, hub_degs)
    _, _, csrs2 = synth_graph(43, n, 32, (4,), 0.1)
    csrs = [csr, csrs2[0]]
    train_pos = np.flatnonzero(labels == 1)[:n_pos].tolist()
    if len(train_pos) < n_pos:                      # (more positives than the labels hold: any distinct nodes will do)
        train_pos = sorted(set(train_pos) | set(range(100, 100 + n_pos - len(train_pos))))
    if len(train_pos) < n_pos:                      # (some of those were positives already: top up to exactly n_pos)
        have = set(train_pos)
        train_pos = sorted(have | set([v for v in range(n) if v not in have][:n_pos - len(have)]))
    assert len(train_pos) == n_pos
    g = P.DeviceGraph(X, csrs, train_pos, dev())
    F, E, R = 32, 16, 2
    gen = torch.Generator().manual_seed(8)
    W, b = torch.randn(2, F, generator=gen).cuda(), torch.randn(2, generator=gen).cuda()
    n_params = int(lib.pcg_dense_n_params(F, E, R))
    theta = torch.zeros(n_params, device=dev())
    o_w, o_b = int(lib.pcg_dense_param_offset(F, E, R, 3, 0)), int(lib.pcg_dense_param_offset(F, E, R, 4, 0))
    theta[o_w:o_w + 2 * F] = W.reshape(-1)
    theta[o_b:o_b + 2] = b
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    slabs = torch.zeros(4, n_params, device=dev())
    step = torch.zeros(1, dtype=torch.int32, device=dev())
    sync = torch.zeros(int(lib.pcg_sync_words_count()), dtype=torch.int32, device=dev())
    sync[3] = 12345                                  # (pcg_step_scores_train must zero the arrival counter itself)
    rs = np.random.RandomState(B)
    n_total = 2 * B + B // 3                         # three batches, the last one shorter
    nodes = np.concatenate([np.arange(len(hub_degs)), rs.randint(0, n, size=n_total - len(hub_degs))]).astype(np.int32)
    rs.shuffle(nodes)
    ids = torch.from_numpy(nodes).cuda()
    lab = torch.from_numpy(labels[nodes].astype(np.int32)).cuda()
    thr, rho = [0.5, 0.7], [0.5, 1.5]
    thr_c, rho_c = ops._host_arrays(g, thr, rho)
    cap = int(ops.sel_capacity(g, nodes, labels[nodes], thr, rho, True).reshape(R, -1)[:, :].sum()) + 64
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    stride = int(lib.pcg_choose_plan_bytes(g.desc_ref(), B, cap))
    n_slots = -(-n_total // B)
    plans = torch.zeros(n_slots * stride, dtype=torch.uint8, device=dev())
    data = torch.zeros(int(lib.pcg_choose_data_bytes(g.desc_ref(), B, cap)), dtype=torch.uint8, device=dev())
    bump = torch.zeros(2, dtype=torch.int64, device=dev())
    st = ops._stream(dev())
    _lib.check(lib.pcg_plan_batches(g.desc_ref(), _p(ids), _p(lab), n_total, B, thr_c, rho_c, 1, 0, _p(plans), stride, cap, _p(status),
                                    _p(bump), st), "pcg_plan_batches")
    s0_b = torch.full((n,), float("nan"), device=dev())
    keys_b = torch.zeros(int(lib.pcg_pos_sort_capacity(g.n_pos)), dtype=torch.int64, device=dev())
    # separate calls (the reference for every slot)
    s0_a = ops.score_table(g, W, b)
    keys_a = ops.pos_sort(g, s0_a)
    half = keys_a.numel() // 2
    for s in range(n_slots):
        sl = slice(s * B, min((s + 1) * B, n_total))
        Bs = sl.stop - sl.start
        ids_s, lab_s = ids[sl].contiguous(), lab[sl].contiguous()
        ws_a = ops.ChooseWorkspace(g, Bs, cap)
        agg_a, cnt_a = ops.choose_aggregate(g, ids_s, lab_s, s0_a, keys_a, thr, rho, True, ws=ws_a)
        # the planned path: scores + unsorted keys, then select (sorting inside) + gather over slot s and the shared data part
        keys_b.zero_()
        state = _lib.TrainState(theta=_p(theta), m=_p(m), v=_p(v), step_counter=_p(step), sync_words=_p(sync), slabs=_p(slabs), emb=E,
                                 hyper=_lib.AdamHyper(0.01, 0.9, 0.999, 1e-8, 0.0))
        _lib.check(lib.pcg_step_scores_train(g.desc_ref(), state, _p(s0_b), _p(keys_b), None, st), "pcg_step_scores_train")
        agg_b = torch.full((R, Bs, F), float("nan"), device=dev())
        cnt_b = torch.zeros(R, Bs, dtype=torch.int32, device=dev())
        _lib.check(lib.pcg_choose_gather_planned(g.desc_ref(), _p(ids[sl]), _p(lab[sl]), Bs, _p(s0_b), None, _p(keys_b), thr_c, rho_c, 1, 0,
                                                 _p(agg_b), F, _p(cnt_b), _p(data), C.c_void_p(plans.data_ptr() + s * stride), cap,
                                                 _p(status), _p(sync), st), "pcg_choose_gather_planned")
        torch.cuda.synchronize()
        assert int(status.item()) == 0 and int(sync[3].item()) == (-(-g.n_pos // 64) if g.n_pos <= 16384 else 0)
        assert int(sync[4:].abs().sum().item()) == 0, "rank accumulators and group tickets are left zero"
        assert torch.equal(s0_a, s0_b)
        assert torch.equal(keys_a[:half], keys_b[:half]), "the in-kernel sort"
        assert torch.equal(cnt_a, cnt_b)
        rows = R * Bs
        off = lambda which: int(lib.pcg_choose_workspace_offset(g.desc_ref(), Bs, cap, which))
        plan_s = plans[s * stride:(s + 1) * stride]
        begin_a = ws_a.view(0, torch.int64, rows + 1)
        begin_b = plan_s[off(0):off(0) + 8 * (rows + 1)].view(torch.int64)
        assert torch.equal(begin_a, begin_b)
        total = int(begin_a[-1])
        len_b = plan_s[off(1):off(1) + 4 * rows].view(torch.int32)
        assert torch.equal(ws_a.view(1, torch.int32, rows), len_b)
        plan_bytes = int(lib.pcg_choose_plan_bytes(g.desc_ref(), Bs, cap))
        lo = off(2) - plan_bytes
        list_b = data[lo:lo + 4 * total].view(torch.int32)
        list_a = ws_a.view(2, torch.int32, total)
        # (only the entries in use are written: compare row by row over each row's length)
        la, lb, bg, ln = list_a.cpu().numpy(), list_b.cpu().numpy(), begin_a.cpu().numpy(), len_b.cpu().numpy()
        for row in range(rows):
            assert np.array_equal(la[bg[row]:bg[row] + ln[row]], lb[bg[row]:bg[row] + ln[row]]), (s, row)
        chunks = ws_a.view(3, torch.int32, rows + 1).cpu().numpy()
        single = torch.from_numpy(np.diff(chunks) == 1).cuda().view(R, Bs)
        assert single.any() and torch.equal(agg_a.view(torch.int32)[single], agg_b.view(torch.int32)[single])
    assert int(bump[0].item()) == 1


def test_touched_rows_only_scoring(P, monkeypatch):
    """Large-table mode: pcg_mark_touched builds a byte map per batch (centres + all their neighbours) and
    pcg_step_scores_train(touched) scores only the rows it marks - bit for bit the whole-table scores on those rows, the other
    entries of s0 untouched; the marks are exactly the batch's centres and neighbours; and two epochs of training with the mode
    forced on leave bit for bit the parameters of two epochs without it."""
    from pcgnn_amd import _lib, synth
    from pcgnn_amd.handler import PCGNNTrainer
    lib = _lib.load()
    ops = P.ops
    _p = ops._p
    w = synth.make_workload("mini", 9000, 32, (6000, 40000, 120000), 0.12, seed=3)
    g = P.DeviceGraph(w.X, w.csr, w.train_pos, dev())
    F, E, R = 32, 16, 3
    gen = torch.Generator().manual_seed(2)
    W, b = torch.randn(2, F, generator=gen).cuda(), torch.randn(2, generator=gen).cuda()
    n_params = int(lib.pcg_dense_n_params(F, E, R))
    theta = torch.zeros(n_params, device=dev())
    o_w, o_b = int(lib.pcg_dense_param_offset(F, E, R, 3, 0)), int(lib.pcg_dense_param_offset(F, E, R, 4, 0))
    theta[o_w:o_w + 2 * F] = W.reshape(-1)
    theta[o_b:o_b + 2] = b
    m, v, slabs = torch.zeros_like(theta), torch.zeros_like(theta), torch.zeros(4, n_params, device=dev())
    step = torch.zeros(1, dtype=torch.int32, device=dev())
    sync = torch.zeros(int(lib.pcg_sync_words_count()), dtype=torch.int32, device=dev())
    B, n_total = 300, 700
    rs = np.random.RandomState(1)
    nodes = rs.randint(0, w.n, size=n_total).astype(np.int32)
    ids = torch.from_numpy(nodes).cuda()
    stride = int(lib.pcg_touched_bytes(w.n))
    assert stride >= w.n + 8 and stride % 512 == 0
    maps = torch.full((3 * stride,), 7, dtype=torch.uint8, device=dev())          # (garbage: the call zeroes the maps itself)
    st = ops._stream(dev())
    queue = torch.zeros(4 + 3 * n_total, dtype=torch.int32, device=dev())
    _lib.check(lib.pcg_mark_touched(g.desc_ref(), _p(ids), n_total, B, _p(maps), stride, _p(queue), st), "pcg_mark_touched")
    # rows of hubs (> 4096 neighbours) are queued and marked by the whole grid in a launch of their own: the same marks
    Xh, lab_h, csr_h = hub_graph(11, 30000, (5000, 9000, 20000))
    gh = P.DeviceGraph(Xh, [csr_h], np.flatnonzero(lab_h == 1)[:50].tolist(), dev())
    assert gh.max_degree > 4096
    hub_nodes = np.concatenate([np.argsort(-np.diff(csr_h[0]))[:3], rs.randint(0, 30000, size=61)]).astype(np.int32)
    stride_h = int(lib.pcg_touched_bytes(30000))
    maps_h = torch.full((2 * stride_h,), 9, dtype=torch.uint8, device=dev())
    queue_h = torch.zeros(4 + 64, dtype=torch.int32, device=dev())
    _lib.check(lib.pcg_mark_touched(gh.desc_ref(), _p(torch.from_numpy(hub_nodes).cuda()), 64, 40, _p(maps_h), stride_h, _p(queue_h), st),
               "pcg_mark_touched")
    torch.cuda.synchronize()
    assert int(queue_h[0]) == 3
    for s_ in range(2):
        sl = hub_nodes[s_ * 40:(s_ + 1) * 40]
        want = np.zeros(stride_h, dtype=np.uint8)
        want[sl] = 1
        want[np.flatnonzero(lab_h == 1)[:50]] = 1
        for v_ in sl:
            want[csr_h[1][csr_h[0][v_]:csr_h[0][v_ + 1]]] = 1
        assert np.array_equal(maps_h[s_ * stride_h:(s_ + 1) * stride_h].cpu().numpy(), want), f"hub batch {s_}"
    # the same maps from the batches' PLANS (pcg_mark_touched_planned: hub rows swept range by range into LDS bitmaps that are
    # expanded into the byte maps - which also writes every other byte zero -, the other rows from the plans' records and tier
    # queues): byte for byte pcg_mark_touched's, over garbage, for both graphs (a shorter last batch in each)
    def planned_maps(gg, ids_t, labels_np, n_tot, Bq, stride_q):
        lab_t = torch.from_numpy(labels_np[ids_t.cpu().numpy()].astype(np.int32)).cuda()
        thr_c, rho_c = ops._host_arrays(gg, [0.5] * gg.R, [0.5] * gg.R)
        cap = int(ops.sel_capacity(gg, ids_t.cpu().numpy(), labels_np[ids_t.cpu().numpy()], [0.5] * gg.R, [0.5] * gg.R, True).sum()) + 64
        pst = int(lib.pcg_choose_plan_bytes(gg.desc_ref(), Bq, cap))
        n_sl = -(-n_tot // Bq)
        plans = torch.zeros(n_sl * pst, dtype=torch.uint8, device=dev())
        status = torch.zeros(1, dtype=torch.int32, device=dev())
        _lib.check(lib.pcg_plan_batches(gg.desc_ref(), _p(ids_t), _p(lab_t), n_tot, Bq, thr_c, rho_c, 1, 0, _p(plans), pst, cap, _p(status),
                                        None, st), "pcg_plan_batches")
        out = torch.full((n_sl * stride_q,), 5, dtype=torch.uint8, device=dev())
        _lib.check(lib.pcg_mark_touched_planned(gg.desc_ref(), _p(ids_t), n_tot, Bq, _p(plans), pst, cap, _p(out), stride_q, st),
                   "pcg_mark_touched_planned")
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        return out
    assert torch.equal(planned_maps(g, ids, w.labels, n_total, B, stride), maps), "planned marks == pcg_mark_touched's"
    assert torch.equal(planned_maps(gh, torch.from_numpy(hub_nodes).cuda(), lab_h, 64, 40, stride_h), maps_h), "... with hub rows"
    s0_full = ops.score_table(g, W, b)
    keys = torch.zeros(int(lib.pcg_pos_sort_capacity(g.n_pos)), dtype=torch.int64, device=dev())
    for s_ in range(3):
        sl = nodes[s_ * B:(s_ + 1) * B]
        want = np.zeros(stride, dtype=np.uint8)
        want[sl] = 1
        want[np.asarray(w.train_pos)] = 1
        for ip, ix in w.csr:
            for v_ in sl:
                want[ix[ip[v_]:ip[v_ + 1]]] = 1
        got = maps[s_ * stride:(s_ + 1) * stride].cpu().numpy()
        assert np.array_equal(got, want), f"batch {s_}: marks = centres + neighbours + train positives"
        s0 = torch.full((w.n,), -12345.0, device=dev())
        state = _lib.TrainState(theta=_p(theta), m=_p(m), v=_p(v), step_counter=_p(step), sync_words=_p(sync), slabs=_p(slabs), emb=E,
                                 hyper=_lib.AdamHyper(0.01, 0.9, 0.999, 1e-8, 0.0))
        _lib.check(lib.pcg_step_scores_train(g.desc_ref(), state, _p(s0), _p(keys), ctypes_ptr(maps, s_ * stride), st),
                   "pcg_step_scores_train")
        torch.cuda.synchronize()
        mk = torch.from_numpy(want[:w.n].astype(bool)).cuda()
        assert 0 < int(mk.sum()) < w.n
        assert torch.equal(s0[mk], s0_full[mk]), "touched rows: the whole-table scores, bit for bit"
        assert bool((s0[~mk] == -12345.0).all()), "the other rows are left alone"
    # training: the mode forced on == off, bit for bit (the selection never reads an unscored row)
    cfg = dict(engine="graph", batch_size=256, seed=5)
    monkeypatch.setenv("PCG_TOUCHED", "0")
    a = PCGNNTrainer(w, cfg, dev())
    monkeypatch.setenv("PCG_TOUCHED", "1")
    t = PCGNNTrainer(w, cfg, dev())
    assert t.fused.touched_on and not a.fused.touched_on
    t.fused.theta.copy_(a.fused.theta)
    t.fused.params_changed()
    for ep in range(2):
        a.run_epoch_one_graph()
        if ep == 0:
            t.run_epoch_one_graph()
        else:                                        # ... batch by batch too (per-batch graphs, an eager step, a stand-alone step)
            ids_e = t.start_epoch_staged()
            nb = t.batches_per_epoch()
            for k in range(nb):
                if k == 1:
                    t.fused.epoch_step_timed(k)
                else:
                    t.fused.epoch_step(k, defer=True)
    a.fused.flush(); t.fused.flush()
    torch.cuda.synchronize()
    t.fused.check()
    for name in ("theta", "m", "v", "step_counter"):
        assert torch.equal(getattr(a.fused, name), getattr(t.fused, name)), name
    ids1 = a.fused._ep_ids[:256].clone()
    lab1 = a.labels_i32[ids1.long()]
    a.fused.train_step(ids1, lab1)
    t.fused.train_step(ids1, lab1)
    torch.cuda.synchronize()
    assert torch.equal(a.fused.theta, t.fused.theta)
    # more train positives than the front launch forms keys for (> 16384): the bucket sort reads s0[train_pos] - those rows
    # must be scored in touched mode too.  One epoch each way on a graph with ~18 K train positives.
    w2 = synth.make_workload("manypos", 60000, 32, (40000, 200000), 0.75, seed=9)
    assert len(w2.train_pos) > 16384
    cfg2 = dict(engine="graph", batch_size=1024, seed=2)
    monkeypatch.setenv("PCG_TOUCHED", "0")
    a2 = PCGNNTrainer(w2, cfg2, dev())
    monkeypatch.setenv("PCG_TOUCHED", "1")
    t2 = PCGNNTrainer(w2, cfg2, dev())
    t2.fused.theta.copy_(a2.fused.theta)
    t2.fused.params_changed()
    a2.fused.stage_epoch(a2.pick_size, 1024); t2.fused.stage_epoch(t2.pick_size, 1024)
    for tr_ in (a2, t2):
        tr_.start_epoch_staged()
        for k in range(6):
            tr_.fused.epoch_step(k, defer=True)
        tr_.fused.flush()
    torch.cuda.synchronize()
    t2.fused.check()
    assert torch.equal(a2.fused.theta, t2.fused.theta) and torch.isfinite(a2.fused.theta).all()


def ctypes_ptr(t, byte_offset=0):
    import ctypes as C
    return C.c_void_p(t.data_ptr() + byte_offset)


def test_fused_trajectory_tracks_oracle(P, case):
    """Four consecutive Adam steps: the HIP path's loss trajectory and parameters follow the CPU oracle's
    (independent implementation: Python sets + torch.sort + dense-mask mean + torch autograd + torch Adam)."""
    c = case
    rho = c.rhos[0]
    m, fz = fused_of(P, c, rho)
    om = O.OraclePCGNN(torch.from_numpy(c.X), c.adj_lists(), c.train_pos, c.params(), rho, c.alpha, dense_mask=False)
    opt = O.make_adam(om, c.lr, c.wd)
    ids = torch.tensor(c.nodes, dtype=torch.int32, device=dev())
    lab = torch.from_numpy(c.batch_labels.astype(np.int32)).cuda()
    half = len(c.nodes) // 2
    for step in range(4):
        sl = slice(0, None) if step % 2 == 0 else slice(half // 2, half // 2 + half)
        want = O.train_step(om, opt, c.nodes[sl], c.batch_labels[sl])
        fz.train_step(ids[sl].contiguous(), lab[sl].contiguous())
        got = float(fz.last_loss())
        assert abs(got - want) < 2e-3 * max(1.0, abs(want)), (step, got, want)
    sd = m.state_dict()
    for k in PARAM_KEYS(c.R):
        np.testing.assert_allclose(sd[k].cpu().numpy(), om.p[k].detach().numpy(), rtol=0, atol=c.lr * 0.3, err_msg=k)


def test_list_overflow_is_reported_not_silent(P):
    """A selection list too small for a batch: the kernels select nothing and set the status word; the engine must raise at
    its next check point (last_loss / check / utils.test) instead of training on stale aggregates."""
    from pcgnn_amd import synth, utils as U
    from pcgnn_amd.handler import PCGNNTrainer
    from pcgnn_amd.fused import FusedPCGNN
    w = synth.make_workload("mini", 4000, 32, (3000, 20000, 60000), 0.12, seed=2)
    tr = PCGNNTrainer(w, dict(engine="fused", batch_size=256), dev())
    small = FusedPCGNN(tr.model, 0.01, 0.001, max_batch=256, list_capacity=500)
    ids = tr.start_epoch(0)[:256].contiguous()
    lab = tr.labels_i32[ids.long()]
    small.train_step(ids, lab)
    with pytest.raises(P.PcgnnLibraryError, match="overflow"):
        small.last_loss()
    small.check()                                   # the word was cleared by the report
    with pytest.raises(P.PcgnnLibraryError, match="overflow"):
        U.test(ids.cpu().numpy(), lab.cpu().numpy(), small, batch_size=256, print_line=False)
    # the same engine with room: no error, and the default capacity of this graph is not clipped
    tr.fused.train_step(ids, lab)
    assert np.isfinite(float(tr.fused.last_loss()))
    assert not tr.fused.clipped


def test_realloc_between_epoch_graphs(P):
    """predict() with a batch larger than max_batch re-allocates every buffer; the whole-epoch graphs captured before
    (raw pointers into the old buffers) must not be replayed afterwards: the next epoch_run re-captures and the
    trajectory equals a run that never re-allocated."""
    from pcgnn_amd import synth
    from pcgnn_amd.handler import PCGNNTrainer
    w = synth.make_workload("mini", 6000, 32, (4000, 30000, 90000), 0.12, seed=3)
    cfg = dict(engine="graph", batch_size=256, seed=5)
    a, b = PCGNNTrainer(w, cfg, dev()), PCGNNTrainer(w, cfg, dev())
    b.fused.theta.copy_(a.fused.theta)
    b.fused.params_changed()
    big = torch.arange(700, dtype=torch.int32, device=dev())
    for ep in range(3):
        a.run_epoch_one_graph()
        b.run_epoch_one_graph()
        if ep == 0:
            out = b.fused.predict(big, None, False)[0]          # B = 700 > 256: _alloc
            assert out.shape == (700, 2) and b.fused.maxB == 700 and not b.fused._ep_graphs
    torch.cuda.synchronize()
    for name in ("theta", "m", "v", "step_counter"):
        assert torch.equal(getattr(a.fused, name), getattr(b.fused, name)), name


# ---------------------------------------------------------------------------
# ingestion on the device, the reference's experiment driver
# ---------------------------------------------------------------------------
def test_device_csr_build_matches_oracle(P):
    """csr_from_pairs_device (sort + unique of (row, column) keys on the GPU) == oracle.adj_to_csr of the dict-of-sets the
    reference's sparse_to_adjlist_for_train builds (src/utils.py:243-254: symmetric, self-loops, no duplicates);
    DeviceGraph.from_adj_lists / from_scipy give the graph the host build gives."""
    import scipy.sparse as sp
    from pcgnn_amd.graph import adj_to_pairs, csr_from_pairs_device
    from pcgnn_amd import utils as U
    rs = np.random.RandomState(0)
    for n, m in ((1, 0), (300, 900), (5000, 60000)):
        src, dst = rs.randint(0, n, m), rs.randint(0, n, m)
        adj = {v: {v} for v in range(n)}
        for a, b in zip(src.tolist(), dst.tolist()):
            adj[a].add(b)
            adj[b].add(a)
        want_ip, want_ix = O.adj_to_csr(adj, n)
        ip, ix = csr_from_pairs_device(n, torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda())
        assert ip.is_cuda and np.array_equal(ip.cpu().numpy(), want_ip) and np.array_equal(ix.cpu().numpy(), want_ix)
        # the reference's dicts (already symmetric, with self-loops) through the DeviceGraph constructors
        X = rs.randn(n, 8).astype(np.float32)
        g_dev = P.DeviceGraph.from_adj_lists(torch.from_numpy(X), [adj], [], dev())
        g_host = P.DeviceGraph.from_adj_lists(torch.from_numpy(X), [adj], [], dev(), build_on_device=False)
        assert torch.equal(g_dev.indptr[0], g_host.indptr[0]) and torch.equal(g_dev.indices[0], g_host.indices[0])
        if m:
            mat = sp.csr_matrix((np.ones(m), (src, dst)), shape=(n, n))
            g_sp = P.DeviceGraph.from_scipy(torch.from_numpy(X), [mat], [], dev())
            hip, hix = U.sparse_to_csr(mat)
            assert np.array_equal(g_sp.indptr[0].cpu().numpy(), hip) and np.array_equal(g_sp.indices[0].cpu().numpy(), hix)
            assert np.array_equal(hip, want_ip) and np.array_equal(hix, want_ix)


@pytest.mark.parametrize("model_name", ["PCGNN", "SAGE", "GCN"])
def test_model_handler_train_loop(P, model_name, tmp_path):
    """ModelHandler(config).train() (src/model_handler.py:24-178): split, epochs with the pick sampler, validation every
    valid_epochs with the gain rule, best checkpoint, patience, restore, final test, ResultManager logs - on a synthetic
    dataset handed over in load_data's return format."""
    import pandas as pd
    from pcgnn_amd import synth
    from pcgnn_amd.handler import ModelHandler
    w = synth.make_workload("mini", 3000, 32, (2500, 12000, 30000), 0.15, seed=4)
    # features that carry the label: the loop has something to learn
    w.X[:, 0] += 2.0 * w.labels
    adj = [csr_to_adj(c, w.n) for c in w.csr]
    if model_name != "PCGNN":
        # the baselines see a node only through the mean over its neighbourhood (graphsage.py:62-96, 200-232): give them a
        # homophilous relation - four of five neighbours share the node's label - so that this mean carries the label too
        rs = np.random.RandomState(11)
        pools = [np.flatnonzero(w.labels == 0), np.flatnonzero(w.labels == 1)]
        homo_adj = {v: {v} for v in range(w.n)}
        for v in range(w.n):
            same = rs.rand(10) < 0.8
            for s_ in same:
                u = int(rs.choice(pools[int(w.labels[v]) if s_ else 1 - int(w.labels[v])]))
                homo_adj[v].add(u)
                homo_adj[u].add(v)
        adj = [homo_adj]
    homo = {v: set().union(*[a[v] for a in adj]) for v in range(w.n)}
    cfg = dict(data_name="yelp", model=model_name, seed=3, train_ratio=0.4, test_ratio=0.67, emb_size=32, lr=0.01, weight_decay=0.001,
               alpha=2, rho=0.5, epochs=12, valid_epochs=2, batch_size=256, patience=3, exp_num="0000",
               result_dir=str(tmp_path / "experimental_results"))
    h = ModelHandler(cfg, dataset=(homo, adj, w.X, w.labels), device=dev())
    ds = h.dataset
    assert len(ds["idx_train"]) == int(0.4 * w.n) and len(set(ds["idx_train"]) & set(ds["idx_test"])) == 0
    assert len(ds["idx_valid"]) + len(ds["idx_test"]) + len(ds["idx_train"]) == w.n
    assert ds["train_pos"] == [v for v, l in zip(ds["idx_train"], ds["y_train"]) if l == 1]
    auc, recall, f1m = h.train()
    assert 0.0 <= recall <= 1.0 and 0.0 < f1m <= 1.0
    assert auc > 0.7, "the loop learns (PCGNN from its self features, the baselines from their homophilous neighbourhood means)"
    assert h.epoch_best % 2 == 1 and h.last_epoch <= 11                      # validated at epochs 1, 3, 5, ...
    assert h.last_epoch == 11 or h.last_epoch - h.epoch_best > 3               # ran out of epochs, or stopped by patience
    # best checkpoint: saved with the reference's state-dict keys, and what the model holds after train()
    sd = torch.load(h.result.model_path, weights_only=True)
    for k, v in h.model.state_dict().items():
        assert torch.equal(v.cpu(), sd[k].cpu()), k
    if model_name == "PCGNN":
        assert {"weight", "inter1.weight", "inter1.label_clf.weight", "inter1.intra_agg3.weight", "inter1.features.weight"} <= set(sd)
    val = open(h.result.log_val_path).read()
    assert val.count("Validation performance") == (h.last_epoch + 1) // 2 and "[Epoch-001] Validation performance" in val
    assert "Test performance: - Epoch_Best: %d\t- F1:" % h.epoch_best in open(h.result.log_test_path).read()
    dt = pd.read_pickle(h.result.df_test_path)
    assert len(dt) == 1 and abs(dt["auc"].iloc[0] - auc) < 1e-9 and dt["model"].iloc[0] == model_name
    with pytest.raises(FileNotFoundError):
        ModelHandler(cfg)                                                     # (no dataset files exist offline)
