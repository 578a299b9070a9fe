"""Scoring nodes that are not in the resident graph (FusedPCGNN.infer_new / pcg_infer_new) on the GPU.

The oracle is an identity, not a tolerance: a FULL graph of N + nq nodes is built, the query is its last nq nodes (their feature
rows and their CSR rows, global ids), the BASE graph is rows [0, N) with every neighbour >= N dropped; with the same theta in both
engines ``base.infer_new(query)`` must be ``torch.equal`` to ``full.infer(arange(N, N + nq))``, gnn and centre logits both.

Golden fixtures: a fixture's graph has 700 .. 1500 nodes, fewer than the largest batch (1000), so the fixture's graph is the
BASE part and the nq query nodes are generated behind it (random features; edges from every query node to random nodes of
the whole id range, symmetrised, self-loops, de-duplicated - the generators' recipe, synth._csr_from_pairs): the full graph
restricted to [0, N) is the fixture's graph."""
import numpy as np
import pytest
import torch

from tests.util import GoldenCase

pytestmark = pytest.mark.gpu

# two fixed-shape inference kernels (with / without the weights' LDS copy) and the run-time-shape one that streams the weights:
# no fixture's shape passes infer_wlds outside the fixed ones - the run-time LDS-weight kernel is tests/test_gpu_edge_shapes.py's
GOLDEN_CASES = ["yelp_small", "yelp_emb128", "feat100", "five_rel", "single_rel"]


def dev():
    return torch.device("cuda", 0)


# ---- graph surgery on the host ------------------------------------------------------------------------------------------
def grow(X, csrs, nq, seed, avg_deg=6):
    """the graph + nq generated nodes behind it: (X_full, csrs_full), symmetric, self-loops, no duplicates"""
    from pcgnn_amd.synth import _csr_from_pairs
    rs = np.random.RandomState(seed)
    n = X.shape[0]
    nf = n + nq
    Xf = np.concatenate([X, rs.randn(nq, X.shape[1]).astype(np.float32)])
    out = []
    for indptr, idx in csrs:
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
        m = nq * avg_deg
        src = rs.randint(n, nf, size=m).astype(np.int64)
        dst = rs.randint(0, nf, size=m).astype(np.int64)
        out.append(_csr_from_pairs(nf, np.concatenate([rows, src]), np.concatenate([idx.astype(np.int64), dst])))
    return Xf, out


def append_rows(X, csrs, Xnew, rows_per_rel):
    """explicit rows behind the graph (directed: only the new rows' own lists): rows_per_rel[r][i] = ids of new node i"""
    Xf = np.concatenate([X, Xnew.astype(np.float32)])
    out = []
    for (indptr, idx), rows in zip(csrs, rows_per_rel):
        rows = [np.unique(np.asarray(r, dtype=np.int64)).astype(np.int32) for r in rows]
        lens = np.array([len(r) for r in rows], dtype=np.int64)
        ip = np.concatenate([indptr, indptr[-1] + np.cumsum(lens)])
        out.append((ip, np.concatenate([idx] + rows).astype(np.int32)))
    return Xf, out


def split(Xf, csrs_full, N):
    """(X_base, csrs_base, X_query, raw query pairs): rows [0, N) without neighbours >= N | rows [N, ..) as they are"""
    base, query = [], []
    for indptr, idx in csrs_full:
        head = idx[:indptr[N]]
        keep = head < N
        rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(indptr[:N + 1]))
        ip = np.zeros(N + 1, dtype=np.int64)
        np.cumsum(np.bincount(rows[keep], minlength=N), out=ip[1:])
        base.append((ip, head[keep].astype(np.int32)))
        query.append((indptr[N:] - indptr[N], idx[indptr[N]:]))
    return Xf[:N], base, Xf[N:], query


# ---- engines -----------------------------------------------------------------------------------------------------------
def engine(X, csrs, train_pos, emb, thresholds, params=None, alpha=2.0, seed=0):
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
    model = P.PCALayer(2, inter, alpha)
    if params is not None:
        sd = model.state_dict()
        for k, v in params.items():
            sd[k].copy_(v)
    return FusedPCGNN(model.cuda(), 0.01, 0.001, max_batch=256)


def same_theta(dst, src):
    src.flush()
    dst.theta.copy_(src.theta)
    dst.params_changed()


def assert_identity(base, full, query, N, ids=None, chunk=None, **kw):
    local = np.arange(query.nq) if ids is None else (ids.cpu().numpy() if torch.is_tensor(ids) else np.asarray(ids))
    want_g, want_c = full.infer(torch.as_tensor(N + local, dtype=torch.int32, device=dev()), want_center=True)
    got_g, got_c = base.infer_new(query, ids=ids, chunk=chunk, want_center=True, **kw)
    assert got_g.shape == (len(local), 2) and got_c.shape == (len(local), 2)
    assert torch.equal(got_g, want_g), f"gnn logits differ (chunk {chunk})"
    assert torch.equal(got_c, want_c), f"centre logits differ (chunk {chunk})"
    assert bool(torch.isfinite(got_c).all())
    return got_g


# ---- the golden fixtures' graphs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 17, 1000])
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_identity_golden_graphs(name, nq):
    from pcgnn_amd.graph import QueryBatch
    c = GoldenCase(name)
    Xf, full_csr = grow(c.X, c.csr, nq, seed=nq)
    Xb, base_csr, Xq, q_pairs = split(Xf, full_csr, c.n)
    for (ip, ix), (fp, fx) in zip(base_csr, c.csr):            # the base part is the fixture's graph (+ self-loops it may lack)
        assert set(zip(np.repeat(np.arange(c.n), np.diff(fp)).tolist(), fx.tolist())) <= \
            set(zip(np.repeat(np.arange(c.n), np.diff(ip)).tolist(), ix.tolist()))
    thr = [0.5] * c.R
    full = engine(Xf, full_csr, c.train_pos, c.emb, thr, c.params(), c.alpha)
    base = engine(Xb, base_csr, c.train_pos, c.emb, thr, c.params(), c.alpha)
    query = QueryBatch(Xq, q_pairs, base.g)
    assert query.nq == nq
    assert_identity(base, full, query, c.n)
    if nq > 1:
        assert_identity(base, full, query, c.n, chunk=7)
    base.check()


@pytest.mark.parametrize("thr", [0.2, 1.0])
def test_identity_thresholds_golden(thr):
    from pcgnn_amd.graph import QueryBatch
    c = GoldenCase("yelp_small")
    Xf, full_csr = grow(c.X, c.csr, 300, seed=3, avg_deg=40)
    Xb, base_csr, Xq, q_pairs = split(Xf, full_csr, c.n)
    full = engine(Xf, full_csr, c.train_pos, c.emb, [thr] * c.R, c.params(), c.alpha)
    base = engine(Xb, base_csr, c.train_pos, c.emb, [thr] * c.R, c.params(), c.alpha)
    query = QueryBatch(Xq, q_pairs, base.g)
    assert_identity(base, full, query, c.n)
    assert_identity(base, full, query, c.n, chunk=64)


# ---- power law: 200 K nodes / 4 M edges + explicit rows of every kind ----------------------------------------------------
N_GEN_QUERY = 2000


@pytest.fixture(scope="module")
def powerlaw():
    from pcgnn_amd import synth
    from pcgnn_amd.graph import BaseShape, QueryBatch
    w = synth.power_law(200_000, 4_000_000, 0, max_share=5e-3)
    n_gen = w.n
    N = n_gen - N_GEN_QUERY
    rs = np.random.RandomState(11)
    n_special = 9
    n_all = n_gen + n_special
    me = lambda i: n_gen + i
    pick = lambda k: rs.choice(n_all, size=k, replace=False)
    special = [
        lambda r: [] if r == 0 else [me(0), 5, 17, N + 3],            # 0: no neighbour at all in relation 0
        lambda r: [me(1)],                                             # 1: its only neighbour is itself
        lambda r: [me(2), me(3), N + 1, N + 100],                      # 2, 3: query-query edges only
        lambda r: [me(3), me(0), N + 7],
        lambda r: pick(129),                                           # 4 .. 7: more than one 128-entry gather chunk
        lambda r: pick(500),
        lambda r: pick(2000),
        lambda r: pick(4096),
        lambda r: pick(6000),                                          # 8: hub tier (> 4096)
    ]
    R = len(w.csr)
    rows = [[special[i](r) for i in range(n_special)] for r in range(R)]
    Xf, full_csr = append_rows(w.X, w.csr, rs.randn(n_special, w.X.shape[1]), rows)
    Xb, base_csr, Xq, q_pairs = split(Xf, full_csr, N)
    query = QueryBatch(Xq, q_pairs, BaseShape(N, Xf.shape[1], R))
    train_pos = [v for v in w.train_pos if v < N]
    return dict(N=N, Xf=Xf, full_csr=full_csr, Xb=Xb, base_csr=base_csr, query=query, train_pos=train_pos, first_special=N_GEN_QUERY)


def powerlaw_engines(p, thr):
    full = engine(p["Xf"], p["full_csr"], p["train_pos"], 64, [thr] * 3, seed=4)
    base = engine(p["Xb"], p["base_csr"], p["train_pos"], 64, [thr] * 3, seed=4)
    same_theta(base, full)
    return base, full


def test_power_law_query_has_every_kind_of_row(powerlaw):
    q, N, s = powerlaw["query"], powerlaw["N"], powerlaw["first_special"]
    assert q.nq == N_GEN_QUERY + 9
    deg = np.stack(q.deg_host)                                          # [R, nq]
    row = lambda r, j: q.csr[r][1][q.csr[r][0][j]:q.csr[r][0][j + 1]]
    assert deg[0, s] == 0 and deg[1, s] > 0                             # no neighbour at all in one relation
    assert all(row(r, s + 1).tolist() == [N + s + 1] for r in range(3))  # its only neighbour is itself
    assert all(row(r, j).min() >= N for r in range(3) for j in (s + 2, s + 3))   # query-query edges only
    multi = [int(deg[0, s + i]) for i in (4, 5, 6, 7)]
    assert all(129 <= d <= 4096 for d in multi) and multi[0] == 129 and multi[-1] == 4096
    assert deg[0, s + 8] > 4096                                         # hub tier
    assert ((deg[:, :s] > 128).any())                                   # generator rows beyond one chunk, too
    # generator rows mix base and query neighbours
    gen = np.concatenate([row(r, j) for r in range(3) for j in range(0, s, 50)])
    assert (gen < N).any() and (gen >= N).any()


@pytest.mark.parametrize("thr", [0.5, 0.2, 1.0])
def test_identity_power_law(powerlaw, thr):
    base, full = powerlaw_engines(powerlaw, thr)
    q, N = powerlaw["query"], powerlaw["N"]
    assert_identity(base, full, q, N)                                   # all rows, one chunk
    if thr != 0.5:
        return
    assert_identity(base, full, q, N, chunk=300)                        # many chunks + a short tail (2009 = 6 * 300 + 209)
    assert_identity(base, full, q, N, chunk=2008)                       # a tail of one row
    rs = np.random.RandomState(6)
    special = np.arange(N_GEN_QUERY, q.nq)
    ids = np.concatenate([rs.choice(q.nq, size=700, replace=False), special, special[:5], rs.choice(q.nq, size=40)])
    rs.shuffle(ids)
    assert len(np.unique(ids)) < len(ids)
    assert_identity(base, full, q, N, ids=ids)
    assert_identity(base, full, q, N, ids=ids, chunk=97)
    assert_identity(base, full, q, N, ids=torch.as_tensor(ids, dtype=torch.int32, device=dev()), chunk=500)
    g, c = base.infer_new(q, ids=np.zeros(0, np.int64), want_center=True)       # an ids of length 0
    assert g.shape == (0, 2) and c.shape == (0, 2)
    assert base.infer_new(q, ids=[]).shape == (0, 2)
    base.check()


# ---- the base-score cache -----------------------------------------------------------------------------------------------
def mini():
    from pcgnn_amd import synth
    from pcgnn_amd.graph import QueryBatch
    from pcgnn_amd.handler import PCGNNTrainer
    w = synth.make_workload("mini", 6000, 32, (4000, 30000, 90000), 0.12, seed=3)
    N = w.n

    def mkq(t, nq=500):
        Xf, full_csr = grow(w.X, w.csr, nq, seed=9, avg_deg=20)
        _, base_csr, Xq, q_pairs = split(Xf, full_csr, N)
        for (ip, ix), (wp, wx) in zip(base_csr, w.csr):
            assert np.array_equal(ip, wp) and np.array_equal(ix, wx)     # the base part is the workload's graph
        return QueryBatch(Xq, q_pairs, t.fused.g)

    mk = lambda: PCGNNTrainer(w, dict(engine="graph", seed=5, batch_size=256), dev())
    return w, mk, mkq


def test_score_cache():
    w, mk, mkq = mini()
    a = mk()
    fz = a.fused
    q = mkq(a)
    first = fz.infer_new(q, want_center=True)
    assert fz._new_scored_base
    second = fz.infer_new(q, want_center=True)                          # score_base = 0 taken
    assert not fz._new_scored_base
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    forced = fz.infer_new(q, want_center=True, reuse_scores=False)
    assert fz._new_scored_base
    assert torch.equal(first[0], forced[0]) and torch.equal(first[1], forced[1])
    # a batch larger than the buffer's capacity (500 rows -> room for 512): the buffer grows to the next power of two and holds
    # no scores; afterwards the smaller batch fits the grown buffer and reuses them
    assert fz._inf["new_s0"].numel() == w.n + 512
    big = mkq(a, 600)
    fz.infer_new(big)
    assert fz._new_scored_base and fz._inf["new_s0"].numel() == w.n + 1024
    fz.infer_new(big)
    assert not fz._new_scored_base
    again = fz.infer_new(q, want_center=True)
    assert not fz._new_scored_base
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    # two training steps: the cached scores must be discarded
    ids = torch.as_tensor(w.idx_train[:256], dtype=torch.int32, device=dev())
    lab = torch.as_tensor(w.labels[w.idx_train[:256]], dtype=torch.int32, device=dev())
    theta0 = fz.theta.clone()
    fz.train_step(ids, lab)
    fz.train_step(ids, lab, defer=True)                                 # (its update is applied by infer_new's flush)
    after = fz.infer_new(q, want_center=True)
    assert fz._new_scored_base
    assert not torch.equal(fz.theta, theta0) and not torch.equal(after[0], first[0])
    b = mk()
    same_theta(b.fused, fz)
    want = b.fused.infer_new(mkq(b), want_center=True)
    assert torch.equal(after[0], want[0]) and torch.equal(after[1], want[1])
    again = fz.infer_new(q, want_center=True)
    assert not fz._new_scored_base
    assert torch.equal(after[0], again[0]) and torch.equal(after[1], again[1])
    # parameters loaded from outside
    b.model.load_state_dict(a.model.state_dict())
    b.fused.infer_new(mkq(b))
    assert b.fused._new_scored_base
    fz.check()


def test_training_engine_untouched():
    """a group, infer_new, two more groups == a group, flush, two more groups - bit for bit; no re-capture, no re-allocation"""
    w, mk, mkq = mini()
    a, b = mk(), mk()
    b.fused.theta.copy_(a.fused.theta)
    b.fused.params_changed()
    for t in (a, b):
        t.run_epoch_one_graph(n_epochs=2)
    maxB, graphs, fresh = a.fused.maxB, dict(a.fused._ep_graphs), a.fused._fresh
    s0 = a.fused.s0.clone()
    q = mkq(a)
    a.fused.infer_new(q, chunk=130, want_center=True)
    a.fused.infer_new(q)
    b.fused.flush()
    torch.cuda.synchronize()
    assert a.fused._fresh == fresh and torch.equal(a.fused.s0, s0)
    for t in (a, b):
        for _ in range(2):
            t.run_epoch_one_graph(n_epochs=2)
    torch.cuda.synchronize()
    for name in ("theta", "m", "v", "step_counter", "clf_next"):
        assert torch.equal(getattr(a.fused, name), getattr(b.fused, name)), name
    assert a.fused.maxB == maxB
    assert set(a.fused._ep_graphs) == set(graphs) and len(b.fused._ep_graphs) == len(graphs)
    assert all(a.fused._ep_graphs[k] is gr for k, gr in graphs.items())
    a.fused.infer_new(q)
    assert a.fused._new_scored_base                           # (the epochs wrote theta)


def test_overflow_is_reported_and_later_calls_work():
    from pcgnn_amd import PcgnnLibraryError
    w, mk, mkq = mini()
    a = mk()
    q = mkq(a)
    want = a.fused.infer_new(q)
    with pytest.raises(PcgnnLibraryError, match="selection list overflow"):
        a.fused.infer_new(q, _list_capacity=50)
    assert torch.equal(a.fused.infer_new(q), want)
    assert torch.equal(a.fused.infer(None, chunk=2500), a.fused.infer(None))
    a.fused.check()


def test_predict_proba_new():
    from pcgnn_amd import utils as U
    w, mk, mkq = mini()
    a = mk()
    q = mkq(a)
    logits = a.fused.infer_new(q)
    prob = U.predict_proba_new(q, a.fused)
    assert prob.dtype == np.float32 and prob.shape == (q.nq,)
    assert np.array_equal(prob, torch.sigmoid(logits).float().cpu().numpy()[:, 1])
    ids = np.array([5, 5, 499, 0])
    assert np.array_equal(U.predict_proba_new(q, a.fused, ids=ids), prob[ids])
