"""Host side of scoring unseen nodes (graph.QueryBatch, the argument checks of pcg_infer_new): everything here runs without a
GPU - the batch is built, sorted, de-duplicated and validated in numpy, and the C entry points reject bad arguments before
any launch."""
import ctypes as C

import numpy as np
import pytest

from oracle import pcgnn_oracle as O

N, F, R = 50, 6, 3


def base(n=N, f=F, r=R):
    from pcgnn_amd.graph import BaseShape
    return BaseShape(n, f, r)


def random_lists(seed, nq, n=N, r=R, self_loops=True):
    """per relation {query index: set(global ids)}: base neighbours, query-query edges, the node itself; row 1 of relation 0
    empty, and a row that is only its self-loop"""
    rs = np.random.RandomState(seed)
    out = []
    for rel in range(r):
        adj = {}
        for j in range(nq):
            s = set(rs.randint(0, n + nq, size=rs.randint(0, 12)).tolist())
            if self_loops:
                s.add(n + j)
            adj[j] = s
        if nq > 1 and rel == 0:
            adj[1] = set()
        if nq > 2:
            adj[2] = {n + 2}
        out.append(adj)
    return out


def raw_pairs(adjs, nq, seed=0, duplicate=True):
    """the same lists as raw (indptr, indices) pairs, rows shuffled and some entries repeated"""
    rs = np.random.RandomState(seed)
    pairs = []
    for adj in adjs:
        indptr, idx = [0], []
        for j in range(nq):
            row = list(adj.get(j, ()))
            if duplicate and row:
                row += [row[0]] * 2
            rs.shuffle(row)
            idx += row
            indptr.append(len(idx))
        pairs.append((np.asarray(indptr, np.int64), np.asarray(idx, np.int64)))
    return pairs


def test_three_constructors_agree_with_each_other_and_the_oracle():
    import scipy.sparse as sp
    from pcgnn_amd.graph import QueryBatch
    nq = 23
    X = np.random.RandomState(1).randn(nq, F).astype(np.float32)
    adjs = random_lists(2, nq)
    a = QueryBatch.from_adj_lists(X, adjs, base())
    b = QueryBatch.from_adj_lists(X, [{N + j: s for j, s in adj.items()} for adj in adjs], base())      # keys as global ids
    c = QueryBatch(X, raw_pairs(adjs, nq), base())
    mats = []
    for adj in adjs:
        rows = [j for j, s in adj.items() for _ in s]
        cols = [v for s in adj.values() for v in s]
        mats.append(sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(nq, N + nq)))
    d = QueryBatch.from_scipy(X, mats, base())
    for r, adj in enumerate(adjs):
        want_ptr, want_idx = O.adj_to_csr(adj, nq)
        for q in (a, b, c, d):
            ip, ix = q.csr[r]
            assert ip.dtype == np.int64 and ix.dtype == np.int32
            assert np.array_equal(ip, want_ptr) and np.array_equal(ix, want_idx)
    for q in (a, b, c, d):
        assert q.nq == nq and q.n_base == N and q.R == R and q.feat_dim == F
        assert np.array_equal(q.X_host, X)


def test_rows_ascending_and_deduplicated():
    from pcgnn_amd.graph import QueryBatch
    nq = 4
    X = np.zeros((nq, F), np.float32)
    indptr = np.array([0, 5, 5, 8, 9], np.int64)
    indices = np.array([52, 3, 3, 52, 0, 7, 7, 7, 53], np.int64)
    q = QueryBatch(X, [(indptr, indices)] * R, base())
    for r in range(R):
        ip, ix = q.csr[r]
        assert ip.tolist() == [0, 3, 3, 4, 5] and ix.tolist() == [0, 3, 52, 7, 53]
        for j in range(nq):
            row = ix[ip[j]:ip[j + 1]]
            assert np.all(np.diff(row) > 0)
        assert q.deg_host[r].tolist() == [3, 0, 1, 1]
    assert q.max_degree == 3


def test_degrees_and_list_capacities_match_the_row_rule():
    from pcgnn_amd import _lib
    from pcgnn_amd.fused import infer_chunks, infer_row_caps
    from pcgnn_amd.graph import QueryBatch
    lib = _lib.load()
    nq = 41
    X = np.zeros((nq, F), np.float32)
    adjs = random_lists(5, nq)
    adjs[1][7] = set(range(0, 40))                    # a longer row: deg > k + 1 at every threshold below 1
    q = QueryBatch.from_adj_lists(X, adjs, base())
    assert q.max_degree == max(len(s) for adj in adjs for s in adj.values()) == 40
    for r, adj in enumerate(adjs):
        assert q.deg_host[r].tolist() == [len(adj[j]) for j in range(nq)]
    for thr in ([0.5] * R, [0.2, 0.5, 1.0]):
        want = np.array([sum(lib.pcg_sel_capacity_row(int(q.deg_host[r][j]), thr[r], 0.0, 0, 0, 0) for r in range(R))
                         for j in range(nq)], dtype=np.int64)
        caps = infer_row_caps(q.deg_host, thr)
        assert np.array_equal(caps, want)
        ids = np.array([7, 7, 0, 40, 3, 1], dtype=np.int64)
        assert np.array_equal(infer_row_caps(q.deg_host, thr, ids), want[ids])
        for chunk in (1, 4, 16, 41, 100):
            _, cap = infer_chunks(caps, chunk)
            assert cap == max(1, max(int(want[lo:lo + chunk].sum()) for lo in range(0, nq, chunk)))


def test_validation_errors_name_relation_and_row():
    from pcgnn_amd.graph import QueryBatch
    nq = 5
    X = np.zeros((nq, F), np.float32)
    ok = (np.array([0, 1, 2, 3, 4, 5], np.int64), np.array([0, 1, 2, 3, N + 4], np.int64))
    QueryBatch(X, [ok] * R, base())
    with pytest.raises(ValueError, match="feature width 7"):
        QueryBatch(np.zeros((nq, F + 1), np.float32), [ok] * R, base())
    with pytest.raises(ValueError, match="2 relations, the base graph 3"):
        QueryBatch(X, [ok] * 2, base())
    # a neighbour id beyond N + nq, and a negative one: relation and row named
    bad = (ok[0], np.array([0, 1, 2, N + nq, N + 4], np.int64))
    with pytest.raises(ValueError, match=rf"relation 1, row 3: neighbour id {N + nq} outside \[0, {N + nq}\)"):
        QueryBatch(X, [ok, bad, ok], base())
    bad = (ok[0], np.array([0, 1, -1, 3, 4], np.int64))
    with pytest.raises(ValueError, match=r"relation 2, row 2: neighbour id -1"):
        QueryBatch(X, [ok, ok, bad], base())
    # indptr not monotone / wrong length / wrong end
    bad = (np.array([0, 2, 1, 3, 4, 5], np.int64), ok[1])
    with pytest.raises(ValueError, match=r"relation 0, row 1: indptr is not monotone"):
        QueryBatch(X, [bad, ok, ok], base())
    with pytest.raises(ValueError, match=r"relation 1: indptr has 5 entries"):
        QueryBatch(X, [ok, (ok[0][:-1], ok[1]), ok], base())
    with pytest.raises(ValueError, match=r"relation 2, row 4: indptr ends at 4"):
        QueryBatch(X, [ok, ok, (np.array([0, 1, 2, 3, 4, 4], np.int64), ok[1])], base())
    # ids must fit int32: a base graph that leaves no room for the batch
    with pytest.raises(ValueError, match="int32"):
        QueryBatch(X, [ok] * R, base(n=(1 << 31) - 3))
    # the reference's form: a key that is no query node; a scipy matrix of the wrong shape
    with pytest.raises(ValueError, match=r"relation 1, row 9: not a query node"):
        QueryBatch.from_adj_lists(X, [{0: {1}}, {9: {1}}, {}], base())
    with pytest.raises(ValueError, match=r"relation 0, row 17: neighbour id 1000"):
        QueryBatch.from_adj_lists(np.zeros((20, F), np.float32), [{17: {1000}}, {}, {}], base())
    # a batch larger than the base graph: a key in [N, nq) is both a query index and a global id - said, not guessed
    small, Xb = base(n=5), np.zeros((10, F), np.float32)
    with pytest.raises(ValueError, match=r"relation 0, row 7: the key is both"):
        QueryBatch.from_adj_lists(Xb, [{7: {1}}, {}, {}], small)
    assert QueryBatch.from_adj_lists(Xb, [{7: {1}}, {}, {}], small, keys="index").deg_host[0].tolist() == [0] * 7 + [1, 0, 0]
    assert QueryBatch.from_adj_lists(Xb, [{7: {1}}, {}, {}], small, keys="global").deg_host[0].tolist() == [0, 0, 1] + [0] * 7
    with pytest.raises(ValueError, match=r"relation 0, row 3: not a query node"):
        QueryBatch.from_adj_lists(Xb, [{3: {1}}, {}, {}], small, keys="global")
    import scipy.sparse as sp
    with pytest.raises(ValueError, match=r"relation 0: matrix shape"):
        QueryBatch.from_scipy(X, [sp.csr_matrix((nq, N))] * R, base())


def test_empty_batch_is_accepted():
    from pcgnn_amd.fused import infer_chunks, infer_row_caps
    from pcgnn_amd.graph import QueryBatch
    X = np.zeros((0, F), np.float32)
    q = QueryBatch(X, [(np.zeros(1, np.int64), np.zeros(0, np.int64))] * R, base())
    assert q.nq == 0 and q.max_degree == 0 and all(d.size == 0 for d in q.deg_host)
    assert QueryBatch.from_adj_lists(X, [{}] * R, base()).nq == 0
    caps = infer_row_caps(q.deg_host, [0.5] * R)
    assert caps.size == 0 and infer_chunks(caps, 8) == ([], 1)


def host_desc(n_nodes, feat_dim=32, n_rel=3, max_degree=100, feat_stride=None):
    from pcgnn_amd import _lib
    d = _lib.GraphDesc()
    d.n_nodes, d.feat_dim, d.feat_stride = n_nodes, feat_dim, feat_stride or (feat_dim + 3) // 4 * 4
    d.n_rel, d.n_pos, d.max_degree = n_rel, 0, max_degree
    return d


def test_c_entry_points_reject_bad_arguments_before_any_launch():
    from pcgnn_amd import _lib
    lib = _lib.load()
    thr = (C.c_double * 3)(0.5, 0.5, 0.5)
    call = lambda g, q: lib.pcg_infer_new(g, q, None, 64, None, 4, 4, None, 1, thr, None, 100, None, None, None, None)
    assert call(None, None) == _lib.PCG_E_ARG
    g = host_desc(1000)
    assert call(C.byref(g), None) == _lib.PCG_E_ARG and call(None, C.byref(host_desc(4))) == _lib.PCG_E_ARG
    for q in (host_desc(4, feat_dim=31), host_desc(4, feat_stride=36), host_desc(4, n_rel=2)):
        assert call(C.byref(g), C.byref(q)) == _lib.PCG_E_ARG
        assert lib.pcg_infer_new_workspace_bytes(C.byref(g), C.byref(q), 64, 4, 100) == _lib.PCG_E_ARG
    # matching tables but no pointers: still rejected before a launch
    assert call(C.byref(g), C.byref(host_desc(4))) == _lib.PCG_E_ARG
    # nothing to do: n == 0 or nq == 0 enqueue nothing and need no pointers
    assert lib.pcg_infer_new(C.byref(g), C.byref(host_desc(4)), None, 64, None, 0, 4, None, 1, thr, None, 100, None, None, None,
                             None) == _lib.PCG_OK
    assert call(C.byref(g), C.byref(host_desc(0))) == _lib.PCG_OK


def test_workspace_bytes():
    from pcgnn_amd import _lib
    lib = _lib.load()
    g = host_desc(100000, max_degree=5000)
    for q_deg in (1, 300, 5000):
        q = host_desc(1000, max_degree=q_deg)
        for chunk, cap in ((1, 1), (17, 900), (1000, 250000), (16384, 1 << 22)):
            new = lib.pcg_infer_new_workspace_bytes(C.byref(g), C.byref(q), 64, chunk, cap)
            assert new > 0
            assert new >= lib.pcg_infer_workspace_bytes(C.byref(q), 64, chunk, cap)
            assert new >= lib.pcg_infer_workspace_bytes(C.byref(g), 64, chunk, cap)
    q = host_desc(1000)
    assert lib.pcg_infer_new_workspace_bytes(None, C.byref(q), 64, 16, 100) < 0
    assert lib.pcg_infer_new_workspace_bytes(C.byref(g), None, 64, 16, 100) < 0
    assert lib.pcg_infer_new_workspace_bytes(C.byref(g), C.byref(q), 64, 0, 100) < 0
    assert lib.pcg_infer_new_workspace_bytes(C.byref(g), C.byref(q), 64, 16, 0) < 0
    assert lib.pcg_infer_new_workspace_bytes(C.byref(g), C.byref(q), 60, 16, 100) < 0
    assert lib.pcg_infer_new_workspace_bytes(C.byref(g), C.byref(host_desc(1000, n_rel=1)), 64, 16, 100) < 0
