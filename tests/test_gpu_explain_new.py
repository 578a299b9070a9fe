"""Explaining nodes that are not in the resident graph (FusedPCGNN.chosen_new / attribute_new, utils.explain_new; pcg_explain_new)
on the GPU.  Run with ``pytest -m gpu``.

The oracle is an identity, not a tolerance - the one ``infer_new`` is tested with (tests/test_gpu_infer_new.py, whose graph
surgery this module imports): a FULL graph of N + nq nodes, the query its last nq nodes, the BASE graph rows [0, N) without
neighbours >= N, the same theta in both engines.  Then for query row j

    base.chosen_new(query) / base.attribute_new(query, neighbours=True)   must have the BITS of
    full.chosen(N + j)     / full.attribute(N + j, neighbours=True)

offsets, ids, dist, logits (also ``base.infer_new``'s), d_self, d_agg, self_contrib, rel_contrib, neigh_contrib.  Every float
comparison is ``torch.equal`` on the int32 view: the bit patterns, so that a NaN (a row with an empty neighbour set may have
some) has to be the same NaN.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_gpu_infer_new import append_rows, engine, grow, mini, same_theta, split
from tests.util import GoldenCase

pytestmark = pytest.mark.gpu

ATTR_KEYS = ("logits", "d_self", "d_agg", "self_contrib", "rel_contrib")
TARGETS = ((0.0, 1.0), (-1.0, 1.0))


def dev():
    return torch.device("cuda", 0)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {tuple(a.shape)} {a.dtype} != {tuple(b.shape)} {b.dtype}"
    assert torch.equal(bits(a), bits(b)), f"{what} differs"


# ---- the oracle: rows of a whole-set result of the FULL engine ---------------------------------------------------------------
class Oracle:
    """full.attribute(arange(N, N + nq), neighbours=True), computed once per (engine, target); ``rows(local)`` restates it for
    any list of query-local rows (duplicates allowed) in the layout a call with those ids returns"""

    def __init__(self, full, N, nq, target=(0.0, 1.0)):
        self.at = full.attribute(torch.arange(N, N + nq, dtype=torch.int32, device=dev()), target=target, neighbours=True)
        self.h = np.asarray(self.at.chosen.host_offsets())
        self.nq, self.R = nq, self.at.chosen.R

    def rows(self, local=None):
        at = self.at
        if local is None:
            return dict(offsets=at.chosen.flat_offsets, ids=at.chosen.ids, dist=at.chosen.dist, neigh_contrib=at.neigh_contrib,
                        **{k: getattr(at, k) for k in ATTR_KEYS})
        local = (local.cpu().numpy() if torch.is_tensor(local) else np.asarray(local)).astype(np.int64).reshape(-1)
        sel = torch.from_numpy(local).to(dev())
        lo = np.concatenate([self.h[r * self.nq + local] for r in range(self.R)])
        ln = np.concatenate([self.h[r * self.nq + local + 1] for r in range(self.R)]) - lo
        off = np.zeros(ln.size + 1, dtype=np.int64)
        np.cumsum(ln, out=off[1:])
        idx = np.repeat(lo - off[:-1], ln) + np.arange(int(off[-1]), dtype=np.int64)
        idx = torch.from_numpy(idx).to(dev())
        return dict(offsets=torch.from_numpy(off).to(dev()), ids=at.chosen.ids[idx], dist=at.chosen.dist[idx],
                    neigh_contrib=at.neigh_contrib[idx], logits=at.logits[sel], d_self=at.d_self[sel], d_agg=at.d_agg[:, sel],
                    self_contrib=at.self_contrib[sel], rel_contrib=at.rel_contrib[:, sel])


def same_chosen(ch, want, what):
    same(ch.flat_offsets, want["offsets"], f"{what}: offsets")
    assert np.array_equal(np.asarray(ch.host_offsets()), want["offsets"].cpu().numpy()), f"{what}: host offsets"
    same(ch.ids, want["ids"], f"{what}: ids")
    same(ch.dist, want["dist"], f"{what}: dist")


def same_attr(at, want, what, neighbours=True):
    for k in ATTR_KEYS:
        same(getattr(at, k), want[k], f"{what}: {k}")
    if neighbours:
        same_chosen(at.chosen, want, what)
        same(at.neigh_contrib, want["neigh_contrib"], f"{what}: neigh_contrib")
    else:
        assert at.chosen is None and at.neigh_contrib is None


def assert_explained(base, oracle, query, ids=None, chunk=None, groups_alone=False):
    """the combined call against the oracle and ``infer_new``; groups_alone: each group requested alone has the same bits"""
    want = oracle.rows(ids)
    what = f"n {want['logits'].shape[0]} chunk {chunk}"
    at = base.attribute_new(query, ids=ids, chunk=chunk, target=oracle.at.target, neighbours=True)
    same_attr(at, want, what)
    same(at.logits, base.infer_new(query, ids=ids, chunk=chunk), f"{what}: logits against infer_new")
    if groups_alone:
        same_chosen(base.chosen_new(query, ids=ids, chunk=chunk), want, f"{what}, chosen_new alone")
        same_attr(base.attribute_new(query, ids=ids, chunk=chunk, target=oracle.at.target), want, f"{what}, attribution alone", False)
    return at


# ---- 1. the golden fixtures' graphs: the fixed-shape and the streamed run-time attribution instantiations -------------------
GOLDEN_CASES = ["yelp_small", "yelp_emb128", "feat100", "amazon_small", "five_rel", "single_rel"]


def golden_pair(name, nq):
    from pcgnn_amd.graph import QueryBatch
    c = GoldenCase(name)
    Xf, full_csr = grow(c.X, c.csr, nq, seed=nq)
    Xb, base_csr, Xq, q_pairs = split(Xf, full_csr, c.n)
    thr = [0.5] * c.R
    full = engine(Xf, full_csr, c.train_pos, c.emb, thr, c.params(), c.alpha)
    base = engine(Xb, base_csr, c.train_pos, c.emb, thr, c.params(), c.alpha)
    query = QueryBatch(Xq, q_pairs, base.g)
    assert query.nq == nq
    return c, base, full, query


@pytest.mark.parametrize("nq", [1, 17, 1000])
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_identity_golden_graphs(name, nq):
    c, base, full, query = golden_pair(name, nq)
    for target in TARGETS:
        at = assert_explained(base, Oracle(full, c.n, nq, target), query)
        assert at.target == target and at.d_self.shape == (nq, c.f) and at.d_agg.shape == (c.R, nq, c.f)
        assert bool(torch.isfinite(at.logits).all())
        # the Attribution is built over the query's own table: its shares and its residual work as for resident nodes
        assert torch.allclose(at.feature_contrib().sum(1), at.self_contrib, rtol=1e-4, atol=1e-4)
        assert float(at.completeness_residual().abs().max()) <= 1e-3 * max(1.0, float(at.target_logit().abs().max()))
    base.check()


# ---- 2. one explicit query: a row at every boundary the path has ---------------------------------------------------------------
KEPT = (16, 17, 63, 64, 65, 128, 129, 400, 2047, 2048, 2049)     # a row of `c` and a row of `2 c` neighbours for each
HUB = 10300
N_FILL = 300                                                     # generated query rows in front of the explicit ones


@pytest.fixture(scope="module")
def explicit():
    from pcgnn_amd import synth
    from pcgnn_amd.graph import BaseShape, QueryBatch
    w = synth.make_workload("explain-base", 12000, 32, (8000, 60000, 180000), 0.12, seed=3)
    N, R = w.n, len(w.csr)
    Xg, csr_g = grow(w.X, w.csr, N_FILL, seed=21, avg_deg=12)
    degs = [0, 1, 2, 2] + [d for c in KEPT for d in (c, 2 * c)] + [HUB]
    n_special = len(degs)
    first = N + N_FILL
    span = first + n_special
    me = lambda i: first + i
    rs = np.random.RandomState(17)

    def mixed(d):        # d ids: query ids (>= N) for up to half of them, base ids for the rest
        nqi = min(d // 2, span - N)
        return np.concatenate([rs.choice(N, size=d - nqi, replace=False), N + rs.choice(span - N, size=nqi, replace=False)])

    def row(i, r):
        if i == 0:
            return [] if r == 0 else [me(0), 5, 17, N + 3]              # no neighbour at all in relation 0
        if i == 1:
            return [me(1)]                                              # its only neighbour is itself
        if i == 2:
            return [me(3), N + 1]                                       # query-query edges only
        if i == 3:
            return [me(2), N + 100]
        return mixed(degs[i])

    rows = [[row(i, r) for i in range(n_special)] for r in range(R)]
    Xf, full_csr = append_rows(Xg, csr_g, rs.randn(n_special, Xg.shape[1]), rows)
    Xb, base_csr, Xq, q_pairs = split(Xf, full_csr, N)
    query = QueryBatch(Xq, q_pairs, BaseShape(N, Xf.shape[1], R))
    train_pos = [v for v in w.train_pos if v < N]
    return dict(N=N, Xf=Xf, full_csr=full_csr, Xb=Xb, base_csr=base_csr, query=query, train_pos=train_pos, degs=degs, engines={})


def explicit_engines(p, thr):
    """(base, full, oracle of every query row, target (0, 1)) - built once per threshold and shared"""
    if thr not in p["engines"]:
        full = engine(p["Xf"], p["full_csr"], p["train_pos"], 64, [thr] * 3, seed=4)
        base = engine(p["Xb"], p["base_csr"], p["train_pos"], 64, [thr] * 3, seed=4)
        same_theta(base, full)
        p["engines"][thr] = (base, full, Oracle(full, p["N"], p["query"].nq))
    return p["engines"][thr]


def kept_count(deg, thr):
    k = int(np.ceil(deg * thr))
    return k if deg > k + 1 else deg


def test_explicit_query_has_every_kind_of_row(explicit):
    q, N, degs = explicit["query"], explicit["N"], explicit["degs"]
    s = N_FILL
    assert q.nq == N_FILL + len(degs) and q.max_degree == HUB
    deg = np.stack(q.deg_host)                                          # [R, nq]
    row = lambda r, j: q.csr[r][1][q.csr[r][0][j]:q.csr[r][0][j + 1]]
    assert deg[0, s] == 0 and deg[1, s] > 0 and deg[2, s] > 0           # no neighbour at all in one relation
    assert all(row(r, s + 1).tolist() == [N + s + 1] for r in range(3))  # its only neighbour is itself
    assert all(row(r, j).min() >= N for r in range(3) for j in (s + 2, s + 3))   # query-query edges only
    for r in range(3):
        assert deg[r, s + 4:].tolist() == degs[4:]
        for j in range(s + 4, q.nq):                                    # every long row: base and query ids, in the row's
            ids = row(r, j)                                             # (ascending) order the query ids are its tail
            assert (ids < N).any() and (ids >= N).any()
            if len(ids) > 128:
                assert (ids[:128] < N).any() and (ids[128:] >= N).any()
    for thr in (0.5, 1.0):
        kept = {kept_count(d, thr) for d in degs}
        for want in KEPT:                                               # 16 / 17: four rows a wave | 63 .. 65: the wave tier |
            assert want in kept, (thr, want)                            # 128 / 129: gather chunks, the gather-dot's tail |
        assert max(kept) == kept_count(HUB, thr) > 2 * 2048             # 400: two tail slices | 2047 .. 2049: rank slices | the hub
    assert any(128 + 256 < k <= 128 + 2 * 256 for k in (kept_count(d, 0.5) for d in degs))
    assert HUB > 4096                                                   # beyond the select kernel's LDS keys: its long-row launch


@pytest.mark.parametrize("thr", [0.5, 1.0])
def test_identity_explicit_query(explicit, thr):
    base, full, oracle = explicit_engines(explicit, thr)
    q, N = explicit["query"], explicit["N"]
    at = assert_explained(base, oracle, q)
    # the ranked rows of the long rows mix base and query ids on both sides of the 128-entry boundary (0.5: distance order)
    h = np.asarray(at.chosen.host_offsets())
    ids = at.chosen.ids.cpu().numpy()
    seen = 0
    for j in range(N_FILL + 4, q.nq):
        lo, hi = int(h[j]), int(h[j + 1])                               # relation 0
        assert hi - lo == kept_count(explicit["degs"][j - N_FILL], thr)
        if thr == 0.5 and hi - lo > 256:
            head, tail = ids[lo:lo + 128], ids[lo + 128:hi]
            assert (head < N).any() and (head >= N).any() and (tail < N).any() and (tail >= N).any()
            seen += 1
    assert thr != 0.5 or seen >= 4
    # (the row with an empty relation was compared like every other: whatever its 0-entry aggregate gives, the same bits)
    assert bool(torch.isfinite(at.logits[N_FILL + 1:]).all())
    base.check()


# ---- 3. independence of position and chunking ---------------------------------------------------------------------------------
def test_subsets_chunks_and_groups(explicit):
    base, full, oracle = explicit_engines(explicit, 0.5)
    q = explicit["query"]
    rs = np.random.RandomState(6)
    special = np.arange(N_FILL, q.nq)
    ids = np.concatenate([rs.choice(q.nq, size=120, replace=False), special, special[:5], rs.choice(q.nq, size=20)])
    rs.shuffle(ids)
    assert len(np.unique(ids)) < len(ids)
    assert_explained(base, oracle, q, ids=ids, groups_alone=True)                   # chunk=None
    assert_explained(base, oracle, q, ids=ids, chunk=37)                            # 4 full chunks and a tail (172 = 4 * 37 + 24)
    assert len(ids) % 37 not in (0, len(ids))
    assert_explained(base, oracle, q, ids=torch.as_tensor(ids, dtype=torch.int32, device=dev()), chunk=len(ids) - 1)   # a tail of one row
    assert_explained(base, oracle, q, chunk=100, groups_alone=True)                 # every row, three full chunks and a tail
    # n = 0
    for empty in (np.zeros(0, np.int64), []):
        at = base.attribute_new(q, ids=empty, neighbours=True)
        assert at.logits.shape == (0, 2) and at.d_self.shape == (0, 32) and at.d_agg.shape == (3, 0, 32)
        assert at.self_contrib.shape == (0,) and at.rel_contrib.shape == (3, 0)
        assert at.chosen.n == 0 and at.chosen.ids.numel() == 0 and at.neigh_contrib.numel() == 0
        assert base.attribute_new(q, ids=empty).chosen is None
        ch = base.chosen_new(q, ids=empty)
        assert ch.n == 0 and ch.ids.numel() == 0 and ch.flat_offsets.tolist() == [0]
    with pytest.raises(ValueError, match="attribute_new: ids outside"):
        base.attribute_new(q, ids=[q.nq])
    with pytest.raises(ValueError, match="chosen_new: ids outside"):
        base.chosen_new(q, ids=[-1])
    for bad in ((1.0,), (float("nan"), 1.0), (0.0, float("inf")), None):
        with pytest.raises(ValueError, match="target"):
            base.attribute_new(q, ids=[0], target=bad)
    base.check()


def test_chunk_of_one_row():
    c, base, full, query = golden_pair("yelp_small", 17)
    oracle = Oracle(full, c.n, 17)
    assert_explained(base, oracle, query, chunk=1, groups_alone=True)
    assert_explained(base, oracle, query, ids=[16, 3, 3, 0], chunk=1)
    # a row that has no list entry at all (and so no entry behind any output pointer)
    from pcgnn_amd.graph import QueryBatch
    lone = QueryBatch(query.X_host[:1], [(np.zeros(2, np.int64), np.zeros(0, np.int64))] * c.R, base.g)
    at = base.attribute_new(lone, neighbours=True)
    assert at.chosen.ids.numel() == 0 and at.neigh_contrib.numel() == 0 and at.logits.shape == (1, 2)
    assert base.chosen_new(lone).flat_offsets.tolist() == [0] * (c.R + 1)
    base.check()


# ---- 4. the base-score cache -----------------------------------------------------------------------------------------------------
def test_score_cache():
    w, mk, mkq = mini()
    a = mk()
    fz = a.fused
    q = mkq(a)
    first = fz.attribute_new(q, neighbours=True)                        # a cold call: the table pass
    assert fz._new_scored_base
    logits = fz.infer_new(q)
    assert not fz._new_scored_base
    same(first.logits, logits, "logits against infer_new")
    for call in (lambda: fz.attribute_new(q, neighbours=True), lambda: fz.chosen_new(q)):      # a call after infer_new is warm
        got = call()
        assert not fz._new_scored_base
        same_chosen(got.chosen if hasattr(got, "chosen") else got, dict(offsets=first.chosen.flat_offsets, ids=first.chosen.ids,
                                                                     dist=first.chosen.dist), "warm call")
    forced = fz.attribute_new(q, neighbours=True, reuse_scores=False)
    assert fz._new_scored_base
    same(forced.neigh_contrib, first.neigh_contrib, "forced table pass")
    fz.chosen_new(q, reuse_scores=False)
    assert fz._new_scored_base
    # training steps: the cached scores must be discarded, and the results are a fresh engine's with the same parameters
    ids = torch.as_tensor(w.idx_train[:256], dtype=torch.int32, device=dev())
    lab = torch.as_tensor(w.labels[w.idx_train[:256]], dtype=torch.int32, device=dev())
    fz.train_step(ids, lab)
    fz.train_step(ids, lab, defer=True)                                 # (its update is applied by the call's flush)
    after = fz.attribute_new(q, neighbours=True)
    assert fz._new_scored_base
    assert not torch.equal(bits(after.logits), bits(first.logits))
    b = mk()
    same_theta(b.fused, fz)
    want = b.fused.attribute_new(mkq(b), neighbours=True)
    assert b.fused._new_scored_base
    same_attr(after, dict(offsets=want.chosen.flat_offsets, ids=want.chosen.ids, dist=want.chosen.dist,
                          neigh_contrib=want.neigh_contrib, **{k: getattr(want, k) for k in ATTR_KEYS}), "after training")
    fz.chosen_new(q)
    assert not fz._new_scored_base
    fz.train_step(ids, lab)
    fz.chosen_new(q)
    assert fz._new_scored_base
    fz.check()


# ---- 5. the training engine is left alone ----------------------------------------------------------------------------------------
def test_training_engine_untouched():
    """a group, attribute_new / chosen_new, two more groups == a group, flush, two more groups - bit for bit; no re-capture, no
    re-allocation"""
    w, mk, mkq = mini()
    a, b = mk(), mk()
    b.fused.theta.copy_(a.fused.theta)
    b.fused.params_changed()
    for t in (a, b):
        t.run_epoch_one_graph(n_epochs=2)
    maxB, graphs, fresh = a.fused.maxB, dict(a.fused._ep_graphs), a.fused._fresh
    s0 = a.fused.s0.clone()
    q = mkq(a)
    a.fused.attribute_new(q, chunk=130, neighbours=True)
    a.fused.chosen_new(q)
    b.fused.flush()
    torch.cuda.synchronize()
    assert a.fused._fresh == fresh and torch.equal(a.fused.s0, s0)
    for t in (a, b):
        t.run_epoch_one_graph(n_epochs=2)
    a.fused.attribute_new(q)
    assert a.fused._new_scored_base                           # (the epochs wrote theta)
    b.fused.flush()
    for t in (a, b):
        t.run_epoch_one_graph(n_epochs=2)
    torch.cuda.synchronize()
    for name in ("theta", "m", "v", "step_counter", "clf_next"):
        assert torch.equal(getattr(a.fused, name), getattr(b.fused, name)), name
    assert a.fused.maxB == maxB
    assert set(a.fused._ep_graphs) == set(graphs) and len(b.fused._ep_graphs) == len(graphs)
    assert all(a.fused._ep_graphs[k] is gr for k, gr in graphs.items())


# ---- 6. status handling -------------------------------------------------------------------------------------------------------------
def raw_call(fz, q, ids_dev, out, cap, chunk):
    """pcg_explain_new with the caller's own output struct (the engine's warm score buffer, a workspace of the call's own)"""
    from pcgnn_amd import _lib
    lib, g, n = fz.lib, fz.g, ids_dev.numel()
    nbytes = lib.pcg_explain_new_workspace_bytes(g.desc_ref(), q.desc_ref(), fz.E, chunk, cap)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.pcg_explain_new(g.desc_ref(), q.desc_ref(), p(fz.theta), fz.E, p(ids_dev), n, chunk, p(fz._inf["new_s0"]), 0, fz._thr,
                             p(ws), cap, 0.0, 1.0, C.byref(out), p(status), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.PCG_OK
    return int(status.item())


def test_overflow_is_reported_and_nothing_leaves_the_buffers():
    from pcgnn_amd import PcgnnLibraryError, _lib
    from pcgnn_amd.fused import infer_row_caps
    w, mk, mkq = mini()
    a = mk()
    fz = a.fused
    q = mkq(a)
    want = fz.attribute_new(q, neighbours=True)
    with pytest.raises(PcgnnLibraryError, match="selection list overflow"):
        fz.attribute_new(q, neighbours=True, _list_capacity=50)
    with pytest.raises(PcgnnLibraryError, match="selection list overflow"):
        fz.chosen_new(q, _list_capacity=50)
    again = fz.attribute_new(q, neighbours=True)                        # the next call works
    same(again.neigh_contrib, want.neigh_contrib, "after an overflow")
    same(again.chosen.ids, want.chosen.ids, "after an overflow")
    same(fz.infer_new(q), want.logits, "infer_new after an overflow")
    # guard words around out_ids and neigh_contrib: an exact capacity, then one that overflows
    n, R, F = q.nq, 3, 32
    ids_dev = torch.arange(n, dtype=torch.int32, device=dev())
    total = want.chosen.ids.numel()
    need = int(infer_row_caps(q.deg_host, fz.thresholds).sum())
    GUARD, FILL = 64, -7
    f32 = dict(dtype=torch.float32, device=dev())
    for cap, overflow in ((need, False), (50, True)):
        ids_buf = torch.full((total + 2 * GUARD,), FILL, dtype=torch.int32, device=dev())
        nc_buf = torch.full((total + 2 * GUARD,), float(FILL), **f32)
        dist = torch.empty(total, **f32)
        keep = [torch.empty(n, 2, **f32), torch.empty(n, F, **f32), torch.empty(R, n, F, **f32), torch.empty(n, **f32),
                torch.empty(R, n, **f32)]
        out = _lib.ExplainOut(*[t.data_ptr() for t in keep], want.chosen.flat_offsets.data_ptr(), ids_buf[GUARD:].data_ptr(),
                              dist.data_ptr(), nc_buf[GUARD:].data_ptr())
        st = raw_call(fz, q, ids_dev, out, cap, n)
        for buf in (ids_buf, nc_buf):
            assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + total:] == FILL).all())
        if overflow:
            assert st & _lib.PCG_ST_SEL_OVERFLOW
            assert bool((ids_buf == FILL).all()), "a chunk that selected nothing ranks nothing"
        else:
            assert st == 0
            same(ids_buf[GUARD:GUARD + total], want.chosen.ids, "raw call: ids")
            same(nc_buf[GUARD:GUARD + total], want.neigh_contrib, "raw call: neigh_contrib")
            same(keep[0], want.logits, "raw call: logits")
    same(fz.chosen_new(q).dist, want.chosen.dist, "after the raw calls")
    fz.check()


# ---- 7. the paths for resident nodes have not moved ---------------------------------------------------------------------------------
def test_resident_paths_unchanged(explicit):
    """ops.choose_ranked, engine.chosen and ops.neighbour_contrib on the FULL (resident) graph, before and after query calls on
    the base engine: the same bits; ids and distances are tests/ranked_ref.py's, the flat gather-dot float64's within the bound
    tests/test_gpu_attribute.py holds it to (``grad_check.Tally``: the one-table instantiations)"""
    from pcgnn_amd import ops
    from tests.grad_check import Tally
    from tests.ranked_ref import ranked_ref
    base, full, oracle = explicit_engines(explicit, 0.5)
    N, q = explicit["N"], explicit["query"]
    nodes = np.concatenate([np.arange(N + N_FILL, N + q.nq), np.random.RandomState(8).randint(0, N, size=100)])
    d = torch.randn(3, len(nodes), 32, generator=torch.Generator().manual_seed(3))

    def run():
        ch = full.chosen(nodes)
        s0 = full._inf["s0"][:full.g.n_nodes].clone()
        cr = ops.choose_ranked(full.g, nodes, s0, full.thresholds)
        return ch, cr, ops.neighbour_contrib(full.g, ch, d.to(dev())), s0

    ch0, cr0, nc0, s0 = run()
    base.attribute_new(q, neighbours=True)
    base.chosen_new(q, chunk=50)
    ch1, cr1, nc1, s1 = run()
    same(s0, s1, "scores")
    for a, b, what in ((ch0, ch1, "chosen"), (cr0, cr1, "choose_ranked"), (ch0, cr0, "chosen against choose_ranked")):
        same(a.flat_offsets, b.flat_offsets, f"{what}: offsets")
        same(a.ids, b.ids, f"{what}: ids")
        same(a.dist, b.dist, f"{what}: dist")
    same(nc0, nc1, "neighbour_contrib")
    off, ids, dist = ranked_ref(explicit["full_csr"], nodes, s0.cpu().numpy(), full.thresholds)
    assert np.array_equal(ch0.offsets.cpu().numpy(), off)
    assert np.array_equal(ch0.ids.cpu().numpy(), ids)
    assert np.array_equal(ch0.dist.cpu().numpy().view(np.uint32), dist.view(np.uint32))
    # the flat kernel against float64 dot products, float32 torch as the yardstick (test_gpu_attribute's oracle and bound)
    h = torch.from_numpy(np.asarray(ch0.host_offsets()))
    cols_all = ch0.ids.cpu().long()
    X = torch.from_numpy(explicit["Xf"])
    ref = {}
    for t in (torch.float64, torch.float32):
        parts = []
        for r in range(3):
            o = h[r * len(nodes):(r + 1) * len(nodes) + 1]
            cnt = o[1:] - o[:-1]
            rows = torch.repeat_interleave(torch.arange(len(nodes)), cnt)
            cols = cols_all[int(o[0]):int(o[-1])]
            parts.append((X.to(t)[cols] * d.to(t)[r][rows]).sum(1) / cnt.to(t)[rows])
        ref[t] = torch.cat(parts)
    tally = Tally("resident neighbour_contrib")
    tally.check("random d_agg", nc0, ref[torch.float64], ref[torch.float32])
    tally.done()


# ---- 8. utils.explain_new ----------------------------------------------------------------------------------------------------------
def test_explain_new_helper(explicit):
    from pcgnn_amd import utils as U
    from pcgnn_amd.graph import Attribution, ChosenLists
    base, full, oracle = explicit_engines(explicit, 0.5)
    q = explicit["query"]
    ids = np.array([5, q.nq - 1, 5, N_FILL, N_FILL + 9])
    two = U.explain_new(base, q, ids)
    assert len(two) == 2 and isinstance(two[0], ChosenLists)
    three = U.explain_new(base, q, ids, attribute=True)
    assert len(three) == 3 and isinstance(three[2], Attribution) and three[2].chosen is three[0]
    want = oracle.rows(ids)
    same_chosen(two[0], want, "explain_new")
    same_attr(three[2], want, "explain_new(attribute=True)")
    prob = torch.sigmoid(base.infer_new(q, ids=ids)).float()
    same(two[1], prob, "prob")
    same(three[1], prob, "prob (attribute=True)")
    allq = U.explain_new(base, q)
    same_chosen(allq[0], oracle.rows(None), "explain_new, every row")
    same(allq[1], torch.sigmoid(base.infer_new(q)).float(), "prob, every row")
