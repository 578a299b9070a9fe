"""Whole-set inference for the GraphSAGE / GCN baselines (pcg_baseline_infer, BaselineEngine) on an MI355X: against float64
(tests/baseline_ref.py) on a crafted graph that holds every row length at which the kernels change strategy, against the
reference's own outputs (the ``s1_*`` arrays of the golden fixtures), against the model's per-batch ``forward``, bit for bit across
node sets / chunks / order / calls, with live parameters, inside a guarded arena at exactly the documented sizes, and through
``utils``' evaluation routing.  Run with ``pytest -m gpu``."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import baseline_ref as BR
from tests.grad_check import Tally
from tests.guarded import GuardedArena
from tests.baseline_ref import FEAT_TOL, GCN_ENC_TOL
from tests.util import GoldenCase, synth_graph

pytestmark = pytest.mark.gpu

N = 6000
# CSR degrees of the crafted rows; every degree >= 2 twice: the node inside its own row, and not
SINGLES = ((0, False), (1, True), (1, False))
DEGREES = (2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1025, 2049, 5000)
SHAPES_ALL = sorted(BR.SHAPES)
FE_ALL = ((25, 64), (32, 128))                               # every model shape
# the concat-SAGE and GCN shapes.  (509, 64) and (509, 128): W_enc does not fit in LDS beside the tile - the dense kernel streams
# it from L2 (BR.w_enc_in_lds); (300, 16): rows of 300 floats, 75 float4 chunks over 64 lanes - some lanes hold two, most one
FE_TWO = ((32, 64), (100, 64), (509, 16), (1, 16), (509, 64), (509, 128), (300, 16))
STREAMED = ((509, 64), (509, 128))
CASES = [(F, E, s) for F, E in FE_ALL for s in SHAPES_ALL] + [(F, E, s) for F, E in FE_TWO for s in ("sage_concat", "gcn")]


def dev():
    return torch.device("cuda", 0)


def crafted_csr():
    """one relation over N nodes: node 0 (degree 2, itself not in the row: every neighbour above it - the united centre comes
    first), node N - 1 (degree 2049, itself not in the row: every neighbour below it - it comes last), the other crafted rows at
    nodes 1 .., every remaining node a short row of 1 - 4 others, half of them with themselves"""
    rs = np.random.RandomState(11)
    spec = {0: (2, False), N - 1: (2049, False)}
    todo = [(d, s) for d, s in SINGLES] + [(d, s) for d in DEGREES for s in (True, False)]
    todo.remove((2, False))
    todo.remove((2049, False))
    for v, ds in enumerate(todo, start=1):
        spec[v] = ds
    rows = []
    for v in range(N):
        if v in spec:
            d, with_self = spec[v]
        else:
            d, with_self = int(rs.randint(1, 5)) + (v % 2), bool(v % 2)
        others = np.delete(np.arange(N), v)
        pick = rs.choice(others, size=d - 1 if with_self else d, replace=False) if d - (1 if with_self else 0) > 0 else np.zeros(0, np.int64)
        row = np.sort(np.concatenate([pick, [v]] if with_self else [pick])).astype(np.int32)
        assert len(row) == d and len(np.unique(row)) == d and (v in row) == with_self
        rows.append(row)
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=indptr[1:])
    deg = np.diff(indptr)
    assert deg[0] == 2 and rows[0].min() > 0 and deg[N - 1] == 2049 and rows[N - 1].max() < N - 1
    for d in (0, 1) + DEGREES:
        assert (deg == d).sum() >= (1 if d == 0 else 2), d
    return indptr, np.concatenate(rows), spec


_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def csr():
    return memo("csr", crafted_csr)[:2]


def hoods(add_self):
    return memo(("hoods", add_self), lambda: BR.neighbourhoods(csr(), np.arange(N), add_self))


def features(F):
    # randn around 1: sums over a row do not cancel to zero
    return memo(("X", F), lambda: (np.random.RandomState(100 + F).randn(N, F) * 0.5 + 1.0).astype(np.float32))


def graph(F):
    import pcgnn_amd as P
    return memo(("g", F), lambda: P.DeviceGraph(features(F), [csr()], [], dev()))


def model_of(F, E, shape):
    from pcgnn_amd import graphsage as GS
    return memo(("model", F, E, shape), lambda: BR.build_model(GS, graph(F), F, E, shape, seed=F * 1000 + E))


def weights(model):
    return model.enc.weight.detach().cpu().numpy(), model.weight.detach().cpu().numpy()


def reference(F, E, shape, dtype):
    """(logits, h, a) over all N nodes, computed once per case and type"""
    def make():
        W_enc, W_cls = weights(model_of(F, E, shape))
        s = BR.SHAPES[shape]
        return BR.forward(features(F), csr(), np.arange(N), W_enc, W_cls, dtype=dtype, hoods=hoods(s["add_self"]), **s)
    return memo(("ref", F, E, shape, dtype), make)


def all_nodes(F, E, shape):
    """(logits, h, a) of ``embed`` over every node with the default chunk: the call the bit-for-bit tests compare against"""
    def make():
        h, logits, a = model_of(F, E, shape).embed(None, want_logits=True, aggregates=True)
        return logits, h, a
    return memo(("all", F, E, shape), make)


def tally_against_f64(tally, what, got, ref64, ref32):
    """NaN exactly where the reference has it (compared on its own), the rest by the project's rule"""
    got = got.detach().cpu().numpy()
    nan = np.isnan(ref64)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN in other places than the reference"
    assert np.array_equal(np.isnan(ref32), nan)
    keep = ~nan.any(axis=1)
    tally.check(what, torch.from_numpy(got[keep]), torch.from_numpy(ref64[keep]), torch.from_numpy(ref32[keep]))
    return int(nan.any(axis=1).sum())


def test_the_cases_cover_both_dense_variants():
    for F, E, shape in CASES:
        assert BR.w_enc_in_lds(F, E, BR.SHAPES[shape]["concat_self"]) == ((F, E) not in STREAMED), (F, E, shape)
    assert sum((F, E) in STREAMED for F, E, _ in CASES) == 4


# ---- 1. against float64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,E,shape", CASES)
def test_against_float64(F, E, shape):
    model = model_of(F, E, shape)
    assert model.engine().shape == dict(emb=E, **BR.SHAPES[shape])
    logits, h, a = all_nodes(F, E, shape)
    assert tuple(logits.shape) == (N, 2) and tuple(h.shape) == (N, E) and tuple(a.shape) == (N, F)
    r64, r32 = reference(F, E, shape, np.float64), reference(F, E, shape, np.float32)
    t = Tally(f"baseline F={F} E={E} {shape}")
    nan_rows = [tally_against_f64(t, what, got, w64, w32) for what, got, w64, w32 in
                (("logits", logits, r64[0], r32[0]), ("embed", h, r64[1], r32[1]), ("aggregates", a, r64[2], r32[2]))]
    # the degree-0 row is NaN without the union and the node's own row with it
    assert nan_rows == ([0, 0, 0] if BR.SHAPES[shape]["add_self"] else [1, 1, 1])
    t.done()


# ---- 2. against the reference's own outputs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BR.s1_cases())
def test_against_golden_fixtures(name):
    import pcgnn_amd as P
    from pcgnn_amd import graphsage as GS
    c = GoldenCase(name)
    z, sub = c.z, c.z["s1_nodes"]
    g = P.DeviceGraph(c.X, [c.homo_csr], [], dev())
    for shape, enc_key, agg_key, tol in (("sage", "s1_sage_enc", "s1_mean", FEAT_TOL), ("gcn", "s1_gcn_enc", "s1_gcn", GCN_ENC_TOL),
                                         ("sage_self", None, "s1_mean_gcn", None)):
        model = BR.build_model(GS, g, c.f, c.emb, shape)
        if enc_key is not None:
            with torch.no_grad():
                model.enc.weight.copy_(torch.from_numpy(z[enc_key + "_w"]))
        h, a = model.embed(sub, aggregates=True)
        if enc_key is not None:
            np.testing.assert_allclose(h.cpu().numpy(), z[enc_key].T, rtol=0, atol=tol, err_msg=enc_key)
        np.testing.assert_allclose(a.cpu().numpy(), z[agg_key], rtol=0, atol=FEAT_TOL, err_msg=agg_key)


# ---- 3. against the model's own per-batch forward ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES_ALL)
def test_against_per_batch_forward(shape):
    import pcgnn_amd as P
    from pcgnn_amd import graphsage as GS
    n, F, E = 1500, 25, 64
    X, _, csrs = memo("synth", lambda: synth_graph(3, n, F, [6], 0.1))
    g = memo("synth_g", lambda: P.DeviceGraph(X, csrs, [], dev()))
    model = BR.build_model(GS, g, F, E, shape, seed=5)
    W_enc, W_cls = weights(model)
    ids = np.arange(n)
    r64 = BR.forward(X, csrs[0], ids, W_enc, W_cls, dtype=np.float64, **BR.SHAPES[shape])[0]
    r32 = BR.forward(X, csrs[0], ids, W_enc, W_cls, dtype=np.float32, **BR.SHAPES[shape])[0]
    with torch.no_grad():
        batched = torch.cat([model.forward(ids[b:b + 64].tolist()) for b in range(0, n, 64)])
    t = Tally(f"baseline vs forward {shape}")
    t.check("infer", model.infer(), torch.from_numpy(r64), torch.from_numpy(r32))
    t.check("per-batch forward", batched, torch.from_numpy(r64), torch.from_numpy(r32))
    t.done()


# ---- 4. bit for bit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,E,shape", [(25, 64, "sage_concat"), (32, 128, "gcn"), (509, 16, "sage_concat"), (100, 64, "gcn"),
                                       (509, 64, "sage_concat"), (509, 64, "gcn"), (509, 128, "gcn"), (300, 16, "sage_concat")])
def test_bit_for_bit(F, E, shape):
    model = model_of(F, E, shape)
    whole = all_nodes(F, E, shape)[0]
    same = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))       # (NaN rows compare by their bits)
    assert same(model.infer(), whole)                                                # a second call
    h, lg = model.embed(None, want_logits=True)
    assert same(lg, whole) and same(h, all_nodes(F, E, shape)[1])
    rs = np.random.RandomState(F + E)
    crafted = np.arange(0, 44)
    for n in (1, 15, 16, 17, 33):
        ids = np.concatenate([rs.choice(crafted, size=min(n, 8), replace=False), rs.randint(0, N, size=n)])[:n]
        for form in (ids.tolist(), ids, torch.from_numpy(ids).to(dev())):
            assert same(model.infer(form), whole[torch.from_numpy(ids).long().to(dev())]), n
    for chunk in (16, 17, 1000, 4096):                                               # 1000 divides N; 4096 leaves a short tail
        assert same(model.infer(None, chunk=chunk), whole), chunk
    perm = np.concatenate([rs.permutation(N), crafted, [N - 1, 0, 0]])
    assert same(model.infer(perm, chunk=999), whole[torch.from_numpy(perm).long().to(dev())])
    assert model.infer([]).shape == (0, 2)


# ---- 5. live parameters ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["sage", "gcn"])
def test_live_parameters(shape):
    from pcgnn_amd import graphsage as GS
    from pcgnn_amd.baseline import BaselineEngine
    F, E = 25, 64
    model = BR.build_model(GS, graph(F), F, E, shape, seed=9)
    ids = np.arange(0, N, 7)
    before = model.infer(ids).clone()
    opt = torch.optim.Adam(model.parameters(), lr=0.05)
    model.loss(ids[:64].tolist(), np.arange(64) % 2).backward()
    opt.step()                                                                       # in place: the engine holds no copy
    after = model.infer(ids)
    fresh = BaselineEngine.from_model(model).infer(ids)
    assert torch.isfinite(after).all() and torch.isfinite(before).all()
    assert torch.equal(after, fresh) and not torch.equal(after, before)


# ---- 6. extents ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,E,shape", [(25, 64, "sage_concat"), (509, 16, "gcn"), (32, 128, "sage_concat"),
                                       (509, 64, "sage_concat"), (509, 128, "gcn"), (300, 16, "gcn")])
def test_extents(F, E, shape):
    from pcgnn_amd import _lib, ops
    model = model_of(F, E, shape)
    eng, lib = model.engine(), _lib.load()
    whole = all_nodes(F, E, shape)
    m, keep = eng._model_desc()
    chunk = 17
    ws_bytes = int(lib.pcg_baseline_workspace_bytes(eng.g.desc_ref(), C.byref(m), chunk))
    assert ws_bytes > 0
    rs = np.random.RandomState(3)
    for n in (1, 17, N):
        ids = np.arange(N) if n == N else np.concatenate([[41], rs.randint(0, N, size=n)])[:n]     # (node 41: a 5000-row)
        arena = GuardedArena(64 << 20, dev())
        ids_dev = arena.take((n,), torch.int32, name="ids")
        ids_dev.copy_(torch.from_numpy(ids.astype(np.int32)))
        ws = arena.take((ws_bytes,), torch.uint8, name="workspace")
        logits, emb, agg = arena.take((n, 2), name="logits"), arena.take((n, E), name="emb"), arena.take((n, F), name="agg")
        status = arena.take((1,), torch.int32, name="status")
        rc = lib.pcg_baseline_infer(eng.g.desc_ref(), C.byref(m), ops._p(ids_dev), n, chunk, ops._p(ws), ws_bytes, ops._p(logits),
                                    ops._p(emb), ops._p(agg), ops._p(status), ops._stream(dev()))
        assert rc == _lib.PCG_OK
        torch.cuda.synchronize()
        arena.check(f"pcg_baseline_infer n={n} chunk={chunk} F={F} E={E} {shape}")
        assert int(status.item()) == 0
        sel = torch.from_numpy(ids).long().to(dev())
        for got, want in zip((logits, emb, agg), whole):
            assert torch.equal(got.view(torch.int32), want[sel].view(torch.int32))
    del keep


# ---- 7. routing ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["sage", "gcn"])
def test_routing(shape):
    import pcgnn_amd as P
    from pcgnn_amd import graphsage as GS, utils as U
    from tests.eval_ref import counts_numpy
    n, F, E, B = 1500, 25, 64, 256
    X, labels, csrs = memo("synth", lambda: synth_graph(3, n, F, [6], 0.1))
    labels = memo("synth_labels", lambda: (np.random.RandomState(8).rand(n) < 0.2).astype(np.int64))
    g = memo("synth_g", lambda: P.DeviceGraph(X, csrs, [], dev()))
    model = BR.build_model(GS, g, F, E, shape, seed=6)
    ids = np.random.RandomState(4).permutation(n)[:1100]
    y = labels[ids]
    # the default: the per-batch loop, bit for bit
    assert model.eval_by_infer is False
    with torch.no_grad():
        loop = torch.cat([model.to_prob(ids[b:b + B].tolist(), y[b:b + B], train_flag=False)[0] for b in range(0, len(ids), B)])
    prob_loop = U.predict_proba(ids, model, B, y)
    assert np.array_equal(prob_loop.view(np.uint32), loop.float().cpu().numpy().view(np.uint32))
    per_batch = U.test(ids, y, model, B, print_line=False)
    model.eval_by_infer = True
    try:
        prob = U.predict_proba(ids, model, B, y)
        assert np.array_equal(prob.view(np.uint32), torch.sigmoid(model.infer(ids)).float().cpu().numpy().view(np.uint32))
        assert len(np.unique(prob[:, 1])) > 100 and 0.0 < U.roc_auc(y, prob[:, 1]) < 1.0, "degenerate scores"
        np.testing.assert_allclose(prob, prob_loop, rtol=0, atol=1e-5)
        host = U.test(ids, y, model, B, print_line=False, on_device=False)
        assert U.test(ids, y, model, B, print_line=False, on_device=True) == host and len(host) == 4
        np.testing.assert_allclose(host, per_batch, rtol=0, atol=0.02)
        assert model.evaluate(ids, y) == U.metrics_from_counts(counts_numpy(prob, y))
        ks = (1, 100, 1000, len(ids) + 5)
        assert model.evaluate_ranking(ids, y, ks=ks) == U.host_ranking(y, prob, ks)
        assert U.test_ranking(ids, y, model, B, ks=(100,), on_device=True, print_line=False) == \
            U.test_ranking(ids, y, model, B, ks=(100,), print_line=False)
        al = model.alerts(ids, k=64, labels=y)
        a_ids, a_pos, a_prob, a_hits = al.to_numpy()
        order = U.alert_order(prob[:, 1])[:64]
        assert np.array_equal(a_pos, order) and np.array_equal(a_ids, ids[order]) and np.array_equal(a_hits, np.cumsum(y[order]))
        assert np.array_equal(a_prob.view(np.uint32), prob[order, 1].view(np.uint32))
        with pytest.raises(ValueError):
            model.alerts(ids, k=8, query=object())
        for bad in ([0, n], [-1], np.array([5, n + 3])):
            with pytest.raises(ValueError):
                model.infer(bad)
        with pytest.raises(ValueError):
            U.predict_proba(np.array([1, n]), model, B)
    finally:
        model.eval_by_infer = False


def test_an_id_outside_the_graph_sets_the_status_bit():
    """the host checks ids before the call; past it, the device clamps the row and reports: the engine raises"""
    from pcgnn_amd import _lib
    model = model_of(25, 64, "sage")
    eng = model.engine()
    bad = torch.tensor([3, N + 5, 7], dtype=torch.int32, device=dev())
    logits = torch.empty(3, 2, device=dev())
    with pytest.raises(_lib.PcgnnLibraryError, match="outside the feature table"):
        eng._call(bad, 3, None, logits, None, None)
    assert int(eng._inf["status"].item()) == 0                                       # cleared for the next call
    assert torch.equal(logits[[0, 2]], all_nodes(25, 64, "sage")[0][[3, 7]])         # the others' rows are what they always are
