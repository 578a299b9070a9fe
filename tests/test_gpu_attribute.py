"""FusedPCGNN.attribute / ops.neighbour_contrib (pcg_attr_set, pcg_attr_neighbours) on the GPU.  Run with ``pytest -m gpu``.

The reference is tests/attr_ref.py in float64 with the device's own selection as input (``engine.chosen(ids)``; the selection
itself is pinned by tests/test_gpu_chosen.py).  Bound, not fitted to the kernels: per case and tensor e = max|x - x64| /
max|x64| over the rows kept; e_kernel <= 8 * e_f32 + 2^-20 (``dense_ref.tolerance``), e_f32 the same reference code in float32
on the CPU - measured in the test.  ReLU kinks: a row any of whose R + 1 pre-activation rows has an entry within 16 x the
float32 rounding of zero is left out (CPU runs only; at most 2 % of a case's rows, asserted; tests/test_attr_ref_host.py checks
the same condition with the oracle's sets).  Every figure goes through ``grad_check.Tally`` before anything is asserted; the
worst RATIO lines of a run on an MI355X are in profiles/r15/attr_f64_ratios.txt.
"""
import numpy as np
import pytest
import torch

from tests import attr_ref as A
from tests.grad_check import Tally
from tests.util import build_model

pytestmark = pytest.mark.gpu

KEYS = ("d_self", "d_agg", "self_contrib", "rel_contrib")


def dev():
    return torch.device("cuda", 0)


def make_engine(c):
    import pcgnn_amd as P
    from pcgnn_amd.fused import FusedPCGNN
    m = build_model(P, c, c.rho, graph=P.DeviceGraph(c.X, c.csr, c.train_pos, dev()))
    return FusedPCGNN(m, c.lr, c.wd, betas=c.betas, max_batch=64)


_ENGINES = {}


def engine_of(key):
    """one case and engine per shape (key "long": the explicit long-row graph), shared by the tests of this module"""
    if key not in _ENGINES:
        c = A.LongRowCase() if key == "long" else A.GradCase.of(key)
        _ENGINES[key] = (c, make_engine(c))
    return _ENGINES[key]


def index_of(ch):
    """a ChosenLists -> per relation (rows, cols, counts), entries in the device's order"""
    h = torch.from_numpy(np.asarray(ch.host_offsets()))
    ids = ch.ids.cpu().long()
    out = []
    for r in range(ch.R):
        off = h[r * ch.n:(r + 1) * ch.n + 1]
        cnt = off[1:] - off[:-1]
        out.append((torch.repeat_interleave(torch.arange(ch.n), cnt), ids[int(off[0]):int(off[-1])], cnt.double()))
    return out


def subset(res, keep):
    """the tensors of an Attribution or a reference dict on the rows kept"""
    get = (lambda k: res[k]) if isinstance(res, dict) else (lambda k: getattr(res, k).detach().cpu())
    return {"d_self": get("d_self")[keep], "d_agg": get("d_agg")[:, keep], "self_contrib": get("self_contrib")[keep],
            "rel_contrib": get("rel_contrib")[:, keep]}


def references(c, fz, ids, target):
    ch = fz.chosen(ids)
    index = index_of(ch)
    r64 = A.attr_ref(c.X, ids, index, c.params(), target, torch.float64)
    r32 = A.attr_ref(c.X, ids, index, c.params(), target, torch.float32)
    keep, share = A.kept_rows(r64["pre"], r32["pre"])
    return ch, index, r64, r32, keep, share


def check_against_float64(tally, what, res, r64, r32, keep, share, target):
    """checks 2 and 3: the four tensors on the rows kept, and completeness on every row"""
    print(f"{tally.tag} {what}: {int((~keep).sum())}/{keep.numel()} rows left out (cap {A.ROW_CAP:.0%})")
    assert share <= A.ROW_CAP, f"{what}: {share:.2%} of the rows have an ambiguous pre-activation - change the seed"
    got, w64, w32 = subset(res, keep), subset(r64, keep), subset(r32, keep)
    for k in KEYS:
        tally.check(f"{what} {k}", got[k], w64[k], w32[k])
    dev_res = {"logits": res.logits, "self_contrib": res.self_contrib, "rel_contrib": res.rel_contrib}
    e_k, e_32 = A.residual(dev_res, target), A.residual(r32, target)
    tol = A.tolerance(e_32)
    print(f"{tally.tag} {what} completeness: residual {e_k:.3e}  residual_f32 {e_32:.3e}  bound {tol:.3e}" + ("" if e_k <= tol else "  MISS"))
    if not e_k <= tol:
        tally.misses.append((f"{what} completeness", e_k, e_32, tol))
    own = float(res.completeness_residual().abs().max()) / float(res.target_logit().abs().max())
    assert abs(own - e_k) <= 1e-6 + 0.5 * e_k, "completeness_residual() is the same quantity in float32"


def same_bits(a, b, what):
    for k in ("logits",) + KEYS:
        assert torch.equal(getattr(a, k), getattr(b, k)), f"{what}: {k} differs"


@pytest.mark.parametrize("shape", list(A.SHAPES))
def test_batches_against_float64(shape):
    """n = 1, 15, 16, 17, 65 with duplicates, both targets: logits == infer, the float64 checks, a permuted list gives the
    same bits per node"""
    c, fz = engine_of(shape)
    tally = Tally(f"{shape} attribute batches")
    for name, ids in A.id_sets(c).items():
        if name == "whole":
            continue
        for target in A.TARGETS:
            res = fz.attribute(ids, target=target)
            assert torch.equal(res.logits, fz.infer(ids)), f"{name}: logits are not infer's"
            assert res.d_self.shape == (len(ids), c.f) and res.d_agg.shape == (c.R, len(ids), c.f)
            assert res.self_contrib.shape == (len(ids),) and res.rel_contrib.shape == (c.R, len(ids)) and res.target == target
            _, _, r64, r32, keep, share = references(c, fz, ids, target)
            check_against_float64(tally, f"{name} target {target}", res, r64, r32, keep, share, target)
            assert torch.allclose(res.feature_contrib().sum(1), res.self_contrib, rtol=1e-4, atol=1e-4), "feature_contrib's rows sum to self_contrib"
    ids = A.id_sets(c)["n65"]
    assert len(np.unique(ids)) < len(ids), "the batch has duplicates"
    res = fz.attribute(ids)
    perm = np.random.RandomState(5).permutation(len(ids))
    got = fz.attribute(torch.from_numpy(ids[perm]).to(dev()))
    inv = torch.from_numpy(np.argsort(perm)).to(dev())
    for k in ("logits", "d_self", "self_contrib"):
        assert torch.equal(getattr(got, k)[inv], getattr(res, k)), f"permuted ids: {k}"
    for k in ("d_agg", "rel_contrib"):
        assert torch.equal(getattr(got, k)[:, inv], getattr(res, k)), f"permuted ids: {k}"
    first = {int(v): i for i, v in reversed(list(enumerate(ids)))}
    for i, v in enumerate(ids):                                   # a node drawn twice: the same bits in both places
        assert torch.equal(res.d_self[i], res.d_self[first[int(v)]]) and torch.equal(res.d_agg[:, i], res.d_agg[:, first[int(v)]])
    tally.done()


@pytest.mark.parametrize("shape", list(A.SHAPES))
def test_whole_graph_chunks_against_float64(shape):
    """every node, chunk None / 1000 (two full chunks) / 999 (two full chunks and a 2-row tail): the float64 checks for each,
    and the same bits whatever the chunk"""
    c, fz = engine_of(shape)
    tally = Tally(f"{shape} attribute whole graph")
    ids = np.arange(c.n)
    for target in A.TARGETS:
        _, _, r64, r32, keep, share = references(c, fz, ids, target)
        base = None
        for chunk in (None, 1000, 999):
            res = fz.attribute(None, chunk=chunk, target=target)
            assert torch.equal(res.logits, fz.infer(None, chunk=chunk)), f"chunk {chunk}: logits are not infer's"
            check_against_float64(tally, f"chunk {chunk} target {target}", res, r64, r32, keep, share, target)
            if base is None:
                base = res
            else:
                same_bits(res, base, f"chunk {chunk}")
    tally.done()


def test_long_rows_against_float64():
    """kept counts 128 / 129 / 150 / 500: one gather chunk, two, several (the dense kernel sums the partial sums while it
    stages) and the sliced rows of the neighbour kernel; twenty ordinary rows beside them, n % 16 != 0"""
    c, fz = engine_of("long")
    ids = c.long_ids()
    tally = Tally("long rows attribute")
    for target in A.TARGETS:
        res = fz.attribute(ids, target=target, neighbours=True)
        assert torch.equal(res.logits, fz.infer(ids))
        ch, index, r64, r32, keep, share = references(c, fz, ids, target)
        off = ch.host_offsets()
        for r in range(3):
            assert [int(off[r * len(ids) + i + 1] - off[r * len(ids) + i]) for i in range(4)] == A.LONG_KEPT
        check_against_float64(tally, f"target {target}", res, r64, r32, keep, share, target)
        check_neighbours(tally, f"target {target}", res, index, r64, r32, keep)
    tally.done()


def row_sums(neigh, index, n):
    """[R, n]: the sums of every row's entries (float64)"""
    out, start = [], 0
    for rows, _, _ in index:
        out.append(torch.zeros(n, dtype=torch.float64).index_add_(0, rows, neigh[start:start + rows.numel()].double()))
        start += rows.numel()
    return torch.stack(out)


def check_neighbours(tally, what, res, index, r64, r32, keep):
    """the neighbour part of an Attribution: aligned with chosen.ids, every entry and every row's sum against float64"""
    n = keep.numel()
    assert torch.equal(res.chosen.ids.cpu().long(), torch.cat([cols for _, cols, _ in index]))
    assert res.neigh_contrib.shape == res.chosen.ids.shape and res.neigh_contrib.dtype == torch.float32
    ekeep = torch.cat([keep[rows] for rows, _, _ in index])
    got = res.neigh_contrib.cpu()
    tally.check(f"{what} neigh_contrib", got[ekeep], r64["neigh_contrib"][ekeep], r32["neigh_contrib"][ekeep])
    tally.check(f"{what} neigh row sums", row_sums(got, index, n)[:, keep], r64["rel_contrib"][:, keep],
                row_sums(r32["neigh_contrib"], index, n)[:, keep])


def test_neighbour_contrib_alone_and_aligned():
    """ops.neighbour_contrib on a random d_agg (short rows and sliced ones), float64 dot products as the reference and float32
    torch as the yardstick; through attribute: top_neighbours is the row of chosen.ids ordered by |contribution|"""
    from pcgnn_amd import ops
    tally = Tally("neighbour_contrib")
    for key, pick in (("long", lambda c: c.long_ids()), ((25, 64, 3), lambda c: c.batch(65)[0]), ((10, 16, 1), lambda c: np.arange(c.n))):
        c, fz = engine_of(key)
        ids = pick(c)
        ch = fz.chosen(ids)
        index = index_of(ch)
        d = torch.randn(c.R, len(ids), c.f, generator=torch.Generator().manual_seed(3))
        got = ops.neighbour_contrib(fz.g, ch, d.to(dev()))
        X = torch.from_numpy(c.X)
        ref = {t: torch.cat([(X.to(t)[cols] * d.to(t)[r][rows]).sum(1) / cnt.to(t)[rows] for r, (rows, cols, cnt) in enumerate(index)])
               for t in (torch.float64, torch.float32)}
        tally.check(f"{key} random d_agg", got, ref[torch.float64], ref[torch.float32])
    c, fz = engine_of("long")
    ids = c.long_ids()
    res = fz.attribute(ids, neighbours=True)
    for r, i in ((0, 3), (2, 1), (1, 10)):
        row_ids, _ = res.chosen.row(r, i)
        lo = int(res.chosen.host_offsets()[r * len(ids) + i])
        vals = res.neigh_contrib[lo:lo + row_ids.numel()]
        top_ids, top_vals = res.top_neighbours(r, i, 5)
        order = torch.argsort(vals.abs(), descending=True, stable=True)[:5]
        assert torch.equal(top_ids, row_ids[order]) and torch.equal(top_vals, vals[order])
        assert (top_vals.abs()[:-1] >= top_vals.abs()[1:]).all()
        all_ids, all_vals = res.top_neighbours(r, i)
        assert sorted(all_ids.tolist()) == sorted(row_ids.tolist()) and all_vals.numel() == row_ids.numel()
    tally.done()


def test_isolated_node_disturbs_no_other_row():
    """a centre with an empty relation (a 0 / 0 aggregate) among fifteen ordinary rows of one tile: its logits are NaN exactly
    where infer's are - the very bits -, every other row is bit for bit what it is without it"""
    c, fz = engine_of("long")
    ids = c.tile_with_isolated()
    at = int(np.nonzero(ids == A.ISOLATED)[0][0])
    assert len(ids) == 16
    res = fz.attribute(ids, neighbours=True)
    logits = fz.infer(ids)
    assert torch.equal(res.logits.isnan(), logits.isnan())
    assert torch.equal(res.logits.view(torch.int32), logits.view(torch.int32))
    assert res.chosen.row(1, at)[0].numel() == 0
    others = np.delete(np.arange(16), at)
    alone = fz.attribute(np.delete(ids, at))
    sel = torch.from_numpy(others).to(dev())
    for k in ("logits", "d_self", "self_contrib"):
        assert torch.equal(getattr(res, k)[sel], getattr(alone, k)), k
    for k in ("d_agg", "rel_contrib"):
        assert torch.equal(getattr(res, k)[:, sel], getattr(alone, k)), k
    assert bool(alone.logits.isfinite().all())


def test_edge_cases():
    c, fz = engine_of((10, 16, 1))
    for nb in (False, True):
        res = fz.attribute(torch.zeros(0, dtype=torch.int32, device=dev()), neighbours=nb)
        assert res.logits.shape == (0, 2) and res.d_self.shape == (0, c.f) and res.d_agg.shape == (c.R, 0, c.f)
        assert res.self_contrib.shape == (0,) and res.rel_contrib.shape == (c.R, 0)
        assert (res.neigh_contrib.numel() == 0 and res.chosen.n == 0) if nb else res.chosen is None
    with pytest.raises(ValueError, match="attribute: ids outside"):
        fz.attribute([0, c.n])
    with pytest.raises(ValueError, match="attribute: ids outside"):
        fz.attribute(np.array([-1]))
    for bad in ((1.0,), (1.0, 2.0, 3.0), (float("nan"), 1.0), (0.0, float("inf")), "ab", None, 1.0):
        with pytest.raises(ValueError, match="target"):
            fz.attribute([0], target=bad)
    with pytest.raises(ValueError, match="no neighbour part"):
        fz.attribute([0]).top_neighbours(0, 0, 1)


def test_corrupted_offsets_are_reported_and_nothing_leaves_the_buffer():
    """one decreasing entry in the offsets handed to ops.neighbour_contrib: the bit is set, guard words on both sides of the
    output stay intact, the rows the entry does not bound are written as without it; an entry below zero: both rows it bounds
    keep their fill"""
    from pcgnn_amd import _lib, ops
    from pcgnn_amd.fused import FusedPCGNN
    from pcgnn_amd.graph import ChosenLists
    c, fz = engine_of("long")
    ids = c.long_ids()
    ch = fz.chosen(ids)
    n, R = len(ids), 3
    d = torch.randn(R, n, c.f, generator=torch.Generator().manual_seed(4)).to(dev())
    good = ops.neighbour_contrib(fz.g, ch, d)
    off = np.asarray(ch.host_offsets()).copy()
    total, GUARD, FILL = int(off[-1]), 64, -7.0
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    k = n + 2                                                    # (the offset between rows (1, 1) and (1, 2): 129 kept | 150 kept)
    assert off[k - 1] >= 1
    for value, untouched in ((-5, (k - 1, k)), (int(off[k - 1]) - 1, ())):
        bad = off.copy()
        bad[k] = value
        assert bad[k] < bad[k - 1]
        buf = torch.full((total + 2 * GUARD,), FILL, dtype=torch.float32, device=dev())
        lists = ChosenLists(torch.from_numpy(bad).to(dev()), ch.ids, ch.dist, R, n)
        ops.neighbour_contrib(fz.g, lists, d, status=status, out=buf[GUARD:GUARD + total])
        st = int(status.item())
        status.zero_()
        assert st == _lib.PCG_ST_RANK_MISMATCH
        with pytest.raises(_lib.PcgnnLibraryError, match="neighbour_contrib"):
            FusedPCGNN._raise_status(st)
        assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + total:] == FILL).all())
        out = buf[GUARD:GUARD + total]
        for row in range(R * n):
            lo, hi = int(off[row]), int(off[row + 1])
            if row in untouched:
                assert bool((out[lo:hi] == FILL).all()), row
            elif row < k - 2 or row > k:
                assert torch.equal(out[lo:hi], good[lo:hi]), row


def test_training_engine_untouched():
    """a group, attribute(None, neighbours=True), two more groups == a group, flush, two more groups - bit for bit"""
    from pcgnn_amd import synth
    from pcgnn_amd.handler import PCGNNTrainer
    w = synth.make_workload("mini", 6000, 32, (4000, 30000, 90000), 0.12, seed=3)
    a, b = (PCGNNTrainer(w, dict(engine="graph", seed=5, batch_size=256), dev()) for _ in range(2))
    b.fused.theta.copy_(a.fused.theta)
    b.fused.params_changed()
    for t in (a, b):
        t.run_epoch_one_graph(n_epochs=2)
    maxB, graphs, fresh = a.fused.maxB, dict(a.fused._ep_graphs), a.fused._fresh
    s0 = a.fused.s0.clone()
    res = a.fused.attribute(None, chunk=2500, neighbours=True)
    b.fused.flush()
    torch.cuda.synchronize()
    assert res.logits.shape == (w.n, 2) and res.neigh_contrib.numel() == res.chosen.ids.numel()
    assert a.fused._fresh == fresh and torch.equal(a.fused.s0, s0)
    for t in (a, b):
        for _ in range(2):
            t.run_epoch_one_graph(n_epochs=2)
    torch.cuda.synchronize()
    for name in ("theta", "m", "v", "step_counter", "clf_next"):
        assert torch.equal(getattr(a.fused, name), getattr(b.fused, name)), name
    assert a.fused.maxB == maxB
    assert set(a.fused._ep_graphs) == set(graphs) and all(a.fused._ep_graphs[k] is gr for k, gr in graphs.items())


def test_explain_nodes_attribute():
    from pcgnn_amd import utils as U
    from pcgnn_amd.graph import Attribution, ChosenLists
    c, fz = engine_of((25, 64, 3))
    ids = c.batch(17)[0]
    two = U.explain_nodes(fz, ids)
    assert len(two) == 2 and isinstance(two[0], ChosenLists)
    three = U.explain_nodes(fz, ids, attribute=True)
    assert len(three) == 3 and isinstance(three[2], Attribution) and three[2].chosen is not None
    assert torch.equal(three[0].ids, two[0].ids) and torch.equal(three[1], two[1])
    assert torch.equal(torch.sigmoid(three[2].logits).float(), two[1])
    assert torch.equal(three[2].chosen.ids, two[0].ids)
