"""The dense kernel family at the shapes no other test launches (dense_ref.EDGE_SHAPES and the lists beside it): whole-set
inference / embeddings and attribution here; the training gradients in tests/test_gpu_grad_f64.py, the seeded backward in
tests/test_gpu_custom_loss.py.  Run with ``pytest -m gpu`` on an MI355X.  What each shape reaches, and which instantiation each
user of dense_tile_body picks for it, is asserted on the host (tests/test_edge_shapes_host.py).

Every tolerance is the project's rule, not fitted to the kernels: e_kernel <= 8 * e_f32 + 2^-20 relative to the tensor's largest
element, e_f32 the same reference in float32 on the CPU (``dense_ref.tolerance``, ``grad_check.Tally``), by the comparisons
tests/test_gpu_embed.py and tests/test_gpu_attribute.py already have, with the device's own chosen lists as the reference's
selection.  Every identity is ``torch.equal``.

1  no launch writes outside its buffers (tests/guarded.py) at the classes of shape nothing had run before: R = 7 and 8, E > 256,
   attribution on rows wider than 256 floats, the attribution's fourth LDS overlay.  The guarded engine runs first.
2  inference, n = 1, 17, 16 * CUs + 17: ``embed(relations=True, want_logits=True)`` against float64; ``infer`` == the
   ``predict`` loop; ``embed``'s logits == ``infer``.
3  attribution: the body of test_gpu_attribute.test_batches_against_float64 (both targets, completeness, logits == ``infer``, a
   permuted list).  (260, 16, 1) also with ``neighbours=True`` and the hub rows among the ids - lists of more than 128
   entries: the neighbour kernel's tail slices with two float4 chunks a lane - and ``ops.neighbour_contrib`` on a random d_agg.
   (361, 16, 1): ``attribute`` raises the library's error, ``infer`` of the same ids works.
4  ``attribute_new`` at stride 260, nq = 17: the bits of ``full.attribute`` on the graph rebuilt with the query rows appended
   (the neighbour kernel's two-table form with the second chunk).

Measured on an MI355X (profiles/r28/edge_shape_ratios.txt): `ratio` = e_kernel / e_f32 over the entries with e_f32 >= 2^-24,
`of bound` = e_kernel / (8 * e_f32 + 2^-20), maximised over the sets, targets and tensors; embed: max error / bound over h_1 ..
h_R, emb and the logits:

    shape (F, E, R)  embed / infer of bound | attribute ratio  of bound
    (16, 64, 4)      0.11                   | 2.52             0.15
    (30, 64, 3)      0.11                   | 2.34             0.16
    (20, 128, 1)     0.09                   | 1.88             0.32
    (20, 32, 7)      0.11                   | 2.39             0.13
    (17, 32, 8)      0.11                   | 2.42             0.19
    (32, 64, 8)      0.10                   | 4.25             0.18
    (64, 64, 3)      0.10                   | 2.38             0.13
    (16, 272, 1)     0.17                   | 3.02             0.20
    (100, 64, 3)     -                      | 3.50             0.19
    (260, 16, 1)     0.36                   | 2.01             0.14   (hub rows, neighbours, random d_agg: 2.01, 0.11)
    (360, 16, 1)     -                      | 3.10             0.23
    (24, 16, 1)      -                      | 1.99             0.11

Every identity held, no guard word was touched.  A first run missed one bound without a wrong kernel: the lone row of (16, 272, 1)
at the salt then in use, `rel_contrib` - one element, an inner product of condition 24 - at 2.08e-6 against 8 * 4.9e-8 + 2^-20 =
1.35e-6 (1.54 of the bound; d_self and d_agg of the same row at 0.11 and 0.15 of theirs, completeness at 0.03): the lone rows are
now drawn among the rows that keep attr_ref.COND_CAP.
"""
import numpy as np
import pytest
import torch

from tests import attr_ref as A
from tests import dense_ref as D
from tests import test_gpu_attribute as TA
from tests import test_gpu_embed as TE
from tests.grad_check import Tally
from tests.guarded import GuardedArena, guarded_allocations
from tests.util import PARAM_KEYS, build_model

pytestmark = pytest.mark.gpu

MIB = 1 << 20
IDS = lambda s: "x".join(map(str, s))
# (1): one shape of every class nothing had run - R = 7, R = 8 with and without the weights' LDS copy, E > 256, F > 256 in the
# attribution, the fourth overlay
GUARDED_SHAPES = [(20, 32, 7), (17, 32, 8), (32, 64, 8), (16, 272, 1), (360, 16, 1), (24, 16, 1)]
_ENGINES = {}


def dev():
    return torch.device("cuda", 0)


def new_engine(c, max_batch=256):
    import pcgnn_amd as P
    from pcgnn_amd.fused import FusedPCGNN
    m = build_model(P, c, c.rho, graph=P.DeviceGraph(c.X, c.csr, c.train_pos, dev()))
    return FusedPCGNN(m, c.lr, c.wd, betas=c.betas, max_batch=max_batch)


def engine_of(shape):
    """one case and engine per shape, shared by the tests of this module (none of them changes a parameter)"""
    if shape not in _ENGINES:
        c = D.GradCase.of(shape)
        _ENGINES[shape] = (c, new_engine(c))
    return _ENGINES[shape]


# ---- 1. extents ---------------------------------------------------------------------------------------------------------------------
def all_calls(fz, c, check, train):
    """every user of the dense tile body once, at 17 rows (a second tile with one row); check(what) after each call"""
    out = {}
    ids_np, lab_np = c.batch(17)
    ids = torch.from_numpy(ids_np.astype(np.int32)).to(dev())
    lab = torch.from_numpy(lab_np.astype(np.int32)).to(dev())
    if train:
        for via in ("acts", "slabs"):
            for k, v in fz.gradients(ids, lab, via=via).items():
                out[f"gradients {via}: {k}"] = v.clone()
            check(f"gradients(via={via!r})")
        named = dict(fz.model.named_parameters())
        gnn, center = fz.forward(ids, lab)
        (gnn.sum() + center.sum()).backward()
        check("forward + backward (pcg_dense_vjp, pcg_wgrad)")
        for k in PARAM_KEYS(c.R):
            out[f"backward: {k}"] = named[k].grad.clone()
            named[k].grad = None
        fz.train_step(ids, lab, defer=True)
        check("train_step(defer=True)")
        fz.flush()
        check("flush")
        out["theta"], out["m"], out["logits"] = fz.theta.clone(), fz.m.clone(), fz.logits[:17].clone()
    out["infer"] = fz.infer(ids_np)
    check("infer")
    out["embed"], out["embed h"], out["embed logits"] = fz.embed(ids_np, relations=True, want_logits=True)
    check("embed")
    at = fz.attribute(ids_np, neighbours=True)
    check("attribute(neighbours=True)")
    for k in ("logits",) + TA.KEYS + ("neigh_contrib",):
        out[f"attribute: {k}"] = getattr(at, k)
    torch.cuda.synchronize()
    fz.check()
    return out


@pytest.mark.parametrize("shape", GUARDED_SHAPES, ids=IDS)
def test_nothing_is_written_outside_the_buffers(shape):
    """an engine of max_batch 17 whose every buffer lies between guard words, then the same calls on a plain one: the same bits"""
    from tests.test_gpu_extents_train import arena_bytes
    c = D.GradCase.of(shape)
    train = shape in D.EDGE_SHAPES
    arena = GuardedArena(arena_bytes(c, 17) + 64 * MIB, dev())
    with guarded_allocations(arena):
        fz = new_engine(c, 17)
        arena.check("building the engine")
        got = all_calls(fz, c, arena.check, train)
    want = all_calls(new_engine(c, 17), c, lambda what: None, train)
    assert list(got) == list(want)
    for k in want:
        assert torch.equal(got[k], want[k]), f"{k}: the guarded engine's bits differ from the plain engine's"


# ---- 2. inference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", D.EDGE_INFER_SHAPES, ids=IDS)
def test_inference_against_float64_and_the_predict_loop(shape):
    c, fz = engine_of(shape)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    worst = 0.0
    for n, ids in D.edge_id_sets(c, cus).items():
        emb, h, lg = fz.embed(ids, relations=True, want_logits=True)
        assert emb.shape == (n, c.emb) and h.shape == (n, c.R, c.emb) and lg.shape == (n, 2)
        inf = fz.infer(ids)
        want_emb, want_logits = TE.predict_loop(fz, ids, 256 if n > 17 else (7 if n == 17 else n))
        assert torch.equal(inf, want_logits), f"n {n}: infer is not the predict loop"
        assert torch.equal(lg, inf), f"n {n}: embed's logits are not infer's"
        assert torch.equal(emb, want_emb), f"n {n}: embed is not the predict loop's combined rows"
        r64, r32 = TE.forward_refs(c, ids, TE.index_of(fz.chosen(ids)))
        b = TE.bounds(r64, r32)
        for t, got in enumerate([h[:, r, :] for r in range(c.R)] + [emb]):
            v64, p64, tol, amb = b[t]
            TE.check_activation(f"{shape} n={n} " + (f"h_{t + 1}" if t < c.R else "emb"), got, v64, p64, tol, amb)
            worst = max(worst, float((got.detach().cpu().double() - v64)[~amb].abs().max()) / tol)
        tol = D.tolerance(D.rel_err(r32["logits"], r64["logits"])) * float(r64["logits"].abs().max())
        mine = emb.cpu().double() @ c.params()["weight"].double().t()
        err, err64 = float((mine - lg.cpu().double()).abs().max()), float((lg.cpu().double() - r64["logits"]).abs().max())
        print(f"{shape} n={n} logits: |emb W_cls^T - logits| {err:.3e}  |logits - float64| {err64:.3e}  bound {tol:.3e}")
        assert err <= tol and err64 <= tol
        worst = max(worst, err / tol, err64 / tol)
    print(f"RATIO {shape} embed / infer: of bound {worst:.2f}")
    fz.check()


# ---- 3. attribution ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", D.EDGE_ATTR_SHAPES, ids=IDS)
def test_attribution_against_float64(shape):
    TA.test_batches_against_float64(shape)
    TA.engine_of(shape)[1].check()


def test_hub_rows_on_wide_rows_against_float64():
    """(260, 16, 1), the hub rows among the ids: the neighbour kernel's tail slices on rows of two float4 chunks a lane"""
    from pcgnn_amd import ops
    shape = (260, 16, 1)
    c, fz = TA.engine_of(shape)
    ids = A.hub_ids(c)
    tally = Tally(f"{shape} attribute, hub rows")
    for target in A.TARGETS:
        res = fz.attribute(ids, target=target, neighbours=True)
        assert torch.equal(res.logits, fz.infer(ids))
        ch, index, r64, r32, keep, share = TA.references(c, fz, ids, target)
        off = np.asarray(ch.host_offsets())
        assert int(np.diff(off).max()) > 128 and fz.g.feat_stride > 256, "a chosen list of several slices on rows of stride > 256"
        TA.check_against_float64(tally, f"target {target}", res, r64, r32, keep, share, target)
        TA.check_neighbours(tally, f"target {target}", res, index, r64, r32, keep)
    d = torch.randn(c.R, len(ids), c.f, generator=torch.Generator().manual_seed(3))
    got = ops.neighbour_contrib(fz.g, ch, d.to(dev()))
    X = torch.from_numpy(c.X)
    ref = {t: torch.cat([(X.to(t)[cols] * d.to(t)[r][rows]).sum(1) / cnt.to(t)[rows] for r, (rows, cols, cnt) in enumerate(index)])
           for t in (torch.float64, torch.float32)}
    tally.check("random d_agg", got, ref[torch.float64], ref[torch.float32])
    fz.check()
    tally.done()


def test_the_first_width_attribution_refuses():
    from pcgnn_amd import PcgnnLibraryError
    (last, refused), = [p for p in D.ATTR_LIMITS if p[1] in D.ATTR_LIMIT_SHAPES]
    c, fz = engine_of(refused)
    ids = c.batch(17)[0]
    with pytest.raises(PcgnnLibraryError, match="pcg_attr_set"):
        fz.attribute(ids)
    with pytest.raises(PcgnnLibraryError, match="pcg_attr_set"):
        fz.attribute(ids, neighbours=True)
    logits = fz.infer(ids)
    assert bool(torch.isfinite(logits).all()) and torch.equal(logits, TE.predict_loop(fz, ids, 7)[1])
    fz.check()


# ---- 4. unseen nodes at stride 260 ---------------------------------------------------------------------------------------------------
def test_attribute_new_on_wide_rows_is_attribute_on_the_rebuilt_graph():
    from pcgnn_amd.graph import QueryBatch
    from tests.test_gpu_explain_new import Oracle, assert_explained
    from tests.test_gpu_infer_new import engine, grow, split
    c = D.GradCase.of((260, 16, 1))
    nq = 17
    Xf, full_csr = grow(c.X, c.csr, nq, seed=nq)
    Xb, base_csr, Xq, q_pairs = split(Xf, full_csr, c.n)
    thr = [0.5] * c.R
    full = engine(Xf, full_csr, c.train_pos, c.emb, thr, c.params(), c.alpha)
    base = engine(Xb, base_csr, c.train_pos, c.emb, thr, c.params(), c.alpha)
    query = QueryBatch(Xq, q_pairs, base.g)
    assert query.nq == nq and base.g.feat_stride > 256
    ix = q_pairs[0][1]
    assert (ix < c.n).any() and (ix >= c.n).any()                          # rows of both tables among a query row's neighbours
    for target in A.TARGETS:
        at = assert_explained(base, Oracle(full, c.n, nq, target), query)
        assert at.d_self.shape == (nq, c.f) and bool(torch.isfinite(at.logits).all())
    base.check()
