"""Training gradients against float64 at batch-size boundaries.  Run with ``pytest -m gpu`` on an MI355X.

Every way the engine forms a gradient - ``gradients(via="acts")`` (dense kernel -> transposed activations -> pcg_wgrad),
``gradients(via="slabs")`` (per-tile slabs summed in tile order) and the real training step (pending words, weight gradients
riding in the next gather launch or in pcg_adam_flush, the label classifier stepped inside the select launch; read back through
Adam's first moment) - against the float64 CPU reference of tests/dense_ref.py, with the chosen sets taken from the device
(selection is index-only and held bit-exact elsewhere).  One engine of max_batch 2049 per shape runs the batch sizes in
descending order - 2049 2048 1025 1024 1023 65 64 63 17 16 15 1, then 17 again - so that every ragged batch follows a longer
one in the same activations, slabs and workspace: the 16-row tile tail, empty wave ranges of the weight-gradient workgroups
(1, 2, 3, 5 blocks), n_split 4 -> 2 -> 1 and kparts 1 -> 2 -> 3 at 64 / 65 and 128 / 129 tiles, the label classifier's
workgroup per 1024 rows, and a short batch on a large engine (the host's block-count hint is not the device's).

Bound (not fitted to the kernels): per case and tensor e = max|x - x64| / max|x64|; e_kernel <= 8 * e_f32 + 2^-20, e_f32 the
same reference code run in float32 on the CPU with the same sets and masks (for the first-moment cases through float32
torch.optim.Adam and the same recovery formula).  One batch row dropped or counted twice moves every tensor by more than ten
such tolerances (tests/test_dense_ref_host.py).  ReLU kinks: dense_ref.py - the device's own mask where |pre_f64| is within
16 x the f32 rounding of zero (at most 1e-4 of a case's activations), asserted equal to the f64 sign everywhere else.

Measured on an MI355X (profiles/r12/grad_f64_ratios.txt), maximised over the batch sizes and over the tensors, loss and logits
included: `ratio` = e_kernel / e_f32 over the entries with e_f32 >= 2^-24 (a float32 run that happens to be exact has no
ratio), `of bound` = e_kernel / (8 * e_f32 + 2^-20) over all entries:

    shape (F, E, R)  kernel                                  gradients() ratio  of bound | train step ratio  of bound
    (32, 64, 3)      dense_step_kernel<true, 32, 64, 3>      2.12               0.30     | 5.46              0.28
    (25, 64, 3)      dense_step_kernel<true, 25, 64, 3>      2.32               0.15     | -                 -
    (32, 128, 3)     dense_step_kernel<false, 32, 128, 3>    2.04               0.25     | -                 -
    (25, 128, 3)     dense_step_kernel<false, 25, 128, 3>    2.74               0.16     | 3.06              0.28
    (10, 16, 1)      dense_step_kernel<false, 0, 0, 0>       2.40               0.16     | -                 -
    (16, 48, 5)      dense_step_kernel<false, 0, 0, 0>       2.28               0.16     | -                 -
    (24, 16, 5)      dense_step_kernel<true, 0, 0, 0>        1.43               0.13     | -                 -

Wide feature rows (dense_ref.WIDE_SHAPES; profiles/r17/wide_f64_ratios.txt): the dense staging's F > 64 self-row loop and its second
aggregate loop (elements beyond the first 2048 of a tile's [R][16][F] aggregates, with a summation of its own), and stride > 256 -
two accumulators per lane, gather_train_kernel<2> with the Adam and weight-gradient riders.  Every batch of these shapes has the
graph's two largest rows pinned at tile rows 0, 1, 14, 15 of the first tile and the hub on a ragged batch's last tile
(dense_ref.wide_pins), and the test asserts from the device's own sets (more than 128 entries: several gather chunks) that a
pinned row is staged by the first 2048 elements and - every batch of a whole tile - one by the loop beyond:

    shape (F, E, R)  kernel                                  gradients() ratio  of bound | train step ratio  of bound
    (100, 64, 3)     dense_step_kernel<false, 0, 0, 0>       2.33               0.14     | 3.08              0.18
    (68, 16, 2)      dense_step_kernel<true, 0, 0, 0>        1.44               0.12     | -                 -
    (260, 16, 1)     dense_step_kernel<true, 0, 0, 0>        2.09               0.20     | 4.11              0.19
    (400, 16, 1)     dense_step_kernel<false, 0, 0, 0>       2.80               0.24     | -                 -

Edge shapes (dense_ref.EDGE_SHAPES; profiles/r28/edge_shape_ratios.txt; what each reaches: the table's comment, asserted by
tests/test_edge_shapes_host.py): the run-time-shape kernel with the weights' LDS copy at E = 32, 64 and 128, R = 4, 7 and 8, E / 16
= 17 column tiles on 16 waves; plain batches (BATCHES_SHORT), train steps at B = 17 / 1025:

    shape (F, E, R)  kernel                                  gradients() ratio  of bound | train step ratio  of bound
    (16, 64, 4)      dense_step_kernel<true, 0, 0, 0>        2.81               0.19     | 3.03              0.18
    (30, 64, 3)      dense_step_kernel<true, 0, 0, 0>        1.64               0.12     | -                 -
    (20, 128, 1)     dense_step_kernel<true, 0, 0, 0>        1.18               0.12     | -                 -
    (20, 32, 7)      dense_step_kernel<true, 0, 0, 0>        1.87               0.14     | -                 -
    (17, 32, 8)      dense_step_kernel<true, 0, 0, 0>        3.48               0.15     | 2.90              0.33
    (32, 64, 8)      dense_step_kernel<false, 0, 0, 0>       2.11               0.13     | -                 -
    (64, 64, 3)      dense_step_kernel<false, 0, 0, 0>       1.58               0.12     | -                 -
    (16, 272, 1)     dense_step_kernel<false, 0, 0, 0>       2.12               0.13     | 4.42              0.23

Every kernel error is a few 1e-7 of the tensor's largest element - the size of the float32 CPU run's own - so the bound is
mostly its floor; nothing came near the margin of 8.  ((10, 16, 1) runs the run-time-shape kernel WITHOUT the weights' LDS copy:
its K-split partial tiles do not fit where the W_intra copy would be; (24, 16, 5) is here for the run-time-shape kernel with it.)
"""
import numpy as np
import pytest
import torch

from tests import dense_ref as D
from tests.grad_check import Tally, check_first_moment
from tests.util import PARAM_KEYS, build_model

pytestmark = pytest.mark.gpu

TRAIN_SHAPES = [(32, 64, 3), (25, 128, 3)]
WIDE_TRAIN_SHAPES = [(100, 64, 3), (260, 16, 1)]      # gather_train_kernel<1> at stride 100 / <2> at stride 260, with their riders
# (shape, B) of the first-moment test: the four boundary sizes for the project's shapes, a short and a long batch for the wide ones
TRAIN_CASES = ([pytest.param(s, B, id=f"shape{i}-{B}") for i, s in enumerate(TRAIN_SHAPES) for B in (17, 1024, 1025, 2049)]
               + [pytest.param(s, B, id=f"shape{len(TRAIN_SHAPES) + i}-{B}") for i, s in enumerate(WIDE_TRAIN_SHAPES)
                  for B in (17, 1025)]
               + [pytest.param(s, B, id=f"edge{i}-{B}") for i, s in enumerate(D.EDGE_TRAIN_SHAPES) for B in (17, 1025)])


@pytest.fixture(scope="module")
def P():
    import pcgnn_amd
    from pcgnn_amd import ops  # noqa: F401  (fails loudly if the .so is missing)
    return pcgnn_amd


def dev():
    return torch.device("cuda", 0)


def engine(P, c):
    from pcgnn_amd.fused import FusedPCGNN
    m = build_model(P, c, c.rho, graph=P.DeviceGraph(c.X, c.csr, c.train_pos, dev()))
    return m, FusedPCGNN(m, c.lr, c.wd, betas=c.betas, max_batch=D.MAX_BATCH)


def on_dev(ids, lab):
    return torch.from_numpy(ids.astype(np.int32)).to(dev()), torch.from_numpy(lab.astype(np.int32)).to(dev())


def table_of(shape):
    return next(t for t in (D.SHAPES, D.WIDE_SHAPES, D.EDGE_SHAPES) if shape in t)


def draw(c, shape, B, salt=0):
    """the case's batch; a wide shape's with the hub rows pinned into it (dense_ref.wide_pins)"""
    return c.wide_batch(B, salt) if shape in D.WIDE_SHAPES else c.batch(B, salt)


def staged_pins(c, shape, sets, B):
    """Wide shapes: the PINNED rows of several gather chunks (the device's own sets: more than 128 entries) the dense kernel's
    staging prologue covers with its first 2048 aggregate elements / with the loop beyond, as (relation, batch row) lists;
    asserted non-empty where the batch has a whole first tile.  None for the project's shapes."""
    if shape not in D.WIDE_SHAPES:
        return None
    pins = c.wide_pins(B)
    direct, beyond = D.staged_multi_chunk_rows(sets, c.f, B)
    direct, beyond = [x for x in direct if x[1] in pins], [x for x in beyond if x[1] in pins]
    print(f"{shape} B={B}: multi-chunk pinned rows (relation, row): first 2048 elements {direct}, loop beyond {beyond}")
    assert direct, f"{shape} B={B}: no row of several chunks among the first 2048 staged elements"
    if B >= D.TILE_ROWS:
        assert beyond, f"{shape} B={B}: no row of several chunks in the staging loop beyond 2048 elements"
    return direct, beyond


def reference(c, fz, ids, lab, sets, B, params=None):
    """reference_pair with the engine's ReLU masks of its last acts-mode dense launch; the cap and the mask rule asserted"""
    masks = D.device_masks(fz.acts, c.f, c.emb, c.R, B)
    r64, r32, share, wrong = D.reference_pair(c, ids, lab, sets, params=params, dev_masks=masks)
    print(f"B={B}: {share:.2e} of the activations ambiguous (cap {D.AMBIGUOUS_CAP:.0e})")
    assert share <= D.AMBIGUOUS_CAP, f"B={B}: {share:.2e} of the activations are ambiguous - change the seed"
    assert wrong == 0, f"B={B}: {wrong} ReLU masks of the device differ from the float64 sign outside the ambiguous band"
    return r64, r32


@pytest.mark.parametrize("shape", list(D.SHAPES) + list(D.WIDE_SHAPES) + list(D.EDGE_SHAPES))
def test_gradients_against_float64(P, shape):
    kernel, batches, _ = table_of(shape)[shape]   # (which dense kernel runs: asserted by the shared-memory rule on the host)
    c = D.GradCase.of(shape)
    m, fz = engine(P, c)
    tally = Tally(f"{shape} gradients()")
    staged = []
    for B in batches:
        ids, lab = draw(c, shape, B)
        ids_d, lab_d = on_dev(ids, lab)
        sets = m.inter1.chosen_sets(ids_d, lab_d, True)
        staged.append(staged_pins(c, shape, sets, B))
        got = {}
        for via in ("acts", "slabs"):
            grads = fz.gradients(ids_d, lab_d, via=via)
            got[via] = (grads, float(fz.last_loss()), fz.logits[:B].clone(), fz.center[:B].clone())
            if via == "acts":
                r64, r32 = reference(c, fz, ids, lab, sets, B)
        for via, (grads, loss, logits, center) in got.items():
            for k in PARAM_KEYS(c.R):
                tally.check(f"B={B} via={via} grad {k}", grads[k], r64["grads"][k], r32["grads"][k])
            tally.check(f"B={B} via={via} loss", torch.tensor(loss), r64["loss"], r32["loss"])
            tally.check(f"B={B} via={via} logits", logits, r64["logits"], r32["logits"])
            tally.check(f"B={B} via={via} label-aware logits", center, r64["center"], r32["center"])
    assert int(fz.step_counter.item()) == 0
    if shape in D.WIDE_SHAPES:      # both staging loops met a row of several chunks (every batch of a whole tile: staged_pins)
        assert any(d for d, _ in staged) and any(b for _, b in staged)
    tally.done()


@pytest.mark.parametrize("shape,B", TRAIN_CASES)
def test_train_step_gradient_through_first_moment(P, shape, B):
    """One deferred train_step, then flush(), on an engine of max_batch 2049: from m = v = 0 the step leaves
    m1 = (1 - beta1) (g + wd theta0), so g = m1 / (1 - beta1) - wd theta0.  (B = 17: the flush launch's block count is the
    engine's 129, the device's pending word says 2.)"""
    c = D.GradCase.of(shape)
    m, fz = engine(P, c)
    ids, lab = draw(c, shape, B)
    ids_d, lab_d = on_dev(ids, lab)
    theta0 = fz.theta.clone()
    sets = m.inter1.chosen_sets(ids_d, lab_d, True)
    staged_pins(c, shape, sets, B)
    fz.train_step(ids_d, lab_d, defer=True)
    fz.flush()
    loss = float(fz.last_loss())
    assert int(fz.step_counter.item()) == 1
    r64, r32 = reference(c, fz, ids, lab, sets, B)
    tally = Tally(f"{shape} train step")
    check_first_moment(tally, c, fz, f"B={B}", fz.m, theta0, r64, r32)
    tally.check(f"B={B} loss", torch.tensor(loss), r64["loss"], r32["loss"])
    tally.check(f"B={B} logits", fz.logits[:B], r64["logits"], r32["logits"])
    tally.done()


@pytest.mark.parametrize("shape", TRAIN_SHAPES + [(260, 16, 1)])
def test_deferred_update_riding_in_the_next_step(P, shape):
    """train_step(defer=True) at B = 2049, again at B = 1025, flush(): the first update rides in the second step's gather launch
    (three workgroups per weight-gradient tile, sized for the engine's 129 blocks).  A second engine flushes in between: both
    end bit-identical, so its theta1 / m1 are what the deferred engine used, and the second step's gradient is
    (m2 - beta1 m1) / (1 - beta1) - wd theta1, compared with the reference at theta1 with the device's sets at theta1."""
    c = D.GradCase.of(shape)
    (ma, fa), (mb, fb) = engine(P, c), engine(P, c)
    (ids1, lab1), (ids2, lab2) = draw(c, shape, 2049), draw(c, shape, 1025, salt=1)
    d1, d2 = on_dev(ids1, lab1), on_dev(ids2, lab2)
    fa.train_step(*d1, defer=True)
    fa.train_step(*d2, defer=True)
    fa.flush()
    fb.train_step(*d1, defer=True)
    fb.flush()
    torch.cuda.synchronize()
    theta1, m1, v1 = fb.theta.clone(), fb.m.clone(), fb.v.clone()
    params1 = {k: v.detach().cpu().clone() for k, v in fb.views.items()}
    sets2 = mb.inter1.chosen_sets(*d2, True)
    staged_pins(c, shape, sets2, 1025)
    fb.train_step(*d2, defer=True)
    fb.flush()
    torch.cuda.synchronize()
    fa.check()
    fb.check()
    assert torch.equal(fa.theta, fb.theta) and torch.equal(fa.m, fb.m), "deferred and flushed engines must end bit-identical"
    assert int(fa.step_counter.item()) == 2
    r64, r32 = reference(c, fa, ids2, lab2, sets2, 1025, params=params1)
    tally = Tally(f"{shape} train step")
    check_first_moment(tally, c, fa, "B=2049 then 1025", fa.m, theta1, r64, r32, state=(m1, v1))
    tally.check("B=2049 then 1025 loss", torch.tensor(float(fa.last_loss())), r64["loss"], r32["loss"])
    tally.check("B=2049 then 1025 logits", fa.logits[:1025], r64["logits"], r32["logits"])
    tally.done()
