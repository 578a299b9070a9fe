"""Custom losses and optimizers on the fused path: FusedPCGNN.forward / vjp / optimizer_step / train_step_custom and
PCGNNTrainer(loss_fn=..., optimizer=...).  Run with ``pytest -m gpu`` on an MI355X.

Cases (tests/vjp_ref.py): dense_ref's shapes (32, 64, 3) and (32, 128, 3) - the fixed-shape dense_vjp_kernel with and without the
weights' LDS copy - and (10, 16, 1), (24, 16, 5) - the run-time-shape one without and with it; batches of 1 (a lone row), 16 (a
full tile), 17 (a ragged tile: zero seeds for the rows beyond the batch) and 1025 (the first size at which pcg_wgrad shares a
weight tile between workgroups); three losses: the built-in one written in torch, class-weighted focal (gamma 2) on the gnn
logits + lambda_1 * CE on the label-aware logits with SUM reduction, and a label-smoothed CE of the gnn logits alone.

1  forward == predict bit for bit, and so are the logits pcg_dense_vjp's own forward writes.
2  every parameter's gradient (loss.backward() into p.grad) against tests/vjp_ref.py in float64, fed the device's own
   selection and the device's ReLU masks where a pre-activation is ambiguous (dense_ref.resolve_masks), by the rule of
   tests/test_gpu_grad_f64.py - e_kernel <= 8 * e_f32 + 2^-20, e_f32 the same reference in float32 on the CPU; not fitted to this
   code.  The built-in loss also against dense_ref.reference_pair's gradients.
3  exact statements: a loss of the gnn logits alone leaves the label classifier's gradients == 0; vjp twice gives identical bits,
   equal to autograd's; a second loss.backward() into the existing .grad gives exactly twice the first.
4  staleness: forward; predict; backward raises, forward; optimizer_step; backward raises, an older forward's backward raises;
   under no_grad forward returns plain tensors.
5  train_step_custom with the built-in loss, three steps at B 17 and 1025: the gradient each step took, recovered from Adam's
   first moment, against float64 (grad_check.check_first_moment), and theta / m / v against tests/adam_ref.py in float64 from
   the device's own state and gradient: m and v within the tolerances of test_adam_step_matches_torch_adam (rtol 1e-5 / 5e-5),
   theta by the same rule as the gradients with float32 torch.optim.Adam on the CPU as the yardstick.  (The absolute
   tolerance the partitioned steps' test holds theta to, lr * 2e-5, is a property of ITS seeds: at (32, 64, 3), B 1025
   one entry's g + wd * theta is 1.1e-8 - the size of eps, 1e-4 of its terms - and float32 torch.optim.Adam itself lands
   5.8 such tolerances from float64 there, on the CPU, before any kernel runs.)
6  PCGNNTrainer(engine="fused", loss_fn, optimizer=SGD): one step leaves theta_old - lr * grad, grad from vjp, bit for bit.
7  a PCGNNTrainer without the new arguments steps as a second default trainer does, bit for bit.

Measured on an MI355X (profiles/r19/custom_loss_ratios.txt): `ratio` = e_kernel / e_f32 over the entries with e_f32 >= 2^-24,
`of bound` = e_kernel / (8 * e_f32 + 2^-20), maximised over the three losses and the tensors (gradients, loss, both logits):

    shape (F, E, R)  kernel                                 B = 1        16           17           1025        | train_step_custom 17 / 1025
    (32, 64, 3)      dense_vjp_kernel<true, 32, 64, 3>      1.86 / 0.09  1.43 / 0.10  1.22 / 0.10  1.24 / 0.09 | 4.57 / 0.22   1.93 / 0.24
    (32, 128, 3)     dense_vjp_kernel<false, 32, 128, 3>    2.11 / 0.13  1.54 / 0.11  1.73 / 0.12  3.22 / 0.14 | -
    (10, 16, 1)      dense_vjp_kernel<false, 0, 0, 0>       2.13 / 0.12  1.99 / 0.09  2.40 / 0.11  1.15 / 0.16 | 4.86 / 0.31   2.93 / 0.38
    (24, 16, 5)      dense_vjp_kernel<true, 0, 0, 0>        1.78 / 0.09  1.83 / 0.12  1.33 / 0.08  1.25 / 0.09 | -

The other two fixed-shape kernels, a wide row and three of dense_ref.EDGE_SHAPES (profiles/r28/edge_shape_ratios.txt):

    (25, 64, 3)      dense_vjp_kernel<true, 25, 64, 3>      2.30 / 0.22  1.80 / 0.11  1.22 / 0.10  1.36 / 0.10
    (25, 128, 3)     dense_vjp_kernel<false, 25, 128, 3>    2.64 / 0.17  1.29 / 0.11  1.53 / 0.13  1.44 / 0.12
    (100, 64, 3)     dense_vjp_kernel<false, 0, 0, 0>       1.00 / 0.06  1.94 / 0.12  1.76 / 0.12  1.21 / 0.10
    (16, 64, 4)      dense_vjp_kernel<true, 0, 0, 0>        2.78 / 0.19  2.87 / 0.12  1.37 / 0.09  1.37 / 0.10
    (20, 128, 1)     dense_vjp_kernel<true, 0, 0, 0>        1.80 / 0.12  1.46 / 0.11  1.31 / 0.10  1.00 / 0.12
    (16, 272, 1)     dense_vjp_kernel<false, 0, 0, 0>       2.40 / 0.19  1.71 / 0.12  1.70 / 0.15  1.29 / 0.09

Every exact statement held; no batch came near the ReLU-kink cap (at most 6.1e-5 of the activations ambiguous).
"""
import numpy as np
import pytest
import torch

from tests import adam_ref as A
from tests import dense_ref as D
from tests import vjp_ref as V
from tests.grad_check import Tally, by_name, check_first_moment
from tests.util import PARAM_KEYS, build_model

pytestmark = pytest.mark.gpu

MAX_BATCH = max(V.BATCHES)
CLF = ("inter1.label_clf.weight", "inter1.label_clf.bias")
_ENGINES = {}


@pytest.fixture(scope="module")
def P():
    import pcgnn_amd
    from pcgnn_amd import ops  # noqa: F401  (fails loudly if the .so is missing)
    yield pcgnn_amd
    _ENGINES.clear()


def dev():
    return torch.device("cuda", 0)


def new_engine(P, c):
    from pcgnn_amd.fused import FusedPCGNN
    m = build_model(P, c, c.rho, graph=P.DeviceGraph(c.X, c.csr, c.train_pos, dev()))
    return m, FusedPCGNN(m, c.lr, c.wd, betas=c.betas, max_batch=MAX_BATCH)


def shared_engine(P, shape):
    """one engine per shape for the tests that never change a parameter"""
    if shape not in _ENGINES:
        c = D.GradCase.of(shape)
        _ENGINES[shape] = (c,) + new_engine(P, c)
    return _ENGINES[shape]


def on_dev(ids, lab):
    return torch.from_numpy(ids.astype(np.int32)).to(dev()), torch.from_numpy(lab.astype(np.int32)).to(dev())


def seeds_of(loss_fn, gnn, center, lab_d):
    """d loss / d (gnn logits, label-aware logits) by autograd on copies of the forward's values"""
    g, c = gnn.detach().clone().requires_grad_(True), center.detach().clone().requires_grad_(True)
    dl, dc = torch.autograd.grad(loss_fn(g, c, lab_d), (g, c), allow_unused=True)
    return dl, torch.zeros_like(c) if dc is None else dc


def torch_adam_f32(theta0, m0, v0, g, steps_before, c):
    """(theta', m', v') of one float32 torch.optim.Adam step on the CPU from the given float32 state and gradient"""
    p = torch.nn.Parameter(theta0.detach().cpu().float().clone())
    p.grad = g.detach().cpu().float().clone()
    opt = torch.optim.Adam([p], lr=c.lr, weight_decay=c.wd, betas=c.betas)
    if steps_before:
        opt.state[p] = {"step": torch.tensor(float(steps_before)), "exp_avg": m0.detach().cpu().clone(),
                        "exp_avg_sq": v0.detach().cpu().clone()}
    opt.step()
    return p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]


def kept_cap(what, share, wrong):
    print(f"{what}: {share:.2e} of the activations ambiguous (cap {D.AMBIGUOUS_CAP:.0e}), {wrong} masks wrong")
    assert share <= D.AMBIGUOUS_CAP, f"{what}: {share:.2e} of the activations are ambiguous - change the seed"
    assert wrong == 0, f"{what}: {wrong} ReLU masks of the device differ from the float64 sign outside the ambiguous band"


@pytest.mark.parametrize("B", V.BATCHES)
@pytest.mark.parametrize("shape", V.SHAPES)
def test_forward_and_gradients(P, shape, B):
    c, m, fz = shared_engine(P, shape)
    ids, lab = c.batch(B)
    ids_d, lab_d = on_dev(ids, lab)
    sets = m.inter1.chosen_sets(ids_d, lab_d, True)
    pred = fz.predict(ids_d, lab_d, True)
    named = dict(m.named_parameters())
    tally = Tally(f"{shape} B={B}")
    for name, make in V.LOSSES.items():
        loss_fn = make(c.alpha)
        for k in PARAM_KEYS(c.R):
            named[k].grad = None
        # 1: forward == predict
        gnn, center = fz.forward(ids_d, lab_d)
        assert gnn.grad_fn is not None and center.grad_fn is not None
        assert torch.equal(gnn, pred[0]) and torch.equal(center, pred[1]), "forward != predict"
        loss = loss_fn(gnn, center, lab_d)
        loss.backward(retain_graph=True)
        g1 = {k: named[k].grad.clone() for k in PARAM_KEYS(c.R)}
        # 2: against float64
        masks = D.device_masks(fz.acts, c.f, c.emb, c.R, B)
        r64, r32, share, wrong = V.reference_pair(c, ids, lab, sets, loss_fn, dev_masks=masks)
        kept_cap(f"{shape} B={B} {name}", share, wrong)
        for k in PARAM_KEYS(c.R):
            if name == "gnn_only" and k in CLF:               # 3: exactly zero (the reference's is zero too: no ratio to form)
                assert not r64["grads"][k].any() and not g1[k].any(), f"{name}: {k} must get no gradient"
                continue
            tally.check(f"{name} grad {k}", g1[k], r64["grads"][k], r32["grads"][k])
        tally.check(f"{name} loss", loss.detach(), r64["loss"], r32["loss"])
        tally.check(f"{name} logits", gnn.detach(), r64["logits"], r32["logits"])
        tally.check(f"{name} label-aware logits", center.detach(), r64["center"], r32["center"])
        if name == "builtin":
            d64, d32, _, _ = D.reference_pair(c, ids, lab, sets, dev_masks=masks)
            for k in PARAM_KEYS(c.R):
                tally.check(f"{name} grad {k} (dense_ref)", g1[k], d64["grads"][k], d32["grads"][k])
        # 3: vjp twice, and against autograd's; the launch's own logits (1)
        dl, dc = seeds_of(loss_fn, gnn, center, lab_d)
        va, logits_v, center_v = fz.vjp(dl, dc, want_logits=True)
        vb = fz.vjp(dl, dc)
        assert torch.equal(logits_v, pred[0]) and torch.equal(center_v, pred[1]), "pcg_dense_vjp's logits != predict"
        for k in PARAM_KEYS(c.R):
            assert torch.equal(va[k], vb[k]), f"{name}: vjp twice differs in {k}"
            assert torch.equal(va[k], g1[k]), f"{name}: vjp differs from loss.backward() in {k}"
        # 3: a second backward accumulates
        loss.backward()
        for k in PARAM_KEYS(c.R):
            assert torch.equal(named[k].grad, 2 * g1[k]), f"{name}: second backward into .grad is not twice the first in {k}"
    for k in PARAM_KEYS(c.R):
        named[k].grad = None
    fz.check()
    assert int(fz.step_counter.item()) == 0
    tally.done()


def test_staleness(P):
    c = D.GradCase.of((10, 16, 1))
    m, fz = new_engine(P, c)
    ids_d, lab_d = on_dev(*c.batch(17))
    loss_fn = V.focal_loss(c.alpha)
    opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=0.0)

    loss = loss_fn(*fz.forward(ids_d, lab_d), lab_d)
    fz.predict(ids_d, lab_d, True)
    with pytest.raises(RuntimeError, match="stale forward"):
        loss.backward()

    opt.zero_grad(set_to_none=True)
    loss = loss_fn(*fz.forward(ids_d, lab_d), lab_d)
    loss.backward(retain_graph=True)                      # (live: fine)
    fz.optimizer_step(opt)
    with pytest.raises(RuntimeError, match="stale forward"):
        loss.backward()

    first = loss_fn(*fz.forward(ids_d, lab_d), lab_d)
    second = loss_fn(*fz.forward(ids_d, lab_d), lab_d)
    with pytest.raises(RuntimeError, match="stale forward"):
        first.backward()
    second.backward()
    fz.forward(ids_d, lab_d)
    fz.train_step(ids_d, lab_d)
    with pytest.raises(RuntimeError, match="stale forward"):
        fz.vjp(torch.zeros(17, 2, device=dev()), torch.zeros(17, 2, device=dev()))

    with torch.no_grad():
        gnn, center = fz.forward(ids_d, lab_d)
    assert gnn.grad_fn is None and center.grad_fn is None and not gnn.requires_grad and not center.requires_grad
    pred = fz.predict(ids_d, lab_d, True)
    assert torch.equal(gnn, pred[0]) and torch.equal(center, pred[1])
    with pytest.raises(ValueError):
        fz.forward(ids_d, None, True)
    fz.check()


@pytest.mark.parametrize("shape,B", [((32, 64, 3), 17), ((32, 64, 3), 1025), ((10, 16, 1), 17), ((10, 16, 1), 1025)])
def test_train_step_custom_against_float64_adam(P, shape, B):
    c = D.GradCase.of(shape)
    m, fz = new_engine(P, c)
    loss_fn = V.builtin_loss(c.alpha)
    tally = Tally(f"{shape} B={B} train_step_custom")
    for step in range(3):
        ids, lab = c.batch(B, salt=step)
        ids_d, lab_d = on_dev(ids, lab)
        theta0, m0, v0 = fz.theta.clone(), fz.m.clone(), fz.v.clone()
        params0 = {k: v.detach().cpu().clone() for k, v in fz.views.items()}
        sets = m.inter1.chosen_sets(ids_d, lab_d, True)
        # the gradient the step is about to take: the same launches with apply = 0
        gnn, center = fz.forward(ids_d, lab_d)
        grads = fz.vjp(*seeds_of(loss_fn, gnn, center, lab_d))
        g_flat = torch.empty_like(theta0)
        for k, dst in by_name(fz, g_flat).items():
            dst.copy_(grads[k])
        loss = fz.train_step_custom(ids_d, lab_d, loss_fn)
        torch.cuda.synchronize()
        assert int(fz.step_counter.item()) == step + 1
        assert torch.equal(fz.clf_next, fz.theta[fz.n_rest:]), "the label classifier is stepped with everything else"
        masks = D.device_masks(fz.acts, c.f, c.emb, c.R, B)
        r64, r32, share, wrong = D.reference_pair(c, ids, lab, sets, params=params0, dev_masks=masks)
        kept_cap(f"{shape} B={B} step {step}", share, wrong)
        check_first_moment(tally, c, fz, f"step {step}", fz.m, theta0, r64, r32, state=None if step == 0 else (m0, v0))
        tally.check(f"step {step} loss", loss, r64["loss"], r32["loss"])
        # Adam itself: float64 adam_ref from the device's own float32 inputs, float32 torch.optim.Adam on the CPU as the yardstick
        # (m, v: the tolerances of test_adam_step_matches_torch_adam; theta: the rule above - see the module docstring)
        fig = A.adam_figures((fz.theta, fz.m, fz.v), theta0, m0, v0, g_flat, step + 1, c.lr, c.betas, 1e-8, c.wd)
        print(f"{shape} B={B} step {step}: Adam, of tolerance: m {fig['m']:.3f}  v {fig['v']:.3f}  (theta at lr * 2e-5: {fig['theta']:.3f})")
        assert max(fig["m"], fig["v"]) <= 1.0, fig
        ref = A.adam_ref(theta0, m0, v0, g_flat, step + 1, c.lr, c.betas, 1e-8, c.wd)
        tally.check(f"step {step} Adam theta", fz.theta, ref[0], torch_adam_f32(theta0, m0, v0, g_flat, step, c)[0])
    fz.check()
    tally.done()


def mini_trainer(**kw):
    from pcgnn_amd import synth
    from pcgnn_amd.handler import PCGNNTrainer
    w = synth.make_workload("mini", 6000, 32, (4000, 30000, 90000), 0.12, seed=3)
    return PCGNNTrainer(w, dict(engine="fused", seed=5, batch_size=256), dev(), **kw)


def test_trainer_with_an_external_optimizer(P):
    lr = 0.05
    loss_fn = V.focal_loss(2.0)
    tr = mini_trainer(loss_fn=loss_fn, optimizer=lambda ps: torch.optim.SGD(ps, lr))
    fz = tr.fused
    ids = tr.start_epoch(0)[:256]
    labels = tr.labels_i32[ids.long()]
    gnn, center = fz.forward(ids, labels)
    grads = fz.vjp(*seeds_of(loss_fn, gnn, center, labels))
    want = {k: v.add(grads[k], alpha=-lr) for k, v in fz.views.items()}       # theta_old - lr * grad
    loss = tr.step(ids)
    torch.cuda.synchronize()
    assert loss is not None and bool(torch.isfinite(loss))
    for k, v in fz.views.items():
        assert float(grads[k].abs().max()) > 0, k
        assert torch.equal(v, want[k]), f"{k}: not theta_old - lr * grad"
    assert torch.equal(fz.clf_next, fz.theta[fz.n_rest:])
    fz.check()
    with pytest.raises(ValueError):
        from pcgnn_amd.handler import PCGNNTrainer
        PCGNNTrainer(tr.w, dict(engine="graph", batch_size=256), dev(), loss_fn=loss_fn)


def test_trainer_custom_loss_with_the_engines_adam(P):
    """loss_fn alone: step() is train_step_custom - with the built-in loss it moves the parameters as three steps of a float64
    Adam would (test_train_step_custom_against_float64_adam holds the numbers); here: the step is taken and counted"""
    tr = mini_trainer(loss_fn=V.builtin_loss(2.0))
    ids = tr.start_epoch(0)[:256]
    before = tr.fused.theta.clone()
    loss = tr.step(ids)
    assert bool(torch.isfinite(loss)) and int(tr.fused.step_counter.item()) == 1 and not torch.equal(before, tr.fused.theta)
    tr.fused.check()


def test_default_trainer_is_unchanged(P):
    a, b = mini_trainer(), mini_trainer(loss_fn=None, optimizer=None)
    assert a.opt is None and b.opt is None and b.loss_fn is None
    ids = a.start_epoch(0)
    for s in range(3):
        batch = ids[s * 256:(s + 1) * 256]
        assert a.step(batch) is None and b.step(batch) is None
    for tr in (a, b):
        tr.fused.flush()
    torch.cuda.synchronize()
    assert torch.equal(a.fused.theta, b.fused.theta) and torch.equal(a.fused.m, b.fused.m)
    assert int(a.fused.step_counter.item()) == 3
    a.fused.check()
