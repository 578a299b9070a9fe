"""Training of the GraphSAGE / GCN baselines on the device (pcg_baseline_train, BaselineEngine.train_step / train_epoch /
loss_and_grad / backward) on an MI355X: loss and gradients against float64 (tests/baseline_train_ref.py) on the crafted graph of
the inference tests at every batch size where the weight GEMM's part split changes, the forward against ``infer`` bit for bit,
twelve Adam steps against float64 Adam, the bit-for-bit equalities between the ways to run the same steps, NaN parity with
autograd, extents inside a guarded arena, the rejections, and ``ModelHandler``'s ``baseline_fused_train``.  Run with
``pytest -m gpu``."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from tests import adam_ref as A
from tests import baseline_ref as BR
from tests import baseline_train_ref as T
from tests import dense_ref as D
from tests.grad_check import Tally
from tests.guarded import GuardedArena

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def graph(F):
    import pcgnn_amd as P
    return T.memo(("g", F), lambda: P.DeviceGraph(T.features(F), [T.csr()], [], dev()))


def fresh_model(F, E, shape):
    """a model of its own with the case's weights (the tests that train change them)"""
    from pcgnn_amd import graphsage as GS
    model = BR.build_model(GS, graph(F), F, E, shape, seed=F * 1000 + E)
    W_enc, W_cls = T.model_weights(F, E, shape)
    assert np.array_equal(model.enc.weight.detach().cpu().numpy(), W_enc) and np.array_equal(model.weight.detach().cpu().numpy(), W_cls)
    return model


def model_of(F, E, shape):
    """the case's model, shared by the tests that only read it"""
    return T.memo(("model", F, E, shape), lambda: fresh_model(F, E, shape))


def weights(model):
    return model.enc.weight.detach().cpu().numpy().copy(), model.weight.detach().cpu().numpy().copy()


def bits(x):
    return x.detach().contiguous().view(torch.int32)


def same(x, y):
    return torch.equal(bits(x), bits(y))


def state_of(model):
    """(W_enc, W_cls, m_enc, v_enc, m_cls, v_cls) clones and the step count"""
    o = model.optimizer_state()
    return [model.enc.weight.detach().clone(), model.weight.detach().clone(), o["m_enc"], o["v_enc"], o["m_cls"], o["v_cls"]], o["step"]


def trainable(F, E, shape):
    model = fresh_model(F, E, shape)
    model.configure_optimizer(T.LR, T.WD, betas=T.BETAS, eps=T.EPS)
    return model


# ---- 1. gradients against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,E,shape", T.CASES)
def test_gradients_against_float64(F, E, shape):
    model = model_of(F, E, shape)
    W_enc, W_cls = T.model_weights(F, E, shape)
    t = Tally(f"baseline train F={F} E={E} {shape}")
    wrong_masks = []
    for B in T.BATCHES:
        ids, labels = T.batch(B, T.salt_of(F, E, shape))
        dev_mask = model.embed(ids) > 0
        loss, d_enc, d_cls = model.loss_and_grad(ids, labels)
        assert tuple(d_enc.shape) == W_enc.shape and tuple(d_cls.shape) == W_cls.shape and loss.dim() == 0
        r64, r32, share, wrong = T.reference_pair(F, shape, ids, labels, W_enc, W_cls, dev_mask)
        assert share <= D.AMBIGUOUS_CAP, (B, share)
        wrong_masks.append((B, wrong))
        print(f"{t.tag} B={B} parts={T.kparts(B)} ambiguous share {share:.2e} mask mismatches {wrong}")
        for what in ("loss", "d_enc", "d_cls"):
            got = {"loss": loss, "d_enc": d_enc, "d_cls": d_cls}[what]
            t.check(f"B={B} {what}", got, torch.as_tensor(r64[what]), torch.as_tensor(r32[what]))
    model.check()
    assert all(w == 0 for _, w in wrong_masks), wrong_masks
    assert same(model.enc.weight, torch.from_numpy(W_enc).to(dev())) and same(model.weight, torch.from_numpy(W_cls).to(dev()))
    t.done()


# ---- 2. forward identity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,E,shape", [(25, 64, "sage_concat"), (32, 128, "gcn"), (509, 64, "gcn"), (1, 16, "sage_concat")])
def test_forward_identity(F, E, shape):
    model = model_of(F, E, shape)
    t = Tally(f"baseline train forward F={F} E={E} {shape}")
    for B in (1, 17, 1025):
        ids, labels = T.batch(B, 3)
        before = model.infer(ids)
        loss, _, _ = model.loss_and_grad(ids, labels)
        assert same(model.infer(ids), before)                      # (nothing moved: the call's logits are these)
        y = torch.from_numpy(labels)
        ce64 = torch.nn.functional.cross_entropy(before.cpu().double(), y)
        ce32 = torch.nn.functional.cross_entropy(before.cpu().float(), y)
        t.check(f"B={B} loss against the cross entropy of infer's logits", loss, ce64, ce32)
        # the batches' losses of a one-batch epoch and of a step are this loss, bit for bit
        m2 = trainable(F, E, shape)
        assert same(m2.train_step(ids, labels), loss)
    t.done()


# ---- 3. twelve training steps against float64 Adam ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(T.STEP_CASES)))
def test_twelve_train_steps(case):
    F, E, shape = T.STEP_CASES[case]
    model = trainable(F, E, shape)
    # (from zero first moments and second moments T.WARM_V - tests/baseline_train_ref.py says why -, through the public call)
    warm = model.optimizer_state()
    assert warm["step"] == 0 and not any(bool(warm[k].any()) for k in ("m_enc", "v_enc", "m_cls", "v_cls"))
    model.load_optimizer_state(dict(warm, v_enc=torch.full_like(warm["v_enc"], T.WARM_V), v_cls=torch.full_like(warm["v_cls"], T.WARM_V)))
    flat = lambda cls, enc: T.flat(cls.detach().cpu(), enc.detach().cpu())
    t = Tally(f"baseline train steps F={F} E={E} {shape}")
    misses = []
    for k, (ids, labels) in enumerate(T.step_batches(case)):
        W_enc, W_cls = weights(model)
        o = model.optimizer_state()
        theta, m, v = flat(model.weight, model.enc.weight), flat(o["m_cls"], o["m_enc"]), flat(o["v_cls"], o["v_enc"])
        assert o["step"] == k
        dev_mask = model.embed(ids) > 0
        loss = model.train_step(ids, labels)
        r64, r32, share, wrong = T.reference_pair(F, shape, ids, labels, W_enc, W_cls, dev_mask)
        assert share <= D.AMBIGUOUS_CAP and wrong == 0, (k, share, wrong)
        t.check(f"step {k + 1} B={len(ids)} loss", loss, torch.as_tensor(r64["loss"]), torch.as_tensor(r32["loss"]))
        o = model.optimizer_state()
        got = (flat(model.weight, model.enc.weight), flat(o["m_cls"], o["m_enc"]), flat(o["v_cls"], o["v_enc"]))
        fig = A.adam_figures(got, theta, m, v, T.flat(r64["d_cls"], r64["d_enc"]), k + 1, T.LR, T.BETAS, T.EPS, T.WD)
        print(f"{t.tag} step {k + 1} B={len(ids)}: of tolerance theta {fig['theta']:.3f} m {fig['m']:.3f} v {fig['v']:.3f} "
              f"excluded {fig['excluded']:.2e}")
        if not (fig["theta"] <= 1 and fig["m"] <= 1 and fig["v"] <= 1 and fig["excluded"] <= A.CANCEL_CAP):
            misses.append((k + 1, fig))
    assert model.optimizer_state()["step"] == 12
    model.check()
    assert not misses, misses
    t.done()


# ---- 4. bit-for-bit equalities ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,E,shape,B", [(25, 64, "sage", 129), (32, 128, "sage_concat", 1040), (509, 64, "gcn", 129)])
def test_epoch_equals_steps_and_runs_repeat(F, E, shape, B):
    rs = np.random.RandomState(B)
    ids = np.concatenate([T.pins(), rs.randint(2, T.N, size=2 * B + 17 - len(T.pins()))])
    labels = T.node_labels()[ids]
    by_epoch, by_step, again = trainable(F, E, shape), trainable(F, E, shape), trainable(F, E, shape)
    losses = by_epoch.train_epoch(ids, labels, B)
    assert losses.shape == (3,) and torch.isfinite(losses).all()
    one = torch.stack([by_step.train_step(ids[b0:b0 + B], labels[b0:b0 + B]) for b0 in range(0, len(ids), B)])
    losses2 = again.train_epoch(torch.from_numpy(ids).to(dev()), torch.from_numpy(labels).to(dev()), B)
    (sa, na), (sb, nb), (sc, nc) = state_of(by_epoch), state_of(by_step), state_of(again)
    assert na == nb == nc == 3
    assert same(losses, one) and same(losses, losses2)
    for x, y, z in zip(sa, sb, sc):
        assert same(x, y) and same(x, z)
    assert not same(sa[0], torch.from_numpy(T.model_weights(F, E, shape)[0]).to(dev()))      # (it trained)
    # infer sees the steps; the state goes out and back in; reset starts over
    assert same(by_epoch.infer(ids[:40]), by_step.infer(ids[:40]))
    saved = by_epoch.optimizer_state()
    by_epoch.train_step(ids[:B], labels[:B])
    by_step.train_step(ids[:B], labels[:B])
    by_epoch.load_optimizer_state(saved)
    assert by_epoch.optimizer_state()["step"] == 3 and same(by_epoch.optimizer_state()["m_enc"], saved["m_enc"])
    by_epoch.reset_optimizer()
    o = by_epoch.optimizer_state()
    assert o["step"] == 0 and not o["m_enc"].any() and not o["v_cls"].any()
    by_epoch.check()


@pytest.mark.parametrize("F,E,shape", [(25, 64, "sage"), (32, 128, "gcn")])
def test_backward_with_a_torch_optimizer_and_accumulation(F, E, shape):
    mine, theirs = trainable(F, E, shape), fresh_model(F, E, shape)
    opt = torch.optim.Adam(theirs.parameters(), lr=T.LR, betas=T.BETAS, eps=T.EPS, weight_decay=T.WD)
    rtol_m, atol_m = A.M_TOL
    rtol_v, atol_v = A.V_TOL
    for k, (ids, labels) in enumerate(T.step_batches(0)[:4]):          # 1040, 1040, 1040, 17 rows
        l1 = mine.train_step(ids, labels)
        l2 = theirs.backward(ids, labels)
        opt.step()
        if k == 0:
            assert same(l1, l2)                                        # (the same weights: the same loss)
        o = mine.optimizer_state()
        for p, pm, pv, q in ((mine.enc.weight, o["m_enc"], o["v_enc"], theirs.enc.weight), (mine.weight, o["m_cls"], o["v_cls"], theirs.weight)):
            st = opt.state[q]
            np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().cpu().numpy(), rtol=0, atol=T.LR * A.THETA_ATOL_PER_LR)
            np.testing.assert_allclose(pm.cpu().numpy(), st["exp_avg"].cpu().numpy(), rtol=rtol_m, atol=atol_m)
            np.testing.assert_allclose(pv.cpu().numpy(), st["exp_avg_sq"].cpu().numpy(), rtol=rtol_v, atol=atol_v)
    # accumulate: twice the gradient, exactly
    ids, labels = T.batch(1025)
    model = fresh_model(F, E, shape)
    model.backward(ids, labels)
    g_enc, g_cls = model.enc.weight.grad.clone(), model.weight.grad.clone()
    _, d_enc, d_cls = model.loss_and_grad(ids, labels)
    assert same(g_enc, d_enc) and same(g_cls, d_cls)
    model.backward(ids, labels, accumulate=True)
    assert same(model.enc.weight.grad, 2 * g_enc) and same(model.weight.grad, 2 * g_cls)
    model.backward(ids, labels)                                        # (not accumulating: replaced)
    assert same(model.enc.weight.grad, g_enc) and g_enc.abs().max() > 0


# ---- 5. NaN parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,finite", [("sage", False), ("sage_concat", False), ("gcn", True)])
def test_nan_parity_with_autograd(shape, finite):
    F, E = 25, 64
    model = fresh_model(F, E, shape)
    ids, labels = T.nan_batch()
    loss, d_enc, d_cls = model.loss_and_grad(ids, labels)
    model.zero_grad()
    ref = model.loss(ids.tolist(), labels)
    ref.backward()
    assert bool(torch.isfinite(loss)) == finite == bool(torch.isfinite(ref))
    assert torch.equal(torch.isnan(d_enc), torch.isnan(model.enc.weight.grad))
    assert torch.equal(torch.isnan(d_cls), torch.isnan(model.weight.grad))
    assert bool(torch.isfinite(d_enc).all()) == finite and bool(torch.isfinite(d_cls).all()) == finite
    if finite:
        np.testing.assert_allclose(d_enc.cpu().numpy(), model.enc.weight.grad.cpu().numpy(), rtol=0, atol=2e-5)
        np.testing.assert_allclose(d_cls.cpu().numpy(), model.weight.grad.cpu().numpy(), rtol=0, atol=2e-5)
    model.check()


# ---- 6. extents -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,E,shape", [(25, 64, "sage_concat"), (509, 64, "gcn"), (32, 128, "sage_concat"), (300, 16, "gcn")])
def test_extents(F, E, shape):
    from pcgnn_amd import _lib, ops
    lib = _lib.load()
    K = 2 * F if BR.SHAPES[shape]["concat_self"] else F
    for n, batch, apply in ((3 * 17 + 5, 17, 1), (17, 17, 0), (1025 + 40, 1025, 1), (1, 1, 0)):
        model = trainable(F, E, shape)
        eng = model.engine()
        m, keep = eng._model_desc()
        ws_bytes = int(lib.pcg_baseline_train_workspace_bytes(eng.g.desc_ref(), C.byref(m), batch))
        assert ws_bytes > 0
        ids, labels = T.batch(n, 5)
        n_batches = (n + batch - 1) // batch
        arena = GuardedArena(64 << 20, dev())
        ids_dev, lab_dev = arena.take((n,), torch.int32, name="ids"), arena.take((n,), torch.int32, name="labels")
        ids_dev.copy_(torch.from_numpy(ids.astype(np.int32)))
        lab_dev.copy_(torch.from_numpy(labels.astype(np.int32)))
        ws = arena.take((ws_bytes,), torch.uint8, name="workspace")
        out_loss = arena.take((n_batches,), name="out_loss")
        grad = arena.take((2 * E + E * K,), name="grad_out")
        state = [arena.take(shp, zero=True, name=nm) for nm, shp in (("m_enc", (E, K)), ("v_enc", (E, K)), ("m_cls", (2, E)), ("v_cls", (2, E)))]
        status = arena.take((1,), torch.int32, zero=True, name="status")
        opt = _lib.BaselineOpt(m_enc=state[0].data_ptr(), v_enc=state[1].data_ptr(), m_cls=state[2].data_ptr(), v_cls=state[3].data_ptr(),
                               first_step=1, apply=apply, hyper=eng._hyper)
        rc = lib.pcg_baseline_train(eng.g.desc_ref(), C.byref(m), C.byref(opt), ops._p(ids_dev), ops._p(lab_dev), n, batch, ops._p(ws),
                                    ws_bytes, ops._p(out_loss), ops._p(grad), ops._p(status), ops._stream(dev()))
        assert rc == _lib.PCG_OK
        torch.cuda.synchronize()
        arena.check(f"pcg_baseline_train n={n} batch={batch} apply={apply} F={F} E={E} {shape}")
        assert int(status.item()) == 0 and torch.isfinite(out_loss).all() and torch.isfinite(grad).all()
        # the same call through the engine, bit for bit
        twin = trainable(F, E, shape)
        if apply:
            assert same(twin.train_epoch(ids, labels, batch), out_loss)
            assert same(twin.enc.weight, model.enc.weight) and same(twin.optimizer_state()["v_enc"], state[1])
        else:
            loss, d_enc, d_cls = twin.loss_and_grad(ids, labels)
            assert same(loss, out_loss[0]) and same(d_cls.reshape(-1), grad[:2 * E]) and same(d_enc.reshape(-1), grad[2 * E:])
            assert not any(bool(s.any()) for s in state)
        del keep


# ---- 7. rejections ----------------------------------------------------------------------------------------------------------------
def test_rejections_launch_nothing_and_bad_values_set_the_status_bit():
    from pcgnn_amd import _lib, ops
    F, E, shape = 25, 64, "sage"
    lib = _lib.load()
    model = trainable(F, E, shape)
    eng = model.engine()
    before = state_of(model)[0]
    ids, labels = T.batch(40)
    ids_dev, lab_dev = ops._i32(ids, dev()), ops._i32(labels, dev())
    m, keep = eng._model_desc()
    ws_bytes = eng.train_workspace_bytes_of(40)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev())
    out_loss, grad = torch.full((3,), 7.0, device=dev()), torch.full((2 * E + E * F,), 7.0, device=dev())
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    o = eng._adam()
    good = dict(m_enc=o["m_enc"].data_ptr(), v_enc=o["v_enc"].data_ptr(), m_cls=o["m_cls"].data_ptr(), v_cls=o["v_cls"].data_ptr(),
                first_step=1, apply=1, hyper=eng._hyper)

    def call(model_desc=m, n=40, batch=40, nbytes=ws_bytes, **opt_over):
        opt = _lib.BaselineOpt(**dict(good, **opt_over))
        return lib.pcg_baseline_train(eng.g.desc_ref(), C.byref(model_desc), C.byref(opt), ops._p(ids_dev), ops._p(lab_dev), n, batch,
                                      ops._p(ws), nbytes, ops._p(out_loss), ops._p(grad), ops._p(status), ops._stream(dev()))

    odd = _lib.BaselineModel.from_buffer_copy(m)
    odd.emb = 40
    assert call(model_desc=odd) == _lib.PCG_E_UNSUPPORTED                           # E % 16 != 0
    assert call(n=40, batch=16, apply=0) == _lib.PCG_E_ARG                          # gradients only: one batch
    for member in ("m_enc", "v_enc", "m_cls", "v_cls"):
        assert call(**{member: None}) == _lib.PCG_E_ARG, member                     # apply without its state
    assert call(nbytes=ws_bytes - 1) == _lib.PCG_E_ARG                              # a workspace that is too small
    torch.cuda.synchronize()
    assert all(same(x, y) for x, y in zip(before, state_of(model)[0])) and int(status.item()) == 0
    assert bool((out_loss == 7.0).all()) and bool((grad == 7.0).all())
    del keep
    # host sequences are checked on the host
    for bad_ids, bad_labels in (([0, T.N], [0, 1]), ([-1, 3], [0, 1]), ([2, 3], [0, 2]), ([2, 3], [0]), ([2, 3], [-1, 0])):
        with pytest.raises(ValueError):
            model.train_step(bad_ids, bad_labels)
    with pytest.raises(ValueError):
        model.loss_and_grad([], [])
    assert model.train_epoch([], [], 16).shape == (0,)
    # device tensors are not read: the kernels clamp what they index and report; check() raises
    model.check()
    bad = ids_dev.clone()
    bad[21] = T.N + 5
    loss = model.train_step(bad, lab_dev)
    with pytest.raises(_lib.PcgnnLibraryError, match="outside the feature table"):
        model.check()
    model.check()                                                                   # (cleared)
    assert bool(torch.isfinite(loss))
    two = lab_dev.clone()
    two[21] = 2
    loss = model.train_step(ids_dev, two)
    with pytest.raises(_lib.PcgnnLibraryError, match="label outside"):
        model.check()
    assert bool(torch.isfinite(loss)) and torch.isfinite(model.enc.weight).all()
    # the row with the bad label contributes nothing: the gradient is that of the batch with its loss term dropped, over B
    keep_rows = np.arange(40) != 21
    fresh = fresh_model(F, E, shape)
    _, d_enc, d_cls = fresh.loss_and_grad(ids_dev, two)
    with pytest.raises(_lib.PcgnnLibraryError):
        fresh.check()
    _, e_enc, e_cls = fresh.loss_and_grad(ids[keep_rows], labels[keep_rows])
    np.testing.assert_allclose(d_enc.cpu().numpy() * 40, e_enc.cpu().numpy() * 39, rtol=0, atol=1e-5)
    np.testing.assert_allclose(d_cls.cpu().numpy() * 40, e_cls.cpu().numpy() * 39, rtol=0, atol=1e-5)


def test_train_step_needs_its_hyper_parameters():
    from pcgnn_amd import _lib
    model = fresh_model(25, 64, "sage")
    ids, labels = T.batch(17)
    with pytest.raises(_lib.PcgnnLibraryError, match="configure_optimizer"):
        model.train_step(ids, labels)
    model.loss_and_grad(ids, labels)                                                # (needs none)


# ---- 8. ModelHandler ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model_name", ["SAGE", "GCN"])
def test_model_handler(model_name, tmp_path):
    from pcgnn_amd import synth
    from pcgnn_amd.handler import ModelHandler
    w = synth.make_workload("mini", 1500, 16, (6000,), 0.15, seed=4)
    cfg = dict(data_name="yelp", model=model_name, seed=3, train_ratio=0.4, test_ratio=0.67, emb_size=32, lr=0.01, weight_decay=0.001,
               alpha=2, rho=0.5, epochs=2, valid_epochs=5, batch_size=256, patience=3, exp_num="0000",
               result_dir=str(tmp_path / "experimental_results"))

    def seeded(handler_cfg):
        h = ModelHandler(handler_cfg, dataset=w, device=dev())
        random.seed(77)
        torch.manual_seed(5)
        return h

    # with the key: the engine's train_epoch over the same seeded shuffles
    h = seeded(dict(cfg, baseline_fused_train=True))
    h.train()
    assert h.engine is None                                                         # no FusedPCGNN
    r = seeded(dict(cfg, baseline_fused_train=True))
    model, engine, _ = r._build()
    assert engine is None
    labels_dev = torch.from_numpy(np.asarray(r.dataset["labels"]).astype(np.int32)).to(dev())
    losses = []
    for _ in range(cfg["epochs"]):
        sampled = list(r.dataset["idx_train"])
        random.shuffle(sampled)
        ids = torch.as_tensor(np.asarray(sampled), device=dev())
        losses.append(model.train_epoch(ids, labels_dev[ids], cfg["batch_size"]))
    model.check()
    assert len(r.dataset["idx_train"]) == 600 and losses[0].shape == (3,) and model.optimizer_state()["step"] == 6
    assert same(h.model.enc.weight, model.enc.weight) and same(h.model.weight, model.weight)
    assert h.model.optimizer_state()["step"] == 6 and all(bool(torch.isfinite(l).all()) for l in losses)
    # without it: the loop as it was - model.loss + torch.optim.Adam per batch
    d = seeded(cfg)
    d.train()
    p = seeded(cfg)
    model, _, opt = p._build()
    for _ in range(cfg["epochs"]):
        sampled = list(p.dataset["idx_train"])
        random.shuffle(sampled)
        for b0 in range(0, len(sampled), cfg["batch_size"]):
            batch_nodes = sampled[b0:b0 + cfg["batch_size"]]
            opt.zero_grad()
            loss = model.loss(batch_nodes, labels_dev[torch.as_tensor(batch_nodes, device=dev())].long())
            loss.backward()
            opt.step()
    assert same(d.model.enc.weight, model.enc.weight) and same(d.model.weight, model.weight)
    assert d.model.engine()._opt is None                                             # (the engine's Adam was never made)
    # the two paths train the same model: the same steps, float32 apart
    np.testing.assert_allclose(h.model.enc.weight.detach().cpu().numpy(), model.enc.weight.detach().cpu().numpy(), rtol=0, atol=1e-4)
