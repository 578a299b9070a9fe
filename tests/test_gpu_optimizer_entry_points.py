"""The small optimizer launches of the C ABI that only the partitioned step runs, on their own: pcg_grad_reduce,
pcg_adam_apply_pending (flag 0 / 1, clear 0 / 1) and the deferred update that rides pcg_step_front_train's first launch.

Shape (F, E, R) = (25, 16, 2): 2596 parameters, the label classifier at offset 2544 - neither a multiple of the 64 parameters a
workgroup owns, so the last workgroup of every launch is ragged.  Gaussian inputs (tests/front_ref.py: opt_inputs), lr 0.01,
weight decay 5e-4, Adam's t = 1 and 7, 1 .. 9 slabs (adam_reduce_body gives each of its four waves a quarter of the slabs: 1, 2,
3 and 5 slabs leave waves without any, 4 | 5 and 8 | 9 are the quarter's edges).

Bit for bit: pcg_grad_reduce's sum is pcg_adam_step(apply = 0)'s, pcg_adam_apply_pending is pcg_adam_step(n_slabs = 1) of the
same gradient, pcg_step_front_train's update of the parameters below the classifier is pcg_adam_step's ("same arithmetic and
summation order", include/pcgnn.h).  Against float64: the sum by dense_ref.tolerance of the sequential float32 sum, the update by
adam_ref.adam_figures' bars (tests/test_front_ref_host.py asserts the inputs keep CANCEL_CAP on the CPU).

Measured on an MI355X (the FIGURE lines of -s, maximised over n_slabs and t; a fraction of the bar, <= 1 passes):
    pcg_grad_reduce          sum against float64: at most 0.07 of 8 * e_f32 + 2^-20 (n_params 2596, 1, 63, 64, 65)
    pcg_adam_apply_pending   theta 0.357  m 0.043  v 0.260   no entry excluded
    pcg_step_front_train     theta 0.354  m 0.294  v 0.270   no entry excluded (from the float64 sum of the slabs)
Every comparison that is stated bit for bit was bit-exact.
"""
import numpy as np
import pytest
import torch

from tests import adam_ref as A
from tests import dense_ref as D
from tests import front_ref as R
from tests.util import synth_graph

pytestmark = pytest.mark.gpu

F, E, NREL = R.OPT_SHAPE
HYPER = dict(lr=R.OPT_LR, betas=R.OPT_BETAS, eps=R.OPT_EPS, wd=R.OPT_WD)


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def P():
    import pcgnn_amd
    from pcgnn_amd import ops  # noqa: F401  (fails loudly if the .so is missing)
    return pcgnn_amd


class Lib:
    def __init__(self, P):
        from pcgnn_amd import _lib
        self.lib, self.ops, self._lib = _lib.load(), P.ops, _lib
        self.p, self.st = P.ops._p, P.ops._stream(dev())
        self.hyper = _lib.AdamHyper(R.OPT_LR, R.OPT_BETAS[0], R.OPT_BETAS[1], R.OPT_EPS, R.OPT_WD)
        self.n_params = int(self.lib.pcg_dense_n_params(F, E, NREL))
        self.o_clf = int(self.lib.pcg_dense_param_offset(F, E, NREL, 3, 0))

    def adam_step(self, theta, m, v, slabs, n_slabs, n_params, step, grad_out, apply):
        import ctypes as C
        self._lib.check(self.lib.pcg_adam_step(self.p(theta), self.p(m), self.p(v), self.p(slabs), n_slabs, n_params, self.p(step),
                                               C.byref(self.hyper), self.p(grad_out), apply, self.st), "pcg_adam_step")

    def grad_reduce(self, slabs, n_slabs, n_params, grad_out, flag):
        self._lib.check(self.lib.pcg_grad_reduce(self.p(slabs), n_slabs, n_params, self.p(grad_out), self.p(flag), self.st), "pcg_grad_reduce")

    def apply_pending(self, theta, m, v, grad, n_params, step, flag, clear):
        import ctypes as C
        self._lib.check(self.lib.pcg_adam_apply_pending(self.p(theta), self.p(m), self.p(v), self.p(grad), n_params, self.p(step), self.p(flag),
                                                        clear, C.byref(self.hyper), self.st), "pcg_adam_apply_pending")


@pytest.fixture(scope="module")
def L(P):
    return Lib(P)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def upload(x):
    return {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev()) for k, a in x.items()}


def slab_tensor(x):
    """the slabs on the device: [max(n_slabs, 1), n_params] (a non-NULL pointer for n_slabs = 0 too)"""
    s = x["slabs"]
    return torch.from_numpy(np.ascontiguousarray(s if s.shape[0] else np.zeros((1, s.shape[1]), np.float32))).to(dev())


def test_offsets_give_a_ragged_last_block(L):
    assert L.o_clf % 64 != 0 and L.n_params % 64 != 0
    assert (L.n_params, L.o_clf) == (R.opt_n_params(F, E, NREL), R.opt_clf_offset(F, E, NREL))


@pytest.mark.parametrize("n_slabs", [0] + R.OPT_SLABS)
def test_grad_reduce(L, n_slabs):
    worst = 0.0
    for n_params in [L.n_params] + R.OPT_SMALL_N:
        x = R.opt_inputs(n_params, n_slabs, 1)
        slabs = slab_tensor(x)
        want = torch.full((n_params + 64,), 7.0, device=dev())
        step = torch.ones(1, dtype=torch.int32, device=dev())
        L.adam_step(None, None, None, slabs, n_slabs, n_params, step, want, 0)
        got = torch.full((n_params + 64,), 7.0, device=dev())
        flag = torch.zeros(2, dtype=torch.int32, device=dev())
        L.grad_reduce(slabs, n_slabs, n_params, got, flag)
        torch.cuda.synchronize()
        assert same_bits(got, want), f"n_slabs {n_slabs} n_params {n_params}: pcg_adam_step(apply = 0)'s sum, and nothing written behind n_params"
        assert bool((got[n_params:] == 7.0).all())
        assert flag.tolist() == [1, 0], "a gradient is waiting"
        if n_slabs == 0:
            assert not bool(got[:n_params].any()), "no slabs: zeros"
            continue
        ref = R.slab_sum_f64(x["slabs"])
        e32 = D.rel_err(R.slab_sum_f32(x["slabs"]), ref)
        e = D.rel_err(got[:n_params].cpu().numpy().astype(np.float64), ref)
        print(f"  grad_reduce n_slabs {n_slabs} n_params {n_params}: e {e:.3e}  e_f32 {e32:.3e}  tolerance {D.tolerance(e32):.3e}")
        worst = max(worst, e / D.tolerance(e32))
        assert e <= D.tolerance(e32), (n_slabs, n_params, e, e32)
    print(f"FIGURE pcg_grad_reduce n_slabs={n_slabs}: of bound {worst:.2f}")


@pytest.mark.parametrize("t", R.OPT_T)
@pytest.mark.parametrize("n_slabs", R.OPT_SLABS)
def test_adam_apply_pending(L, n_slabs, t):
    n_params = L.n_params
    x = R.opt_inputs(n_params, n_slabs, t)
    d = upload({k: x[k] for k in ("theta", "m", "v")})
    slabs = slab_tensor(x)
    step = torch.full((1,), t, dtype=torch.int32, device=dev())
    grad = torch.empty(n_params, device=dev())
    flag = torch.zeros(1, dtype=torch.int32, device=dev())
    # flag 0: nothing happens (clear = 0 and 1)
    for clear in (0, 1):
        th, m, v = d["theta"].clone(), d["m"].clone(), d["v"].clone()
        L.apply_pending(th, m, v, slabs, n_params, step, flag, clear)
        torch.cuda.synchronize()
        assert same_bits(th, d["theta"]) and same_bits(m, d["m"]) and same_bits(v, d["v"]), "flag 0: unchanged"
        assert int(flag.item()) == 0
    L.grad_reduce(slabs, n_slabs, n_params, grad, flag)
    # flag 1: pcg_adam_step(slabs = grad, n_slabs = 1, apply = 1) on copies
    want = [d[k].clone() for k in ("theta", "m", "v")]
    L.adam_step(*want, grad, 1, n_params, step, None, 1)
    got = [d[k].clone() for k in ("theta", "m", "v")]
    L.apply_pending(*got, grad, n_params, step, flag, 0)
    torch.cuda.synchronize()
    assert int(flag.item()) == 1, "clear = 0 leaves the flag to the caller's next launch"
    for name, a, b in zip(("theta", "m", "v"), got, want):
        assert same_bits(a, b), f"{name}: pcg_adam_step's bits"
        assert not same_bits(a, d[name]), f"{name} moved"
    again = [d[k].clone() for k in ("theta", "m", "v")]
    L.apply_pending(*again, grad, n_params, step, flag, 1)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0, "clear = 1 leaves the flag 0"
    for a, b in zip(again, want):
        assert same_bits(a, b)
    # against float64, from the device's own gradient (the sum has its own bar, test_grad_reduce)
    fig = A.adam_figures(got, d["theta"], d["m"], d["v"], grad, t, **HYPER)
    print(f"FIGURE pcg_adam_apply_pending n_slabs={n_slabs} t={t}: theta {fig['theta']:.3f}  m {fig['m']:.3f}  v {fig['v']:.3f}  "
          f"excluded {fig['excluded']:.1e}")
    assert fig["theta"] <= 1 and fig["m"] <= 1 and fig["v"] <= 1 and fig["excluded"] <= A.CANCEL_CAP, fig


# ---- the deferred update riding pcg_step_front_train ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def front_case(P):
    n = 2000
    X, labels, csrs = synth_graph(71, n, F, (6, 20), 0.15)
    train_pos = np.flatnonzero(labels == 1)[:200]
    g = P.DeviceGraph(X, csrs, train_pos.tolist(), dev())
    rs = np.random.RandomState(72)
    nodes = rs.randint(0, n, size=77).astype(np.int32)
    nodes[0] = 7
    return g, torch.from_numpy(nodes).cuda(), torch.from_numpy(labels[nodes].astype(np.int32)).cuda()


@pytest.mark.parametrize("t", R.OPT_T)
@pytest.mark.parametrize("n_slabs", R.OPT_SLABS)
def test_step_front_train_applies_the_waiting_update(L, front_case, n_slabs, t):
    import ctypes as C
    g, nodes, lab = front_case
    lib, _lib, ops, _p = L.lib, L._lib, L.ops, L.p
    n_params, o_clf, B = L.n_params, L.o_clf, nodes.numel()
    x = R.opt_inputs(n_params, n_slabs, t)
    d = upload({k: x[k] for k in ("theta", "m", "v")})
    slabs = torch.zeros(max(n_slabs, 8), n_params, device=dev())
    slabs[:n_slabs] = torch.from_numpy(x["slabs"]).to(dev())
    step = torch.full((1,), t, dtype=torch.int32, device=dev())
    thr, rho = [0.5, 0.7], [0.5, 1.5]
    # what the update must give, and the front of the same batch without a training state
    want = [d[k].clone() for k in ("theta", "m", "v")]
    L.adam_step(*want, slabs, n_slabs, n_params, step, None, 1)
    W = d["theta"][o_clf:o_clf + 2 * F].view(2, F).contiguous()
    b = d["theta"][o_clf + 2 * F:o_clf + 2 * F + 2].contiguous()
    s0_f = torch.empty(g.n_nodes, device=dev())
    keys_f = torch.zeros(int(lib.pcg_pos_sort_capacity(g.n_pos)), dtype=torch.int64, device=dev())
    ws_f = ops.ChooseWorkspace(g, B)
    ops.step_front(g, W, b, s0_f, keys_f, nodes, lab, thr, rho, True, ws_f)
    full = ops.score_table(g, W, b)
    sorted_ref = ops.pos_sort(g, full)
    # pcg_step_front_train with the update waiting
    th, m, v = (d[k].clone() for k in ("theta", "m", "v"))
    sync = torch.zeros(int(lib.pcg_sync_words_count()), dtype=torch.int32, device=dev())
    sync[1], sync[2] = 1, n_slabs
    ws_t = ops.ChooseWorkspace(g, B)
    tarr, rarr = ops._host_arrays(g, thr, rho)
    st = _lib.TrainState(theta=_p(th), m=_p(m), v=_p(v), step_counter=_p(step), sync_words=_p(sync), slabs=_p(slabs), emb=E,
                         hyper=L.hyper)
    batch = _lib.Batch(ids=_p(nodes), labels=_p(lab), cnt=None, plan=None, B=B, inv_count=1.0 / B)
    sel = _lib.SelectWs(thresholds=tarr, rho=rarr, workspace=_p(ws_t.buf), status=_p(ws_t.status), list_capacity=ws_t.list_capacity, add_self=0)
    s0_t = torch.full((g.n_nodes,), -1.0, device=dev())
    keys_t = torch.zeros_like(keys_f)

    def front_train():
        _lib.check(lib.pcg_step_front_train(g.desc_ref(), C.byref(st), _p(s0_t), _p(keys_t), C.byref(batch), C.byref(sel), L.st),
                   "pcg_step_front_train")
        torch.cuda.synchronize()

    front_train()
    for name, a, w_, old in zip(("theta", "m", "v"), (th, m, v), want, (d["theta"], d["m"], d["v"])):
        assert same_bits(a[:o_clf], w_[:o_clf]), f"{name} [0, o_clf): pcg_adam_step's bits"
        assert same_bits(a[o_clf:], old[o_clf:]), f"{name} [o_clf, n_params): untouched"
        assert not same_bits(a[:o_clf], old[:o_clf])
    assert sync[:4].tolist() == [0, 0, n_slabs, 0], "the second launch clears sync_words[1]"
    assert int(step.item()) == t
    assert same_bits(s0_t, full) and same_bits(s0_f, full), "s0: pcg_score_table's with theta's classifier"
    half = keys_t.numel() // 2
    assert torch.equal(keys_t[:half], sorted_ref[:half]) and torch.equal(keys_f[:half], sorted_ref[:half])
    # the plan: the planned select + gather on either workspace leaves the same offsets, lists, counts and aggregates
    agg_t, cnt_t = ops.choose_aggregate(g, nodes, lab, s0_t, keys_t, thr, rho, True, ws=ws_t, planned=True)
    agg_f, cnt_f = ops.choose_aggregate(g, nodes, lab, s0_f, keys_f, thr, rho, True, ws=ws_f, planned=True)
    torch.cuda.synchronize()
    ws_t.check(); ws_f.check()
    rows = g.R * B
    begin = ws_f.view(0, torch.int64, rows + 1)
    assert torch.equal(ws_t.view(0, torch.int64, rows + 1), begin)
    total = int(begin[-1])
    assert total > 0 and torch.equal(ws_t.view(1, torch.int32, rows), ws_f.view(1, torch.int32, rows))
    assert torch.equal(ws_t.view(2, torch.int32, total), ws_f.view(2, torch.int32, total))
    assert torch.equal(cnt_t, cnt_f) and same_bits(agg_t, agg_f)
    # against float64: the device's update of the parameters below the classifier, from the float64 sum of the slabs
    g64 = torch.from_numpy(R.slab_sum_f64(x["slabs"]))[:o_clf]
    fig = A.adam_figures([a[:o_clf] for a in (th, m, v)], d["theta"][:o_clf], d["m"][:o_clf], d["v"][:o_clf], g64, t, **HYPER)
    print(f"FIGURE pcg_step_front_train n_slabs={n_slabs} t={t}: theta {fig['theta']:.3f}  m {fig['m']:.3f}  v {fig['v']:.3f}  "
          f"excluded {fig['excluded']:.1e}")
    assert fig["theta"] <= 1 and fig["m"] <= 1 and fig["v"] <= 1 and fig["excluded"] <= A.CANCEL_CAP, fig
    # a second call with nothing pending changes no parameter
    after = [a.clone() for a in (th, m, v)]
    front_train()
    for a, b_ in zip((th, m, v), after):
        assert same_bits(a, b_), "nothing pending: no parameter moves"
    assert same_bits(s0_t, full) and sync[:4].tolist() == [0, 0, n_slabs, 0]
