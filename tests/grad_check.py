"""What the GPU gradient tests share (tests/test_gpu_grad_f64.py, tests/test_gpu_dist_train_f64.py, tests/train_adam_ref.py): the tally that prints every
figure before anything is asserted, the flat-buffer -> per-parameter views, and the first-moment check (the gradient a training
step took, recovered from Adam's first moment, with float32 torch.optim.Adam on the float32 reference as its yardstick)."""
import types

import torch

from tests import dense_ref as D
from tests.util import PARAM_KEYS


class Tally:
    """every figure is printed before anything is asserted; the misses are asserted together at the end of the test"""

    def __init__(self, tag):
        self.tag, self.misses, self.ratio, self.of_bound = tag, [], 0.0, 0.0

    def check(self, what, got, ref64, ref32):
        e_k, e_32 = D.rel_err(got, ref64), D.rel_err(ref32, ref64)
        tol = D.tolerance(e_32)
        if e_32 >= 2.0 ** -24:
            self.ratio = max(self.ratio, e_k / e_32)
        self.of_bound = max(self.of_bound, e_k / tol)
        print(f"{self.tag} {what}: e_kernel {e_k:.3e}  e_f32 {e_32:.3e}  bound {tol:.3e}" + ("" if e_k <= tol else "  MISS"))
        if not e_k <= tol:
            self.misses.append((what, e_k, e_32, tol))

    def done(self):
        print(f"RATIO {self.tag}: ratio {self.ratio:.2f}  of bound {self.of_bound:.2f}")
        assert not self.misses, self.misses


def by_name(fz, flat):
    """a flat [n_params] tensor in theta's layout -> per-parameter tensors under the state-dict names"""
    return {k: flat[v.storage_offset():v.storage_offset() + v.numel()].view(v.shape) for k, v in fz.views.items()}


def dist_views(d):
    """What by_name needs of an engine, for a DistributedPCGNN (which keeps no ``views``): the state-dict names -> views into its
    flat theta, placed by pcg_dense_param_offset (which: 0 the gnn classifier, 1 the inter-relation weight, 2 a relation's weight,
    3 / 4 the label classifier's weight / bias).  Returns an object with that ``views`` dict."""
    F, E, R = d.F, d.E, d.R
    spec = [("weight", 0, 0, (2, E)), ("inter1.weight", 1, 0, (F + R * E, E)), ("inter1.label_clf.weight", 3, 0, (2, F)),
            ("inter1.label_clf.bias", 4, 0, (2,))] + [(f"inter1.intra_agg{r + 1}.weight", 2, r, (2 * F, E)) for r in range(R)]
    views, total = {}, 0
    for name, which, rel, shape in spec:
        off = int(d.lib.pcg_dense_param_offset(F, E, R, which, rel))
        n = int(torch.Size(shape).numel())
        views[name] = d.theta[off:off + n].view(shape)
        total += n
    assert total == d.n_params and d.theta.storage_offset() == 0, "the names cover the flat buffer"
    return types.SimpleNamespace(views=views)


def adam_first_moment_f32(theta_old, grad32, c, state=None):
    """float32 torch.optim.Adam on the float32 reference's gradient: the first moment after the step (state: (m, v) of one
    step taken before it)"""
    p = torch.nn.Parameter(theta_old.detach().cpu().float().clone())
    p.grad = grad32.float().clone()
    opt = torch.optim.Adam([p], lr=c.lr, weight_decay=c.wd, betas=c.betas)
    if state is not None:
        opt.state[p] = {"step": torch.tensor(1.0), "exp_avg": state[0].detach().cpu().clone(), "exp_avg_sq": state[1].detach().cpu().clone()}
    opt.step()
    return opt.state[p]["exp_avg"]


def recovered_pair(c, m_new, theta_old, grad32, state=None):
    """One parameter: (the gradient the step took, recovered from its first moment m_new; the yardstick - the float32
    reference's gradient sent through float32 torch.optim.Adam and the same recovery).  state: the parameter's (m, v) before."""
    mo = None if state is None else state[0]
    m32 = adam_first_moment_f32(theta_old, grad32, c, state)
    return D.recover_grad(m_new, theta_old, c.betas[0], c.wd, mo), D.recover_grad(m32, theta_old, c.betas[0], c.wd, mo)


def check_first_moment(tally, c, fz, what, m_new, theta_old, r64, r32, state=None):
    """the gradient the step took, recovered from Adam's first moment, per parameter; the yardstick goes the same way"""
    th, mn = by_name(fz, theta_old), by_name(fz, m_new)
    m_old = None if state is None else by_name(fz, state[0])
    v_old = None if state is None else by_name(fz, state[1])
    for k in PARAM_KEYS(c.R):
        g_dev, g_32 = recovered_pair(c, mn[k], th[k], r32["grads"][k], None if state is None else (m_old[k], v_old[k]))
        tally.check(f"{what} grad {k}", g_dev, r64["grads"][k], g_32)
