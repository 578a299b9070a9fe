"""CPU-only tests of what the partitioned training test compares the device with (tests/adam_ref.py, used by
tests/test_gpu_dist_train_f64.py): ``adam_ref`` is torch.optim.Adam; the mistakes that test is there to catch each move the
parameters after the second step by more than ten of its tolerances; and the reference alone - float32 torch.optim.Adam on the
float32 reference gradient - keeps those tolerances and the caps on every step of every case."""
import numpy as np
import pytest
import torch

from tests import adam_ref as A
from tests import dense_ref as D
from tests.util import PARAM_KEYS

CLF = ("inter1.label_clf.weight", "inter1.label_clf.bias")


def test_adam_ref_is_torch_adam_in_float64():
    gen = torch.Generator().manual_seed(3)
    for lr, wd, betas, eps in ((0.01, 0.001, (0.9, 0.999), 1e-8), (0.005, 0.0, (0.8, 0.99), 1e-6), (0.02, 0.05, (0.9, 0.999), 1e-8)):
        p = torch.nn.Parameter((torch.randn(4099, generator=gen) * 0.1).double())
        opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps, weight_decay=wd)
        theta, m, v = p.detach().clone(), torch.zeros(4099).double(), torch.zeros(4099).double()
        for t in range(1, 5):
            g = (torch.randn(4099, generator=gen) * 10.0 ** -(t % 3)).double()
            if t == 3:
                g[::7] = 0.0
            p.grad = g.clone()
            opt.step()
            theta, m, v = A.adam_ref(theta, m, v, g, t, lr, betas, eps, wd)
            st = opt.state[p]
            for what, got, want in (("theta", theta, p.detach()), ("m", m, st["exp_avg"]), ("v", v, st["exp_avg_sq"])):
                assert D.rel_err(got, want) <= 1e-12, (what, t, lr)


def test_global_batch_is_rank_order():
    ids, lab = A.global_batch([torch.tensor([5, 3], dtype=torch.int32), np.array([9, 1])], [np.array([1, 0]), torch.tensor([0, 0])])
    assert ids.tolist() == [5, 3, 9, 1] and lab.tolist() == [1, 0, 0, 0] and ids.dtype == np.int64
    assert A.STEPS == 2 * [(0, 0, 129), (0, 129, 129), (0, 258, 129), (0, 387, 17), (1, 0, 129), (1, 129, 17)]


@pytest.fixture(scope="module")
def cases():
    return {(shape, world): A.DistCase(shape, world) for shape in A.CASES for world in A.WORLDS}


def test_cases_keep_the_shape_limits(cases):
    for (shape, world), c in cases.items():
        assert c.n <= 8000 and len(c.train_pos) < 16384 and len(c.csr) == 3 and c.X.shape == (c.n, shape[0])
        assert all(p.n_local > 0 for p in c.parts) and c.parts[-1].hi == c.n
        for k in range(len(A.STEPS)):
            ids, lab = c.step_batch(k)
            assert ids.size == world * A.STEPS[k][2] and set(lab.tolist()) == {0, 1}      # (both classes in every batch)


def two_steps(c, fixed, t_shift=0, decoupled=False, stale_clf=False, grad_scale=1.0, row_twice=False):
    """theta after steps 1 and 2 of the case in float64 (per parameter), with one planted mistake.  The selections and ReLU
    masks are `fixed` - per step dict(index, masks) of the correct run, the reference's own -, so only the planted arithmetic
    differs."""
    p0 = {k: v.double() for k, v in c.params().items()}
    theta, like = A.flatten(p0, c.R), p0
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    at, clf = 0, torch.zeros_like(theta, dtype=torch.bool)
    for k in PARAM_KEYS(c.R):
        clf[at:at + like[k].numel()] = k in CLF
        at += like[k].numel()
    for step in range(2):
        ids, lab = c.step_batch(step)
        ref = fixed[step]
        params = A.unflatten(theta, like, c.R) if step else p0
        w = None
        if row_twice and step == 1:
            w = np.ones(ids.size)
            w[ids.size - 1] = 2.0                      # the last row of the global batch (the last rank's single-row tile)
        g = D.dense_ref(c.X, ids, lab, ref["index"], params, c.alpha, masks=ref["masks"], row_weight=w)["grads"]
        g = A.flatten(g, c.R) * grad_scale
        m_in, v_in = m, v
        if stale_clf and step == 1:                    # the label classifier's m, v as of one step earlier (zero)
            m_in, v_in = torch.where(clf, torch.zeros_like(m), m), torch.where(clf, torch.zeros_like(v), v)
        wd = 0.0 if decoupled else c.wd
        new, m, v = A.adam_ref(theta, m_in, v_in, g, step + 1 + t_shift, c.lr, c.betas, c.eps, wd)
        theta = new - c.lr * c.wd * theta if decoupled else new            # (AdamW's decay)
    return A.unflatten(theta, like, c.R)


@pytest.fixture(scope="module")
def correct(cases):
    """per case: (the correct float64 run's selections and masks of steps 1 and 2 - the second at the float64 theta after the
    first -, its theta after step 2)"""
    out = {}
    for key, c in cases.items():
        fixed = []
        theta = {k: v.double() for k, v in c.params().items()}
        for step in range(2):
            ids, lab = c.step_batch(step)
            index = D.sets_to_index(c.host_sets(ids, lab, {k: v.float() for k, v in theta.items()}))
            r64, _, _, _ = D.reference_pair(c, ids, lab, index, params=theta)
            fixed.append(dict(index=index, masks=[(t > 0).double() for t in r64["pre"]]))
            if step == 0:
                flat, _, _ = A.adam_ref(A.flatten(theta, c.R), 0.0 * A.flatten(theta, c.R), 0.0 * A.flatten(theta, c.R),
                                        A.flatten(r64["grads"], c.R), 1, c.lr, c.betas, c.eps, c.wd)
                theta = A.unflatten(flat, theta, c.R)
        out[key] = (fixed, two_steps(c, fixed))
    return out


PLANTED = {
    "t off by one": (dict(t_shift=1), None),
    "decoupled weight decay": (dict(decoupled=True), None),
    "classifier m, v one step old": (dict(stale_clf=True), CLF),
    "loss / B instead of / (B world)": (dict(grad_scale=2.0), None),
    "a batch row counted twice": (dict(row_twice=True), None),
}


@pytest.mark.parametrize("what", list(PLANTED))
def test_planted_mistake_is_ten_tolerances_away(cases, correct, what):
    """every planted mistake moves theta after step 2 (its largest change over the parameters the mistake touches) by more than
    10 x (lr * 2e-5), the tolerance the GPU test holds theta to.  That is a statement about theta as a whole, not about every
    tensor - the figures are printed per parameter tensor, and two of the mistakes are NOT caught tensor by tensor through theta:
    Adam's update is nearly invariant to the gradient's scale (only the weight decay term and eps see it), so a wrong loss scale
    moves the label classifier's two biases by less than one tolerance; and a row counted twice in a batch of 129 or 258 moves
    some trunk tensors by fewer than ten (the gnn classifier's `weight` by four at (25, 128, 3), world 2), the case passing on
    the label classifier's weight.  For both, what holds every tensor is the GPU test's direct comparison of the all-reduced
    gradient with float64 (2c; tests/test_dense_ref_host.py: one row wrong moves every tensor's gradient by ten of ITS
    tolerances), not its check of Adam's arithmetic (2b)."""
    kwargs, touched = PLANTED[what]
    short = []
    for (shape, world), c in cases.items():
        if "world" in what and world != 2:           # (the planted scale is 2 = the world size)
            continue
        fixed, good = correct[shape, world]
        bad = two_steps(c, fixed, **kwargs)
        tol, most = c.lr * A.THETA_ATOL_PER_LR, 0.0
        for k in PARAM_KEYS(c.R):
            if touched is not None and k not in touched:
                assert torch.equal(bad[k], good[k]), k
                continue
            moved = float((bad[k] - good[k]).abs().max())
            most = max(most, moved)
            print(f"{shape} world {world} {what:32s} {k:28s} moved {moved:.3e}  tolerance {tol:.3e}  x{moved / tol:.1f}")
        if not most > 10 * tol:
            short.append((shape, world, what, most, tol))
    assert not short, short


@pytest.mark.parametrize("world", A.WORLDS)
@pytest.mark.parametrize("shape", list(A.CASES))
def test_reference_alone_keeps_tolerances_and_caps(cases, shape, world):
    """Every step with the reference alone: float32 torch.optim.Adam on the float32 reference's gradient (the oracle's
    selection at every step's own parameters) against adam_ref from the same float32 inputs keeps the Adam tolerances; at most
    CANCEL_CAP of a step's parameters are left out of theta's comparison; at most AMBIGUOUS_CAP of a batch's activations are
    ambiguous."""
    c = cases[shape, world]
    like = c.params()
    p = torch.nn.Parameter(A.flatten(like, c.R).clone())
    opt = torch.optim.Adam([p], lr=c.lr, betas=c.betas, eps=c.eps, weight_decay=c.wd)
    m, v = torch.zeros_like(p.data), torch.zeros_like(p.data)
    bad = []
    for k in range(len(A.STEPS)):
        ids, lab = c.step_batch(k)
        theta = p.detach().clone()
        params = A.unflatten(theta, like, c.R)
        _, r32, share, _ = D.reference_pair(c, ids, lab, c.host_sets(ids, lab, params), params=params)
        g = A.flatten(r32["grads"], c.R).float()
        p.grad = g.clone()
        opt.step()
        st = opt.state[p]
        fig = A.adam_figures((p.detach(), st["exp_avg"], st["exp_avg_sq"]), theta, m, v, g, k + 1, c.lr, c.betas, c.eps, c.wd)
        m, v = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
        print(f"{shape} world {world} step {k} (B {A.STEPS[k][2]}): ambiguous {share:.2e}  of tolerance: theta {fig['theta']:.2f} "
              f"m {fig['m']:.2f} v {fig['v']:.2f}  excluded {fig['excluded']:.2e}")
        if share > D.AMBIGUOUS_CAP or fig["excluded"] > A.CANCEL_CAP or max(fig["theta"], fig["m"], fig["v"]) > 1.0:
            bad.append((k, share, fig))
    assert not bad, f"{shape} world {world}: change the seed in adam_ref.CASES - {bad}"
