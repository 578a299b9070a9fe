"""What holds the built-in training step's Adam (FusedPCGNN.train_step: the label classifier stepped inside the select launch,
every other parameter per weight-gradient tile in the next gather launch or in the flush) to float64 at every step of a sequence:
shared by tests/test_train_adam_host.py (CPU) and tests/test_gpu_train_adam_f64.py (GPU).

The step never materialises its gradient, so the gradient it took is recovered from the first moment.  With theta_k, m_k, v_k
and theta_{k+1}, m_{k+1}, v_{k+1} the float32 state before and after step k (0-based; Adam's t = k + 1):

    g_rec = dense_ref.recover_grad(m_{k+1}, theta_k, beta1, wd, m_k)                      (float64)
    ref   = adam_ref.adam_ref(theta_k, m_k, v_k, g_rec, k + 1, lr, betas, eps, wd)       (float64)

ref's m is m_{k+1} by construction; the information is in
  (i)   g_rec against the float64 gradient of dense_ref at theta_k: e_kernel <= 8 * e_f32 + 2^-20, e_f32 the float32 reference's
        gradient sent through float32 torch.optim.Adam and the same recovery (grad_check.recovered_pair, the rule of
        grad_check.check_first_moment);
  (ii)  v_{k+1} against ref's within adam_ref.V_TOL;
  (iii) theta_{k+1} against ref's within lr * adam_ref.THETA_ATOL_PER_LR - the tolerances of test_adam_step_matches_torch_adam.
The first moment in (iii) is the step's own, so theta depends on g_rec only through v: the cancellation of g + wd * theta that
the custom-loss test leaves entries out for does not reach it, and ``step_figures`` leaves nothing out unless it is asked to
(``exclude_cancelled``; no case needs it - tests/test_train_adam_host.py asserts that with the reference alone).
"""
import torch

from tests import adam_ref as A
from tests import dense_ref as D
from tests.grad_check import recovered_pair
from tests.util import PARAM_KEYS

EPS = 1e-8                                # FusedPCGNN's default; GradCase carries every other hyper-parameter
# batch sizes of the steps, in order; batches are GradCase.batch(B, salt=step) (step_batch; SALT below)
# max_batch 2049: 3, 2, 1, 1, 1, 2, 1, 1, 1, 3 classifier workgroups - fewer behind more (the slab slots and the ticket of the
# step before), more behind fewer; 1 and 17 rows in buffers sized for 2049; t runs to 10, where 1 - 0.999^t is still ~1e-2
SEQUENCE = (2049, 1025, 17, 1024, 1, 2048, 65, 1023, 17, 2049)
# max_batch 8193: eight classifier workgroups with slices of 1088 rows (ids and labels staged in two blocks, the last slice
# short), eight full slices of 1024, two workgroups, eight again
SEQUENCE_LARGE = (8193, 8192, 1025, 8193)
SEQUENCES = {"sequence": (SEQUENCE, 2049), "large": (SEQUENCE_LARGE, 8193)}     # name -> (batch sizes, the engine's max_batch)
# (F, E, R): the two fixed-shape kernels, the run-time shape, and stride 260 - clf_step_body<2, 2>, 2F + 2 = 522 > 512 threads'
# worth of classifier parameters, gather_train_kernel<2> riders
CASES = ([(s, "sequence") for s in ((32, 64, 3), (25, 128, 3), (10, 16, 1), (260, 16, 1))]
         + [(s, "large") for s in ((32, 64, 3), (260, 16, 1))])
# case -> what is added to the step number in the batches' salt (default 0): on the reference's own trajectory every step then
# keeps dense_ref.AMBIGUOUS_CAP with a third to spare, no activation of a batch of 1 or 17 rows - where one is above the cap -
# is ambiguous, and nothing is beyond a tolerance (tests/test_train_adam_host.py asserts all three)
SALT = {((32, 64, 3), "sequence"): 300, ((260, 16, 1), "sequence"): 200}
AMBIGUOUS_HOST = D.AMBIGUOUS_CAP * 2 / 3
CLF = ("inter1.label_clf.weight", "inter1.label_clf.bias")


def case_id(case):
    (F, E, R), seq = case
    return f"{F}-{E}-{R}-{seq}"


def step_batch(c, seq, k):
    """(ids, labels) of step k of a sequence: int64 numpy"""
    return c.batch(SEQUENCES[seq][0][k], salt=SALT.get(((c.f, c.emb, c.R), seq), 0) + k)


def step_figures(c, k, before, after, r64, r32, tag="", exclude_cancelled=False):
    """Step k (0-based) of a sequence.  before / after: dicts theta, m, v of per-parameter float32 tensors under the state-dict
    names (the state the step found and left); r64 / r32: dense_ref at ``before``'s theta in float64 / float32.
    Returns name -> dict(grad, v, theta: (i), (ii), (iii) as fractions of their tolerances - <= 1 passes -, ratio: (i)'s
    e_kernel / e_f32 or None where the float32 run is exact, excluded: the share of the parameter's entries left out of theta's
    comparison).  Every figure is printed."""
    out = {}
    for name in PARAM_KEYS(c.R):
        th, m, v = before["theta"][name], before["m"][name], before["v"][name]
        g_rec, g_32 = recovered_pair(c, after["m"][name], th, r32["grads"][name], (m, v))
        e_k, e_32 = D.rel_err(g_rec, r64["grads"][name]), D.rel_err(g_32, r64["grads"][name])
        ref = A.adam_ref(th, m, v, g_rec, k + 1, c.lr, c.betas, EPS, c.wd)
        err_th = (after["theta"][name].detach().cpu().double() - ref[0]).abs()
        err_v = (after["v"][name].detach().cpu().double() - ref[2]).abs()
        assert float((after["m"][name].detach().cpu().double() - ref[1]).abs().max()) <= 1e-12, "ref's m is the step's own"
        keep = ~A.cancelled(th, g_rec, c.wd) if exclude_cancelled else torch.ones_like(err_th, dtype=torch.bool)
        fig = dict(grad=e_k / D.tolerance(e_32), ratio=e_k / e_32 if e_32 >= 2.0 ** -24 else None,
                   v=float((err_v / (A.V_TOL[1] + A.V_TOL[0] * ref[2].abs())).max()),
                   theta=float((err_th[keep] / (c.lr * A.THETA_ATOL_PER_LR)).max()) if bool(keep.any()) else 0.0,
                   excluded=1.0 - float(keep.double().mean()))
        print(f"{tag} step {k} {name:28s} (i) e_kernel {e_k:.3e} e_f32 {e_32:.3e} of bound {fig['grad']:.3f} | of tolerance: "
              f"(ii) v {fig['v']:.3f}  (iii) theta {fig['theta']:.3f}  left out {fig['excluded']:.1e}"
              + ("" if max(fig["grad"], fig["v"], fig["theta"]) <= 1.0 else "  MISS"))
        out[name] = fig
    return out


def worst(figs):
    """the maxima of step_figures' results (a list over the steps) over steps and parameters: dict(grad, ratio, v, theta, excluded)"""
    every = [f for step in figs for f in step.values()]
    out = {key: max(f[key] for f in every) for key in ("grad", "v", "theta", "excluded")}
    out["ratio"] = max((f["ratio"] for f in every if f["ratio"] is not None), default=0.0)
    return out


def misses(figs):
    """(step, name, figures) of everything beyond a tolerance or the exclusion cap"""
    return [(k, name, f) for k, step in enumerate(figs) for name, f in step.items()
            if not (max(f["grad"], f["v"], f["theta"]) <= 1.0 and f["excluded"] <= A.CANCEL_CAP)]
