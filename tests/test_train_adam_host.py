"""CPU-only tests of what the training-step Adam test compares the device with (tests/train_adam_ref.py, used by
tests/test_gpu_train_adam_f64.py): the reference alone - float32 torch.optim.Adam on the float32 reference gradient, the oracle's
selection at every step's own parameters - keeps every tolerance and cap on every step of every case, with nothing left out;
and each mistake the GPU test is there to catch, planted in a float32 Adam of a few lines, takes one of its three checks
beyond ten tolerances at some step."""
import numpy as np
import pytest
import torch

from tests import adam_ref as A
from tests import dense_ref as D
from tests import train_adam_ref as T
from tests.util import PARAM_KEYS


def test_sequences_are_the_stated_ones():
    assert T.SEQUENCE == (2049, 1025, 17, 1024, 1, 2048, 65, 1023, 17, 2049) and T.SEQUENCE_LARGE == (8193, 8192, 1025, 8193)
    wgs = [(B + 1023) // 1024 for B in T.SEQUENCE]                  # the label classifier's workgroups: one per 1024 rows
    # fewer workgroups behind more (slab slots of the step before are stale), more behind fewer, and the same count again
    assert {(a, b) for a, b in zip(wgs, wgs[1:])} == {(3, 2), (2, 1), (1, 1), (1, 2), (1, 3)}
    assert [min((B + 1023) // 1024, 8) for B in T.SEQUENCE_LARGE] == [8, 8, 2, 8]      # (at most eight: slices of 1088 rows at 8193)
    assert clf_slice_weights(8193, 7, 0.0).sum() == 7 * 1088 and clf_slice_weights(2049, 1, 2.0).sum() == 2049 + 704
    assert all(max(seq) == cap for seq, cap in T.SEQUENCES.values())
    assert [s for s, q in T.CASES if q == "sequence"] == [(32, 64, 3), (25, 128, 3), (10, 16, 1), (260, 16, 1)]
    assert [s for s, q in T.CASES if q == "large"] == [(32, 64, 3), (260, 16, 1)]
    for F, _, _ in {s for s, _ in T.CASES}:
        assert (2 * F + 2 > 512) == (F == 260) == ((F + 3) // 4 * 4 > 256)


def named(flat, like, R):
    return A.unflatten(flat, like, R)


def state_of(theta, m, v, like, R):
    return dict(theta=named(theta, like, R), m=named(m, like, R), v=named(v, like, R))


@pytest.fixture(scope="module")
def runs():
    """case -> the reference's own float32 trajectory, computed once: per step dict(index, masks: the oracle's selection at the
    step's parameters and the float64 ReLU signs there; share: of ambiguous activations; figs: step_figures)"""
    out = {}
    for shape, seq in T.CASES:
        c = D.GradCase.of(shape)
        like = c.params()
        p = torch.nn.Parameter(A.flatten(like, c.R).clone())
        opt = torch.optim.Adam([p], lr=c.lr, betas=c.betas, eps=T.EPS, weight_decay=c.wd)
        m, v = torch.zeros_like(p.data), torch.zeros_like(p.data)
        steps = []
        for k, B in enumerate(T.SEQUENCES[seq][0]):
            ids, lab = T.step_batch(c, seq, k)
            theta = p.detach().clone()
            params = named(theta, like, c.R)
            index = D.sets_to_index(c.host_sets(ids, lab, params))
            r64, r32, share, _ = D.reference_pair(c, ids, lab, index, params=params)
            p.grad = A.flatten(r32["grads"], c.R).float().clone()
            opt.step()
            st = opt.state[p]
            figs = T.step_figures(c, k, state_of(theta, m, v, like, c.R),
                                  state_of(p.detach(), st["exp_avg"], st["exp_avg_sq"], like, c.R), r64, r32,
                                  tag=f"{T.case_id((shape, seq))} B={B}")
            print(f"{T.case_id((shape, seq))} step {k} B={B}: ambiguous {share:.2e} (cap {D.AMBIGUOUS_CAP:.0e})")
            m, v = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
            steps.append(dict(index=index, masks=[(t > 0).double() for t in r64["pre"]], share=share, figs=figs))
        out[shape, seq] = steps
    return out


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_reference_alone_keeps_tolerances_and_caps(runs, case):
    """float32 torch on the CPU keeps (ii) and (iii) on every step with no entry left out ((i) is then the yardstick against
    itself), and every step's batch keeps AMBIGUOUS_CAP at that step's parameters"""
    steps = runs[case]
    figs = [s["figs"] for s in steps]
    w = T.worst(figs)
    print(f"FIGURES {T.case_id(case)}: of tolerance: (ii) v {w['v']:.3f}  (iii) theta {w['theta']:.3f}  (i) of bound {w['grad']:.3f}  "
          f"left out {w['excluded']:.1e}  ambiguous {max(s['share'] for s in steps):.2e}")
    assert not T.misses(figs), f"{case}: change the salt of the batches, not the cap - {T.misses(figs)}"
    assert w["excluded"] == 0.0
    # (the cap with a third to spare here: the device's parameters differ from these in the last bits, its count may by one or two)
    assert T.AMBIGUOUS_HOST < D.AMBIGUOUS_CAP
    over = [(k, s["share"]) for k, s in enumerate(steps) if s["share"] > T.AMBIGUOUS_HOST]
    assert not over, f"{case}: ambiguous ReLU pre-activations above {T.AMBIGUOUS_HOST}: {over} - change the salt of the batches"
    assert all(s["share"] == 0.0 for s, B in zip(steps, T.SEQUENCES[case[1]][0]) if B <= 17)
    for step in figs:
        assert all(f["ratio"] in (None, 1.0) for f in step.values())       # (the yardstick against itself)


# ---------------------------------------------------------------------------------------------------------------------------
# planted mistakes: a float32 Adam in a few lines, one mistake each; the selections and masks are the correct run's
# ---------------------------------------------------------------------------------------------------------------------------
def clf_slice_weights(B, wg, times):
    """row weights that count workgroup wg's slice of the label classifier's step `times` times (slices as the select launch cuts
    them: ceil(B / 1024) workgroups, at most eight, of ceil(B / workgroups) rows rounded up to 64)"""
    n_wg = min((B + 1023) // 1024, 8)
    per = (-(-B // n_wg) + 63) // 64 * 64
    w = np.ones(B)
    w[wg * per:min((wg + 1) * per, B)] = times
    return w


def planted_run(shape, fixed, t_of=lambda k: k + 1, eps_inside=False, decoupled=False, beta2=None, v_unwritten_from=None,
                stale_p=False, slice_times=None):
    """SEQUENCE with one mistake planted: step_figures of every step, the reference taken at the planted run's own theta_k - as
    the GPU test takes it at the device's"""
    c = D.GradCase.of(shape)
    like = c.params()
    R, b1, b2 = c.R, c.betas[0], c.betas[1] if beta2 is None else beta2
    theta = A.flatten(like, R).clone()
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    at, clf = 0, torch.zeros_like(theta, dtype=torch.bool)
    for name in PARAM_KEYS(R):
        clf[at:at + like[name].numel()] = name in T.CLF
        at += like[name].numel()
    clf_at = int(clf.nonzero()[0])                     # (the classifier's weight and bias are adjacent in PARAM_KEYS' order)
    theta_prev, figs = theta.clone(), []
    for k, B in enumerate(T.SEQUENCE):
        ids, lab = T.step_batch(c, "sequence", k)
        params = named(theta, like, R)
        args = (c.X, ids, lab, fixed[k]["index"], params, c.alpha)
        r64 = D.dense_ref(*args, dtype=torch.float64, masks=fixed[k]["masks"])
        r32 = D.dense_ref(*args, dtype=torch.float32, masks=fixed[k]["masks"])
        g = A.flatten(r32["grads"], R).float()
        if slice_times is not None and B == 2049:      # the classifier's gradient with workgroup 1's slice missing / twice
            w = clf_slice_weights(B, 1, slice_times)
            bad = D.dense_ref(*args, dtype=torch.float32, masks=fixed[k]["masks"], row_weight=w)
            g = torch.where(clf, A.flatten(bad["grads"], R).float(), g)
        p = torch.where(clf, theta_prev, theta) if stale_p else theta
        t = t_of(k)
        # ---- float32 Adam (torch.optim.Adam's arithmetic) with the mistake ----
        gt = g if decoupled else g + c.wd * p
        m1 = b1 * m + (1 - b1) * gt
        v1 = b2 * v + (1 - b2) * gt * gt
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        denom = (v1 / bc2 + T.EPS).sqrt() if eps_inside else v1.sqrt() / bc2 ** 0.5 + T.EPS
        new = p - (c.lr / bc1) * (m1 / denom) - (c.lr * c.wd * p if decoupled else 0.0)
        if v_unwritten_from is not None:
            v1[clf_at + v_unwritten_from:clf_at + int(clf.sum())] = v[clf_at + v_unwritten_from:clf_at + int(clf.sum())]
        figs.append(T.step_figures(c, k, state_of(theta, m, v, like, R), state_of(new, m1, v1, like, R), r64, r32,
                                   tag=f"planted B={B}"))
        theta_prev, theta, m, v = theta, new, m1, v1
    return figs


# what -> (shape, planted_run's arguments, the check that must catch it: grad = (i), v = (ii), theta = (iii))
PLANTED = {
    "correct": ((32, 64, 3), dict(), None),
    "t one ahead from step 2 on": ((32, 64, 3), dict(t_of=lambda k: k + 1 + (k >= 1)), "theta"),
    "t one behind from step 2 on": ((32, 64, 3), dict(t_of=lambda k: k + 1 - (k >= 1)), "theta"),
    "t frozen at 1": ((32, 64, 3), dict(t_of=lambda k: 1), "theta"),
    "eps inside the square root": ((32, 64, 3), dict(eps_inside=True), "theta"),
    "decoupled weight decay": ((32, 64, 3), dict(decoupled=True), "grad"),
    "beta2 taken as beta1": ((32, 64, 3), dict(beta2=D.GradCase.betas[0]), "v"),
    "v unwritten from the classifier's entry 512 on": ((260, 16, 1), dict(v_unwritten_from=512), "v"),
    "classifier stepped from the parameters of the step before": ((32, 64, 3), dict(stale_p=True), "theta"),
    "a workgroup's slice missing from the classifier's gradient": ((32, 64, 3), dict(slice_times=0.0), "grad"),
    "a workgroup's slice counted twice": ((32, 64, 3), dict(slice_times=2.0), "grad"),
}


@pytest.mark.parametrize("what", list(PLANTED))
def test_planted_mistake_is_ten_tolerances_away(runs, what):
    """each mistake takes the named check beyond ten of its tolerances at some step of SEQUENCE (the first such step is
    printed); the same few lines without a mistake keep every tolerance"""
    shape, kwargs, by = PLANTED[what]
    figs = planted_run(shape, runs[shape, "sequence"], **kwargs)
    if by is None:
        assert not T.misses(figs), T.misses(figs)
        return
    w = T.worst(figs)
    first = next(((k, name) for k, step in enumerate(figs) for name, f in step.items() if f[by] > 10.0), (0, "nothing"))
    print(f"PLANTED {what}: worst of tolerance (i) {w['grad']:.1f}  (ii) v {w['v']:.1f}  (iii) theta {w['theta']:.1f}; "
          f"caught by {by} first at step {first[0]} (B {T.SEQUENCE[first[0]]}) in {first[1]}")
    assert w[by] > 10.0
    touched = T.CLF if kwargs.keys() & {"v_unwritten_from", "stale_p", "slice_times"} else PARAM_KEYS(shape[2])
    for step in figs:                                  # (a mistake in the classifier's step leaves the other checks alone)
        for name, f in step.items():
            assert name in touched or max(f["grad"], f["v"], f["theta"]) <= 1.0, (what, name, f)
