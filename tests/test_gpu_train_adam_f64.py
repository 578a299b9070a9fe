"""The built-in training step's Adam against float64 at every step of a sequence.  Run with ``pytest -m gpu`` on an MI355X.

``FusedPCGNN.train_step`` - and everything held bit-identical to it: the pipelined step, the classifier-two-ahead step, the
epoch graphs - updates its parameters through three statements of Adam of its own, none of them ``pcg_adam_step``: the label
classifier in ``clf_step_body`` (csrc/select.hip: one to eight workgroups of the select launch, its own forward, cross-entropy
gradient and Adam; above 1024 rows per-workgroup gradients through slab slots and a ticket; a second turn of its parameter loop
when 2F + 2 > 512; two float4 chunks per lane for strides above 256; slices of more than 1024 rows staged block by block), every
other parameter per 16 x 16 tile in ``wgrad_adam_body`` (csrc/wgrad.h: riders of the NEXT step's gather launch, or
``pcg_adam_flush``), and the flush paths.  Here every step of a sequence is held to the float64 statement of torch.optim.Adam
(tests/adam_ref.py) through the gradient recovered from the first moment - tests/train_adam_ref.py: (i) that gradient against
float64, (ii) v, (iii) theta, each for every parameter at every step.

Sequences (train_adam_ref.py): ten steps of 2049, 1025, 17, 1024, 1, 2048, 65, 1023, 17, 2049 rows on an engine of max_batch 2049
(3, 2, 1, 1, 1, 2, 1, 1, 1, 3 classifier workgroups; t to 10) for shapes (32, 64, 3), (25, 128, 3), (10, 16, 1), (260, 16, 1); four
steps of 8193, 8192, 1025, 8193 on an engine of max_batch 8193 (eight classifier workgroups with slices of 1088 rows, the last one
short, then of 1024; two; eight again) for (32, 64, 3) and (260, 16, 1).

Two engines per case.  A runs the sequence as the product does: train_step(defer=True) for every step - each update rides in the
next step's gather launch - and one flush() at the end.  B flushes and synchronises after every step and keeps theta_k, m_k, v_k,
the device's chosen sets at theta_k and the step's ReLU masks, loss and logits.

  3a  every step of B: step_counter == k + 1; clf_next equals theta's label classifier bit for bit; at most 1e-4 of the
      activations ambiguous and no ReLU mask wrong outside that band (dense_ref.py); then, per parameter,
        (i)   the recovered gradient within e_kernel <= 8 * e_f32 + 2^-20 of dense_ref's in float64 at theta_k (e_f32: the
              float32 reference through float32 torch.optim.Adam and the same recovery - the rule of test_gpu_grad_f64.py),
        (ii)  v_{k+1} within rtol 5e-5, atol 1e-12 and
        (iii) theta_{k+1} within lr * 2e-5 of adam_ref(theta_k, m_k, v_k, recovered gradient, t = k + 1) - the tolerances of
              test_adam_step_matches_torch_adam, with no entry left out;
      the loss and the logits within the same rule as (i).
  3b  A and B end bit-identical in theta, m, v, clf_next and the step counter (the sequence's length); check() passes on both.

No bar is taken from the device's output; what the reference alone keeps, and which check catches which planted mistake (Adam's
t off by one or frozen, eps inside the root, decoupled decay, beta2 = beta1, v unwritten from the classifier's entry 512 on, a
stale classifier, a workgroup's slice missing or twice): tests/test_train_adam_host.py.

Measured on an MI355X (profiles/r21/train_adam_f64_ratios.txt): the maximum over the steps and the parameters of (ii) and (iii)
as fractions of their tolerances, of (i)'s `ratio` = e_kernel / e_f32 (entries with e_f32 >= 2^-24) and `of bound` =
e_kernel / (8 * e_f32 + 2^-20) - loss and logits included -, of the share of entries left out and of ambiguous activations:

    shape (F, E, R)  sequence         | (ii) v  (iii) theta | (i) ratio  of bound | left out  ambiguous
    (32, 64, 3)      ten steps        | 0.270   0.462       | 5.93       0.29     | 0         2.9e-5
    (25, 128, 3)     ten steps        | 0.272   0.454       | 4.20       0.28     | 0         4.2e-5
    (10, 16, 1)      ten steps        | 0.270   0.511       | 4.26       0.29     | 0         0
    (260, 16, 1)     ten steps        | 0.270   0.524       | 3.19       0.23     | 0         4.6e-5
    (32, 64, 3)      four, to 8193    | 0.270   0.465       | 3.14       0.18     | 0         4.2e-5
    (260, 16, 1)     four, to 8193    | 0.269   0.502       | 4.53       0.41     | 0         5.0e-5

3b held bit for bit in every case.  v's quarter of its tolerance is the float32 constant 1 - 0.999f against 0.001 (1.3e-5
relative, rtol 5e-5), as on the partitioned path, where theta's figure is the same half too, at every shape (the reference alone -
float32 torch on the CPU - has 0.006 and 0.15: tests/test_train_adam_host.py).  The largest (i) ratios are the label classifier's
(5.93: its two biases at step 0, e_kernel 3.8e-7).  From the second step on the recovery subtracts beta1 m_k, which raises
e_kernel and e_f32 alike: to at most 8.2e-6 and 5.7e-6 of a tensor's largest element.  No bug was found: the three statements of
Adam agree with torch.optim.Adam at every step and size here.
"""
import numpy as np
import pytest
import torch

from tests import adam_ref as A
from tests import dense_ref as D
from tests import train_adam_ref as T
from tests.grad_check import Tally, by_name

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import pcgnn_amd
    from pcgnn_amd import ops  # noqa: F401  (fails loudly if the .so is missing)
    return pcgnn_amd


def dev():
    return torch.device("cuda", 0)


def engine(P, c, max_batch):
    """test_gpu_grad_f64.engine with the sequence's max_batch"""
    from pcgnn_amd.fused import FusedPCGNN
    from tests.util import build_model
    m = build_model(P, c, c.rho, graph=P.DeviceGraph(c.X, c.csr, c.train_pos, dev()))
    fz = FusedPCGNN(m, c.lr, c.wd, betas=c.betas, max_batch=max_batch)
    assert fz.eps == T.EPS and fz.maxB == max_batch
    return m, fz


def on_dev(ids, lab):
    return torch.from_numpy(ids.astype(np.int32)).to(dev()), torch.from_numpy(lab.astype(np.int32)).to(dev())


def state(fz):
    """theta, m, v per parameter (clones) and the flat clones"""
    torch.cuda.synchronize()
    flat = dict(theta=fz.theta.clone(), m=fz.m.clone(), v=fz.v.clone())
    return {k: {n: t.cpu() for n, t in by_name(fz, x).items()} for k, x in flat.items()}, flat


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_train_step_adam_against_float64(P, case):
    shape, seq = case
    sizes, max_batch = T.SEQUENCES[seq]
    tag = T.case_id(case)
    c = D.GradCase.of(shape)
    (_, fa), (mb, fb) = engine(P, c, max_batch), engine(P, c, max_batch)
    batches = [T.step_batch(c, seq, k) for k in range(len(sizes))]

    # ---- A: as the product runs it ----
    for ids, lab in batches:
        fa.train_step(*on_dev(ids, lab), defer=True)
    fa.flush()

    # ---- B: a flush after every step; 3a ----
    tally, figs, shares, problems = Tally(tag), [], [], []
    before, _ = state(fb)
    for k, (ids, lab) in enumerate(batches):
        B = ids.size
        d = on_dev(ids, lab)
        sets = mb.inter1.chosen_sets(*d, True)                 # (the device's selection with theta_k's classifier)
        fb.train_step(*d, defer=True)
        fb.flush()
        after, flat = state(fb)
        if int(fb.step_counter.item()) != k + 1:
            problems.append(f"step counter {int(fb.step_counter.item())} after step {k}")
        if not torch.equal(fb.clf_next, flat["theta"][fb.n_rest:]):
            problems.append(f"step {k}: clf_next is not theta's label classifier after the flush")
        masks = D.device_masks(fb.acts, c.f, c.emb, c.R, B)
        r64, r32, share, wrong = D.reference_pair(c, ids, lab, sets, params=before["theta"], dev_masks=masks)
        print(f"{tag} step {k} B={B}: {share:.2e} of the activations ambiguous (cap {D.AMBIGUOUS_CAP:.0e}), {wrong} masks wrong")
        shares.append(share)
        if share > D.AMBIGUOUS_CAP:
            problems.append(f"step {k}: {share:.2e} of the activations are ambiguous - change the salt of the batches")
        if wrong:
            problems.append(f"step {k}: {wrong} ReLU masks differ from the float64 sign outside the ambiguous band")
        figs.append(T.step_figures(c, k, before, after, r64, r32, tag=f"{tag} B={B}"))
        tally.check(f"step {k} B={B} loss", torch.tensor(float(fb.last_loss())), r64["loss"], r32["loss"])
        tally.check(f"step {k} B={B} logits", fb.logits[:B], r64["logits"], r32["logits"])
        before = after

    # ---- 3b ----
    torch.cuda.synchronize()
    for name in ("theta", "m", "v", "clf_next", "step_counter"):
        a, b = getattr(fa, name), getattr(fb, name)
        if not torch.equal(a, b):
            problems.append(f"deferred and flushed engines end with different {name} ({int((a != b).sum())} entries)")
    if int(fa.step_counter.item()) != len(sizes):
        problems.append(f"step counter {int(fa.step_counter.item())} after {len(sizes)} steps")
    fa.check()
    fb.check()

    w = T.worst(figs)
    print(f"FIGURES {tag}: of tolerance: (ii) v {w['v']:.3f}  (iii) theta {w['theta']:.3f} | (i) ratio "
          f"{max(w['ratio'], tally.ratio):.2f}  of bound {max(w['grad'], tally.of_bound):.2f} | left out {w['excluded']:.1e}  "
          f"ambiguous {max(shares):.2e}")
    assert w["excluded"] <= A.CANCEL_CAP
    assert not T.misses(figs), T.misses(figs)
    assert not problems, problems
    tally.done()
