"""numpy statement of what pcg_baseline_train computes for one batch (include/pcgnn.h; src/graphsage.py:37-39, 176-178): the mean
two-class cross entropy over ``baseline_ref.forward``'s logits and its gradients to W_enc [E, K] and W_cls [2, E], in float64 (the
reference) and in float32 (the same code: the yardstick the kernels' error is measured by), for the five shapes of
``baseline_ref.SHAPES`` - and the seeded cases the training tests run it on (tests/test_baseline_train_ref_host.py on the CPU,
tests/test_gpu_baseline_train.py on the GPU).

ReLU kinks are handled as in ``dense_ref``: ``mask`` [B, E] of 0 / 1 replaces ``relu(pre)`` by ``pre * mask`` with the mask held
constant (``dense_ref.ambiguous`` / ``resolve_masks`` pick it).  Without a mask the ReLU and its backward are torch's: a NaN
pre-activation goes through both.

The graph is the crafted CSR of tests/test_gpu_baseline_infer.py (every row length at which the aggregation changes strategy);
its node 1 has no neighbours - a NaN aggregate without the self union - and is kept out of every batch here but ``nan_batch``.
"""
import numpy as np
import torch

from tests import adam_ref as A
from tests import baseline_ref as BR
from tests import dense_ref as D

N = 6000
EMPTY_NODE = 1                                        # crafted_csr: the degree-0 row
FE_ALL = ((25, 64), (32, 128))                        # every model shape
FE_TWO = ((509, 64), (300, 16), (1, 16))              # sage_concat and gcn; (509, 64): W_enc is streamed, not staged
STREAMED = ((509, 64),)
CASES = [(F, E, s) for F, E in FE_ALL for s in sorted(BR.SHAPES)] + [(F, E, s) for F, E in FE_TWO for s in ("sage_concat", "gcn")]
# the weight GEMM shares a batch between ceil(B / 1024) workgroups per tile, at most 4 (csrc/baseline_train.hip: bt_kparts): one
# size on each side of 1024, 2048 and 3072; 1, 15, 16, 17: a lone row, a ragged tile, a full one, a second tile
PART_ROWS, MAX_PARTS = 1024, 4
BATCHES = (1, 15, 16, 17, 1024, 1025, 2048, 2049, 3072, 3073)
LR, WD, BETAS, EPS = 0.01, 0.001, (0.9, 0.999), 1e-8
# The twelve training steps: adam_ref.STEPS' pattern - two rounds of a window of three full batches and a tail of 17 and one of a
# full batch and a tail - at a full batch of 1040: two workgroups per tile of the weight GEMM, and enough pre-activations per
# step (1040 * 64) that AMBIGUOUS_CAP leaves room for the handful a float32 run of this size has (at 129 rows the cap is one
# entry of 8256).
STEP_CASES = [(25, 64, "sage"), (32, 128, "sage_concat"), (509, 64, "gcn")]      # (509, 64): W_enc streamed
# From a zero state Adam's first step moves a parameter by lr * g / (|g| + eps): where |g + wd theta| is within a few hundred
# eps = 1e-8 - of ~35 000 parameters a dozen are - a float32 error of the gradient of 1e-9, far inside adam_ref.M_TOL, moves theta
# by many times adam_ref.THETA_ATOL_PER_LR, for ANY float32 Adam (the float32 yardstick's own first step misses that tolerance by
# factors of 5 to 400 on every draw of the centres).  So the twelve steps start from a state loaded through
# load_optimizer_state - zero first moments, second moments WARM_V, step count 0 - where sqrt(v) carries the denominator, and the
# condition, asserted on the reference alone (tests/test_baseline_train_ref_host.py), is that the float32 yardstick's gradient
# through float32 Adam keeps YARDSTICK_THETA of theta's tolerance at every step.  (The first step from zeros is held to
# torch.optim.Adam, float32 against float32, by test_backward_with_a_torch_optimizer_and_accumulation.)
STEP_SALTS = {(25, 64, "sage"): 0, (32, 128, "sage_concat"): 1, (509, 64, "gcn"): 2}
WARM_V = 1e-8
YARDSTICK_THETA = 0.75       # (a float32 theta of up to 0.3 is rounded to 1.5e-8, several times per update: that alone is ~0.5)
STEP_BATCH = 1040
STEP_WINDOWS = (3 * STEP_BATCH + 17, STEP_BATCH + 17)
STEPS = [(w, b0, min(STEP_BATCH, n - b0)) for _ in range(A.ROUNDS) for w, n in enumerate(STEP_WINDOWS) for b0 in range(0, n, STEP_BATCH)]
# (F, E, shape) -> salt of its batches where the draws of salt 0 do not keep AMBIGUOUS_CAP at every size (the host test asserts it)
SALTS = {(300, 16, "gcn"): 4}
_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def kparts(B):
    """bt_kparts of csrc/baseline_train.hip, restated: the workgroups that share a 16 x 16 tile's batch"""
    return max(1, min(MAX_PARTS, ((B + 15) // 16 + PART_ROWS // 16 - 1) // (PART_ROWS // 16)))


def csr_spec():
    from tests.test_gpu_baseline_infer import crafted_csr
    return memo("csr", crafted_csr)


def csr():
    return csr_spec()[:2]


def features(F):
    """Features of the training tests' own.  The ReLU-kink rule (``dense_ref.ambiguous``) sets ONE threshold per batch, 16 times
    the largest float32 error of any pre-activation, and every batch here holds the 5000-row: a float32 sum over 5000 arbitrary
    rows (numpy adds them one after the other) has an error that makes a share of 1e-4 of all pre-activations ambiguous by
    itself, and so does a GCN aggregate (sum / sqrt(count)) many times an ordinary row's.  So the values are odd multiples of
    1 / 128 below 4 with mean zero: every row's sum is exact in float32 in any order - what these tests measure is the dense
    part; the aggregation kernels are held to float64 on arbitrary values by the inference tests -, and no value is zero.
    F = 1: a pre-activation is one product, and a zero aggregate would sit on the kink of every unit: positive values."""
    def make():
        k = np.clip(np.round(np.random.RandomState(200 + F).randn(N, F) * 32.0), -192, 191)
        x = (2.0 * k + 1.0) / 128.0
        return (np.abs(x) if F == 1 else x).astype(np.float32)
    return memo(("X", F), make)


def node_labels():
    return memo("labels", lambda: (np.random.RandomState(7).rand(N) < 0.3).astype(np.int64))


def crafted_node(degree, with_self):
    """the crafted node of that CSR degree which is / is not in its own row"""
    for v, ds in csr_spec()[2].items():
        if ds == (degree, with_self):
            return v
    raise KeyError((degree, with_self))


def pins():
    """what every batch of 15 or more holds: rows of more than 512 neighbours (5000, 1025 and 513: the workgroup's rows; 2049),
    centres that are in their own row and centres that are not, and a duplicated id"""
    return [crafted_node(5000, True), crafted_node(513, False), crafted_node(1025, True), crafted_node(2049, False),
            crafted_node(17, False), crafted_node(5000, True), crafted_node(512, True)]


def salt_of(F, E, shape):
    return SALTS.get((F, E, shape), 0)


def batch(B, salt=0):
    """(ids, labels) int64: drawn with replacement from every node but the empty one, the pins at the front (B = 1: the first)"""
    rs = np.random.RandomState(1000003 * salt + 31 * B + 5)
    ids = rs.randint(0, N - 1, size=B)
    ids[ids >= EMPTY_NODE] += 1
    p = pins()[:B]
    ids[:len(p)] = p
    return ids, node_labels()[ids]


def nan_batch(B=40):
    """a batch with the node that has no neighbours, not on the first tile"""
    ids, _ = batch(B, salt=9)
    ids[21] = EMPTY_NODE
    return ids, node_labels()[ids]


def step_batches(case):
    """(ids, labels) of the twelve steps of STEP_CASES[case]: STEPS' windows drawn once, the second round on the same centres"""
    rs = np.random.RandomState(7919 * STEP_SALTS[STEP_CASES[case]] + 11)
    windows = []
    for n in STEP_WINDOWS:
        ids = rs.randint(0, N - 1, size=n)
        ids[ids >= EMPTY_NODE] += 1
        p = pins()
        ids[:len(p)] = p
        windows.append(ids)
    return [(windows[w][b0:b0 + B], node_labels()[windows[w][b0:b0 + B]]) for w, b0, B in STEPS]


def model_weights(F, E, shape):
    """(W_enc, W_cls) float32 numpy of ``baseline_ref.build_model(..., seed=F * 1000 + E)`` - drawn on the CPU, as the GPU tests'
    models are before they move"""
    def make():
        from pcgnn_amd import graphsage as GS
        m = BR.build_model(GS, None, F, E, shape, seed=F * 1000 + E, device=None)
        return m.enc.weight.detach().numpy().copy(), m.weight.detach().numpy().copy()
    return memo(("w", F, E, shape), make)


def aggregates(F, shape, dtype):
    """a [N, F] of every node in `dtype` (``baseline_ref.aggregate``: ``forward``'s own first step), computed once"""
    s = BR.SHAPES[shape]
    key = ("agg", F, s["add_self"], s["norm"], np.dtype(dtype).name)
    hoods = memo(("hoods", s["add_self"]), lambda: BR.neighbourhoods(csr(), np.arange(N), s["add_self"]))
    return memo(key, lambda: BR.aggregate(features(F), csr(), np.arange(N), s["add_self"], s["norm"], dtype, hoods))


def loss_and_grad(F, shape, ids, labels, W_enc, W_cls, dtype=np.float64, mask=None):
    """dict(loss, d_enc [E, K], d_cls [2, E], logits [B, 2], pre [B, E]) in `dtype` for the batch on the crafted graph.
    ``baseline_ref.forward``'s formulas (a, z, pre, h, logits - the unmasked logits ARE forward's), then the mean cross entropy,
    dlogits = (softmax - onehot) / B, d_cls = dlogits^T h, dpre = (dlogits W_cls) under the mask, d_enc = dpre^T z."""
    s = BR.SHAPES[shape]
    ids = np.asarray(ids, dtype=np.int64)
    y = np.asarray(labels, dtype=np.int64)
    B = len(ids)
    X = features(F)
    a = aggregates(F, shape, dtype)[ids]
    z = np.concatenate([X[ids].astype(dtype), a], axis=1) if s["concat_self"] else a
    We, Wc = np.asarray(W_enc).astype(dtype), np.asarray(W_cls).astype(dtype)
    with np.errstate(invalid="ignore"):
        pre = (z @ We.T).astype(dtype)
        h = np.where(pre <= 0, dtype(0), pre) if mask is None else pre * np.asarray(mask).astype(dtype)
        logits = (h @ Wc.T).astype(dtype)
        top = logits.max(axis=1, keepdims=True)
        ex = np.exp(logits - top)
        lse = (top[:, 0] + np.log(ex.sum(axis=1))).astype(dtype)
        loss = ((lse - logits[np.arange(B), y]).sum() / dtype(B)).astype(dtype)
        dlog = ex / ex.sum(axis=1, keepdims=True)
        dlog[np.arange(B), y] -= dtype(1)
        dlog = (dlog / dtype(B)).astype(dtype)
        d_cls = (dlog.T @ h).astype(dtype)
        dh = (dlog @ Wc).astype(dtype)
        dpre = np.where(pre <= 0, dtype(0), dh) if mask is None else dh * np.asarray(mask).astype(dtype)
        d_enc = (dpre.T @ z).astype(dtype)
    return dict(loss=loss, d_enc=d_enc, d_cls=d_cls, logits=logits, pre=pre)


def reference_pair(F, shape, ids, labels, W_enc, W_cls, dev_mask=None):
    """The float64 reference and its float32 yardstick for one batch, with the ReLU-kink rule applied (``dense_ref``'s).
    dev_mask: the device's ``h > 0`` [B, E] (None: the float64 sign everywhere).  Returns (ref64, ref32, share of ambiguous
    pre-activations, non-ambiguous entries where the device's mask is not the float64 sign)."""
    args = (F, shape, ids, labels, W_enc, W_cls)
    p64, p32 = loss_and_grad(*args, dtype=np.float64), loss_and_grad(*args, dtype=np.float32)
    pre64, pre32 = [torch.from_numpy(p64["pre"])], [torch.from_numpy(p32["pre"])]
    _, amb, share = D.ambiguous(pre64, pre32)
    masks, wrong = D.resolve_masks(pre64, amb, None if dev_mask is None else [torch.as_tensor(dev_mask).cpu()])
    mask = masks[0].numpy()
    return loss_and_grad(*args, dtype=np.float64, mask=mask), loss_and_grad(*args, dtype=np.float32, mask=mask), share, wrong


def autograd_f64(F, shape, ids, labels, W_enc, W_cls):
    """(loss, d_enc, d_cls) by torch autograd in float64 over the same formulas: what the host test holds ``loss_and_grad`` to"""
    s = BR.SHAPES[shape]
    ids = np.asarray(ids, dtype=np.int64)
    a = torch.from_numpy(aggregates(F, shape, np.float64)[ids])
    x = torch.from_numpy(features(F)[ids].astype(np.float64))
    z = torch.cat((x, a), dim=1) if s["concat_self"] else a
    We = torch.from_numpy(np.asarray(W_enc)).double().requires_grad_(True)
    Wc = torch.from_numpy(np.asarray(W_cls)).double().requires_grad_(True)
    logits = torch.relu(z.mm(We.t())).mm(Wc.t())
    loss = torch.nn.functional.cross_entropy(logits, torch.from_numpy(np.asarray(labels, dtype=np.int64)))
    d_enc, d_cls = torch.autograd.grad(loss, [We, Wc])
    return loss.detach().numpy(), d_enc.numpy(), d_cls.numpy()


def flat(d_cls, d_enc):
    """the two matrices as one vector in pcg_baseline_train's grad_out order: [W_cls | W_enc]"""
    return torch.cat([torch.as_tensor(d_cls).reshape(-1), torch.as_tensor(d_enc).reshape(-1)])


def adam_f32(theta, m, v, g, t, lr, betas, eps, wd):
    """``adam_ref.adam_ref`` with every operation in float32 (the yardstick of a float32 Adam)"""
    f = lambda x: torch.as_tensor(x).float()
    theta, m, v, g = f(theta), f(m), f(v), f(g)
    b1, b2, one = f(betas[0]), f(betas[1]), f(1.0)
    g = g + f(wd) * theta
    m1 = b1 * m + (one - b1) * g
    v1 = b2 * v + (one - b2) * g * g
    bc1, bc2 = one - b1 ** t, one - b2 ** t
    return theta - (f(lr) / bc1) * (m1 / (v1.sqrt() / bc2.sqrt() + f(eps))), m1, v1


def adam_steps_f64(F, shape, batches, W_enc, W_cls):
    """The float64 run of the steps from float32 starting weights: the reference alone (masks: the float64 sign), every step from
    the float64 state of the one before, the first from (m, v) = (0, WARM_V).  Yields (k, ref64 of the step, share of ambiguous pre-activations, share of cancelled
    Adam entries, (theta, m, v) after the step, ``adam_ref.adam_figures`` of the float32 yardstick - its gradient through
    ``adam_f32`` from the state rounded to float32)."""
    theta = flat(W_cls, W_enc).double()
    m, v = torch.zeros_like(theta), torch.full_like(theta, WARM_V)
    E = np.asarray(W_cls).shape[1]
    for k, (ids, labels) in enumerate(batches):
        Wc, We = theta[:2 * E].view(2, E).numpy(), theta[2 * E:].view(E, -1).numpy()
        r64, r32, share, _ = reference_pair(F, shape, ids, labels, We, Wc)
        g = flat(r64["d_cls"], r64["d_enc"])
        out = float(A.cancelled(theta, g, WD).double().mean())
        t32, m32, v32 = theta.float(), m.float(), v.float()
        # (the yardstick's own gradient is that of the float32 weights: the reference at them, so that only Adam's inputs differ)
        q64, q32, _, _ = reference_pair(F, shape, ids, labels, t32[2 * E:].view(E, -1).numpy(), t32[:2 * E].view(2, E).numpy())
        yard = A.adam_figures(adam_f32(t32, m32, v32, flat(q32["d_cls"], q32["d_enc"]), k + 1, LR, BETAS, EPS, WD), t32, m32, v32,
                              flat(q64["d_cls"], q64["d_enc"]), k + 1, LR, BETAS, EPS, WD)
        theta, m, v = A.adam_ref(theta, m, v, g, k + 1, LR, BETAS, EPS, WD)
        yield k, r64, share, out, (theta, m, v), yard
