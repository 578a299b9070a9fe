"""A plain float64 statement of one ``torch.optim.Adam`` step, and the seeded cases of the partitioned training tests
(tests/test_adam_ref_host.py on the CPU, tests/test_gpu_dist_train_f64.py on the GPU).

``adam_ref``: coupled (L2) weight decay, bias correction with the 1-based step number t, eps added outside the square root -
torch.optim.Adam(amsgrad=False, maximize=False), what ``adam_update`` (csrc/common.h) restates in float32.

The partitioned step's reference needs no code of its own: every rank's dense launch scales its rows' loss by
1 / (B * world), the all-reduce sums the ranks' gradients, so the step's gradient is that of the mean loss over the GLOBAL
batch - plain ``dense_ref`` (which divides by the length of the batch it is given) on the ranks' ids and labels concatenated in
rank order (``global_batch``).  The loss scale is what that tests.

``DistCase``: a ``synth.make_workload`` graph, the parameters ``DistributedPCGNN`` draws from its seed (restated here, so that
the CPU tests can run the reference on exactly the batches the GPU test trains on; the GPU test asserts the two equal), and
every rank's centres of two windows, drawn on the host.  It carries the fields ``dense_ref.GradCase.host_sets`` and
``dense_ref.reference_pair`` read.
"""
import math

import numpy as np
import torch

from tests import dense_ref as D
from tests.util import PARAM_KEYS

# the tolerances of test_adam_step_matches_torch_adam (tests/test_gpu_parity.py), by which the partitioned step's Adam is held too
THETA_ATOL_PER_LR = 2e-5                  # theta: atol = lr * 2e-5, rtol 0
M_TOL = (1e-5, 2e-7)                      # (rtol, atol)
V_TOL = (5e-5, 1e-12)
CANCEL = 2.0 ** -16                       # |g + wd theta| below this x max(|g|, wd |theta|): the float32 sum has no correct digit
CANCEL_CAP = 1e-3                         # at most this share of a step's parameters may be left out for it (a condition)


def adam_ref(theta, m, v, g, t, lr, betas, eps, wd):
    """One step of torch.optim.Adam in float64 on the given values: returns (theta', m', v').  t: the step's number, 1-based."""
    theta, m, v, g = (torch.as_tensor(x).detach().cpu().double() for x in (theta, m, v, g))
    b1, b2 = float(betas[0]), float(betas[1])
    g = g + wd * theta
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    denom = v1.sqrt() / math.sqrt(bc2) + eps
    return theta - (lr / bc1) * (m1 / denom), m1, v1


def cancelled(theta, g, wd):
    """entries whose float64 |g + wd theta| is below 2^-16 of the larger term: bool tensor"""
    theta, g = torch.as_tensor(theta).detach().cpu().double(), torch.as_tensor(g).detach().cpu().double()
    return (g + wd * theta).abs() < CANCEL * torch.maximum(g.abs(), wd * theta.abs())


def adam_figures(got, theta, m, v, g, t, lr, betas, eps, wd):
    """(theta', m', v') of some float32 Adam against adam_ref in float64 from the same inputs.  Returns dict(theta, m, v: the
    worst error as a fraction of the tolerance - <= 1 passes, by numpy.testing.assert_allclose's rule |x - ref| <= atol +
    rtol |ref|; theta over the entries that are not ``cancelled`` -, excluded: the share of entries left out of theta's)."""
    ref = adam_ref(theta, m, v, g, t, lr, betas, eps, wd)
    err = [(torch.as_tensor(x).detach().cpu().double() - r).abs() for x, r in zip(got, ref)]
    out = cancelled(theta, g, wd)
    keep = ~out
    return dict(theta=float((err[0][keep] / (lr * THETA_ATOL_PER_LR)).max()) if bool(keep.any()) else 0.0,
                m=float((err[1] / (M_TOL[1] + M_TOL[0] * ref[1].abs())).max()),
                v=float((err[2] / (V_TOL[1] + V_TOL[0] * ref[2].abs())).max()),
                excluded=float(out.double().mean()))


def global_batch(ids_by_rank, labels_by_rank):
    """the global batch of a partitioned step: the ranks' (global) ids and labels concatenated in rank order -> int64 numpy"""
    return (np.concatenate([np.asarray(torch.as_tensor(x).cpu()).astype(np.int64).reshape(-1) for x in ids_by_rank]),
            np.concatenate([np.asarray(torch.as_tensor(x).cpu()).astype(np.int64).reshape(-1) for x in labels_by_rank]))


def flatten(by_name, R):
    """per-parameter tensors -> one flat vector in PARAM_KEYS order (the host tests' own layout: Adam is element-wise)"""
    return torch.cat([by_name[k].reshape(-1) for k in PARAM_KEYS(R)])


def unflatten(flat, like, R):
    out, at = {}, 0
    for k in PARAM_KEYS(R):
        n = like[k].numel()
        out[k] = flat[at:at + n].view(like[k].shape)
        at += n
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the cases.  Per-rank batch 129 = eight full 16-row tiles and one row; a window of 3 * 129 + 17 centres per rank (steps of 129,
# 129, 129 and 17: the short one follows longer ones in the same buffers), then a window of 129 + 17 (an update rides across
# the window boundary; batch position 1 sees another size than before).  The two windows run TWICE, on the same centres: the
# first use of a step's graph runs a warm-up step that applies the waiting update itself, so only from the second round on
# does every step of the captured path - the 17-row tails included - find a gradient waiting at its replay.
# ---------------------------------------------------------------------------------------------------------------------------
BATCH = 129
WINDOWS = (3 * BATCH + 17, BATCH + 17)
ROUNDS = 2
# (window, first centre, batch size) of every step, in order
STEPS = [(w, b0, min(BATCH, n - b0)) for _ in range(ROUNDS) for w, n in enumerate(WINDOWS) for b0 in range(0, n, BATCH)]
NODES, REL_EDGES = 6000, (3000, 18000, 48000)
# (F, E, R) -> seed of the case (graph, parameters, centres): one at which every step's global batch keeps
# dense_ref.AMBIGUOUS_CAP and every step's CANCEL_CAP at world sizes 1 and 2 (tests/test_adam_ref_host.py asserts both)
CASES = {(32, 64, 3): 17, (25, 128, 3): 27}
WORLDS = (1, 2)


class DistCase:
    lr, wd, rho, alpha = 0.01, 0.001, 0.5, 2.0
    betas, eps = (0.9, 0.999), 1e-8

    def __init__(self, shape, world):
        from pcgnn_amd import synth
        from pcgnn_amd.dist import Partition, total_degree
        F, E, R = shape
        assert R == len(REL_EDGES)
        self.shape, self.world, self.seed = shape, world, CASES[shape]
        self.f, self.emb, self.R, self.n = F, E, R, NODES
        self.w = synth.make_workload("t", NODES, F, REL_EDGES, 0.15, seed=self.seed, skew=1.5)
        self.X, self.labels, self.csr, self.train_pos = self.w.X, self.w.labels, self.w.csr, list(self.w.train_pos)
        assert len(self.train_pos) < 16384
        self.cfg = dict(emb_size=E, rho=self.rho, alpha=self.alpha, lr=self.lr, weight_decay=self.wd, batch_size=BATCH, seed=self.seed)
        self.parts = [Partition.balanced(total_degree(self.w.csr), world, r) for r in range(world)]
        # DistributedPCGNN.__init__'s draws, in its order: xavier_uniform_ for the matrices, nn.Linear's for the label classifier
        gen = torch.Generator().manual_seed(self.seed)
        self._params = {}
        for k, shp in ([("weight", (2, E)), ("inter1.weight", (F + R * E, E))]
                       + [(f"inter1.intra_agg{r + 1}.weight", (2 * F, E)) for r in range(R)]):
            bound = math.sqrt(6.0 / (shp[0] + shp[1]))
            self._params[k] = ((torch.rand(shp[0] * shp[1], generator=gen) * 2 - 1) * bound).view(shp)
        for k, shp in (("inter1.label_clf.weight", (2, F)), ("inter1.label_clf.bias", (2,))):
            self._params[k] = ((torch.rand(int(np.prod(shp)), generator=gen) * 2 - 1) / math.sqrt(F)).view(shp)

    def params(self):
        return {k: v.clone() for k, v in self._params.items()}

    def centres(self, rank, window):
        """rank's centres of a window: LOCAL rows of training nodes it owns, drawn with replacement (int64 numpy)"""
        part = self.parts[rank]
        own = self.w.idx_train[(self.w.idx_train >= part.lo) & (self.w.idx_train < part.hi)]
        rs = np.random.RandomState(self.seed * 100003 + 1009 * window + 31 * rank + self.world)
        return own[rs.randint(0, own.size, size=WINDOWS[window])] - part.lo

    def step_batch(self, k):
        """(ids, labels) of step k's GLOBAL batch (global node ids)"""
        win, b0, B = STEPS[k]
        ids = [self.centres(r, win)[b0:b0 + B] + self.parts[r].lo for r in range(self.world)]
        return global_batch(ids, [self.labels[i] for i in ids])

    def host_sets(self, ids, labels, params=None):
        """the oracle's training-mode selection on the whole graph (CPU tests: no device to take the sets from)"""
        return D.GradCase.host_sets(self, ids, labels, params)
