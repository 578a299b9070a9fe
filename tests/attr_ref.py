"""A plain-torch CPU reference of ``FusedPCGNN.attribute`` (tests/test_attr_ref_host.py, tests/test_gpu_attribute.py): the gnn
path of tests/dense_ref.py - mean of the chosen rows, ``relu(cat(x, a_r) @ W_r)`` per relation, ``relu(cat(x, h_1 .. h_R) @
W_inter)``, ``logits = comb @ W_cls^T`` - with the selection taken as an input and the centre rows ``x`` and every aggregate
``a_r`` as autograd leaves; the attributed scalar is ``w0 * logit0 + w1 * logit1`` per row (rows do not interact, so one backward
of the sum gives every row's gradient).  ``dtype`` picks the precision of every operation: float64 is the reference, float32 -
the same code - the yardstick the kernels' error is measured by.

ReLU kinks: ``attribute`` exposes no masks, so a row any of whose R + 1 pre-activation rows has an entry within rounding of
zero (``dense_ref.ambiguous``: |pre_f64| < 16 * max|pre_f32 - pre_f64|, CPU runs only) is left out of a comparison
(``kept_rows``); at most ``ROW_CAP`` of a case's rows may be.
"""
import numpy as np
import torch
import torch.nn.functional as Fn

from tests.dense_ref import SHAPES, GradCase, ambiguous, rel_err, sets_to_index, tolerance  # noqa: F401  (shared with the tests)

ROW_CAP = 0.02
TARGETS = [(0.0, 1.0), (-1.0, 1.0)]
BATCH_SIZES = [1, 15, 16, 17, 65]


def _weights(params, R, dtype):
    return ([params[f"inter1.intra_agg{r + 1}.weight"].detach().to(dtype) for r in range(R)], params["inter1.weight"].detach().to(dtype),
            params["weight"].detach().to(dtype))


def aggregates(X, index, n, dtype):
    """a_r [n, F] per relation: the mean of the chosen rows (0 / 0 = NaN for an empty set, as the reference's mask.div).  A row's
    entries are added in ascending id order whatever order the index lists them in (``sets_to_index``'s own): the float32 run -
    and with it the ReLU-kink condition - is then a function of the chosen SETS, the same for the oracle's sets on the host and
    a device's ranked lists."""
    out = []
    for rows, cols, cnt in index:
        order = torch.argsort(rows * X.shape[0] + cols)
        out.append(torch.zeros(n, X.shape[1], dtype=dtype).index_add_(0, rows[order], X[cols[order]]) / cnt.to(dtype)[:, None])
    return out


def attr_ref(X, ids, index, params, target, dtype=torch.float64):
    """X [N, F]; ids [n]; index: per relation (rows, cols, counts) - ``sets_to_index`` of sets[r][b], or a device selection's
    lists in their own order; params: state-dict names -> tensors; target (w0, w1).  Returns dict(logits [n, 2], d_self [n, F],
    d_agg [R, n, F], self_contrib [n], rel_contrib [R, n], neigh_contrib [total] - entry e of relation r's (rows, cols), the
    relations one after the other: <X[cols[e]], d_agg[r, rows[e]]> / counts[rows[e]] -, pre: R + 1 tensors [n, E]), in ``dtype``."""
    X = torch.as_tensor(X).to(dtype)
    ids = torch.as_tensor(np.asarray(ids)).long()
    index = sets_to_index(index)
    n, R = ids.numel(), len(index)
    Wr, Wi, Wc = _weights(params, R, dtype)
    x = X[ids].clone().requires_grad_(True)
    a = [t.detach().requires_grad_(True) for t in aggregates(X, index, n, dtype)]
    pre = [torch.cat((x, a[r]), dim=1).mm(Wr[r]) for r in range(R)]
    pre.append(torch.cat([x] + [Fn.relu(p) for p in pre], dim=1).mm(Wi))
    logits = Fn.relu(pre[-1]).mm(Wc.t())
    w = torch.tensor(target, dtype=dtype)
    grads = torch.autograd.grad((logits * w).sum(), [x] + a)
    d_self, d_agg = grads[0], torch.stack(grads[1:])
    return finish(X, x.detach(), [t.detach() for t in a], index, logits.detach(), d_self, d_agg, [p.detach() for p in pre])


def finish(X, x, a, index, logits, d_self, d_agg, pre):
    neigh = [(X[cols] * d_agg[r][rows]).sum(1) / cnt.to(X.dtype)[rows] for r, (rows, cols, cnt) in enumerate(index)]
    return dict(logits=logits, d_self=d_self, d_agg=d_agg, self_contrib=(x * d_self).sum(1),
                rel_contrib=torch.stack([(a[r] * d_agg[r]).sum(1) for r in range(len(a))]),
                neigh_contrib=torch.cat(neigh) if neigh else torch.zeros(0, dtype=X.dtype), pre=pre)


def attr_manual(X, ids, index, params, target, dtype=torch.float64):
    """The same values by the kernel's three hand-written phases instead of autograd:
    dcomb = (w0 W_cls[0] + w1 W_cls[1]) * (comb > 0);  dh_r = (dcomb W_inter[F + rE .., :]^T) * (h_r > 0),  dx0 = dcomb
    W_inter[:F, :]^T;  dcat_r = dh_r W_r^T;  d_self = dx0 + sum_r dcat_r[:, :F],  d_agg_r = dcat_r[:, F:]."""
    X = torch.as_tensor(X).to(dtype)
    ids = torch.as_tensor(np.asarray(ids)).long()
    index = sets_to_index(index)
    n, R, F = ids.numel(), len(index), X.shape[1]
    Wr, Wi, Wc = _weights(params, R, dtype)
    E = Wi.shape[1]
    x, a = X[ids], aggregates(X, index, n, dtype)
    pre = [torch.cat((x, a[r]), dim=1).mm(Wr[r]) for r in range(R)]
    pre.append(torch.cat([x] + [Fn.relu(p) for p in pre], dim=1).mm(Wi))
    logits = Fn.relu(pre[-1]).mm(Wc.t())
    dcomb = (target[0] * Wc[0] + target[1] * Wc[1])[None, :] * (pre[-1] > 0).to(dtype)
    d_self = dcomb.mm(Wi[:F].t())
    d_agg = []
    for r in range(R):
        dh = dcomb.mm(Wi[F + r * E:F + (r + 1) * E].t()) * (pre[r] > 0).to(dtype)
        dcat = dh.mm(Wr[r].t())
        d_self = d_self + dcat[:, :F]
        d_agg.append(dcat[:, F:])
    return finish(X, x, a, index, logits, d_self, torch.stack(d_agg), pre)


def kept_rows(pre64, pre32, widen=1.0):
    """bool [n]: the rows none of whose R + 1 pre-activation rows has an ambiguous entry; and the share left out.  widen: the
    band times this factor (the host test's margin: the float32 run, and with it the band, differs a little from CPU to CPU)"""
    tau, _, _ = ambiguous(pre64, pre32)
    out = torch.zeros(pre64[0].shape[0], dtype=torch.bool)
    for p in pre64:
        out |= (p.abs() < widen * tau).any(dim=1)
    return ~out, float(out.double().mean()) if out.numel() else 0.0


def target_logit(logits, target):
    return target[0] * logits[:, 0] + target[1] * logits[:, 1]


def residual(res, target):
    """max|self_contrib + sum_r rel_contrib - target . logits| / max|target . logits| (float64 arithmetic on the given values)"""
    s = target_logit(res["logits"].detach().cpu().double(), target)
    gap = res["self_contrib"].detach().cpu().double() + res["rel_contrib"].detach().cpu().double().sum(0) - s
    return float(gap.abs().max()) / float(s.abs().max())


def host_test_sets(case, ids):
    """the oracle's TEST-mode selection of the case's own parameters for ids (CPU tests: no device to take the lists from)"""
    from oracle import pcgnn_oracle as O
    p = case.params()
    s0 = Fn.linear(torch.from_numpy(case.X), p["inter1.label_clf.weight"], p["inter1.label_clf.bias"])[:, 0]
    ids = [int(v) for v in ids]
    sets = []
    for indptr, idx in case.csr:
        lists = [idx[indptr[v]:indptr[v + 1]].tolist() for v in ids]
        nsc = [s0[torch.as_tensor(l).long()] for l in lists]
        sets.append(O.choose_sets(s0[torch.as_tensor(ids).long()], None, lists, nsc, case.train_pos, s0[:0], 0.5, 0.0, False))
    return sets


# GradCase.batch's salt per shape: the first at which every batch keeps the ReLU-kink condition with the band DOUBLED (a batch of
# 17 rows may leave out none: one row a few per cent inside the band on one CPU is outside it on another)
BATCH_SALT = {(32, 64, 3): 2, (25, 128, 3): 1}
# the edge and wide shapes of dense_ref.EDGE_ATTR_SHAPES (tests/test_gpu_edge_shapes.py): a salt at which no row of any batch lies
# in the doubled band (E = 272 has 544 activations a row: one row in twenty of its graph has one in the band), the batch of 65
# draws a node twice, and the lone row keeps COND_CAP below (tests/test_edge_shapes_host.py asserts all three)
BATCH_SALT.update({(16, 64, 4): 388, (30, 64, 3): 443, (20, 128, 1): 86, (20, 32, 7): 1111, (17, 32, 8): 137, (32, 64, 8): 1509,
                   (64, 64, 3): 1919, (16, 272, 1): 5484, (100, 64, 3): 685, (260, 16, 1): 1022, (360, 16, 1): 225, (24, 16, 1): 11})


def id_sets(case):
    """name -> ids of the GPU test's cases: the batches (drawn with replacement) and the whole graph"""
    salt = BATCH_SALT.get((case.f, case.emb, case.R), 0)
    out = {f"n{B}": case.batch(B, salt)[0] for B in BATCH_SIZES}
    out["whole"] = np.arange(case.n)
    return out


# A batch of ONE row: self_contrib and rel_contrib are tensors of one element, so "relative to the tensor's largest element" is
# relative to the inner product itself, and where its terms cancel the figure is the sum's condition number (sum |terms| /
# |sum terms|) times the rounding of its inputs, whatever computes it: merely rounding one factor of every term to float32 moves
# the sum by up to 2^-24 * condition, and the float32 yardstick of a single element is one draw - at (16, 272, 1) a row with
# <a_1, ds / da_1> = 0.0088 from terms of 0.21 in all (condition 24) has float32 torch at 5e-8 or 1.7e-6 of it depending on the
# order of the set alone, and a device error of 2.1e-6, under ONE ulp of the summands, missed the bound (8 * 4.9e-8 + 2^-20).
# The lone row of the edge shapes is therefore one whose inner products - the self product and every relation's, both targets -
# keep 2^-24 * condition under the tolerance's floor 2^-20: condition <= COND_CAP = 16 (a condition on the float64 reference
# alone, like the ReLU-kink one).  Batches of several rows need none: their largest element is the yardstick of every row.
COND_CAP = 16.0


def contrib_condition(X, ids, index, r64):
    """max over the rows, and over the self product and every relation's, of sum |terms| / |sum terms| (float64; r64: attr_ref's
    float64 result for the same ids and index)"""
    X = torch.as_tensor(X).double()
    x = X[torch.as_tensor(np.asarray(ids)).long()]
    a = aggregates(X, sets_to_index(index), len(ids), torch.float64)
    terms = [x * r64["d_self"]] + [a[r] * r64["d_agg"][r] for r in range(len(a))]
    return max(float((t.abs().sum(1) / t.sum(1).abs()).max()) for t in terms)


def hub_ids(case):
    """the batch of 65 with the graph's two largest rows at its first two positions (lists of more than 128 chosen entries:
    the neighbour kernel's tail slices)"""
    hub, second = case.hubs(2)
    return case.batch(65, BATCH_SALT.get((case.f, case.emb, case.R), 0), pins={0: hub, 1: second})[0]


# ---------------------------------------------------------------------------------------------------------------------------
# long rows: an explicit graph whose first centres' kept counts straddle the gather's 128-entry chunk (threshold 0.5: a row of
# deg > ceil(deg / 2) + 1 keeps ceil(deg / 2)) - 256 -> 128 (one chunk), 258 -> 129 (two), 300 -> 150, 1000 -> 500 - and one
# node with an empty row in relation 1 (a 0 / 0 aggregate)
# ---------------------------------------------------------------------------------------------------------------------------
LONG_DEGS = [256, 258, 300, 1000]
LONG_KEPT = [128, 129, 150, 500]
LONG_N, ISOLATED = 1500, 30


class LongRowCase(GradCase):
    def __init__(self, seed=11):
        super().__init__(32, 64, 3, seed=seed)
        rs = np.random.RandomState(seed + 77)
        self.n = LONG_N
        self.X = rs.randn(LONG_N, 32).astype(np.float32)
        self.labels = (rs.rand(LONG_N) < 0.15).astype(np.int64)
        self.train_pos = [int(v) for v in range(LONG_N // 2) if self.labels[v] == 1]
        self.csr = []
        for r in range(3):
            rows = []
            for v in range(LONG_N):
                deg = LONG_DEGS[v] if v < len(LONG_DEGS) else int(rs.randint(2, 9))
                nb = set(rs.choice(LONG_N, size=deg, replace=False).tolist())
                if v >= len(LONG_DEGS):
                    nb.add(v)                                   # (ordinary rows keep the reference's self-loop)
                if v == ISOLATED and r == 1:
                    nb = set()
                rows.append(sorted(nb))
            indptr = np.zeros(LONG_N + 1, dtype=np.int64)
            indptr[1:] = np.cumsum([len(x) for x in rows])
            self.csr.append((indptr, np.array([j for x in rows for j in x], dtype=np.int32)))

    def long_ids(self):
        """the four long centres and twenty ordinary nodes (n % 16 != 0), the isolated node not among them"""
        return np.concatenate([np.arange(len(LONG_DEGS)), np.arange(100, 120)])

    def tile_with_isolated(self):
        """the isolated node in a tile with fifteen ordinary rows"""
        return np.concatenate([np.arange(200, 207), [ISOLATED], np.arange(207, 215)])
