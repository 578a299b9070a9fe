"""A plain-torch CPU reference of the dense tail of a PC-GNN training step, and the seeded synthetic cases the gradient tests
run it on (tests/test_dense_ref_host.py, tests/test_gpu_grad_f64.py).

The function is ``OraclePCGNN.forward`` / ``.loss`` (oracle/pcgnn_oracle.py) with the selection taken as an input: mean of the
chosen rows, ``relu(cat(self, agg_r) @ W_r)`` per relation, ``relu(cat(self, h_1 .. h_R) @ W_inter)``, gnn logits, label-aware
logits from ``X[ids]``, ``CE(gnn) + lambda_1 * CE(label)`` (mean reduction), autograd for every parameter.  ``dtype`` picks the
precision of every operation: float64 is the reference, float32 - the same code - the yardstick the kernels' error is
measured by.

ReLU kinks: a pre-activation within rounding of zero may take another mask in f32 than in f64, and the gradient jumps with it.
``ambiguous`` marks such entries (|pre_f64| < 16 * max|pre_f32 - pre_f64|), ``resolve_masks`` takes the device's own mask for
them and the f64 sign for every other entry, and a reference run with ``masks`` computes ``pre * mask`` with the mask held
constant instead of ``relu(pre)``.
"""
import numpy as np
import torch
import torch.nn.functional as Fn

from tests.util import PARAM_KEYS, synth_graph

AMBIGUOUS_CAP = 1e-4        # at most this share of a case's activations may be ambiguous (a condition, not a measurement)
MARGIN, FLOOR = 8.0, 2.0 ** -20


def sets_to_index(sets):
    """sets[r][b] (Python sets of node ids) -> a list of per-relation tuples (rows int64, cols int64, counts float64 [B])"""
    if len(sets) and isinstance(sets[0], tuple):         # (an index already)
        return sets
    out = []
    for rel in sets:
        cnt = np.array([len(s) for s in rel], dtype=np.int64)
        rows = np.repeat(np.arange(len(rel), dtype=np.int64), cnt)
        cols = np.fromiter((j for s in rel for j in sorted(s)), dtype=np.int64, count=int(cnt.sum()))
        out.append((torch.from_numpy(rows), torch.from_numpy(cols), torch.from_numpy(cnt.astype(np.float64))))
    return out


def dense_ref(X, ids, labels, sets, params, lambda_1, dtype=torch.float64, masks=None, row_weight=None):
    """X [n, F]; ids / labels [B]; sets: sets[r][b] or sets_to_index(sets); params: the reference's state-dict names -> tensors;
    masks: None (F.relu) or R + 1 tensors [B, E] (h_1 .. h_R, combined) of 0 / 1 - the masked ReLU ``pre * mask``.
    row_weight [B]: every row's loss term times its weight before the sum / B (None: ones - the mean; the host tests drop or
    double a row with it).  Returns dict(loss, logits [B, 2], center [B, 2], pre: R + 1 tensors [B, E], grads: name -> tensor),
    everything in ``dtype``, detached."""
    X = torch.as_tensor(X).to(dtype)
    ids = torch.as_tensor(np.asarray(ids)).long()
    y = torch.as_tensor(np.asarray(labels)).long()
    B, R = ids.numel(), len(sets)
    index = sets_to_index(sets)
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    self_feats = X[ids]
    act = (lambda r, pre: Fn.relu(pre)) if masks is None else (lambda r, pre: pre * masks[r].to(dtype))
    feats, pre = [self_feats], []
    for r, (rows, cols, cnt) in enumerate(index):
        agg = torch.zeros(B, X.shape[1], dtype=dtype).index_add_(0, rows, X[cols]) / cnt.to(dtype)[:, None]
        pre.append(torch.cat((self_feats, agg), dim=1).mm(p[f"inter1.intra_agg{r + 1}.weight"]))
        feats.append(act(r, pre[-1]))
    pre.append(torch.cat(feats, dim=1).mm(p["inter1.weight"]))
    comb = act(R, pre[-1])
    logits = comb.mm(p["weight"].t())
    center = Fn.linear(self_feats, p["inter1.label_clf.weight"], p["inter1.label_clf.bias"])
    rows_loss = Fn.cross_entropy(logits, y, reduction="none") + lambda_1 * Fn.cross_entropy(center, y, reduction="none")
    if row_weight is not None:
        rows_loss = rows_loss * torch.as_tensor(row_weight).to(dtype)
    loss = rows_loss.sum() / B
    names = list(p)
    grads = torch.autograd.grad(loss, [p[k] for k in names])
    return dict(loss=loss.detach(), logits=logits.detach(), center=center.detach(), pre=[t.detach() for t in pre],
                grads={k: g.detach() for k, g in zip(names, grads)})


def ambiguous(pre64, pre32):
    """(tau, per-activation bool tensors, share of the case's activations): |pre_f64| < tau = 16 * max|pre_f32 - pre_f64|"""
    tau = 16.0 * max(float((a.double() - b).abs().max()) for a, b in zip(pre32, pre64))
    amb = [b.abs() < tau for b in pre64]
    return tau, amb, sum(int(a.sum()) for a in amb) / sum(a.numel() for a in amb)


def resolve_masks(pre64, amb, dev_masks=None):
    """The masks a reference run uses: the f64 sign, and the device's own mask where the entry is ambiguous (dev_masks None -
    no device at hand -: the f64 sign there too).  Returns (masks, number of NON-ambiguous entries where the device's mask is
    not the f64 sign - which the caller asserts to be zero)."""
    masks, wrong = [], 0
    for r, p64 in enumerate(pre64):
        sign = p64 > 0
        if dev_masks is None:
            masks.append(sign.double())
            continue
        d = dev_masks[r].bool()
        wrong += int(((d != sign) & ~amb[r]).sum())
        masks.append(torch.where(amb[r], d, sign).double())
    return masks, wrong


def device_masks(acts, F, E, R, B):
    """``h > 0`` for h_1 .. h_R and the combined embeddings, from an engine's ``acts`` buffer after an acts-mode dense launch
    (layout: the top of csrc/wgrad.h - a batch row per column): R + 1 bool tensors [B, E] on the CPU."""
    a = acts.detach().cpu()
    r_comb = (F + R * E) + R * F + E + R * E
    out = [(a[F + r * E:F + (r + 1) * E, :B] > 0).t().contiguous() for r in range(R)]
    out.append((a[r_comb:r_comb + E, :B] > 0).t().contiguous())
    return out


def rel_err(x, ref):
    """max|x - ref| / max|ref| (float64 arithmetic)"""
    x, ref = torch.as_tensor(x).detach().cpu().double(), torch.as_tensor(ref).double()
    return float((x - ref).abs().max()) / float(ref.abs().max())


def tolerance(e_f32):
    """what a kernel's error may be where the same code in float32 on the CPU has error e_f32 (both by rel_err against float64):
    the kernels and torch add the same terms in different orders, so a small multiple; the floor - a few ulps of the largest
    element - covers cases where the float32 run happens to be exact (B = 1)"""
    return MARGIN * e_f32 + FLOOR


def recover_grad(m_new, theta_old, beta1, wd, m_old=None):
    """The gradient one Adam step took, from its first moment: m_new = beta1 * m_old + (1 - beta1) * (g + wd * theta_old)
    (torch.optim.Adam, coupled weight decay; m_old None: zero).  float64 arithmetic on the given (float32) values."""
    m_new, theta_old = m_new.detach().cpu().double(), theta_old.detach().cpu().double()
    if m_old is not None:
        m_new = m_new - beta1 * m_old.detach().cpu().double()
    return m_new / (1.0 - beta1) - wd * theta_old


# ---------------------------------------------------------------------------------------------------------------------------
# the cases: one seeded graph and parameter set per (F, E, R); batches drawn with replacement (duplicate centres occur)
# ---------------------------------------------------------------------------------------------------------------------------
BATCHES = [2049, 2048, 1025, 1024, 1023, 65, 64, 63, 17, 16, 15, 1, 17]       # descending; then 17 once more, after B = 1
BATCHES_SHORT = [2049, 1025, 65, 17, 1, 17]
# (F, E, R) -> (kernel, batch sizes, seed of the case: one at which every batch keeps AMBIGUOUS_CAP)
SHAPES = {
    (32, 64, 3): ("dense_step_kernel<true, 32, 64, 3>", BATCHES, 11),
    (25, 64, 3): ("dense_step_kernel<true, 25, 64, 3>", BATCHES, 11),
    (32, 128, 3): ("dense_step_kernel<false, 32, 128, 3>", BATCHES, 11),
    (25, 128, 3): ("dense_step_kernel<false, 25, 128, 3>", BATCHES, 11),
    (10, 16, 1): ("dense_step_kernel<false, 0, 0, 0>", BATCHES_SHORT, 11),
    (16, 48, 5): ("dense_step_kernel<false, 0, 0, 0>", BATCHES_SHORT, 11),
    (24, 16, 5): ("dense_step_kernel<true, 0, 0, 0>", BATCHES_SHORT, 12),
}
# Wide feature rows (the attribution tests parametrise over SHAPES: a table of its own keeps them as they are).  What each reaches
# in the dense kernel's staging prologue (csrc/dense.h: element e = r * 16 * F + t * F + f of a tile's [R][16][F] aggregates;
# the first 2048 elements are loaded two per thread, the rest by a loop with a summation of its own) and in the gather:
#   (100, 64, 3)  F > 64 self-row loop; the loop beyond for relation 1 from tile row 4 on and all of relation 2; stride 100
#   (68, 16, 2)   first width past 64; the loop beyond only for relation 1's tile rows 14 and 15; with the weights' LDS copy
#   (260, 16, 1)  two accumulators per lane (stride > 256): gather_train_kernel<2>; the loop beyond from tile row 7 / 8 on
#   (400, 16, 1)  the same without the weights' LDS copy; the loop beyond from tile row 5 / 6 on
# Every batch of these has the graph's hub rows pinned into it (wide_pins): only a set of more than 128 entries - several gather
# chunks - makes the staging code add partial sums, and random draws put one there in the largest batches only.
WIDE_SHAPES = {
    (100, 64, 3): ("dense_step_kernel<false, 0, 0, 0>", BATCHES_SHORT, 11),
    (68, 16, 2): ("dense_step_kernel<true, 0, 0, 0>", BATCHES_SHORT, 12),
    (260, 16, 1): ("dense_step_kernel<true, 0, 0, 0>", BATCHES_SHORT, 11),
    (400, 16, 1): ("dense_step_kernel<false, 0, 0, 0>", BATCHES_SHORT, 11),
}
WIDE_LDS_BYTES = {(100, 64, 3): 98432, (68, 16, 2): 63104, (260, 16, 1): 123392, (400, 16, 1): 101216}
REL_DEG = {1: (12,), 2: (12, 3), 3: (4, 12, 3), 4: (4, 12, 3, 6), 5: (4, 12, 3, 6, 2), 7: (4, 12, 3, 6, 2, 5, 3),
           8: (4, 12, 3, 6, 2, 5, 3, 8)}
MAX_BATCH = 2049
TILE_ROWS, STAGED_DIRECT, CHUNK = 16, 2048, 128     # rows of a dense tile | aggregate elements loaded two per thread | a gather chunk


def dense_smem_bytes(F, E, R, wlds):
    """dense_smem_bytes of csrc/dense.h, restated: the dense launch's dynamic LDS with / without the weights' copy"""
    kpad, tb, waves = 16, 16, 16
    k1p, k2p = (2 * F + kpad - 1) // kpad * kpad, (F + R * E + kpad - 1) // kpad * kpad
    ntile_e = E // 16
    kparts = waves // ntile_e if ntile_e <= waves else 1
    floats = R * tb * (k1p + 1) + tb * (k2p + 1) + (2 + R) * tb * (E + 1) + 4 * tb + 2 * E + 2 * F + 4 + 4
    floats += (k2p + R * k1p) * (E + 4) if wlds else kparts * tb * E
    return 4 * floats


def dense_wlds(F, E, R):
    """The dense kernel's rule for staging the weight matrices in LDS (dense_wlds / dense_smem_bytes in csrc/dense.h),
    restated: which of the two run-time-shape kernels a shape gets."""
    kpad, tb, waves = 16, 16, 16
    k1p = (2 * F + kpad - 1) // kpad * kpad
    ntile_e = E // 16
    kparts = waves // ntile_e if ntile_e <= waves else 1
    return (dense_smem_bytes(F, E, R, True) <= 160 * 1024 and (waves * 64) % (E // 4) == 0
            and kparts * tb * E <= R * k1p * (E + 4))


def infer_wlds(F, E, R):
    """infer_wlds of csrc/infer.hip, restated: a forward-only launch (whole-set inference, attribution) keeps the weights' LDS
    copy alive across tiles, so its K-split partial tiles go where the backward's dcomb / dh_r arrays are - if they fit there"""
    tb, waves = 16, 16
    ntile_e = E // 16
    kparts = waves // ntile_e if ntile_e <= waves else 1
    return dense_wlds(F, E, R) and kparts * tb * E <= (1 + R) * tb * (E + 1)


def attr_dcat_over_cat(F, E, R):
    """attr_dcat_over_cat of csrc/attr.hip, restated: dcat [R][16][2F + 1] lies over the forward's [self | h_1 .. h_R] tile"""
    k2p = (F + R * E + 15) // 16 * 16
    return R * (2 * F + 1) <= k2p + 1


def attr_dx0_over_comb(F, E):
    """attr_dx0_over_comb of csrc/attr.hip, restated: dx0 [16][F + 1] lies over `combined` [16][E + 1]"""
    return F <= E


def attr_smem_bytes(F, E, R):
    """attr_smem_bytes of csrc/attr.hip with the forward's own choice of the weights' copy, restated: the attribution launch's LDS"""
    extra = (0 if attr_dcat_over_cat(F, E, R) else R * 16 * (2 * F + 1)) + (0 if attr_dx0_over_comb(F, E) else 16 * (F + 1))
    return dense_smem_bytes(F, E, R, infer_wlds(F, E, R)) + 4 * extra


def attr_shape_ok(F, E, R):
    return attr_smem_bytes(F, E, R) <= 160 * 1024


# the four users of dense_tile_body and the six instantiations of each: four fixed shapes (the weights' LDS copy: a template
# argument the host's rule must agree with, else the shape falls through to the run-time kernels) and two run-time-shape ones
USERS = {"train": "dense_step_kernel", "vjp": "dense_vjp_kernel", "infer": "infer_dense_kernel", "attr": "attr_dense_kernel"}
FIXED = {(32, 64, 3): True, (25, 64, 3): True, (32, 128, 3): False, (25, 128, 3): False}
INSTANTIATIONS = [(True, 32, 64, 3), (True, 25, 64, 3), (False, 32, 128, 3), (False, 25, 128, 3), (True, 0, 0, 0), (False, 0, 0, 0)]


def kernel_of(user, F, E, R):
    """The instantiation a user's launch picks for a shape - launch_dense (csrc/dense.hip), pcg_dense_vjp (csrc/vjp.hip),
    launch_infer_dense (csrc/infer.hip), launch_attr_dense (csrc/attr.hip), restated - as the kernel's name; None: refused"""
    forward_only = user in ("infer", "attr")
    wlds = (infer_wlds if forward_only else dense_wlds)(F, E, R)
    if E < 16 or E % 16 or not 1 <= R <= 8 or dense_smem_bytes(F, E, R, wlds) > 160 * 1024:
        return None
    if user == "attr" and not attr_shape_ok(F, E, R):
        return None
    fixed = FIXED.get((F, E, R)) == wlds
    args = f"{str(wlds).lower()}, {F}, {E}, {R}" if fixed else f"{str(wlds).lower()}, 0, 0, 0"
    return f"{USERS[user]}<{args}" + ((", true>" if fixed else ", false>") if forward_only else ">")


# The fifth user: the fused launch of the pipelined training step (launch_dense_select, csrc/select.hip) - the same six shapes by
# training's rule, times PRE, the select half's presorted instantiation: twelve kernels.
FUSED_KERNEL = "dense_select_kernel"
PIPE_MAX_TILES, WG_KEYCAP, SEL_BLOCKS, SEL_SHARDS, RANK_MAX = 128, 10240, 768, 8, 16384


def dense_select_blocks(F, E, R, B, n_pos, max_degree, cus=None):
    """dense_select_blocks of csrc/select.hip, restated: the select workgroups of the fused launch beside the tiles of a batch of
    B rows, or 0 - the step keeps its three launches"""
    cus = EDGE_CUS if cus is None else cus
    if B < 1 or E < 16 or E % 16 or not 1 <= R <= 8:
        return 0
    n_tiles = (B + TILE_ROWS - 1) // TILE_ROWS
    if n_tiles > PIPE_MAX_TILES or (F + 3) // 4 * 4 > 256 or max_degree > WG_KEYCAP:
        return 0
    if dense_smem_bytes(F, E, R, dense_wlds(F, E, R)) > 160 * 1024:
        return 0
    n_sel = max(min(cus - n_tiles, SEL_BLOCKS), 0) // SEL_SHARDS * SEL_SHARDS
    n_sort = (n_pos + 63) // 64 if 0 < n_pos <= RANK_MAX else 0
    return n_sel if n_sel >= 64 and n_sel - 8 >= n_sort else 0


def fused_steps_ahead(F, E, R, B, n_pos, max_degree, switch, n_steps):
    """FusedPCGNN._ahead, restated: whether a pipelined sequence of n_steps batches of up to B rows steps the label classifier
    two batches ahead - the switch (clf_ahead), three steps or more, the keys a refresh leaves sorted (pcg_dense_sorts_keys; or
    none at all) and room for the sort riders (pcg_dense_select_ahead_ok)"""
    tiles, riders = (B + TILE_ROWS - 1) // TILE_ROWS, (n_pos + 63) // 64
    presort = 1 <= n_pos <= RANK_MAX and tiles + riders <= 256
    room = dense_select_blocks(F, E, R, B, n_pos, max_degree) > 0 and (n_pos <= 0 or (n_pos <= RANK_MAX and riders <= 4 * tiles))
    return bool(switch and n_steps >= 3 and (presort or n_pos == 0) and room)


def fused_kernel_of(F, E, R, B, n_pos, max_degree, ahead):
    """The instantiation launch_dense_select picks for the tiles of a batch of B rows beside a selection whose keys were sorted a
    launch earlier (ahead) or are sorted in the launch itself, as the kernel's name; None: the step is not pipelined"""
    if not dense_select_blocks(F, E, R, B, n_pos, max_degree):
        return None
    wlds = dense_wlds(F, E, R)
    args = f"{F}, {E}, {R}" if FIXED.get((F, E, R)) == wlds else "0, 0, 0"
    pre = ahead or not 0 < n_pos <= RANK_MAX           # (nothing for the select half to sort: sorted already, or no in-kernel sort)
    return f"{FUSED_KERNEL}<{str(wlds).lower()}, {args}, {str(bool(pre)).lower()}>"


# Edge shapes: what the host rules accept and the tables above do not reach.  Per shape: (the training kernel, batch sizes, seed
# of the case).  tests/test_edge_shapes_host.py re-derives every statement below from the restated rules:
#   (16, 64, 4)   the run-time LDS-weight kernels of all four users; R = 4
#   (30, 64, 3)   next to the fixed shapes (the dispatch falls through); F % 4 != 0 (stride 32)
#   (20, 128, 1)  LDS weights at E = 128 (kparts 2), R = 1
#   (20, 32, 7)   E = 32 (kparts 8), R = 7; attribution: dcat appended with dx0 over `combined`
#   (17, 32, 8)   R = PCG_MAX_REL with the weights' copy; odd F (stride 20)
#   (32, 64, 8)   R = 8 streamed; R * E / 16 = 32 h-tiles: two turns of the wave loop
#   (64, 64, 3)   attribution: dcat appended with dx0 over `combined`, streamed; the last width before the F > 64 staging loop
#   (16, 272, 1)  E / 16 = 17 > 16 waves: kparts 1, every E-tiled wave loop takes a second turn
EDGE_SHAPES = {
    (16, 64, 4): ("dense_step_kernel<true, 0, 0, 0>", BATCHES_SHORT, 12),
    (30, 64, 3): ("dense_step_kernel<true, 0, 0, 0>", BATCHES_SHORT, 11),
    (20, 128, 1): ("dense_step_kernel<true, 0, 0, 0>", BATCHES_SHORT, 11),
    (20, 32, 7): ("dense_step_kernel<true, 0, 0, 0>", BATCHES_SHORT, 11),
    (17, 32, 8): ("dense_step_kernel<true, 0, 0, 0>", BATCHES_SHORT, 11),
    (32, 64, 8): ("dense_step_kernel<false, 0, 0, 0>", BATCHES_SHORT, 11),
    (64, 64, 3): ("dense_step_kernel<false, 0, 0, 0>", BATCHES_SHORT, 11),
    (16, 272, 1): ("dense_step_kernel<false, 0, 0, 0>", BATCHES_SHORT, 11),
}
EDGE_TRAIN_SHAPES = [(16, 64, 4), (17, 32, 8), (16, 272, 1)]      # the first-moment train-step cases, at B = 17 and 1025
# the widest rows attribution accepts at (F, 16, 1) and the first it refuses -> seed of the case ((122 | 123, 64, 3): the same
# limit at the project's E and R, through the C ABI only)
ATTR_LIMIT_SHAPES = {(360, 16, 1): 11, (361, 16, 1): 11}
ATTR_LIMITS = [((360, 16, 1), (361, 16, 1)), ((122, 64, 3), (123, 64, 3))]
# what whole-set inference / embed and attribution run beyond EDGE_SHAPES
EDGE_INFER_SHAPES = list(EDGE_SHAPES) + [(260, 16, 1)]
EDGE_ATTR_SHAPES = list(EDGE_SHAPES) + [(100, 64, 3), (260, 16, 1), (360, 16, 1), (24, 16, 1)]
# (24, 16, 1): the attribution's fourth LDS overlay - dcat over the [self | h_1] tile with dx0 appended - which only R = 1 with
# E < F <= E + 8 and 2F <= K2p reaches; here dcat [16][49] fills the tile [16][K2p + 1] to the float.  -> seed of the case
ATTR_OVERLAY_SHAPES = {(24, 16, 1): 11}
# (the attribution batches are attr_ref.id_sets', with attr_ref.BATCH_SALT's salt per shape)
EDGE_CUS = 256                                       # an MI355X's; the host test draws the long id set for it
EDGE_SET_SIZES = lambda cus: (1, 17, 16 * cus + 17)  # a lone row, a ragged second tile, a second tile on every workgroup


def edge_id_sets(case, cus=EDGE_CUS):
    """n -> ids of the inference tests' sets: n = 1, 17 (no duplicates), 16 * CUs + 17 (drawn with replacement)"""
    rs = np.random.RandomState(case.seed * 7919 + 13)
    out = {}
    for n in EDGE_SET_SIZES(cus):
        out[n] = rs.choice(case.n, size=n, replace=False) if n <= 17 else rs.randint(0, case.n, size=n)
    return out


class GradCase:
    """The fields ``tests.util.build_model`` reads (n, f, emb, R, alpha, train_pos, X, params()) over a ``synth_graph`` of 2000
    nodes, ~15 % positives, the train positives those among the first half of the nodes; seeded Xavier-scale parameters."""
    lr, wd, rho, alpha = 0.01, 0.001, 0.5, 2.0
    betas = (0.9, 0.999)

    def __init__(self, F, E, R, seed=11):
        self.n, self.f, self.emb, self.R, self.seed = 2000, F, E, R, seed
        self.X, self.labels, self.csr = synth_graph(seed, self.n, F, REL_DEG[R], 0.15)
        self.train_pos = [int(v) for v in range(self.n // 2) if self.labels[v] == 1]
        gen = torch.Generator().manual_seed(seed + 1000 * F + 10 * E + R)
        shapes = {"weight": (2, E), "inter1.weight": (F + R * E, E), "inter1.label_clf.weight": (2, F), "inter1.label_clf.bias": (2,)}
        shapes.update({f"inter1.intra_agg{r + 1}.weight": (2 * F, E) for r in range(R)})
        self._params = {}
        for k in PARAM_KEYS(R):
            shp = shapes[k]
            # xavier_uniform_'s bound for the matrices, nn.Linear's 1 / sqrt(fan_in) for the label classifier
            bound = (6.0 / (shp[0] + shp[1])) ** 0.5 if "label_clf" not in k else 1.0 / F ** 0.5
            self._params[k] = ((torch.rand(shp, generator=gen) * 2 - 1) * bound).float()

    @classmethod
    def of(cls, shape):
        for table in (SHAPES, WIDE_SHAPES, EDGE_SHAPES):
            if shape in table:
                return cls(*shape, seed=table[shape][2])
        return cls(*shape, seed={**ATTR_LIMIT_SHAPES, **ATTR_OVERLAY_SHAPES}[shape])

    def params(self):
        return {k: v.clone() for k, v in self._params.items()}

    def batch(self, B, salt=0, pins=None):
        """(ids, labels) int64 numpy, drawn with replacement; pins {position: node}: those positions hold those nodes instead
        of their draws (the other positions are what they are without pins)"""
        rs = np.random.RandomState(self.seed * 100003 + 31 * B + salt)
        ids = rs.randint(0, self.n, size=B)
        for at, node in (pins or {}).items():
            ids[at] = node
        return ids, self.labels[ids]

    def hubs(self, k=2):
        """the k nodes of the highest total degree (synth_graph's hub first: it is the largest row of every relation)"""
        deg = sum(np.diff(indptr) for indptr, _ in self.csr)
        return [int(v) for v in np.argsort(-deg, kind="stable")[:k]]

    def wide_pins(self, B):
        """{position: node} that puts rows of several gather chunks where the staging loops differ: the hub at tile rows 0 and
        15 of the first tile, the second largest row at 1 and 14, and - a ragged batch - the hub on the last tile's first row;
        B = 1: the hub itself"""
        hub, second = self.hubs(2)
        if B < TILE_ROWS:
            return {0: hub}
        pins = {0: hub, 1: second, TILE_ROWS - 2: second, TILE_ROWS - 1: hub}
        if B % TILE_ROWS:
            pins[B // TILE_ROWS * TILE_ROWS] = hub
        return pins

    def wide_batch(self, B, salt=0):
        return self.batch(B, salt, pins=self.wide_pins(B))

    def host_sets(self, ids, labels, params=None):
        """the oracle's training-mode selection for a batch (CPU tests: no device to take the sets from)"""
        from oracle import pcgnn_oracle as O
        p = self._params if params is None else params
        X = torch.from_numpy(self.X)
        s0 = Fn.linear(X, p["inter1.label_clf.weight"].float(), p["inter1.label_clf.bias"].float())[:, 0]
        pos = torch.as_tensor(self.train_pos).long()
        sets = []
        for indptr, idx in self.csr:
            lists = [idx[indptr[v]:indptr[v + 1]].tolist() for v in ids]
            nsc = [s0[torch.as_tensor(l).long()] for l in lists]
            sets.append(O.choose_sets(s0[torch.as_tensor(ids).long()], labels.tolist(), lists, nsc, self.train_pos, s0[pos],
                                      0.5, self.rho, True))
        return sets


def staged_multi_chunk_rows(sets, F, B):
    """Where the dense kernel's staging prologue meets rows of several gather chunks (sets of more than 128 entries) in a batch:
    (rows the first 2048 aggregate elements of their tile cover, rows the loop beyond covers) as lists of (relation, batch row),
    from a row's elements [r * 16 * F + t * F, + F) of its tile; a row across the boundary is in both."""
    direct, beyond = [], []
    for r, rel in enumerate(sets):
        for b in range(B):
            if len(rel[b]) <= CHUNK:
                continue
            e0 = r * TILE_ROWS * F + (b % TILE_ROWS) * F
            if e0 < STAGED_DIRECT:
                direct.append((r, b))
            if e0 + F > STAGED_DIRECT:
                beyond.append((r, b))
    return direct, beyond


def reference_pair(case, ids, labels, sets, params=None, dev_masks=None):
    """The float64 reference and its float32 yardstick for one batch, with the ReLU-kink rule applied.  Returns
    (ref64, ref32, share of ambiguous activations, non-ambiguous entries where the device's mask is not the f64 sign)."""
    params = case.params() if params is None else params
    index = sets_to_index(sets)
    args = (case.X, ids, labels, index, params, case.alpha)
    plain64, plain32 = dense_ref(*args, dtype=torch.float64), dense_ref(*args, dtype=torch.float32)
    _, amb, share = ambiguous(plain64["pre"], plain32["pre"])
    masks, wrong = resolve_masks(plain64["pre"], amb, dev_masks)
    return dense_ref(*args, dtype=torch.float64, masks=masks), dense_ref(*args, dtype=torch.float32, masks=masks), share, wrong
