"""Marked-row scoring (score_marked_body, csrc/common.h) at every row geometry, against pcg_score_table bit for bit.

(a) the front launch (front_a_kernel: pcg_step_scores_train, pcg_step_scores) with hand-made byte maps: feature widths on both
    sides of every lanes-per-row tier - 8 lanes (10, 25, 32), 16 (64), 32 (100), 64 (166, 256) and 64 with a second float4 chunk
    per lane (260, 400, 512; 256 | 260 is the boundary), ragged last float4s (10, 25, 166) - times table sizes round the 512-row
    mark group (1, 511, 512, 513, 5000) times mark densities chosen on purpose.  A marked row's score is pcg_score_table's bits,
    every other entry keeps its sentinel, and pcg_score_table itself is within test_feature_widths' bar (1e-4) of a float64
    X @ W0 + b0.  One table of 2 097 152 + 513 rows gives the 1024-workgroup grid a second turn of its grid-stride loop.
(b) the gather launch (gather_train_kernel<1> at widths 64, 100, 256; <2> at 260, 512 - SCORE_K 1 and 2): a touched-rows
    engine's s0 after a step is the whole-table score under the stepped classifier on every row the NEXT batch's map marks, and
    a short epoch leaves bit for bit the parameters and Adam state of an engine that scores the whole table."""
import numpy as np
import pytest
import torch

from tests import mark_ref as M

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
WIDTHS = [10, 25, 32, 64, 100, 166, 256, 260, 400, 512]
SIZES = [1, 511, 512, 513, 5000]
GROUP = 512


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def P():
    import pcgnn_amd
    from pcgnn_amd import ops  # noqa: F401  (fails loudly if the .so is missing)
    return pcgnn_amd


def lanes_per_row(stride):
    q, l = stride // 4, 8
    while l < q and l < 64:
        l *= 2
    return l


def test_widths_cover_every_geometry():
    geo = {}
    for F in WIDTHS:
        stride = (F + 3) // 4 * 4
        geo.setdefault((lanes_per_row(stride), stride > 256), []).append(F)
    assert sorted(geo) == [(8, False), (16, False), (32, False), (64, False), (64, True)]
    assert any(F % 4 for F in WIDTHS) and 256 in geo[(64, False)] and 260 in geo[(64, True)]


def self_loop_graph(P, X, train_pos):
    n = X.shape[0]
    return P.DeviceGraph(X, [(np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32))], train_pos, dev())


def mark_sets(n, rs):
    """name -> byte values [n] (uint8): the densities the issue lists"""
    out = {}
    out["all zero"] = np.zeros(n, dtype=np.uint8)
    out["all one"] = np.ones(n, dtype=np.uint8)
    m = np.zeros(n, dtype=np.uint8); m[0] = 1
    out["only row 0"] = m
    m = np.zeros(n, dtype=np.uint8); m[n - 1] = 1
    out["only row n - 1"] = m
    m = np.zeros(n, dtype=np.uint8)
    for k in range(-(-n // GROUP)):                      # one mark per group of 512, at a position that moves through the group
        m[min(k * GROUP + (k * 197 + 511) % GROUP, n - 1)] = 1
    out["one per group"] = m
    m = np.zeros(n, dtype=np.uint8)
    for k in range(0, -(-n // GROUP), 2):                # a full group next to an empty one
        m[k * GROUP:(k + 1) * GROUP] = 1
    out["full | empty groups"] = m
    out["random 1 %"] = (rs.rand(n) < 0.01).astype(np.uint8)
    out["random 50 %"] = (rs.rand(n) < 0.5).astype(np.uint8)
    m = (rs.rand(n) < 0.5).astype(np.uint8)
    m[m != 0] = np.where(rs.rand(int(m.sum())) < 0.5, 0x80, 0xFF).astype(np.uint8)
    out["bytes 0x80 / 0xFF"] = m
    return out


class FrontState:
    """the training state pcg_step_scores_train wants: theta holding the label classifier (W [2, F], b [2]), nothing pending"""

    def __init__(self, lib, F, W, b, E=16, R=1):
        from pcgnn_amd import _lib
        from pcgnn_amd.ops import _p
        n_params = int(lib.pcg_dense_n_params(F, E, R))
        self.theta = torch.zeros(n_params, device=dev())
        o_w, o_b = int(lib.pcg_dense_param_offset(F, E, R, 3, 0)), int(lib.pcg_dense_param_offset(F, E, R, 4, 0))
        self.theta[o_w:o_w + 2 * F] = W.reshape(-1)
        self.theta[o_b:o_b + 2] = b
        self.m, self.v = torch.zeros_like(self.theta), torch.zeros_like(self.theta)
        self.slabs = torch.zeros(4, n_params, device=dev())
        self.step = torch.zeros(1, dtype=torch.int32, device=dev())
        self.sync = torch.zeros(int(lib.pcg_sync_words_count()), dtype=torch.int32, device=dev())
        self.c = _lib.TrainState(theta=_p(self.theta), m=_p(self.m), v=_p(self.v), step_counter=_p(self.step), sync_words=_p(self.sync),
                                 slabs=_p(self.slabs), emb=E, hyper=_lib.AdamHyper(0.01, 0.9, 0.999, 1e-8, 0.0))


def check_scores(s0, full, marks_np, what):
    mk = torch.from_numpy(marks_np != 0).cuda()
    assert torch.equal(s0[mk].view(torch.int32), full[mk].view(torch.int32)), f"{what}: a marked row's score is the whole-table pass's bits"
    assert bool((s0[~mk] == SENTINEL).all()), f"{what}: an unmarked row keeps its sentinel"


def padded_map(lib, marks_np):
    n = marks_np.shape[0]
    buf = torch.zeros(int(lib.pcg_touched_bytes(n)), dtype=torch.uint8, device=dev())      # (padding zero: the builder's contract)
    buf[:n] = torch.from_numpy(marks_np).cuda()
    return buf


@pytest.mark.parametrize("feat", WIDTHS)
def test_front_launch_scores_exactly_the_marked_rows(P, feat):
    from pcgnn_amd import _lib
    lib, ops = _lib.load(), P.ops
    _p, st = ops._p, ops._stream(dev())
    rs = np.random.RandomState(1000 + feat)
    X = rs.randn(max(SIZES), feat).astype(np.float32)
    gen = torch.Generator().manual_seed(feat)
    W, b = torch.randn(2, feat, generator=gen), torch.randn(2, generator=gen)
    ref64 = X.astype(np.float64) @ W[0].double().numpy() + float(b[0].double())
    W, b = W.cuda(), b.cuda()
    state = FrontState(lib, feat, W, b)
    for n in SIZES:
        g = self_loop_graph(P, X[:n], sorted({0, n // 2, n - 1}))
        full = ops.score_table(g, W, b)
        np.testing.assert_allclose(full.cpu().numpy(), ref64[:n], rtol=0, atol=1e-4)      # (test_feature_widths' bar)
        keys = torch.zeros(int(lib.pcg_pos_sort_capacity(g.n_pos)), dtype=torch.int64, device=dev())
        for what, marks in mark_sets(n, rs).items():
            tmap = padded_map(lib, marks)
            s0 = torch.full((n,), SENTINEL, device=dev())
            _lib.check(lib.pcg_step_scores_train(g.desc_ref(), state.c, _p(s0), _p(keys), _p(tmap), st), "pcg_step_scores_train")
            torch.cuda.synchronize()
            check_scores(s0, full, marks, f"feat {feat} n {n} {what}")
        if n == max(SIZES):                              # the same launch without a training state: pcg_step_scores
            marks = mark_sets(n, rs)["random 50 %"]
            s0 = torch.full((n,), SENTINEL, device=dev())
            _lib.check(lib.pcg_step_scores(g.desc_ref(), _p(W), _p(b), 0, n, _p(s0), None, _p(keys), -1, _p(state.sync), _p(padded_map(lib, marks)),
                                           st), "pcg_step_scores")
            torch.cuda.synchronize()
            check_scores(s0, full, marks, f"feat {feat} n {n} pcg_step_scores")
    assert int(state.step.item()) == 0 and not bool(state.m.any()), "no update was pending: the state is as it was"


def test_front_launch_second_grid_stride_turn(P):
    """2 097 152 + 513 rows of 4 features (34 MB): the launch has 1024 score workgroups of 4 waves, a wave takes 512 rows at a
    time - 2 097 152 rows per turn of the grid-stride loop -, so the last 513 rows (a whole group and a group of one row) are
    scored in the second turn."""
    from pcgnn_amd import _lib
    lib, ops = _lib.load(), P.ops
    _p, st = ops._p, ops._stream(dev())
    per_turn = 1024 * 4 * GROUP
    n, feat = per_turn + 513, 4
    rs = np.random.RandomState(7)
    X = rs.standard_normal((n, feat)).astype(np.float32)
    W = torch.tensor([[0.5, -1.25, 2.0, 0.75], [1.0, 1.0, 1.0, 1.0]])
    b = torch.tensor([0.125, -3.0])
    ref64 = X.astype(np.float64) @ W[0].double().numpy() + float(b[0])
    W, b = W.cuda(), b.cuda()
    g = self_loop_graph(P, X, [])
    assert g.n_pos == 0
    full = ops.score_table(g, W, b)
    np.testing.assert_allclose(full.cpu().numpy(), ref64, rtol=0, atol=1e-4)
    marks = (rs.rand(n) < 0.001).astype(np.uint8)
    edge = [0, GROUP - 1, GROUP, per_turn - GROUP, per_turn - 1, per_turn, per_turn + 1, per_turn + 300, per_turn + GROUP - 1, per_turn + GROUP]
    marks[edge] = 1
    assert edge[-1] == n - 1 and int(marks[per_turn:].sum()) >= 5 and int(marks.sum()) < n // 100
    state = FrontState(lib, feat, W, b)
    s0 = torch.full((n,), SENTINEL, device=dev())
    _lib.check(lib.pcg_step_scores_train(g.desc_ref(), state.c, _p(s0), None, _p(padded_map(lib, marks)), st), "pcg_step_scores_train")
    torch.cuda.synchronize()
    check_scores(s0, full, marks, "second turn")


# ---- (b) the gather launch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feat", [64, 100, 256, 260, 512])
def test_gather_launch_scores_the_next_batch_rows(P, feat, monkeypatch):
    from pcgnn_amd import synth
    from pcgnn_amd.handler import PCGNNTrainer
    ops = P.ops
    w = synth.make_workload("touched", 3000, feat, (20000,), 0.12, seed=4)
    cfg = dict(engine="graph", batch_size=96, seed=6, emb_size=16)
    monkeypatch.setenv("PCG_TOUCHED", "0")
    a = PCGNNTrainer(w, cfg, dev())
    monkeypatch.setenv("PCG_TOUCHED", "1")
    t = PCGNNTrainer(w, cfg, dev())
    assert t.fused.touched_on and not a.fused.touched_on
    t.fused.theta.copy_(a.fused.theta)
    t.fused.params_changed()
    nb = t.batches_per_epoch()
    assert nb >= 3 and a.batches_per_epoch() == nb
    ids_a, ids_t = a.start_epoch_staged(), t.start_epoch_staged()
    assert torch.equal(ids_a, ids_t)
    fz, n, k = t.fused, w.n, 0
    stride = fz._touch_stride
    clf_start = fz.clf_next.clone()
    fz.epoch_step(k, defer=True)                         # batch k; its gather launch scores the rows batch k + 1 can read
    torch.cuda.synchronize()
    marks = fz._ep_sets[fz._cur]["touched"][(k + 1) * stride:(k + 2) * stride]
    want = M.touched_ids(w.csr, w.train_pos, ids_t.cpu().numpy(), 96, n)[k + 1]
    assert np.array_equal(torch.nonzero(marks).view(-1).cpu().numpy(), want) and 0 < len(want) < n
    W, b = fz.clf_next[:2 * feat].view(2, feat), fz.clf_next[2 * feat:2 * feat + 2]
    assert not torch.equal(fz.clf_next, clf_start), "the step has moved the classifier on"
    full = ops.score_table(fz.g, W, b)
    mk = marks[:n].bool()
    assert torch.equal(fz.s0[mk].view(torch.int32), full[mk].view(torch.int32)), "marked rows: the stepped classifier's whole-table scores"
    # the rest of the epoch on this engine, the whole epoch on the whole-table one: the same parameters and Adam state
    for j in range(k + 1, nb):
        fz.epoch_step(j, defer=True)
    for j in range(nb):
        a.fused.epoch_step(j, defer=True)
    a.fused.flush(); fz.flush()
    torch.cuda.synchronize()
    fz.check()
    a.fused.check()
    for name in ("theta", "m", "v", "step_counter"):
        assert torch.equal(getattr(a.fused, name), getattr(fz, name)), name
    assert int(fz.step_counter.item()) == nb and bool(torch.isfinite(fz.theta).all())
