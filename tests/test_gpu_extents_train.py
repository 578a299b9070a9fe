"""No training kernel writes - or depends on a read - outside the buffer sizes include/pcgnn.h documents.

Every other GPU test allocates an engine's buffers with torch.empty / torch.zeros: the caching allocator rounds each request up
to 512 bytes, packs small buffers side by side, and most engines are built with max_batch 2049 or 256 and run at B = 17 - a
16-row tile that stores its tail rows past logits[B], or a size function a few hundred bytes short, is invisible there.  Here the
engine is built with ``max_batch == B`` inside ``tests.guarded.guarded_allocations``: every buffer of fused.py (logits [B, 2],
cnt [2, R, B], slabs [max(tiles, 8), n_params], acts [pcg_wgrad_act_rows, act_ld], pcg_wgrad_scratch_bytes, the plan slot of
pcg_choose_plan_bytes, the data part of pcg_choose_data_bytes, keys [pcg_pos_sort_capacity], the graph's own arrays ...) has
exactly the size the header's size function gives, starts at an address that is 256 mod 512, and lies between guard words.

Each test runs the same calls on a guarded engine and on a plain one and asserts
  (a) after every call, every byte of the arena outside the buffers handed out still holds the guard pattern, and
  (b) every output and every piece of engine state is ``torch.equal`` to the plain engine's - the read side: the plain engine
      sees zeros or a neighbour's data beyond an extent, the guarded one the pattern.
The guarded engine runs FIRST: a kernel that oversteps is caught between guard words, and the test ends, before the same call
runs on buffers that have no bands around them - where the stray store would land in whatever the allocator put next to them.

Shapes (dense_ref): (32, 64, 3) and (25, 128, 3) the two fixed-shape dense kernels, (10, 16, 1) / (24, 16, 5) the run-time-shape
kernel without / with the weights' LDS copy, (260, 16, 1) gather_train_kernel<2> (hub rows pinned: dense_ref.wide_pins).
B = 1, 15, 16, 17, 1025: a lone row, a tile less one, a whole tile, a tile and one, and the first size with a second label
classifier workgroup, act_ld above 1024 (the weight-gradient scratch in use) and 65 tiles.

Run with ``pytest -m gpu`` on an MI355X."""
import numpy as np
import pytest
import torch

from tests import dense_ref as D
from tests import vjp_ref as V
from tests.guarded import GuardedArena, guarded_allocations
from tests.util import PARAM_KEYS, build_model

pytestmark = pytest.mark.gpu

SHAPES = [(32, 64, 3), (25, 128, 3), (10, 16, 1), (24, 16, 5), (260, 16, 1)]
BATCHES = [1, 15, 16, 17, 1025]
STATE = ("theta", "m", "v", "step_counter", "clf_next")
MIB = 1 << 20


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def P():
    import pcgnn_amd
    from pcgnn_amd import ops  # noqa: F401  (fails loudly if the .so is missing)
    return pcgnn_amd


_CASES = {}


def case_of(shape):
    if shape not in _CASES:
        _CASES[shape] = D.GradCase.of(shape)
    return _CASES[shape]


def engine(P, c, B, **kw):
    from pcgnn_amd.fused import FusedPCGNN
    m = build_model(P, c, c.rho, graph=P.DeviceGraph(c.X, c.csr, c.train_pos, dev()))
    return FusedPCGNN(m, c.lr, c.wd, betas=c.betas, max_batch=B, **kw)


def on_dev(ids, lab):
    return torch.from_numpy(ids.astype(np.int32)).to(dev()), torch.from_numpy(lab.astype(np.int32)).to(dev())


def draw(c, shape, B, salt=0):
    return c.wide_batch(B, salt) if shape in D.WIDE_SHAPES else c.batch(B, salt)


def arena_bytes(c, B):
    """room for one engine: the selection list's worst case (every centre the hub, with its minority picks) and the gather's
    partial sums dominate; everything else is a few MiB"""
    deg = max(int(np.diff(ip).max()) for ip, _ in c.csr)
    per_row = deg + min(2 * deg, len(c.train_pos)) + 1
    lists = 4 * per_row * c.R * B
    return 64 * MIB + 3 * lists + lists // 128 * max(c.f, 128)


def in_arena(arena, t, nbytes):
    return 0 < arena.offset_of(t) < arena.nbytes and t.untyped_storage().nbytes() == nbytes and t.data_ptr() % 512 == 256


def assert_same(got, want):
    assert list(got) == list(want)
    for k in want:
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), f"{k}: the guarded engine's bits differ from the plain engine's"


def training_calls(fz, c, shape, B, check):
    """the calls of one engine; check(what) after every one.  -> name -> tensor"""
    out = {}
    loss_fn = V.focal_loss(c.alpha)
    ids, lab = on_dev(*draw(c, shape, B))
    ids2, lab2 = on_dev(*draw(c, shape, B, salt=1))

    def state(tag):
        for name in STATE:
            out[f"{tag}: {name}"] = getattr(fz, name).clone()
        out[f"{tag}: logits"], out[f"{tag}: center"] = fz.logits[:B].clone(), fz.center[:B].clone()
        out[f"{tag}: loss"] = fz.last_loss().clone()

    fz.train_step(ids, lab, defer=True)
    check("train_step(defer=True)")
    fz.flush()
    check("flush")
    state("step 1")
    # two deferred steps back to back: the first one's update rides in the second one's gather launch
    fz.train_step(ids2, lab2, defer=True)
    check("a second train_step(defer=True)")
    fz.train_step(ids, lab, defer=True)
    check("a deferred step whose predecessor's update rides in its gather launch")
    fz.flush()
    check("flush after the riding update")
    state("step 3")
    for via in ("acts", "slabs"):
        grads = fz.gradients(ids2, lab2, via=via)
        check(f"gradients(via={via!r})")
        for k, v in grads.items():
            out[f"gradients {via}: {k}"] = v
    gnn, center, comb = fz.predict(ids, None, False, want_combined=True)
    check("predict(want_combined=True), test mode")
    out["predict: gnn"], out["predict: center"], out["predict: combined"] = gnn, center, comb
    # forward + backward under autograd (pcg_dense_vjp + pcg_wgrad), then the same loss with the engine's Adam
    named = dict(fz.model.named_parameters())
    for k in PARAM_KEYS(c.R):
        named[k].grad = None
    gnn, center = fz.forward(ids2, lab2)
    check("forward")
    loss = loss_fn(gnn, center, lab2)
    loss.backward()
    check("backward (pcg_dense_vjp, pcg_wgrad)")
    out["forward: gnn"], out["forward: center"], out["forward: loss"] = gnn.detach().clone(), center.detach().clone(), loss.detach().clone()
    for k in PARAM_KEYS(c.R):
        out[f"backward: {k}"] = named[k].grad.clone()
        named[k].grad = None
    out["custom: returned loss"] = fz.train_step_custom(ids, lab, loss_fn).clone()
    check("train_step_custom")
    for name in STATE:
        out[f"custom: {name}"] = getattr(fz, name).clone()
    torch.cuda.synchronize()
    fz.check()
    check("the end")
    assert int(fz.step_counter.item()) == 4
    return out


def guarded_engine_buffers(arena, fz, B):
    """the engine's buffers are the arena's, at exactly the documented sizes"""
    lib, F, E, R = fz.lib, fz.F, fz.E, fz.R
    tiles = int(lib.pcg_dense_n_tiles(B))
    assert tiles == -(-B // 16) and fz.act_ld == 16 * tiles
    sizes = dict(logits=8 * B, center=8 * B, row_loss=4 * B, cnt2=4 * 2 * R * B, agg=4 * R * B * F, theta=4 * fz.n_params,
                 slabs=4 * max(tiles, 8) * fz.n_params, acts=4 * int(lib.pcg_wgrad_act_rows(F, E, R)) * fz.act_ld,
                 wg_scratch=int(lib.pcg_wgrad_scratch_bytes(F, E, R, fz.act_ld)),
                 keys=8 * int(lib.pcg_pos_sort_capacity(fz.g.n_pos)), s0=4 * fz.g.n_nodes,
                 data=int(lib.pcg_choose_data_bytes(fz.g.desc_ref(), B, fz.list_capacity)))
    for name, nbytes in sizes.items():
        assert in_arena(arena, getattr(fz, name), nbytes), f"{name}: not a guarded buffer of {nbytes} bytes"
    assert in_arena(arena, fz._plan_slot(B), int(lib.pcg_choose_plan_bytes(fz.g.desc_ref(), B, fz.list_capacity)))
    # fused.py takes parameter offsets from the views' storage offsets: they must be relative to theta itself
    for k, v in fz.views.items():
        assert v.data_ptr() == fz.theta.data_ptr() + 4 * v.storage_offset(), k


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_training_calls_keep_their_extents(P, shape, B):
    c = case_of(shape)
    arena = GuardedArena(arena_bytes(c, B), dev())
    with guarded_allocations(arena):
        fz = engine(P, c, B)
        arena.check("building the engine")
        got = training_calls(fz, c, shape, B, arena.check)
        guarded_engine_buffers(arena, fz, B)
    want = training_calls(engine(P, c, B), c, shape, B, lambda what: None)
    assert_same(got, want)


def need_of(g, thresholds, rho, ids, lab):
    """the sum of pcg_sel_capacity_row over the batch's train-mode rows (and ops.sel_capacity, its vectorised form); the same
    for a test-mode selection"""
    from pcgnn_amd import _lib, ops
    lib = _lib.load()
    need = 0
    for r in range(g.R):
        for v, y in zip(ids.tolist(), lab.tolist()):
            need += int(lib.pcg_sel_capacity_row(int(g.deg_host[r][v]), float(thresholds[r]), float(rho[r]), int(y == 1), g.n_pos, 0))
    assert need == int(ops.sel_capacity(g, ids, lab, thresholds, rho, True).sum())
    return need, int(ops.sel_capacity(g, ids, None, thresholds, 0.0, False).sum())


def one_step(fz, ids, lab, check):
    B = ids.numel()
    fz.train_step(ids, lab)
    check("train_step")
    out = {name: getattr(fz, name).clone() for name in STATE}
    out["logits"], out["center"], out["loss"] = fz.logits[:B].clone(), fz.center[:B].clone(), fz.last_loss().clone()
    return out


@pytest.mark.parametrize("B", [17, 1025])
def test_exact_fit_selection_list(P, B):
    """list_capacity == what the batch needs: the same bits as the default capacity; one entry less: the overflow is reported,
    nothing is written outside any buffer, and the engine works afterwards"""
    from pcgnn_amd import PcgnnLibraryError
    shape = (32, 64, 3)
    c = case_of(shape)
    ids_np, lab_np = draw(c, shape, B)
    ids, lab = on_dev(ids_np, lab_np)

    arena = GuardedArena(arena_bytes(c, B), dev())
    with guarded_allocations(arena):
        probe = engine(P, c, 1)                            # (its graph, thresholds and rho: what the need is computed from)
        need, need_test = need_of(probe.g, probe.thresholds, probe.rho, ids_np, lab_np)
        assert need_test < need, "the batch has minority picks: a test-mode selection fits a list of need - 1"
        fz = engine(P, c, B, list_capacity=need)
        assert fz.list_capacity == need
        assert fz.data.untyped_storage().nbytes() == int(fz.lib.pcg_choose_data_bytes(fz.g.desc_ref(), B, need))
        first = fz.predict(ids, None, False)
        arena.check("predict on the exact list")
        got = one_step(fz, ids, lab, arena.check)
        fz.check()

        short = engine(P, c, B, list_capacity=need - 1)
        pred = short.predict(ids, None, False)
        arena.check("predict on the short list")
        short.check()
        assert torch.equal(pred[0], first[0]) and torch.equal(pred[1], first[1])
        theta0 = short.theta.clone()
        short.train_step(ids, lab)
        arena.check("a training step whose selection list overflows")
        with pytest.raises(PcgnnLibraryError, match="selection list overflow"):
            short.check()
        arena.check("reading the overflow")
        # afterwards: from the parameters it started with, the engine predicts what it predicted
        short.flush()
        short.theta.copy_(theta0)
        short.params_changed()
        pred = short.predict(ids, None, False)
        arena.check("predict after the overflow")
        short.check()
        assert torch.equal(pred[0], first[0]) and torch.equal(pred[1], first[1])

    plain = engine(P, c, B)
    assert need < plain.list_capacity
    pred = plain.predict(ids, None, False)
    assert torch.equal(pred[0], first[0]) and torch.equal(pred[1], first[1])
    assert_same(got, one_step(plain, ids, lab, lambda what: None))


def test_whole_epoch_launch_keeps_its_extents(P):
    """Epoch plans, the two epoch buffer sets, graph capture and replay: one ``run_epoch_one_graph()`` of a trainer built inside
    the arena (the "mini" workload of tests/test_gpu_epoch_engine.py: 6000 nodes, batches of 256, a shorter last one)"""
    from pcgnn_amd import synth
    from pcgnn_amd.handler import PCGNNTrainer
    w = synth.make_workload("mini", 6000, 32, (4000, 30000, 90000), 0.12, seed=3)
    cfg = dict(engine="graph", batch_size=256, seed=5)

    def epoch(t, check):
        n = t.run_epoch_one_graph()
        check("run_epoch_one_graph")
        torch.cuda.synchronize()
        t.fused.check()
        assert n == t.pick_size and t.pick_size % 256 != 0
        out = {name: getattr(t.fused, name).clone() for name in STATE}
        out["ids"] = t.fused._ep_ids[:n].clone()
        out["logits"] = t.fused.logits[:t.fused._lastB].clone()
        return out

    arena = GuardedArena(256 * MIB, dev())
    with guarded_allocations(arena):
        t = PCGNNTrainer(w, dict(cfg), dev())
        theta0 = t.fused.theta.clone()
        arena.check("building the trainer")
        got = epoch(t, arena.check)
        f = t.fused
        assert in_arena(arena, f.logits, 8 * 256)
        for st in f._ep_sets:
            assert in_arena(arena, st["plans"], len(f._ep_batches) * f._plan_bytes(256))
            assert in_arena(arena, st["ids"], 4 * t.pick_size)
    plain = PCGNNTrainer(w, dict(cfg), dev())
    plain.fused.theta.copy_(theta0)                       # (the same parameters whatever the initialisation drew)
    plain.fused.params_changed()
    want = epoch(plain, lambda what: None)
    assert int(want["step_counter"].item()) == len(f._ep_batches) >= 3
    assert_same(got, want)
