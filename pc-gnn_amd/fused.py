"""Whole-step driver: every launch of one PC-GNN train step, back to back on one
stream, no torch ops and no host synchronisation in between - three launches:

    select_rows          [the train positives' sort by its first workgroups || the label classifier's own step for this batch
                          (one workgroup: forward, loss gradient, Adam) || every row's selection]
    gather_train_kernel  [gather || Adam of the previous step's gradient (all but the label classifier) || the NEXT step's score
                          pass and train-pos keys, with the classifier the select launch has just stepped]
    dense_step           [sums of multi-chunk rows, forward, loss, backward partials (per-tile slabs)]

(``pcg_choose_gather_train`` / ``pcg_train_dense(adam_clf = 2)``; the first step after anything else has run is preceded by one
score launch, ``pcg_step_scores``).  Why this order is legal: the label classifier's parameters get gradient from nothing but
the centres' feature rows and labels, so its step does not have to wait for the dense kernel - and the scores the next batch is
selected by can be formed beside this batch's gather instead of at the head of the next step.  ``clf_next`` is that classifier,
one step ahead of theta's copy (which the current step's loss term is computed with); ``flush()`` makes them equal;
``params_changed()`` after parameters were written from outside.

The PLAN of a batch (row records, list
offsets, tier queues, the gather's chunk table) depends only on the batch's ids, labels and the CSR degrees - not on any
parameter - so it is not part of a step: ``pcg_plan_batches`` plans every batch of an epoch in ONE launch right after the
sampler (one plan slot per batch; the selection list and the partial sums - the data part - are shared).  A deferred Adam
update is flushed (``pcg_adam_flush``) before any public call returns unless the caller asks otherwise, so the parameters a
caller sees are always complete.  The same sequence is captured into hipGraphs (``torch.cuda.CUDAGraph``) - per batch, or a
whole epoch in one - so that a step costs no host work at all.

The model's parameters are re-pointed into ONE flat f32 buffer (order: see
``pcg_dense_step`` in include/pcgnn.h); the ``nn.Parameter`` objects, their names
and ``state_dict()`` stay exactly the reference's.

Another objective or optimizer than the reference's stays on this path too: ``forward`` returns the two logit tensors under
autograd (the backward is ``pcg_dense_vjp`` - the dense kernel's backward from the caller's loss gradients - and ``pcg_wgrad``),
``optimizer_step`` lets any ``torch.optim`` optimizer write the flat buffer, ``train_step_custom`` keeps the engine's Adam.

The whole-set calls over the resident graph and over query batches (``infer``, ``chosen``, ``attribute``, ``embed``, ``nearest``,
``evaluate``, the ``*_new`` forms) and their host planner live in wholeset.py; ``FusedPCGNN`` inherits them (``WholeSetCalls``).
The hipGraph capture and the staged-epoch engine (``train_step_graph``, ``stage_epoch`` .. ``epoch_run``) live in epoch.py
(``EpochCalls``); the launches of a step - every ``_enqueue_*`` - are here.

Reference loop replaced: src/model_handler.py:147-153 (and :305 of utils.py for
``predict``).
"""
import ctypes as C
import os
from contextlib import contextmanager
from typing import Dict, Optional

import torch

from . import _lib, ops
from .epoch import EpochCalls
from .graph import DeviceGraph
from .model import PCALayer
from .wholeset import (WholeSetCalls, default_infer_chunk, infer_chunks, infer_row_caps, whole_set_buffers,  # noqa: F401
                       whole_set_chunk, whole_set_ids, whole_set_workspace)

_p = ops._p


def default_list_capacity(g: DeviceGraph, B: int, max_list_bytes: int = 8 << 30):
    """Worst case of the graph for a batch of B (every centre being the largest hub), clipped to ``max_list_bytes``:
    kept <= deg, minority m = int(ceil(deg / 2) * rho) <= 2 * deg for rho <= 4 (and <= n_pos), +1 self.
    Returns (entries, clipped)."""
    per_row = g.max_degree + min(2 * max(g.max_degree, 1), g.n_pos) + 1
    worst = per_row * g.R * max(B, 1)
    cap = min(worst, max_list_bytes // 4, (1 << 31) - 1)
    return int(max(cap, 1)), cap < worst


class _SeededDense(torch.autograd.Function):
    """FusedPCGNN.forward under autograd: the engine's train-mode forward as a function of the model's parameters.  The backward
    hands the loss gradients of the two logit tensors to pcg_dense_vjp + pcg_wgrad (FusedPCGNN._enqueue_vjp); the ids, labels and
    the selection get no gradient (the selection is index-only: the reference does not differentiate it either)."""

    @staticmethod
    def forward(ctx, fz, ids, labels, train_flag, *params):
        gnn, center = fz._forward_live(ids, labels, train_flag)
        ctx.fz, ctx.serial = fz, fz._live["serial"]
        return gnn, center

    @staticmethod
    def backward(ctx, d_gnn, d_center):
        fz = ctx.fz
        flat = fz._enqueue_vjp(fz._live_of(ctx.serial), d_gnn, d_center)
        return (None, None, None, None) + tuple(fz._by_name(flat).values())


class FusedPCGNN(EpochCalls, WholeSetCalls):
    def __init__(self, model: PCALayer, lr: float, weight_decay: float, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_batch: int = 1024, global_batch_scale: int = 1, list_capacity: Optional[int] = None,
                 pipeline: Optional[bool] = None, infer_workspace_bytes: int = 1 << 30, clf_ahead: Optional[bool] = None):
        lib = _lib.load()
        self.lib = lib
        self.model = model
        inter = model.inter1
        self.g: DeviceGraph = inter.graph()
        g = self.g
        self.dev = g.device
        self.F, self.E, self.R = g.feat_dim, inter.embed_dim, g.R
        self.lr, self.wd, self.betas, self.eps = lr, weight_decay, betas, eps
        self.lambda_1 = float(model.lambda_1)
        self.scale = global_batch_scale           # ranks sharing one global batch (loss is a mean over all of it)
        self.thresholds = list(inter.thresholds)
        self.rho = [a.rho for a in inter.intra_aggs]

        n = lib.pcg_dense_n_params(self.F, self.E, self.R)
        self.n_params = int(n)
        self.theta = torch.zeros(n, dtype=torch.float32, device=self.dev)
        named = dict(model.named_parameters())
        spec = [("weight", 0, 0), ("inter1.weight", 1, 0)] + \
               [(f"inter1.intra_agg{r + 1}.weight", 2, r) for r in range(self.R)] + \
               [("inter1.label_clf.weight", 3, 0), ("inter1.label_clf.bias", 4, 0)]
        self.views: Dict[str, torch.Tensor] = {}
        for name, which, rel in spec:
            p = named[name]
            off = lib.pcg_dense_param_offset(self.F, self.E, self.R, which, rel)
            view = self.theta[off:off + p.numel()].view(p.shape)
            view.copy_(p.data.to(self.dev))
            p.data = view                      # the Parameter now lives inside the flat buffer
            self.views[name] = view
        self._params = [named[name] for name, _, _ in spec]     # the Parameters behind self.views, in its order (forward()'s inputs)
        self._live = None          # forward(): the one forward whose plan, lists, aggregates and counts are still in the workspace
        self._live_serial = 0
        self.w_clf = self.views["inter1.label_clf.weight"]
        self.b_clf = self.views["inter1.label_clf.bias"]
        self.m = torch.zeros_like(self.theta)
        self.v = torch.zeros_like(self.theta)
        self.step_counter = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.grad = torch.zeros_like(self.theta)
        # [ticket of the dense kernel, update pending, its slab count, group counter of the select kernel's in-kernel sort | its
        #  rank accumulators and group tickets]
        self.sync = torch.zeros(int(lib.pcg_sync_words_count()), dtype=torch.int32, device=self.dev)
        self.n_rest = int(lib.pcg_dense_param_offset(self.F, self.E, self.R, 3, 0))   # parameters before the label classifier
        # The label classifier is stepped on its own, one step ahead of the rest (pcg_choose_gather_train): clf_next is the
        # classifier the NEXT select launch scores by; theta's copy is the one the current step's loss is computed with.  flush()
        # makes them equal.  _fresh: s0 / the unsorted train-pos keys hold the scores of clf_next (a training step with
        # score_next leaves them so); anything else that touches s0, the keys or the parameters clears it.
        self.clf_next = self.theta[self.n_rest:].clone()
        self._fresh = False
        # model.load_state_dict writes the parameters behind the engine's back (they are views into theta): a deferred update
        # is applied first, the stepped classifier and the score table are taken from theta again afterwards
        model.register_load_state_dict_pre_hook(lambda *a, **k: self.flush())
        model.register_load_state_dict_post_hook(lambda *a, **k: self.params_changed())

        # Score only the rows a batch's selection can read (its centres and their neighbours: a byte map per batch, built per epoch
        # beside the plans) instead of the whole table - worth it when the table is far larger than what a batch touches
        # (PCG_TOUCHED=0/1 overrides; default: tables of 512 MB and more.  Measured, power-law graphs, batch 4096: 10 M nodes
        #  (1.28 GB): score pass 232 -> 63 us per step for ~35 us per step of map building; 2 M nodes (256 MB): 48 -> 25 us for
        #  ~30 us - not worth it there)
        env = os.environ.get("PCG_TOUCHED")
        self.touched_on = (env == "1") if env in ("0", "1") else g.n_nodes * g.X.stride(0) * 4 >= (512 << 20)
        self._touch_stride = int(lib.pcg_touched_bytes(g.n_nodes)) if self.touched_on else 0
        self._list_capacity_arg = list_capacity  # entries of the selection list (None: worst case of the graph)
        # Pipelined steps (epoch_run): batch t + 1's selection runs in ONE launch with batch t's dense tiles, on the CUs they leave
        # idle - two launches per step instead of three (pcg_dense_select_train; batches of up to 128 tiles, whole-table scoring).
        # pipeline=None: on unless PCG_PIPELINE=0 (A/B runs)
        env = os.environ.get("PCG_PIPELINE")
        self.pipeline = bool(pipeline) if pipeline is not None else env != "0"
        # ... with the label classifier stepped TWO batches ahead (_enqueue_pipelined_ahead): every select of a sequence finds its
        # train-pos keys sorted a launch earlier.  It costs three launches more at the start of a sequence and saves the select
        # half its in-kernel sort and the positive rows' wait for it, which grow with the number of keys: clf_ahead=None / no
        # PCG_CLF_AHEAD: on for graphs of 1024 train positives and more (measured: YelpChi-like, 2.7 K keys, 39.1 -> 37.4 us per
        # step; Amazon-like, 0.3 K keys and 24-step sequences, 27.1 -> 27.5: off there); True / False, PCG_CLF_AHEAD=1 / 0: forced
        env = os.environ.get("PCG_CLF_AHEAD")
        if clf_ahead is not None:
            self.clf_ahead = bool(clf_ahead)
        elif env in ("0", "1"):
            self.clf_ahead = env == "1"
        else:
            self.clf_ahead = g.n_pos >= 1024
        self.status = torch.zeros(1, dtype=torch.int32, device=self.dev)   # ONE device status word
        self._init_epoch_state()   # (captured graphs, the two sets of epoch buffers: _alloc clears them)
        self._thr, self._rhos = ops._host_arrays(g, self.thresholds, self.rho)
        self._hyper = _lib.AdamHyper(lr, betas[0], betas[1], eps, weight_decay)
        self._alloc(max_batch)
        self._prof = None          # bench.py: list of (start, end) events around the choose+aggregate launch
        self.last_counts = None
        # infer(): a workspace of its own (score table, plan slots, data part, aggregates, counts, status word), grown on demand;
        # its default chunk keeps the workspace within infer_workspace_bytes
        self.infer_workspace_bytes = int(infer_workspace_bytes)
        self._inf = {}
        # infer_new(): the base table's scores are kept across calls and reused while theta is what they were computed with.
        # _param_version counts the host calls that enqueue a write of theta (training steps, epoch runs, a flush with an update
        # pending, params_changed / a loaded state dict); _theta_dirty: such a call may have left a deferred update for flush()
        self._param_version = 0
        self._theta_dirty = False
        self._new_scored_base = None
        # utils.test / test_f1 evaluate through infer() - unless the caller bounded the selection list (list_capacity): infer()
        # sizes its own list exactly, so such an engine keeps the per-batch predict loop, whose batches report an overflow
        self.eval_by_infer = list_capacity is None

    # ------------------------------------------------------------------
    def _alloc(self, B: int):
        g, dev, lib = self.g, self.dev, self.lib
        if torch.cuda.is_current_stream_capturing():
            raise _lib.PcgnnLibraryError("batch larger than max_batch inside a graph capture: allocate before capturing")
        self._drop_prepared()                        # (an epoch prepared ahead goes with its buffers)
        self._live = None
        # every captured graph holds raw pointers into the buffers replaced below
        self._graphs.clear()
        self._ep_graphs.clear()
        self._ep_sets = None
        self._fresh = False
        self.maxB = B
        if self._list_capacity_arg is None:
            self.list_capacity, self.clipped = default_list_capacity(g, B)
        else:
            self.list_capacity, self.clipped = int(max(self._list_capacity_arg, 1)), False
        self.s0 = torch.empty(g.n_nodes, dtype=torch.float32, device=dev)
        self.keys = torch.empty(lib.pcg_pos_sort_capacity(g.n_pos), dtype=torch.int64, device=dev)
        nbytes = lib.pcg_choose_data_bytes(g.desc_ref(), B, self.list_capacity)
        if nbytes < 0:
            raise _lib.PcgnnLibraryError("pcg_choose_data_bytes rejected the arguments")
        self.data = torch.zeros(int(nbytes), dtype=torch.uint8, device=dev)     # list | partial sums | key scratch: shared by every plan
        self._plans = {}                                                        # batch size -> a single plan slot (calls outside an epoch)
        self._touch_one = None                                                  # ... and their byte map of touched rows
        self.agg = torch.empty(g.R, B, g.feat_dim, dtype=torch.float32, device=dev)
        # two count buffers: a pipelined step's fused launch selects batch t + 1 (its counts into one) while batch t's dense tiles
        # read the other; every other step uses the first
        self.cnt2 = torch.empty(2, g.R, B, dtype=torch.int32, device=dev)
        self.cnt = self.cnt2[0]
        # the classifier each pipelined step's dense tiles read: a ring of three (the tiles of t read the one batch t was selected
        # with while the steps of t + 1 and t + 2 have left theirs: _enqueue_pipelined_ahead; _enqueue_pipelined uses two)
        self.clf_slots = torch.empty(3, 2 * self.F + 2, dtype=torch.float32, device=dev)
        # the second score table / key buffer of a sequence whose classifier runs two batches ahead: batch t + 2's scores and keys
        # are written while batch t + 1's are still to be read.  Scratch of a sequence: it begins and ends on s0 / keys
        self.s0_alt = torch.empty_like(self.s0)
        self.keys_alt = torch.empty_like(self.keys)
        self._pipe_blocks = int(lib.pcg_dense_select_blocks(g.desc_ref(), self.E, B))
        self.logits = torch.empty(B, 2, dtype=torch.float32, device=dev)
        self.center = torch.empty(B, 2, dtype=torch.float32, device=dev)
        self.row_loss = torch.zeros(B, dtype=torch.float32, device=dev)
        self.slabs = torch.empty(max(lib.pcg_dense_n_tiles(B), 8), self.n_params, dtype=torch.float32, device=dev)
        # the training step's dense kernel leaves no gradient slabs: it leaves the step's activations / activation gradients,
        # transposed ([rows][act_ld], a batch row per column), and the weight gradients are GEMMs over the batch riding in the next
        # step's gather launch (pcg_train_dense(adam_clf = 3), wgrad.h).  (slabs: the gradient-only paths - gradients(via="slabs"),
        # data-parallel all-reduce - and the classifier step's scratch)
        self.act_ld = 16 * int(lib.pcg_dense_n_tiles(B))
        self.acts = torch.zeros(int(lib.pcg_wgrad_act_rows(self.F, self.E, self.R)), self.act_ld, dtype=torch.float32, device=dev)
        self.wg_scratch = torch.zeros(int(lib.pcg_wgrad_scratch_bytes(self.F, self.E, self.R, self.act_ld)) // 4, dtype=torch.float32, device=dev)
        # One dense workgroup per 16 rows leaves most CUs of a batch of <= ~3000 rows idle: the dense launch then also SORTS the
        # next step's train-pos keys (formed beside the gather before it), and the select launch that follows is told so - it
        # sorts nothing, no row waits for the sort, a positive hub row's window search runs beside its key pass.  The engine's
        # invariant in this mode: whenever s0 / the keys are fresh (_fresh) the keys are SORTED (a refresh sorts them itself).
        self.presort = bool(lib.pcg_dense_sorts_keys(B, g.n_pos)) and os.environ.get("PCG_PRESORT", "1") != "0"
        self.ids_buf = torch.zeros(B, dtype=torch.int32, device=dev)
        self.lab_buf = torch.zeros(B, dtype=torch.int32, device=dev)
        self._bind()

    def _bind(self):
        """The parameter structs of the training calls (include/pcgnn.h), built where the buffers they point to are allocated;
        a call fills only its batch.  A member that one call wants NULL and another set: two instances."""
        own = dict(theta=_p(self.theta), m=_p(self.m), v=_p(self.v), sync_words=_p(self.sync), emb=self.E, act_ld=self.act_ld,
                   lambda_1=self.lambda_1, hyper=self._hyper)
        self._st = _lib.TrainState(step_counter=_p(self.step_counter), clf_next=_p(self.clf_next), slabs=_p(self.slabs),
                                   acts=_p(self.acts), wg_scratch=_p(self.wg_scratch), **own)
        self._st_fwd = _lib.TrainState(**own)       # pcg_train_dense forward only: no gradient, no step counted
        # pcg_wgrad(apply = 0): the gradient of the activations at hand, no parameter is read or written
        self._st_grad = _lib.TrainState(acts=_p(self.acts), wg_scratch=_p(self.wg_scratch), emb=self.E, act_ld=self.act_ld,
                                        hyper=self._hyper)
        self._sel = _lib.SelectWs(self._thr, self._rhos, _p(self.data), _p(self.status), self.list_capacity, 0)
        self._out = _lib.DenseOut(_p(self.logits), _p(self.center), None, _p(self.row_loss))

    def _batch(self, ids, labels, B, plan: Optional[int] = None, cnt=None) -> _lib.Batch:
        return _lib.Batch(_p(ids), _p(labels), _p(cnt), plan, B, 1.0 / (max(B, 1) * self.scale))

    def _stream(self):
        return ops._stream(self.dev)

    def _agg_of(self, B) -> torch.Tensor:
        """the aggregates of a batch of B: the front of ``agg`` as [R, B, F]"""
        R, F = self.R, self.F
        return self.agg.view(-1)[:R * B * F].view(R, B, F)

    def _cnt_of(self, B, p: int = 0) -> torch.Tensor:
        """the kept counts of a batch of B in count buffer p, flat (``last_counts`` is the [R, B] view of the same storage)"""
        return self.cnt2[p].view(-1)[:self.R * B]

    def _fit(self, B, flush: bool = True):
        """Grow every buffer for a batch above max_batch.  A deferred update is applied first - it lives in buffers that are
        replaced; flush=False: the caller has flushed already."""
        if B > self.maxB:
            if flush:
                self.flush()
            self._alloc(B)

    @contextmanager
    def _bracket(self, always: bool = False):
        """Two timing events around the launches made inside, appended to ``_prof`` as a (start, end) pair (bench.py).  Nothing is
        recorded while ``_prof`` is None or the stream is capturing.  always: the events are recorded whatever ``_prof`` is - a
        timed sequence of graph replays costs the same with and without a reader - and appended only if it is set."""
        if not always and (self._prof is None or torch.cuda.is_current_stream_capturing()):
            yield
            return
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        yield
        ev[1].record()
        if self._prof is not None:
            self._prof.append(ev)

    @contextmanager
    def _choosing(self, B):
        """What the two select + gather calls share: -> (aggregates [R, B, F], flat counts) of the batch for the library call
        made inside, which is bracketed for ``_prof``; afterwards ``last_counts`` names the counts it wrote."""
        self._live = None                            # (lists, aggregates and counts are overwritten)
        agg, cnt = self._agg_of(B), self._cnt_of(B)
        with self._bracket():
            yield agg, cnt
        self.last_counts = cnt.view(self.R, B)

    def _plan_bytes(self, B):
        n = self.lib.pcg_choose_plan_bytes(self.g.desc_ref(), B, self.list_capacity)
        if n < 0:
            raise _lib.PcgnnLibraryError("pcg_choose_plan_bytes rejected the arguments")
        return int(n)

    def _plan_slot(self, B) -> torch.Tensor:
        """the plan slot of calls that are not part of a staged epoch (one per batch size: the layout depends on it)"""
        buf = self._plans.get(B)
        if buf is None:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.PcgnnLibraryError("a new batch size inside a graph capture: warm up before capturing")
            buf = self._plans[B] = torch.zeros(self._plan_bytes(B), dtype=torch.uint8, device=self.dev)
        return buf

    # ------------------------------------------------------------------
    def _enqueue_plan(self, ids, labels, n_total, B, plans: torch.Tensor, stride: int, train_flag, bump_counter=None, n_epochs: int = 1):
        """the plans of the batches ids[s * B : (s + 1) * B] (s < ceil(n_total / B)) - of every one of n_epochs epochs of n_total
        picks each -, one launch"""
        _lib.check(self.lib.pcg_plan_epochs(
            self.g.desc_ref(), _p(ids), _p(labels if train_flag else None), n_total, n_epochs, B, self._thr, self._rhos,
            1 if train_flag else 0, 0, _p(plans), stride, self.list_capacity, _p(self.status), _p(bump_counter), self._stream()),
            "pcg_plan_epochs")

    def _enqueue_plan_one(self, ids, labels, B, train_flag) -> int:
        """plan of ONE batch into this batch size's own slot (+ its touched-row map); returns the slot's address"""
        slot = self._plan_slot(B)
        self._live = None                            # (the slot of a forward() still waiting for its backward is overwritten)
        self._enqueue_plan(ids, labels, B, B, slot, slot.numel(), train_flag)
        if self.touched_on and train_flag:
            if self._touch_one is None:
                if torch.cuda.is_current_stream_capturing():
                    raise _lib.PcgnnLibraryError("first use of the touched-row map inside a graph capture: warm up before capturing")
                self._touch_one = torch.zeros(self._touch_stride, dtype=torch.uint8, device=self.dev)
            self._enqueue_mark(ids, B, B, self._touch_one, slot.data_ptr(), slot.numel())
        return slot.data_ptr()

    def _enqueue_mark(self, ids, n_total, B, maps: torch.Tensor, plans: int, stride: int):
        """byte maps of the rows each batch's selection can read, from the batches' plans (`plans`: address of the first batch's
        slot): two launches for all batches (pcg_mark_touched_planned)"""
        _lib.check(self.lib.pcg_mark_touched_planned(self.g.desc_ref(), _p(ids), n_total, B, C.c_void_p(plans), stride, self.list_capacity,
                                                     _p(maps), self._touch_stride, self._stream()), "pcg_mark_touched_planned")

    def _enqueue_scores(self, train_flag):
        """label-aware score table + per-step sort of the train positives (the calls of their own: evaluation, parity)."""
        g = self.g
        self._fresh = False                         # (s0 / the keys are overwritten: theta's classifier, sorted keys)
        ops.score_table(g, self.w_clf, self.b_clf, out=self.s0)
        return ops.pos_sort(g, self.s0, self.keys) if (train_flag and g.n_pos) else None

    def _enqueue_scores_train(self, touched: Optional[int] = None):
        """the front of a training step: score pass || train-pos keys (unsorted) || the previous step's deferred Adam update.
        touched: address of the batch's byte map - only the rows it marks are scored."""
        g = self.g
        self._fresh = False                         # (the four-launch step: scores of theta's classifier, every step)
        _lib.check(self.lib.pcg_step_scores_train(
            g.desc_ref(), self._st, _p(self.s0), _p(self.keys) if g.n_pos else None,
            None if touched is None else C.c_void_p(touched), self._stream()), "pcg_step_scores_train")
        return self.keys if g.n_pos else None

    def _theta_written(self):
        """a call that enqueues a write of theta (now, or deferred to the next flush): infer_new's cached base scores are stale"""
        self._param_version += 1
        self._theta_dirty = True
        self._live = None

    def params_changed(self):
        """Tell the engine that the parameters were written from outside (a state dict loaded into the flat buffer's views):
        the stepped copy of the label classifier and the score table are taken from theta again."""
        self.flush()
        self._param_version += 1
        self._live = None
        self.clf_next.copy_(self.theta[self.n_rest:])
        self._fresh = False

    def _enqueue_refresh(self, touched: Optional[int] = None, into=None):
        """scores + unsorted train-pos keys of the classifier the next select launch uses (clf_next), one launch (no update of
        anything): the first training step after anything else has run, and every first step of an epoch of a touched-rows
        engine (whose previous step could not know this batch's map).  into: another (s0, keys) pair than the engine's own - a
        sequence's second buffers; the engine's own are then left as they are."""
        g = self.g
        F = self.F
        s0, keys = (self.s0, self.keys) if into is None else into
        _lib.check(self.lib.pcg_step_scores(
            g.desc_ref(), _p(self.clf_next), C.c_void_p(self.clf_next.data_ptr() + 8 * F), 0, g.n_nodes, _p(s0), None,
            _p(keys) if g.n_pos else None, -1, _p(self.sync), None if touched is None else C.c_void_p(touched),
            self._stream()), "pcg_step_scores")
        if self.presort:                             # (the steps that follow are told the keys are sorted)
            ops.pos_sort(g, s0, keys)
        if into is None:
            self._fresh = True

    def _enqueue_choose_train(self, ids, labels, B, plan: int, score_next: bool, next_touched: Optional[int] = None):
        """select (+ the label classifier's step for this batch) and gather (+ the deferred update of the other parameters,
        + the next step's scores if score_next) of a training step: pcg_choose_gather_train."""
        g = self.g
        with self._choosing(B) as (agg, cnt):
            _lib.check(self.lib.pcg_choose_gather_train(
                g.desc_ref(), self._batch(ids, labels, B, plan, cnt), _p(self.s0), _p(self.keys) if g.n_pos else None, self._sel,
                _p(agg), agg.stride(-2), self._st, 1 if score_next else 0,
                None if next_touched is None else C.c_void_p(next_touched), 1 if self.presort else 0, self._stream()),
                "pcg_choose_gather_train")
        self._fresh = bool(score_next)
        return agg, self.last_counts

    def _enqueue_choose(self, ids, labels, B, keys, train_flag, plan: int, sort_in_kernel: bool):
        """select + gather over the batch's plan (rows of several chunks are left as partial sums for the dense kernel).
        sort_in_kernel: the launch follows ``_enqueue_scores_train`` - `keys` holds this step's UNSORTED train-pos keys (the
        select kernel sorts them itself unless there are too many: then they are sorted already) and the launch clears the
        "deferred update pending" word."""
        g = self.g
        with self._choosing(B) as (agg, cnt):
            _lib.check(self.lib.pcg_choose_gather_planned(
                g.desc_ref(), _p(ids), _p(labels if train_flag else None), B, _p(self.s0), None, _p(keys), self._thr, self._rhos,
                1 if train_flag else 0, 0, _p(agg), agg.stride(-2), _p(cnt), _p(self.data), C.c_void_p(plan), self.list_capacity,
                _p(self.status), _p(self.sync) if sort_in_kernel else None, self._stream()), "pcg_choose_gather_planned")
        return agg, self.last_counts

    def _enqueue_tail(self, ids, labels, B, agg, plan: int, train: bool, combined=None, adam_clf: Optional[bool] = None, cnt=None):
        """dense tail reading the gather's partial sums (no combine launch); training: the gradient slabs are left pending
        (adam_clf 3, the default: no slabs at all - the kernel leaves its transposed activations and the next step's gather launch
        or flush() runs the weight-gradient GEMMs + Adam; 2: the same with per-tile gradient slabs; either way the label
        classifier has been stepped by this step's select launch).  adam_clf=0 (training): gradient slabs only - the caller
        reduces / all-reduces them itself; 1: the label classifier's Adam by the kernel's last workgroup (the four-launch step of
        pcg_step_scores_train); 4: transposed activations only, nothing marked as waiting (gradients())."""
        g = self.g
        cnt = self._cnt_of(B) if cnt is None else cnt
        adam_clf = (3 if train else 0) if adam_clf is None else int(adam_clf)
        out = _lib.DenseOut(_p(self.logits), _p(self.center), _p(combined), _p(self.row_loss) if labels is not None else None)
        _lib.check(self.lib.pcg_train_dense(
            g.desc_ref(), self._st if train else self._st_fwd, self._batch(ids, labels, B, plan, cnt), _p(agg), agg.stride(1),
            self._sel, out, adam_clf,
            # (the next step's keys: formed by the gather launch before this one if it scored ahead - then sorted here)
            _p(self.keys) if (adam_clf == 3 and self.presort and self._fresh) else None, self._stream()), "pcg_train_dense")
        if adam_clf == 1:                           # (the four-launch step updates theta's classifier in place)
            self.clf_next.copy_(self.theta[self.n_rest:])

    def _pipelines(self, batches) -> bool:
        """whether a sequence of training steps over these (lo, B) batches runs pipelined (_enqueue_pipelined)"""
        return (self.pipeline and not self.touched_on and len(batches) >= 2 and self._pipe_blocks > 0
                and max(B for _, B in batches) <= self.maxB)

    def _enqueue_part(self, part: int, ids, labels, B, plan: int, cnt, keys_sorted: int, clf_out=None, bufs=None,
                      score_next: bool = True):
        """one launch of a whole-table engine's pcg_choose_gather_train (pcg_choose_train_part): part 1 = the select launch
        (clf_out: the classifier slot it fills), 2 = the gather launch.
        bufs: the (s0, keys) pair the launch reads (select) or writes (the gather launch's score pass), default the engine's own"""
        g = self.g
        self._live = None                            # (lists, aggregates and counts are overwritten)
        agg = self._agg_of(B)
        s0, keys = (self.s0, self.keys) if bufs is None else bufs
        _lib.check(self.lib.pcg_choose_train_part(
            part, g.desc_ref(), self._batch(ids, labels, B, plan, cnt), _p(s0), _p(keys) if g.n_pos else None, self._sel, _p(agg),
            agg.stride(-2), self._st, 1 if score_next else 0, None, keys_sorted, _p(clf_out), self._stream()), "pcg_choose_train_part")

    def _ahead(self, steps) -> bool:
        """whether a pipelined sequence [(ids, labels, B, plan)] steps the label classifier two batches ahead
        (_enqueue_pipelined_ahead): three steps or more (shorter ones have no steady state), the keys a refresh leaves are sorted
        (presort; or there are none), and the fused launch has room for the sort riders (pcg_dense_select_ahead_ok)"""
        return (self.clf_ahead and len(steps) >= 3 and (self.presort or self.g.n_pos == 0)
                and bool(self.lib.pcg_dense_select_ahead_ok(self.g.desc_ref(), self.E, max(s[2] for s in steps))))

    def _enqueue_pipelined_ahead(self, steps):
        """_enqueue_pipelined with the label classifier two batches ahead.  The classifier's steps need nothing but the batches'
        own feature rows and labels, so the chain classifier step -> scores -> train-pos keys -> sort of batch t + 2 runs a launch
        earlier and every select reads keys sorted a launch before it (C_t: the classifier batch t is selected with):
            [scores + sorted keys of C_0 at hand]
            select(0) + classifier step 0 | scores + sorted keys of C_1 -> batch 1's buffers | classifier step 1
            per step t:  gather(t) [|| Adam of t - 1 || scores + raw keys of C_t+2 -> batch t + 2's buffers]
                         dense(t) || select(t + 1), keys sorted || classifier step t + 2 || riders: sort of batch t + 2's keys
            the last step: gather, dense(t) alone
        Batch n (= len(steps)) does not exist: its scores and sorted keys are what the sequence leaves for whatever follows, and
        there the look-ahead ends - no classifier step beside dense(n - 3 ...)'s successors, no riders in the last two steps.
        Buffers: batch t >= 1 uses (s0, keys) or (s0_alt, keys_alt) by the parity of n - t, so batch n's are the engine's own;
        batch 0's are the engine's own too and are read by select(0) before anything is written.  The classifier slot of batch t
        is t % 3.  Bit for bit what _enqueue_pipelined leaves."""
        g, lib = self.g, self.lib
        n = len(steps)
        if not self._fresh:
            self._enqueue_refresh()
        st = self._stream()
        cnt = lambda p, B: self._cnt_of(B, p)
        own, alt = (self.s0, self.keys), (self.s0_alt, self.keys_alt)
        buf = lambda t: own if (n - t) % 2 == 0 else alt
        slot = lambda t: self.clf_slots[t % 3]
        ids, lab, B, plan = steps[0]
        self._enqueue_part(1, ids, lab, B, plan, cnt(0, B), 1, clf_out=slot(0))
        self._fresh = False
        self._enqueue_refresh(into=buf(1))
        ids1, lab1, B1, _ = steps[1]
        _lib.check(lib.pcg_clf_step(g.desc_ref(), self._batch(ids1, lab1, B1), self._st, _p(slot(1)), 2, st), "pcg_clf_step")
        p = 0
        for t, (ids, lab, B, plan) in enumerate(steps):
            # (the gather launch's score pass writes batch t + 2's buffers with the classifier the launch before has stepped)
            self._enqueue_part(2, ids, lab, B, plan, cnt(p, B), 0, bufs=buf(t + 2), score_next=t + 2 <= n)
            agg = self._agg_of(B)
            if t + 1 == n:
                self._enqueue_tail(ids, lab, B, agg, plan, True, cnt=cnt(p, B))       # (_fresh is off: no key sort rides here)
                break
            nids, nlab, nB, nplan = steps[t + 1]
            s0n, keysn = buf(t + 1)
            cids, clab, cB = steps[t + 2][:3] if t + 2 < n else (None, None, 0)
            _lib.check(lib.pcg_dense_select_ahead(
                g.desc_ref(), self._st, self._sel, self._batch(ids, lab, B, plan, cnt(p, B)),
                self._batch(nids, nlab, nB, nplan, cnt(p ^ 1, nB)), self._batch(cids, clab, cB), _p(agg), agg.stride(1), _p(slot(t)),
                self._out, _p(slot(t + 2)) if cB else None, _p(s0n), _p(keysn) if g.n_pos else None,
                _p(buf(t + 2)[1]) if (g.n_pos and t + 2 <= n) else None, st), "pcg_dense_select_ahead")
            p ^= 1
        self.last_counts = cnt(p, B).view(g.R, B)
        self._fresh = True

    def _enqueue_pipelined(self, steps):
        """Consecutive training steps [(ids, labels, B, plan)] (deferred Adam, as train_step(defer=True) each), pipelined:
            select(0)
            per step t:  gather(t) [|| Adam of t - 1 || scores + keys of t + 1]
                         dense(t) || select(t + 1)      one launch (pcg_dense_select_train); the last step: dense(t) alone
        Bit for bit what the three-launch steps leave.  The selection of t + 1 writes the other count buffer and the other
        classifier slot than the dense tiles of t read; it sorts its train-pos keys itself."""
        if self._ahead(steps):
            return self._enqueue_pipelined_ahead(steps)
        g, lib = self.g, self.lib
        if not self._fresh:
            self._enqueue_refresh()
        st = self._stream()
        cnt = lambda p, B: self._cnt_of(B, p)
        ids, lab, B, plan = steps[0]
        self._enqueue_part(1, ids, lab, B, plan, cnt(0, B), 1 if self.presort else 0, clf_out=self.clf_slots[0])
        p = 0
        for t, (ids, lab, B, plan) in enumerate(steps):
            self._enqueue_part(2, ids, lab, B, plan, cnt(p, B), 0)
            agg = self._agg_of(B)
            if t + 1 == len(steps):
                self._fresh = True
                self._enqueue_tail(ids, lab, B, agg, plan, True, cnt=cnt(p, B))
                break
            nids, nlab, nB, nplan = steps[t + 1]
            _lib.check(lib.pcg_dense_select_train(
                g.desc_ref(), self._st, self._sel, self._batch(ids, lab, B, plan, cnt(p, B)),
                self._batch(nids, nlab, nB, nplan, cnt(p ^ 1, nB)), _p(agg), agg.stride(1), _p(self.clf_slots[p]), self._out,
                _p(self.clf_slots[p ^ 1]), _p(self.s0), _p(self.keys) if g.n_pos else None, st), "pcg_dense_select_train")
            p ^= 1
        self.last_counts = cnt(p, B).view(g.R, B)
        self._fresh = True

    def flush(self):
        """Apply a deferred Adam update now (no-op on the device if none is pending).  Enqueued, not synchronised."""
        if self._theta_dirty:                        # (a training call since the last flush: an update may be pending)
            self._param_version += 1
            self._theta_dirty = False
        _lib.check(self.lib.pcg_adam_flush(self._st, 0, self.n_params, self.n_rest, self.F, self.R, self._stream()), "pcg_adam_flush")

    def _enqueue_step(self, ids, labels, B, plan: int, defer: bool, touched: Optional[int] = None,
                      next_touched: Optional[int] = None):
        """the three launches of one training step over an existing plan (+ the flush unless deferred; + a score launch first
        if the scores at hand are not those of the current classifier).  touched / next_touched: the byte maps of this batch
        and of the one that follows (a touched-rows engine scores the next step's rows only if it is told which they are)."""
        if not self._fresh:
            self._enqueue_refresh(touched)
        score_next = (not self.touched_on) or next_touched is not None
        agg, _ = self._enqueue_choose_train(ids, labels, B, plan, score_next, next_touched)
        self._enqueue_tail(ids, labels, B, agg, plan, True)
        if not defer:
            self.flush()

    def _enqueue_adam(self, B, apply=True, want_grad=False, from_grad=False):
        """from_grad: the (all-reduced) flat gradient in self.grad is the single slab."""
        slabs, n_slabs = (self.grad, 1) if from_grad else (self.slabs, self.lib.pcg_dense_n_tiles(B))
        _lib.check(self.lib.pcg_adam_step(
            _p(self.theta), _p(self.m), _p(self.v), _p(slabs), n_slabs, self.n_params, _p(self.step_counter), self._hyper,
            _p(self.grad) if want_grad else None, 1 if apply else 0, self._stream()), "pcg_adam_step")

    def _enqueue_grad_slabs(self, ids, labels, B):
        """plan, scores, sort, select, gather, dense forward + backward partials: the gradient is left in the slabs (no Adam)."""
        plan = self._enqueue_plan_one(ids, labels, B, True)
        keys = self._enqueue_scores(True)
        agg, _ = self._enqueue_choose(ids, labels, B, keys, True, plan, sort_in_kernel=False)
        self._enqueue_tail(ids, labels, B, agg, plan, True, adam_clf=False)

    # ------------------------------------------------------------------
    def train_step(self, ids: torch.Tensor, labels: torch.Tensor, allreduce=None, defer: bool = False, plan: Optional[int] = None,
                   touched: Optional[int] = None, next_touched: Optional[int] = None):
        """zero_grad + loss + backward + Adam step for one batch (model_handler.py:149-153).
        ids / labels: int32 device tensors.  Nothing is returned and nothing syncs;
        ``last_loss()`` reads the batch loss afterwards.  ``allreduce(flat_grad)`` (data-parallel
        ranks) is called between the gradient reduction and the Adam update.  ``defer``: leave the Adam update of
        everything but the label classifier to the next step's front (or ``flush()``) - inside an epoch.
        ``plan``: address of this batch's plan slot if it has been planned already (a staged epoch); else it is planned here."""
        B = ids.numel()
        if B == 0:
            return
        self._theta_written()
        self._fit(B)
        self._lastB = B
        if allreduce is None:
            if plan is None:
                plan = self._enqueue_plan_one(ids, labels, B, True)
                touched = self._touch_one.data_ptr() if self.touched_on else None
            self._enqueue_step(ids, labels, B, plan, defer, touched, next_touched)
            return
        # data-parallel ranks: gradient of the local batch -> all-reduce -> the same Adam on every rank
        self.flush()
        self._enqueue_grad_slabs(ids, labels, B)
        self._enqueue_adam(B, apply=False, want_grad=True)
        allreduce(self.grad)
        self._enqueue_adam(B, apply=True, from_grad=True)
        self.clf_next.copy_(self.theta[self.n_rest:])      # (the label classifier is stepped with everything else here)

    # train_step_graph, begin_epoch / stage_epoch .. epoch_step, epoch_run, read_batch_lists: EpochCalls (epoch.py)

    def check(self):
        """Raise if any batch since the last check did not fit its selection list (the kernels then select nothing and
        only set the device status word), or a list named a row outside its table, or an in-kernel wait ran out.  Reads one
        word: synchronises - call it where the host waits anyway (``last_loss``, the end of an evaluation pass or of an epoch,
        after a timed region)."""
        st = int(self.status.item())
        if st == 0:
            return
        self.status.zero_()
        self._raise_status(st)

    @staticmethod
    def _raise_status(st: int):
        what = []
        if st & _lib.PCG_ST_SEL_OVERFLOW:
            what.append("selection list overflow: a batch needed more list entries than the workspace holds - raise "
                        "FusedPCGNN(list_capacity=...)")
        if st & _lib.PCG_ST_LIST_ID_RANGE:
            what.append("a selection list named a row outside the feature table")
        if st & _lib.PCG_ST_SYNC_TIMEOUT:
            what.append("a bounded in-kernel wait ran out: the select kernel's wait for its own train-pos sort, or a plan "
                        "workgroup's wait for its predecessors' totals")
        if st & _lib.PCG_ST_SORT_OVERFLOW:
            what.append("the one-launch sort of the train positives met a bucket of more than 4096 keys: minority picks may be wrong")
        if st & _lib.PCG_ST_RANK_MISMATCH:
            what.append("rank_lists: a row's kept count on the device is not the extent its output offsets give it - the row "
                        "was not written (rank_minority: a row's extent is negative, above n_pos or leaves its array; "
                        "neighbour_contrib: a row's offsets are not ascending inside the lists)")
        raise _lib.PcgnnLibraryError("; ".join(what) or f"device status {st}")

    def last_loss(self) -> torch.Tensor:
        self.check()
        B = self._lastB
        return self.row_loss[:B].sum() / (B * self.scale)

    def gradients(self, ids: torch.Tensor, labels: torch.Tensor, via: str = "acts") -> Dict[str, torch.Tensor]:
        """loss.backward() without the optimizer step: per-parameter gradients (parity tests).  via="acts": the training
        step's kernels (dense kernel -> transposed activations -> the weight-gradient GEMMs of pcg_wgrad, the label
        classifier's tiles included); via="slabs": per-tile gradient slabs summed in tile order (the data-parallel paths')."""
        B = ids.numel()
        self.flush()
        self._fit(B, flush=False)
        if via == "slabs":
            self._enqueue_grad_slabs(ids, labels, B)
            self.step_counter -= 1               # the dense kernel counted a step that is not taken
            self._enqueue_adam(B, apply=False, want_grad=True)
        else:
            plan = self._enqueue_plan_one(ids, labels, B, True)
            keys = self._enqueue_scores(True)
            agg, _ = self._enqueue_choose(ids, labels, B, keys, True, plan, sort_in_kernel=False)
            self._enqueue_tail(ids, labels, B, agg, plan, True, adam_clf=4)
            self.step_counter -= 1
            _lib.check(self.lib.pcg_wgrad(self._st_grad, B, self.F, self.R, _p(self.grad), 0, 1, None, self._stream()), "pcg_wgrad")
        self._lastB = B
        out = {}
        for name, view in self.views.items():
            off = view.storage_offset()
            out[name] = self.grad[off:off + view.numel()].view(view.shape).clone()
        return out

    def predict(self, ids: torch.Tensor, labels: Optional[torch.Tensor] = None, train_flag: bool = False,
                want_combined: bool = False):
        """forward only -> (gnn logits [B,2], label-aware logits [B,2][, combined [B,E]])
        (PCALayer.forward, model.py:34-39; utils.py:305 calls it with train_flag=False)."""
        B = ids.numel()
        self.flush()
        self._fit(B, flush=False)
        plan = self._enqueue_plan_one(ids, labels, B, train_flag)
        keys = self._enqueue_scores(train_flag)
        agg, _ = self._enqueue_choose(ids, labels, B, keys, train_flag, plan, sort_in_kernel=False)
        comb = torch.empty(B, self.E, dtype=torch.float32, device=self.dev) if want_combined else None
        self._enqueue_tail(ids, None, B, agg, plan, False, combined=comb)
        res = (self.logits[:B].clone(), self.center[:B].clone())
        return res + (comb,) if want_combined else res

    # -- custom losses and optimizers on the fused path ----------------------------------------------
    # The whole backward of the dense kernel is a function of two small arrays - d loss / d gnn logits and d loss / d label-aware
    # logits - and of the forward's state; the selection is not differentiated.  So: a forward that returns the two logit tensors
    # under autograd, and a backward that hands whatever gradients autograd brings for them to pcg_dense_vjp + pcg_wgrad.
    # Out of scope (they keep the built-in loss and Adam): DistributedPCGNN, the GraphSAGE / GCN models, the graph, pipelined and
    # whole-epoch engines (train_step_graph, epoch_*), and hipGraph capture of the custom step.
    def _forward_live(self, ids, labels, train_flag):
        """predict, remembered as THE forward whose plan, lists, aggregates and counts are in the workspace"""
        if train_flag and labels is None:
            raise ValueError("forward(train_flag=True) needs the batch's labels (the training-mode selection reads them)")
        res = self.predict(ids, labels, train_flag)
        B = ids.numel()
        self._live_serial += 1
        self._live = dict(serial=self._live_serial, ids=ids, B=B, plan=self._plan_slot(B).data_ptr())
        return res

    def _live_of(self, serial: int) -> dict:
        live = self._live
        if live is None or live["serial"] != serial:
            raise RuntimeError("stale forward: the engine's workspace or parameters have been overwritten since this forward() "
                               "(another forward / predict / gradients / train_step* / epoch_* call, or params_changed / "
                               "optimizer_step) - one forward is outstanding per engine; run forward() again")
        return live

    def _by_name(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        return {k: flat[v.storage_offset():v.storage_offset() + v.numel()].view(v.shape) for k, v in self.views.items()}

    def _enqueue_vjp(self, live: dict, d_logits, d_center, apply: bool = False, out=None) -> Optional[torch.Tensor]:
        """pcg_dense_vjp over what the live forward left in the workspace, then the weight-gradient GEMMs: the flat gradient in a
        buffer of its own (apply=False), or the engine's Adam on every parameter (apply=True; the caller has moved the step
        counter on).  out: (logits, center) tensors the launch's own forward writes.  Nothing synchronises."""
        g, B = self.g, live["B"]
        if B == 0:
            return None if apply else torch.zeros(self.n_params, dtype=torch.float32, device=self.dev)
        seeds = []
        for what, d in (("d_logits", d_logits), ("d_center", d_center)):
            if d is None:
                d = torch.zeros(B, 2, dtype=torch.float32, device=self.dev)
            if tuple(d.shape) != (B, 2) or d.device != self.dev:
                raise ValueError(f"{what}: a [{B}, 2] tensor on {self.dev} expected, got {tuple(d.shape)} on {d.device}")
            seeds.append(d.detach().to(torch.float32).contiguous())
        agg, cnt = self._agg_of(B), self._cnt_of(B)
        dense_out = None if out is None else _lib.DenseOut(_p(out[0]), _p(out[1]), None, None)
        _lib.check(self.lib.pcg_dense_vjp(
            g.desc_ref(), self._st, self._batch(live["ids"], None, B, live["plan"], cnt), _p(agg), agg.stride(1), self._sel,
            _p(seeds[0]), _p(seeds[1]), dense_out, self._stream()), "pcg_dense_vjp")
        if apply:
            _lib.check(self.lib.pcg_wgrad(self._st, B, self.F, self.R, None, 1, 1, None, self._stream()), "pcg_wgrad")
            return None
        grad = torch.empty(self.n_params, dtype=torch.float32, device=self.dev)
        _lib.check(self.lib.pcg_wgrad(self._st_grad, B, self.F, self.R, _p(grad), 0, 1, None, self._stream()), "pcg_wgrad")
        return grad

    def forward(self, ids: torch.Tensor, labels: Optional[torch.Tensor] = None, train_flag: bool = True):
        """The forward of a training step as a differentiable function of the model's parameters -> (gnn logits [B, 2],
        label-aware logits [B, 2]); the values are bit for bit ``predict(ids, labels, train_flag)``.  Under ``torch.no_grad()`` it IS
        predict.  Otherwise the two tensors come from an autograd function whose inputs are the model's parameters, so any loss of
        them - ``loss.backward()`` - leaves the gradients in ``p.grad`` of ``model.parameters()``, accumulated as autograd
        accumulates.  The backward runs on the device: pcg_dense_vjp (the dense kernel's backward, started from the loss
        gradients of the two logit tensors) over the plan, lists, aggregates and counts this forward left in the workspace, then
        the weight-gradient GEMMs of pcg_wgrad.  Nothing synchronises.  The selection is not differentiated.
        ONE forward is outstanding per engine: any call that overwrites the workspace or enqueues a write of theta (another
        forward / predict / gradients / train_step* / epoch_*, params_changed, optimizer_step) makes it stale, and its backward
        then raises a RuntimeError instead of computing from overwritten buffers.  A second backward of a live forward
        (retain_graph=True) gives the same gradients again.  ``ids`` is kept by reference until then: do not write it.
        train_flag=True needs labels, as predict does.  Not captured into hipGraphs."""
        if not torch.is_grad_enabled():
            return self.predict(ids, labels, train_flag)
        return _SeededDense.apply(self, ids, labels, train_flag, *self._params)

    def vjp(self, d_logits: torch.Tensor, d_center: torch.Tensor, want_logits: bool = False):
        """The low-level form of forward()'s backward: the per-parameter gradients (the format ``gradients()`` returns) of the live
        forward for the given d loss / d gnn logits and d loss / d label-aware logits ([B, 2] each, used as given).
        want_logits: also the (gnn, label-aware) logits the launch's own forward wrote -> (grads, logits, center)."""
        if self._live is None:
            self._live_of(-1)
        live = self._live
        out = None
        if want_logits:
            out = tuple(torch.empty(live["B"], 2, dtype=torch.float32, device=self.dev) for _ in range(2))
        grads = self._by_name(self._enqueue_vjp(live, d_logits, d_center, out=out))
        return (grads,) + out if want_logits else grads

    def optimizer_step(self, opt):
        """``opt.step()`` for any ``torch.optim`` optimizer over ``model.parameters()``: the parameters are views into the flat
        buffer, so the optimizer writes theta directly; ``params_changed()`` then tells the engine (the stepped copy of the label
        classifier and the score table are taken from theta again; an outstanding forward becomes stale)."""
        opt.step()
        self.params_changed()

    def train_step_custom(self, ids: torch.Tensor, labels: torch.Tensor, loss_fn):
        """One training step with the caller's loss and the ENGINE's Adam (its lr, betas, eps, weight decay): forward ->
        ``loss_fn(gnn_logits, center_logits, labels)`` (a scalar) -> its autograd down to the two logit tensors -> pcg_dense_vjp ->
        pcg_wgrad(apply = 1, with_clf = 1).  Every parameter, the label classifier included, is stepped together from this batch's
        gradient: there is no one-step-ahead classifier on this path.  Returns the loss tensor (detached); nothing synchronises.
        Eager launches only - the graph, pipelined and whole-epoch engines keep the built-in loss."""
        if ids.numel() == 0:
            return None
        with torch.no_grad():
            gnn, center = self._forward_live(ids, labels, True)
        live = self._live
        gnn.requires_grad_(True)
        center.requires_grad_(True)
        with torch.enable_grad():
            loss = loss_fn(gnn, center, labels)
        d_gnn, d_center = torch.autograd.grad(loss, (gnn, center), allow_unused=True)
        self._theta_written()                        # (the forward is spent: theta is about to change)
        self.step_counter += 1                       # Adam's t, on the device, ahead of the launch that reads it
        self._enqueue_vjp(live, d_gnn, d_center, apply=True)
        self.clf_next.copy_(self.theta[self.n_rest:])      # (the label classifier is stepped with everything else here)
        self._fresh = False
        return loss.detach()

    # infer, chosen, attribute, embed, nearest, evaluate and their *_new forms: WholeSetCalls (wholeset.py)
