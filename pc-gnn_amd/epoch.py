"""The fused engine's steps as hipGraphs, and the staged epoch: ``train_step_graph`` (one graph per batch size), ``stage_epoch`` /
``begin_epoch`` / ``plan_staged`` (an epoch's ids, labels and plans in static buffers), ``epoch_step`` / ``epoch_step_timed`` (a
graph per staged batch) and ``epoch_run`` (a whole epoch, or several, as ONE graph launch) - ``EpochCalls``, a mix-in of
``fused.FusedPCGNN``.  What is captured is the engine's own launch sequence (fused.py, ``_enqueue_*`` / ``train_step``): this file
decides which batch runs from which buffers, when something is captured, and what a replay leaves behind on the host side.
"""
import gc
from typing import Optional

import torch

from . import _lib


def epoch_batches(n: int, batch_size: int, n_epochs: int = 1):
    """The batches of n_epochs epochs of n picks each, staged back to back: [(first pick, size)].  Every epoch is cut on its
    own: only an epoch's last batch may be the shorter one."""
    return [(e * n + lo, min(batch_size, n - lo)) for e in range(n_epochs) for lo in range(0, n, batch_size)]


class EpochCalls:
    """The graph and staged-epoch surface of ``fused.FusedPCGNN``, as a mix-in.  Its state is what ``_init_epoch_state`` declares
    (the engine's ``__init__`` calls it before ``_alloc``, which clears the graphs and the buffer sets with the buffers they point
    into) plus the staged shape ``stage_epoch`` sets (``_ep_n``, ``_ep_bs``, ``_ep_k``, ``_ep_batches``); the only buffers it
    allocates are the two epoch buffer sets.  What it uses of the engine: ``g``, ``lib``, ``dev``, ``R``, ``maxB``, ``data``,
    ``list_capacity``, ``touched_on``, ``_touch_stride``, ``_touch_one``, ``ids_buf`` / ``lab_buf``, ``keys``, the optimizer state
    (``theta``, ``m``, ``v``, ``step_counter``, ``clf_next``), ``_fresh``, ``_prof``, ``_lastB``, ``last_counts``; ``flush``,
    ``train_step``, ``_theta_written``, ``_fit``, ``_bracket``, ``_agg_of`` / ``_cnt_of``, ``_plan_bytes`` / ``_plan_slot``,
    ``_pipelines`` and the launches ``_enqueue_plan``, ``_enqueue_plan_one``, ``_enqueue_mark``, ``_enqueue_refresh``,
    ``_enqueue_choose_train``, ``_enqueue_tail`` and ``_enqueue_pipelined``."""

    def _init_epoch_state(self):
        self._graphs = {}          # batch size -> the graphs of train_step_graph
        self._ep_graphs = {}       # the graphs of the staged epoch: per batch, per timed batch, per whole-epoch call shape
        self._ep_sets = None       # two sets of epoch buffers: ids | labels | plan slots | touched-row maps (stage_epoch)
        self._cur, self._cur_ready, self._ep_stride = 0, False, 0      # the current set; it holds an epoch prepared ahead
        self._ep_shape = None      # (n, batch_size, n_epochs) of the last stage_epoch
        # epoch_run(prefetch="stream"): the side stream, "the set prepared there is ready", "the other set's last reader is done"
        self._side = self._ev_ready = self._ev_free = None

    # -- one step as a graph ----------------------------------------------------------------------------------------------
    def train_step_graph(self, ids: torch.Tensor, labels: torch.Tensor, timed: bool = False):
        """Same as train_step through captured hipGraphs (one set per batch size): one graph launch
        per step.  timed=True (bench.py, every Nth step) replays the step as [plan + scores graph] ->
        choose+aggregate bracketed by HIP events -> [dense+Adam graph]; same kernels, same order."""
        B = ids.numel()
        if B == 0:
            return
        self._theta_written()
        self._fit(B)
        self._lastB = B
        gr = self._graphs.get(B) or self._capture(B)
        self.ids_buf[:B].copy_(ids)
        self.lab_buf[:B].copy_(labels)
        if timed and self._prof is not None:
            gr["pre"].replay()
            with self._bracket():
                gr["choose"].replay()      # the same launches as inside "full", as a graph of their own
            self.last_counts = self._cnt_of(B).view(self.R, B)
            gr["post"].replay()
        else:
            gr["full"].replay()

    def _capture_graphs(self, fns, warm=None):
        """Warm up (kernel attributes, per-batch-size plan slots: nothing may allocate inside a capture) on a side
        stream, capture every fn into a hipGraph of its own, and put the optimizer state back.  A deferred Adam update
        of real steps is applied first (the saved state then includes it); the warm-up's own is flushed and undone."""
        self.flush()
        # (the classifier slots, s0_alt / keys_alt and the second count buffer are scratch of ONE pipelined sequence: nothing of
        #  them is read after it, so they are not part of the state; s0 / keys are marked stale below)
        state = (self.theta.clone(), self.m.clone(), self.v.clone(), self.step_counter.clone(), self.clf_next.clone())
        prof, self._prof = self._prof, None
        s = torch.cuda.Stream(self.dev)
        s.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(s):
            for fn in (warm if warm is not None else fns):
                fn()
            self.flush()
        torch.cuda.current_stream(self.dev).wait_stream(s)
        graphs = []
        # (no garbage collection while a stream is capturing: a collected engine of the caller's - tensors, events, other graphs -
        #  is torn down with HIP calls that are not allowed during a capture and end the process)
        gc.collect()
        was_on = gc.isenabled()
        gc.disable()
        try:
            for fn in fns:
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    fn()
                graphs.append(gr)
        finally:
            if was_on:
                gc.enable()
        for dst, src in zip((self.theta, self.m, self.v, self.step_counter, self.clf_next), state):
            dst.copy_(src)
        self._fresh = False                          # (s0 holds the warm-up's scores)
        self._prof = prof
        return graphs

    def _capture(self, B):
        ids, lab = self.ids_buf[:B], self.lab_buf[:B]
        agg = self._agg_of(B)
        plan = self._plan_slot(B).data_ptr()

        def pre():                     # (a step on its own: nothing is known about the batch before or after it)
            self._enqueue_plan_one(ids, lab, B, True)
            self._enqueue_refresh(self._touch_one.data_ptr() if self.touched_on else None)

        def post():
            self._enqueue_tail(ids, lab, B, agg, plan, True)
            self.flush()

        def choose():
            self._enqueue_choose_train(ids, lab, B, plan, False)

        def full():
            pre()
            choose()
            post()

        graphs = self._graphs[B] = dict(zip(("full", "pre", "choose", "post"),
                                            self._capture_graphs([full, pre, choose, post], warm=[full])))
        return graphs

    # -- whole-epoch path: ids / labels of an epoch live in static buffers, one plan slot and one graph per batch ------
    # There are TWO sets of epoch buffers (ids | labels | plan slots).  The picks of an epoch and its plans depend on nothing
    # a training step computes, so with ``epoch_run(prefetch=True)`` the sampler and the plan launches of epoch e + 1 run on a
    # parallel branch of epoch e's graph, into the other set - off the steps' serial chain altogether.
    def _ep_set(self, which: Optional[int] = None) -> dict:
        """buffer set `which` (default: the current one)"""
        return self._ep_sets[self._cur if which is None else which]

    @property
    def _ep_ids(self):
        return None if self._ep_sets is None else self._ep_set()["ids"]

    @property
    def _ep_lab(self):
        return self._ep_set()["lab"]

    @property
    def _ep_plans(self):
        return None if self._ep_sets is None else self._ep_set()["plans"]

    def stage_epoch(self, n: int, batch_size: int, n_epochs: int = 1):
        """Static id / label buffers and plan slots of n_epochs epochs of n picks each (the ids are filled by begin_epoch or by a
        sampler; ``plan_staged()`` must follow before any of the staged steps runs).  Several epochs staged together are sampled
        and planned by ONE launch each - the sampler's and the plan's latency chains are paid once per n_epochs epochs - and are
        walked as one sequence of batches 0 .. n_epochs * ceil(n / batch_size) - 1 (every epoch's last batch may be the shorter
        one).  Returns the CURRENT set's (ids, labels), n_epochs * n long.
        Another (n, batch_size, n_epochs) than the last call's DROPS a set that ``epoch_run(prefetch=...)`` has prepared: its ids
        and plans are laid out for the old shape.  The call waits for whatever is still preparing it, the set counts as not
        ready, and the next epoch is sampled and planned anew, at the new shape.  The epoch numbers the dropped set had consumed
        are SKIPPED, not drawn again: the sampler's device counter only ever moves forward (it was moved on when the set was
        planned), so the next epoch sampled is the one after the dropped set's last.  Every epoch number still names
        independent draws of the same distribution, and no number is trained twice."""
        self._fit(batch_size)
        batches = epoch_batches(n, batch_size, n_epochs)
        nb, total = len(batches), n * n_epochs
        stride = self._plan_bytes(batch_size)
        sets = self._ep_sets
        if sets is None or sets[0]["ids"].numel() < total or self._ep_stride != stride or sets[0]["plans"].numel() < nb * stride:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.PcgnnLibraryError("stage_epoch with a new shape inside a graph capture")
            self._drop_prepared()                    # (before the old buffers go: nothing may still be writing them)
            self._ep_sets = [dict(ids=torch.zeros(total, dtype=torch.int32, device=self.dev),
                                  lab=torch.zeros(total, dtype=torch.int32, device=self.dev),
                                  plans=torch.zeros(nb * stride, dtype=torch.uint8, device=self.dev),
                                  touched=torch.zeros(nb * self._touch_stride, dtype=torch.uint8, device=self.dev)
                                  if self.touched_on else None) for _ in range(2)]
            self._ep_stride = stride
            self._cur, self._cur_ready = 0, False
            self._ep_graphs.clear()
        shape = (n, batch_size, n_epochs)
        if self._ep_shape is not None and self._ep_shape != shape:
            # another epoch shape inside the same buffers: the last batch's (shorter) plan layout moves to another slot, and the
            # plan launch's look-back tags (a small integer per workgroup) would sit on top of whatever the old layout left
            # there - zero the slots so that no stale word can pass for a published total
            if torch.cuda.is_current_stream_capturing():
                raise _lib.PcgnnLibraryError("stage_epoch with a new epoch size inside a graph capture")
            # a set prepared ahead holds the old shape's ids and is about to lose its plans: it is dropped (its epoch numbers are
            # skipped), after whatever is still writing it has finished
            self._drop_prepared()
            for st in self._ep_sets:
                st["plans"].zero_()
            self._ep_graphs.clear()
        self._ep_shape = shape
        self._ep_n, self._ep_bs, self._ep_k = n, batch_size, n_epochs
        self._ep_batches = batches                   # batch j of the staged sequence: (first pick, size)
        return self._ep_ids[:total], self._ep_lab[:total]

    def _drop_prepared(self):
        """Forget a set that ``epoch_run(prefetch=...)`` has sampled and planned ahead - its buffers are about to be rewritten or
        replaced.  The current stream first waits for the side stream's sampler and plan launches (prefetch="stream"): nothing
        may still be writing the set.  The epoch numbers it had consumed are skipped (``stage_epoch``)."""
        if not torch.cuda.is_current_stream_capturing():      # (a capturing stream cannot wait for work outside its capture)
            main = torch.cuda.current_stream(self.dev)
            if self._ev_ready is not None:
                main.wait_event(self._ev_ready)
            if self._side is not None:
                main.wait_stream(self._side)
        self._cur_ready, self._ev_ready = False, None

    def take_prefetched(self) -> bool:
        """True if the current set already holds a sampled and planned epoch that no step has used yet (left by
        ``epoch_run(prefetch=True)``) - the caller then starts on it instead of sampling; the set counts as used from here on."""
        ready, self._cur_ready = self._cur_ready, False
        if ready and self._ev_ready is not None:     # (prepared on the side stream: epoch_run(prefetch="stream"))
            torch.cuda.current_stream(self.dev).wait_event(self._ev_ready)
            self._ev_ready = None
        return ready

    def plan_staged(self, bump_counter: Optional[torch.Tensor] = None, which: Optional[int] = None):
        """Plan every batch of the staged epoch (set `which`, default the current one): one launch (after the sampler, before
        the epoch's first step).  bump_counter: the sampler's device epoch counter, incremented by it."""
        st = self._ep_set(which)
        self._enqueue_plan(st["ids"], st["lab"], self._ep_n, self._ep_bs, st["plans"], self._ep_stride, True, bump_counter, self._ep_k)
        if self.touched_on:
            nb_e = -(-self._ep_n // self._ep_bs)
            for e in range(self._ep_k):              # (an epoch's last batch may be the shorter one: the maps are made epoch by epoch)
                self._enqueue_mark(st["ids"][e * self._ep_n:], self._ep_n, self._ep_bs, st["touched"][e * nb_e * self._touch_stride:],
                                   st["plans"].data_ptr() + e * nb_e * self._ep_stride, self._ep_stride)
            self._fresh = False                      # (new maps: the rows scored so far need not cover the new first batch)

    def _sample_and_plan(self, which: int, sample, bump_counter):
        """a new epoch into set `which`: the sampler (if there is one: it fills the set's ids and labels), then the plans"""
        if sample is not None:
            st, n = self._ep_set(which), self._ep_n * self._ep_k
            sample(st["ids"][:n], st["lab"][:n])
        self.plan_staged(bump_counter, which=which)

    def _ep_slice(self, b: int, which: Optional[int] = None):
        """(ids, labels, size) of staged batch b, views into set `which`"""
        lo, B = self._ep_batches[b]
        st = self._ep_set(which)
        return st["ids"][lo:lo + B], st["lab"][lo:lo + B], B

    def _ep_plan(self, b: int, which: Optional[int] = None) -> int:
        return self._ep_set(which)["plans"].data_ptr() + b * self._ep_stride

    def _ep_touch(self, b: int, which: Optional[int] = None) -> Optional[int]:
        return self._ep_set(which)["touched"].data_ptr() + b * self._touch_stride if self.touched_on else None

    def _ep_next_touch(self, b: int, which: Optional[int] = None) -> Optional[int]:
        """the map of the batch after b, if the staged sequence has one"""
        if not self.touched_on or b + 1 >= len(self._ep_batches):
            return None
        return self._ep_touch(b + 1, which)

    def _scores_next(self, b: int, which: Optional[int] = None) -> bool:
        """whether the step of staged batch b also scores for the batch after it (a touched-rows engine: only if there is one,
        whose map says which rows) - so the scores at hand are fresh after it"""
        return (not self.touched_on) or self._ep_next_touch(b, which) is not None

    def begin_epoch(self, ids: torch.Tensor, labels: torch.Tensor, batch_size: int):
        """Stage an epoch's (already shuffled) ids and labels and plan its batches; afterwards ``epoch_step(b)`` is exactly
        one graph launch - no copies, no indexing kernels (model_handler.py:142-148 slices a Python list here)."""
        n = ids.numel()
        ep_ids, ep_lab = self.stage_epoch(n, batch_size)
        self._drop_prepared()                        # (the ids go into the current set: an epoch prepared ahead there is lost)
        ep_ids.copy_(ids)
        ep_lab.copy_(labels)
        self.plan_staged()

    def epoch_step(self, b: int, defer: bool = False):
        """Batch b of the staged (and planned) epoch as one graph replay.  defer: as inside epoch_run - the Adam update of
        everything but the label classifier is left to the next batch's front launch (the epoch's last batch flushes it), so
        the parameters are complete only after the last batch or a flush()."""
        if b >= len(self._ep_batches):
            return
        lo, B = self._ep_batches[b]
        self._lastB = B
        self._theta_written()
        defer = defer and b + 1 < len(self._ep_batches)
        key = (self._cur, lo, B, self._ep_shape, "deferred") if defer else (self._cur, lo, B, self._ep_shape)
        gr = self._ep_graphs.get(key)
        if gr is None:
            ids, lab, _ = self._ep_slice(b)
            gr = self._ep_graphs[key] = self._capture_graphs([lambda: self.train_step(
                ids, lab, defer=defer, plan=self._ep_plan(b), touched=self._ep_touch(b), next_touched=self._ep_next_touch(b))])[0]
        if not self._fresh:                          # (the graph was captured with the scores at hand, or scores them itself)
            self._enqueue_refresh(self._ep_touch(b))
        gr.replay()
        self._fresh = self._scores_next(b)

    def epoch_step_timed(self, b: int, eager: bool = True, flush: bool = True):
        """Batch b of the staged epoch with HIP events around the select + gather call (appended to ``_prof``): the same
        kernels in the same order as one step of ``epoch_run``, reading the staged ids in place (no copies, no label
        gather).  eager: the four kernels launched one by one with the two event records between them (the host stays
        ahead of the GPU, so the events bracket the two kernels and nothing else); otherwise three graphs - scores | select +
        gather | dense - whose launch latency lands inside the bracket."""
        if b >= len(self._ep_batches):
            return
        lo, B = self._ep_batches[b]
        self._lastB = B
        self._theta_written()
        ids, lab, _ = self._ep_slice(b)
        plan, agg = self._ep_plan(b), self._agg_of(B)
        # the staged sequence's last batch: nothing follows that would apply the deferred update (flush=False: the caller's next
        # launches - the next group's first gather launch, or its own flush - do)
        last = flush and b + 1 >= len(self._ep_batches)
        touched, nxt, score_next = self._ep_touch(b), self._ep_next_touch(b), self._scores_next(b)

        def choose():                                # (eager: it records the two events itself)
            self._enqueue_choose_train(ids, lab, B, plan, score_next, nxt)

        def tail():
            self._enqueue_tail(ids, lab, B, agg, plan, True)
            if last:
                self.flush()

        if not self._fresh:
            self._enqueue_refresh(touched)
        if eager:
            choose()
            tail()
            return
        key = (self._cur, lo, B, self._ep_shape, "timed")
        grs = self._ep_graphs.get(key)
        if grs is None:
            grs = self._ep_graphs[key] = self._capture_graphs(
                [choose, tail], warm=[lambda: (self._enqueue_refresh(touched), choose(), tail())])
            self._enqueue_refresh(touched)
        with self._bracket(always=True):
            grs[0].replay()
        self.last_counts = self._cnt_of(B).view(self.R, B)
        grs[1].replay()
        self._fresh = score_next

    def epoch_run(self, n_steps: Optional[int] = None, sample=None, bump_counter: Optional[torch.Tensor] = None,
                  flush: bool = True, prefetch: bool = False, first_step: int = 0):
        """All batches of the staged epoch as ONE graph launch: the host latency between two graph launches (~8 us)
        is paid once per epoch instead of once per batch.  ``sample(ids, labels)``, if given, is enqueued (and captured): it
        fills the given id / label buffers on the device (pick + shuffle + labels), so a replay is a whole new epoch;
        the plans of all batches follow (which also bumps ``bump_counter``, the sampler's epoch number).
        flush=False: the last batch's deferred Adam update (everything but the label classifier) is left to whatever comes
        next - the next epoch's first front launch applies it, any other public call flushes it first.
        prefetch=True (needs ``sample``): the sampler and the plans of the NEXT epoch run on a parallel branch of this epoch's
        graph, into the other buffer set; afterwards that set is the current one and ready (``take_prefetched``).  The first
        such call - or one after the ready set was used up by other calls - samples its own epoch first.
        A prepared set is DROPPED by whatever rewrites or replaces its buffers before a step has used it: ``stage_epoch`` with
        another (n, batch_size, n_epochs), ``begin_epoch`` (its ids go into that set), a batch above max_batch anywhere (every
        buffer is re-allocated).  The epoch numbers the dropped set had consumed are skipped - ``bump_counter`` is never moved
        back - and the next epoch is sampled and planned anew.  Calls that leave the epoch buffers alone (``train_step`` within
        max_batch, ``predict``, ``infer``, ``chosen``, ``flush``) leave the prepared set ready.
        prefetch="stream": the same division of labour without a fork inside the graph: the sampler and plan launches of the next
        epoch are enqueued - by the host, behind this epoch's graph launch - on a second stream, where they run beside this
        epoch's kernels; the only cross-stream waits are two events per epoch (the other buffer set is free / is ready).
        first_step > 0: the REST of an epoch that is staged and planned already and whose first batches have been run some other
        way (batches first_step .. n_steps - 1): no sampler, no plans."""
        self._theta_written()
        nb = len(self._ep_batches)
        n_steps = nb if n_steps is None else min(n_steps, nb)
        if first_step > 0:
            sample, prefetch = None, False
        on_stream = prefetch == "stream" and sample is not None
        prefetch = prefetch is True and sample is not None
        cur = self._cur
        primed = (prefetch or on_stream) and self._cur_ready
        if primed and self._ev_ready is not None:
            # the side stream has sampled and planned this set: wait here, in front of a capture too - its warm-up plans the
            # set again and runs the steps over it
            torch.cuda.current_stream(self.dev).wait_event(self._ev_ready)
            self._ev_ready = None
        key = ("epoch", cur, self._ep_shape, n_steps, sample is not None, None if bump_counter is None else bump_counter.data_ptr(),
               flush, prefetch, primed, on_stream, first_step)
        gr = self._ep_graphs.get(key)
        if gr is None:
            gr = self._ep_graphs[key] = self._capture_epoch(cur, first_step, n_steps, sample, bump_counter, flush, prefetch,
                                                            on_stream, primed)
        self._lastB = self._ep_batches[n_steps - 1][1]
        # (whole-table engine: the graph was captured with the scores at hand - it holds no score launch of its own; a
        #  touched-rows engine's graph scores its first batch's rows itself, behind its sampler and maps)
        if first_step > 0:
            if not self._fresh:                      # (the graph was captured with the scores at hand)
                self._enqueue_refresh(self._ep_touch(first_step, cur))
        elif not self.touched_on and not self._fresh:
            self._enqueue_refresh()
        gr.replay()
        self._fresh = self._scores_next(n_steps - 1, cur)
        self._hand_over(cur, sample, bump_counter, prefetch, on_stream)
        return n_steps

    def _run_staged(self, cur: int, first_step: int, n_steps: int, flush: bool):
        """the training steps of batches first_step .. n_steps - 1 of set `cur`, each one's Adam update deferred to the next
        (+ the flush): pipelined if the sequence allows it"""
        if self._pipelines(self._ep_batches[first_step:n_steps]):
            self._lastB = self._ep_batches[n_steps - 1][1]
            self._enqueue_pipelined([self._ep_slice(b, cur) + (self._ep_plan(b, cur),) for b in range(first_step, n_steps)])
        else:
            for b in range(first_step, n_steps):
                ids, lab, _ = self._ep_slice(b, cur)
                self.train_step(ids, lab, defer=True, plan=self._ep_plan(b, cur), touched=self._ep_touch(b, cur),
                                next_touched=self._ep_next_touch(b, cur))
        if flush:
            self.flush()

    def _capture_epoch(self, cur: int, first_step: int, n_steps: int, sample, bump_counter, flush: bool, prefetch: bool,
                       on_stream: bool, primed: bool):
        """the graph of one ``epoch_run`` call shape (its arguments: the fields of the graph key) over set `cur`"""
        def warm():                              # (the warm-up leaves the staged ids - and the epoch counter - as they are)
            if first_step == 0:
                self.plan_staged(which=cur)
            elif not self._fresh:
                self._enqueue_refresh(self._ep_touch(first_step, cur))
            self._run_staged(cur, first_step, n_steps, flush)
            if prefetch or on_stream:            # (the other set's plan slots and kernels get their first use outside a capture)
                self.plan_staged(which=cur ^ 1)

        def captured():
            if not primed and first_step == 0:
                self._sample_and_plan(cur, sample, bump_counter)
            if prefetch:                         # fork: the next epoch's sampler + plans beside this epoch's steps
                main = torch.cuda.current_stream(self.dev)
                side = torch.cuda.Stream(self.dev)
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    self._sample_and_plan(cur ^ 1, sample, bump_counter)
            self._run_staged(cur, first_step, n_steps, flush)
            if prefetch:
                main.wait_stream(side)

        return self._capture_graphs([captured], warm=[warm])[0]

    def _hand_over(self, cur: int, sample, bump_counter, prefetch: bool, on_stream: bool):
        """after the replay of an epoch over set `cur`: which set is the current one, and whether it holds an epoch prepared
        ahead.  prefetch="stream" prepares it here"""
        if on_stream:
            # the next epoch's sampler + plans, on the side stream: behind the graph launched BEFORE this one (the last reader of
            # the other set), beside this one
            if self._side is None:
                self._side = torch.cuda.Stream(self.dev)
            if self._ev_free is not None:
                self._side.wait_event(self._ev_free)
            with torch.cuda.stream(self._side):
                self._sample_and_plan(cur ^ 1, sample, bump_counter)
                self._ev_ready = torch.cuda.Event()
                self._ev_ready.record(self._side)
            self._ev_free = torch.cuda.Event()
            self._ev_free.record(torch.cuda.current_stream(self.dev))    # (this epoch's graph: the last reader of the set it ran on)
        self._cur, self._cur_ready = (cur ^ 1, True) if (on_stream or prefetch) else (cur, False)

    def read_batch_lists(self, b: int):
        """The selection lists batch b of the staged epoch has in the workspace RIGHT NOW - what the last select launch on that
        batch's plan slot wrote (the data part is shared by all batches: call it before another batch is selected) - copied to
        the host: sets[r][i] for relation r, centre i.  Synchronises.  (bench.py's `verified`, tests.)"""
        g, lib = self.g, self.lib
        B = self._ep_batches[b][1]
        rows = g.R * B
        torch.cuda.synchronize(self.dev)
        off = lambda which: int(lib.pcg_choose_workspace_offset(g.desc_ref(), B, self.list_capacity, which))
        slot = self._ep_plans[b * self._ep_stride:(b + 1) * self._ep_stride]
        begin = slot[off(0):off(0) + 8 * (rows + 1)].view(torch.int64).cpu().numpy()
        length = slot[off(1):off(1) + 4 * rows].view(torch.int32).cpu().numpy()
        d0 = off(2) - self._plan_bytes(B)
        lst = self.data[d0:d0 + 4 * max(int(begin[-1]), 1)].view(torch.int32).cpu().numpy()
        sets = []
        for r in range(g.R):
            row_sets = []
            for i in range(B):
                row = r * B + i
                seg = lst[begin[row]:begin[row] + length[row]]
                row_sets.append(set(seg[seg >= 0].tolist()))
            sets.append(row_sets)
        return sets
