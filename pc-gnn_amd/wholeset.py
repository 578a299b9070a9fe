"""The whole-set calls of the fused engine: one call over the resident graph or over a query batch of unseen nodes instead of
a host loop of batches - ``infer``, ``chosen``, ``attribute``, ``embed``, ``nearest``, ``evaluate`` and the query forms
``infer_new``, ``chosen_new``, ``attribute_new``, ``embed_new`` (``WholeSetCalls``, a mix-in of ``fused.FusedPCGNN``), and the
host planner that sizes them (``infer_row_caps`` .. ``whole_set_buffers``; ``dist.DistributedPCGNN.infer`` plans with it too).

The seven entry points behind them (pcg_infer_set, pcg_embed_set, pcg_attr_set, pcg_chosen_set, pcg_infer_new, pcg_embed_new,
pcg_explain_new; include/pcgnn.h) share one call shape

    g [, q], theta, E, ids, n, chunk, s0 [, score_base], thr, ws, cap [, w0, w1], <outputs>, status, stream

which is written down once: ``whole_set_args`` puts an argument tuple in that order, ``WORKSPACES`` says which workspace an
entry point runs in and which function sizes it, ``WholeSetCalls._whole_set_call`` plans, allocates, launches and reads the status
word.  A new entry point is a row of the table and a method that allocates its outputs.
"""
import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib, ops
from .graph import AlertList, Attribution, CaseList, ChosenLists, NearestExamples, QueryBatch

_p = ops._p


def infer_row_caps(deg_host, thresholds, ids: Optional[np.ndarray] = None) -> np.ndarray:
    """List entries a test-mode selection of each id can need, summed over the relations (pcg_sel_capacity_row with no minority
    picks and no self, vectorised); ids=None: every node 0 .. n - 1, straight from the degree arrays."""
    total = None
    for r, deg in enumerate(deg_host):
        d = (deg if ids is None else deg[ids]).astype(np.int64)
        k = np.ceil(d * float(thresholds[r])).astype(np.int64)
        cap = np.where(d > k + 1, k, d)
        total = cap if total is None else total + cap
    return total if total is not None else np.zeros(0, np.int64)


def infer_chunks(caps: np.ndarray, chunk: int):
    """Chunks [lo, hi) of `chunk` consecutive ids (the last one may be shorter) and the selection-list capacity that covers the
    largest of them exactly (>= 1)."""
    n = len(caps)
    chunk = max(int(chunk), 1)
    bounds = [(lo, min(lo + chunk, n)) for lo in range(0, n, chunk)]
    if n == 0:
        return bounds, 1
    sums = np.add.reduceat(np.asarray(caps, dtype=np.int64), np.arange(0, n, chunk))
    return bounds, max(int(sums.max()), 1)


def default_infer_chunk(caps: np.ndarray, workspace_bytes, max_bytes: int, min_chunk: int = 16384) -> int:
    """The whole set in one chunk if its workspace (workspace_bytes(chunk, list_capacity)) stays within max_bytes; else halved
    until it does, down to min_chunk rows (never fewer, whatever the bound)."""
    c = max(len(caps), 1)
    while c > min_chunk:
        nbytes = workspace_bytes(c, infer_chunks(caps, c)[1])
        if 0 <= nbytes <= max_bytes:
            break
        c = max(min_chunk, (c + 1) // 2)
    return c


def host_array(x) -> np.ndarray:
    """A tensor, numpy array or list as a 1-D numpy array on the host."""
    return (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).reshape(-1)


def whole_set_ids(ids, rows: int, dev, what: str, note: str = "", all_ids: Optional[torch.Tensor] = None):
    """The ids of a whole-set call (a tensor, numpy array or list of row numbers in [0, rows); None = every row) as
    (ids_host int64 - None when ids is None -, ids_dev int32 on dev, n).  all_ids: the caller's cached arange(rows) for None.
    `what` names the method and its argument in the range error (f"{what} outside 0 .. {rows - 1}{note}")."""
    if ids is None:
        if all_ids is None or all_ids.numel() != rows:
            all_ids = torch.arange(rows, dtype=torch.int32, device=dev)
        return None, all_ids, rows
    ids_host = host_array(ids).astype(np.int64)
    n = int(ids_host.size)
    if n and (ids_host.min() < 0 or ids_host.max() >= rows):
        raise ValueError(f"{what} outside 0 .. {rows - 1}{note}")
    ids_dev = ops._i32(ids, dev).view(-1) if torch.is_tensor(ids) else torch.from_numpy(ids_host.astype(np.int32)).to(dev)
    return ids_host, ids_dev, n


def whole_set_workspace(inf: dict, key: str, dev, ws_bytes, what: str, chunk: int, cap: int, need: Optional[int] = None):
    """inf[key]: the grow-only device workspace of a whole-set call, of at least ws_bytes(chunk, cap) bytes (and of
    ws_bytes(chunk, need), when a list capacity other than the exact one, `need`, was forced)."""
    nbytes = ws_bytes(chunk, cap)
    if nbytes >= 0 and need is not None:
        nbytes = max(nbytes, ws_bytes(chunk, need))
    if nbytes < 0:
        raise _lib.PcgnnLibraryError(f"{what} rejected chunk {chunk} / list capacity {cap} ({nbytes})")
    if inf.get(key) is None or inf[key].numel() < nbytes:
        inf[key] = None
        inf[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return inf[key]


def whole_set_chunk(inf: dict, key: str, dev, ws_bytes, what: str, caps: np.ndarray, chunk: Optional[int], max_bytes: int,
                    list_capacity: Optional[int] = None):
    """(chunk, list capacity, workspace) of a whole-set call over len(caps) > 0 ids: the caller's chunk (None: default_infer_chunk)
    clamped to the set, the capacity that covers its largest chunk exactly, and inf[key] grown to hold them.  list_capacity
    forces another capacity (the tests' way to an overflow): a bounded list that overflows leaves the dense launch walking the
    chunk offsets the plan worked out for the rows of several chunks - the buffer is as large as the exact capacity's, so those
    reads stay inside it."""
    chunk = default_infer_chunk(caps, ws_bytes, max_bytes) if chunk is None else int(chunk)
    chunk = max(1, min(chunk, len(caps)))
    _, need = infer_chunks(caps, chunk)
    cap = need if list_capacity is None else max(int(list_capacity), 1)
    return chunk, cap, whole_set_workspace(inf, key, dev, ws_bytes, what, chunk, cap, need)


def whole_set_buffers(inf: dict, dev, s0_key: str, need: int, alloc: Optional[int] = None) -> bool:
    """inf["status"] (the call's status word) and inf[s0_key] (its score buffer, at least `need` floats; a new one has `alloc`),
    created when missing.  True: the score buffer is new and holds no scores."""
    if inf.get("status") is None:
        inf["status"] = torch.zeros(1, dtype=torch.int32, device=dev)
    if inf.get(s0_key) is not None and inf[s0_key].numel() >= need:
        return False
    inf[s0_key] = None
    inf[s0_key] = torch.zeros(alloc or need, dtype=torch.float32, device=dev)
    return True


# entry point -> (its workspace's key in the engine's ``_inf``, the function that sizes it: (g [, q] [, emb], chunk, capacity);
# pcg_chosen_workspace_bytes takes no emb - no dense launch runs in that workspace)
WORKSPACES = {
    "pcg_infer_set": ("ws", "pcg_infer_workspace_bytes"),
    "pcg_embed_set": ("ws", "pcg_infer_workspace_bytes"),
    "pcg_attr_set": ("ws", "pcg_infer_workspace_bytes"),
    "pcg_chosen_set": ("chosen_ws", "pcg_chosen_workspace_bytes"),
    "pcg_infer_new": ("new_ws", "pcg_infer_new_workspace_bytes"),
    "pcg_embed_new": ("new_ws", "pcg_infer_new_workspace_bytes"),
    "pcg_explain_new": ("new_ws", "pcg_explain_new_workspace_bytes"),
}


def whole_set_args(head, sizing, outputs, tail, query=None, weights=()) -> tuple:
    """The argument tuple of any whole-set entry point, in the header's order: head (g, theta, E, ids, n, chunk, s0), sizing
    (thr, ws, cap), the call's own outputs, tail (status, stream); query (q, score_base) - q follows g, score_base follows s0 -
    for the calls over a query batch, weights (w0, w1) for the attributing ones."""
    head = tuple(head)
    if query is not None:
        q, score_base = query
        head = head[:1] + (q,) + head[1:] + (score_base,)
    return head + tuple(sizing) + tuple(weights) + tuple(outputs) + tuple(tail)


def _target_weights(what: str, target):
    """(w0, w1) of ``target`` for the public method `what`: two finite floats, else ValueError"""
    try:
        w0, w1 = (float(t) for t in target)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: target must be two finite floats, got {target!r}") from None
    if not (np.isfinite(w0) and np.isfinite(w1)):
        raise ValueError(f"{what}: target must be two finite floats, got {target!r}")
    return w0, w1


class EvalCalls:
    """What an engine with ``infer`` gets for nothing, as a mix-in without state: the metrics of a node set without its
    probabilities leaving the device (``evaluate``, ``evaluate_ranking``) and the alert list (``alerts``).  What it uses of the
    engine: ``infer(ids, chunk=)``, ``g``, ``dev``, ``flush()`` and ``_inf`` (all_ids, eval_labels) - ``alerts(query=)`` also
    ``infer_new`` / ``_new_query``.  ``WholeSetCalls`` (FusedPCGNN) and ``baseline.BaselineEngine`` (GraphSAGE / GCN) inherit it."""

    def _resident_ids(self, ids, what: str):
        """What every call over the resident graph does first: a deferred update applied; -> whole_set_ids of ``ids`` (None =
        every node: the arange is kept for the next call)."""
        inf = self._inf
        self.flush()
        ids_host, ids_dev, n = whole_set_ids(ids, self.g.n_nodes, self.dev, f"{what}: ids", all_ids=inf.get("all_ids"))
        if ids is None:
            inf["all_ids"] = ids_dev
        return ids_host, ids_dev, n

    def evaluate(self, ids, labels, thresholds=None, chunk: Optional[int] = None) -> dict:
        """The evaluation metrics of a node set without its probabilities leaving the device: ``infer`` -> sigmoid (torch, so
        the scores are the very float32 values ``utils.predict_proba`` hands the host) -> the integer counts (pcg_eval_counts)
        -> ``utils.metrics_from_counts``: every value ``==`` what ``utils.test`` / ``test_f1`` compute on the host.  ids as
        ``infer`` (None = every node); labels: the ids' labels (host sequence or tensor) - they go to the device once and are
        kept for the next pass over the same labels object / the same values; thresholds: None = linspace(0.01, 0.99, 100)."""
        from . import utils as U
        lab = self._eval_labels(labels)
        with torch.no_grad():
            prob = torch.sigmoid(self.infer(ids, chunk=chunk)).float()
        if lab.numel() != prob.shape[0]:
            raise ValueError(f"evaluate: {lab.numel()} labels for {prob.shape[0]} ids")
        return U.device_metrics(prob, lab, thresholds)

    def evaluate_ranking(self, ids, labels, ks=(100, 1000), chunk: Optional[int] = None) -> dict:
        """The ranking metrics of a node set without its probabilities leaving the device: ``infer`` -> sigmoid -> pcg_pr_counts
        (+ pcg_topk_alerts, a gather of the labels and a cumulative sum when ``ks`` is given) -> ``utils.ranking_from_counts``.
        Keys: average_precision, gmean (of the argmax prediction), precision_at / recall_at (dicts keyed by k: the positives
        among the first min(k, n) alerts over min(k, n) / over the number of positives), n_pos, n_points.  The alert order is
        the stable sort by probability, descending; a tie at the cut k is resolved by input position (the lower position in
        ``ids`` first).  Every value ``==`` ``utils.host_ranking`` on ``utils.predict_proba``'s output.  ids, labels: as
        ``evaluate``; labels from the host also size the point arrays (their number of positives)."""
        from . import utils as U
        lab = self._eval_labels(labels)
        cap = None if torch.is_tensor(labels) else int(np.count_nonzero(np.asarray(labels)))
        with torch.no_grad():
            prob = torch.sigmoid(self.infer(ids, chunk=chunk)).float()
        if lab.numel() != prob.shape[0]:
            raise ValueError(f"evaluate_ranking: {lab.numel()} labels for {prob.shape[0]} ids")
        return U.device_ranking(prob, lab, ks, cap=cap)

    def alerts(self, ids=None, k: int = 100, chunk: Optional[int] = None, labels=None, query: Optional[QueryBatch] = None) -> AlertList:
        """The alert list: the k rows of the requested set with the highest positive-class probability, as ``graph.AlertList``
        (ids / pos / prob [k] on the device, padded with -1 / -1 / -inf when the set has fewer than k rows): ``infer`` -> sigmoid
        -> pcg_topk_alerts.  The order is the stable sort by probability, descending: among equal probabilities - test-mode
        scores tie often, at saturated logits and on identical neighbourhoods - the lower position in ``ids`` comes first, so a
        tie at the cut k is resolved by input position and the list is the same on every run.  ids: as ``infer`` (None = every
        node); 1 <= k <= 65536.  labels (one per requested row, 0 / 1): the result also holds ``hits`` [k], the positives among
        the alerts up to each slot.  query: the rows of that ``graph.QueryBatch`` are ranked through ``infer_new`` instead; ids
        (and the returned ids) are then query-local.  Synchronises (the status words)."""
        with torch.no_grad():
            if query is None:
                _, ids_dev, n = self._resident_ids(ids, "alerts")
                prob = torch.sigmoid(self.infer(ids, chunk=chunk)).float()
            else:
                _, ids_dev, n = self._new_query(query, ids, "alerts")
                prob = torch.sigmoid(self.infer_new(query, ids=ids, chunk=chunk)).float()
            status = ops.eval_status(self.dev)
            pos, score = ops.topk_alerts(prob, int(k))
            safe = pos.clamp(min=0).long()
            out_ids = torch.where(pos >= 0, ids_dev[safe] if n else torch.zeros_like(pos), torch.full_like(pos, -1))
            hits = None
            if labels is not None:
                lab = self._eval_labels(labels)
                if lab.numel() != n:
                    raise ValueError(f"alerts: {lab.numel()} labels for {n} rows")
                taken = (lab[safe] != 0) & (pos >= 0) if n else torch.zeros_like(pos, dtype=torch.bool)
                hits = torch.cumsum(taken.to(torch.int64), 0)
            st = int(status.item())
            if st:
                status.zero_()
                raise _lib.PcgnnLibraryError("alerts: a NaN probability" if st & _lib.PCG_ST_EVAL_INPUT else f"device status {st}")
        return AlertList(out_ids, pos, score, n, hits)

    def cases(self, ids=None, k: int = 100, relations=None, chunk: Optional[int] = None, labels=None, query=None) -> CaseList:
        """The alert list grouped into cases, as ``graph.CaseList``: ``alerts(ids, k, chunk)`` -> pcg_alert_cases on its ids.  Two
        alerts are linked when they are the same node or when, in a selected relation of the resident graph, either is in the
        other's CSR row; a case is a connected component, its head the highest-ranked alert in it, and cases are numbered by
        their heads, so case 0 holds alert 0 - every integer the same on every run, like the alert order itself.  relations:
        None = all, else a non-empty subset of range(R).  labels (one per requested row, 0 / 1, as for ``alerts``): gathered to
        the slots; the result holds ``hits`` [C], the positives per case.  The alert list is attached (``.alerts``).
        Out of scope: ``query=`` batches (their ids are query-local: ValueError), partitioned graphs (``DistributedPCGNN``),
        2-hop linking, more than 65536 alerts.  Synchronises (the alert list's status word, then the case header)."""
        if query is not None:
            raise ValueError("cases: a query batch's alert ids are query-local; grouping them against the resident graph is not supported")
        ops.relation_mask(self.g, relations)                               # (a bad relation set fails before the inference pass)
        al = self.alerts(ids, k=k, chunk=chunk)
        slot_labels = None
        if labels is not None:
            lab = self._eval_labels(labels)
            if lab.numel() != al.n:
                raise ValueError(f"cases: {lab.numel()} labels for {al.n} rows")
            slot_labels = lab[al.pos.clamp(min=0).long()] if al.n else torch.zeros_like(al.pos)
        return ops.group_members(self.g, al.ids, relations=relations, labels=slot_labels, alerts=al)

    def _eval_labels(self, labels) -> torch.Tensor:
        if torch.is_tensor(labels):
            return ops._i32(labels, self.dev).view(-1)
        host = np.ascontiguousarray(np.asarray(labels).reshape(-1), dtype=np.int32)
        cache = self._inf.setdefault("eval_labels", {})
        key = host.size                                  # (one set per size: train-time validation and the final test alternate)
        hit = cache.get(key)
        if hit is None or not np.array_equal(hit[0], host):
            if len(cache) >= 4:
                cache.clear()
            hit = cache[key] = (host.copy(), torch.from_numpy(host).to(self.dev))
        return hit[1]


class WholeSetCalls(EvalCalls):
    """The whole-set surface of ``fused.FusedPCGNN``, as a mix-in: it has no state and no ``__init__`` of its own.  What it uses
    of the engine: ``g``, ``lib``, ``dev``, ``E``, ``theta``, ``thresholds``, ``rho``, ``_thr``; ``_stream()``, ``flush()``,
    ``_raise_status``; ``_param_version``, ``infer_workspace_bytes``, ``_inf`` (every buffer and cache of these calls, grown on
    demand: status, s0, new_s0, new_s0_version, ws, chosen_ws, new_ws, pos_keys, all_ids, bank, eval_labels) and
    ``_new_scored_base`` - all of them created by the engine's ``__init__``."""

    def _whole_set_call(self, name: str, ids_dev, n: int, caps, chunk, outputs, query: Optional[QueryBatch] = None,
                        reuse_scores: bool = True, weights=(), list_capacity: Optional[int] = None, read_status: bool = True):
        """One whole-set entry point `name` over n > 0 ids whose rows need ``caps`` list entries each: chunk, list capacity and
        workspace picked (WORKSPACES; list_capacity forces a capacity), the score buffer at hand (the resident table, or - query -
        the query calls' with its cached base scores), the call enqueued, the status word read.  outputs: the call's own, tensors
        or None (anything else is passed as it is).  read_status=False: the caller enqueues more and reads the word itself."""
        g, lib, inf = self.g, self.lib, self._inf
        key, size_name = WORKSPACES[name]
        size_fn = getattr(lib, size_name)
        lead = (g.desc_ref(),) if query is None else (g.desc_ref(), query.desc_ref())
        if size_name != "pcg_chosen_workspace_bytes":
            lead += (self.E,)
        chunk, cap, ws = whole_set_chunk(inf, key, self.dev, lambda c, cap: int(size_fn(*lead, c, cap)), size_name, caps, chunk,
                                         self.infer_workspace_bytes, list_capacity)
        if query is None:
            whole_set_buffers(inf, self.dev, "s0", g.n_nodes)
            s0, q_part = inf["s0"], None
        else:
            score_base = self._new_scores(query, reuse_scores)
            s0, q_part = inf["new_s0"], (query.desc_ref(), 1 if score_base else 0)
        outs = [_p(o) if o is None or torch.is_tensor(o) else o for o in outputs]
        _lib.check(getattr(lib, name)(*whole_set_args(
            (g.desc_ref(), _p(self.theta), self.E, _p(ids_dev), n, chunk, _p(s0)), (self._thr, _p(ws), cap), outs,
            (_p(inf["status"]), self._stream()), q_part, weights)), name)
        if query is not None:
            # (the table pass is enqueued before anything that could overflow: the scores are valid whatever the status says)
            inf["new_s0_version"] = self._param_version
        if read_status:
            self._infer_status()

    def _infer_outputs(self, n: int, want_center: bool):
        logits = torch.empty(n, 2, dtype=torch.float32, device=self.dev)
        center = torch.empty(n, 2, dtype=torch.float32, device=self.dev) if want_center else None
        return logits, center

    @staticmethod
    def _infer_result(logits, center):
        return logits if center is None else (logits, center)

    def infer(self, ids=None, chunk: Optional[int] = None, want_center: bool = False):
        """Test-mode logits of a whole node set in one call (pcg_infer_set): ONE score pass, then per chunk of ids plan ->
        select -> gather -> a persistent forward-only dense launch.  ids: node ids (any order, duplicates allowed; a device
        tensor, numpy array or list), None = every node 0 .. n_nodes - 1.  Returns the gnn logits [n, 2] (+ the label-aware
        logits [n, 2] if want_center): bit for bit what ``predict(ids[b:b + B], None, False)`` returns batch by batch, for any
        B and any chunk.  chunk: ids per chunk (default: all of them, or fewer - never under 16384 - if the workspace would
        exceed infer_workspace_bytes).  The training engine is left alone: its score table, keys, plans, captured graphs and
        buffer sizes are untouched (a deferred update is applied first, as predict does).  Synchronises once (the status word)."""
        ids_host, ids_dev, n = self._resident_ids(ids, "infer")
        logits, center = self._infer_outputs(n, want_center)
        if n:
            self._whole_set_call("pcg_infer_set", ids_dev, n, infer_row_caps(self.g.deg_host, self.thresholds, ids_host), chunk,
                                 (logits, center))
        return self._infer_result(logits, center)

    def chosen(self, ids=None, chunk: Optional[int] = None, labels=None, train_flag: bool = False) -> ChosenLists:
        """WHY a node scores as it does: for every requested node and relation, the neighbours the test-mode selection kept - the
        selection ``infer`` and a deployed model use - in the reference's order with their distances (choose_step_test's
        samp_neighs / samp_scores, src/layers.py:713-736), on the device (pcg_chosen_set): ONE score pass, then per chunk of ids
        plan -> select -> rank; no gather, no dense launch.  ids, chunk: as ``infer`` (None = every node; any order, duplicates
        allowed; a device tensor, numpy array or list; range-checked on the host).  The output offsets are host arithmetic on
        the degrees (a test-mode row keeps exactly deg > k + 1 ? k : deg entries), so the result is sized exactly.  Returns a
        ``ChosenLists``.  The training engine is left alone exactly as by ``infer`` (a deferred update is applied first).
        Synchronises once (the status word).
        train_flag=True, labels (one per id, 0 / 1): the TRAIN-mode lists (choose_step_neighs, src/layers.py:633-697).  The
        neighbour part is the one above, unchanged - k and the keep-all rule are the same in both modes -; the result carries
        the minority part beside it (``minor_row``, ``has_minority``): per row of a positive centre the m = min(int(k * rho),
        n_pos) training positives nearest to its score, ranked, with their distances (pcg_rank_minority, one more pass over all
        n ids after the chunks; the train-positive keys of the call's own scores are sorted into a buffer of the call's own -
        the training engine's keys are neither read nor written).
        Nodes that are not in the graph (``infer_new``'s query batches): ``chosen_new`` (test mode only)."""
        g, lib, inf = self.g, self.lib, self._inf
        if train_flag and labels is None:
            raise ValueError("chosen: train_flag=True needs labels (one per id)")
        ids_host, ids_dev, n = self._resident_ids(ids, "chosen")
        if ids_host is None:
            ids_host = np.arange(n, dtype=np.int64)                                   # (ops.sel_capacity indexes the degrees)
        minor = {}
        if train_flag:
            labels_host = host_array(labels)
            if labels_host.size != n:
                raise ValueError(f"chosen: {labels_host.size} labels for {n} ids")
            if n and not np.isin(labels_host, (0, 1)).all():
                raise ValueError("chosen: labels must be 0 or 1")
            moff = ops.rank_offsets(ops.minority_counts(g, ids_host, labels_host, self.thresholds, self.rho))
            minor = dict(minor_flat_offsets=torch.from_numpy(moff).to(self.dev), minor_host_offsets=moff,
                         minor_ids=torch.empty(int(moff[-1]), dtype=torch.int32, device=self.dev),
                         minor_dist=torch.empty(int(moff[-1]), dtype=torch.float32, device=self.dev))
        caps2 = ops.sel_capacity(g, ids_host, None, self.thresholds, 0.0, False)      # [R, n]: exact in test mode
        off = ops.rank_offsets(caps2)
        total = int(off[-1])
        out_begin = torch.from_numpy(off).to(self.dev)
        out_ids = torch.empty(total, dtype=torch.int32, device=self.dev)
        out_dist = torch.empty(total, dtype=torch.float32, device=self.dev)
        res = ChosenLists(out_begin, out_ids, out_dist, g.R, n, host_offsets=off, **minor)
        if n == 0:
            return res
        # (the sum == infer_row_caps; the status word is read below, after the minority pass)
        self._whole_set_call("pcg_chosen_set", ids_dev, n, caps2.sum(0), chunk, (out_begin, out_ids, out_dist), read_status=False)
        if minor and g.n_pos and int(minor["minor_host_offsets"][-1]):
            cap_keys = int(lib.pcg_pos_sort_capacity(g.n_pos))
            if inf.get("pos_keys") is None or inf["pos_keys"].numel() < cap_keys:
                inf["pos_keys"] = torch.empty(cap_keys, dtype=torch.int64, device=self.dev)
            ops.pos_sort(g, inf["s0"], inf["pos_keys"])
            ops.rank_minority(g, ids_dev, inf["s0"], inf["pos_keys"], minor["minor_flat_offsets"], minor["minor_ids"],
                              minor["minor_dist"], inf["status"])
        self._infer_status()
        return res

    def attribute(self, ids=None, chunk: Optional[int] = None, target=(0.0, 1.0), neighbours: bool = False) -> Attribution:
        """WHAT pushed a node's score: the exact split of ``target[0] * logit0 + target[1] * logit1`` (default: the fraud logit,
        whose sigmoid is the probability ``evaluate`` / ``predict_proba`` report; (-1, 1): the margin) into the shares of the
        node's own features, of every relation and - neighbours=True - of every chosen neighbour (pcg_attr_set,
        pcg_attr_neighbours).  The gnn path has no bias, so with the test-mode selection held fixed (it is not differentiable; the
        reference's autograd treats it the same way) the scalar is positively homogeneous of degree 1 in the node's row and the
        means of its chosen rows: gradient times input adds up to it exactly (``Attribution.completeness_residual``).
        ids, chunk: as ``infer`` (None = every node; any order, duplicates allowed; a device tensor, numpy array or list;
        range-checked on the host).  ``infer``'s launches with the backward to the inputs behind each tile's forward: the
        result's logits are ``infer(ids)`` bit for bit, and a node's values do not depend on its position, chunk or company.
        neighbours=True calls ``chosen(ids)`` and adds its lists and ``neigh_contrib`` beside them.  The training engine is left
        alone exactly as by ``infer`` (a deferred update is applied first).  Synchronises once (the status word; once more per
        ``chosen`` call).  target: two finite floats, else ValueError.
        Nodes that are not in the graph (``infer_new``'s query batches): ``attribute_new``.
        Out of scope: ``DistributedPCGNN``, the train-mode selection and its minority picks, the GraphSAGE / GCN baselines."""
        g, inf = self.g, self._inf
        weights = _target_weights("attribute", target)
        ids_host, ids_dev, n = self._resident_ids(ids, "attribute")
        F, R, f32 = g.feat_dim, g.R, dict(dtype=torch.float32, device=self.dev)
        res = Attribution(ids_dev, g.X, F, torch.empty(n, 2, **f32), torch.empty(n, F, **f32), torch.empty(R, n, F, **f32),
                          torch.empty(n, **f32), torch.empty(R, n, **f32), weights)
        if n:
            # (neighbours: chosen reads the status word itself - the attribution's launches are covered by that read)
            self._whole_set_call("pcg_attr_set", ids_dev, n, infer_row_caps(g.deg_host, self.thresholds, ids_host), chunk,
                                 (res.logits, res.d_self, res.d_agg, res.self_contrib, res.rel_contrib), weights=weights,
                                 read_status=not neighbours)
        if neighbours:
            if n:
                res.chosen = self.chosen(ids if ids is None else ids_dev, chunk=chunk)
                res.neigh_contrib = ops.neighbour_contrib(g, res.chosen, res.d_agg, status=inf["status"])
                self._infer_status()
            else:
                res.chosen = self.chosen(ids_dev)
                res.neigh_contrib = torch.empty(0, **f32)
        return res

    def _infer_status(self):
        """the status word of an infer / infer_new call: one read (synchronises); a set bit is cleared and raised"""
        st = int(self._inf["status"].item())
        if st:
            self._inf["status"].zero_()
            self._raise_status(st)

    def infer_new(self, query: QueryBatch, ids=None, chunk: Optional[int] = None, want_center: bool = False,
                  reuse_scores: bool = True, _list_capacity: Optional[int] = None):
        """Test-mode logits of nodes that are NOT in the graph (pcg_infer_new): ``query`` holds nq new nodes - a feature row
        each and, per relation, a neighbour list of global ids in [0, N + nq), query node j being N + j (graph.QueryBatch).
        Returns the gnn logits [n, 2] (+ the label-aware logits [n, 2] if want_center) of the query rows ``ids`` (query-local,
        any order, duplicates allowed; None = all nq): bit for bit what ``infer`` would return for node N + j on a graph built
        with the query rows appended - a node's test-mode logits depend on its own row, its own lists, the scores and rows
        of those neighbours and the parameters, on nothing else.  The base graph is not modified, nothing of it is
        recomputed, and the batch is not appended to it.  chunk as ``infer``'s, over the query's degrees.
        The base table's scores are kept between calls (a buffer of N + capacity floats) and reused while nothing has written
        the parameters since (training steps, epoch runs, a flush with an update pending, ``params_changed``, a loaded state
        dict - a parameter-version counter); a warm call scores the nq query rows only.  reuse_scores=False forces the table
        pass.  The training engine is left alone exactly as by ``infer`` (a deferred update is applied first).  Synchronises
        once (the status word).  (_list_capacity: not part of the interface - the tests' way to make a selection list
        overflow; the call sizes its list exactly.)"""
        ids_host, ids_dev, n = self._new_query(query, ids, "infer_new")
        logits, center = self._infer_outputs(n, want_center)
        if n:
            self._whole_set_call("pcg_infer_new", ids_dev, n, infer_row_caps(query.deg_host, self.thresholds, ids_host), chunk,
                                 (logits, center), query, reuse_scores, list_capacity=_list_capacity)
        return self._infer_result(logits, center)

    # -- embeddings and nearest labelled examples --------------------------------------------------------
    # Out of scope: DistributedPCGNN, the GraphSAGE / GCN models, train-mode selection (the embeddings are the test-mode ones).
    def _embed_outputs(self, n: int, relations: bool, want_logits: bool):
        emb = torch.empty(n, self.E, dtype=torch.float32, device=self.dev)
        rel = torch.empty(n, self.g.R * self.E, dtype=torch.float32, device=self.dev) if relations else None
        logits = torch.empty(n, 2, dtype=torch.float32, device=self.dev) if want_logits else None
        return emb, rel, logits

    def _embed_result(self, emb, rel, logits):
        res = (emb,)
        if rel is not None:
            res += (rel.view(rel.shape[0], self.g.R, self.E),)
        if logits is not None:
            res += (logits,)
        return res[0] if len(res) == 1 else res

    def embed(self, ids=None, chunk: Optional[int] = None, relations: bool = False, want_logits: bool = False):
        """The vector the classifier sees, for a whole node set in one call (pcg_embed_set: ``infer``'s launches, whose dense
        launch also stores the rows): emb [n, E] = relu([self | h_1 .. h_R] W), the row W_cls multiplies - bit for bit what
        ``predict(ids[b:b + B], want_combined=True)`` returns batch by batch, for any B and any chunk.  relations=True: also
        h [n, R, E], the per-relation embeddings h_r = relu([self | agg_r] W_r) (a view of an [n, R * E] buffer);
        want_logits=True: also the gnn logits [n, 2], bit for bit ``infer``'s.  ids and chunk as ``infer``'s; the training
        engine is left alone as by ``infer`` (a deferred update is applied first).  Synchronises once (the status word).
        Test mode only; not for DistributedPCGNN or the GraphSAGE / GCN models."""
        ids_host, ids_dev, n = self._resident_ids(ids, "embed")
        emb, rel, logits = self._embed_outputs(n, relations, want_logits)
        if n:
            self._whole_set_call("pcg_embed_set", ids_dev, n, infer_row_caps(self.g.deg_host, self.thresholds, ids_host), chunk,
                                 (logits, None, emb, rel))
        return self._embed_result(emb, rel, logits)

    def embed_new(self, query: QueryBatch, ids=None, chunk: Optional[int] = None, relations: bool = False,
                  want_logits: bool = False, reuse_scores: bool = True):
        """``embed`` for nodes that are NOT in the graph (pcg_embed_new over ``infer_new``'s launches): the rows ``ids``
        (query-local; None = all nq) of a ``graph.QueryBatch`` -> emb [n, E] (+ h [n, R, E], + logits [n, 2]), bit for bit
        what ``embed`` returns for node N + j on a graph built with the query rows appended.  Shares ``infer_new``'s base-score
        cache (reuse_scores as there).  Synchronises once (the status word)."""
        ids_host, ids_dev, n = self._new_query(query, ids, "embed_new")
        emb, rel, logits = self._embed_outputs(n, relations, want_logits)
        if n:
            self._whole_set_call("pcg_embed_new", ids_dev, n, infer_row_caps(query.deg_host, self.thresholds, ids_host), chunk,
                                 (logits, None, emb, rel), query, reuse_scores)
        return self._embed_result(emb, rel, logits)

    def _nearest_bank(self, among, chunk):
        """(among ids on the device, their embeddings [M, E]): cached until the parameters or ``among`` change"""
        g, inf = self.g, self._inf
        among_host = np.asarray(g.train_pos_host, dtype=np.int64) if among is None else host_array(among).astype(np.int64)
        self.flush()                                       # (a pending update bumps the version: before it is compared)
        b = inf.get("bank")
        if b is not None and b["version"] == self._param_version and np.array_equal(b["among_host"], among_host):
            return b["among"], b["emb"]
        inf["bank"] = None
        emb = self.embed(among_host, chunk=chunk)
        among_dev = torch.from_numpy(among_host.astype(np.int32)).to(self.dev)
        inf["bank"] = {"version": self._param_version, "among_host": among_host, "among": among_dev, "emb": emb}
        return among_dev, emb

    def nearest(self, ids=None, k: int = 5, among=None, metric: str = "cosine", exclude_self: bool = True,
                chunk: Optional[int] = None, query: Optional[QueryBatch] = None) -> NearestExamples:
        """Which labelled examples each node looks like: the k nodes of ``among`` (node ids; None = the graph's training
        positives, ``g.train_pos``) whose embeddings (``embed``) are most similar to each requested node's, as
        ``graph.NearestExamples`` (ids / pos / score [n, k], sorted by score descending, ties by lower position in ``among``,
        padded with -1 / -inf).  metric: "cosine" (0 for an all-zero embedding), "dot", or "l2" (minus the squared distance).
        exclude_self: a node is never its own example.  query: the searched rows are ``embed_new(query, ids)`` instead (ids
        query-local; query node j has the global id N + j, which is never in ``among``).
        The bank ``embed(among)`` is kept on the engine and rebuilt when the parameters or ``among`` change.  The requested
        rows are embedded and searched a chunk at a time (``chunk`` rows, default as ``infer``'s): the call holds the outputs,
        the bank and one chunk of embeddings - never an [n, M] matrix (pcg_topk_similar).  Test mode only; not for
        DistributedPCGNN or the GraphSAGE / GCN models."""
        g = self.g
        if metric not in ops.TOPK_METRICS:
            raise ValueError(f"nearest: metric {metric!r} is none of {sorted(ops.TOPK_METRICS)}")
        among_dev, bank = self._nearest_bank(among, chunk)
        if query is None:
            ids_host, ids_dev, n = whole_set_ids(ids, g.n_nodes, self.dev, "nearest: ids", all_ids=self._inf.get("all_ids"))
            gid = ids_dev
        else:
            ids_host, ids_dev, n = self._new_query(query, ids, "nearest")
            gid = ids_dev + g.n_nodes
        k = int(k)
        pos = torch.empty(n, k, dtype=torch.int32, device=self.dev)
        score = torch.empty(n, k, dtype=torch.float32, device=self.dev)
        step = n if chunk is None else max(int(chunk), 1)
        if chunk is None and n > (1 << 20):
            step = 1 << 20
        for lo in range(0, n, max(step, 1)):
            hi = min(lo + step, n)
            part = ids_dev[lo:hi]
            q = self.embed(part, chunk=chunk) if query is None else self.embed_new(query, part, chunk=chunk)
            p, s = ops.topk_similar(q, bank, k, metric, gid[lo:hi] if exclude_self else None, among_dev if exclude_self else None)
            pos[lo:hi], score[lo:hi] = p, s
        safe = pos.clamp(min=0).long()
        ex_ids = torch.where(pos >= 0, among_dev[safe] if among_dev.numel() else torch.zeros_like(pos), torch.full_like(pos, -1))
        return NearestExamples(ex_ids, pos, score, among_dev, metric)

    def _new_query(self, query: QueryBatch, ids, what: str):
        """What every query call does first: a deferred update applied, the batch checked against this engine's graph and
        uploaded for it if it is not; -> whole_set_ids of the query-local ``ids`` (None = all nq)."""
        g = self.g
        self.flush()
        if query.n_base != g.n_nodes or query.feat_dim != g.feat_dim or query.R != g.R:
            raise ValueError(f"{what}: the query batch was built for a base graph of {query.n_base} nodes / {query.feat_dim} "
                             f"features / {query.R} relations, this engine's has {g.n_nodes} / {g.feat_dim} / {g.R}")
        if query.X is None or query.device != self.dev or query.feat_stride != g.feat_stride:
            query.to(self.dev, g)
        return whole_set_ids(ids, query.nq, self.dev, f"{what}: ids", " (query-local rows)")

    def _new_scores(self, query: QueryBatch, reuse_scores: bool) -> bool:
        """The score buffer of the query calls (inf["new_s0"], N + capacity floats) for this batch; -> whether the call has to
        run the base table's score pass (the buffer is new, the parameters were written since it was filled, or the caller
        says so)."""
        g, inf, nq = self.g, self._inf, query.nq
        # a grown buffer holds no scores: capacity in powers of two, so a stream of batches grows it a few times at most
        if whole_set_buffers(inf, self.dev, "new_s0", g.n_nodes + nq, g.n_nodes + (1 << max(nq - 1, 255).bit_length())):
            inf["new_s0_version"] = None
        score_base = not (reuse_scores and inf["new_s0_version"] == self._param_version)
        self._new_scored_base = score_base          # (whether the last query call ran the table pass: tests, scripts)
        return score_base

    def _explain_new(self, what: str, query: QueryBatch, ids, chunk, target, want_attr: bool, want_chosen: bool, reuse_scores: bool,
                     list_capacity: Optional[int]):
        """chosen_new / attribute_new: ONE pcg_explain_new call - one selection per chunk feeds the ranking and the attribution.
        -> (Attribution or None, ChosenLists or None)."""
        g = self.g
        weights = _target_weights(what, target)
        ids_host, ids_dev, n = self._new_query(query, ids, what)
        if ids_host is None:
            ids_host = np.arange(n, dtype=np.int64)                                      # (ops.sel_capacity indexes the degrees)
        F, R, f32 = g.feat_dim, g.R, dict(dtype=torch.float32, device=self.dev)
        out = _lib.ExplainOut()
        attr = chosen = None
        caps2 = ops.sel_capacity(query, ids_host, None, self.thresholds, 0.0, False)     # [R, n]: exact in test mode
        if want_chosen:
            off = ops.rank_offsets(caps2)
            total = int(off[-1])
            out_begin = torch.from_numpy(off).to(self.dev)
            # (at least one entry behind every pointer: an empty tensor has none, and a NULL member means "group not requested")
            ids_buf, dist_buf = torch.empty(max(total, 1), dtype=torch.int32, device=self.dev), torch.empty(max(total, 1), **f32)
            chosen = ChosenLists(out_begin, ids_buf[:total], dist_buf[:total], R, n, host_offsets=off)
            out.out_begin, out.out_ids, out.out_dist = _p(out_begin), _p(ids_buf), _p(dist_buf)
        if want_attr:
            attr = Attribution(ids_dev, query.X, F, torch.empty(n, 2, **f32), torch.empty(n, F, **f32), torch.empty(R, n, F, **f32),
                               torch.empty(n, **f32), torch.empty(R, n, **f32), weights)
            out.logits, out.d_self, out.d_agg = _p(attr.logits), _p(attr.d_self), _p(attr.d_agg)
            out.self_contrib, out.rel_contrib = _p(attr.self_contrib), _p(attr.rel_contrib)
            if want_chosen:
                nc_buf = torch.empty(max(total, 1), **f32)
                attr.chosen, attr.neigh_contrib = chosen, nc_buf[:total]
                out.neigh_contrib = _p(nc_buf)
        if n:
            self._whole_set_call("pcg_explain_new", ids_dev, n, caps2.sum(0), chunk, (C.byref(out),), query, reuse_scores,
                                 weights, list_capacity)                                 # (the sum == infer_row_caps)
        return attr, chosen

    def chosen_new(self, query: QueryBatch, ids=None, chunk: Optional[int] = None, reuse_scores: bool = True,
                   _list_capacity: Optional[int] = None) -> ChosenLists:
        """``chosen`` for nodes that are NOT in the graph: for every requested row of ``query`` (graph.QueryBatch, as
        ``infer_new``'s) and every relation, the neighbours the test-mode selection kept - the selection ``infer_new`` scores
        the row with - in the reference's order, with their distances (pcg_explain_new, its chosen group alone: per chunk plan
        -> select -> rank; no gather, no dense launch).  ids: query-local rows in [0, nq) (None = all; any order, duplicates
        allowed); the ids IN the returned lists are global, in [0, N + nq): base nodes, other nodes of the batch (N + j), the
        node itself.  The offsets are host arithmetic on the query's degrees (a row keeps deg > k + 1 ? k : deg entries).
        Bit for bit what ``chosen(N + ids)`` returns on a graph built with the query rows appended.  chunk, reuse_scores and
        the cached base scores: ``infer_new``'s - a call after ``infer_new`` (or another query call) scores the nq query rows
        only.  The base graph is not modified; the training engine is left alone as by ``infer``.  Synchronises once (the
        status word).  Out of scope: train-mode / minority lists (a query's logits are test-mode by definition)."""
        return self._explain_new("chosen_new", query, ids, chunk, (0.0, 1.0), False, True, reuse_scores, _list_capacity)[1]

    def attribute_new(self, query: QueryBatch, ids=None, chunk: Optional[int] = None, target=(0.0, 1.0), neighbours: bool = False,
                      reuse_scores: bool = True, _list_capacity: Optional[int] = None) -> Attribution:
        """``attribute`` for nodes that are NOT in the graph: the exact split of ``target[0] * logit0 + target[1] * logit1`` of
        every requested row of ``query`` into the shares of the row's own features, of every relation and - neighbours=True -
        of every chosen neighbour (pcg_explain_new).  The result's logits are ``infer_new(query, ids)`` bit for bit; it is
        built over the query's feature table and the query-local ids, so ``feature_contrib`` and ``completeness_residual``
        work as for resident nodes.  neighbours=True adds ``chosen`` (what ``chosen_new`` returns: global ids) and
        ``neigh_contrib`` from the SAME call and the same single selection per chunk - no second plan / select, no second
        score pass.  Every value is bit for bit what ``attribute(N + ids, neighbours=True)`` returns on a graph built with
        the query rows appended.  ids, chunk, reuse_scores and the cached base scores: ``infer_new``'s; target: two finite
        floats, else ValueError.  The base graph is not modified; the training engine is left alone as by ``infer``.
        Synchronises once (the status word).  Out of scope: ``DistributedPCGNN``, the train-mode selection, GraphSAGE / GCN."""
        return self._explain_new("attribute_new", query, ids, chunk, target, True, bool(neighbours), reuse_scores, _list_capacity)[0]
