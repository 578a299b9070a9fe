"""Whole-set inference for the GraphSAGE / GCN baselines (``graphsage.GraphSage`` / ``graphsage.GCN``): ``BaselineEngine``.

One call over any node set (or the whole graph) instead of the per-batch ``to_prob`` loop: pcg_baseline_infer (csrc/baseline.hip)
reads every centre's CSR row in place - no plan, no selection, no per-edge list - and runs the encoder and the head on exact
float32 MFMA tiles.  ``infer`` returns the logits, ``embed`` the encoder's output (and the aggregates); ``evaluate``,
``evaluate_ranking`` and ``alerts`` are ``wholeset.EvalCalls``', the methods a FusedPCGNN has.  The engine holds no copy of the
parameters: every call passes the live ``enc.weight`` / ``model.weight``, so an optimizer step between two calls is seen.
Out of scope: training (torch autograd over the per-batch aggregator), the random fan-out, query batches, ``nearest``, attribution.
"""
import ctypes as C
from typing import Optional

import torch

from . import _lib, ops
from .wholeset import EvalCalls

_p = ops._p


def model_shape(model) -> dict:
    """(add_self, norm, concat_self, emb) of a ``GraphSage`` / ``GCN``, read off its aggregator and encoder classes - the five
    shapes the reference's classes can express (src/graphsage.py:42-150, 181-275)."""
    from . import graphsage as GS
    enc = getattr(model, "enc", None)
    agg = getattr(enc, "aggregator", None)
    if isinstance(enc, GS.GCNEncoder) and isinstance(agg, GS.GCNAggregator):
        concat_self = False
    elif isinstance(enc, GS.Encoder) and isinstance(agg, (GS.MeanAggregator, GS.GCNAggregator)):
        concat_self = not enc.gcn
    else:
        raise TypeError(f"BaselineEngine: {type(model).__name__} is no GraphSage / GCN over an Encoder / GCNEncoder with a "
                        f"MeanAggregator / GCNAggregator")
    return dict(add_self=bool(agg.gcn), norm=int(agg._norm), concat_self=concat_self, emb=int(enc.embed_dim))


class BaselineEngine(EvalCalls):
    """The whole-set calls of a GraphSAGE / GCN baseline: ``infer``, ``embed`` and, through ``wholeset.EvalCalls``, ``evaluate``,
    ``evaluate_ranking`` and ``alerts`` (resident ids only).  Build it with ``from_model``."""

    def __init__(self, model, graph, workspace_bytes: int = 1 << 30):
        self.model = model
        self.shape = model_shape(model)
        self.g = graph
        self.dev = graph.device
        _lib.load()
        self.E = self.shape["emb"]
        self.workspace_bytes = int(workspace_bytes)          # the default chunk keeps the workspace within this
        self._inf = {}                                       # status, ws, all_ids, eval_labels: grown on demand
        K = (2 if self.shape["concat_self"] else 1) * graph.feat_dim
        if tuple(model.enc.weight.shape) != (self.E, K) or tuple(model.weight.shape) != (2, self.E):
            raise ValueError(f"BaselineEngine: encoder weight {tuple(model.enc.weight.shape)} / head weight {tuple(model.weight.shape)}, "
                             f"expected {(self.E, K)} / {(2, self.E)} for a table of {graph.feat_dim} features")

    @classmethod
    def from_model(cls, model, workspace_bytes: int = 1 << 30) -> "BaselineEngine":
        """The engine of a ``GraphSage`` / ``GCN``: add_self, the norm and concat_self read off its aggregator and encoder, on
        the model's own ``DeviceGraph`` (built from its adjacency lists now if no forward has built it yet)."""
        from .graphsage import _graph_of
        model_shape(model)                                   # (TypeError before anything is built)
        agg = model.enc.aggregator
        graph = _graph_of(agg, agg.features, agg.adj_lists, model.weight.device)
        return cls(model, graph, workspace_bytes)

    def flush(self):
        """(nothing is deferred: the parameters are read when a call is enqueued)"""

    def _model_desc(self):
        """pcg_baseline_model over the LIVE parameters (+ the tensors it points into, to be kept until the call is enqueued)"""
        w_enc, w_cls = self.model.enc.weight, self.model.weight
        for name, w in (("enc.weight", w_enc), ("weight", w_cls)):
            if w.dtype != torch.float32 or not w.is_contiguous() or w.device != self.dev:
                raise _lib.PcgnnLibraryError(f"BaselineEngine: {name} must be float32, contiguous and on {self.dev} "
                                             f"(it is {w.dtype}, contiguous={w.is_contiguous()}, on {w.device})")
        s = self.shape
        m = _lib.BaselineModel(rel=0, norm=s["norm"], add_self=int(s["add_self"]), concat_self=int(s["concat_self"]), emb=self.E,
                               W_enc=w_enc.data_ptr(), W_cls=w_cls.data_ptr())
        return m, (w_enc, w_cls)

    def workspace_bytes_of(self, chunk: int) -> int:
        m, _ = self._model_desc()
        nbytes = int(_lib.load().pcg_baseline_workspace_bytes(self.g.desc_ref(), C.byref(m), int(chunk)))
        if nbytes < 0:
            raise _lib.PcgnnLibraryError(f"pcg_baseline_workspace_bytes rejected chunk {chunk} ({nbytes})")
        return nbytes

    def default_chunk(self, n: int, min_chunk: int = 16384) -> int:
        """All n rows in one chunk if its workspace stays within ``workspace_bytes``; else halved until it does, down to
        min_chunk rows (as ``wholeset.default_infer_chunk``)."""
        c = max(int(n), 1)
        while c > min_chunk and self.workspace_bytes_of(c) > self.workspace_bytes:
            c = max(min_chunk, (c + 1) // 2)
        return c

    def _call(self, ids_dev, n: int, chunk: Optional[int], logits, emb, agg):
        """pcg_baseline_infer over n > 0 ids; the status word read once (synchronises)"""
        inf = self._inf
        chunk = self.default_chunk(n) if chunk is None else int(chunk)
        chunk = max(1, min(chunk, n))
        nbytes = self.workspace_bytes_of(chunk)
        if inf.get("ws") is None or inf["ws"].numel() < nbytes:
            inf["ws"] = None
            inf["ws"] = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        if inf.get("status") is None:
            inf["status"] = torch.zeros(1, dtype=torch.int32, device=self.dev)
        m, keep = self._model_desc()
        _lib.check(_lib.load().pcg_baseline_infer(self.g.desc_ref(), C.byref(m), _p(ids_dev), n, chunk, _p(inf["ws"]), inf["ws"].numel(),
                                               _p(logits), _p(emb), _p(agg), _p(inf["status"]), ops._stream(self.dev)),
                   "pcg_baseline_infer")
        del keep
        st = int(inf["status"].item())
        if st:
            inf["status"].zero_()
            raise _lib.PcgnnLibraryError("an id outside the feature table (in ids or in the graph's rows)"
                                         if st & _lib.PCG_ST_LIST_ID_RANGE else f"device status {st}")

    def infer(self, ids=None, chunk: Optional[int] = None) -> torch.Tensor:
        """The logits [n, 2] of a whole node set in one call: ``model.forward`` without the batches.  ids: node ids (any order,
        duplicates allowed; a device tensor, numpy array or list), None = every node.  A node's logits are bit for bit the same
        whatever the set, its order or the chunk.  chunk: ids per chunk (default: all of them, or fewer - never under 16384 - if
        the workspace would exceed ``workspace_bytes``).  Synchronises once (the status word)."""
        _, ids_dev, n = self._resident_ids(ids, "infer")
        logits = torch.empty(n, 2, dtype=torch.float32, device=self.dev)
        if n:
            with torch.no_grad():
                self._call(ids_dev, n, chunk, logits, None, None)
        return logits

    def embed(self, ids=None, chunk: Optional[int] = None, want_logits: bool = False, aggregates: bool = False):
        """The encoder's output h [n, E] of a node set - the TRANSPOSE of what ``Encoder.forward`` returns -, (+ the logits [n, 2],
        bit for bit ``infer``'s, if want_logits) (+ the aggregates a [n, F] if aggregates).  ids, chunk: as ``infer``."""
        _, ids_dev, n = self._resident_ids(ids, "embed")
        f32 = dict(dtype=torch.float32, device=self.dev)
        logits, emb = torch.empty(n, 2, **f32), torch.empty(n, self.E, **f32)
        agg = torch.empty(n, self.g.feat_dim, **f32) if aggregates else None
        if n:
            with torch.no_grad():
                self._call(ids_dev, n, chunk, logits, emb, agg)
        res = (emb,) + ((logits,) if want_logits else ()) + ((agg,) if aggregates else ())
        return res[0] if len(res) == 1 else res

    def alerts(self, ids=None, k: int = 100, chunk: Optional[int] = None, labels=None, query=None):
        """``wholeset.EvalCalls.alerts`` over resident ids; a baseline has no query batches"""
        if query is not None:
            raise ValueError("alerts: query batches are not supported for the GraphSAGE / GCN baselines")
        return super().alerts(ids, k=k, chunk=chunk, labels=labels)
