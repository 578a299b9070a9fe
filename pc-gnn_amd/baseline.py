"""The GraphSAGE / GCN baselines (``graphsage.GraphSage`` / ``graphsage.GCN``) on the device: ``BaselineEngine``.

Whole-set inference - one call over any node set (or the whole graph) instead of the per-batch ``to_prob`` loop: pcg_baseline_infer
(csrc/baseline.hip) reads every centre's CSR row in place - no plan, no selection, no per-edge list - and runs the encoder and
the head on exact float32 MFMA tiles.  ``infer`` returns the logits, ``embed`` the encoder's output (and the aggregates);
``evaluate``, ``evaluate_ranking`` and ``alerts`` are ``wholeset.EvalCalls``', the methods a FusedPCGNN has.

Training - pcg_baseline_train (csrc/baseline_train.hip): the same aggregation and forward tile, the two-class cross entropy, the
backward to ``enc.weight`` / ``weight`` as MFMA GEMMs over the batch and torch.optim.Adam's update, per batch in three launches
with no host synchronisation.  ``train_step`` / ``train_epoch`` run the engine's own Adam (``configure_optimizer``) in place on the
live parameters; ``loss_and_grad`` / ``backward`` stop at the gradients, so that any ``torch.optim`` optimizer or clipping can
follow.  Nothing here reads the device: ``check()`` reads the status word once and raises on a bad id or label.

The engine holds no copy of the parameters: every call passes the live ``enc.weight`` / ``model.weight``, so a step between two
calls - the engine's or an optimizer's - is seen.
Out of scope: the random fan-out, query batches, ``nearest``, attribution, custom losses, gradients to the feature table.
"""
import ctypes as C
from typing import Optional

import numpy as np
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
    ``evaluate_ranking`` and ``alerts`` (resident ids only), and its training calls: ``train_step``, ``train_epoch``,
    ``loss_and_grad``, ``backward``.  Build it with ``from_model``."""

    def __init__(self, model, graph, workspace_bytes: int = 1 << 30):
        self.model = model
        self.shape = model_shape(model)
        self.g = graph
        self.dev = graph.device
        _lib.load()
        self.E = self.shape["emb"]
        self.workspace_bytes = int(workspace_bytes)          # the default chunk keeps the workspace within this
        self._inf = {}                                       # status, ws, train_ws, all_ids, eval_labels: grown on demand
        self._hyper = None                                   # configure_optimizer
        self._opt = None                                     # the engine's Adam state, made by the first train_step
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
        self.check()

    def check(self):
        """Reads the status word once (synchronises) and raises if a call since the last look met an id outside the feature
        table - in ids or in the graph's rows - or, training, a label outside {0, 1}.  The word is cleared for the next call."""
        status = self._inf.get("status")
        st = 0 if status is None else int(status.item())
        if st:
            status.zero_()
            what = [msg for bit, msg in ((_lib.PCG_ST_LIST_ID_RANGE, "an id outside the feature table (in ids or in the graph's rows)"),
                                         (_lib.PCG_ST_EVAL_INPUT, "a label outside {0, 1}")) if st & bit]
            raise _lib.PcgnnLibraryError("; ".join(what) if what else f"device status {st}")

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


    # ---- training (pcg_baseline_train) ----------------------------------------------------------------------------------------
    def configure_optimizer(self, lr: float, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8):
        """The hyper-parameters of the engine's own Adam (torch.optim.Adam's, coupled weight decay), what ``train_step`` /
        ``train_epoch`` apply.  The state (moments, step count) is created on first use and kept across calls of this."""
        self._hyper = _lib.AdamHyper(float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay))

    def _adam(self) -> dict:
        """the engine's Adam state: m / v of both matrices (zeros on first use) and the number of steps taken"""
        if self._hyper is None:
            raise _lib.PcgnnLibraryError("BaselineEngine: configure_optimizer(lr, weight_decay) before the first train_step")
        if self._opt is None:
            w_enc, w_cls = self.model.enc.weight, self.model.weight
            self._opt = dict(step=0, m_enc=torch.zeros_like(w_enc.data), v_enc=torch.zeros_like(w_enc.data),
                             m_cls=torch.zeros_like(w_cls.data), v_cls=torch.zeros_like(w_cls.data))
        return self._opt

    def reset_optimizer(self):
        """zero moments and step count: the next ``train_step`` is step 1 (the hyper-parameters stay)"""
        self._opt = None

    def optimizer_state(self) -> dict:
        """a copy of the engine's Adam state: ``step`` and the tensors ``m_enc``, ``v_enc`` [E, K], ``m_cls``, ``v_cls`` [2, E]"""
        o = self._adam()
        return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in o.items()}

    def load_optimizer_state(self, state: dict):
        """``optimizer_state()``'s dict back in (shapes checked)"""
        o = self._adam()
        for k in ("m_enc", "v_enc", "m_cls", "v_cls"):
            if tuple(state[k].shape) != tuple(o[k].shape):
                raise ValueError(f"load_optimizer_state: {k} {tuple(state[k].shape)}, expected {tuple(o[k].shape)}")
        for k in ("m_enc", "v_enc", "m_cls", "v_cls"):
            o[k].copy_(state[k])
        o["step"] = int(state["step"])

    def _train_args(self, ids, labels, what: str):
        """ids and their labels as int32 device tensors.  Host sequences are range-checked here; device tensors are not read -
        the kernels clamp what they index and report through the status word (``check``)."""
        if torch.is_tensor(ids):
            ids_dev = ops._i32(ids, self.dev).view(-1)
        else:
            host = np.asarray(ids).reshape(-1).astype(np.int64)
            if host.size and (host.min() < 0 or host.max() >= self.g.n_nodes):
                raise ValueError(f"{what}: ids outside 0 .. {self.g.n_nodes - 1}")
            ids_dev = torch.from_numpy(host.astype(np.int32)).to(self.dev)
        if torch.is_tensor(labels):
            lab_dev = ops._i32(labels, self.dev).view(-1)
        else:
            host = np.asarray(labels).reshape(-1).astype(np.int64)
            if host.size and (host.min() < 0 or host.max() > 1):
                raise ValueError(f"{what}: labels outside {{0, 1}}")
            lab_dev = torch.from_numpy(host.astype(np.int32)).to(self.dev)
        if lab_dev.numel() != ids_dev.numel():
            raise ValueError(f"{what}: {lab_dev.numel()} labels for {ids_dev.numel()} ids")
        return ids_dev, lab_dev, int(ids_dev.numel())

    def train_workspace_bytes_of(self, batch_rows: int) -> int:
        m, _ = self._model_desc()
        nbytes = int(_lib.load().pcg_baseline_train_workspace_bytes(self.g.desc_ref(), C.byref(m), int(batch_rows)))
        if nbytes < 0:
            raise _lib.PcgnnLibraryError(f"pcg_baseline_train_workspace_bytes rejected batch {batch_rows} ({nbytes})")
        return nbytes

    def _train_call(self, ids_dev, lab_dev, n: int, batch_rows: int, apply: bool, grad_out):
        """pcg_baseline_train over n > 0 ids -> the batches' losses [ceil(n / batch_rows)]; nothing is read back"""
        inf = self._inf
        nbytes = self.train_workspace_bytes_of(batch_rows)
        if inf.get("train_ws") is None or inf["train_ws"].numel() < nbytes:
            inf["train_ws"] = None
            inf["train_ws"] = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        if inf.get("status") is None:
            inf["status"] = torch.zeros(1, dtype=torch.int32, device=self.dev)
        n_batches = (n + batch_rows - 1) // batch_rows
        losses = torch.empty(n_batches, dtype=torch.float32, device=self.dev)
        m, keep = self._model_desc()
        if apply:
            o = self._adam()
            opt = _lib.BaselineOpt(m_enc=o["m_enc"].data_ptr(), v_enc=o["v_enc"].data_ptr(), m_cls=o["m_cls"].data_ptr(),
                                   v_cls=o["v_cls"].data_ptr(), first_step=o["step"] + 1, apply=1, hyper=self._hyper)
        else:
            opt = _lib.BaselineOpt(apply=0)
        _lib.check(_lib.load().pcg_baseline_train(self.g.desc_ref(), C.byref(m), C.byref(opt), _p(ids_dev), _p(lab_dev), n, batch_rows,
                                               _p(inf["train_ws"]), inf["train_ws"].numel(), _p(losses), _p(grad_out),
                                               _p(inf["status"]), ops._stream(self.dev)), "pcg_baseline_train")
        del keep
        if apply:
            o["step"] += n_batches
        return losses

    def loss_and_grad(self, ids, labels):
        """(loss, d_enc [E, K], d_cls [2, E]) of one batch: ``model.loss(ids, labels)`` and its gradients to ``enc.weight`` /
        ``weight``, device tensors; nothing is updated.  ids, labels: device tensors, numpy arrays or lists (duplicate ids count
        twice)."""
        ids_dev, lab_dev, n = self._train_args(ids, labels, "loss_and_grad")
        if n == 0:
            raise ValueError("loss_and_grad: an empty batch has no mean loss")
        E = self.E
        grad = torch.empty(2 * E + self.model.enc.weight.numel(), dtype=torch.float32, device=self.dev)
        with torch.no_grad():
            loss = self._train_call(ids_dev, lab_dev, n, n, False, grad)[0]
        return loss, grad[2 * E:].view(tuple(self.model.enc.weight.shape)), grad[:2 * E].view(2, E)

    def backward(self, ids, labels, accumulate: bool = False):
        """``loss_and_grad`` with the gradients put into ``enc.weight.grad`` / ``weight.grad`` (added to what is there when
        accumulate) -> the loss: any ``torch.optim`` optimizer, clipping or accumulation can follow."""
        loss, d_enc, d_cls = self.loss_and_grad(ids, labels)
        for p, d in ((self.model.enc.weight, d_enc), (self.model.weight, d_cls)):
            if accumulate and p.grad is not None:
                p.grad.add_(d)
            else:
                p.grad = d.clone()
        return loss

    def train_step(self, ids, labels):
        """One training step on the batch: forward, loss, backward and the engine's own Adam (``configure_optimizer``) on the
        live parameters, in place -> the loss, a device scalar that nothing reads."""
        ids_dev, lab_dev, n = self._train_args(ids, labels, "train_step")
        if n == 0:
            raise ValueError("train_step: an empty batch")
        with torch.no_grad():
            return self._train_call(ids_dev, lab_dev, n, n, True, None)[0]

    def train_epoch(self, ids, labels, batch_size: int):
        """``train_step`` over ids [b0, b0 + batch_size) for b0 = 0, batch_size, ... - the batches in the given order, the last
        one partial - in ONE call -> their losses [n_batches] (device).  Bit for bit the same steps one by one."""
        ids_dev, lab_dev, n = self._train_args(ids, labels, "train_epoch")
        if int(batch_size) < 1:
            raise ValueError(f"train_epoch: batch_size {batch_size}")
        if n == 0:
            return torch.empty(0, dtype=torch.float32, device=self.dev)
        with torch.no_grad():
            return self._train_call(ids_dev, lab_dev, n, min(int(batch_size), n), True, None)
