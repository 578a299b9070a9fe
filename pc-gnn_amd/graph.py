"""Device-resident graph container: multi-relation CSR + frozen feature table.

Input contract = what the reference hands its layers:
``adj_lists``: list of ``dict[int -> set[int]]`` per relation, symmetric, with
self-loops (src/utils.py:226-239); ``features``: frozen ``nn.Embedding`` weight
``[N, F]`` (src/model_handler.py:85-87); ``train_pos``: list of ids.

Layout in HBM (see include/pcgnn.h): X ``[N, Fs]`` f32 with ``Fs = ceil4(F)``
zero-padded so every row is a whole number of 16-byte chunks (128-B rows for
YelpChi F=32 and for Amazon F=25), per relation ``indptr`` int64 ``[N+1]`` and
``indices`` int32 ascending inside a row, ``train_pos`` int32.
"""
import ctypes as C
from typing import Dict, List, Optional, Sequence, Set, Tuple

import numpy as np
import torch

from . import _lib

AdjList = Dict[int, Set[int]]


def adj_to_csr(adj: AdjList, n_nodes: int) -> Tuple[np.ndarray, np.ndarray]:
    """dict-of-sets -> (indptr int64 [N+1], indices int32, ascending per row)."""
    deg = np.zeros(n_nodes, dtype=np.int64)
    for v, s in adj.items():
        deg[int(v)] = len(s)
    indptr = np.zeros(n_nodes + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = np.empty(int(indptr[-1]), dtype=np.int32)
    for v, s in adj.items():
        if s:
            v = int(v)
            row = np.fromiter(s, dtype=np.int32, count=len(s))
            row.sort()
            indices[indptr[v]:indptr[v + 1]] = row
    return indptr, indices


def csr_from_pairs_device(n_nodes: int, src: torch.Tensor, dst: torch.Tensor, symmetrise: bool = True,
                          self_loops: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """CSR of an edge list, built ON THE DEVICE: what ``sparse_to_adjlist_for_train`` builds on the host with Python sets
    (src/utils.py:243-254: both directions, one self-loop per node, duplicates dropped) as one sort + unique of 64-bit
    (row, column) keys.  src / dst: integer device tensors of equal length.  Returns (indptr int64 [N + 1], indices int32
    ascending inside a row), both on the device of `src`."""
    dev = src.device
    a, b = src.to(torch.int64), dst.to(torch.int64)
    if a.numel() and (int(torch.min(torch.minimum(a, b))) < 0 or int(torch.max(torch.maximum(a, b))) >= n_nodes):
        raise ValueError("edge endpoint out of range")
    rows, cols = [a], [b]
    if symmetrise:
        rows.append(b)
        cols.append(a)
    if self_loops:
        loop = torch.arange(n_nodes, dtype=torch.int64, device=dev)
        rows.append(loop)
        cols.append(loop)
    key = torch.unique(torch.cat(rows) * n_nodes + torch.cat(cols))          # sorted: by row, then by column
    r = torch.div(key, n_nodes, rounding_mode="floor")
    indptr = torch.zeros(n_nodes + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.bincount(r, minlength=n_nodes), 0)
    return indptr, (key - r * n_nodes).to(torch.int32)


def adj_to_pairs(adj: AdjList) -> Tuple[np.ndarray, np.ndarray]:
    """dict-of-sets -> (src, dst) int64 arrays (one pass over the dict; the sort / de-duplication happens on the device)."""
    n_entries = sum(len(s) for s in adj.values())
    src = np.empty(n_entries, dtype=np.int64)
    dst = np.empty(n_entries, dtype=np.int64)
    at = 0
    for v, s in adj.items():
        k = len(s)
        if k:
            src[at:at + k] = int(v)
            dst[at:at + k] = np.fromiter(s, dtype=np.int64, count=k)
            at += k
    return src, dst


class DeviceGraph:
    def __init__(self, X, csr: Sequence[Tuple[np.ndarray, np.ndarray]], train_pos: Sequence[int],
                 device: Optional[torch.device] = None, id_space: Optional[int] = None):
        """id_space: size of the id space neighbour / train_pos ids live in when it is not this
        table's own row count (a shard of a partitioned graph keeps GLOBAL ids, see dist.py)."""
        _lib.load()
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.PcgnnLibraryError("DeviceGraph needs a GPU device: the PC-GNN hot path has no CPU fallback")
        X = torch.as_tensor(X, dtype=torch.float32)
        self.n_nodes, self.feat_dim = int(X.shape[0]), int(X.shape[1])
        self.id_space = int(id_space or X.shape[0])
        self.feat_stride = (self.feat_dim + 3) // 4 * 4
        if self.feat_stride > 512:
            raise _lib.PcgnnLibraryError(f"feat_dim {self.feat_dim} > 512 is not supported by the gather kernels")
        Xp = torch.zeros(self.n_nodes, self.feat_stride, dtype=torch.float32, device=self.device)
        Xp[:, :self.feat_dim] = X.to(self.device)
        self.X = Xp
        self.R = len(csr)
        if not 1 <= self.R <= _lib.PCG_MAX_REL:
            raise ValueError(f"1..{_lib.PCG_MAX_REL} relations supported, got {self.R}")
        self.indptr, self.indices, self.deg_host = [], [], []
        self.max_degree = 0
        for indptr, indices in csr:
            indptr = np.ascontiguousarray(indptr, dtype=np.int64)
            indices = np.ascontiguousarray(indices, dtype=np.int32)
            if indptr.shape[0] != self.n_nodes + 1 or indptr[-1] != indices.shape[0]:
                raise ValueError("CSR shape does not match the feature table")
            if indices.size and (indices.min() < 0 or indices.max() >= (id_space or self.n_nodes)):
                raise ValueError("neighbour id out of range")
            deg = np.diff(indptr)
            self.deg_host.append(deg)
            self.max_degree = max(self.max_degree, int(deg.max()) if deg.size else 0)
            self.indptr.append(torch.from_numpy(indptr).to(self.device))
            self.indices.append(torch.from_numpy(indices).to(self.device) if indices.size
                                else torch.zeros(1, dtype=torch.int32, device=self.device))
        tp = np.asarray(list(train_pos), dtype=np.int64)
        if tp.size and (tp.min() < 0 or tp.max() >= (id_space or self.n_nodes)):
            raise ValueError("train_pos id out of range")
        if np.unique(tp).size != tp.size:
            raise ValueError("train_pos contains duplicate ids (the reference builds it with pos_neg_split, "
                             "src/utils.py:256-271, which never does)")
        self.n_pos = int(tp.size)
        self.train_pos_host = tp
        self.train_pos = (torch.from_numpy(tp.astype(np.int32)).to(self.device) if tp.size
                          else torch.zeros(1, dtype=torch.int32, device=self.device))
        self._desc = None

    # -- constructors ---------------------------------------------------------
    @classmethod
    def from_adj_lists(cls, features_weight, adj_lists: Sequence[AdjList], train_pos, device=None, build_on_device: bool = True):
        """From the reference's input format (list of dict[int -> set[int]] incl. self-loops, src/utils.py:226-239).  The
        dicts are flattened in one host pass; sorting / de-duplicating the rows happens on the device
        (``csr_from_pairs_device``) unless ``build_on_device=False`` (per-row host sort, ``adj_to_csr``)."""
        n = int(features_weight.shape[0])
        X = features_weight.detach().cpu() if torch.is_tensor(features_weight) else features_weight
        if not build_on_device:
            return cls(X, [adj_to_csr(a, n) for a in adj_lists], train_pos, device)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise _lib.PcgnnLibraryError("DeviceGraph needs a GPU device: the PC-GNN hot path has no CPU fallback")
        csr = []
        for a in adj_lists:
            src, dst = adj_to_pairs(a)
            ip, ix = csr_from_pairs_device(n, torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev),
                                           symmetrise=False, self_loops=False)       # the reference's dicts are complete already
            csr.append((ip.cpu().numpy(), ix.cpu().numpy()))
        return cls(X, csr, train_pos, dev)

    @classmethod
    def from_scipy(cls, features_weight, matrices, train_pos, device=None):
        """From scipy sparse adjacency matrices (what data_process.py reads from the .mat files): symmetrised, self-loops
        added, duplicates dropped on the device (src/utils.py:243-254 semantics)."""
        import scipy.sparse as sp
        n = int(features_weight.shape[0])
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        csr = []
        for m in matrices:
            coo = sp.coo_matrix(m)
            ip, ix = csr_from_pairs_device(n, torch.from_numpy(coo.row.astype(np.int64)).to(dev),
                                           torch.from_numpy(coo.col.astype(np.int64)).to(dev))
            csr.append((ip.cpu().numpy(), ix.cpu().numpy()))
        X = features_weight.detach().cpu() if torch.is_tensor(features_weight) else features_weight
        return cls(X, csr, train_pos, dev)

    # -- C ABI view -------------------------------------------------------------
    @property
    def desc(self) -> _lib.GraphDesc:
        if self._desc is None:
            d = _lib.GraphDesc()
            d.n_nodes, d.feat_dim, d.feat_stride = self.n_nodes, self.feat_dim, self.feat_stride
            d.n_rel, d.n_pos, d.max_degree = self.R, self.n_pos, self.max_degree
            d.X = self.X.data_ptr()
            d.train_pos = self.train_pos.data_ptr()
            for r in range(self.R):
                d.indptr[r] = self.indptr[r].data_ptr()
                d.indices[r] = self.indices[r].data_ptr()
            self._desc = d
        return self._desc

    def desc_ref(self):
        return C.byref(self.desc)

    def nbytes(self) -> int:
        return (self.X.numel() * 4 + sum(t.numel() * 8 for t in self.indptr) + sum(t.numel() * 4 for t in self.indices)
                + self.train_pos.numel() * 4)


class ChosenLists:
    """The neighbours a test-mode selection kept, in the reference's order, with their distances - device tensors
    (``FusedPCGNN.chosen``, ``ops.choose_ranked``; the kernel: pcg_rank_lists).  Row (r, i) - relation r, the i-th requested
    node - is ``ids[offsets[r, i]:offsets[r, i + 1]]`` / ``dist[...]``: ascending distance, ties by position in the ascending-id
    neighbour row, where the reference ranks (deg > k + 1); the ascending-id row itself where it keeps every neighbour
    (choose_step_test, src/layers.py:713-736).  ``dist`` is ``torch.abs(centre score - neighbour score)`` bit for bit.

    offsets int64 [R, n + 1] (a view of the flat [R * n + 1] array: offsets[r, n] == offsets[r + 1, 0]) | ids int32 [total] |
    dist float32 [total].

    A train-mode result (``chosen(train_flag=True)``, ``choose_ranked(labels=...)``; the kernel: pcg_rank_minority) carries the
    MINORITY part beside it, in the same layout - ``minor_offsets`` [R, n + 1] (a view of ``minor_flat_offsets``), ``minor_ids``,
    ``minor_dist``; ``has_minority`` says so: per row of a positive centre the m = min(int(k * rho), n_pos) training positives
    nearest to its score, ascending distance, ties by position in train_pos (choose_step_neighs, src/layers.py:675-691); a pick
    that is also a kept neighbour is listed in both parts, as the reference's samp_score_diff lists it.  ``row`` and the fields
    above are the neighbour part in either case: it is the same in both modes."""

    def __init__(self, flat_offsets: torch.Tensor, ids: torch.Tensor, dist: torch.Tensor, R: int, n: int,
                 host_offsets: Optional[np.ndarray] = None, minor_flat_offsets: Optional[torch.Tensor] = None,
                 minor_ids: Optional[torch.Tensor] = None, minor_dist: Optional[torch.Tensor] = None,
                 minor_host_offsets: Optional[np.ndarray] = None):
        self.R, self.n = int(R), int(n)
        self.flat_offsets = flat_offsets
        self.offsets = flat_offsets.as_strided((self.R, self.n + 1), (self.n, 1))
        self.ids, self.dist = ids, dist
        self._host = host_offsets
        self.has_minority = minor_flat_offsets is not None
        self.minor_flat_offsets, self.minor_ids, self.minor_dist = minor_flat_offsets, minor_ids, minor_dist
        self.minor_offsets = minor_flat_offsets.as_strided((self.R, self.n + 1), (self.n, 1)) if self.has_minority else None
        self._minor_host = minor_host_offsets

    def __iter__(self):
        return iter((self.offsets, self.ids, self.dist))

    def host_offsets(self) -> np.ndarray:
        """The flat offsets [R * n + 1] on the host (formed there: no copy unless the object was built from device data)."""
        if self._host is None:
            self._host = self.flat_offsets.cpu().numpy()
        return self._host

    def minor_host_offsets(self) -> np.ndarray:
        """The minority part's flat offsets [R * n + 1] on the host."""
        if not self.has_minority:
            raise ValueError("this ChosenLists has no minority part (a test-mode result)")
        if self._minor_host is None:
            self._minor_host = self.minor_flat_offsets.cpu().numpy()
        return self._minor_host

    def row(self, r: int, i: int):
        """(ids, dist) of relation r, requested node i: views."""
        h = self.host_offsets()
        lo, hi = int(h[r * self.n + i]), int(h[r * self.n + i + 1])
        return self.ids[lo:hi], self.dist[lo:hi]

    def minor_row(self, r: int, i: int):
        """(ids, dist) of the minority picks of relation r, requested node i: views (empty for a negative centre)."""
        h = self.minor_host_offsets()
        lo, hi = int(h[r * self.n + i]), int(h[r * self.n + i + 1])
        return self.minor_ids[lo:hi], self.minor_dist[lo:hi]

    def mean_dist(self, include_minority: bool = False) -> torch.Tensor:
        """The average neighbour distance of every row, [R, n] (the paper's per-relation diagnostic); NaN for an empty row.
        include_minority: over the neighbour and the minority entries together (the mean of the reference's train-mode row)."""
        rows = self.R * self.n
        dev = self.dist.device
        cnt = (self.flat_offsets[1:] - self.flat_offsets[:-1])
        seg = torch.repeat_interleave(torch.arange(rows, device=dev), cnt)
        tot = torch.zeros(rows, dtype=torch.float64, device=dev).index_add_(0, seg, self.dist.double())
        if include_minority and self.has_minority:
            mcnt = (self.minor_flat_offsets[1:] - self.minor_flat_offsets[:-1])
            seg = torch.repeat_interleave(torch.arange(rows, device=dev), mcnt)
            tot.index_add_(0, seg, self.minor_dist.double())
            cnt = cnt + mcnt
        return (tot / cnt.double()).float().view(self.R, self.n)

    def to_reference(self, r: int):
        """Relation r in the reference's return shape: (samp_neighs list[set[int]], samp_scores list[list[float]]).  With a
        minority part it is the train-mode shape: the set union of neighbour and minority ids, and the neighbour distances
        followed by the minority distances (src/layers.py:690-695)."""
        h = self.host_offsets()
        lo, hi = int(h[r * self.n]), int(h[(r + 1) * self.n])
        ids = self.ids[lo:hi].cpu().numpy()
        dist = self.dist[lo:hi].cpu().numpy()
        cut = (h[r * self.n:(r + 1) * self.n + 1] - lo).tolist()
        sets = [set(ids[a:b].tolist()) for a, b in zip(cut[:-1], cut[1:])]
        scores = [dist[a:b].tolist() for a, b in zip(cut[:-1], cut[1:])]
        if self.has_minority:
            h = self.minor_host_offsets()
            lo, hi = int(h[r * self.n]), int(h[(r + 1) * self.n])
            ids = self.minor_ids[lo:hi].cpu().numpy()
            dist = self.minor_dist[lo:hi].cpu().numpy()
            cut = (h[r * self.n:(r + 1) * self.n + 1] - lo).tolist()
            for i, (a, b) in enumerate(zip(cut[:-1], cut[1:])):
                sets[i].update(ids[a:b].tolist())
                scores[i].extend(dist[a:b].tolist())
        return sets, scores


class Attribution:
    """Exact input attributions of ``target[0] * logit0 + target[1] * logit1`` for n requested nodes (``FusedPCGNN.attribute``;
    the kernels: pcg_attr_set, pcg_attr_neighbours) - device tensors.  The gnn path has no bias, so with the selection held fixed
    the attributed scalar is positively homogeneous of degree 1 in the node's own row x and the means a_r of its chosen rows,
    and gradient times input splits it completely:  target . logits[i] = self_contrib[i] + sum_r rel_contrib[r, i].

    logits [n, 2] (``infer``'s, bit for bit) | d_self [n, F] = d target / d x | d_agg [R, n, F] = d target / d a_r |
    self_contrib [n] = <x, d_self> | rel_contrib [R, n] = <a_r, d_agg_r> | target (w0, w1).
    With neighbours: ``chosen`` - the ``ChosenLists`` of the same ids - and neigh_contrib float32 [total], entry for entry beside
    ``chosen.ids``: <X[id], d_agg[r, i]> / row length; a row's entries sum to rel_contrib[r, i].
    A node with an empty neighbour set (a 0 / 0 aggregate) has the logits ``infer`` gives it; its attributions are unspecified."""

    def __init__(self, ids: torch.Tensor, X: torch.Tensor, feat_dim: int, logits, d_self, d_agg, self_contrib, rel_contrib, target,
                 chosen: Optional[ChosenLists] = None, neigh_contrib: Optional[torch.Tensor] = None):
        self.ids, self._X, self._F = ids, X, int(feat_dim)
        self.logits, self.d_self, self.d_agg = logits, d_self, d_agg
        self.self_contrib, self.rel_contrib = self_contrib, rel_contrib
        self.target = (float(target[0]), float(target[1]))
        self.chosen, self.neigh_contrib = chosen, neigh_contrib

    def target_logit(self) -> torch.Tensor:
        """The attributed scalar of every node, [n]."""
        return self.target[0] * self.logits[:, 0] + self.target[1] * self.logits[:, 1]

    def feature_contrib(self) -> torch.Tensor:
        """``X[ids] * d_self`` [n, F]: the share of each of the node's own features (its rows sum to self_contrib)."""
        return self._X[self.ids.long(), :self._F] * self.d_self

    def completeness_residual(self) -> torch.Tensor:
        """self_contrib + rel_contrib.sum(0) - target . logits, [n]: rounding error only."""
        return self.self_contrib + self.rel_contrib.sum(0) - self.target_logit()

    def top_neighbours(self, r: int, i: int, k: Optional[int] = None):
        """(ids, contributions) of relation r, requested node i, by descending absolute contribution (the first k; None: all)."""
        if self.chosen is None:
            raise ValueError("this Attribution has no neighbour part (attribute(neighbours=True))")
        h = self.chosen.host_offsets()
        lo, hi = int(h[r * self.chosen.n + i]), int(h[r * self.chosen.n + i + 1])
        c = self.neigh_contrib[lo:hi]
        order = torch.argsort(c.abs(), descending=True, stable=True)
        if k is not None:
            order = order[:int(k)]
        return self.chosen.ids[lo:hi][order], c[order]


class NearestExamples:
    """The k labelled examples each of n requested nodes looks most like (``FusedPCGNN.nearest``; the kernel:
    pcg_topk_similar) - device tensors, a row per requested node, sorted by score descending with ties by lower position:

    ids [n, k] int32: global node ids of the examples, -1 where a node has fewer than k eligible examples |
    pos [n, k] int32: their positions in ``among`` (-1 likewise) | score [n, k] float32 (-inf likewise) |
    among: the searched node ids [M] | metric: "cosine", "dot" or "l2" (always maximised: l2 is minus the squared distance)."""

    def __init__(self, ids: torch.Tensor, pos: torch.Tensor, score: torch.Tensor, among: torch.Tensor, metric: str):
        self.ids, self.pos, self.score, self.among, self.metric = ids, pos, score, among, metric
        self.n, self.k = int(pos.shape[0]), int(pos.shape[1])

    def row(self, i: int):
        """(ids, pos, score) of requested node i, without its padding."""
        keep = self.pos[i] >= 0
        return self.ids[i][keep], self.pos[i][keep], self.score[i][keep]

    def to_numpy(self):
        """(ids, pos, score) as host arrays [n, k]."""
        return self.ids.cpu().numpy(), self.pos.cpu().numpy(), self.score.cpu().numpy()


class AlertList:
    """The k highest-scoring rows of a requested set, in alert order (``FusedPCGNN.alerts``; the kernel: pcg_topk_alerts) -
    device tensors.  The alert order is the stable sort by positive-class probability, descending: among equal probabilities
    the lower position in the requested set comes first, so a tie at the cut k is resolved by input position and the list is
    the same on every run.

    ids [k] int32: node ids (query-local for a query batch) | pos [k] int32: positions in the requested set | prob [k]
    float32: the positive-class probability; slots beyond the set's size hold -1 / -1 / -inf | hits [k] int64 (only with
    labels): positives among the alerts up to and including each slot | n: rows that were ranked."""

    def __init__(self, ids: torch.Tensor, pos: torch.Tensor, prob: torch.Tensor, n: int, hits: Optional[torch.Tensor] = None):
        self.ids, self.pos, self.prob, self.hits = ids, pos, prob, hits
        self.n, self.k = int(n), int(pos.shape[0])

    def to_numpy(self):
        """(ids, pos, prob) - with labels (ids, pos, prob, hits) - as host arrays [k]."""
        out = (self.ids.cpu().numpy(), self.pos.cpu().numpy(), self.prob.cpu().numpy())
        return out if self.hits is None else out + (self.hits.cpu().numpy(),)


class CaseList:
    """Alerts grouped into cases (``FusedPCGNN.cases``, ``ops.group_members``; the kernel: pcg_alert_cases).  A slot is a position
    of the member list, which is in alert order.  Slot p is linked to slot q when both name the same node or when, in a selected
    relation, either node occurs in the other's CSR row (an edge stored one way links; a shared neighbour that is no member
    does not: there is no 2-hop linking).  A case is a connected component of the non-padding slots; its head is its lowest
    slot - its highest-ranked alert - and cases are numbered by ascending head, so case 0 holds alert 0.  Every value is a
    function of the inputs alone: the same bits on every run.

    case_of [m] int32: the slot's case, -1 for padding | head [C] int32 | offsets [C + 1] int32 and order [m_valid] int32: case
    c's slots, ascending, are order[offsets[c] : offsets[c + 1]] | links [C] int32: the CSR entries of the case's members, over
    the selected relations, whose target is another member node (directed: a symmetric edge counts twice; self-loops count
    zero) | hits [C] int32 or None: the case's slots with label 1 | n_cases: C | members [m] int32: the grouped ids |
    alerts: the ``AlertList`` the members are the ids of, or None.  Device tensors (the methods work on CPU tensors too)."""

    def __init__(self, case_of: torch.Tensor, head: torch.Tensor, offsets: torch.Tensor, order: torch.Tensor, links: torch.Tensor,
                 hits: Optional[torch.Tensor], n_cases: int, members: torch.Tensor, alerts: Optional["AlertList"] = None):
        self.case_of, self.head, self.offsets, self.order, self.links, self.hits = case_of, head, offsets, order, links, hits
        self.n_cases, self.members, self.alerts = int(n_cases), members, alerts

    def size(self) -> torch.Tensor:
        """[C] int32: the slots of each case."""
        return self.offsets[1:] - self.offsets[:-1]

    def case(self, c: int):
        """The slots of case c, ascending - with an alert list attached (slots, ids, prob)."""
        if not 0 <= c < self.n_cases:
            raise IndexError(f"case {c} of {self.n_cases}")
        lo, hi = (int(v) for v in self.offsets[c:c + 2].tolist())
        slots = self.order[lo:hi]
        if self.alerts is None:
            return slots
        at = slots.long()
        return slots, self.alerts.ids[at], self.alerts.prob[at]

    def expected_hits(self) -> torch.Tensor:
        """float64 [C]: the sum of the members' positive-class probabilities per case (needs the alert list).  A segmented
        reduction over ``order`` (torch.segment_reduce: every case is summed on its own, in slot order) - no atomics, no
        ``index_add_``, the same bits on every run."""
        if self.alerts is None:
            raise ValueError("expected_hits: this CaseList was made from bare members, without an alert list's probabilities")
        p = self.alerts.prob[self.order.long()].double()
        if self.n_cases == 0:
            return p[:0]
        return torch.segment_reduce(p, "sum", lengths=self.size().long(), unsafe=True)

    def to_numpy(self):
        """(case_of, head, offsets, order, links) - with labels (..., hits) - as host arrays."""
        out = tuple(t.cpu().numpy() for t in (self.case_of, self.head, self.offsets, self.order, self.links))
        return out if self.hits is None else out + (self.hits.cpu().numpy(),)


class BaseShape:
    """What a ``QueryBatch`` is validated against: the base graph's node count, feature width and relation count.  A
    ``DeviceGraph`` has the same three attributes; this stands in for one where there is no GPU (host-side checks, tests)."""

    def __init__(self, n_nodes: int, feat_dim: int, n_rel: int):
        self.n_nodes, self.feat_dim, self.R = int(n_nodes), int(feat_dim), int(n_rel)


class QueryBatch:
    """nq NEW nodes to be scored against a resident base graph of N nodes (``FusedPCGNN.infer_new``, pcg_infer_new): a feature
    row each and, per relation, a neighbour list of GLOBAL ids in [0, N + nq) - query node j has the global id N + j; its
    neighbours may be base nodes, other nodes of the batch and the node itself (the reference keeps self-loops,
    src/utils.py:226-239: a caller mirroring it puts N + j into row j).  The base graph is not modified and nothing of it is
    recomputed; the batch is not appended to it.

    Everything here happens in numpy ON THE HOST: rows are sorted ascending and de-duplicated, the per-relation degrees and
    ``max_degree`` computed, and the input validated - ``ValueError`` naming the relation and the row: feature width and
    relation count against the base graph, every neighbour id in [0, N + nq), ``indptr`` monotone, nq / N + nq / list sizes
    within int32.  ``to(device, base_graph)`` uploads (features padded to the base graph's ``feat_stride``).

    ``base``: the base ``DeviceGraph``, or a ``BaseShape(n_nodes, feat_dim, n_rel)``.  ``csr``: one raw ``(indptr [nq + 1],
    indices)`` pair per relation (rows in any order, duplicates allowed)."""

    def __init__(self, features, csr: Sequence[Tuple[np.ndarray, np.ndarray]], base):
        N, F, R = int(base.n_nodes), int(base.feat_dim), int(base.R)
        X = features.detach().cpu().numpy() if torch.is_tensor(features) else np.asarray(features)
        if X.ndim != 2:
            raise ValueError(f"query features must be [nq, {F}], got shape {tuple(X.shape)}")
        nq = int(X.shape[0])
        if X.shape[1] != F:
            raise ValueError(f"query feature width {X.shape[1]} != the base graph's {F}")
        if len(csr) != R:
            raise ValueError(f"query batch has {len(csr)} relations, the base graph {R}")
        if nq >= (1 << 31) or N + nq >= (1 << 31):
            raise ValueError(f"nq {nq} + {N} base nodes does not fit int32 ids")
        self.n_base, self.nq, self.feat_dim, self.R = N, nq, F, R
        self.X_host = np.ascontiguousarray(X, dtype=np.float32)
        self.csr: List[Tuple[np.ndarray, np.ndarray]] = []
        self.deg_host: List[np.ndarray] = []
        self.max_degree = 0
        span = N + nq
        for r, (indptr, indices) in enumerate(csr):
            indptr = np.asarray(indptr).astype(np.int64).reshape(-1)
            indices = np.asarray(indices).astype(np.int64).reshape(-1)
            if indptr.shape[0] != nq + 1:
                raise ValueError(f"relation {r}: indptr has {indptr.shape[0]} entries for {nq} query rows (want nq + 1)")
            if indptr[0] != 0:
                raise ValueError(f"relation {r}, row 0: indptr does not start at 0")
            deg = np.diff(indptr)
            if deg.size and deg.min() < 0:
                raise ValueError(f"relation {r}, row {int(np.argmax(deg < 0))}: indptr is not monotone")
            if indptr[-1] != indices.shape[0]:
                raise ValueError(f"relation {r}, row {nq - 1}: indptr ends at {int(indptr[-1])}, the list has {indices.shape[0]} entries")
            if indices.shape[0] >= (1 << 31):
                raise ValueError(f"relation {r}: {indices.shape[0]} list entries do not fit int32")
            rows = np.repeat(np.arange(nq, dtype=np.int64), deg)
            bad = (indices < 0) | (indices >= span)
            if bad.any():
                at = int(np.argmax(bad))
                raise ValueError(f"relation {r}, row {int(rows[at])}: neighbour id {int(indices[at])} outside [0, {span}) "
                                 f"({N} base nodes + {nq} query nodes)")
            key = np.unique(rows * span + indices)              # sorted by row, then by id; duplicates dropped
            krow = key // span if key.size else key
            ip = np.zeros(nq + 1, dtype=np.int64)
            np.cumsum(np.bincount(krow, minlength=nq), out=ip[1:])
            ix = (key - krow * span).astype(np.int32)
            d = np.diff(ip)
            self.csr.append((ip, ix))
            self.deg_host.append(d)
            self.max_degree = max(self.max_degree, int(d.max()) if d.size else 0)
        self.device = None
        self.X = None
        self.indptr, self.indices = [], []
        self.feat_stride = 0
        self._desc = None

    # -- constructors ---------------------------------------------------------
    @classmethod
    def from_adj_lists(cls, features, adj_lists: Sequence[AdjList], base, keys: str = "auto"):
        """From the reference's form: ``features [nq, F]`` and, per relation, ``{node: set(global ids)}``; rows without a key
        are empty.  keys="index": the dict keys are query indices in [0, nq); keys="global": global ids in [N, N + nq).
        keys="auto" decides per dict - all keys >= N: global ids, else query indices - and raises where the two readings
        cannot be told apart (a batch larger than the base graph, N < nq, with a key in [N, nq)): say which one is meant."""
        if keys not in ("auto", "index", "global"):
            raise ValueError(f"keys must be 'auto', 'index' or 'global', got {keys!r}")
        N = int(base.n_nodes)
        nq = int(features.shape[0])
        csr = []
        for r, adj in enumerate(adj_lists):
            kk = np.fromiter((int(k) for k in adj.keys()), dtype=np.int64, count=len(adj))
            if keys == "auto":
                amb = (kk >= N) & (kk < nq)
                if amb.any():
                    raise ValueError(f"relation {r}, row {int(kk[int(np.argmax(amb))])}: the key is both a query index in [0, {nq}) "
                                     f"and a global id in [{N}, {N + nq}) - pass keys='index' or keys='global'")
                off = N if kk.size and kk.min() >= N else 0
            else:
                off = N if keys == "global" else 0
            bad = (kk - off < 0) | (kk - off >= nq)
            if bad.any():
                k = int(kk[int(np.argmax(bad))])
                raise ValueError(f"relation {r}, row {k}: not a query node - neither a query index in [0, {nq}) nor a "
                                 f"global id in [{N}, {N + nq}), or the dict mixes the two")
            deg = np.zeros(nq, dtype=np.int64)
            for k, s in adj.items():
                deg[int(k) - off] = len(s)
            indptr = np.zeros(nq + 1, dtype=np.int64)
            np.cumsum(deg, out=indptr[1:])
            indices = np.empty(int(indptr[-1]), dtype=np.int64)
            for k, s in adj.items():
                if s:
                    j = int(k) - off
                    indices[indptr[j]:indptr[j + 1]] = np.fromiter(s, dtype=np.int64, count=len(s))
            csr.append((indptr, indices))
        return cls(features, csr, base)

    @classmethod
    def from_scipy(cls, features, matrices, base):
        """From scipy sparse matrices of shape [nq, N + nq] (row j: the neighbours of query node j; every stored entry is an
        edge).  Nothing is symmetrised and no self-loop is added: the lists are the caller's."""
        import scipy.sparse as sp
        N = int(base.n_nodes)
        nq = int(features.shape[0])
        csr = []
        for r, m in enumerate(matrices):
            if tuple(m.shape) != (nq, N + nq):
                raise ValueError(f"relation {r}: matrix shape {tuple(m.shape)} != ({nq}, {N + nq}) = (nq, N + nq)")
            c = sp.csr_matrix(m)
            csr.append((c.indptr.astype(np.int64), c.indices.astype(np.int64)))
        return cls(features, csr, base)

    # -- device side ------------------------------------------------------------
    def to(self, device, base_graph: "DeviceGraph"):
        """Upload for ``base_graph`` (the features padded to its ``feat_stride``); returns self."""
        g = base_graph
        if (g.n_nodes, g.feat_dim, g.R) != (self.n_base, self.feat_dim, self.R):
            raise ValueError(f"query batch built for a base graph of {self.n_base} nodes / {self.feat_dim} features / {self.R} "
                             f"relations, not {g.n_nodes} / {g.feat_dim} / {g.R}")
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.PcgnnLibraryError("QueryBatch.to needs a GPU device: the PC-GNN hot path has no CPU fallback")
        self.device = device
        self.feat_stride = g.feat_stride
        Xp = torch.zeros(max(self.nq, 1), self.feat_stride, dtype=torch.float32, device=device)
        if self.nq:
            Xp[:self.nq, :self.feat_dim] = torch.from_numpy(self.X_host).to(device)
        self.X = Xp
        self.indptr = [torch.from_numpy(ip).to(device) for ip, _ in self.csr]
        self.indices = [torch.from_numpy(ix).to(device) if ix.size else torch.zeros(1, dtype=torch.int32, device=device)
                        for _, ix in self.csr]
        self._desc = None
        return self

    @property
    def desc(self) -> _lib.GraphDesc:
        if self.X is None:
            raise _lib.PcgnnLibraryError("QueryBatch.desc: call to(device, base_graph) first")
        if self._desc is None:
            d = _lib.GraphDesc()
            d.n_nodes, d.feat_dim, d.feat_stride = self.nq, self.feat_dim, self.feat_stride
            d.n_rel, d.n_pos, d.max_degree = self.R, 0, self.max_degree
            d.X = self.X.data_ptr()
            d.train_pos = None
            for r in range(self.R):
                d.indptr[r] = self.indptr[r].data_ptr()
                d.indices[r] = self.indices[r].data_ptr()
            self._desc = d
        return self._desc

    def desc_ref(self):
        return C.byref(self.desc)
