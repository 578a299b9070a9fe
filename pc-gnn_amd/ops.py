"""torch-tensor level wrappers over the C ABI (include/pcgnn.h).

Every function enqueues HIP kernels on torch's current stream and returns
torch tensors that live on the graph's device; nothing here computes on the CPU
and nothing synchronises (except ``chosen_sets``, a test/debug helper that
copies index sets back to the host).
"""
import ctypes as C
from typing import List, Optional, Sequence, Set

import numpy as np
import torch

from . import _lib
from .graph import CaseList, ChosenLists, DeviceGraph


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _i32(x, device) -> torch.Tensor:
    """ids / labels in whatever the reference passes (python list, numpy, LongTensor) -> int32 on device."""
    if torch.is_tensor(x):
        return x.to(device=device, dtype=torch.int32, non_blocking=True).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.int32)).to(device, non_blocking=True)


def score_table(g: DeviceGraph, W: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None,
                row_begin: int = 0, row_end: Optional[int] = None) -> torch.Tensor:
    """Class-0 label-aware logit of every node (layers.py:230-237)."""
    lib = _lib.load()
    if out is None:
        out = torch.empty(g.n_nodes, dtype=torch.float32, device=g.device)
    W = W.detach().contiguous()
    b = b.detach().contiguous()
    _lib.check(lib.pcg_score_table(g.desc_ref(), _p(W), _p(b), row_begin, g.n_nodes if row_end is None else row_end,
                                   _p(out), _stream(g.device)), "pcg_score_table")
    return out


def score_rows(g: DeviceGraph, W: torch.Tensor, b: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """Both label-aware logits of the given rows -> [n, 2] (layers.py:243)."""
    lib = _lib.load()
    out = torch.empty(ids.numel(), 2, dtype=torch.float32, device=g.device)
    W = W.detach().contiguous()
    b = b.detach().contiguous()
    _lib.check(lib.pcg_score_rows(g.desc_ref(), _p(W), _p(b), _p(ids), ids.numel(), _p(out), _stream(g.device)),
               "pcg_score_rows")
    return out


def pos_sort(g: DeviceGraph, s0: torch.Tensor, keys: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sorted (score, position) keys of the training positives (uint64 bit patterns in an int64 tensor)."""
    lib = _lib.load()
    cap = lib.pcg_pos_sort_capacity(g.n_pos)
    if keys is None:
        keys = torch.empty(cap, dtype=torch.int64, device=g.device)
    _lib.check(lib.pcg_pos_sort(g.desc_ref(), _p(s0), _p(keys), _stream(g.device)), "pcg_pos_sort")
    return keys


def gather_rows(g: DeviceGraph, ids: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = _lib.load()
    if out is None:
        out = torch.empty(ids.numel(), g.feat_dim, dtype=torch.float32, device=g.device)
    _lib.check(lib.pcg_gather_rows(g.desc_ref(), _p(ids), ids.numel(), _p(out), out.stride(0), _stream(g.device)),
               "pcg_gather_rows")
    return out


class ChooseWorkspace:
    """Per-(graph, batch size) scratch so the step itself never allocates: the tier queues,
    the selection list every row's chosen ids are written to, the gather's chunk table and
    partial sums.  ``list_capacity`` (entries) must cover sum over rows of the per-row bound
    ``(deg > k+1 ? k : deg) + m (+1)``; the default is the worst case for this graph and batch
    size (every centre being the largest hub), clipped to ``max_list_bytes``."""

    def __init__(self, g: DeviceGraph, B: int, list_capacity: Optional[int] = None, max_list_bytes: int = 8 << 30,
                 status: Optional[torch.Tensor] = None):
        lib = _lib.load()
        self.B = B
        self.clipped = False       # the default capacity was cut below the worst case: overflow is possible, check()!
        if list_capacity is None:
            # kept <= deg, minority m = int(ceil(deg/2) * rho) <= 2 * deg for rho <= 4 (and <= n_pos), +1 self
            per_row = g.max_degree + min(2 * max(g.max_degree, 1), g.n_pos) + 1
            worst = per_row * g.R * max(B, 1)
            list_capacity = min(worst, max_list_bytes // 4, (1 << 31) - 1)
            self.clipped = list_capacity < worst
        self.list_capacity = int(max(list_capacity, 1))
        nbytes = lib.pcg_choose_workspace_bytes(g.desc_ref(), B, self.list_capacity)
        if nbytes < 0:
            raise _lib.PcgnnLibraryError("pcg_choose_workspace_bytes rejected the arguments")
        self.buf = torch.zeros(int(nbytes), dtype=torch.uint8, device=g.device)
        self.status = status if status is not None else torch.zeros(1, dtype=torch.int32, device=g.device)
        self._g = g

    def view(self, which: int, dtype, count: int) -> torch.Tensor:
        off = _lib.load().pcg_choose_workspace_offset(self._g.desc_ref(), self.B, self.list_capacity, which)
        nbytes = count * torch.empty((), dtype=dtype).element_size()
        return self.buf[off:off + nbytes].view(dtype)

    def check(self):
        """Raise if a batch did not fit the selection list (reads the status word: synchronises)."""
        if int(self.status.item()) & _lib.PCG_ST_SEL_OVERFLOW:
            self.status.zero_()
            raise _lib.PcgnnLibraryError("selection list overflow: raise ChooseWorkspace(list_capacity=...)")


def sel_capacity(g: DeviceGraph, nodes_host: np.ndarray, labels_host: Optional[np.ndarray],
                 thresholds: Sequence[float], rho, train_flag: bool, add_self: bool = False) -> np.ndarray:
    """Host-side upper bound of every row's chosen-set size, [R, B] (pcg_sel_capacity_row, vectorised)."""
    minor = minority_counts(g, nodes_host, labels_host, thresholds, rho) if train_flag else None
    caps = []
    for r in range(g.R):
        deg = g.deg_host[r][nodes_host].astype(np.int64)
        k = np.ceil(deg * float(thresholds[r])).astype(np.int64)
        cap = np.where(deg > k + 1, k, deg)
        if train_flag:
            cap = cap + minor[r]
        caps.append(cap + (1 if add_self else 0))
    return np.stack(caps)


def minority_counts(g: DeviceGraph, nodes_host: np.ndarray, labels_host: np.ndarray, thresholds: Sequence[float],
                    rho) -> np.ndarray:
    """The number of minority picks of every train-mode row, int64 [R, n]: m = min(int(k * rho), n_pos) for a positive centre
    (label 1), 0 otherwise (layers.py:675-691; pcg_sel_capacity_row's minority term, vectorised)."""
    pos = np.asarray(labels_host) == 1
    out = []
    for r in range(g.R):
        deg = g.deg_host[r][nodes_host].astype(np.int64)
        k = np.ceil(deg * float(thresholds[r])).astype(np.int64)
        rr = float(rho) if np.isscalar(rho) else float(rho[r])
        m = np.minimum((k * rr).astype(np.int64), g.n_pos)
        out.append(np.where(pos, np.maximum(m, 0), 0).astype(np.int64))
    return np.stack(out)


def _host_arrays(g, thresholds, rho):
    thr = (C.c_double * g.R)(*[float(t) for t in thresholds])
    rhos = (C.c_double * g.R)(*([float(rho)] * g.R if np.isscalar(rho) else [float(x) for x in rho]))
    return thr, rhos


def choose_select(g: DeviceGraph, nodes, labels, s0, pos_keys, thresholds, rho, train_flag: bool, ws: ChooseWorkspace,
                  cnt: torch.Tensor, add_self: bool = False, center_s0=None, planned: bool = False):
    """plan + select only: every row's chosen ids into ws's selection list, |set| into cnt [R*B].
    planned: ws already holds this batch's plan (step_front / step_front_a + _b)."""
    lib = _lib.load()
    thr, rhos = _host_arrays(g, thresholds, rho)
    args = (g.desc_ref(), _p(nodes), _p(labels), nodes.numel(), _p(s0), _p(center_s0), _p(pos_keys), thr, rhos,
            1 if train_flag else 0, 1 if add_self else 0, _p(cnt), _p(ws.buf))
    rest = (ws.list_capacity, _p(ws.status), _stream(g.device))
    if planned:
        _lib.check(lib.pcg_choose_select_planned(*args, None, ws.list_capacity, _p(ws.status), None, 0, _stream(g.device)),
                   "pcg_choose_select_planned")
    else:
        _lib.check(lib.pcg_choose_select(*args, *rest), "pcg_choose_select")


def aggregate_lists(g: DeviceGraph, X: torch.Tensor, B: int, ws: ChooseWorkspace, cnt: torch.Tensor, agg: torch.Tensor,
                    norm: int = _lib.PCG_NORM_COUNT):
    """gather + mean of the lists ws holds, from feature table X [*, feat_stride] (g.X or an extended table)."""
    lib = _lib.load()
    _lib.check(lib.pcg_aggregate_lists(_p(X), g.feat_dim, X.stride(0), X.shape[0], g.R * B, _p(cnt), g.desc_ref(), B, _p(ws.buf),
                                       ws.list_capacity, norm, _p(agg), agg.stride(-2), _p(ws.status), _stream(g.device)),
               "pcg_aggregate_lists")


def choose_aggregate(g: DeviceGraph, nodes: torch.Tensor, labels: Optional[torch.Tensor], s0: torch.Tensor,
                     pos_keys: Optional[torch.Tensor], thresholds: Sequence[float], rho, train_flag: bool,
                     norm: int = _lib.PCG_NORM_COUNT, add_self: bool = False,
                     center_s0: Optional[torch.Tensor] = None, ws: Optional[ChooseWorkspace] = None,
                     agg: Optional[torch.Tensor] = None, cnt: Optional[torch.Tensor] = None, planned: bool = False):
    """choose + mean for all relations of a batch -> agg [R, B, F] (and |set| [R, B]).
    planned: ws already holds this batch's plan (step_front)."""
    lib = _lib.load()
    B = nodes.numel()
    if ws is None or ws.B != B:
        ws = ChooseWorkspace(g, B)
    if agg is None:
        agg = torch.empty(g.R, B, g.feat_dim, dtype=torch.float32, device=g.device)
    if cnt is None:
        cnt = torch.empty(g.R, B, dtype=torch.int32, device=g.device)
    thr, rhos = _host_arrays(g, thresholds, rho)
    fn = lib.pcg_choose_aggregate_planned if planned else lib.pcg_choose_aggregate
    _lib.check(fn(
        g.desc_ref(), _p(nodes), _p(labels), B, _p(s0), _p(center_s0), _p(pos_keys), thr, rhos,
        1 if train_flag else 0, norm, 1 if add_self else 0, _p(agg), agg.stride(-2), _p(cnt),
        _p(ws.buf), ws.list_capacity, _p(ws.status), _stream(g.device)), "pcg_choose_aggregate")
    return agg, cnt


def step_front(g: DeviceGraph, W: torch.Tensor, b: torch.Tensor, s0: torch.Tensor, pos_keys: Optional[torch.Tensor],
               nodes: torch.Tensor, labels: Optional[torch.Tensor], thresholds: Sequence[float], rho, train_flag: bool,
               ws: ChooseWorkspace, add_self: bool = False):
    """score table + train-pos sort + the batch's plan in two launches (pcg_step_front); follow with
    choose_aggregate(..., planned=True) on the same arguments.  Returns the sorted keys (or None)."""
    lib = _lib.load()
    B = nodes.numel()
    assert ws.B == B
    thr, rhos = _host_arrays(g, thresholds, rho)
    sort = bool(train_flag) and g.n_pos > 0
    _lib.check(lib.pcg_step_front(
        g.desc_ref(), _p(W), _p(b), _p(s0), _p(pos_keys) if sort else None, _p(nodes), _p(labels), B, thr, rhos,
        1 if train_flag else 0, 1 if add_self else 0, _p(ws.buf), ws.list_capacity, _p(ws.status),
        _stream(g.device)), "pcg_step_front")
    return pos_keys if sort else None


def read_sets(g: DeviceGraph, B: int, ws: ChooseWorkspace):
    """Copy the selection list of the last call to the host -> sets[r][b] (synchronises)."""
    rows = g.R * B
    torch.cuda.synchronize(g.device)
    ws.check()
    begin = ws.view(0, torch.int64, rows + 1).cpu().numpy()
    length = ws.view(1, torch.int32, rows).cpu().numpy()
    total = int(begin[-1])
    lst = ws.view(2, torch.int32, max(total, 1)).cpu().numpy()
    sets: List[List[Set[int]]] = []
    for r in range(g.R):
        row_sets = []
        for b in range(B):
            row = r * B + b
            seg = lst[begin[row]:begin[row] + length[row]]
            row_sets.append(set(seg[seg >= 0].tolist()))
        sets.append(row_sets)
    return sets


def chosen_sets(g: DeviceGraph, nodes, labels, s0, pos_keys, thresholds, rho, train_flag,
                norm=_lib.PCG_NORM_COUNT, add_self=False, center_s0=None, list_capacity=None):
    """Debug / parity helper: run the hot path and copy the chosen index sets to the host.
    Returns (sets[r][b], agg, cnt)."""
    B = nodes.numel()
    if list_capacity is None:     # exact requirement of this batch (host arithmetic)
        labels_h = None if labels is None else labels.cpu().numpy()
        list_capacity = int(sel_capacity(g, nodes.cpu().numpy(), labels_h, thresholds, rho, train_flag, add_self).sum())
    ws = ChooseWorkspace(g, B, list_capacity=max(list_capacity, 1))
    agg, cnt = choose_aggregate(g, nodes, labels, s0, pos_keys, thresholds, rho, train_flag, norm, add_self,
                                center_s0, ws)
    sets = read_sets(g, B, ws)
    return sets, agg, cnt


def check_status(status: torch.Tensor):
    """Read a device status word (synchronises); a set bit is cleared and raised, every bit by name."""
    st = int(status.item())
    if st:
        status.zero_()
        from .fused import FusedPCGNN
        FusedPCGNN._raise_status(st)


def rank_offsets(caps: np.ndarray) -> np.ndarray:
    """The flat output offsets [R * n + 1] of the per-row kept counts caps [R, n] (sel_capacity in test mode: exact)."""
    off = np.zeros(caps.size + 1, dtype=np.int64)
    np.cumsum(np.asarray(caps, dtype=np.int64).reshape(-1), out=off[1:])
    return off


def rank_lists(g: DeviceGraph, nodes: torch.Tensor, s0: torch.Tensor, ws: ChooseWorkspace, out_begin: torch.Tensor,
               out_ids: torch.Tensor, out_dist: torch.Tensor, center_s0: Optional[torch.Tensor] = None):
    """The lists a TEST-mode choose_select / choose_aggregate call left in ``ws``, in the reference's order with their
    distances (pcg_rank_lists): row (r, b) at out_begin[r * B + b] of out_ids / out_dist.  out_begin: int64 device tensor
    [R * B + 1] (rank_offsets of the rows' exact kept counts).  A row whose device count differs from its extent sets
    PCG_ST_RANK_MISMATCH in ws.status and is not written.  Nothing synchronises."""
    lib = _lib.load()
    _lib.check(lib.pcg_rank_lists(g.desc_ref(), _p(nodes), nodes.numel(), _p(s0), _p(center_s0), _p(ws.buf), ws.list_capacity,
                                  _p(out_begin), _p(out_ids), _p(out_dist), _p(ws.status), _stream(g.device)), "pcg_rank_lists")


def rank_minority(g: DeviceGraph, nodes: torch.Tensor, s0: torch.Tensor, pos_keys: torch.Tensor, out_begin: torch.Tensor,
                  out_ids: torch.Tensor, out_dist: torch.Tensor, status: torch.Tensor,
                  center_s0: Optional[torch.Tensor] = None):
    """The minority picks of train-mode rows, ranked, with their distances (pcg_rank_minority): row (r, i) - its extent in
    out_begin (int64 device tensor [R * n + 1], rank_offsets of minority_counts) IS its m - receives the m training positives
    nearest to the centre's score, ascending distance, ties by position in train_pos.  pos_keys: pos_sort's of the same s0.
    An extent that is negative, above n_pos or leaves the arrays sets PCG_ST_RANK_MISMATCH in ``status`` and the row is not
    written.  Needs no workspace and no plan; nothing synchronises."""
    lib = _lib.load()
    _lib.check(lib.pcg_rank_minority(g.desc_ref(), _p(nodes), nodes.numel(), _p(s0), _p(center_s0), _p(pos_keys), _p(out_begin),
                                     _p(out_ids), _p(out_dist), _p(status), _stream(g.device)), "pcg_rank_minority")


def choose_ranked(g: DeviceGraph, nodes, s0: torch.Tensor, thresholds: Sequence[float],
                  center_s0: Optional[torch.Tensor] = None, labels=None, rho=None,
                  pos_keys: Optional[torch.Tensor] = None) -> ChosenLists:
    """choose_step_test for all relations of a batch, on the device: select (test mode) followed by rank.  Returns a
    ``ChosenLists`` (offsets [R, B + 1], ids, dist - unpacks as ``offsets, ids, dist = choose_ranked(...)``).  The offsets are
    host arithmetic on the degrees; one read of the status word at the end (synchronises).
    With ``labels`` (one per node, 0 / 1) it is choose_step_neighs - train mode: the neighbour part is the test-mode one
    unchanged (k and the keep-all rule are the same in both modes), and the result carries the minority part too - per row of a
    positive centre the m = min(int(k * rho), n_pos) nearest training positives, ranked (``rank_minority``; rho: a scalar or
    one per relation; pos_keys: ``pos_sort`` of s0, sorted here if not given)."""
    nodes = _i32(nodes, g.device).view(-1)
    B = nodes.numel()
    nodes_host = nodes.cpu().numpy().astype(np.int64)
    caps = sel_capacity(g, nodes_host, None, thresholds, 0.0, False)
    off = rank_offsets(caps)
    total = int(off[-1])
    out_begin = torch.from_numpy(off).to(g.device)
    ids = torch.empty(total, dtype=torch.int32, device=g.device)
    dist = torch.empty(total, dtype=torch.float32, device=g.device)
    minor = {}
    if labels is not None:
        labels_host = (labels.detach().cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)).reshape(-1)
        if labels_host.size != B:
            raise ValueError(f"choose_ranked: {labels_host.size} labels for {B} nodes")
        moff = rank_offsets(minority_counts(g, nodes_host, labels_host, thresholds, 0.0 if rho is None else rho))
        minor = dict(minor_flat_offsets=torch.from_numpy(moff).to(g.device), minor_host_offsets=moff,
                     minor_ids=torch.empty(int(moff[-1]), dtype=torch.int32, device=g.device),
                     minor_dist=torch.empty(int(moff[-1]), dtype=torch.float32, device=g.device))
    if B:
        ws = ChooseWorkspace(g, B, list_capacity=max(total, 1))
        cnt = torch.empty(g.R * B, dtype=torch.int32, device=g.device)
        choose_select(g, nodes, None, s0, None, thresholds, 0.0, False, ws, cnt, center_s0=center_s0)
        rank_lists(g, nodes, s0, ws, out_begin, ids, dist, center_s0=center_s0)
        if minor and g.n_pos and int(minor["minor_host_offsets"][-1]):
            if pos_keys is None:
                pos_keys = pos_sort(g, s0)
            rank_minority(g, nodes, s0, pos_keys, minor["minor_flat_offsets"], minor["minor_ids"], minor["minor_dist"], ws.status,
                          center_s0=center_s0)
        check_status(ws.status)
    return ChosenLists(out_begin, ids, dist, g.R, B, host_offsets=off, **minor)


def neighbour_contrib(g: DeviceGraph, chosen: ChosenLists, d_agg: torch.Tensor, status: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Every chosen neighbour's share of its relation's contribution (pcg_attr_neighbours): for entry e of row (r, i) of
    ``chosen``, out[e] = <X[chosen.ids[e]], d_agg[r, i]> / row length - float32 [total], beside ``chosen.ids``.  d_agg: any
    float32 [R, n, F] tensor (``Attribution.d_agg``: a row's entries then sum to rel_contrib[r, i]).  An id outside the table
    sets PCG_ST_LIST_ID_RANGE in ``status``, a row whose offsets are not ascending inside [0, total] PCG_ST_RANK_MISMATCH (and
    is not written).  status None: a word of the call's own, read at the end (synchronises) and raised; else nothing
    synchronises.  out: a contiguous float32 tensor of chosen.ids.numel() entries to write into (None: a new one)."""
    lib = _lib.load()
    R, n = chosen.R, chosen.n
    d_agg = d_agg.detach()
    if d_agg.dtype != torch.float32 or tuple(d_agg.shape) != (R, n, g.feat_dim):
        raise ValueError(f"neighbour_contrib: d_agg must be float32 [{R}, {n}, {g.feat_dim}], got {d_agg.dtype} {tuple(d_agg.shape)}")
    if R != g.R or chosen.flat_offsets.numel() != R * n + 1 or chosen.flat_offsets.dtype != torch.int64:
        raise ValueError("neighbour_contrib: the lists are not this graph's (relations / offsets)")
    d_agg = d_agg.to(g.device).contiguous()
    if out is None:
        out = torch.empty(chosen.ids.numel(), dtype=torch.float32, device=g.device)
    elif out.dtype != torch.float32 or out.numel() != chosen.ids.numel() or not out.is_contiguous() or out.device != d_agg.device:
        raise ValueError("neighbour_contrib: out must be a contiguous float32 device tensor with one entry per list entry")
    if out.numel() == 0:
        return out
    own = status is None
    if own:
        status = torch.zeros(1, dtype=torch.int32, device=g.device)
    _lib.check(lib.pcg_attr_neighbours(g.desc_ref(), _p(chosen.flat_offsets), _p(chosen.ids), R, n, _p(d_agg), _p(out), _p(status),
                                       _stream(g.device)), "pcg_attr_neighbours")
    if own:
        check_status(status)
    return out


def segment_mean(g: DeviceGraph, begin: torch.Tensor, count: torch.Tensor, idx: torch.Tensor,
                 norm: int = _lib.PCG_NORM_COUNT, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Mean of explicit index lists (mask.div(n).mm(X[unique]), layers.py:599-624)."""
    lib = _lib.load()
    n = begin.numel()
    if out is None:
        out = torch.empty(n, g.feat_dim, dtype=torch.float32, device=g.device)
    _lib.check(lib.pcg_segment_mean(g.desc_ref(), _p(begin), _p(count), _p(idx), n, norm, _p(out), out.stride(0),
                                    _stream(g.device)), "pcg_segment_mean")
    return out


def pick(cum: torch.Tensor, idx_train: torch.Tensor, k: int, uniforms: Optional[torch.Tensor] = None,
         seed: int = 0, epoch: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Label-balanced pick (random.choices with cumulative weights, utils.py:274-278)."""
    lib = _lib.load()
    if out is None:
        out = torch.empty(k, dtype=torch.int32, device=cum.device)
    _lib.check(lib.pcg_pick(_p(cum), _p(idx_train), idx_train.numel(), _p(uniforms), seed & (2 ** 64 - 1),
                            epoch & (2 ** 64 - 1), k, _p(out), _stream(cum.device)), "pcg_pick")
    return out


def pick_shuffled(cum: torch.Tensor, idx_train: torch.Tensor, k: int, seed: int, epoch_base: int,
                  out_ids: torch.Tensor, labels_all: Optional[torch.Tensor] = None,
                  out_labels: Optional[torch.Tensor] = None, epoch_counter: Optional[torch.Tensor] = None,
                  bump: bool = False, n_epochs: int = 1):
    """An epoch's picks, shuffled, with their labels, in one launch (pcg_pick_shuffled): the same draws as
    ``pick(seed, epoch)``, in a uniformly random order.  epoch = epoch_base + epoch_counter[0] (a device int64 the
    call increments afterwards when ``bump``: a captured graph then replays a new epoch every time).  n_epochs > 1: that many
    consecutive epochs in one launch, epoch e's k draws at out_ids[e * k:] (the counter moves on by n_epochs)."""
    lib = _lib.load()
    _lib.check(lib.pcg_pick_shuffled_epochs(_p(cum), _p(idx_train), idx_train.numel(), seed & (2 ** 64 - 1),
                                            epoch_base & (2 ** 64 - 1), _p(epoch_counter), 1 if bump else 0, n_epochs, k,
                                            _p(labels_all), _p(out_ids), _p(out_labels), _stream(cum.device)),
               "pcg_pick_shuffled_epochs")
    return out_ids


def step_front_a(g: DeviceGraph, W: torch.Tensor, b: torch.Tensor, s0_out: torch.Tensor, row_begin: int, row_end: int,
                 nodes: torch.Tensor, labels: Optional[torch.Tensor], thresholds: Sequence[float], rho, train_flag: bool,
                 ws: ChooseWorkspace, add_self: bool = False, row_ids: Optional[torch.Tensor] = None):
    """first half of step_front: scores of rows [row_begin, row_end) (as score_table; with row_ids: row r's score goes to
    s0_out[row_ids[r]], negative = skipped) || plan pass 1."""
    lib = _lib.load()
    thr, rhos = _host_arrays(g, thresholds, rho)
    _lib.check(lib.pcg_step_front_a(g.desc_ref(), _p(W), _p(b), row_begin, row_end, _p(s0_out), _p(row_ids), None, _p(nodes), _p(labels),
                                    nodes.numel(), thr, rhos, 1 if train_flag else 0, 1 if add_self else 0, _p(ws.buf),
                                    ws.list_capacity, _p(ws.status), _stream(g.device)), "pcg_step_front_a")


def step_front_b(g: DeviceGraph, s0: torch.Tensor, pos_keys: Optional[torch.Tensor], nodes: torch.Tensor,
                 labels: Optional[torch.Tensor], thresholds: Sequence[float], rho, train_flag: bool, ws: ChooseWorkspace,
                 add_self: bool = False, center_out: Optional[torch.Tensor] = None, center_id_offset: int = 0):
    """second half of step_front: train-pos sort by s0 || plan pass 2 (|| center_out[i] = s0[nodes[i] + center_id_offset]).
    Returns the sorted keys (or None)."""
    lib = _lib.load()
    thr, rhos = _host_arrays(g, thresholds, rho)
    sort = bool(train_flag) and g.n_pos > 0
    _lib.check(lib.pcg_step_front_b(g.desc_ref(), _p(s0), _p(pos_keys) if sort else None, 0, _p(nodes), _p(labels),
                                    nodes.numel(), thr, rhos, 1 if train_flag else 0, 1 if add_self else 0, _p(ws.buf),
                                    ws.list_capacity, _p(ws.status), _p(center_out), center_id_offset, _stream(g.device)),
               "pcg_step_front_b")
    return pos_keys if sort else None


_EVAL_CACHE = {}


def eval_thresholds(thresholds=None) -> np.ndarray:
    """The threshold vector of an evaluation: float64, ascending; default the reference's linspace(0.01, 0.99, 100)."""
    th = np.linspace(0.01, 0.99, 100) if thresholds is None else np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if th.size < 1 or th.size > 1024 or np.any(np.isnan(th)) or np.any(np.diff(th) < 0):
        raise ValueError("eval_counts: 1 .. 1024 ascending thresholds")
    return th


def eval_counts(prob: torch.Tensor, labels: torch.Tensor, thresholds=None, stream=None, status: Optional[torch.Tensor] = None):
    """The integer counts every reported metric is a function of (pcg_eval_counts): uint64 words in an int64 device tensor
    [8 + 2 T] = tp, fp, fn, tn, n1, n0, 2U, 0, tp_t[T], npred_t[T].  prob: float32 [n, 2] on the device, labels: int32 [n] on the
    device, thresholds: None (linspace(0.01, 0.99, 100)), a host sequence or a float64 device tensor.  Nothing synchronises;
    a bad label / a NaN sets PCG_ST_EVAL_INPUT in ``status`` (a device int32 word; the per-device default one is read by
    utils.device_metrics).  The workspace and the default thresholds are kept per device and reused by the next call."""
    lib = _lib.load()
    dev = prob.device
    if dev.type != "cuda":
        raise _lib.PcgnnLibraryError("eval_counts runs on the GPU only: there is no CPU fallback for the product path")
    if prob.dtype != torch.float32 or prob.dim() != 2 or prob.shape[1] != 2 or labels.dtype != torch.int32 or labels.numel() != prob.shape[0]:
        raise ValueError("eval_counts: prob float32 [n, 2], labels int32 [n]")
    prob, labels = prob.contiguous(), labels.contiguous()
    n = prob.shape[0]
    cache = _EVAL_CACHE.setdefault((dev.type, dev.index if dev.index is not None else torch.cuda.current_device()), {})
    if torch.is_tensor(thresholds):
        th = thresholds.to(device=dev, dtype=torch.float64).contiguous()
    else:
        key = None if thresholds is None else tuple(float(t) for t in np.asarray(thresholds, dtype=np.float64).reshape(-1))
        th = cache.get(("th", key))
        if th is None:
            th = cache[("th", key)] = torch.from_numpy(eval_thresholds(thresholds)).to(dev)
    T = th.numel()
    nbytes = lib.pcg_eval_workspace_bytes(n, T)
    if nbytes < 0:
        raise _lib.PcgnnLibraryError(f"pcg_eval_workspace_bytes rejected n {n} / {T} thresholds")
    if cache.get("ws") is None or cache["ws"].numel() < nbytes:
        cache["ws"] = None
        cache["ws"] = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    if status is None:
        status = cache.get("status")
        if status is None:
            status = cache["status"] = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty(8 + 2 * T, dtype=torch.int64, device=dev)
    st = _stream(dev) if stream is None else C.c_void_p(stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream))
    _lib.check(lib.pcg_eval_counts(_p(prob), _p(labels), n, _p(th), T, _p(cache["ws"]), _p(out), _p(status), st), "pcg_eval_counts")
    return out


def eval_status(device) -> torch.Tensor:
    """The per-device status word eval_counts ORs PCG_ST_EVAL_INPUT into by default."""
    dev = torch.device(device)
    cache = _EVAL_CACHE.setdefault((dev.type, dev.index if dev.index is not None else torch.cuda.current_device()), {})
    if cache.get("status") is None:
        cache["status"] = torch.zeros(1, dtype=torch.int32, device=dev)
    return cache["status"]


def _eval_cache(dev) -> dict:
    return _EVAL_CACHE.setdefault((dev.type, dev.index if dev.index is not None else torch.cuda.current_device()), {})


def _cached_ws(cache: dict, key: str, nbytes: int, dev) -> torch.Tensor:
    if cache.get(key) is None or cache[key].numel() < nbytes:
        cache[key] = None
        cache[key] = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    return cache[key]


def pr_counts(prob: torch.Tensor, labels: torch.Tensor, cap: Optional[int] = None, stream=None, status: Optional[torch.Tensor] = None):
    """The integers average precision and the G-mean are functions of (pcg_pr_counts) -> (hdr, tp_g, npred_g) on the device:
    hdr int64 [8] = tp, fp, fn, tn, n1, n0, G, 0 (the first six are eval_counts'); tp_g / npred_g int32 [cap] (uint32 words), of
    which the first min(G, cap) are written, in descending score order: with u_1 > ... > u_G the distinct p1 of the positives,
    tp_g = #{y = 1, p1 >= u_g}, npred_g = #{p1 >= u_g}.  prob: float32 [n, 2] on the device, labels: int32 [n] on the device;
    cap: None = n (n1 always suffices); G > cap sets PCG_ST_PR_OVERFLOW in ``status``, a bad label / a NaN PCG_ST_EVAL_INPUT
    (the per-device default word is read by utils.device_ranking).  Nothing synchronises; the workspace is kept per device."""
    lib = _lib.load()
    dev = prob.device
    if dev.type != "cuda":
        raise _lib.PcgnnLibraryError("pr_counts runs on the GPU only: there is no CPU fallback for the product path")
    if prob.dtype != torch.float32 or prob.dim() != 2 or prob.shape[1] != 2 or labels.dtype != torch.int32 or labels.numel() != prob.shape[0]:
        raise ValueError("pr_counts: prob float32 [n, 2], labels int32 [n]")
    prob, labels = prob.contiguous(), labels.contiguous()
    n = prob.shape[0]
    cap = n if cap is None else int(cap)
    if cap < 0:
        raise ValueError("pr_counts: cap >= 0")
    cache = _eval_cache(dev)
    nbytes = lib.pcg_pr_workspace_bytes(n)
    if nbytes < 0:
        raise _lib.PcgnnLibraryError(f"pcg_pr_workspace_bytes rejected n {n}")
    ws = _cached_ws(cache, "pr_ws", nbytes, dev)
    status = eval_status(dev) if status is None else status
    hdr = torch.empty(8, dtype=torch.int64, device=dev)
    tp_g = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)     # (an empty tensor has no address)
    npred_g = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    st = _stream(dev) if stream is None else C.c_void_p(stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream))
    _lib.check(lib.pcg_pr_counts(_p(prob), _p(labels), n, cap, _p(ws), _p(hdr), _p(tp_g), _p(npred_g), _p(status), st), "pcg_pr_counts")
    return hdr, tp_g[:cap], npred_g[:cap]


def topk_alerts(prob: torch.Tensor, k: int, stream=None, status: Optional[torch.Tensor] = None):
    """The first k rows of the alert order (pcg_topk_alerts) -> (pos int32 [k], score float32 [k]) on the device.  The alert
    order is the stable sort of the rows by p1 + 0.0f, descending: among equal scores the lower position in the input comes
    first, so a tie at the cut is resolved by input position.  prob: float32 on the device, [n, 2] (column 1 is ranked) or a
    vector [n]; 1 <= k <= PCG_ALERTS_MAX_K (65536); slots at and beyond n hold -1 / -inf.  A NaN sets PCG_ST_EVAL_INPUT in
    ``status`` (default: the per-device word of eval_status).  Nothing synchronises; the workspace is kept per device."""
    lib = _lib.load()
    dev = prob.device
    if dev.type != "cuda":
        raise _lib.PcgnnLibraryError("topk_alerts runs on the GPU only: there is no CPU fallback for the product path")
    if prob.dtype != torch.float32 or not (prob.dim() == 1 or (prob.dim() == 2 and prob.shape[1] == 2)):
        raise ValueError("topk_alerts: prob float32 [n, 2] or [n]")
    k = int(k)
    if k < 1 or k > _lib.PCG_ALERTS_MAX_K:
        raise ValueError(f"topk_alerts: 1 <= k <= {_lib.PCG_ALERTS_MAX_K}")
    prob = prob.contiguous()
    n, stride = prob.shape[0], (2 if prob.dim() == 2 else 1)
    nbytes = lib.pcg_topk_alerts_workspace_bytes(n, k)
    if nbytes < 0:
        raise _lib.PcgnnLibraryError(f"pcg_topk_alerts_workspace_bytes rejected n {n} / k {k}")
    ws = _cached_ws(_eval_cache(dev), "alerts_ws", nbytes, dev)
    status = eval_status(dev) if status is None else status
    pos = torch.empty(k, dtype=torch.int32, device=dev)
    score = torch.empty(k, dtype=torch.float32, device=dev)
    p1 = None if n == 0 else C.c_void_p(prob.data_ptr() + 4 * (stride - 1))
    st = _stream(dev) if stream is None else C.c_void_p(stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream))
    _lib.check(lib.pcg_topk_alerts(p1, stride, n, k, _p(ws), _p(pos), _p(score), _p(status), st), "pcg_topk_alerts")
    return pos, score


def relation_mask(g: DeviceGraph, relations) -> int:
    """``relations`` (None = all, else a non-empty subset of range(R)) as pcg_alert_cases' bit mask."""
    if relations is None:
        return (1 << g.R) - 1
    rel = sorted({int(r) for r in relations})
    if not rel or rel[0] < 0 or rel[-1] >= g.R:
        raise ValueError(f"relations: a non-empty subset of range({g.R}), got {list(relations)!r}")
    return sum(1 << r for r in rel)


def group_members_enqueue(g: DeviceGraph, members: torch.Tensor, rel_mask: int, labels: Optional[torch.Tensor], status: torch.Tensor):
    """pcg_alert_cases on the current stream, nothing read back: -> (case_of, head, offsets, order, links, hits or None, hdr), every
    buffer at the size include/pcgnn.h documents (head / links / hits [m], offsets [m + 1], order [m], hdr [4] = C, valid slots,
    the status word, 0).  members int32 [m] and labels int32 [m] or None on the device.  Capture-safe once the per-device
    workspace has its size (a first call outside the capture)."""
    lib = _lib.load()
    dev = g.device
    m = int(members.numel())
    if m > _lib.PCG_ALERTS_MAX_K:
        raise ValueError(f"group_members: at most {_lib.PCG_ALERTS_MAX_K} members, got {m}")
    nbytes = int(lib.pcg_alert_cases_workspace_bytes(g.n_nodes, m))
    if nbytes < 0:
        _lib.check(nbytes, f"pcg_alert_cases_workspace_bytes(n_nodes={g.n_nodes}, m={m})")
    ws = _cached_ws(_eval_cache(dev), "cases_ws", nbytes, dev)
    cap = max(m, 1)                                                     # (an empty tensor has no address)
    case_of, head, order, links = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(4))
    offsets = torch.empty(m + 1, dtype=torch.int32, device=dev)
    hits = None if labels is None else torch.empty(cap, dtype=torch.int32, device=dev)
    hdr = torch.empty(4, dtype=torch.int32, device=dev)
    _lib.check(lib.pcg_alert_cases(g.desc_ref(), _p(members) if m else None, m, rel_mask, _p(labels) if m else None, _p(ws), nbytes,
                                   _p(case_of), _p(head), _p(offsets), _p(order), _p(links), _p(hits) if m else None, _p(hdr),
                                   _p(status), _stream(dev)), "pcg_alert_cases")
    return case_of[:m], head, offsets, order, links, hits, hdr


def group_members(g: DeviceGraph, members, relations=None, labels=None, status: Optional[torch.Tensor] = None, alerts=None):
    """Members grouped into cases (pcg_alert_cases) -> ``graph.CaseList``.  members: up to 65536 node ids of ``g`` in alert
    order (int sequence or tensor), -1 = padding (in no case); slot p is linked to slot q when both name the same node or, in a
    selected relation, either node is in the other's CSR row; a case is a connected component, numbered by its lowest slot.
    relations: None = all, else a non-empty subset of range(R).  labels (one per slot, 0 / 1): the result holds ``hits``.
    Enqueues on the current stream and reads the header - the number of cases and the status word - once: an id that is
    neither -1 nor a node (it is then treated as padding), a label outside {0, 1} or a bounded loop that ran out raises.
    status: a zeroed int32 device word of the caller's - then nothing raises, the word is the report (``check_status``).
    Out of scope: the ids of a query batch (they are query-local), a partitioned graph, 2-hop linking, more than 65536 members."""
    dev = g.device
    members = _i32(members, dev).view(-1)
    m = int(members.numel())
    rel_mask = relation_mask(g, relations)
    lab = None
    if labels is not None:
        lab = _i32(labels, dev).view(-1)
        if lab.numel() != m:
            raise ValueError(f"group_members: {lab.numel()} labels for {m} members")
    own = status is None
    st = torch.zeros(1, dtype=torch.int32, device=dev) if own else status
    case_of, head, offsets, order, links, hits, hdr = group_members_enqueue(g, members, rel_mask, lab, st)
    n_cases, n_valid, word, _ = (int(v) for v in hdr.tolist())            # the one synchronisation
    if own and word:
        what = [name for bit, name in ((_lib.PCG_ST_LIST_ID_RANGE, "a member id that is neither -1 nor a node of the graph"),
                                       (_lib.PCG_ST_EVAL_INPUT, "a label outside {0, 1}"),
                                       (_lib.PCG_ST_SYNC_TIMEOUT, "a bounded union-find loop ran out")) if word & bit]
        raise _lib.PcgnnLibraryError(f"group_members: {', '.join(what) or 'device status'} (status {word})")
    return CaseList(case_of, head[:n_cases], offsets[:n_cases + 1], order[:n_valid], links[:n_cases],
                    None if hits is None else hits[:n_cases], n_cases, members, alerts)


TOPK_METRICS = {"dot": 0, "cosine": 1, "l2": 2}
_TOPK_CACHE: dict = {}


def topk_similar(Q: torch.Tensor, bank: torch.Tensor, k: int, metric: str = "cosine", q_ids: Optional[torch.Tensor] = None,
                 bank_ids: Optional[torch.Tensor] = None, _slices: int = 0):
    """The k rows of ``bank`` [M, E] most similar to each row of ``Q`` [n, E] (float32 device tensors, E a multiple of 16 in
    16 .. 512, 1 <= k <= 64) -> (pos [n, k] int32 bank positions, score [n, k] float32), sorted by score descending with ties
    by lower position; slots beyond the number of eligible rows hold -1 / -inf (pcg_topk_similar: exact-f32 MFMA scores and a
    running top-k, no [n, M] matrix).  metric - always maximised: "dot" q.c | "cosine" q.c / (|q| |c|), 0 when either norm is
    0 | "l2" min(0, 2 q.c - |q|^2 - |c|^2).  q_ids [n], bank_ids [M] (both or neither): bank row c is skipped for query row i
    when bank_ids[c] == q_ids[i].  The result does not depend on how the kernel slices the bank (_slices: the tests' way to
    force a slice count; 0 = the kernel's choice).  Enqueues on the current stream; does not synchronise."""
    lib = _lib.load()
    if metric not in TOPK_METRICS:
        raise ValueError(f"topk_similar: metric {metric!r} is none of {sorted(TOPK_METRICS)}")
    if Q.dim() != 2 or bank.dim() != 2 or Q.shape[1] != bank.shape[1]:
        raise ValueError(f"topk_similar: Q {tuple(Q.shape)} and bank {tuple(bank.shape)} are not [n, E] and [M, E]")
    if Q.dtype != torch.float32 or bank.dtype != torch.float32 or Q.device != bank.device or Q.device.type != "cuda":
        raise _lib.PcgnnLibraryError("topk_similar: Q and bank must be float32 tensors on one GPU (there is no CPU path)")
    if (q_ids is None) != (bank_ids is None):
        raise ValueError("topk_similar: q_ids and bank_ids go together")
    dev = Q.device
    Q, bank = Q.detach().contiguous(), bank.detach().contiguous()
    n, E, M, k = int(Q.shape[0]), int(Q.shape[1]), int(bank.shape[0]), int(k)
    if q_ids is not None:
        q_ids, bank_ids = _i32(q_ids, dev).view(-1), _i32(bank_ids, dev).view(-1)
        if q_ids.numel() != n or bank_ids.numel() != M:
            raise ValueError("topk_similar: q_ids / bank_ids must have one id per row of Q / bank")
        if n == 0 or M == 0:                                # (nothing to exclude; an empty tensor has no address to pass)
            q_ids = bank_ids = None
    nbytes = int(lib.pcg_topk_similar_workspace_bytes(n, M, E, k))
    if nbytes < 0:
        _lib.check(nbytes, f"pcg_topk_similar_workspace_bytes(n={n}, M={M}, emb={E}, k={k})")
    cache = _TOPK_CACHE.setdefault((dev.type, dev.index if dev.index is not None else torch.cuda.current_device()), {})
    if cache.get("ws") is None or cache["ws"].numel() < nbytes:
        cache["ws"] = None
        cache["ws"] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        cache["status"] = torch.zeros(1, dtype=torch.int32, device=dev)
    pos = torch.empty(n, k, dtype=torch.int32, device=dev)
    score = torch.empty(n, k, dtype=torch.float32, device=dev)
    lib.pcg_debug_set_topk_slices(int(_slices))
    try:
        _lib.check(lib.pcg_topk_similar(_p(Q), n, _p(bank), M, E, k, TOPK_METRICS[metric], _p(q_ids), _p(bank_ids), _p(pos), _p(score),
                                        _p(cache["ws"]), _p(cache["status"]), _stream(dev)), "pcg_topk_similar")
    finally:
        if _slices:
            lib.pcg_debug_set_topk_slices(0)
    return pos, score
