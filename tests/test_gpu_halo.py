"""The halo exchange kernels of the node-partitioned path (pcg_halo_collect / _serve / _lookup, pcg_gather_lists_dist) against
the host reference tests/halo_ref.py, in ONE process on one GPU: the ranks are simulated one after another and the two
all-to-alls are slice copies.  The C ABI is driven directly (pcgnn_amd._lib); the whole-exchange test goes through
HaloExchangeHip (group=None: only its _a2a touches torch.distributed)."""
import time

import numpy as np
import pytest
import torch

from tests import halo_ref as H
from tests.util import synth_graph

pytestmark = pytest.mark.gpu

FEAT_TOL = 2e-5          # tests/test_gpu_parity.py's tolerance for aggregated features (reported against, not asserted with)
EMPTY = 0xFFFFFFFF


@pytest.fixture(scope="module")
def P():
    import pcgnn_amd
    from pcgnn_amd import ops  # noqa: F401  (fails loudly if the .so is missing)
    return pcgnn_amd


def dev():
    return torch.device("cuda", 0)


def _dt(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=dtype)).to(dev())


def _u32(t):
    return t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def ext_csr(csr_rows, n_table_rows):
    """a shard's CSR rows padded with empty rows up to the extended table's row count"""
    out = []
    for ip, ix in csr_rows:
        ip = np.asarray(ip, dtype=np.int64)
        out.append((np.concatenate([ip, np.full(n_table_rows - (ip.shape[0] - 1), ip[-1], dtype=np.int64)]), np.asarray(ix, np.int32)))
    return out


def rows_to_csr(rows):
    ip = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=ip[1:])
    return ip, (np.concatenate(rows).astype(np.int32) if ip[-1] else np.zeros(0, np.int32))


class Engine:
    """One rank's halo state (table, counts - zeroed ONCE -, request list) on a graph of its own CSR rows, driven through the C ABI."""

    def __init__(self, P, csr_rows, lo, hi, bounds, self_rank, train_pos, id_space, halo_cap, pitch, X_local=None, feat=4):
        from pcgnn_amd import _lib, ops
        self.lib, self._lib, self.ops = _lib.load(), _lib, ops
        self.lo, self.hi, self.n_local = int(lo), int(hi), int(hi - lo)
        self.bounds_host = [int(b) for b in bounds]
        self.world, self.self_rank = len(bounds) - 1, self_rank
        self.tp = np.asarray(list(train_pos), dtype=np.int64)
        self.P = int(self.tp.size)
        order = np.argsort(self.tp, kind="stable")
        self.pos_ids_host, self.pos_idx_host = self.tp[order], order
        self.halo_cap, self.pitch = int(halo_cap), int(pitch)
        self.halo_base = self.n_local + self.P
        n_rows = self.halo_base + max(self.halo_cap, 1)
        X = np.zeros((n_rows, feat), np.float32)
        if X_local is not None:
            X[:self.n_local] = X_local
        self.g = P.DeviceGraph(X, ext_csr(csr_rows, n_rows), list(train_pos), dev(), id_space=id_space)
        self.slots = int(self.lib.pcg_halo_table_slots(self.halo_cap))
        self.table = torch.empty(2 * self.slots, dtype=torch.int32, device=dev())
        self.counts = torch.zeros(131, dtype=torch.int32, device=dev())
        self.uniq = torch.full((max(self.halo_cap, 1),), -7, dtype=torch.int32, device=dev())
        self.pos_ids = _dt(self.pos_ids_host if self.P else [0])
        self.pos_idx = _dt(self.pos_idx_host if self.P else [0])
        self.bounds = _dt(self.bounds_host)

    def collect_rc(self, centres, n=None, world=None, self_rank=None):
        _p = self.ops._p
        centres = np.asarray(centres, dtype=np.int32)
        c = _dt(centres) if centres.size else torch.zeros(1, dtype=torch.int32, device=dev())     # (an empty tensor has no address)
        return self.lib.pcg_halo_collect(
            self.g.desc_ref(), _p(c), int(centres.size if n is None else n), self.lo, self.hi, self.n_local, _p(self.pos_ids), self.P,
            _p(self.bounds), self.world if world is None else world, _p(self.table), self.slots, _p(self.counts), _p(self.uniq),
            self.halo_cap, self.halo_base, self.pitch, self.self_rank if self_rank is None else self_rank, self.ops._stream(dev()))

    def collect(self, centres, n=None):
        self._lib.check(self.collect_rc(centres, n), "pcg_halo_collect")
        torch.cuda.synchronize()

    def state(self):
        t = _u32(self.table)
        return self.uniq.cpu().numpy()[:self.halo_cap], _u32(self.counts), t[:self.slots], t[self.slots:]

    def flags(self):
        return int(self.counts[128].item())

    def clear_flags(self):
        self.counts[128] = 0

    def check(self, expected):
        uniq, counts, keys, vals = self.state()
        return H.check_collect(uniq, counts, keys, vals, expected, self.bounds_host, self.pitch, self.halo_cap, self.world, self.self_rank)

    def lookup(self, ws, B):
        _p = self.ops._p
        self._lib.check(self.lib.pcg_halo_lookup(
            self.g.desc_ref(), B, _p(ws.buf), None, ws.list_capacity, self.lo, self.hi, self.n_local, _p(self.pos_ids), _p(self.pos_idx),
            self.P, _p(self.table), self.slots, _p(self.counts), self.halo_cap, self.halo_base, self.ops._stream(dev())), "pcg_halo_lookup")
        torch.cuda.synchronize()

    def row_gid(self):
        return np.concatenate([np.arange(self.lo, self.hi), self.tp, self.uniq.cpu().numpy()[:self.halo_cap].astype(np.int64)])

    def fill_halo(self, X_full_padded):
        """the halo rows straight from the whole table (what the two all-to-alls and pcg_halo_serve deliver)"""
        u = self.uniq[:self.halo_cap].long()
        ok = u >= 0
        self.g.X[self.halo_base:self.halo_base + self.halo_cap][ok] = X_full_padded[u[ok]]


def select_lists(ops, g, ids_local, labels, s0, keys, thr, rho, train, lo, slack=77, fill=None):
    """pcg_choose_select on a rank's extended-table graph (single-buffer workspace, plan inside): the lists hold GLOBAL ids.
    fill: value the list region holds before the select (what lies outside every row afterwards)."""
    ids_np = np.asarray(ids_local, dtype=np.int64)
    B = ids_np.size
    lab_np = None if labels is None else np.asarray(labels)
    cap = int(ops.sel_capacity(g, ids_np, lab_np, thr, rho, train).sum()) + slack
    ws = ops.ChooseWorkspace(g, B, list_capacity=cap)
    if fill is not None:
        ws.view(2, torch.int32, cap).fill_(int(fill))
    cnt = torch.zeros(g.R * B, dtype=torch.int32, device=dev())
    ids_t = _dt(ids_np)
    ops.choose_select(g, ids_t, None if labels is None else _dt(lab_np), s0, keys if train else None, thr, rho, train, ws, cnt,
                      center_s0=s0[(ids_t.long() + lo)].contiguous())
    torch.cuda.synchronize()
    ws.check()
    return ws, cnt


def read_lists(ws, rows):
    begin = ws.view(0, torch.int64, rows + 1).cpu().numpy()
    length = ws.view(1, torch.int32, rows).cpu().numpy()
    return begin, length, ws.view(2, torch.int32, ws.list_capacity).cpu().numpy().copy()


def in_use_mask(begin, length, cap):
    m = np.zeros(cap, dtype=bool)
    for b, n in zip(begin[:-1].tolist(), length.tolist()):
        m[b:b + n] = True
    return m


# ---------------------------------------------------------------------------------------------------------------------------
# collect
# ---------------------------------------------------------------------------------------------------------------------------
N_IDS = 6000
DEGREES = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000]        # (the collect loop takes 4 x 64 ids per pass)


def make_bounds(world, n, self_rank):
    """equal shards, but one OTHER rank's shard empty and another's a single node (world 3 has room for one of the two: an
    empty shard beside ranks 0 and 2, a one-node shard beside rank 1); what they give up goes to a third rank"""
    width = [n // world] * world
    others = [r for r in range(world) if r != self_rank]
    if world >= 4:
        e, o = others[len(others) // 2 - 1], others[-1]
        width[e], width[o] = 0, 1
    elif world == 3:
        width[others[0]] = 1 if self_rank == 1 else 0
    normal = [r for r in others if width[r] > 1]
    width[normal[0] if normal else self_rank] += n - sum(width)
    return np.concatenate([[0], np.cumsum(width)]).astype(np.int64)


def collect_case(world, self_rank, R, seed):
    rs = np.random.RandomState(seed)
    bounds = make_bounds(world, N_IDS, self_rank)
    lo, hi = int(bounds[self_rank]), int(bounds[self_rank + 1])
    n_local = hi - lo
    assert n_local >= 24
    edge = np.unique([i for i in (0, lo - 1, lo, hi - 1, hi, N_IDS - 1) if 0 <= i < N_IDS])
    csr_rows = []
    for r in range(R):
        degs = DEGREES[r * 5:] + DEGREES[:r * 5]                            # every relation has every degree, on other rows
        rows = [np.sort(rs.choice(N_IDS, size=d, replace=False)) for d in degs]
        rows.append(edge if r == 0 else edge[::-1][:3][::-1])
        rows += [np.sort(rs.choice(N_IDS, size=3, replace=False)) for _ in range(4)]
        rows += [np.zeros(0, np.int64)] * (n_local - len(rows))
        csr_rows.append(rows_to_csr(rows))
    big = csr_rows[0][1][csr_rows[0][0][11]:csr_rows[0][0][12]].astype(np.int64)        # the 1000-neighbour row
    remote = big[(big < lo) | (big >= hi)]
    tp = np.unique(np.concatenate([remote[::25], np.arange(lo, hi)[3:40:4]]))             # remote (never inserted) and owned ones
    tp = tp[~np.isin(tp, edge)]                                                           # (the edge ids stay requests: a one-node shard's id is one)
    tp = tp[rs.permutation(tp.size)]                                                      # (train_pos is not sorted)
    centres = np.concatenate([np.arange(len(DEGREES) + 5), [3, 3, 11, 12], [-1, n_local]]).astype(np.int32)
    rs.shuffle(centres)
    return bounds, lo, hi, csr_rows, tp, centres


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("world,self_rank", [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (8, 0), (8, 3), (8, 7), (64, 0), (64, 31), (64, 63)])
def test_collect_matches_reference(P, world, self_rank, R):
    """request list, counts and hash table of one window against set arithmetic, in the pitched and the packed layout"""
    bounds, lo, hi, csr_rows, tp, centres = collect_case(world, self_rank, R, 100 * world + self_rank)
    want = H.remote_set(csr_rows, centres, lo, hi, hi - lo, tp)
    per_owner = np.bincount(H.owners(bounds, want), minlength=world)[:world]
    if world > 1:
        others = [r for r in range(world) if r != self_rank and bounds[r + 1] > bounds[r]]
        assert want.size > 200 and (per_owner > 0).sum() >= min(len(others), 2)
        assert not np.isin(tp, want).any() and np.isin(tp, np.concatenate([ix for _, ix in csr_rows])).sum() > 5
    else:
        assert want.size == 0
    peers = max(world - 1, 1)
    for pitch in (int(per_owner.max()) + 3, 0):
        halo_cap = peers * pitch if pitch else int(want.size) + 5
        e = Engine(P, csr_rows, lo, hi, bounds, self_rank, tp, N_IDS, halo_cap, pitch)
        e.collect(centres)
        assert e.flags() == 0
        slot_of = e.check(want)
        assert len(slot_of) == want.size
        c = e.state()[1]
        assert (int(c[129]), int(c[130])) == (int(want.size), int(per_owner.max()))


def test_collect_hi_behind_an_empty_shard(P):
    """self at rank 0 of [0, a, a, a + 1, n]: `hi` belongs to the one-node shard BEHIND the empty one (the largest r with
    bounds[r] <= id), `hi + 1` to the last rank"""
    a_ = 40
    bounds = np.array([0, a_, a_, a_ + 1, N_IDS], dtype=np.int64)
    rows = [np.array([0, a_ - 1, a_, a_ + 1, N_IDS - 1]), np.array([a_, 77])] + [np.zeros(0, np.int64)] * (a_ - 2)
    for pitch in (4, 0):
        e = Engine(P, [rows_to_csr(rows)], 0, a_, bounds, 0, [], N_IDS, 12 if pitch else 4, pitch)
        e.collect([0, 1])
        assert e.flags() == 0
        slot_of = e.check(np.array([a_, a_ + 1, 77, N_IDS - 1]))
        assert e.state()[1][:4].tolist() == [0, 0, 1, 3] and len(slot_of) == 4
        if pitch:
            assert 4 <= slot_of[a_] < 8 and all(8 <= slot_of[i] < 12 for i in (a_ + 1, 77, N_IDS - 1))


def test_collect_rejects_bad_worlds(P):
    from pcgnn_amd import _lib
    bounds, lo, hi, csr_rows, tp, centres = collect_case(2, 0, 1, 1)
    e = Engine(P, csr_rows, lo, hi, bounds, 0, tp, N_IDS, 64, 64)
    wide = np.concatenate([bounds, np.full(70, N_IDS)])
    e.bounds = _dt(wide)
    assert e.collect_rc(centres, world=65) == _lib.PCG_E_ARG
    assert e.collect_rc(centres, world=2, self_rank=2) == _lib.PCG_E_ARG
    assert e.collect_rc(centres, world=2, self_rank=-1) == _lib.PCG_E_ARG
    assert e.collect_rc(centres, world=64, self_rank=64) == _lib.PCG_E_ARG
    torch.cuda.synchronize()
    assert int(e.counts.abs().sum().item()) == 0 and int((e.uniq != -7).sum().item()) == 0, "a rejected call touches nothing"


def test_collect_without_centres_resets(P):
    """n_centres == 0 (a one-element tensor for the address): request list all -1, counts zero, an empty table - also after a
    window that filled them"""
    bounds, lo, hi, csr_rows, tp, centres = collect_case(3, 1, 1, 2)
    want = H.remote_set(csr_rows, centres, lo, hi, hi - lo, tp)
    e = Engine(P, csr_rows, lo, hi, bounds, 1, tp, N_IDS, 2 * int(want.size), int(want.size))
    for fill_first in (False, True):
        if fill_first:
            e.collect(centres)
            assert len(e.check(want)) == want.size
        e.collect(np.zeros(0, np.int32), n=0)
        uniq, counts, keys, _ = e.state()
        assert np.all(uniq == -1) and np.all(counts[:128] == 0) and np.all(keys == EMPTY) and e.flags() == 0
        e.check(np.zeros(0, np.int64))
    # centres that are all outside the shard: the same
    e.collect(np.array([-1, hi - lo, -5], np.int32))
    e.check(np.zeros(0, np.int64))


def capacity_case():
    """world 3, self 1: row 0 has exactly 40 ids of owner 0, row 1 one more id of owner 0, row 2 seven ids of owner 2"""
    bounds = np.array([0, 2000, 4000, 6000], dtype=np.int64)
    rs = np.random.RandomState(5)
    a = np.sort(rs.choice(2000, size=41, replace=False))
    b = 4000 + np.sort(rs.choice(2000, size=7, replace=False))
    rows = [a[:40], a[40:], b] + [np.zeros(0, np.int64)] * 29
    return bounds, [rows_to_csr(rows)], a, b


def test_collect_capacity_pitched(P):
    bounds, csr_rows, a, b = capacity_case()
    e = Engine(P, csr_rows, 2000, 4000, bounds, 1, [], N_IDS, 80, 40)
    e.collect([0, 2])                                   # owner 0 exactly full
    assert e.flags() == 0
    assert len(e.check(np.concatenate([a[:40], b]))) == 47
    e.collect([0, 1, 2])                                # one id over owner 0's pitch
    assert e.flags() == 2
    slot_of = e.check(np.concatenate([a, b]))           # (exactly 40 of owner 0's 41 ids have slots, owner 2 is unaffected)
    assert len(slot_of) == 47 and all(int(i) in slot_of for i in b)
    c = e.state()[1]
    assert c[:3].tolist() == [41, 0, 7] and (int(c[129]), int(c[130])) == (48, 41)


def test_collect_capacity_packed(P):
    bounds, csr_rows, a, b = capacity_case()
    e = Engine(P, csr_rows, 2000, 4000, bounds, 1, [], N_IDS, 47, 0)
    e.collect([0, 2])                                   # the total exactly halo_cap
    assert e.flags() == 0
    assert len(e.check(np.concatenate([a[:40], b]))) == 47
    e.collect([0, 1, 2])                                # one over: bit 2 and no slot at all
    assert e.flags() == 2
    assert e.check(np.concatenate([a, b])) == {}
    assert np.all(e.state()[0] == -1)


def test_second_collect_replaces_the_first(P):
    """two windows on one engine, the second smaller: table, request list and per-owner counts are the second's alone; the
    running maxima and the (sticky) overflow bit are the first's until the caller clears it"""
    bounds, csr_rows, a, b = capacity_case()
    e = Engine(P, csr_rows, 2000, 4000, bounds, 1, [], N_IDS, 80, 40)
    e.collect([0, 1, 2])
    assert e.flags() == 2
    e.collect([2, 2])
    assert len(e.check(b)) == 7
    c = e.state()[1]
    assert c[:64].tolist() == [0, 0, 7] + [0] * 61
    assert (int(c[129]), int(c[130])) == (48, 41)
    assert e.flags() == 2, "bit 2 of the first window stays until it is cleared"
    e.clear_flags()
    e.collect([2])
    assert e.flags() == 0 and len(e.check(b)) == 7


# ---------------------------------------------------------------------------------------------------------------------------
# probing (halo_hash re-implemented in halo_ref ONLY to choose the inputs; expected values are set arithmetic)
# ---------------------------------------------------------------------------------------------------------------------------
ID_SPACE = 1 << 20


@pytest.fixture(scope="module")
def homes():
    ids = np.arange(64, ID_SPACE, dtype=np.int64)
    home = (H.halo_hash(ids) & np.uint64(1023)).astype(np.int64)
    per = np.bincount(home, minlength=1024)
    assert per.min() >= 2 * H.HALO_MAX_PROBE, "enough ids per home slot of a 1024-slot table"
    return ids, home


def probe_engine(P, rows):
    """this rank owns [0, 64) of a 2^20 id space; world 2; halo_cap 512 -> a table of 1024 slots; row i = rows[i]"""
    rows = [np.sort(np.asarray(r, dtype=np.int64)) for r in rows] + [np.zeros(0, np.int64)] * (64 - len(rows))
    e = Engine(P, [rows_to_csr(rows)], 0, 64, [0, 64, ID_SPACE], 0, [], ID_SPACE, 512, 512)
    assert e.slots == 1024
    return e


def lookup_all_found(P, e, row, ids):
    """keep-all select of local row `row` (threshold 1.0, test mode) + pcg_halo_lookup: every id is found in its slot"""
    s0 = torch.zeros(ID_SPACE, dtype=torch.float32, device=dev())
    ws, cnt = select_lists(P.ops, e.g, [row], None, s0, None, [1.0], 0.5, False, 0)
    begin, length, before = read_lists(ws, 1)
    assert int(length[0]) == len(ids) and np.array_equal(np.sort(before[begin[0]:begin[0] + length[0]]), np.sort(ids))
    e.lookup(ws, 1)
    after = read_lists(ws, 1)[2]
    gid = e.row_gid()
    seg = slice(int(begin[0]), int(begin[0] + length[0]))
    assert np.all(after[seg] >= e.halo_base) and np.array_equal(gid[after[seg]], before[seg])


def test_probe_run_wraps_around_the_table_end(P, homes):
    ids, home = homes
    pick = np.concatenate([ids[home == h][:10] for h in range(1014, 1024)])          # 100 ids homed in the last 10 slots
    e = probe_engine(P, [pick])
    e.collect([0])
    assert e.flags() == 0
    assert len(e.check(pick)) == 100
    keys = e.state()[2]
    assert np.all(keys[1014:] != EMPTY) and np.all(keys[:90] != EMPTY) and np.all(keys[90:1014] == EMPTY), "the run wrapped to slot 0"
    lookup_all_found(P, e, 0, pick)
    assert e.flags() == 0


def test_probe_bound_and_sticky_table_full_bit(P, homes):
    """HALO_MAX_PROBE ids with one home slot all fit (bit 1 clear) and are found; one more reports the table full (bit 1) -
    promptly.  Bit 1 is sticky and halo_collect_kernel stops walking while it is set: a HEALTHY window collected before the
    caller cleared it collects nothing (pcgnn.h says so at counts[128]); after clearing it the same window is whole."""
    ids, home = homes
    same = ids[home == 700]
    healthy = ids[home == 3][:20]
    e = probe_engine(P, [same[:H.HALO_MAX_PROBE], same[:H.HALO_MAX_PROBE + 1], healthy])
    e.collect([0])
    assert e.flags() == 0
    assert len(e.check(same[:128])) == 128
    lookup_all_found(P, e, 0, same[:128])
    assert e.flags() == 0
    t0 = time.perf_counter()
    e.collect([1])
    assert time.perf_counter() - t0 < 5.0
    assert e.flags() & 1, "129 ids with one home slot: a capacity report"
    # bit 1 still set: the healthy window collects nothing
    e.collect([2])
    uniq, counts, keys, _ = e.state()
    assert e.flags() & 1
    assert np.all(uniq == -1) and np.all(counts[:128] == 0) and np.all(keys == EMPTY)
    e.clear_flags()
    e.collect([2])
    assert e.flags() == 0 and len(e.check(healthy)) == 20


# ---------------------------------------------------------------------------------------------------------------------------
# serve
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feat", [10, 25, 32, 64, 100, 166, 400, 512])
def test_serve_rows_bit_for_bit(P, feat):
    from pcgnn_amd import _lib, ops
    lib = _lib.load()
    rs = np.random.RandomState(feat)
    n_local, lo = 301, 1000
    X = rs.randn(n_local, feat).astype(np.float32)
    ip = np.zeros(n_local + 1, dtype=np.int64)
    g = P.DeviceGraph(X, [(ip, np.zeros(0, np.int32))], [], dev(), id_space=5000)
    stride = g.feat_stride
    assert stride == (feat + 3) // 4 * 4
    Xp = g.X.cpu().numpy()
    lpr = 8
    while lpr < stride // 4 and lpr < 64:
        lpr *= 2
    step = 4 * (64 // lpr)                               # ids one workgroup takes per pass
    for out_stride in (stride, stride + 8):
        for n_req in (0, 1, 3 * step - 1, 3 * step, 3 * step + 1):
            req = rs.randint(lo, lo + n_local, size=max(n_req, 1)).astype(np.int32)
            special = [-1, lo - 1, lo + n_local, 0, 4999, lo, lo + n_local - 1]     # unused, owned by someone else (x4), first, last
            at = rs.permutation(max(n_req, 1))[:len(special)]
            req[at] = special[:at.size]
            if n_req >= 2:
                req[n_req - 1], req[0] = lo + n_local - 1, lo
            elif n_req == 1:
                req[0] = lo + 5
            rows = max(n_req, 1) + 2
            out = torch.full((rows, out_stride), -123.5, dtype=torch.float32, device=dev())
            _lib.check(lib.pcg_halo_serve(g.desc_ref(), ops._p(_dt(req)), n_req, lo, n_local, ops._p(out), out_stride, ops._stream(dev())),
                       "pcg_halo_serve")
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            want = np.full((rows, out_stride), -123.5, np.float32)
            for i in range(n_req):
                if lo <= req[i] < lo + n_local:
                    want[i, :stride] = Xp[req[i] - lo]               # the whole padded row; columns beyond it keep the sentinel
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (feat, out_stride, n_req)


# ---------------------------------------------------------------------------------------------------------------------------
# look-up and translating gather on real lists
# ---------------------------------------------------------------------------------------------------------------------------
HUB_DEGS = [1, 64, 65, 127, 128, 129, 300, 2, 254, 256, 258, 600, 130, 4]   # threshold 1.0 keeps deg; 0.5 keeps 127 128 129 300 65 2 of the last six
N_NODES = 3000
BOUNDS3 = [0, 1100, 2050, N_NODES]


class Whole:
    """a whole graph (two relations with the same degrees), its scores, and one simulated rank of a world of 3"""

    def __init__(self, P, feat, rank=1):
        ops = P.ops
        self.P, self.feat, self.rank = P, feat, rank
        rs = np.random.RandomState(40 + feat)
        X, labels, csrs = synth_graph(7 + feat, N_NODES, feat, (5.0, 7.0), 0.1, hub=False)
        lo, hi = BOUNDS3[rank], BOUNDS3[rank + 1]
        self.lo, self.hi = lo, hi
        out = []
        for ip, ix in csrs:
            rows = [ix[ip[v]:ip[v + 1]] for v in range(N_NODES)]
            for i, d in enumerate(HUB_DEGS):
                rows[lo + i] = np.sort(rs.choice(N_NODES, size=d, replace=False))
                assert len(rows[lo + i]) == d
            out.append(rows_to_csr(rows))
        self.csr = out
        labels = labels.copy()
        labels[lo:lo + len(HUB_DEGS):2] = 1                       # positive hub centres take minority picks in training
        self.labels = labels
        self.train_pos = rs.permutation(np.flatnonzero(labels == 1))[:150].tolist()
        self.X = X
        self.G = P.DeviceGraph(X, out, self.train_pos, dev())
        gen = torch.Generator().manual_seed(3)
        self.s0 = ops.score_table(self.G, torch.randn(2, feat, generator=gen).to(dev()), torch.randn(2, generator=gen).to(dev()))
        self.csr_rows = [(ip[lo:hi + 1] - ip[lo], ix[ip[lo]:ip[hi]]) for ip, ix in out]

    def engine(self, window_centres, halo_cap=None):
        want = H.remote_set(self.csr_rows, window_centres, self.lo, self.hi, self.hi - self.lo, self.train_pos)
        per = np.bincount(H.owners(BOUNDS3, want), minlength=3)
        pitch = int(per.max()) + 1
        e = Engine(self.P, self.csr_rows, self.lo, self.hi, BOUNDS3, self.rank, self.train_pos, N_NODES, 2 * pitch, pitch,
                   X_local=self.X[self.lo:self.hi], feat=self.feat)
        e.g.X[e.n_local:e.n_local + e.P] = self.G.X[torch.as_tensor(np.asarray(self.train_pos, dtype=np.int64), device=dev())]
        e.collect(window_centres)
        assert e.flags() == 0
        e.slot_of = e.check(want)
        e.fill_halo(self.G.X)
        e.keys = self.P.ops.pos_sort(e.g, self.s0)
        return e

    def batch(self, B, seed):
        rs = np.random.RandomState(seed)
        n_local = self.hi - self.lo
        if B == 1:
            return np.array([6])                                   # the 300-neighbour row
        ids = np.concatenate([np.arange(len(HUB_DEGS)), rs.randint(0, n_local, size=B - len(HUB_DEGS))])
        ids[-1] = ids[0]
        ids[-2] = 11                                               # duplicates in the batch
        return ids


@pytest.fixture(scope="module")
def whole32(P):
    return Whole(P, 32)


def check_lookup(w, e, ids, train, window_has_all=True):
    ops = w.P.ops
    B = len(ids)
    labels = w.labels[ids + w.lo] if train else None
    fetched = next(iter(e.slot_of))                                # a fetched id: what a stray translation outside the rows would change
    ws, cnt = select_lists(ops, e.g, ids, labels, w.s0, e.keys, [1.0, 0.5], 0.5, train, w.lo, fill=fetched)
    rows = 2 * B
    begin, length, before = read_lists(ws, rows)
    e.clear_flags()
    e.lookup(ws, B)
    after = read_lists(ws, rows)[2]
    used = in_use_mask(begin, length, before.size)
    assert used.sum() == length.sum() and (~used).sum() >= 77
    assert np.array_equal(after[~used], before[~used]), "entries outside every row's [begin, begin + len) are left alone"
    assert np.all(before[~used] == fetched)
    old, new = before[used].astype(np.int64), after[used].astype(np.int64)
    want = np.array([H.translate(i, w.lo, w.hi, e.n_local, e.pos_ids_host, e.pos_idx_host, e.slot_of) for i in old.tolist()])
    assert np.array_equal(new, want)
    hole = old < 0
    assert np.array_equal(new[hole], old[hole]), "a hole stays a hole"
    gid = e.row_gid()
    found = ~hole & (want != H.MISS)
    assert np.all(new[found] < gid.size) and np.array_equal(gid[new[found]], old[found]), "row_gid[new] == old"
    missed = ~hole & (want == H.MISS)
    assert bool(e.flags() & 4) == bool(missed.any()) and (e.flags() & ~4) == 0
    assert bool(missed.any()) != window_has_all
    return length, hole, old, missed


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("B", [1, 17, 300])
def test_lookup_on_real_lists(P, whole32, B, train):
    w = whole32
    ids = w.batch(B, B)
    e = w.engine(ids)
    length, hole, old, _ = check_lookup(w, e, ids, train)
    if B >= 17:
        assert {1, 64, 65, 127, 128, 129, 300} <= set(length.tolist())
        if not train:
            assert set(length[:14].tolist()) == set(HUB_DEGS) and {127, 128, 129, 300, 65, 2} <= set(length[B:B + 14].tolist())
    if train and B >= 17:
        assert hole.any(), "training adds minority picks, duplicates of kept neighbours leave -1 holes"
        assert np.isin(old[~hole], np.asarray(w.train_pos)).any()


def test_lookup_outside_the_window(P, whole32):
    """a window that leaves out one centre's neighbours: those entries become -1 and bit 4 is set, the rest as usual"""
    w = whole32
    ids = w.batch(17, 17)
    e = w.engine(ids[ids != 11])                                   # the 600-neighbour centre is not part of the window
    _, _, _, missed = check_lookup(w, e, ids, False, window_has_all=False)
    assert missed.sum() > 100
    e.clear_flags()


def gather_dist(e, ws, cnt, B, snap=None, theta=None, m=None, v=None, off=0, n=0, status=None):
    ops, g = e.ops, e.g
    _p = ops._p
    agg = torch.full((g.R * B, g.feat_dim), 7.0, dtype=torch.float32, device=dev())
    e._lib.check(e.lib.pcg_gather_lists_dist(
        _p(g.X), g.feat_dim, g.X.stride(0), g.X.shape[0], g.R * B, _p(cnt), g.desc_ref(), B, _p(ws.buf), None, ws.list_capacity, _p(agg),
        agg.stride(0), _p(status if status is not None else ws.status), e.lo, e.hi, e.n_local, _p(e.pos_ids), _p(e.pos_idx), e.P, _p(e.table),
        e.slots, _p(e.counts), e.halo_cap, e.halo_base, _p(theta), _p(m), _p(v), off, n, _p(snap), ops._stream(dev())), "pcg_gather_lists_dist")
    torch.cuda.synchronize()
    return agg


def clone_ws(ops, g, ws, B):
    ws2 = ops.ChooseWorkspace(g, B, list_capacity=ws.list_capacity)
    ws2.buf.copy_(ws.buf)
    return ws2


def reference_means(w, e, begin, length, lst, cnt):
    """mean_f64 and its bound per list row from the WHOLE graph's feature rows (float64), skipping holes and missed ids"""
    X64 = w.X.astype(np.float64)
    means, bounds, n_found = [], [], []
    for row in range(len(length)):
        ids = lst[begin[row]:begin[row] + length[row]].astype(np.int64)
        ids = ids[ids >= 0]
        ok = np.array([H.translate(i, w.lo, w.hi, e.n_local, e.pos_ids_host, e.pos_idx_host, e.slot_of) != H.MISS for i in ids.tolist()],
                      dtype=bool) if ids.size else np.zeros(0, bool)
        rows = X64[ids[ok]]
        c = int(cnt[row])
        means.append(H.mean_f64(rows.reshape(-1, w.feat), c) if c else np.zeros(w.feat))
        bounds.append(H.mean_bound(rows.reshape(-1, w.feat), c) if c else np.zeros(w.feat))
        n_found.append(int(ok.sum()))
    return np.stack(means), np.stack(bounds), np.array(n_found)


@pytest.mark.parametrize("feat", [25, 64, 400])
def test_translating_gather(P, feat):
    """pcg_gather_lists_dist on the untranslated lists == pcg_halo_lookup + pcg_gather_lists_planned on a copy, bit for bit
    (agg of single-chunk rows, the partial sums of the others); pcg_halo_lookup + pcg_aggregate_lists_planned against the
    float64 mean of the whole graph's rows within (cnt + 1) 2^-24 sum|x| / cnt per element.
    Measured on an MI355X (the same with and without the missed id): worst error / bound 0.38 (F 25), 0.45 (F 64), 0.47 (F 400);
    worst absolute error 1.29e-7, 1.43e-7, 1.49e-7 = 0.0065, 0.0072, 0.0075 x FEAT_TOL (2e-5) of tests/test_gpu_parity.py."""
    from pcgnn_amd import _lib
    lib, ops = _lib.load(), P.ops
    w = Whole(P, feat)
    B = 40
    ids = w.batch(B, 5)
    labels = w.labels[ids + w.lo]
    rows = 2 * B
    for miss in (False, True):
        e = w.engine(ids[ids != 11] if miss else ids)
        ws, cnt = select_lists(ops, e.g, ids, labels, w.s0, e.keys, [1.0, 0.5], 0.5, True, w.lo)
        begin, length, lst = read_lists(ws, rows)
        ws2, ws3 = clone_ws(ops, e.g, ws, B), clone_ws(ops, e.g, ws, B)
        e.clear_flags()
        agg1 = gather_dist(e, ws, cnt, B)
        assert int(ws.status.item()) == 0, "*status is unchanged"
        assert bool(e.flags() & 4) == miss and (e.flags() & ~4) == 0
        assert np.array_equal(read_lists(ws, rows)[2], lst), "the translating gather leaves the list as it is"
        e.clear_flags()
        e.lookup(ws2, B)
        assert bool(e.flags() & 4) == miss
        agg2 = torch.full_like(agg1, 7.0)
        _p = ops._p
        _lib.check(lib.pcg_gather_lists_planned(_p(e.g.X), e.g.feat_dim, e.g.X.stride(0), e.g.X.shape[0], rows, _p(cnt), e.g.desc_ref(), B,
                                                _p(ws2.buf), None, ws2.list_capacity, _p(agg2), agg2.stride(0), _p(ws2.status),
                                                ops._stream(dev())), "pcg_gather_lists_planned")
        torch.cuda.synchronize()
        assert int(ws2.status.item()) == 0
        nch = np.diff(ws.view(3, torch.int32, rows + 1).cpu().numpy())
        single = torch.from_numpy(nch == 1).to(dev())
        assert 0 < int(single.sum()) < rows and nch.max() >= 3
        assert torch.equal(agg1[single].view(torch.int32), agg2[single].view(torch.int32))
        chunk_cap = ws.list_capacity // 128 + rows + 1
        part1 = ws.view(6, torch.int32, chunk_cap * e.g.feat_stride)
        part2 = ws2.view(6, torch.int32, chunk_cap * e.g.feat_stride)
        assert int((part1 != 0).sum()) > 0 and torch.equal(part1, part2)
        # finished means against float64
        e.lookup(ws3, B)
        agg3 = torch.full_like(agg1, 7.0)
        _lib.check(lib.pcg_aggregate_lists_planned(_p(e.g.X), e.g.feat_dim, e.g.X.stride(0), e.g.X.shape[0], rows, _p(cnt), e.g.desc_ref(), B,
                                                   _p(ws3.buf), None, ws3.list_capacity, _lib.PCG_NORM_COUNT, _p(agg3), agg3.stride(0),
                                                   _p(ws3.status), ops._stream(dev())), "pcg_aggregate_lists_planned")
        torch.cuda.synchronize()
        e.clear_flags()
        cnt_h = cnt.cpu().numpy()
        mean, bound, n_found = reference_means(w, e, begin, length, lst, cnt_h)
        assert cnt_h.min() >= 1 and cnt_h.max() >= 300
        if miss:
            assert (n_found < cnt_h).any(), "a row lost ids and keeps its count as the divisor"
        else:
            assert np.array_equal(n_found, cnt_h)
        # a wrong row of a unit-variance table moves an element by about 1 / cnt: ten times the bound, for every row compared
        assert np.all(1.0 / cnt_h >= 10.0 * bound.max(axis=1))
        err = np.abs(agg3.cpu().numpy().astype(np.float64) - mean)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"feat {feat} miss {miss}: worst |err| {err.max():.3e} = {err.max() / FEAT_TOL:.4f} x FEAT_TOL; worst err / bound {worst:.4f}")
        assert np.all(err <= bound)
        # single-chunk rows of the translating gather are finished means too
        err1 = np.abs(agg1.cpu().numpy().astype(np.float64) - mean)[nch == 1]
        assert np.all(err1 <= bound[nch == 1])


@pytest.mark.parametrize("feat", [10, 400])
def test_gather_dist_snapshot(P, feat):
    """snap_dst: theta / m / v [clf_offset, clf_offset + clf_n) copied exactly (3 * clf_n below and above one workgroup's 256
    threads); snap_dst == NULL: nothing is written"""
    ops = P.ops
    w = Whole(P, feat)
    ids = np.array([0, 3, 9])
    e = w.engine(ids)
    ws, cnt = select_lists(ops, e.g, ids, None, w.s0, None, [1.0, 0.5], 0.5, False, w.lo)
    n, off = 2 * feat + 2, 5
    assert (3 * n < 256) == (feat == 10)
    theta, m, v = (torch.arange(off + n + 9, dtype=torch.float32, device=dev()) * k + k for k in (1.0, -0.5, 0.25))
    snap = torch.full((3 * n + 8,), -9.0, dtype=torch.float32, device=dev())
    gather_dist(e, ws, cnt, 3, snap=snap, theta=theta, m=m, v=v, off=off, n=n)
    want = torch.cat([theta[off:off + n], m[off:off + n], v[off:off + n], torch.full((8,), -9.0, device=dev())])
    assert torch.equal(snap, want)
    snap.fill_(-9.0)
    gather_dist(e, ws, cnt, 3, snap=None, theta=theta, m=m, v=v, off=off, n=n)
    assert bool((snap == -9.0).all()) and e.flags() == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the whole exchange, every rank simulated in one process
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3, 8])
def test_whole_exchange_in_one_process(P, world):
    """collect on every rank -> the request slices copied as the equal-split all-to-all lays them out -> serve on every owner ->
    the rows copied back into the halo regions -> per rank select + look-up + aggregate == ops.choose_aggregate on the whole
    graph for the same global ids, bit for bit (cnt and agg)."""
    from pcgnn_amd import _lib
    from pcgnn_amd.dist import HaloExchangeHip, Partition, total_degree
    lib, ops = _lib.load(), P.ops
    n, F, B = 4001, 32, 64
    X, labels, csr = synth_graph(77, n, F, (4.0, 6.0, 9.0), 0.1, hub=False)
    train_pos = np.flatnonzero(labels == 1)[::2][:180].tolist()
    G = P.DeviceGraph(X, csr, train_pos, dev())
    gen = torch.Generator().manual_seed(9)
    s0 = ops.score_table(G, torch.randn(2, F, generator=gen).to(dev()), torch.randn(2, generator=gen).to(dev()))
    keys_G = ops.pos_sort(G, s0)
    thr, rho = [0.5, 0.5, 0.7], 0.5
    parts = [Partition.balanced(total_degree(csr), world, r) for r in range(world)]
    bounds = parts[0].bounds_host
    rs = np.random.RandomState(world)
    shards, batches, need = [], [], 0
    for part in parts:
        rows = [(ip[part.lo:part.hi + 1] - ip[part.lo], ix[ip[part.lo]:ip[part.hi]]) for ip, ix in csr]
        ids = rs.randint(0, part.n_local, size=B)
        ids[B // 2:B // 2 + 6] = ids[:6]                           # duplicates in the batch
        want = H.remote_set(rows, ids, part.lo, part.hi, part.n_local, train_pos)
        need = max(need, int(np.bincount(H.owners(bounds, want), minlength=world).max()))
        shards.append(rows)
        batches.append(ids)
    pitch = max(need, 1)                                           # just large enough for the fullest owner range of any rank
    peers = world - 1
    Ptp = len(train_pos)
    ranks = []
    for part, rows in zip(parts, shards):
        n_ext = part.n_local + Ptp + peers * pitch
        X_ext = np.zeros((n_ext, F), np.float32)
        X_ext[:part.n_local] = X[part.lo:part.hi]
        X_ext[part.n_local:part.n_local + Ptp] = X[np.asarray(train_pos)]
        g = P.DeviceGraph(X_ext, ext_csr(rows, n_ext), train_pos, dev(), id_space=n)
        hx = HaloExchangeHip(part, g.X, train_pos, pitch, group=None)
        ranks.append((part, g, hx))
    for (part, g, hx), ids in zip(ranks, batches):
        hx.collect(g, _dt(ids))
    torch.cuda.synchronize()
    for r, (part, g, hx) in enumerate(ranks):
        assert int(hx.counts[128].item()) == 0
        u, c = hx.req_out.cpu().numpy(), _u32(hx.counts)
        t = _u32(hx.table)
        want = H.remote_set(shards[r], batches[r], part.lo, part.hi, part.n_local, train_pos)
        H.check_collect(u, c, t[:hx.slots], t[hx.slots:], want, bounds, pitch, hx.halo_cap, world, r)
    assert max(int(_u32(hx.counts)[130]) for _, _, hx in ranks) == pitch, "some owner range is exactly full"
    # all-to-all #1: rank r's slice for owner o -> owner o's slice from rank r
    sl = lambda me, other: slice((other - (other > me)) * pitch, (other - (other > me) + 1) * pitch)
    for r, (_, _, hx) in enumerate(ranks):
        for o, (_, _, ho) in enumerate(ranks):
            if o != r:
                ho.req_in[sl(o, r)] = hx.req_out[sl(r, o)]
    for _, g, hx in ranks:
        hx.rows_out.fill_(float("nan"))
        hx.serve(g)
    # all-to-all #2: the rows come back in the request list's layout
    for r, (_, _, hx) in enumerate(ranks):
        for o, (_, _, ho) in enumerate(ranks):
            if o != r:
                hx.halo_rows[sl(r, o)] = ho.rows_out[sl(o, r)]
    torch.cuda.synchronize()
    for (part, g, hx), ids in zip(ranks, batches):
        lab = labels[ids + part.lo]
        ws, cnt = select_lists(ops, g, ids, lab, s0, ops.pos_sort(g, s0), thr, rho, True, part.lo, slack=0)
        hx.lookup(ws.buf, None, ws.list_capacity, B, g)
        agg = torch.empty(3, B, F, dtype=torch.float32, device=dev())
        _p = ops._p
        _lib.check(lib.pcg_aggregate_lists_planned(_p(g.X), F, g.X.stride(0), g.X.shape[0], 3 * B, _p(cnt), g.desc_ref(), B, _p(ws.buf), None,
                                                   ws.list_capacity, _lib.PCG_NORM_COUNT, _p(agg), agg.stride(1), _p(ws.status),
                                                   ops._stream(dev())), "pcg_aggregate_lists_planned")
        torch.cuda.synchronize()
        assert int(hx.counts[128].item()) == 0 and int(ws.status.item()) == 0
        gids = _dt(ids + part.lo)
        agg_G, cnt_G = ops.choose_aggregate(G, gids, _dt(lab), s0, keys_G, thr, rho, True)
        torch.cuda.synchronize()
        assert torch.equal(cnt.view(3, B), cnt_G)
        assert torch.equal(agg.view(torch.int32), agg_G.view(torch.int32)), f"rank {part.rank} of {world}"
