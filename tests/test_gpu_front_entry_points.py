"""The layer under the selection tests: class-0 scores, train-pos keys formed from feature rows, and the centres' own scores,
through the entry points of include/pcgnn.h that no other GPU test calls (pcg_step_front_a with row_ids, pcg_step_front_b with
center_s0_out / center_id_offset / raw_keys_ready = 0, pcg_step_scores with row_ids and pos_row_base) - tests/front_ref.py is
the host side, tests/test_front_ref_host.py shows what the bounds below can and cannot miss.

Scores: 16 widths on both sides of every lanes-per-row tier (ragged and full last float4), table sizes round a workgroup's rows
per iteration (1, rb - 1, rb, rb + 1, 1000) and one table of 32768 + 33 rows of 260 floats (a second grid-stride turn at 64 lanes
per row).  pcg_score_table and both columns of pcg_score_rows against a float64 X @ W + b: per call
e = max|x - x64| / max|x64| <= 8 * e_f32 + 2^-20 (dense_ref.tolerance; e_f32 the sequential float32 dot on the CPU).  Then bit
for bit against pcg_score_table: pcg_score_rows' column 0 on shuffled ids with duplicates, sub-ranges (sentinels outside them
kept), pcg_step_front_a with a batch, pcg_step_front_a and pcg_step_scores with row_ids (a permutation into a longer s0 with a
tenth of the rows skipped).

Raw keys (one width per tier; train_pos shuffled, n_pos on both sides of the key group's grid-stride turn; rows copied onto
others so that positions break ties): the unsorted keys pcg_step_front_a, pcg_step_scores_train and pcg_step_scores (train
positives by node id and as a block of the table) leave in the scratch half equal the host key of the device's own s0, and
pcg_step_front_b's sorted half - from those raw keys and from s0 - is pcg_pos_sort's.

Centres: pcg_step_front_b's center_s0_out with offsets 0 and 37 at B = 1, 1023, 1024, 1025, and the plan _a + _b leave.

Measured on an MI355X (python3 -m pytest tests/test_gpu_front_entry_points.py -m gpu -s; the RATIO lines, maximised over a
width's table sizes; of bound = e / (8 * e_f32 + 2^-20), ratio = e / e_f32 where e_f32 >= 2^-24):
    F     pcg_score_table          pcg_score_rows (both columns)
          ratio   of bound         ratio   of bound
    1      0.00    0.04             0.00    0.04
    3      0.72    0.04             1.00    0.05
    4      1.35    0.06             1.35    0.06
    5      1.00    0.05             1.00    0.06
    29     0.92    0.06             0.92    0.17
    32     0.61    0.04             0.61    0.04
    33     0.69    0.05             1.00    0.07
    64     0.49    0.04             3.80    0.23
    65     1.00    0.11             3.28    0.22
    128    0.40    0.11             0.51    0.11
    129    0.44    0.04             0.73    0.08
    256    0.45    0.04             0.45    0.04
    257    0.69    0.06             0.69    0.06
    260    0.30    0.03             0.91    0.07
    509    0.28    0.03             0.28    0.03
    512    0.94    0.10             0.94    0.10
    260, 32768 + 33 rows (pcg_score_table whole and second turn alone, pcg_score_rows column 1): ratio 0.18, of bound 0.02
(F = 1: one product and one sum, e_f32 below 2^-24 - no ratio.)  Every comparison that is stated bit for bit was bit-exact.
"""
import numpy as np
import pytest
import torch

from tests import front_ref as R
from tests.util import synth_graph

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def P():
    import pcgnn_amd
    from pcgnn_amd import ops  # noqa: F401  (fails loudly if the .so is missing)
    return pcgnn_amd


@pytest.fixture(scope="module")
def data():
    return R.table()


def self_loop_graph(P, X, train_pos=()):
    n = X.shape[0]
    return P.DeviceGraph(X, [(np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32))], list(train_pos), dev())


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def call(rc, what):
    from pcgnn_amd import _lib
    _lib.check(rc, what)


class Lib:
    """the library and the few things every call needs"""

    def __init__(self, P):
        from pcgnn_amd import _lib
        self.lib, self.ops, self._lib = _lib.load(), P.ops, _lib
        self.p, self.st = P.ops._p, P.ops._stream(dev())

    def score_table(self, g, W, b, lo, hi, out):
        call(self.lib.pcg_score_table(g.desc_ref(), self.p(W), self.p(b), lo, hi, self.p(out), self.st), "pcg_score_table")

    def sync_words(self):
        return torch.zeros(int(self.lib.pcg_sync_words_count()), dtype=torch.int32, device=dev())

    def key_buffer(self, n_pos, fill=0):
        return torch.full((int(self.lib.pcg_pos_sort_capacity(n_pos)),), fill, dtype=torch.int64, device=dev())

    def front_a(self, g, W, b, lo, hi, s0, row_ids, keys, nodes, labels, thr, rho, train, ws):
        t, r = self.ops._host_arrays(g, thr, rho)
        call(self.lib.pcg_step_front_a(g.desc_ref(), self.p(W), self.p(b), lo, hi, self.p(s0), self.p(row_ids), self.p(keys), self.p(nodes),
                                       self.p(labels), nodes.numel(), t, r, 1 if train else 0, 0, self.p(ws.buf), ws.list_capacity,
                                       self.p(ws.status), self.st), "pcg_step_front_a")

    def front_b(self, g, s0, keys, raw_ready, nodes, labels, thr, rho, train, ws, center_out=None, offset=0):
        t, r = self.ops._host_arrays(g, thr, rho)
        call(self.lib.pcg_step_front_b(g.desc_ref(), self.p(s0), self.p(keys), raw_ready, self.p(nodes), self.p(labels), nodes.numel(), t, r,
                                       1 if train else 0, 0, self.p(ws.buf), ws.list_capacity, self.p(ws.status), self.p(center_out),
                                       offset, self.st), "pcg_step_front_b")

    def step_scores(self, g, W, b, lo, hi, s0, row_ids, keys, pos_row_base, sync):
        call(self.lib.pcg_step_scores(g.desc_ref(), self.p(W), self.p(b), lo, hi, self.p(s0), self.p(row_ids), self.p(keys), pos_row_base,
                                      self.p(sync), None, self.st), "pcg_step_scores")


@pytest.fixture(scope="module")
def L(P):
    return Lib(P)


def hold(what, F, n, got, X, w, b, worst):
    e, e32, tol = R.score_check(got, X, w, b)
    print(f"  {what} F={F} n={n}: e {e:.3e}  e_f32 {e32:.3e}  tolerance {tol:.3e}")
    worst[0] = max(worst[0], e / tol)
    if e32 >= 2.0 ** -24:
        worst[1] = max(worst[1], e / e32)
    assert e <= tol, (what, F, n, e, e32, tol)


def row_id_map(n, seed):
    """int32 [n]: a permutation of the rows into n + 100 entries, a tenth of the rows skipped (-1)"""
    rs = np.random.RandomState(seed)
    ids = rs.permutation(n + 100)[:n].astype(np.int32)
    skip = rs.permutation(n)[:n // 10]
    ids[skip] = -1
    return ids


def check_row_ids(s0_out, full, ids_np, what):
    named = ids_np >= 0
    dst = torch.from_numpy(ids_np[named].astype(np.int64)).cuda()
    src = torch.from_numpy(np.flatnonzero(named)).cuda()
    assert same_bits(s0_out[dst], full[src]), f"{what}: every named entry holds its row's bits"
    rest = torch.ones(s0_out.numel(), dtype=torch.bool, device=dev())
    rest[dst] = False
    assert bool((s0_out[rest] == SENTINEL).all()), f"{what}: every other entry keeps its sentinel"
    assert int(rest.sum()) == s0_out.numel() - int(named.sum()) >= 100


# ---- scores --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", R.SCORE_WIDTHS)
def test_scores_against_float64_and_each_other(P, L, data, F):
    W_np, b_np = R.weights(F, 0)
    W, b = torch.from_numpy(W_np).cuda(), torch.from_numpy(b_np).cuda()
    Xh = np.ascontiguousarray(data[:, :F])
    rb, rw = R.rows_per_block(F), R.rows_per_workgroup_launch(F)
    worst_t, worst_r = [0.0, 0.0], [0.0, 0.0]
    for n in R.table_sizes(F):
        g = self_loop_graph(P, Xh[:n])
        full = torch.full((n,), SENTINEL, device=dev())
        L.score_table(g, W, b, 0, n, full)
        # score_rows: shuffled ids with duplicates, a length that is no multiple of a workgroup's rows
        length = (max(n, rw) // rw + 1) * rw + 1            # (a last workgroup with a single row)
        ids_np = R.shuffled_ids(n, length, 100 * F + n)
        assert n == 1 or np.unique(ids_np).size < length
        ids = torch.from_numpy(ids_np).cuda()
        rows = L.ops.score_rows(g, W, b, ids)
        torch.cuda.synchronize()
        hold("pcg_score_table", F, n, full.cpu().numpy(), Xh[:n], W_np[0], b_np[0], worst_t)
        for col in (0, 1):
            hold(f"pcg_score_rows[{col}]", F, n, rows[:, col].cpu().numpy(), Xh[ids_np], W_np[col], b_np[col], worst_r)
        assert same_bits(rows[:, 0], full[ids.long()]), f"F {F} n {n}: pcg_score_rows column 0 is pcg_score_table's bits"
        if n != R.TABLE_ROWS:
            continue
        # sub-ranges: the same bits inside, the sentinel outside
        for lo, hi in ((0, n), (1, n - 1), (n - 1, n), (7, 7 + rb + 1), (5, 5)):
            part = torch.full((n,), SENTINEL, device=dev())
            L.score_table(g, W, b, lo, hi, part)
            assert same_bits(part[lo:hi], full[lo:hi]), (F, lo, hi)
            assert bool((part[:lo] == SENTINEL).all()) and bool((part[hi:] == SENTINEL).all()), (F, lo, hi)
        # the front launch, with a batch (test mode: no keys) and row_ids = NULL
        nodes = torch.from_numpy(R.shuffled_ids(n, 37, F)).cuda()
        ws = L.ops.ChooseWorkspace(g, 37)
        s0 = torch.full((n,), SENTINEL, device=dev())
        L.front_a(g, W, b, 0, n, s0, None, None, nodes, None, [0.5], 0.5, False, ws)
        assert same_bits(s0, full), f"F {F}: pcg_step_front_a's score pass"
        part = torch.full((n,), SENTINEL, device=dev())
        L.front_a(g, W, b, 7, 7 + rb + 1, part, None, None, nodes, None, [0.5], 0.5, False, ws)
        assert same_bits(part[7:8 + rb], full[7:8 + rb]) and bool((part[:7] == SENTINEL).all()) and bool((part[8 + rb:] == SENTINEL).all())
        # ... and with row_ids: into an s0 of n + 100 entries
        ids_map = row_id_map(n, F)
        rid = torch.from_numpy(ids_map).cuda()
        out = torch.full((n + 100,), SENTINEL, device=dev())
        L.front_a(g, W, b, 0, n, out, rid, None, nodes, None, [0.5], 0.5, False, ws)
        check_row_ids(out, full, ids_map, f"F {F} pcg_step_front_a(row_ids)")
        out = torch.full((n + 100,), SENTINEL, device=dev())
        sync = L.sync_words()
        sync[3] = 77
        L.step_scores(g, W, b, 0, n, out, rid, None, -1, sync)
        check_row_ids(out, full, ids_map, f"F {F} pcg_step_scores(row_ids)")
        assert int(sync[3].item()) == 0, "the launch zeroes sync_words[3]"
        ws.check()
    print(f"RATIO pcg_score_table F={F}: ratio {worst_t[1]:.2f}  of bound {worst_t[0]:.2f}")
    print(f"RATIO pcg_score_rows  F={F}: ratio {worst_r[1]:.2f}  of bound {worst_r[0]:.2f}")


def test_scores_second_grid_stride_turn(P, L):
    """32768 + 33 rows of 260 floats (34 MB): pcg_score_table's grid is capped at 1024 workgroups of 32 rows per iteration at 64
    lanes per row, so the last 33 rows - a whole iteration of the first workgroup and one row of the second - are scored in a
    second turn of the grid-stride loop"""
    F, n = R.SECOND_TURN
    Xh = R.table(seed=29, rows=n, width=F)
    W_np, b_np = R.weights(F, 2)
    W, b = torch.from_numpy(W_np).cuda(), torch.from_numpy(b_np).cuda()
    g = self_loop_graph(P, Xh)
    full = torch.full((n,), SENTINEL, device=dev())
    L.score_table(g, W, b, 0, n, full)
    worst = [0.0, 0.0]
    torch.cuda.synchronize()
    got = full.cpu().numpy()
    hold("pcg_score_table", F, n, got, Xh, W_np[0], b_np[0], worst)
    hold("pcg_score_table (second turn only)", F, 33, got[32768:], Xh[32768:], W_np[0], b_np[0], worst)
    ids_np = np.concatenate([np.arange(32768 - 3, n), R.shuffled_ids(n, 1000, 5)]).astype(np.int32)
    ids = torch.from_numpy(ids_np).cuda()
    rows = L.ops.score_rows(g, W, b, ids)
    assert same_bits(rows[:, 0], full[ids.long()])
    hold("pcg_score_rows[1]", F, n, rows[:, 1].cpu().numpy(), Xh[ids_np], W_np[1], b_np[1], worst)
    s0 = torch.full((n,), SENTINEL, device=dev())
    L.step_scores(g, W, b, 0, n, s0, None, None, -1, L.sync_words())
    assert same_bits(s0, full), "the front launch's score pass: the same grid, the same second turn"
    print(f"RATIO second turn F={F} n={n}: ratio {worst[1]:.2f}  of bound {worst[0]:.2f}")


# ---- raw keys ------------------------------------------------------------------------------------------------------------------
class FrontState:
    """the training state pcg_step_scores_train wants: theta holding the label classifier (W [2, F], b [2]), nothing pending"""

    def __init__(self, L, F, W, b, E=16, Rn=1):
        lib, _lib, _p = L.lib, L._lib, L.p
        n_params = int(lib.pcg_dense_n_params(F, E, Rn))
        self.theta = torch.zeros(n_params, device=dev())
        o_w, o_b = int(lib.pcg_dense_param_offset(F, E, Rn, 3, 0)), int(lib.pcg_dense_param_offset(F, E, Rn, 4, 0))
        self.theta[o_w:o_w + 2 * F] = W.reshape(-1)
        self.theta[o_b:o_b + 2] = b
        self.m, self.v = torch.zeros_like(self.theta), torch.zeros_like(self.theta)
        self.slabs = torch.zeros(4, n_params, device=dev())
        self.step = torch.zeros(1, dtype=torch.int32, device=dev())
        self.sync = L.sync_words()
        self.c = _lib.TrainState(theta=_p(self.theta), m=_p(self.m), v=_p(self.v), step_counter=_p(self.step), sync_words=_p(self.sync),
                                 slabs=_p(self.slabs), emb=E, hyper=_lib.AdamHyper(0.01, 0.9, 0.999, 1e-8, 0.0))


def raw_half(keys, n_pos):
    cap = keys.numel() // 2
    return keys[cap:cap + n_pos].cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("F", R.KEY_WIDTHS)
def test_raw_keys_are_the_keys_of_the_device_scores(P, L, F):
    Xh, n = R.key_table(F)
    W_np, b_np = R.weights(F, 1)
    W, b = torch.from_numpy(W_np).cuda(), torch.from_numpy(b_np).cuda()
    state = FrontState(L, F, W, b)
    nodes = torch.from_numpy(R.shuffled_ids(n, 37, F)).cuda()
    labels = torch.from_numpy((np.arange(37) % 3 == 0).astype(np.int32)).cuda()
    thr, rho = [0.5], 0.5
    ties = 0
    for n_pos in R.n_pos_list(F):
        tp = R.train_pos_list(n, n_pos, n_pos)
        g = self_loop_graph(P, Xh, tp)
        cap = int(L.lib.pcg_pos_sort_capacity(n_pos)) // 2
        assert cap == R.sort_capacity(n_pos)
        full = torch.empty(n, device=dev())
        L.score_table(g, W, b, 0, n, full)
        want_sorted = torch.from_numpy(R.sorted_keys(full.cpu().numpy(), tp, cap).view(np.int64)).cuda()
        ref_sorted = L.ops.pos_sort(g, full)[:cap]
        assert torch.equal(ref_sorted, want_sorted), "pcg_pos_sort: the host keys, sorted, all-ones behind them"
        ties += n_pos - np.unique(full.cpu().numpy()[tp]).size
        ws = L.ops.ChooseWorkspace(g, 37)

        def check(s0, keys, what):
            torch.cuda.synchronize()
            assert same_bits(s0[:n], full), f"{what}: the scores are pcg_score_table's"
            want = R.pos_keys(s0.cpu().numpy(), tp)
            assert np.array_equal(raw_half(keys, n_pos), want), f"F {F} n_pos {n_pos} {what}: raw key i is the key of s0[train_pos[i]]"

        # producer 1: pcg_step_front_a(pos_keys, train_flag = 1, B > 0), then _b sorting from the raw keys and from s0
        s0, keys = torch.full((n,), SENTINEL, device=dev()), L.key_buffer(n_pos, 0x55)
        L.front_a(g, W, b, 0, n, s0, None, keys, nodes, labels, thr, rho, True, ws)
        check(s0, keys, "pcg_step_front_a")
        L.front_b(g, s0, keys, 1, nodes, labels, thr, rho, True, ws)
        assert torch.equal(keys[:cap], ref_sorted), f"F {F} n_pos {n_pos}: pcg_step_front_b(raw_keys_ready = 1) is pcg_pos_sort's, padding included"
        keys2 = L.key_buffer(n_pos, 0x33)                 # (no raw keys in this buffer: the sort gathers the scores itself)
        L.front_b(g, s0, keys2, 0, nodes, labels, thr, rho, True, ws)
        assert torch.equal(keys2[:cap], ref_sorted), f"F {F} n_pos {n_pos}: pcg_step_front_b(raw_keys_ready = 0)"
        ws.check()
        # producer 2: pcg_step_scores_train
        s0, keys = torch.full((n,), SENTINEL, device=dev()), L.key_buffer(n_pos, 0x55)
        call(L.lib.pcg_step_scores_train(g.desc_ref(), state.c, L.p(s0), L.p(keys), None, L.st), "pcg_step_scores_train")
        check(s0, keys, "pcg_step_scores_train")
        # producer 3: pcg_step_scores, train positives by node id ...
        s0, keys = torch.full((n,), SENTINEL, device=dev()), L.key_buffer(n_pos, 0x55)
        L.step_scores(g, W, b, 0, n, s0, None, keys, -1, L.sync_words())
        check(s0, keys, "pcg_step_scores(pos_row_base = -1)")
        # ... and as a block of the table of their own, in train_pos order, behind the rows
        g2 = self_loop_graph(P, np.concatenate([Xh, Xh[tp]]), tp)
        s0, keys = torch.full((n + n_pos,), SENTINEL, device=dev()), L.key_buffer(n_pos, 0x55)
        L.step_scores(g2, W, b, 0, n + n_pos, s0, None, keys, n, L.sync_words())
        check(s0, keys, "pcg_step_scores(pos_row_base = n)")
        assert same_bits(s0[n:], full[torch.from_numpy(tp).cuda()]), "the block's rows score as the rows they copy"
        # (the keys come from the BLOCK's rows: a table whose block differs from the rows by node id gives the block's keys)
        if n_pos == R.n_pos_list(F)[-1]:
            Xb = np.concatenate([Xh, Xh[tp][::-1]])
            g3 = self_loop_graph(P, Xb, tp)
            s0, keys = torch.full((n + n_pos,), SENTINEL, device=dev()), L.key_buffer(n_pos, 0x55)
            L.step_scores(g3, W, b, 0, n + n_pos, s0, None, keys, n, L.sync_words())
            torch.cuda.synchronize()
            block = s0[n:].cpu().numpy()
            want = (R.orderable(block).astype(np.uint64) << np.uint64(32)) | np.arange(n_pos, dtype=np.uint64)
            assert np.array_equal(raw_half(keys, n_pos), want)
    assert ties > 0, "equal scores among the train positives: the position decides"
    assert int(state.step.item()) == 0 and not bool(state.m.any()), "no update was pending: the state is as it was"


# ---- centres -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def centre_case(P):
    n, F = 3000, 32
    X, labels, csrs = synth_graph(61, n, F, (12,), 0.15)
    train_pos = np.flatnonzero(labels == 1)[:300]
    g = P.DeviceGraph(X, csrs, train_pos.tolist(), dev())
    W_np, b_np = R.weights(F, 3)
    return g, labels, torch.from_numpy(W_np).cuda(), torch.from_numpy(b_np).cuda()


@pytest.mark.parametrize("B", [1, 1023, 1024, 1025])
def test_front_b_centre_scores_and_plan(P, L, centre_case, B):
    """PLAN_THREADS = 1024 centres per workgroup of front_b's first group: one, a full one less one, a full one, one more"""
    g, labels, W, b = centre_case
    n, ops = g.n_nodes, L.ops
    rs = np.random.RandomState(B)
    nodes_np = rs.randint(0, n, size=B).astype(np.int32)
    nodes_np[0] = 7                                        # (synth_graph's hub)
    nodes = torch.from_numpy(nodes_np).cuda()
    lab = torch.from_numpy(labels[nodes_np].astype(np.int32)).cuda()
    thr, rho = [0.5], [0.5]
    # separate calls
    s0_a = ops.score_table(g, W, b)
    keys_a = ops.pos_sort(g, s0_a)
    ws_a = ops.ChooseWorkspace(g, B)
    agg_a, cnt_a = ops.choose_aggregate(g, nodes, lab, s0_a, keys_a, thr, rho, True, ws=ws_a)
    # _a + _b, the centres' scores written on the way (offset 0)
    ws_b = ops.ChooseWorkspace(g, B)
    s0_b, keys_b = torch.full((n,), SENTINEL, device=dev()), L.key_buffer(g.n_pos)
    centre = torch.full((B + 64,), SENTINEL, device=dev())
    L.front_a(g, W, b, 0, n, s0_b, None, keys_b, nodes, lab, thr, rho, True, ws_b)
    L.front_b(g, s0_b, keys_b, 1, nodes, lab, thr, rho, True, ws_b, centre, 0)
    agg_b, cnt_b = ops.choose_aggregate(g, nodes, lab, s0_b, keys_b, thr, rho, True, ws=ws_b, planned=True)
    torch.cuda.synchronize()
    ws_a.check(); ws_b.check()
    assert same_bits(s0_a, s0_b)
    assert same_bits(centre[:B], s0_a[nodes.long()]) and bool((centre[B:] == SENTINEL).all()), "offset 0"
    half = keys_a.numel() // 2
    assert torch.equal(keys_a[:half], keys_b[:half])
    assert torch.equal(cnt_a, cnt_b) and same_bits(agg_a, agg_b)
    rows = g.R * B
    begin_a, begin_b = ws_a.view(0, torch.int64, rows + 1), ws_b.view(0, torch.int64, rows + 1)
    assert torch.equal(begin_a, begin_b)
    total = int(begin_a[-1])
    assert torch.equal(ws_a.view(1, torch.int32, rows), ws_b.view(1, torch.int32, rows))
    assert torch.equal(ws_a.view(2, torch.int32, total), ws_b.view(2, torch.int32, total))
    # offset 37: s0 is longer by the offset, the centres are read 37 entries on; a test-mode front (no sort)
    s0_long = torch.from_numpy(np.random.RandomState(B + 1).randn(n + 37).astype(np.float32)).cuda()
    centre = torch.full((B + 64,), SENTINEL, device=dev())
    ws_c = ops.ChooseWorkspace(g, B)
    L.front_a(g, W, b, 0, n, s0_b, None, None, nodes, None, thr, rho, False, ws_c)
    L.front_b(g, s0_long, None, 0, nodes, None, thr, rho, False, ws_c, centre, 37)
    torch.cuda.synchronize()
    assert same_bits(centre[:B], s0_long[nodes.long() + 37]) and bool((centre[B:] == SENTINEL).all()), "offset 37"
    assert not same_bits(centre[:B], s0_long[nodes.long()])
    # ... and the plan those two left is the test-mode plan: the planned select + gather equals the unplanned one
    agg_c, cnt_c = ops.choose_aggregate(g, nodes, None, s0_a, None, thr, rho, False, ws=ws_c, planned=True)
    agg_d, cnt_d = ops.choose_aggregate(g, nodes, None, s0_a, None, thr, rho, False, ws=ops.ChooseWorkspace(g, B))
    torch.cuda.synchronize()
    ws_c.check()
    assert torch.equal(cnt_c, cnt_d) and same_bits(agg_c, agg_d)
