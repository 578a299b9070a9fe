"""The touched-rows byte maps, exactly: pcg_mark_touched_planned (csrc/mark.hip: long rows swept id range by id range into LDS
bitmaps, the other rows from the plans' tier queues) and pcg_mark_touched (csrc/score.hip: one byte store per neighbour, hub rows
by the whole grid) against tests/mark_ref.py - the nonzero coordinates of every map, every byte 0 or 1, nothing at or beyond
row n, over a garbage fill, and the two entry points byte for byte.

Graph A (600 000 nodes, map stride 600 576) runs at four batch counts.  With the rule in mark.hip - the widest range of 2^shift
ids, 19 >= shift >= 16, that still gives 256 workgroups -
    128 batches -> shift 19,  2 ranges        100 batches -> shift 18,  3 ranges
     60 batches -> shift 17,  5 ranges         30 batches -> shift 16, 10 ranges
(mark_ref.shift_rule is a copy of the rule: a change of it in mark.hip fails these tests' coverage assert).  Its planted centre
rows sit in every degree tier, cross every 2^16-id boundary, lie wholly inside one range, skip middle ranges, and have stretches
of exactly 1, 256 and 257 ids inside a range; one centre has no neighbour at all in either relation (DeviceGraph accepts a row of
degree 0).  tests/test_mark_ref_host.py checks on the CPU that the graphs contain all that.
Graph B (200 000 nodes) has 1 200 rows of 513 .. 700 neighbours in one batch: three turns of the sweep's 512-row loop."""
import numpy as np
import pytest
import torch

from tests import mark_ref as M

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def P():
    import pcgnn_amd
    from pcgnn_amd import ops  # noqa: F401  (fails loudly if the .so is missing)
    return pcgnn_amd


def planned_maps(P, gg, ids_t, labels_np, n_tot, Bq, stride_q, fill):
    """pcg_plan_batches + pcg_mark_touched_planned over a buffer filled with `fill` (the plan-building helper of
    test_gpu_parity.py::test_touched_rows_only_scoring)"""
    from pcgnn_amd import _lib
    lib, ops = _lib.load(), P.ops
    _p, st = ops._p, ops._stream(dev())
    lab_t = torch.from_numpy(labels_np[ids_t.cpu().numpy()].astype(np.int32)).cuda()
    thr_c, rho_c = ops._host_arrays(gg, [0.5] * gg.R, [0.5] * gg.R)
    cap = int(ops.sel_capacity(gg, ids_t.cpu().numpy(), labels_np[ids_t.cpu().numpy()], [0.5] * gg.R, [0.5] * gg.R, True).sum()) + 64
    pst = int(lib.pcg_choose_plan_bytes(gg.desc_ref(), Bq, cap))
    n_sl = -(-n_tot // Bq)
    plans = torch.zeros(n_sl * pst, dtype=torch.uint8, device=dev())
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    _lib.check(lib.pcg_plan_batches(gg.desc_ref(), _p(ids_t), _p(lab_t), n_tot, Bq, thr_c, rho_c, 1, 0, _p(plans), pst, cap, _p(status),
                                    None, st), "pcg_plan_batches")
    out = torch.full((n_sl * stride_q,), fill, dtype=torch.uint8, device=dev())
    assert bool((out > 1).all()), "the maps start from garbage"
    _lib.check(lib.pcg_mark_touched_planned(gg.desc_ref(), _p(ids_t), n_tot, Bq, _p(plans), pst, cap, _p(out), stride_q, st),
               "pcg_mark_touched_planned")
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    return out


def direct_maps(P, gg, ids_t, n_tot, Bq, stride_q, fill):
    """pcg_mark_touched over a buffer filled with `fill`; returns (maps, rows its hub queue took)"""
    from pcgnn_amd import _lib
    lib, ops = _lib.load(), P.ops
    out = torch.full((-(-n_tot // Bq) * stride_q,), fill, dtype=torch.uint8, device=dev())
    assert bool((out > 1).all()), "the maps start from garbage"
    queue = torch.full((4 + gg.R * n_tot,), -1, dtype=torch.int32, device=dev())
    _lib.check(lib.pcg_mark_touched(gg.desc_ref(), ops._p(ids_t), n_tot, Bq, ops._p(out), stride_q, ops._p(queue), ops._stream(dev())),
               "pcg_mark_touched")
    torch.cuda.synchronize()
    return out, int(queue[0].item())


def assert_exact(maps, n_slots, stride, n, want):
    """maps [n_slots * stride] bytes on the device; want: per batch the sorted ids (mark_ref.touched_ids)"""
    assert maps.numel() == n_slots * stride and len(want) == n_slots
    assert int(maps.max().item()) <= 1, "every byte is 0 or 1"
    m2 = maps.view(n_slots, stride)
    assert not bool(m2[:, n:].any()), "no byte at or beyond row n is set, up to the stride"
    got = torch.nonzero(maps).view(-1).cpu().numpy()
    exp = np.concatenate([s * stride + ids for s, ids in enumerate(want)])
    if not np.array_equal(got, exp):
        missing, extra = np.setdiff1d(exp, got), np.setdiff1d(got, exp)
        raise AssertionError(f"{len(missing)} marks missing, {len(extra)} too many; first (batch, id): "
                             f"missing {[divmod(int(x), stride) for x in missing[:8]]} extra {[divmod(int(x), stride) for x in extra[:8]]}")


@pytest.fixture(scope="module")
def graph_a(P):
    csrs, train_pos, planted, _ = M.graph_a()
    X = np.zeros((M.A_N, 4), dtype=np.float32)
    return P.DeviceGraph(X, csrs, train_pos, dev()), csrs, train_pos, planted


# (batches, shift, id ranges, bytes of map stride beyond the minimum)
CASES_A = [(128, 19, 2, 0), (100, 18, 3, 0), (60, 17, 5, 0), (30, 16, 10, 0), (30, 16, 10, 1040)]


@pytest.mark.parametrize("n_slots,shift,n_ranges,extra", CASES_A)
def test_graph_a_marks_are_exact(P, graph_a, n_slots, shift, n_ranges, extra):
    from pcgnn_amd import _lib
    g, csrs, train_pos, planted = graph_a
    lib = _lib.load()
    stride = int(lib.pcg_touched_bytes(M.A_N)) + extra
    assert stride == 600576 + extra and stride % 16 == 0
    assert M.shift_rule(n_slots, stride) == (shift, n_ranges) and n_ranges > 1, "this case no longer reaches the shift it is here for"
    B, n_total = M.A_B, (n_slots - 1) * M.A_B + M.A_TAIL
    nodes = M.nodes_a(planted, n_slots, B, M.A_TAIL)
    assert len(nodes) == n_total and n_total % B != 0, "a shorter last batch"
    ids = torch.from_numpy(nodes).cuda()
    want = M.touched_ids(csrs, train_pos, nodes, B, M.A_N)
    got_p = planned_maps(P, g, ids, M.labels_a(), n_total, B, stride, 0xA5)
    assert_exact(got_p, n_slots, stride, M.A_N, want)
    got_d, n_hub = direct_maps(P, g, ids, n_total, B, stride, 7)
    assert_exact(got_d, n_slots, stride, M.A_N, want)
    deg0 = np.diff(csrs[0][0])
    assert n_hub == int((deg0[nodes] > 4096).sum()) and n_hub >= 3 * 3, "rows of > 4096 neighbours went through the hub queue"
    assert torch.equal(got_p, got_d), "planned marks == pcg_mark_touched's, byte for byte"


def test_graph_b_more_than_512_long_rows_in_a_batch(P):
    """One batch of 600 centres with 513 .. 700 neighbours in both relations - 1 200 long rows: the sweep locates 512 rows at
    a time, so its row loop takes three turns, the last with 176 rows - and a tail batch of 37 (74 long rows), over 4 id
    ranges of 2^16."""
    from pcgnn_amd import _lib
    lib = _lib.load()
    csrs, train_pos, nodes = M.graph_b()
    g = P.DeviceGraph(np.zeros((M.B_N, 4), dtype=np.float32), csrs, train_pos, dev())
    stride = int(lib.pcg_touched_bytes(M.B_N))
    B, n_total = 600, 637
    assert M.shift_rule(2, stride) == (16, 4)
    assert sum(int((np.diff(ip)[nodes[:B]] > 512).sum()) for ip, _ in csrs) == 1200
    ids = torch.from_numpy(nodes).cuda()
    want = M.touched_ids(csrs, train_pos, nodes, B, M.B_N)
    got_p = planned_maps(P, g, ids, np.zeros(M.B_N, dtype=np.int64), n_total, B, stride, 0x5A)
    assert_exact(got_p, 2, stride, M.B_N, want)
    got_d, n_hub = direct_maps(P, g, ids, n_total, B, stride, 9)
    assert_exact(got_d, 2, stride, M.B_N, want)
    assert n_hub == -1 or n_hub == 0                      # (no row of > 4096 neighbours: the queue is not used, or is left empty)
    assert torch.equal(got_p, got_d), "planned marks == pcg_mark_touched's, byte for byte"
