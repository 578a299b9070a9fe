"""tests/halo_ref.py (the host reference the GPU halo tests compare the HIP kernels with) against the torch class
HaloExchange, which tests/test_dist_cpu.py checks over gloo: same request sets per owner range, same counts, same translated
rows, same overflow bits - for every rank of worlds 1, 2, 3 and 8, equal and in-edge balanced partitions, and partitions with
an empty and a one-node shard.  collect / lookup are called directly: no process group."""
import numpy as np
import pytest
import torch

from tests import halo_ref as H


@pytest.fixture(scope="module")
def W():
    import pcgnn_amd  # noqa: F401
    from pcgnn_amd import synth
    return synth.make_workload("t", 601, 25, (900, 4000), 0.2, seed=3)


def _partitions(w):
    from pcgnn_amd.dist import Partition, total_degree
    deg = total_degree(w.csr)
    out = []
    for world in (1, 2, 3, 8):
        for rank in range(world):
            out.append(("equal", Partition(w.n, world, rank)))
            out.append(("balanced", Partition.balanced(deg, world, rank)))
    for bounds in ([0, 200, 200, 201, 601], [0, 0, 300, 301, 601, 601]):      # empty and one-node shards, also first / last
        for rank in range(len(bounds) - 1):
            out.append(("given", Partition(w.n, len(bounds) - 1, rank, bounds)))
    return out


def _run(w, part, pitch, seed):
    from pcgnn_amd.dist import HaloExchange, shard_workload
    sh = shard_workload(w, part)
    tp = np.asarray(sh["train_pos"], dtype=np.int64)
    P, n_local, world, rank = len(tp), part.n_local, part.world, part.rank
    peers = max(world - 1, 1)
    hx = HaloExchange(part, torch.zeros(n_local + P + peers * pitch, 28), sh["train_pos"], pitch)
    csr_t = [(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64))) for ip, ix in sh["csr"]]
    pos_ids, pos_idx = hx.pos_ids.numpy(), hx.pos_idx.numpy()
    assert np.array_equal(pos_ids, np.sort(tp)) and np.array_equal(tp[pos_idx], pos_ids)
    bounds = part.bounds_host
    rs = np.random.RandomState(seed)
    most_total = most_owner = 0
    bit2 = False
    for n_c in (40, 0, 9):
        centres = rs.randint(0, max(n_local, 1), size=n_c).astype(np.int32) if n_local else np.zeros(n_c, np.int32)
        centres = np.concatenate([centres, centres[:3], np.array([-1, n_local], np.int32)])   # duplicates, outside the shard
        hx.collect(csr_t, torch.from_numpy(centres))
        want = H.remote_set(sh["csr"], centres, part.lo, part.hi, n_local, tp)
        own = H.owners(bounds, want)
        per_owner = np.bincount(own, minlength=world)[:world]
        counts = hx.counts.numpy()
        assert np.array_equal(counts[:world], per_owner)
        most_total, most_owner = max(most_total, int(want.size)), max(most_owner, int(per_owner.max()))
        assert (int(counts[129]), int(counts[130])) == (most_total, most_owner)
        bit2 |= bool((per_owner > pitch).any())
        req = hx.req_out.numpy().astype(np.int64)
        used = np.zeros(req.size, dtype=bool)
        slot_of = {}
        for o, (b, e) in enumerate(H.owner_ranges(world, rank, pitch, per_owner)):
            seg = req[b:e]
            got, mine = seg[seg >= 0], want[own == o]
            if mine.size > pitch:
                assert got.size == pitch and set(got.tolist()) <= set(mine.tolist())
            else:
                assert np.array_equal(np.sort(got), mine), f"owner {o}"
            used[b:e] |= seg >= 0
            slot_of.update({int(seg[i]): b + i for i in np.flatnonzero(seg >= 0).tolist()})
        assert np.all(req[~used] == -1) and len(slot_of) == int((req >= 0).sum())
        # a list of owned ids, train positives (owned and remote), fetched ids, holes and ONE id outside the window
        far = np.setdiff1d(np.arange(w.n), np.concatenate([np.arange(part.lo, part.hi), tp, want]))[:1]
        lst = np.concatenate([np.arange(part.lo, part.hi)[:: max(n_local // 30, 1)], tp[:25], want[::3]]).astype(np.int32)
        rs.shuffle(lst)
        lst[:: 7] = -1
        lst = np.insert(lst, 1, far.astype(np.int32))
        for with_far in (False, True):
            mine = lst.copy() if with_far else lst[lst != (far[0] if far.size else -2)].copy()
            ref = np.array([H.translate(i, part.lo, part.hi, n_local, pos_ids, pos_idx, slot_of) for i in mine.tolist()])
            hx.counts[128] &= ~4
            t = torch.from_numpy(mine.copy())
            hx.lookup(t)
            assert np.array_equal(t.numpy(), ref)
            missed = bool(((ref == H.MISS) & (mine >= 0)).any())
            assert bool(int(hx.counts[128]) & 4) == missed
            if with_far and far.size:
                assert missed
            if not with_far and not bit2:
                assert not missed, "every id of the window is in one of the three"
        assert bool(int(hx.counts[128]) & 2) == bit2
    return bit2


def test_reference_agrees_with_torch_halo_exchange(W):
    for name, part in _partitions(W):
        assert not _run(W, part, pitch=400, seed=part.world * 16 + part.rank), (name, part.world, part.rank)


def test_reference_agrees_with_torch_halo_exchange_over_pitch(W):
    """a pitch too small: the same `exactly pitch ids of that owner get a slot` rule, the same bit 2, the same misses"""
    over = [_run(W, part, pitch=3, seed=part.world * 16 + part.rank) for _, part in _partitions(W) if part.world > 1]
    assert sum(over) > len(over) // 2


def test_owner_handles_empty_shards():
    b = [0, 0, 5, 5, 5, 9, 9]
    assert [H.owner(b, i) for i in (0, 4, 5, 8)] == [1, 1, 4, 4]
    assert H.owner([0, 10], 9) == 0 and H.owner([0, 3, 10], 3) == 1 and H.owner([0, 3, 10], 2) == 0


def test_remote_set_and_translate_by_hand():
    ip = np.array([0, 3, 3, 6], dtype=np.int64)
    ix = np.array([1, 7, 12, 0, 9, 12], dtype=np.int32)
    ip2 = np.array([0, 1, 2, 2], dtype=np.int64)
    ix2 = np.array([20, 21], dtype=np.int32)
    got = H.remote_set([(ip, ix), (ip2, ix2)], [0, 0, 2, -1, 3], 5, 8, 3, [9])
    assert got.tolist() == [0, 1, 12, 20]                       # 7 owned, 9 train-pos, 21 belongs to centre 1 (not asked)
    slot_of = {12: 2, 0: 0}
    tr = lambda i: H.translate(i, 5, 8, 3, [6, 9], [1, 0], slot_of)
    assert [tr(i) for i in (5, 7, 6, 9, 12, 0, 1, -1)] == [0, 2, 1, 3, 5 + 2, 5, H.MISS, -1]
    assert H.mean_f64(np.array([[1.0, 2.0], [3.0, 4.0]]), 4).tolist() == [1.0, 1.5]
