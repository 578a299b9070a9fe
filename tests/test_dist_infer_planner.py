"""The host planner of partitioned whole-set inference (dist.plan_infer_chunks / infer_pitch / infer_remote_pairs): chunks
whose per-owner remote demand fits the pitch, counted here independently; no GPU."""
import numpy as np
import pytest

from pcgnn_amd import dist
from pcgnn_amd.fused import infer_row_caps


def random_shard(n, world, rank, n_edges, seed, n_rel=3, hub=None):
    """rank `rank`'s CSR rows (global neighbour ids) of a random graph; hub: (local row, degree) of one row that names
    that many distinct remote nodes"""
    rs = np.random.RandomState(seed)
    bounds = np.linspace(0, n, world + 1).astype(np.int64)
    lo, hi = int(bounds[rank]), int(bounds[rank + 1])
    csr = []
    for r in range(n_rel):
        rows = rs.randint(0, hi - lo, n_edges)
        cols = rs.randint(0, n, n_edges)
        if hub is not None and r == 0:
            remote = np.setdiff1d(np.arange(n), np.arange(lo, hi))
            rows = np.concatenate([rows, np.full(hub[1], hub[0])])
            cols = np.concatenate([cols, rs.choice(remote, hub[1], replace=False)])
        key = np.unique(rows.astype(np.int64) * n + cols)
        rr, cc = key // n, key % n
        indptr = np.zeros(hi - lo + 1, np.int64)
        indptr[1:] = np.cumsum(np.bincount(rr, minlength=hi - lo))
        csr.append((indptr, cc.astype(np.int32)))
    return csr, bounds


def demand(csr, bounds, rank, pos_sorted, ids):
    """distinct remote, non-train-pos neighbour ids per owner of a set of local rows (np.unique, no shared code)"""
    lo, hi = bounds[rank], bounds[rank + 1]
    got = [np.zeros(0, np.int64)]
    for indptr, idx in csr:
        for i in ids:
            got.append(idx[indptr[i]:indptr[i + 1]].astype(np.int64))
    nb = np.unique(np.concatenate(got))
    nb = nb[((nb < lo) | (nb >= hi)) & ~np.isin(nb, pos_sorted)]
    return np.bincount(np.searchsorted(bounds[1:-1], nb, side="right"), minlength=len(bounds) - 1)


def test_chunks_fit_pitch_cover_in_order_and_size_the_list():
    csr, bounds = random_shard(3000, 3, 1, 4000, seed=1)
    pos = np.sort(np.random.RandomState(2).choice(3000, 60, replace=False))
    rs = np.random.RandomState(3)
    ids = np.concatenate([rs.permutation(1000), rs.choice(1000, 200)])          # shuffled, with duplicates
    thr = [0.5] * 3
    pitch = dist.infer_pitch(dist.infer_remote_pairs(csr, bounds, 1, pos, ids), bounds, 150)
    assert pitch == 150                                   # (the whole set asks for far more than 150 rows of an owner)
    chunks, cap = dist.plan_infer_chunks(csr, bounds, 1, pos, ids, pitch, 400, thr)
    assert len(chunks) >= 4
    assert chunks[0][0] == 0 and chunks[-1][1] == len(ids)
    assert all(a < b and b - a <= 400 for a, b in chunks)
    assert all(chunks[k][1] == chunks[k + 1][0] for k in range(len(chunks) - 1))
    caps = infer_row_caps([np.diff(ip) for ip, _ in csr], thr, ids)
    assert cap == max(int(caps[a:b].sum()) for a, b in chunks)
    for a, b in chunks:
        d = demand(csr, bounds, 1, pos, ids[a:b])
        assert d[1] == 0 and d.max() <= pitch
        if b < len(ids) and b - a < 400:                  # cut by the pitch: one more row would not have fitted
            assert demand(csr, bounds, 1, pos, ids[a:b + 1]).max() > pitch


def test_pitch_raised_for_a_hub_row_and_capped_by_the_set():
    csr, bounds = random_shard(4000, 2, 0, 2000, seed=4, hub=(7, 900))
    pos = np.zeros(0, np.int64)
    ids = np.arange(2000)
    pairs = dist.infer_remote_pairs(csr, bounds, 0, pos, ids)
    hub_need = demand(csr, bounds, 0, pos, [7]).max()
    assert hub_need >= 900
    assert dist.infer_pitch(pairs, bounds, 100) == hub_need                   # a budget below one row's demand is raised
    whole = demand(csr, bounds, 0, pos, ids).max()
    assert dist.infer_pitch(pairs, bounds, 10 ** 9) == whole                  # never more than the whole set asks
    chunks, _ = dist.plan_infer_chunks(csr, bounds, 0, pos, ids, hub_need, 10 ** 6, [0.5] * 3, pairs)
    assert any(a <= 7 < b for a, b in chunks)
    for a, b in chunks:
        assert demand(csr, bounds, 0, pos, ids[a:b]).max() <= hub_need


def test_empty_and_local_only_sets():
    csr, bounds = random_shard(1000, 2, 1, 800, seed=5)
    pos = np.zeros(0, np.int64)
    assert dist.plan_infer_chunks(csr, bounds, 1, pos, np.zeros(0, np.int64), 10, 100, [0.5] * 3) == ([], 1)
    pairs = dist.infer_remote_pairs(csr, bounds, 1, pos, np.zeros(0, np.int64))
    assert pairs[0].size == 0 and dist.infer_pitch(pairs, bounds, 50) == 1
    one, _ = random_shard(1000, 1, 0, 800, seed=6)                           # world 1: nothing is remote, only the row cap cuts
    ids = np.arange(1000)
    chunks, cap = dist.plan_infer_chunks(one, np.array([0, 1000]), 0, pos, ids, 1, 300, [0.5] * 3)
    assert chunks == [(0, 300), (300, 600), (600, 900), (900, 1000)] and cap >= 1


def test_agreed_chunk_counts_when_ranks_differ():
    """every rank runs max-over-ranks chunks with the agreed pitch (simulated ranks: the max a collective would return)"""
    world, n = 3, 6000
    shards = [random_shard(n, world, r, 3000 + 1500 * r, seed=10 + r) for r in range(world)]
    pos = np.sort(np.random.RandomState(9).choice(n, 40, replace=False))
    ids = [np.arange(2000), np.arange(500), np.zeros(0, np.int64)]          # (rank 2: no ids at all)
    pitches = [dist.infer_pitch(dist.infer_remote_pairs(c, b, r, pos, ids[r]), b, 200) for r, (c, b) in enumerate(shards)]
    pitch = max(pitches)
    plans = [dist.plan_infer_chunks(c, b, r, pos, ids[r], pitch, 500, [0.5] * 3)[0] for r, (c, b) in enumerate(shards)]
    counts = [len(p) for p in plans]
    assert counts[2] == 0 and counts[0] != counts[1]
    agreed = max(counts)
    assert agreed == max(counts[0], counts[1]) and agreed >= 4
    for r, p in enumerate(plans):                                           # the chunks a rank lacks are empty exchanges
        padded = p + [(len(ids[r]), len(ids[r]))] * (agreed - len(p))
        assert len(padded) == agreed and sum(b - a for a, b in padded) == len(ids[r])
        for a, b in p:
            assert demand(shards[r][0], shards[r][1], r, pos, ids[r][a:b]).max() <= pitch


@pytest.mark.parametrize("world", [2, 4])
def test_remote_pairs_match_bruteforce(world):
    csr, bounds = random_shard(2000, world, 1, 1500, seed=20 + world)
    pos = np.sort(np.random.RandomState(1).choice(2000, 30, replace=False))
    ids = np.random.RandomState(2).choice(2000 // world, 300)
    p, v = dist.infer_remote_pairs(csr, bounds, 1, pos, ids)
    want = set()
    lo, hi = bounds[1], bounds[2]
    for i, row in enumerate(ids):
        for indptr, idx in csr:
            for x in idx[indptr[row]:indptr[row + 1]]:
                if (x < lo or x >= hi) and x not in pos:
                    want.add((i, int(x)))
    assert sorted(want) == list(zip(p.tolist(), v.tolist()))
    assert np.all(np.diff(p) >= 0)
