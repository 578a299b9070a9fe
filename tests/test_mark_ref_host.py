"""CPU-only tests of the reference the touched-rows byte maps are checked with (tests/mark_ref.py): a 12-node, 2-relation graph
whose answer is written out by hand, planted errors that the comparison the GPU tests make must notice, and the coverage the two
hand-built graphs promise - every degree tier, every 2^16-id boundary, the id-range shifts 16 to 19, more than 512 long rows in one
batch - recomputed from the graphs themselves."""
import numpy as np
import pytest

from tests import mark_ref as M

# relation 0: a path 0-1-2-...-11 with self-loops on 0..5 only; relation 1: a star round 7 (7: 2, 7, 9, 11), 3: 10 and an
# out-of-range id 12 (dropped), node 11: no neighbour at all
R0 = {0: [0, 1], 1: [0, 1, 2], 2: [1, 2, 3], 3: [2, 3, 4], 4: [3, 4, 5], 5: [4, 5, 6], 6: [5, 7], 7: [6, 8], 8: [7, 9], 9: [8, 10],
      10: [9, 11], 11: [10]}
R1 = {3: [10, 12], 7: [2, 7, 9, 11]}
N = 12


def tiny_csr(rows):
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum([len(rows.get(v, [])) for v in range(N)], out=indptr[1:])
    idx = np.array([x for v in range(N) for x in rows.get(v, [])], dtype=np.int32)
    return indptr, idx


@pytest.fixture(scope="module")
def tiny():
    csrs = [tiny_csr(R0), tiny_csr(R1)]
    train_pos = [5, 11, -1]                      # (-1: out of range, dropped)
    nodes = [0, 7, 3, 11, 6]                     # B = 2: batches [0, 7], [3, 11], [6]
    return csrs, train_pos, nodes


# centres | relation 0 | relation 1 | train positives
WANT = [[0, 1, 2, 5, 6, 7, 8, 9, 11],            # {0, 7} | {0, 1} + {6, 8} | {2, 7, 9, 11} | {5, 11}
        [2, 3, 4, 5, 10, 11],                    # {3, 11} | {2, 3, 4} + {10} | {10} (12 dropped) | {5, 11}
        [5, 6, 7, 11]]                           # {6} | {5, 7} | - | {5, 11}


def test_hand_written_answer(tiny):
    csrs, train_pos, nodes = tiny
    got = M.touched_ids(csrs, train_pos, nodes, 2, N)
    assert [g.tolist() for g in got] == WANT
    assert all(g.dtype == np.int64 for g in got)
    # a batch size that does not divide: one batch of all five, the union
    got = M.touched_ids(csrs, train_pos, nodes, 8, N)
    assert len(got) == 1 and got[0].tolist() == sorted(set(sum(WANT, [])))
    # n smaller than the id space: ids >= n are dropped like the kernels drop them
    assert M.touched_ids(csrs, train_pos, nodes, 2, 8)[0].tolist() == [0, 1, 2, 5, 6, 7]


def coords(per_batch, stride):
    """what the GPU tests compare: flat nonzero coordinates of the batches' maps"""
    return np.concatenate([s * stride + ids for s, ids in enumerate(per_batch)])


def test_planted_errors_are_noticed(tiny):
    csrs, train_pos, nodes = tiny
    stride = 16
    want = coords(M.touched_ids(csrs, train_pos, nodes, 2, N), stride)
    maps = np.zeros(3 * stride, dtype=np.uint8)
    maps[want] = 1
    assert np.array_equal(np.flatnonzero(maps), want)
    planted = {"a dropped boundary id": (0 * stride + 11, 0),             # the last id of the table, batch 0
               "a mark in the wrong batch": (2 * stride + 0, 1),          # batch 0's centre marked in batch 2
               "a missing train positive": (2 * stride + 11, 0)}
    for what, (at, value) in planted.items():
        bad = maps.copy()
        assert bad[at] != value, what
        bad[at] = value
        assert not np.array_equal(np.flatnonzero(bad), want), what
    # ... and when the reference itself is handed the faulty input: a row cut one id short, the centres shifted by one batch,
    # the train positives forgotten
    cut = (csrs[0][0].copy(), csrs[0][1].copy())
    cut[1][cut[0][10 + 1] - 1] = 9                                        # row 10: [9, 11] -> [9, 9]
    assert not np.array_equal(coords(M.touched_ids([cut, csrs[1]], [], [10], 2, N), stride),
                              coords(M.touched_ids(csrs, [], [10], 2, N), stride))
    assert not np.array_equal(coords(M.touched_ids(csrs, train_pos, nodes[1:] + nodes[:1], 2, N), stride), want)
    assert not np.array_equal(coords(M.touched_ids(csrs, [], nodes, 2, N), stride), want)


# ---- the coverage the GPU tests' graphs promise --------------------------------------------------------------------------------
def stretch(row, lo, hi):
    return int(np.searchsorted(row, hi) - np.searchsorted(row, lo))


def test_shift_rule_cases():
    """the four batch counts graph A runs at reach shifts 19, 18, 17, 16 with 2, 3, 5, 10 id ranges"""
    stride = (M.A_N + 1023) // 512 * 512
    assert stride == 600576
    assert [M.shift_rule(nb, stride) for nb in (128, 100, 60, 30)] == [(19, 2), (18, 3), (17, 5), (16, 10)]
    assert M.shift_rule(30, stride + 1040) == (16, 10) and (stride + 1040) % 16 == 0 and (stride + 1040) % 512 != 0
    assert M.shift_rule(2, (M.B_N + 1023) // 512 * 512) == (16, 4)


def test_graph_a_covers_what_it_promises():
    csrs, train_pos, planted, facts = M.graph_a()
    n = M.A_N
    deg = [np.diff(ip) for ip, _ in csrs]
    row = lambda v, r: csrs[r][1][csrs[r][0][v]:csrs[r][0][v + 1]].astype(np.int64)
    for r in (0, 1):
        for v in planted:
            x = row(v, r)
            assert np.all(np.diff(x) > 0) and (x.size == 0 or (x[0] >= 0 and x[-1] < n))
    d0 = deg[0][planted]
    # every degree tier of the plan (<= 16 | <= 64 | <= 512 | <= 4096 | longer) and the tier edges themselves
    assert {16, 17, 64, 65, 512, 513, 4096, 4097} <= set(d0.tolist()) and d0.max() > 6000
    assert deg[0][4000] == 0 and deg[1][4000] == 0                        # a centre with no neighbour at all
    assert int((deg[0] == 1).sum()) == n - len(planted) and int(deg[1].sum()) == sum(len(row(v, 1)) for v in (1003, 2000, 3003))
    long_rows = [(v, r) for r in (0, 1) for v in planted if deg[r][v] > 512]
    assert sorted(long_rows) == sorted(facts["long_rows"])
    every = np.unique(np.concatenate([row(v, r) for v, r in long_rows]))
    assert 0 in every and n - 1 in every
    assert np.isin(facts["bounds"], every).all() and len(facts["bounds"]) == 2 * 9
    assert np.isin(facts["bounds"], row(1000, 0)).all()                   # one row that crosses every boundary
    E = M.A_EDGE
    for shift in (16, 17, 18, 19):
        w, nr = 1 << shift, -(-600576 >> shift)
        per_row = {vr: [stretch(row(*vr), q * w, (q + 1) * w) for q in range(nr)] for vr in long_rows}
        # a row wholly inside one range; a row with nothing in some MIDDLE range (neighbours on both sides of it)
        assert any(sum(1 for c in cs if c) == 1 for cs in per_row.values()), shift
        if nr > 2:
            assert any(any(cs[q] == 0 and any(cs[:q]) and any(cs[q + 1:]) for q in range(1, nr - 1)) for cs in per_row.values()), shift
    # stretches of exactly 1, 256 and 257 ids inside a range (the sweep takes 256 ids at a time), at the narrowest ranges
    cs = [stretch(row(1003, 0), q * E, (q + 1) * E) for q in range(10)]
    assert cs[4] == 1 and cs[5] == 256 and cs[7] == 257 and row(1003, 0)[600] == 5 * E - 1 and row(1003, 0)[601] == 5 * E
    # ... and at shift 17, where ranges 4 and 5 merge: 257 on both sides
    assert stretch(row(1003, 0), 4 * E, 6 * E) == 257
    assert {0, E - 1, E, 5 * E, (1 << 19) - 1, n - 1} <= set(train_pos)
    # the batches: a shorter last one, every planted row in the first, a middle and the last, rows of <= 16 and of 17 .. 64
    # neighbours not a multiple of four in them (the short-row kernel takes four to a wave)
    for nb in (128, 100, 60, 30):
        nodes = M.nodes_a(planted, nb, M.A_B, M.A_TAIL)
        assert len(nodes) == (nb - 1) * M.A_B + M.A_TAIL and M.A_TAIL < M.A_B and nodes.min() >= 0 and nodes.max() < n
        lab = M.labels_a()
        for s in (0, nb // 2, nb - 1):
            c = nodes[s * M.A_B:(s + 1) * M.A_B]
            assert set(planted) <= set(c.tolist())
            na, n0 = 0, 0
            for r in (0, 1):
                d = deg[r][c]
                tail = (lab[c] == 1) & ((np.ceil(d * 0.5) * 0.5).astype(np.int64) > 0)
                na += int(((d <= 16) & ~tail).sum())
                n0 += int(((d <= 64) & ~((d <= 16) & ~tail)).sum())
            assert na % 4 != 0 and n0 % 4 != 0, (nb, s, na, n0)
        for s in range(nb):
            assert set(nodes[s * M.A_B:(s + 1) * M.A_B].tolist()) & set(planted)
        # A boundary id that a centre, a train positive or a short row marks as well says nothing about the sweep: the first
        # and the last id of every range of this run's shift (but the two starts given to the train positives) is, in some
        # batch, marked by long rows ALONE
        shift, nr = M.shift_rule(nb, 600576)
        need = {q << shift for q in range(1, nr)} | {(q << shift) - 1 for q in range(1, nr)} | {n - 1}
        need -= set(train_pos)
        starts = [q << shift for q in range(1, nr) if (q << shift) in need]
        assert len(starts) == nr - 1 if shift > 16 else len(starts) == nr - 3
        for s in range(nb):
            c = nodes[s * M.A_B:(s + 1) * M.A_B]
            short = [c, np.asarray(train_pos)] + [row(v, r) for r in (0, 1) for v in c if deg[r][v] <= 512]
            long_ = [row(v, r) for r in (0, 1) for v in c if deg[r][v] > 512]
            if long_:
                need -= set(np.setdiff1d(np.concatenate(long_), np.concatenate(short)).tolist())
        assert not need, (nb, sorted(need))


def test_graph_b_has_more_than_512_long_rows_in_one_batch():
    csrs, train_pos, nodes = M.graph_b()
    deg = [np.diff(ip) for ip, _ in csrs]
    assert len(nodes) == 637 and 637 == 600 + 37
    for r in (0, 1):
        d = deg[r][nodes]
        assert d.min() >= 513 and d.max() <= 700
    first = sum(int((deg[r][nodes[:600]] > 512).sum()) for r in (0, 1))
    assert first == 1200 and first > 2 * 512 and first % 512 == 176       # three turns of the 512-row loop, the last partial
    assert int(deg[1].sum()) == int(deg[1][nodes].sum())                   # relation 1: nothing outside the centres' rows
