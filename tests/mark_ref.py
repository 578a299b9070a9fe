"""Host reference of the touched-rows byte maps (pcg_mark_touched / pcg_mark_touched_planned, include/pcgnn.h) and the two
hand-built graphs tests/test_gpu_touched_marks.py runs them on.  Plain numpy, written from the contract - batch s marks its
centres, every neighbour of a centre in any relation, and every train positive; ids outside [0, n) are dropped - with no id
range, degree tier or queue anywhere in it."""
import numpy as np


def touched_ids(csrs, train_pos, nodes, B, n):
    """Per batch nodes[s * B : (s + 1) * B] the sorted int64 array of the ids its map must mark."""
    nodes = np.asarray(nodes, dtype=np.int64)
    pos = np.asarray(train_pos, dtype=np.int64).reshape(-1)
    out = []
    for lo in range(0, len(nodes), B):
        centres = nodes[lo:lo + B]
        parts = [centres, pos]
        for indptr, indices in csrs:
            for v in centres:
                if 0 <= v < len(indptr) - 1:
                    parts.append(np.asarray(indices[indptr[v]:indptr[v + 1]], dtype=np.int64))
        ids = np.unique(np.concatenate(parts))
        out.append(ids[(ids >= 0) & (ids < n)])
    return out


def shift_rule(n_slots, map_stride):
    """The id-range width pcg_mark_touched_planned picks (2^shift ids per workgroup): a copy of the rule in csrc/mark.hip, kept
    here so that a change of the rule fails the tests' coverage check instead of silently un-covering a shift."""
    shift = 19
    while shift > 16 and n_slots * ((map_stride + (1 << shift) - 1) >> shift) < 256:
        shift -= 1
    return shift, (map_stride + (1 << shift) - 1) >> shift


def csr_of_rows(n, rows, default_self_loop=True):
    """(indptr int64, indices int32) of a graph whose row v is rows[v] (a sorted id array) where given, else the self-loop
    [v] (or nothing)."""
    deg = np.full(n, 1 if default_self_loop else 0, dtype=np.int64)
    for v, row in rows.items():
        deg[v] = len(row)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = np.empty(int(indptr[-1]), dtype=np.int32)
    if default_self_loop:
        keep = np.ones(n, dtype=bool)
        keep[list(rows)] = False
        indices[indptr[:-1][keep]] = np.flatnonzero(keep).astype(np.int32)
    for v, row in rows.items():
        row = np.asarray(row, dtype=np.int64)
        assert row.size == 0 or (np.all(np.diff(row) > 0) and row[0] >= 0 and row[-1] < n), v
        indices[indptr[v]:indptr[v + 1]] = row.astype(np.int32)
    return indptr, indices


# ---- graph A: 600 000 nodes, rows planted at every degree tier and across every 2^16-id boundary ----------------------------
A_N = 600_000
A_EDGE = 1 << 16                      # the narrowest id range; every wider one's boundaries are multiples of it
A_B, A_TAIL = 49, 29                  # batch size and the (shorter) last batch of every run of graph A


def labels_a():
    """Two positive centres: 3002 (16 neighbours, with minority picks to come: the plan gives it a wave of its own, not a
    quarter of one) and the hub 1000."""
    lab = np.zeros(A_N, dtype=np.int64)
    lab[[3002, 1000]] = 1
    return lab


def _with(ids, *more):
    return np.unique(np.concatenate([np.asarray(ids, dtype=np.int64)] + [np.asarray(m, dtype=np.int64) for m in more]))


def graph_a():
    """Returns (csrs, train_pos, centres, facts).  Relation 0: a self-loop per node except the planted centre rows; relation 1:
    empty rows except three of the planted centres.  `facts`: what the planted rows are meant to contain, for the coverage test.
    Every planted row is described by (node, relation): its stretch inside an id range is a property the coverage test recomputes
    from the row itself."""
    n = A_N
    rs = np.random.RandomState(20)
    bounds = np.array([b for k in range(1, n // A_EDGE + 1) for b in (A_EDGE * k - 1, A_EDGE * k) if A_EDGE * k < n], dtype=np.int64)
    rows0, rows1 = {}, {}
    # > 4096 neighbours (the hub queue of pcg_mark_touched too): every boundary id, 0 and n - 1, the rest spread over the table
    rows0[1000] = _with(rs.choice(n, size=6000, replace=False), bounds, [0, n - 1, 1000])
    # > 4096, nothing at all in [2 * 65536, 6 * 65536): empty in middle ranges at every shift
    lo_part = rs.choice(2 * A_EDGE, size=2500, replace=False)
    hi_part = 6 * A_EDGE + rs.choice(n - 6 * A_EDGE, size=2500, replace=False)
    rows0[1001] = _with(lo_part, hi_part, [0, 2 * A_EDGE - 1, 6 * A_EDGE, n - 1])
    # 513 .. 4096: wholly inside one 2^16 range (range 3), touching its first and last id
    base = 3 * A_EDGE
    rows0[1002] = _with(base + rs.choice(A_EDGE, size=900, replace=False), [base, base + A_EDGE - 1])
    # 513 .. 4096: stretches of exactly 1, 256 and 257 ids inside 2^16 ranges 4, 5 and 7 (the sweep's 256-id piece edges), the
    # rest in range 0; range 4's single id is its LAST id, range 5's 256 begin at its first
    rows0[1003] = _with(np.arange(100, 100 + 600), [5 * A_EDGE - 1], 5 * A_EDGE + np.arange(256),
                        7 * A_EDGE + 11 + 3 * np.arange(257))
    # 513 .. 4096: nothing in [4 * 65536, 8 * 65536) - the middle one of the three ranges of 2^18 ids
    rows0[1007] = _with(rs.choice(4 * A_EDGE, size=600, replace=False), 8 * A_EDGE + rs.choice(n - 8 * A_EDGE, size=600, replace=False))
    # 513 .. 4096 in relation 1 too (the sparse relation): the last range's end, n - 1 included, and the first ids of the table
    rows1[1003] = _with(np.arange(0, 300), n - 1 - np.arange(300))
    # 513 exactly, and 4096 / 4097: the tier edges themselves
    rows0[1004] = _with(rs.choice(n, size=513, replace=False))[:513]
    rows0[1005] = _with(rs.choice(n, size=4200, replace=False))[:4096]
    rows0[1006] = _with(rs.choice(n, size=4200, replace=False), bounds)[:4097]
    # 65 .. 512 (a wave per row): boundary ids again, 0 and n - 1
    rows0[2000] = _with(rs.choice(n, size=300, replace=False), bounds[:6], [0, n - 1])
    rows0[2001] = _with(rs.choice(n, size=64, replace=False), [2001])[:65]
    rows0[2002] = _with(rs.choice(n, size=512, replace=False))[:512]
    rows1[2000] = _with(rs.choice(n, size=100, replace=False), bounds[6:])
    # <= 64 (four rows to a wave): 64 exactly, 17, 16, 2; every other centre is a self-loop row of one neighbour
    rows0[3000] = _with(rs.choice(n, size=64, replace=False))[:64]
    rows0[3001] = _with(rs.choice(n, size=17, replace=False), bounds[-2:])[:17]
    rows0[3002] = _with(rs.choice(n, size=16, replace=False))[:16]
    rows0[3003] = np.array([0, n - 1], dtype=np.int64)
    rows1[3003] = np.array([A_EDGE - 1, A_EDGE], dtype=np.int64)
    # a row of degree 0 in both relations (DeviceGraph accepts it), away from the end of the neighbour array
    rows0[4000] = np.zeros(0, dtype=np.int64)
    csr0 = csr_of_rows(n, rows0, True)
    csr1 = csr_of_rows(n, rows1, False)
    # train positives on range boundaries - but a train positive is marked in EVERY batch, so an id that is one hides what the
    # sweep does with it: only two range starts (65536 and 5 * 65536, starts at shift 16 alone) are given away; the first id of
    # every wider range is left to the long rows
    train_pos = [0, A_EDGE - 1, A_EDGE, 3 * A_EDGE - 1, 5 * A_EDGE, (1 << 19) - 1, n - 1, 77]
    planted = sorted(rows0)
    return [csr0, csr1], train_pos, planted, dict(bounds=bounds, long_rows=[(1000, 0), (1001, 0), (1002, 0), (1003, 0), (1003, 1),
                                                                          (1004, 0), (1005, 0), (1006, 0), (1007, 0)])


def nodes_a(planted, n_slots, B, tail):
    """n_total = (n_slots - 1) * B + tail centres: the planted rows spread over the batches so that every batch has some, the
    first, a middle and the LAST (shorter) batch have all of them, the rest self-loop rows."""
    rs = np.random.RandomState(100 + n_slots)
    n_total = (n_slots - 1) * B + tail
    nodes = 5000 + rs.choice(A_N - 5000, size=n_total, replace=False).astype(np.int64)      # (self-loop rows: ids >= 5000)
    k = len(planted)
    assert tail >= k and B >= k
    for s in range(n_slots):
        lo = s * B
        if s in (0, n_slots // 2, n_slots - 1):
            nodes[lo:lo + k] = planted
        else:
            nodes[lo:lo + 3] = [planted[s % k], planted[(s * 7 + 3) % k], planted[(s * 5 + 1) % k]]
    return nodes.astype(np.int32)


# ---- graph B: more than 512 long rows in one batch ---------------------------------------------------------------------------
B_N = 200_000


def graph_b():
    """200 000 nodes, 2 relations; the 637 centres (ids 0 .. 636) have 513 .. 700 neighbours in BOTH relations, everything else
    a self-loop in relation 0 and nothing in relation 1.  One batch of 600 -> 1 200 long rows: three turns of the sweep's
    512-row loop, the last one partial (176 rows)."""
    n = B_N
    rs = np.random.RandomState(21)
    rows = [{}, {}]
    for v in range(637):
        for r in (0, 1):
            d = 513 + (v * 7 + r * 3) % 188
            rows[r][v] = _with(rs.randint(0, n, size=d + 24))[:d]          # (a few repeats at most: still >= d distinct ids)
            assert len(rows[r][v]) == d
    return [csr_of_rows(n, rows[0], True), csr_of_rows(n, rows[1], False)], [5, 65535, 65536, n - 1], np.arange(637, dtype=np.int32)
