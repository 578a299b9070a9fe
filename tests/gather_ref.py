"""Host side of the gather + combine geometry matrix (tests/test_gpu_gather_geometry.py, tests/test_gather_ref_host.py): a
one-relation graph whose centre rows have exactly the degrees at which the aggregation path changes geometry, two feature tables
over it, and the two references of a row's mean - an exact one for integer data and float64 with its float32 yardstick for
Gaussian data.

Geometry (csrc/common.h, csrc/gather.hip): lanes_per_row(stride) lanes share a feature row - 8 / 16 / 32 / 64 lanes for strides
up to 32 / 64 / 128 / 256 floats, 64 lanes with two float4 accumulators each up to 512 -, a wave-instruction gathers 64 / lpr
rows, eight in flight (per_iter = 64, 32, 16, 8 list entries), a list is cut into chunks of 128 entries, and combine_rows adds a
row's chunk sums 16 (one accumulator) or 8 (two) at a time.
"""
import numpy as np

from tests import dense_ref as D

CHUNK = 128
# per_iter +- 1 of every tier | the chunk edges | the combine-batch edges (8 | 9, 16 | 17, 17 | 18 chunks) | degree 1
DEG = [7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1024, 1025, 2048, 2049, 2176, 2177, 1]
# both sides of every tier edge, ragged and full last float4
WIDTHS = [1, 3, 4, 5, 29, 32, 33, 61, 64, 65, 125, 128, 129, 253, 256, 257, 509, 512]
NORM_WIDTHS = [32, 100, 260, 512]
MAX_WIDTH = 512
N_NODES = 2300
INT_RANGE = 8               # the integer data: values in [-8, 8]


def lanes_per_row(stride):
    """csrc/common.h, restated"""
    lanes = 8
    while lanes < stride // 4 and lanes < 64:
        lanes *= 2
    return lanes


def geometry_graph(seed=17):
    """(indptr int64 [n + 1], indices int32): centre i < len(DEG) has exactly DEG[i] neighbours - itself and DEG[i] - 1 distinct
    others drawn from the whole graph -, every other node itself and two others; ids ascending inside a row."""
    rs = np.random.RandomState(seed)
    rows = []
    for v in range(N_NODES):
        d = DEG[v] if v < len(DEG) else 3
        others = rs.choice(N_NODES - 1, size=d - 1, replace=False)
        others += others >= v                                  # (skips v: the self-loop is added once)
        rows.append(np.sort(np.concatenate([others, [v]])).astype(np.int32))
    indptr = np.zeros(N_NODES + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=indptr[1:])
    return indptr, np.concatenate(rows)


def batch_nodes(seed=18):
    """every centre once, shuffled, then three of them again (the longest row, a two-chunk row, the row of one entry)"""
    order = np.random.RandomState(seed).permutation(len(DEG))
    return np.concatenate([order, [DEG.index(2177), DEG.index(129), DEG.index(1)]]).astype(np.int32)


def tables(seed=19):
    """(integers in [-8, 8], N(0, 1)), float32 [N_NODES, 512] each: width F of the matrix is the first F columns"""
    rs = np.random.RandomState(seed)
    xi = rs.randint(-INT_RANGE, INT_RANGE + 1, size=(N_NODES, MAX_WIDTH)).astype(np.float32)
    return xi, rs.randn(N_NODES, MAX_WIDTH).astype(np.float32)


def int_sums(X, sets):
    """the rows' sums over their sets in int64 (X holds integers) [B, F] and the set sizes [B]"""
    xi = X.astype(np.int64)
    assert np.array_equal(xi.astype(np.float32), X), "integer data only"
    return np.stack([xi[sorted(s)].sum(0) for s in sets]), np.array([len(s) for s in sets], dtype=np.int64)


def exact_mean(sums, cnt, norm=0):
    """What a float32 device must give bit for bit: every partial sum of the integer data is exact in float32 in any order
    (|sum| < 2^24), so the only rounding is the one correctly rounded division by float(cnt) (norm 0) or by
    sqrtf(float(cnt)) (norm 1) - numpy's float32 division and sqrt are IEEE too."""
    assert int(np.abs(sums).max()) < 2 ** 24 and int(cnt.max()) < 2 ** 24
    den = cnt.astype(np.float32)
    if norm == 1:
        den = np.sqrt(den)                                     # (float32 in, float32 out: correctly rounded)
    assert den.dtype == np.float32
    return sums.astype(np.float32) / den[:, None]


def mean_f64(X, idx):
    return X[idx].astype(np.float64).sum(0) / float(len(idx))


def mean_f32_sequential(X, idx):
    """the yardstick: the same mean summed one entry after the other in float32"""
    return np.cumsum(X[idx], axis=0, dtype=np.float32)[-1] / np.float32(len(idx))


def gaussian_row_check(got, X, s):
    """(e_kernel, e_f32, tolerance) of one row: rel_err against the float64 mean over the set, the project's bound
    8 * e_f32 + 2^-20 from the sequential float32 sum of the same entries"""
    idx = np.array(sorted(s), dtype=np.int64)
    ref = mean_f64(X, idx)
    e_32 = D.rel_err(mean_f32_sequential(X, idx), ref)
    return D.rel_err(got, ref), e_32, D.tolerance(e_32)
