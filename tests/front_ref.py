"""Host side of the front / score / optimizer entry-point tests (tests/test_front_ref_host.py on the CPU,
tests/test_gpu_front_entry_points.py, tests/test_gpu_optimizer_entry_points.py and tests/test_gpu_primitives_geometry.py on the
GPU): the row geometry of the score pass restated, the train-pos sort key, the float64 / float32 class-0 score, and the seeded
inputs the three GPU files share.

Geometry (csrc/common.h): lanes_per_row(stride) lanes share a feature row (8 / 16 / 32 / 64 for strides up to 32 / 64 / 128 /
256 floats; 64 lanes with a second float4 chunk each up to 512).  A score workgroup has 4 waves, a wave-instruction takes
64 / lpr rows, 8 in flight: ``rows_per_block`` rows per iteration of score_table_body.  The keys-from-feature-rows group
(pos_key_body) has at most 256 workgroups of 4 waves, a wave forms 64 / lpr keys at a time: ``keys_per_turn`` keys per turn of its
grid-stride loop.
"""
import numpy as np

from tests import dense_ref as D
from tests.gather_ref import lanes_per_row  # noqa: F401  (re-exported: the one restatement of csrc/common.h's rule)

SCORE_WIDTHS = [1, 3, 4, 5, 29, 32, 33, 64, 65, 128, 129, 256, 257, 260, 509, 512]
KEY_WIDTHS = [32, 64, 100, 256, 260]                     # one per tier: 8, 16, 32, 64 lanes and 64 lanes with two chunks
MAX_WIDTH = 512
TABLE_ROWS = 1000
SECOND_TURN = (260, 32768 + 33)                          # (F, n): 1024 workgroups x 32 rows per turn at 64 lanes per row
RANK_MAX = 16384                                         # the most train positives whose keys are formed beside the score pass
SCORE_BLOCKS_MAX = 1024                                  # score_table_blocks' cap (256 CUs x 4)
KEY_BLOCKS_MAX = 256                                     # front_a's cap on the key group


def stride_of(F):
    return (F + 3) // 4 * 4


def rows_per_block(F):
    """rows a score workgroup takes per iteration: 4 waves x 64 / lpr rows x 8 in flight"""
    return 4 * (64 // lanes_per_row(stride_of(F))) * 8


def rows_per_workgroup_launch(F):
    """rows a workgroup of pcg_score_rows / pcg_gather_rows takes: 4 waves x 64 / lpr rows"""
    return 4 * (64 // lanes_per_row(stride_of(F)))


def table_sizes(F):
    rb = rows_per_block(F)
    return sorted({1, rb - 1, rb, rb + 1, TABLE_ROWS})


def keys_per_turn(F):
    """keys the key group forms per turn of its grid-stride loop: 256 workgroups x 4 waves x 64 / lpr"""
    return KEY_BLOCKS_MAX * 4 * (64 // lanes_per_row(stride_of(F)))


def n_pos_list(F):
    T = keys_per_turn(F)
    return [1, T - 1, T, T + 1, min(2 * T + 3, RANK_MAX)]


def orderable(s):
    """float32 array -> uint32 whose unsigned order is the floats' order (-0.0 < +0.0): csrc's orderable()"""
    bits = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def pos_keys(s0, train_pos):
    """(orderable(s0[train_pos[i]]) << 32) | i, uint64 [n_pos]: the unsorted keys"""
    tp = np.asarray(train_pos, dtype=np.int64)
    return (orderable(np.asarray(s0)[tp]).astype(np.uint64) << np.uint64(32)) | np.arange(tp.size, dtype=np.uint64)


def sorted_keys(s0, train_pos, cap):
    """what pcg_pos_sort leaves in the first `cap` entries: the keys ascending, all-ones behind them"""
    out = np.full(cap, np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    k = np.sort(pos_keys(s0, train_pos))
    out[:k.size] = k
    return out


def sort_capacity(n_pos):
    """half of pcg_pos_sort_capacity: ceil_pow2(max(n_pos, 4096))"""
    cap = 4096
    while cap < n_pos:
        cap *= 2
    return cap


def weights(F, seed):
    """(W float32 [2, F], b float32 [2]): |w| in [0.5, 1.5] with a random sign - no column is negligible in a score"""
    rs = np.random.RandomState(9000 + 7 * seed + F)
    W = (rs.uniform(0.5, 1.5, size=(2, F)) * np.where(rs.rand(2, F) < 0.5, -1.0, 1.0)).astype(np.float32)
    b = (rs.uniform(0.5, 1.5, size=2) * np.where(rs.rand(2) < 0.5, -1.0, 1.0)).astype(np.float32)
    return W, b


def table(seed=23, rows=TABLE_ROWS, width=MAX_WIDTH):
    """N(0, 1) float32 [rows, width]: width F of the matrix is the first F columns"""
    return np.random.RandomState(seed).randn(rows, width).astype(np.float32)


def scores_f64(X, w, b):
    """X [n, F] float32, w [F], b scalar -> float64 [n]"""
    return X.astype(np.float64) @ np.asarray(w, dtype=np.float64) + float(b)


def scores_f32(X, w, b):
    """the yardstick: the same dot summed one column after the other in float32"""
    prod = X.astype(np.float32) * np.asarray(w, dtype=np.float32)[None, :]
    return np.cumsum(prod, axis=1, dtype=np.float32)[:, -1] + np.float32(b)


def score_check(got, X, w, b):
    """(e_kernel, e_f32, tolerance) of one call: rel_err against float64 over the call's rows, the project's bound
    8 * e_f32 + 2^-20 from the sequential float32 dot of the same rows"""
    ref = scores_f64(X, w, b)
    e32 = D.rel_err(scores_f32(X, w, b), ref)
    return D.rel_err(np.asarray(got, dtype=np.float64), ref), e32, D.tolerance(e32)


def dropped_columns(F):
    """the columns a sensitivity check leaves out: the last one, column 4, and for F > 256 one at or past 256"""
    cols = {F - 1}
    if F > 4:
        cols.add(4)
    if F > 256:
        cols.add(256 + (F - 256) // 2)
    return sorted(cols)


def shuffled_ids(n, length, seed):
    """int32 [length] ids in [0, n), shuffled, every id of a small table at least once when length allows, with duplicates"""
    rs = np.random.RandomState(seed)
    ids = np.concatenate([rs.permutation(n)[:length], rs.randint(0, n, size=max(length - n, 0))])[:length]
    if length >= 3:
        ids[length // 2] = ids[0]                          # (a duplicate even where length <= n)
        ids[-1] = ids[1]
    return rs.permutation(ids).astype(np.int32)


def key_table(F, seed=31):
    """(X float32 [n, F], n): the raw-key tests' table - large enough for the longest train_pos list of the width, with
    a few dozen rows copied onto others so that equal scores occur among the train positives and the position decides"""
    n = max(n_pos_list(F)) + 500
    rs = np.random.RandomState(seed + F)
    X = rs.randn(n, F).astype(np.float32)
    src = rs.choice(n, size=48, replace=False)
    dst = rs.choice(n, size=48, replace=False)
    X[dst] = X[src]
    return X, n


def train_pos_list(n, n_pos, seed):
    """distinct ids, shuffled - not ascending (asserted for n_pos > 2 by the host test)"""
    return np.random.RandomState(seed).permutation(n)[:n_pos].astype(np.int64)


# ---- the optimizer entry points' inputs ----------------------------------------------------------------------------------------
OPT_SHAPE = (25, 16, 2)                                  # (F, E, R): label_clf.weight's offset is no multiple of 64
OPT_SLABS = [1, 2, 3, 4, 5, 8, 9]                        # the quarter-per-wave edges of adam_reduce_body, with empty wave ranges
OPT_T = [1, 7]
OPT_LR, OPT_WD, OPT_BETAS, OPT_EPS = 0.01, 5e-4, (0.9, 0.999), 1e-8
OPT_SMALL_N = [1, 63, 64, 65]


def opt_n_params(F, E, R):
    """pcg_dense_n_params restated: weight [2, E] | inter1.weight [F + R E, E] | R x [2F, E] | label_clf.weight [2, F] | bias [2]"""
    return 2 * E + (F + R * E) * E + R * 2 * F * E + 2 * F + 2


def opt_clf_offset(F, E, R):
    return 2 * E + (F + R * E) * E + R * 2 * F * E


def opt_inputs(n_params, n_slabs, seed):
    """Gaussian theta, m, slabs and v >= 0, float32: dict(theta, m, v, slabs [n_slabs, n_params]).
    adam_ref's bar on theta is ABSOLUTE, lr * 2e-5 = 2e-7, so the scales keep the values where float32 can hold it: theta has
    standard deviation 0.1 (initialised weights; float32 values of magnitude 2 and more are 2.4e-7 and more apart), and the
    moments describe a state Adam could be in - m of standard deviation 0.01 beside v = N(0, 1)^2, so that m / sqrt(v) stays of
    order one after the bias correction of t = 1 (a large m beside a tiny v, which no run of Adam produces, makes the update
    itself of magnitude 1 and more, and its few float32 roundings alone exceed the bar).  OPT_STEP_CAP and
    tests/test_front_ref_host.py state this as a condition on the float64 reference."""
    rs = np.random.RandomState(5000 + 131 * seed + 17 * n_slabs + n_params % 97)
    return dict(theta=(0.1 * rs.randn(n_params)).astype(np.float32), m=(0.01 * rs.randn(n_params)).astype(np.float32),
                v=(rs.randn(n_params) ** 2).astype(np.float32),
                slabs=rs.randn(max(n_slabs, 1), n_params).astype(np.float32)[:n_slabs])


# |theta' - theta| and |theta'| of the float64 reference stay below these (a condition on the inputs): the update's handful of
# float32 operations then err by a few 2^-24 * 0.25 = 1.5e-8 each, and theta' is stored to within 2^-25 = 3e-8
OPT_STEP_CAP, OPT_THETA_CAP = 0.25, 1.0


def slab_sum_f64(slabs):
    return slabs.astype(np.float64).sum(0)


def slab_sum_f32(slabs):
    """the yardstick: the slabs added one after the other in float32"""
    return np.cumsum(slabs, axis=0, dtype=np.float32)[-1]
