"""Shared by tests/test_presorted_window_host.py (CPU) and tests/test_gpu_presorted_window.py: the sizes, the crafted scores and the
search index's arithmetic (select.hip: key_index_stride, window_bracket) restated in Python."""
import math

import numpy as np

KIDX_MAX = 512
UNIT = 2.0 ** -10              # every score is a multiple: sums and differences are exact in float32
SIZES = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193]      # 8193: the stride becomes 32
PLAIN_SIZE, PLAIN_M = 8300, 4100     # a bracket wider than two probe rounds (64 * 64): no size of SIZES has one
DEGREES = [17, 20, 64, 65, 130, 300, 512, 513, 600]       # lane rows (<= 64), wave rows (<= 512), workgroup rows
M_TARGETS = (1, 2, 47, 48, 49)
THR = 0.5


def index_stride(P):
    stride = 16
    while (P + stride - 1) // stride > KIDX_MAX:
        stride *= 2
    return stride


def index_shape(P):
    stride = index_stride(P)
    return stride, (P + stride - 1) // stride


def key_scores(P):
    """the sorted scores of P training positives: 4, 8, 12, ... units"""
    return (4 * np.arange(1, P + 1) * UNIT).astype(np.float32)


def centre_scores(P):
    """eight centre scores by their position among the keys"""
    s = key_scores(P)
    stride, n_idx = index_shape(P)
    on_index = s[stride * (n_idx // 2)] if n_idx >= 3 else s[min(stride, P - 1)]
    between = s[stride + 3] + 2 * UNIT if n_idx >= 3 else s[0] + 2 * UNIT
    return {"below": np.float32(0.0), "above": np.float32(s[-1] + 4 * UNIT), "on_key": s[P // 3], "first": s[0], "last": s[-1],
            "on_index": np.float32(on_index), "between": np.float32(between), "between_end": np.float32(s[-1] - 2 * UNIT)}


def m_values(P):
    return sorted({m for m in M_TARGETS + (P - 1, P, P + 1) if 1 <= m <= P + 1})


def bracket(scores, c, m):
    """window_bracket: (lo_min, lo_max, t) - t = index entries below c"""
    s = np.asarray(scores, dtype=np.float32)
    P = s.size
    stride, n_idx = index_shape(P)
    ix = s[::stride]
    assert ix.size == n_idx
    t = int(np.searchsorted(ix, np.float32(c), side="left"))
    pc_lo = (t - 1) * stride + 1 if t > 0 else 0
    pc_hi = min(t * stride, P)
    lo_min = max(pc_lo - m, 0)
    lo_max = min(pc_hi, P - m)
    return lo_min, max(lo_max, lo_min), t


def sample_count(d, thr=THR):
    return int(math.ceil(d * thr))


def gpu_cases(P):
    """the launches of the GPU test at P: (m_star, d_star, rho) - rho makes int(k * rho) == m_star on the rows of degree d_star;
    the other degrees get int(k_d * rho), clipped to P by the plan"""
    if P == PLAIN_SIZE:
        return [(PLAIN_M, 130, (PLAIN_M + 0.5) / sample_count(130))]
    out = []
    for m in m_values(P):
        for d_star in ((20, 130, 600) if m in M_TARGETS else (130,)):
            k = sample_count(d_star)
            out.append((m, d_star, (m + 0.5) / k))
    return out


def row_m(d, rho, P):
    return min(int(sample_count(d) * rho), P)


# ---- the bucket-sorted sizes (n_pos >= 16384: strides of 32 .. 1024) --------------------------------------------------------------
LARGE_SIZES = [16384, 16385, 32768, 32769, 65537, 131072, 131073, 262145]
LARGE_STRIDES = [32, 64, 64, 128, 256, 256, 512, 1024]
STAGE_MAX = 64 * 64                 # win_stageable: stride - 1 + m <= 4096 (two probe rounds)
LARGE_PLAIN_M = 4200                # stride - 1 + m > 4096 at every stride: a third probe round
LARGE_WHOLE = 16385                 # the one large size whose windows reach P - 1, P and P + 1 (host oracle: sets of P ids)
SHORT_DEGREES = [d for d in DEGREES if d <= 65]


def large_cases(P):
    """the launches of the GPU test at a large P: (m_star, d_star, rho, degrees) - the rows of degree d_star get m_star, the
    other degrees of `degrees` int(k_d * rho) (None: every degree of DEGREES).  m_star = 1, 2, 48 on every centre; both sides of
    the staging switch and one m above two probe rounds on the longest single-wave row (512: the smaller degrees get smaller
    windows, 513 and 600 - workgroup rows - slightly larger ones); the switch again on a lane row (64), among the short rows
    alone (a workgroup row's window would be ten times that); at LARGE_WHOLE the windows that are all but one, all, and more
    than all of the keys, on the rows of one degree."""
    stride = index_stride(P)
    out = [(m, 130, (m + 0.5) / sample_count(130), None) for m in (1, 2, 48)]
    for m in (STAGE_MAX + 1 - stride, STAGE_MAX + 2 - stride, LARGE_PLAIN_M):
        out.append((m, 512, (m + 0.5) / sample_count(512), None))
    for m in (STAGE_MAX + 1 - stride, STAGE_MAX + 2 - stride):
        out.append((m, 64, (m + 0.5) / sample_count(64), SHORT_DEGREES))
    if P == LARGE_WHOLE:
        out += [(m, 130, (m + 0.5) / sample_count(130), [130]) for m in (P - 1, P, P + 1)]
    return out


def stageable(P, m):
    return 0 < m < P and index_stride(P) - 1 + m <= STAGE_MAX


# ---- ties across the window's edge at large strides -------------------------------------------------------------------------------
# Runs of TIE_RUN equal scores (select_ref's m_tie_left / m_tie_right / m_all_equal scaled up: there ONE key sits at the m-th
# distance, or all of them; here a run longer than a wave does): a window's m-th distance falls inside a run on the left, on the
# right, or inside two runs at the same distance on both sides - more than 64 ties, of which the earliest positions in train_pos
# are taken (window_resolve's bisection over positions).
TIE_RUN = 100
TIE_SIZES = [16385, 131073]         # strides 64 and 512
TIE_KINDS = ["on_run", "left_nearer", "midway", "right_nearer", "below", "above", "first_run", "last_run"]


def tie_key_scores(P, run=TIE_RUN):
    """sorted scores: run 0 at 4 units, run 1 at 8, ... (the last run may be shorter); run = P: every key equal"""
    return (4 * (np.arange(P) // run + 1) * UNIT).astype(np.float32)


def tie_centre_scores(P, run=TIE_RUN):
    s = tie_key_scores(P, run)
    mid = float(s[P // 2])
    return {"on_run": np.float32(mid), "left_nearer": np.float32(mid + UNIT), "midway": np.float32(mid + 2 * UNIT),
            "right_nearer": np.float32(mid + 3 * UNIT), "below": np.float32(0.0), "above": np.float32(s[-1] + 4 * UNIT),
            "first_run": s[0], "last_run": s[-1]}


def tie_cases(P, run=TIE_RUN):
    """(m_star, d_star, rho, degrees): windows that end inside a run - part of one run, one run and part of the next two, and
    the staged search's widest window"""
    stride = index_stride(P)
    out = [(m, 130, (m + 0.5) / sample_count(130), None) for m in (run // 2 - 2, run + run // 2)]
    m = STAGE_MAX + 1 - stride
    out.append((m, 512, (m + 0.5) / sample_count(512), None))
    return out


def tie_shape(scores, c, m):
    """(n_lt, T, need_t) of a window: keys strictly nearer than the m-th distance, keys at it, how many of those are taken"""
    dist = np.abs(np.float32(c) - np.asarray(scores, dtype=np.float32)).astype(np.float32)
    ks = np.partition(dist, m - 1)[m - 1]
    n_lt, T = int((dist < ks).sum()), int((dist == ks).sum())
    return n_lt, T, m - n_lt


def nearest_candidates(c, pos_scores, m):
    """Positions (ascending) of the training positives whose distance to c is at most the m-th smallest one - the float32
    subtraction the oracle and the device make.  The m smallest (distance, position) pairs are all among them and keep their
    order, so an oracle handed only these returns the picks of the whole list; its stable sort of all P distances (20 ms at
    262145 keys, once per positive centre and launch) is what this saves.  A list that came out short would make the oracle
    miss picks and the comparison fail."""
    dist = np.abs(np.float32(c) - np.asarray(pos_scores, dtype=np.float32))
    assert dist.dtype == np.float32 and 0 < m < dist.size
    cand = np.flatnonzero(dist <= np.partition(dist, m - 1)[m - 1])
    assert cand.size >= m
    return cand
