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
