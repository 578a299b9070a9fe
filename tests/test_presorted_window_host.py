"""The search index of the sorted train-pos keys (select.hip: key_index_stride, window_bracket) restated in Python, on the CPU:
the bracket [lo_min, lo_max] that the index gives for a centre score contains the start of the window of the m nearest keys, at
every size and centre position tests/test_gpu_presorted_window.py uses - and those cases reach the boundaries they are meant
for (a stride of 32, a bracket wider than one probe round, centres on and between index entries, an empty bracket)."""
import numpy as np
import pytest

from tests import presorted_ref as R


def true_window_start(scores, c, m):
    """first lo in [0, P - m] whose left end is not farther from c than the element right of the window (the search predicate
    of minority_window, in float32 as on the device) - by linear scan"""
    s = np.asarray(scores, dtype=np.float32)
    c = np.float32(c)
    P = s.size
    for lo in range(P - m):
        if not (np.float32(c - s[lo]) > np.float32(s[lo + m] - c)):
            return lo
    return P - m


def window_start_fast(scores, c, m):
    """the same by bisection (the predicate is true on a prefix)"""
    s = np.asarray(scores, dtype=np.float32)
    c = np.float32(c)
    lo, hi = 0, s.size - m
    while lo < hi:
        mid = (lo + hi) // 2
        if np.float32(c - s[mid]) > np.float32(s[mid + m] - c):
            lo = mid + 1
        else:
            hi = mid
    return lo


def test_index_shape():
    assert [R.index_stride(P) for P in (1, 16, 17, 8191, 8192)] == [16] * 5
    assert R.index_stride(8193) == 32 and R.index_stride(16384) == 32 and R.index_stride(16385) == 64
    for P in R.SIZES:
        stride, n_idx = R.index_shape(P)
        assert 1 <= n_idx <= R.KIDX_MAX and (n_idx - 1) * stride < P <= n_idx * stride
    assert R.index_shape(8192) == (16, 512) and R.index_shape(8193) == (32, 257)


def test_bisection_is_the_scan():
    for P in (1, 2, 15, 16, 17, 33, 65):
        s = R.key_scores(P)
        for m in R.m_values(P):
            if m >= P:
                continue
            for name, c in R.centre_scores(P).items():
                assert window_start_fast(s, c, m) == true_window_start(s, c, m), (P, m, name)


@pytest.mark.parametrize("P", R.SIZES)
def test_bracket_contains_the_window_start(P):
    s = R.key_scores(P)
    stride, n_idx = R.index_shape(P)
    centres = R.centre_scores(P)
    seen = set()
    for m in R.m_values(P):
        for name, c in centres.items():
            lo_min, lo_max, t = R.bracket(s, c, min(m, P))
            seen.add((name, t))
            if m >= P:                              # the whole buffer is the window: no search
                continue
            lo = window_start_fast(s, c, m)
            assert 0 <= lo_min <= lo_max <= P - m, (P, m, name)
            assert lo_min <= lo <= lo_max, (P, m, name, lo_min, lo, lo_max)
            assert lo_max - lo_min <= stride + m
            seen.add((name, t))
            if lo_max - lo_min > 64:
                seen.add("two_rounds")
            if lo_max == lo_min:
                seen.add("empty")
    # the positions: below every key (t = 0), above every key (t = n_idx), on a key, on an index entry, between two entries
    assert ("below", 0) in seen and ("above", n_idx) in seen
    assert any(n == "on_key" for n, _ in [x for x in seen if isinstance(x, tuple)])
    if n_idx >= 3:
        assert any(n == "on_index" and 0 < t < n_idx for n, t in [x for x in seen if isinstance(x, tuple)])
        assert any(n == "between" and 0 < t < n_idx for n, t in [x for x in seen if isinstance(x, tuple)])
    if P > 1 and (P - 1) % stride == 0:
        assert "empty" in seen                      # a centre above every key, the last index entry alone in its stride
    # an interior bracket is stride - 1 + m wide: with a stride of 16 the m of this list stay within one probe round of 64
    # (m = 49: exactly 64), with a stride of 32 they take a second one
    assert ("two_rounds" in seen) == (stride - 1 + 49 > 64 and P > 200)


def test_gpu_batches_reach_every_search_regime():
    """the rows of the GPU test's launches (their m follows from the row's degree): brackets of one probe round, of two, and
    beyond two (the staged search hands over to the plain one), and windows that are the whole buffer"""
    seen = set()
    for P in R.SIZES + [R.PLAIN_SIZE]:
        s = R.key_scores(P)
        for m_star, d_star, rho in R.gpu_cases(P):
            assert R.row_m(d_star, rho, P) == min(m_star, P)
            for d in R.DEGREES:
                m = R.row_m(d, rho, P)
                if m >= P:
                    seen.add(("all", d > 512))
                    continue
                for c in R.centre_scores(P).values():
                    lo_min, lo_max, _ = R.bracket(s, c, m)
                    assert lo_min <= window_start_fast(s, c, m) <= lo_max
                    w = lo_max - lo_min
                    assert w <= 4096 or P == R.PLAIN_SIZE
                    seen.add(("none" if w == 0 else "one" if w <= 64 else "two" if w <= 4096 else "plain", d <= 64, d > 512))
    for regime in ("none", "one", "two"):
        for lane_row, wg_row in ((True, False), (False, False), (False, True)):
            assert (regime, lane_row, wg_row) in seen, (regime, lane_row, wg_row)
    assert ("plain", False, False) in seen and ("all", False) in seen and ("all", True) in seen


def test_centre_positions_are_what_they_say():
    for P in R.SIZES:
        s = R.key_scores(P)
        stride, n_idx = R.index_shape(P)
        c = R.centre_scores(P)
        assert c["below"] < s[0] and c["above"] > s[-1]
        assert c["on_key"] in s and c["first"] == s[0] and c["last"] == s[-1]
        if n_idx >= 3:
            at = int(np.flatnonzero(s == c["on_index"])[0])
            assert at % stride == 0 and at > 0
            lo_i = int((s < c["between"]).sum())
            assert c["between"] not in s and (lo_i - 1) // stride == lo_i // stride and lo_i % stride != 0
        assert len(set(np.float32(v) for v in c.values())) >= min(len(c), 3)


def test_m_values():
    assert R.m_values(1) == [1, 2]
    assert R.m_values(17) == [1, 2, 16, 17, 18]
    assert R.m_values(8193) == [1, 2, 47, 48, 49, 8192, 8193, 8194]
    assert R.index_stride(64) + 48 == 64 and R.index_stride(64) + 49 > 64
