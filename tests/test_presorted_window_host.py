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


# ---- the bucket-sorted sizes: strides of 32 .. 1024 ------------------------------------------------------------------------------
def test_large_index_shape():
    assert [R.index_stride(P) for P in R.LARGE_SIZES] == R.LARGE_STRIDES
    for P in R.LARGE_SIZES:
        stride, n_idx = R.index_shape(P)
        print(f"P {P}: stride {stride}, {n_idx} index entries")
        assert 1 <= n_idx <= R.KIDX_MAX and (n_idx - 1) * stride < P <= n_idx * stride
    assert R.index_shape(16384) == (32, 512) and R.index_shape(16385) == (64, 257) and R.index_shape(262145) == (1024, 257)
    assert {R.index_stride(P) for P in R.TIE_SIZES} == {64, 512}


@pytest.mark.parametrize("P", R.LARGE_SIZES)
def test_large_centre_positions_are_what_they_say(P):
    s = R.key_scores(P)
    assert np.all(np.diff(s.astype(np.float64)) == 4 * R.UNIT)                  # exact in float32 up to 262145 keys
    stride, n_idx = R.index_shape(P)
    c = R.centre_scores(P)
    assert c["below"] < s[0] and c["above"] > s[-1] and c["on_key"] in s and c["first"] == s[0] and c["last"] == s[-1]
    at = int(np.flatnonzero(s == c["on_index"])[0])
    assert at % stride == 0 and at > 0
    lo_i = int((s < c["between"]).sum())
    assert c["between"] not in s and (lo_i - 1) // stride == lo_i // stride and lo_i % stride != 0
    assert len(set(np.float32(v) for v in c.values())) == len(c)


@pytest.mark.parametrize("P", R.LARGE_SIZES)
def test_large_cases_reach_both_sides_of_the_staging_switch(P):
    """every row of the GPU test's launches at a large size: the bracket holds the window's start; the rows of degree d_star
    get m_star; the longest single-wave row and a lane row sit on both sides of stride - 1 + m <= 4096; a bracket of three
    probe rounds occurs; at LARGE_WHOLE the whole buffer is a window"""
    s = R.key_scores(P)
    stride, n_idx = R.index_shape(P)
    centres = R.centre_scores(P)
    seen = set()
    for m_star, d_star, rho, degrees in R.large_cases(P):
        assert R.row_m(d_star, rho, P) == min(m_star, P)
        for d in degrees or R.DEGREES:
            m = R.row_m(d, rho, P)
            if m >= P:
                seen.add(("all", d))
                continue
            if m == 0:
                continue
            for name, c in centres.items():
                lo_min, lo_max, t = R.bracket(s, c, m)
                lo = window_start_fast(s, c, m)
                assert 0 <= lo_min <= lo <= lo_max <= P - m, (P, m, name, lo_min, lo, lo_max)
                w = lo_max - lo_min
                assert w <= stride - 1 + m
                assert w <= R.STAGE_MAX or not R.stageable(P, m)
                seen.add((name, "t0" if t == 0 else "tn" if t == n_idx else "mid"))
                if d <= 512:
                    seen.add(("staged" if R.stageable(P, m) else "plain", d <= 64, w))
                seen.add("three_rounds" if w > R.STAGE_MAX else "two_rounds" if w > 64 else "one_round")
    assert ("below", "t0") in seen and ("above", "tn") in seen and ("on_index", "mid") in seen and ("between", "mid") in seen
    for lane_row in (False, True):
        # an interior centre's bracket on either side of the switch: exactly 4096 wide and staged, 4097 wide and not
        assert ("staged", lane_row, R.STAGE_MAX) in seen and ("plain", lane_row, R.STAGE_MAX + 1) in seen, lane_row
    assert {"one_round", "two_rounds", "three_rounds"} <= seen
    assert (("all", 130) in seen) == (P == R.LARGE_WHOLE)
    print(f"P {P}: stride {stride}, m* {[c[0] for c in R.large_cases(P)]}")


@pytest.mark.parametrize("P", R.TIE_SIZES)
def test_tie_cases_put_more_than_a_wave_of_ties_on_the_window_edge(P):
    """the runs table: windows whose m-th distance lies inside a run on the left only, on the right only, and on both sides -
    more than 64 ties, not all of them taken (the bisection over train_pos positions); the brackets hold the start"""
    for run in (R.TIE_RUN, P):
        s = R.tie_key_scores(P, run)
        assert np.all(np.diff(s) >= 0)
        centres = R.tie_centre_scores(P, run)
        assert list(centres) == R.TIE_KINDS
        sides = set()
        for m_star, d_star, rho, degrees in R.tie_cases(P, min(run, R.TIE_RUN)):
            for d in degrees or R.DEGREES:
                m = R.row_m(d, rho, P)
                if m == 0 or m >= P:
                    continue
                for name, c in centres.items():
                    lo_min, lo_max, _ = R.bracket(s, c, m)
                    assert lo_min <= window_start_fast(s, c, m) <= lo_max, (P, run, m, name)
                    n_lt, T, need_t = R.tie_shape(s, c, m)
                    if T > 64 and need_t < T:
                        dist = np.abs(np.float32(c) - s)
                        ks = np.partition(dist, m - 1)[m - 1]
                        left, right = bool(((dist == ks) & (s < c)).any()), bool(((dist == ks) & (s >= c)).any())
                        sides.add((left, right, R.stageable(P, m)))
        if run == P:
            assert sides                                                        # every key is a tie, on one side of the centre
        else:
            assert {(l, r) for l, r, _ in sides} == {(True, False), (False, True), (True, True)}
            assert any(stg for _, _, stg in sides) and any(not stg for _, _, stg in sides)


def test_nearest_candidates_hold_every_pick():
    """the shortened list the large GPU cases hand the oracle: a stable sort of the candidates' distances picks what a stable
    sort of all distances picks, ties by position included"""
    rs = np.random.RandomState(4)
    s = (rs.randint(0, 300, size=5000) * R.UNIT).astype(np.float32)             # many equal scores
    for c in (np.float32(0.0), np.float32(150 * R.UNIT), np.float32(150.5 * R.UNIT), np.float32(1.0)):
        dist = np.abs(c - s)
        full = np.argsort(dist, kind="stable")
        for m in (1, 2, 63, 64, 65, 1000, 4999):
            cand = R.nearest_candidates(c, s, m)
            assert np.all(np.diff(cand) > 0)
            assert np.array_equal(cand[np.argsort(dist[cand], kind="stable")[:m]], full[:m]), (float(c), m)
