"""Crafted score tables for the neighbour selection (select.hip) and a host model that says what each of them reaches.

With a centre whose score is +0.0 the distance key of neighbour j is the bit pattern of ``s0[j]``, so a test dictates every key
bit for bit.  ``histogram_rounds`` is a plain model of the selection's round loop ("narrow [lo, hi] by ``hbits`` bits per round
while more than 64 keys remain").  It QUALIFIES inputs - it shows that a case reaches the branch it is meant for - and is never the
expected result: expected sets come from the oracle (``oracle.pcgnn_oracle.choose_sets``) or from a ``lexsort`` on the key bits.

Numpy only; tests/test_select_ref_host.py asserts the coverage, tests/test_gpu_select_keys.py runs the cases on the GPU.
"""
import math
from collections import namedtuple

import numpy as np

WAVE = 64
# the tier limits of the selection (choose.h: TA_CAP, TB_CAP, T1_CAP, T4_CAP, WG_KEYCAP, LONG_KEYCAP), each +-1; 130: the smallest
# length that reaches four rounds; 1100: a workgroup row whose wave stretches are not all full
LENGTHS = [4, 5, 16, 17, 63, 64, 65, 66, 130, 511, 512, 513, 1100, 4096, 4097, 10240, 10241, 32768, 32769]
LONG_LENGTHS = [10241, 32768, 32769]
POOL = max(LENGTHS)
KEY_MIN, KEY_MAX = 0x00800000, 0x7F000000          # normal floats only: no denormal handling is involved
BASE = 0x3F800000 + 0x5A5A5A                       # aligned to no round's bin width
TIERS = {8: (65, 512), 11: (513, 10240), 12: (10241, 32769)}


def hbits_of(d):
    """Histogram bits per round of a row of d neighbours: 8 on one wave, 11 on an 8-wave workgroup, 12 on the 16-wave long-row
    launch; None for the rows that are ranked lane against lane (no k-th value is formed)."""
    if d <= WAVE:
        return None
    return 8 if d <= 512 else (11 if d <= 10240 else 12)


def sample_count(d, thr):
    return math.ceil(d * thr)


Rounds = namedtuple("Rounds", "n_rounds shifts bins ending n_equal need")


def histogram_rounds(keys, k, hbits):
    """The round loop on `keys` (uint32) for the k-th smallest (k 1-based): per round its shift and the bin it chose; how the loop
    ended - 'rank' (at most 64 candidates left in lo < hi: they are ranked in one wave) or 'exact' (lo == hi: the k-th key itself);
    n_equal = #keys equal to the k-th key, need = how many of those belong to the k smallest."""
    keys = np.asarray(keys, dtype=np.uint32).astype(np.int64)
    lo, hi = int(keys.min()), int(keys.max())
    below, cnt = 0, keys.size
    shifts, bins = [], []
    while lo < hi and cnt > WAVE:
        shift = max((hi - lo).bit_length() - hbits, 0)
        inside = keys[(keys >= lo) & (keys <= hi)]
        hist = np.bincount((inside - lo) >> shift, minlength=1 << hbits)
        assert hist.size == 1 << hbits
        cum = np.cumsum(hist)
        b = int(np.searchsorted(cum, k - below, side="left"))
        below += int(cum[b] - hist[b])
        cnt = int(hist[b])
        lo += b << shift
        hi = min(lo + (1 << shift) - 1, hi)
        shifts.append(shift)
        bins.append(b)
    kstar = int(np.sort(keys)[k - 1])
    n_equal = int((keys == kstar).sum())
    need = k - int((keys < kstar).sum())
    if lo == hi:
        assert lo == kstar and cnt == n_equal and k - below == need
    return Rounds(len(shifts), tuple(shifts), tuple(bins), "exact" if lo == hi else "rank", n_equal, need)


def lexsort_set(keys, k):
    """Positions of the k smallest keys, ties to the earlier position (what a stable sort of the distances keeps)."""
    keys = np.asarray(keys, dtype=np.uint32)
    return set(np.lexsort((np.arange(keys.size), keys))[:k].tolist())


# ---------------------------------------------------------------------------------------------------------------------------
# key families: (d, rng) -> uint32 keys of a row of d neighbours
# ---------------------------------------------------------------------------------------------------------------------------
def nested(w, low=KEY_MIN):
    """Two outliers at the ends of the 31-bit range (positions 0 and 1), the other d - 2 keys uniform in [base, base + 2^w): the
    first round isolates the cluster, the later ones pick non-zero bins (base is aligned to 2^w and to nothing coarser that a
    round uses)."""
    def family(d, rng):
        base = BASE & ~((1 << w) - 1)
        keys = (base + rng.integers(0, 1 << w, size=d, dtype=np.int64)).astype(np.uint32)
        keys[0] = low
        if d > 1:
            keys[1] = KEY_MAX
        return keys
    return family


def all_equal(d, rng):
    return np.full(d, BASE, dtype=np.uint32)


def two_values(p):
    """a and a + 1, a fraction p of a at random positions: with k = d / 2 the cut falls inside the run of a (p = 0.6) or inside
    the run of a + 1 (p = 0.3)."""
    def family(d, rng):
        return (BASE + (rng.random(d) >= p)).astype(np.uint32)
    return family


def cut_tie(thr):
    """Distinct keys, except exactly two equal ones at ranks k and k + 1 (k = ceil(d * thr)), far apart in position (d // 20 and
    d - 1 - d // 20: the first and the last wave's stretch of a workgroup row).  Only the earlier one is kept.  The smallest and
    the largest key are the ends of the 31-bit range, so the tie is found in a second or third round."""
    def family(d, rng):
        k = sample_count(d, thr)
        vals = np.sort(rng.choice(8 * d, size=d, replace=False)) + (BASE & ~0xFFF)
        vals[0], vals[-1] = KEY_MIN, KEY_MAX            # the ends of the 31-bit range: a first round that only finds the cluster
        if d > k + 1:
            vals[k] = vals[k - 1]                       # (0-based: ranks k and k + 1)
        a, b = d // 20, d - 1 - d // 20
        order = rng.permutation(d)
        if d > k + 1 and a != b:                        # the two equal keys go to positions a and b
            for rank, pos in ((k - 1, a), (k, b)):
                j = int(np.flatnonzero(order == pos)[0])
                order[j], order[rank] = order[rank], order[j]
        keys = np.empty(d, dtype=np.uint32)
        keys[order] = vals
        return keys
    return family


def ramp(descending, outliers):
    """base + position (or base + (POOL - 1 - position)): distinct keys, adjacent in bits, so the shift == 0 round runs with one
    key per bin.  outliers: positions 0 and 1 hold the ends of the 31-bit range, which puts three rounds before that one."""
    def family(d, rng):
        pos = np.arange(d, dtype=np.int64)
        keys = ((BASE & ~0xFFFF) + 0x4000 + (POOL - 1 - pos if descending else pos)).astype(np.uint32)
        if outliers and d > 1:
            keys[0], keys[1] = KEY_MIN, KEY_MAX
        return keys
    return family


zero_first = nested(12, low=0)      # one key of distance 0 (the centre in its own row): the range starts at 0

THR_EDGE = [q / d for d in (512, 10240, 32769) for q in (0.5, 1.5, d - 2.5)]     # k = 1, 2, d - 2 at the top of every tier
KeyFamily = namedtuple("KeyFamily", "name make prefix lengths thresholds")
# prefix: one table of POOL keys serves every length (a row is its first d keys); otherwise one table per length
_SHORT = [d for d in LENGTHS if d <= 10240]
KEY_FAMILIES = [
    KeyFamily("nested23", nested(23), True, _SHORT, [0.5]),
    KeyFamily("nested20", nested(20), True, _SHORT, [0.5]),
    KeyFamily("nested15", nested(15), True, _SHORT, [0.5, 0.27]),
    KeyFamily("nested12", nested(12), True, _SHORT, [0.5]),
    KeyFamily("nested9", nested(9), True, LENGTHS, [0.5] + THR_EDGE),
    KeyFamily("nested7", nested(7), True, _SHORT, [0.5, 0.27]),
    KeyFamily("nested6", nested(6), True, _SHORT, [0.5]),
    KeyFamily("nested3", nested(3), True, _SHORT, [0.5, 0.8]),
    KeyFamily("nested0", nested(0), True, LENGTHS, [0.5, 0.27]),
    KeyFamily("all_equal", all_equal, True, _SHORT, [0.5, 0.27]),
    KeyFamily("two_values_a", two_values(0.6), True, LENGTHS, [0.5]),
    KeyFamily("two_values_a1", two_values(0.3), True, LENGTHS, [0.5]),
    KeyFamily("cut_tie", cut_tie(0.5), False, LENGTHS, [0.5]),
    KeyFamily("ramp_down", ramp(True, False), True, _SHORT, [0.5] + THR_EDGE[:6]),
    KeyFamily("ramp_up_out", ramp(False, True), True, _SHORT, [0.5, 0.27]),
    KeyFamily("ramp_down_out", ramp(True, True), True, _SHORT, [0.5, 0.27]),
    KeyFamily("zero_first", zero_first, True, _SHORT, [0.5]),
]
KEY_FAMILY = {f.name: f for f in KEY_FAMILIES}


def family_tables(fam, seed=20):
    """{d: keys of the row of length d} - for a prefix family every row is the head of one table of POOL keys."""
    rng = np.random.default_rng([seed, sum(map(ord, fam.name))])
    if fam.prefix:
        table = fam.make(POOL, rng)
        return {d: table[:d] for d in fam.lengths}
    return {d: fam.make(d, rng) for d in fam.lengths}


def boundary_threshold(keys):
    """A threshold near 0.5 whose cut falls between two different keys of the row: every key equal to the k-th one is kept
    (n_equal == need)."""
    d = keys.size
    srt = np.sort(keys)
    k = next(k for k in range(d // 2, d - 2) if srt[k - 1] != srt[k])
    return (k - 0.5) / d


def family_thresholds(fam, tables):
    """the family's thresholds; nested9 adds one per tier whose cut falls on a boundary between two key values"""
    if fam.name != "nested9":
        return list(fam.thresholds)
    return list(fam.thresholds) + [boundary_threshold(tables[d]) for d in (512, 10240, 32769)]


def key_cases(fam, seed=20):
    """Every (d, threshold, k, keys) of a family that goes through the k-th-key search (d > k + 1; the others keep every id)."""
    out = []
    tables = family_tables(fam, seed)
    for d, keys in tables.items():
        for thr in family_thresholds(fam, tables):
            k = sample_count(d, thr)
            if d > k + 1:
                out.append((d, thr, k, keys))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# minority families: (P, rng) -> (scores of the P training positives in train_pos order, centre score, m), or None where the
# family makes no sense at that P.  Scores are multiples of 2^-10 (every distance is exact in float32); which position holds
# which score is a random permutation, so the two sides of the centre are interleaved in train_pos.
# ---------------------------------------------------------------------------------------------------------------------------
UNIT = 2.0 ** -10
CENTRE = 384 * UNIT
MINORITY_P = [1, 2, 63, 64, 65, 300, 4097]
MINORITY_ROWS = [20, 300, 600, 10241]        # finish_row<1> from a lane row and a wave row, finish_row<8> (window by the last wave), <16>


def _scores(offsets, rng, shuffle=True):
    off = np.asarray(offsets, dtype=np.int64)
    if shuffle:
        off = off[rng.permutation(off.size)]
    return (CENTRE + off * UNIT).astype(np.float32)


def _distinct(P, rng, mth_sign=0, m=None):
    """offsets of distinct magnitude 1 .. P with random signs; the one of magnitude m gets mth_sign (if not 0)"""
    off = np.arange(1, P + 1) * rng.choice([-1, 1], size=P)
    if mth_sign and m:
        off[m - 1] = mth_sign * m
    return off


def m_interior(P, rng):
    m = P // 2
    return (_scores(_distinct(P, rng), rng), CENTRE, m) if m >= 2 else None


def m_tie_left(P, rng):
    m = P // 2
    return (_scores(_distinct(P, rng, -1, m), rng), CENTRE, m) if m >= 2 else None


def m_tie_right(P, rng):
    m = P // 2
    return (_scores(_distinct(P, rng, +1, m), rng), CENTRE, m) if m >= 2 else None


def m_one_unique(P, rng):
    return (_scores(_distinct(P, rng), rng), CENTRE, 1) if P >= 2 else None


def m_one_pair(P, rng):
    if P < 3:
        return None
    off = _distinct(P, rng)
    off[0], off[1] = -1, 1
    return _scores(off, rng), CENTRE, 1


def _sym_ties(n_side, need_t):
    def family(P, rng):
        if P < 2 * n_side + 10:
            return None
        n_lt = min(20, P - 2 * n_side - 5)
        far = P - n_lt - 2 * n_side
        D = n_lt + 1
        off = np.concatenate([_distinct(n_lt, rng), np.full(n_side, -D), np.full(n_side, D),
                              (D + 1 + np.arange(far)) * rng.choice([-1, 1], size=far)])
        return _scores(off, rng), CENTRE, n_lt + need_t
    return family


m_ties_10 = _sym_ties(10, 7)         # T = 20 <= 64: ranked in registers
m_ties_100 = _sym_ties(100, 75)      # T = 200 > 64: bisection on the train_pos position


def m_all_equal(P, rng):
    m = P // 2
    return (_scores(np.full(P, 3), rng), CENTRE, m) if m >= 1 else None


def m_centre_below(P, rng):
    m = P // 2
    return (_scores(np.arange(1, P + 1), rng), CENTRE, m) if m >= 1 else None


def m_centre_above(P, rng):
    m = P // 2
    return (_scores(-np.arange(1, P + 1), rng), CENTRE, m) if m >= 1 else None


def m_all_but_one(P, rng):
    return (_scores(_distinct(P, rng), rng), CENTRE, P - 1) if P >= 2 else None


def m_all(P, rng):
    return _scores(_distinct(P, rng), rng), CENTRE, P


def m_more_than_all(P, rng):
    return _scores(_distinct(P, rng), rng), CENTRE, P + 5


def m_in_row(P, rng):
    """the training positives that are neighbours of the centre (the first of train_pos, see minority_train_pos) are its
    nearest ones: they are kept as neighbours AND picked, so the list keeps a -1 hole for each"""
    n_in = len(minority_in_row(P))
    if n_in < 2:
        return None
    off = _distinct(P, rng)
    head = _scores(off[:n_in], rng, shuffle=False)
    return np.concatenate([head, _scores(off[n_in:], rng)]), CENTRE, max(P // 2, n_in)


MINORITY_FAMILIES = {
    "interior": m_interior, "tie_left": m_tie_left, "tie_right": m_tie_right, "one_unique": m_one_unique,
    "one_pair": m_one_pair, "ties_10": m_ties_10, "ties_100": m_ties_100, "all_equal": m_all_equal,
    "centre_below": m_centre_below, "centre_above": m_centre_above, "all_but_one": m_all_but_one, "all": m_all,
    "more_than_all": m_more_than_all, "in_row": m_in_row,
}
# where each family has to land (minority_branch)
MINORITY_BRANCH = {
    "interior": {"single"}, "tie_left": {"single"}, "tie_right": {"single"}, "one_unique": {"single"}, "one_pair": {"ranked"},
    "ties_10": {"ranked"}, "ties_100": {"bisect"}, "all_equal": {"ranked", "bisect"}, "centre_below": {"single"},
    "centre_above": {"single"}, "all_but_one": {"single"}, "all": {"all"}, "more_than_all": {"all"}, "in_row": {"single"},
}
POS_BASE = 12000            # the training positives that are nobody's neighbour in the minority rows (ids beyond the longest row)


def minority_in_row(P):
    """ids of the training positives inside every minority row (even ids below 16)"""
    return list(range(0, 16, 2))[:min(8, P // 3)]


def minority_train_pos(P):
    head = minority_in_row(P)
    return head + list(range(POS_BASE, POS_BASE + P - len(head)))


def minority_cases(P, seed=20):
    """{family name: (scores, centre, m)} of the families that make sense at P"""
    out = {}
    for name, fam in MINORITY_FAMILIES.items():
        case = fam(P, np.random.default_rng([seed, P, sum(map(ord, name))]))
        if case is not None:
            out[name] = case
    return out


def distance_bits(scores, c):
    return np.abs(np.float32(c) - np.asarray(scores, dtype=np.float32)).astype(np.float32).view(np.uint32)


def minority_branch(scores, c, m):
    """Where the specification puts a case: the m-th smallest distance, n_lt strictly nearer, T at that distance, need_t of them
    taken -> 'all' (m >= P), 'single' (T == 1), 'taken' (every tie is taken), 'ranked' (T <= 64), 'bisect' (T > 64)."""
    dist = distance_bits(scores, c)
    P = dist.size
    if m >= P:
        return "all", P, 0, 0, 0
    ks = np.sort(dist)[m - 1]
    n_lt, T = int((dist < ks).sum()), int((dist == ks).sum())
    need_t = m - n_lt
    name = "single" if T == 1 else "taken" if T == need_t else "ranked" if T <= WAVE else "bisect"
    return name, int(ks), n_lt, T, need_t


def minority_picks(scores, c, m):
    """train_pos positions of the m nearest positives, ties to the earlier position"""
    dist = distance_bits(scores, c)
    return np.lexsort((np.arange(dist.size), dist))[:m]


def minority_score_table(n_nodes, train_pos, scores, c, centres, rng):
    """A score table for a minority case: the positives get their scores, the centres c, every other node a score at least
    4.0 away from c (so a positive inside a row is nearer than its other neighbours)."""
    off = (4096 + rng.integers(0, 4096, size=n_nodes)) * rng.choice([-1, 1], size=n_nodes)
    s0 = (np.float32(c) + off * UNIT).astype(np.float32)
    s0[np.asarray(train_pos, dtype=np.int64)] = scores
    s0[np.asarray(centres, dtype=np.int64)] = np.float32(c)
    return s0
