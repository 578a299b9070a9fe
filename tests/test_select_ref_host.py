"""CPU-only tests of the crafted selection inputs (tests/select_ref.py): the host model of the round loop on hand-made keys, the
coverage each tier's cases promise - recomputed from the cases themselves -, where every minority case lands, and the oracle
against a lexsort on the key bits for every case the GPU tests run."""
import numpy as np
import pytest
import torch

from oracle import pcgnn_oracle as O
from tests import select_ref as S


def test_round_model_on_hand_made_keys():
    # 100 keys 1000 .. 1099 and two outliers: 8 bits per round
    keys = np.concatenate([[S.KEY_MIN, S.KEY_MAX], 0x3F800000 + 1000 + np.arange(100)]).astype(np.uint32)
    r = S.histogram_rounds(keys, 51, 8)
    # round 1: 31 bits -> shift 23, the cluster's bin; round 2: 23 bits -> shift 15, bin 0; round 3: shift 7, 1000 .. 1099 spans
    # bins 7 (24 keys: 1000 .. 1023) and 8 (76 keys); the 50th cluster key, 1049, is in bin 8: 76 > 64 -> round 4, shift 0
    assert r.shifts == (23, 15, 7, 0) and r.bins == ((0x3F800000 - S.KEY_MIN) >> 23, 0, 8, 1049 - 1024)
    assert (r.ending, r.n_equal, r.need) == ("exact", 1, 1)
    r = S.histogram_rounds(keys, 12, 8)                # 1010: bin 7 of round 3 holds 24 keys -> ranked
    assert r.shifts == (23, 15, 7) and r.bins[2] == 7 and r.ending == "rank"
    r = S.histogram_rounds(np.full(200, 77, dtype=np.uint32), 9, 11)
    assert (r.n_rounds, r.ending, r.n_equal, r.need) == (0, "exact", 200, 9)
    r = S.histogram_rounds(np.array([5] * 70 + [6] * 70, dtype=np.uint32), 100, 12)
    assert (r.shifts, r.bins, r.ending, r.n_equal, r.need) == ((0,), (1,), "exact", 70, 30)
    assert S.lexsort_set(np.array([3, 1, 3, 1, 2], dtype=np.uint32), 4) == {1, 3, 4, 0}


@pytest.fixture(scope="module")
def qualified():
    """[(family, d, thr, k, keys, Rounds)] of every case that goes through the round loop"""
    out = []
    for fam in S.KEY_FAMILIES:
        for d, thr, k, keys in S.key_cases(fam):
            hb = S.hbits_of(d)
            if hb is not None:
                out.append((fam.name, d, thr, k, keys, S.histogram_rounds(keys, k, hb)))
    return out


def test_keys_are_normal_floats():
    for fam in S.KEY_FAMILIES:
        for d, keys in S.family_tables(fam).items():
            assert keys.dtype == np.uint32 and keys.size == d
            body = keys[keys != 0] if fam.name == "zero_first" else keys
            assert body.min() >= S.KEY_MIN and body.max() <= S.KEY_MAX
            if fam.name == "zero_first":
                assert keys[0] == 0 and (keys[1:] != 0).all()
    assert sorted({d for f in S.KEY_FAMILIES for d in f.lengths}) == S.LENGTHS
    assert {f.name for f in S.KEY_FAMILIES if set(S.LONG_LENGTHS) & set(f.lengths)} == \
        {"nested9", "nested0", "two_values_a", "two_values_a1", "cut_tie"}


@pytest.mark.parametrize("hbits,round_counts", [(8, (2, 3, 4)), (11, (2, 3)), (12, (2, 3))])
def test_every_tier_reaches_every_round_and_tie_shape(qualified, hbits, round_counts):
    lo, hi = S.TIERS[hbits]
    tier = [q for q in qualified if lo <= q[1] <= hi]
    assert {q[1] for q in tier} == {d for d in S.LENGTHS if lo <= d <= hi}
    rounds = [q[5] for q in tier]
    for n in round_counts:
        assert any(r.n_rounds == n for r in rounds), f"no case with {n} rounds"
    assert any(r.n_rounds >= 2 and r.ending == "rank" for r in rounds)
    assert any(r.n_rounds >= 2 and r.ending == "exact" and r.n_equal == r.need for r in rounds)
    assert any(r.n_rounds >= 2 and r.ending == "exact" and r.n_equal > r.need for r in rounds)
    assert any(r.ending == "rank" and r.n_equal > r.need for r in rounds), "a tie across the cut among ranked candidates"
    assert any(r.n_rounds >= 2 and all(b != 0 for b in r.bins[1:]) for r in rounds)
    assert any(r.n_rounds == max(round_counts) and all(b != 0 for b in r.bins[1:]) for r in rounds)
    assert any(r.n_rounds >= 2 and r.shifts[-1] == 0 for r in rounds)
    # every later shift the tier can take is taken with a non-zero bin: 31 bits -> hbits per round
    later = {8: {15, 7, 0}, 11: {9, 0}, 12: {7, 0}}[hbits]
    seen = {s for r in rounds for s, b in zip(r.shifts[1:], r.bins[1:]) if b != 0}
    assert later <= seen
    if hbits < 12:       # (the long rows run four families only: none of them has distinct keys in its last round)
        assert any(r.n_rounds >= 2 and r.shifts[-1] == 0 and np.unique(q[4]).size == q[4].size for q, r in zip(tier, rounds))
    for want in (1, 2):
        assert any(q[3] == want for q in tier), f"k = {want}"
    assert any(q[3] == q[1] - 2 for q in tier), "k = d - 2"
    # n_equal from a single key up to the whole cluster
    assert any(r.n_equal == 1 for r in rounds) and any(r.n_equal == q[1] - 2 for q, r in zip(tier, rounds))


def test_families_reach_what_they_are_named_for(qualified):
    by = {}
    for name, d, thr, k, keys, r in qualified:
        by.setdefault(name, []).append((d, k, keys, r))
    for d, k, keys, r in by["all_equal"]:
        assert (r.n_rounds, r.ending, r.n_equal, r.need) == (0, "exact", d, k)
    for name, inside_a in (("two_values_a", True), ("two_values_a1", False)):
        for d, k, keys, r in by[name]:
            n_a = int((keys == keys.min()).sum())
            assert r.ending == "exact" and 0 < r.need < r.n_equal
            assert (k < n_a) if inside_a else (k > n_a)
    for d, k, keys, r in by["cut_tie"]:
        assert (r.n_equal, r.need) == (2, 1) and (r.n_rounds >= 2 or d < 130)      # (65, 66: the cluster is 64 keys at most)
        a, b = np.flatnonzero(keys == np.sort(keys)[k - 1])
        assert (a, b) == (d // 20, d - 1 - d // 20)
        if d > 512:         # a workgroup row: the two are in the first and in one of the last two waves' stretches
            nw = 8 if d <= 10240 else 16
            seg = (-(-d // nw) + 63) & ~63
            assert a // seg == 0 and b // seg >= max(-(-d // seg) - 2, 1)
    for name in ("ramp_down", "ramp_up_out", "ramp_down_out"):
        for d, k, keys, r in by[name]:
            assert np.unique(keys).size == d
            if name.endswith("_out") and d >= 130:
                assert r.shifts[-1] == 0 and r.ending == "exact" and r.n_rounds == (4 if d <= 512 else 3)
    assert any(r.shifts == (0,) and r.ending == "exact" for d, k, keys, r in by["ramp_down"]), "one round, one key per bin"
    for d, k, keys, r in by["zero_first"]:
        assert keys.min() == 0 and (r.n_rounds >= 2 or d < 130)


def test_oracle_equals_lexsort_on_every_key_case():
    c0 = torch.zeros(())
    n = 0
    for fam in S.KEY_FAMILIES:
        for d, thr, k, keys in S.key_cases(fam):
            assert O.sample_count(d, thr) == k
            got = O.choose_row(c0, range(d), torch.from_numpy(keys.view(np.float32).copy()), k)
            assert got == S.lexsort_set(keys, k), (fam.name, d, thr)
            n += 1
    assert n > 400


# ---------------------------------------------------------------------------------------------------------------------------
def test_minority_cases_land_where_their_names_say():
    seen = {}
    for P in S.MINORITY_P:
        cases = S.minority_cases(P)
        tp = S.minority_train_pos(P)
        assert len(tp) == P == len(set(tp))
        for name, (scores, c, m) in cases.items():
            assert scores.dtype == np.float32 and scores.size == P and m >= 1
            assert np.array_equal(np.round(scores.astype(np.float64) * 1024), scores.astype(np.float64) * 1024)
            branch, ks, n_lt, T, need_t = S.minority_branch(scores, c, m)
            assert branch in S.MINORITY_BRANCH[name], (name, P, branch)
            seen.setdefault(name, {})[P] = (branch, n_lt, T, need_t)
            dist = S.distance_bits(scores, c)
            picks = S.minority_picks(scores, c, m)
            side = np.sign(scores.astype(np.float64) - c)
            last = picks[-1] if m <= P else None
            if name == "tie_left":
                assert side[last] < 0
            if name == "tie_right":
                assert side[last] > 0
            if name in ("interior", "tie_left", "tie_right", "all_but_one"):
                assert P < 8 or (set(side[picks]) == {-1.0, 1.0} and set(side) == {-1.0, 1.0}), "both sides of the centre"
            if name == "one_pair":
                assert (T, need_t, m) == (2, 1, 1) and sorted(side[dist == ks]) == [-1, 1]
            if name == "ties_10":
                assert (T, need_t) == (20, 7) and (side[dist == ks] < 0).sum() == 10
            if name == "ties_100":
                assert (T, need_t) == (200, 75) and (side[dist == ks] < 0).sum() == 100
            if name == "all_equal":
                assert T == P and need_t == m and n_lt == 0
            if name == "centre_below":
                assert (side > 0).all()
            if name == "centre_above":
                assert (side < 0).all()
            if name == "all_but_one":
                assert m == P - 1
            if name == "more_than_all":
                assert m > P
            if name == "in_row":
                n_in = len(S.minority_in_row(P))
                assert n_in >= 2 and set(range(n_in)) <= set(picks.tolist()), "the positives inside the row are picked"
    # every family runs at every size of the 64-ary search it makes sense for
    assert set(seen["interior"]) == {63, 64, 65, 300, 4097} and set(seen["all"]) == set(S.MINORITY_P)
    assert set(seen["ties_10"]) == {63, 64, 65, 300, 4097} and set(seen["ties_100"]) == {300, 4097}
    assert set(seen["one_pair"]) == {63, 64, 65, 300, 4097} and set(seen["all_equal"]) == {2, 63, 64, 65, 300, 4097}
    assert {seen["all_equal"][P][0] for P in (2, 63, 64)} == {"ranked"} and {seen["all_equal"][P][0] for P in (65, 300, 4097)} == {"bisect"}
    assert set(seen["in_row"]) == {63, 64, 65, 300, 4097} and set(seen["one_unique"]) == set(S.MINORITY_P) - {1}


def test_oracle_equals_lexsort_on_every_minority_case():
    for P in S.MINORITY_P:
        tp = S.minority_train_pos(P)
        for name, (scores, c, m) in S.minority_cases(P).items():
            got = O.choose_row(torch.tensor(c, dtype=torch.float32), [], torch.zeros(0), 0, (tp, torch.from_numpy(scores), m))
            want = {tp[i] for i in S.minority_picks(scores, c, m).tolist()}
            assert got == want and len(want) == min(m, P), (name, P)
