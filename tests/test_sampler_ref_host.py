"""tests/sampler_ref.py (the host reference the GPU sampler tests compare with) against what is published and what can be
worked out by hand: the Philox4x32-10 known-answer vectors of the Random123 distribution (kat_vectors), the 53-bit uniform,
and bisect_right's behaviour on cumulative weights with runs of equal values.  No GPU."""
import bisect
import struct

import numpy as np
import pytest

from tests import sampler_ref as S

KAT = [  # counter, key, output (Random123 kat_vectors: philox4x32 10)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def bits(x: float) -> bytes:
    return struct.pack("<d", x)


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    assert S.philox4x32_10(counter, key) == want


def test_counter_and_key_layout():
    """counter = (draw, 0, epoch low, epoch high), key = (seed low, seed high): the high words of both arguments are used"""
    assert S.counter_key(0, 0, 0) == ((0, 0, 0, 0), (0, 0))
    assert S.counter_key(2 ** 32 + 5, 2 ** 40 + 3, 9) == ((9, 0, 3, 256), (5, 1))
    assert S.counter_key(2 ** 63 + 1, 2 ** 32 + 7, 0xFFFFFFFF) == ((0xFFFFFFFF, 0, 7, 1), (1, 2 ** 31))


def test_uniform_is_the_53_bit_construction():
    # draw 0 of (seed 0, epoch 0) is the all-zero known-answer vector: a = 0x6627e8d5 >> 5, b = 0xe169c58d >> 6
    a, b = 0x6627e8d5 >> 5, 0xe169c58d >> 6
    assert (a, b) == (0x03313F46, 0x0385A716)
    want = (a * 67108864 + b) / 9007199254740992
    assert bits(S.uniform(0, 0, 0)) == bits(want) and 0.0 <= want < 1.0
    assert bits(want) == bits((a * 2 ** 26 + b) * 2.0 ** -53) and (a * 2 ** 26 + b) < 2 ** 53      # (an exact integer, scaled)
    # other counters, the formula applied by hand to the words of philox4x32_10 on the counter / key written out
    for (seed, epoch, draw), (counter, key) in (((2 ** 32 + 5, 2 ** 40 + 3, 9), ((9, 0, 3, 256), (5, 1))),
                                                ((11, 100, 999), ((999, 0, 100, 0), (11, 0))),
                                                ((2 ** 63 + 1, 2 ** 32 + 7, 1), ((1, 0, 7, 1), (1, 2 ** 31)))):
        c = S.philox4x32_10(counter, key)
        want = ((c[0] >> 5) * 2 ** 26 + (c[1] >> 6)) / 2 ** 53
        assert bits(S.uniform(seed, epoch, draw)) == bits(want)
    # the extremes of the construction: all-zero words give 0, all-one words the largest double below 1
    assert (0 * 2 ** 26 + 0) / 2 ** 53 == 0.0
    top = ((0xFFFFFFFF >> 5) * 2 ** 26 + (0xFFFFFFFF >> 6)) / 2 ** 53
    assert top == 1.0 - 2.0 ** -53 and top < 1.0


@pytest.mark.parametrize("seed,epoch", [(0, 0), (11, 100), (2 ** 32 + 5, 3), (2 ** 63 + 1, 2 ** 32 + 7), (5, 2 ** 40)])
def test_vectorised_uniforms_equal_the_scalar_ones(seed, epoch):
    u = S.uniforms(seed, epoch, 300)
    assert u.dtype == np.float64 and ((0.0 <= u) & (u < 1.0)).all()
    assert [bits(float(x)) for x in u] == [bits(S.uniform(seed, epoch, i)) for i in range(300)]
    assert len(np.unique(u)) == 300
    assert abs(float(u.mean()) - 0.5) < 0.1              # (300 uniforms: sigma of the mean = 0.017)


def test_picks_follow_random_choices():
    """picks == random.choices' own arithmetic (bisect over the running sum, hi = n - 1) given the same uniforms"""
    rs = np.random.RandomState(0)
    w = S.positive_weights(50, rs)
    cum = np.cumsum(w)
    idx = np.arange(50) * 3 + 1
    u = S.uniforms(4, 2, 200)
    want = [int(idx[bisect.bisect(list(cum), float(x) * float(cum[-1]), 0, 49)]) for x in u]
    assert S.picks(cum, idx, 4, 2, 200).tolist() == want
    assert len(set(want)) > 25


@pytest.mark.parametrize("n", [1, 2, 3, 15, 16, 17, 18, 255, 256, 257, 4095, 4096, 4097, 65537])
def test_zero_weight_entries_are_never_picked_but_by_the_clip(n):
    """The zero-run weight vectors of the GPU test: about half zero, zero at both ends, a run of 40 from n = 100 on.  The
    reference never returns an entry of weight zero - x = u * cum[-1] < cum[-1] always, and bisect_right steps over equal
    values - except when NOTHING is positive (n <= 2): cum is all zero and the hi = n - 1 clip returns the last index."""
    rs = np.random.RandomState(n)
    w = S.weights_with_zero_runs(n, rs)
    assert w[0] == 0.0 and w[-1] == 0.0
    cum = np.cumsum(w)
    pos = S.positions(cum, 7, 1, 2000)
    if n <= 2:
        assert not w.any() and (pos == n - 1).all()
        return
    assert 0.3 < (w == 0).mean() < 0.75 or n < 15
    if n >= 100:
        z = np.flatnonzero(w == 0)
        runs = np.split(z, np.flatnonzero(np.diff(z) > 1) + 1)
        assert max(len(r) for r in runs) >= 40
    assert (w[pos] > 0).all()
    # the edges of the search: x = 0 lands on the first positive entry, the largest x on the last positive one
    first, last = int(np.flatnonzero(w > 0)[0]), int(np.flatnonzero(w > 0)[-1])
    c = [float(x) for x in cum]
    assert bisect.bisect_right(c, 0.0, 0, n - 1) == first
    assert bisect.bisect_right(c, (1.0 - 2.0 ** -53) * c[-1], 0, n - 1) == last
