"""Plain host restatement of the device sampler (pcg_pick / pcg_pick_shuffled_epochs): numpy and Python integers only, written
from Salmon et al., "Parallel random numbers: as easy as 1, 2, 3" (SC'11) and from the definitions in the kernel's comments;
it imports nothing of the package.

    draw i of (seed, epoch):  u = uniform(seed, epoch, i)                                  in [0, 1), 53 bits
                              pick = idx_train[bisect_right(cum, u * cum[-1], 0, n - 1)]   (random.choices, CPython)

All arithmetic on u is float64 and the product u * cum[-1] is ONE rounded multiply (a Python float product)."""
import bisect

import numpy as np

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57        # the two multipliers of Philox4x32
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85        # the Weyl increments of the two key words (golden ratio, sqrt(3) - 1)


def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds: counter (4 words), key (2 words) -> 4 words.  One round:
    (c0, c1, c2, c3) -> (hi(M1 * c2) ^ c1 ^ k0, lo(M1 * c2), hi(M0 * c0) ^ c3 ^ k1, lo(M0 * c0)); the key is bumped by the Weyl
    constants between rounds (not after the last)."""
    c0, c1, c2, c3 = (int(x) & M32 for x in counter)
    k0, k1 = (int(x) & M32 for x in key)
    for r in range(10):
        if r:
            k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
    return c0, c1, c2, c3


def counter_key(seed: int, epoch: int, draw: int):
    """counter = (draw, 0, epoch low word, epoch high word), key = (seed low word, seed high word)"""
    seed, epoch = int(seed) & (2 ** 64 - 1), int(epoch) & (2 ** 64 - 1)
    return (int(draw) & M32, 0, epoch & M32, epoch >> 32), (seed & M32, seed >> 32)


def uniform(seed: int, epoch: int, draw: int) -> float:
    """CPython's own 53-bit construction (random_random: a = word >> 5, b = word >> 6, (a * 2^26 + b) / 2^53) from the first two
    output words"""
    c = philox4x32_10(*counter_key(seed, epoch, draw))
    return ((c[0] >> 5) * 2 ** 26 + (c[1] >> 6)) / 2 ** 53


def uniforms(seed: int, epoch: int, k: int) -> np.ndarray:
    """uniform(seed, epoch, i) for i = 0 .. k - 1 as a float64 array: the same rounds on numpy uint64 lanes (every product of
    two 32-bit words fits 64 bits), the same integer -> double step (exact: the integer is below 2^53)."""
    (_, _, e0, e1), (k0, k1) = counter_key(seed, epoch, 0)
    m = np.uint64(M32)
    c0 = np.arange(k, dtype=np.uint64)
    c1 = np.zeros(k, dtype=np.uint64)
    c2 = np.full(k, e0, dtype=np.uint64)
    c3 = np.full(k, e1, dtype=np.uint64)
    s = np.uint64(32)
    for r in range(10):
        if r:
            k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> s) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> s) ^ c3 ^ np.uint64(k1), p0 & m
    bits = (c0 >> np.uint64(5)) * np.uint64(2 ** 26) + (c1 >> np.uint64(6))
    return bits.astype(np.float64) / float(2 ** 53)


def positions(cum, seed: int, epoch: int, k: int) -> np.ndarray:
    """bisect_right(cum, u_i * cum[-1], 0, n - 1) for the k draws of (seed, epoch): positions into idx_train"""
    cum = [float(x) for x in cum]
    n, total = len(cum), cum[-1]
    return np.array([bisect.bisect_right(cum, float(u) * total, 0, n - 1) for u in uniforms(seed, epoch, k)], dtype=np.int64)


def picks(cum, idx_train, seed: int, epoch: int, k: int) -> np.ndarray:
    """the k picks of (seed, epoch) in draw order"""
    return np.asarray(idx_train)[positions(cum, seed, epoch, k)]


# ---- the weight vectors the sampler tests draw from ---------------------------------------------------------------------------
def positive_weights(n: int, rs: np.random.RandomState) -> np.ndarray:
    """degree / label-frequency like weights, all positive"""
    return rs.randint(1, 50, size=n) / 7.0


def weights_with_zero_runs(n: int, rs: np.random.RandomState) -> np.ndarray:
    """About half the entries zero (degree-0 training nodes), laid out in runs of 1 .. 8 entries, the first and the last entry
    zero and - from n = 100 on - one run of 40 zeros: the cumulative weights have runs of equal values, at both ends too.
    (n <= 2 leaves nothing positive: cum is all zero and every draw is clipped to the last index.)"""
    w = positive_weights(n, rs)
    i, zero = 0, True
    while i < n:
        run = int(rs.randint(1, 9))
        if zero:
            w[i:i + run] = 0.0
        i, zero = i + run, not zero
    if n >= 100:
        w[n // 3:n // 3 + 40] = 0.0
        w[n // 3 + 40] = 3.0 / 7.0
    w[0] = w[-1] = 0.0
    return w
