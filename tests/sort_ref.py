"""Host side of the bucket-sort tests (tests/test_sort_ref_host.py on the CPU, tests/test_gpu_bucket_sort.py and
tests/test_gpu_train_many_positives.py on the GPU): the geometry of both bucket sorts of csrc/sort.hip restated - bucket and
sample counts, the sample positions, the splitter choice, bucket_of, the key buffer's capacity - and score layouts that put a
chosen number of keys into bucket 0.

Both sorts draw their sample from evenly spaced POSITIONS of the unsorted keys, ``(j * n_pos) // n_sample``; the sorted sample's
every ``per``-th key (per = n_sample / n_buckets) is a splitter, splitters[0] = 0 and the last bucket is open above.  A layout
decides which scores sit on the sample positions and so how many keys fall below the second splitter.

  pcg_pos_sort      (four launches, n_pos > 16384): a bucket of any size is sorted - in LDS tiles of TILE keys (bk_sort)
  pcg_pos_sort_raw  (one launch, 16384 < n_pos <= 131072): a bucket of more than TILE keys is reported, its surplus dropped

``bucket_counts`` QUALIFIES an input (it shows that a case reaches the bucket size it is meant for); the expected result of a sort
is ``np.sort`` of the host keys, never this module.  Numpy only.
"""
import numpy as np

from tests.front_ref import orderable

RANK_MAX = 16384               # above it: the bucket sorts
BK1_MAX = 131072               # the one-launch sort's largest n_pos
TILE = 4096                    # BK_TILE (bk_sort's LDS tile) and BK1_TILE (the most keys a bucket of bk_onepass holds)
BK_MAX = 1024                  # buckets of the four-launch sort
BK_SCRATCH = 2 * BK_MAX        # uint64 entries behind the bucketed keys: splitters | counts, cursors
SORT_MAX_SAMPLE = 4096
SORT_MIN_CAP = 4096
SORT_THREADS = 1024            # bk_splitters ranks a sample of up to this many keys; a larger one goes through the bitonic network
ST_SORT_OVERFLOW = 8           # PCG_ST_SORT_OVERFLOW (include/pcgnn.h)
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
SENTINEL = 0x5A5A5A5AA5A5A5A5  # prefill of a key buffer: no key (a key's low word is a position < n_pos), not the padding
UNIT = 2.0 ** -10              # every crafted score is a small integer times UNIT: exact in float32


def one_launch_geometry(n_pos):
    """bk1_geometry: (n_buckets, n_sample) - ~300 - 512 keys a bucket, four samples a bucket"""
    nb = 32
    while nb < 256 and nb * 512 < n_pos:
        nb *= 2
    return nb, nb * 4


def four_launch_geometry(n_pos):
    """pcg_pos_sort: (n_buckets, n_sample) - ~1024 keys a bucket, eight samples a bucket, the sample capped at 4096"""
    nb = 16
    while nb < BK_MAX and nb * 1024 < n_pos:
        nb *= 2
    return nb, min(nb * 8, SORT_MAX_SAMPLE)


def splitter_branch(n_sample):
    """how bk_splitters sorts its sample"""
    return "rank" if n_sample <= SORT_THREADS else "bitonic"


def half_capacity(n_pos):
    """sort_capacity: entries of the sorted half - a power of two >= 4096 that holds the keys and, above RANK_MAX, the bucket
    sort's 2048 scratch entries behind its scatter buffer"""
    need = n_pos + BK_SCRATCH if n_pos > RANK_MAX else n_pos
    cap = SORT_MIN_CAP
    while cap < need:
        cap *= 2
    return cap


def capacity(n_pos):
    """pcg_pos_sort_capacity: sorted half + scratch half"""
    return 2 * half_capacity(n_pos)


def sample_positions(n_pos, n_sample):
    return (np.arange(n_sample, dtype=np.int64) * n_pos) // n_sample


def splitters(keys, geometry):
    """uint64 [n_buckets]: splitters[0] = 0, splitters[b] = the (b * per)-th smallest sample key"""
    nb, ns = geometry
    keys = np.asarray(keys, dtype=np.uint64)
    samp = np.sort(keys[sample_positions(keys.size, ns)])
    spl = samp[::ns // nb].copy()
    assert spl.size == nb
    spl[0] = 0
    return spl


def bucket_of(spl, keys):
    """largest b with spl[b] <= key (spl[0] = 0, the last bucket open)"""
    return np.searchsorted(spl, np.asarray(keys, dtype=np.uint64), side="right") - 1


def bucket_counts(keys, geometry):
    spl = splitters(keys, geometry)
    return np.bincount(bucket_of(spl, keys), minlength=spl.size)


def tiles(n):
    """LDS tiles rank_sort_body<BK_TILE> walks for a bucket of n keys"""
    return (n + TILE - 1) // TILE


def raw_keys(scores):
    """(orderable(score) << 32) | position, uint64: the unsorted keys of scores given in train_pos order"""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    return (orderable(s).astype(np.uint64) << np.uint64(32)) | np.arange(s.size, dtype=np.uint64)


def sorted_with_padding(keys, cap):
    """what either sort leaves in the first `cap` entries: the keys ascending, all-ones behind them"""
    out = np.full(cap, ALL_ONES, dtype=np.uint64)
    out[:keys.size] = np.sort(keys)
    return out


# ---- layouts: float32 scores in train_pos order ---------------------------------------------------------------------------------
def _ranked_scores(order):
    """order[r] = the position that holds the r-th smallest score: distinct scores (r - n / 2) * UNIT, both signs"""
    n = order.size
    assert np.array_equal(np.sort(order), np.arange(n))
    s = np.empty(n, dtype=np.float32)
    s[order] = ((np.arange(n, dtype=np.int64) - n // 2) * UNIT).astype(np.float32)
    return s


def crafted(n_pos, geometry, K):
    """Bucket 0 holds exactly K keys, every other bucket near the mean.  In score order: the first `per` sample positions, then
    K - per positions that are no sample, then every other sample position followed by an equal share of what is left."""
    nb, ns = geometry
    per = ns // nb
    samples = sample_positions(n_pos, ns)
    assert np.unique(samples).size == ns and per <= K <= n_pos - (ns - per)
    is_sample = np.zeros(n_pos, dtype=bool)
    is_sample[samples] = True
    others = np.flatnonzero(~is_sample)
    head, rest = others[:K - per], others[K - per:]
    later = samples[per:]
    share, extra = divmod(rest.size, later.size)
    parts = [samples[:per], head]
    at = 0
    for j, sp in enumerate(later):
        n_j = share + (j < extra)
        parts.append(np.concatenate([[sp], rest[at:at + n_j]]))
        at += n_j
    assert at == rest.size
    return _ranked_scores(np.concatenate(parts).astype(np.int64))


def periodic(n_pos, n_sample):
    """Distinct high scores on exactly the sample positions, one low score everywhere else: every key that is no sample falls
    below the second splitter - bucket 0 holds all but n_sample - per keys"""
    s = np.full(n_pos, -1.0, dtype=np.float32)
    samples = sample_positions(n_pos, n_sample)
    s[samples] = (8.0 + np.arange(n_sample) * UNIT).astype(np.float32)
    return s


def constant(n_pos):
    return np.full(n_pos, 0.25, dtype=np.float32)


def ascending(n_pos):
    return _ranked_scores(np.arange(n_pos))


def descending(n_pos):
    return _ranked_scores(np.arange(n_pos)[::-1].copy())


def half_constant(n_pos):
    """a random half of the positions holds one score (with -0.0 and +0.0 among the others), the rest rounded Gaussians"""
    rs = np.random.RandomState(n_pos % 9973 + 1)
    s = np.round(rs.randn(n_pos), 2).astype(np.float32)
    s[rs.rand(n_pos) < 0.5] = np.float32(0.25)
    s[rs.randint(0, n_pos, 8)] = np.float32(-0.0)
    s[rs.randint(0, n_pos, 8)] = np.float32(0.0)
    return s


def gaussian(n_pos):
    """rounded Gaussians: many equal scores, both signs"""
    rs = np.random.RandomState(n_pos % 9973 + 2)
    s = np.round(rs.randn(n_pos), 2).astype(np.float32)
    s[rs.randint(0, n_pos, 50)] = np.float32(-0.0)
    return s


NATURAL = {"constant": constant, "ascending": ascending, "descending": descending, "half_constant": half_constant,
           "gaussian": gaussian}

# ---- the cases of tests/test_gpu_bucket_sort.py ---------------------------------------------------------------------------------
CRAFTED_K = [TILE, TILE + 1, 2 * TILE + 1]                  # one tile exactly, the first two-tile bucket, a three-tile bucket
FOUR_RANDOM_SIZES = [131073, 262145, 524289, 1048577]       # 256 / 512 / 1024 / 1024 buckets, 2048 / 4096 / 4096 / 4096 samples
FOUR_CRAFTED_SIZES = [16385, 131073]
PERIODIC_SIZES = [16385, 40000]                             # (almost the whole array in one bucket: quadratic, so this small)
SCRATCH_RAISES_CAPACITY = 32000                             # 32000 + 2048 > 32768
ONE_SIZES = [16385, 40000, 65537, 131072]


def overflow_extent(keys, geometry):
    """(first overflowing bucket's begin, end) in the sorted order of the one-launch sort, or None"""
    counts = bucket_counts(keys, geometry)
    over = np.flatnonzero(counts > TILE)
    if over.size == 0:
        return None
    b = int(over[0])
    begin = int(counts[:b].sum())
    return begin, begin + int(counts[b])
