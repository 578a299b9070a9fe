"""The bucket geometry of csrc/sort.hip restated (tests/sort_ref.py), on the CPU: both sorts' bucket and sample counts at the
sizes where they change, the key buffer's capacity against the library's own, the splitter rule against a plain scan - and the
bucket sizes of every layout tests/test_gpu_bucket_sort.py and tests/test_gpu_train_many_positives.py send to the GPU: a case that
claims a bucket of 4096, 4097 or 8193 keys shows it here first, and no natural layout comes near the tile."""
import numpy as np
import pytest

from tests import front_ref as F
from tests import sort_ref as S


def test_geometry_at_its_edges():
    assert [S.one_launch_geometry(n) for n in (16385, 32768, 32769, 65536, 65537, 131072)] == \
        [(64, 256), (64, 256), (128, 512), (128, 512), (256, 1024), (256, 1024)]
    assert [S.four_launch_geometry(n) for n in (16385, 32768, 32769, 131072, 131073, 262144, 262145, 524288, 524289, 1048577)] == \
        [(32, 256), (32, 256), (64, 512), (128, 1024), (256, 2048), (256, 2048), (512, 4096), (512, 4096), (1024, 4096),
         (1024, 4096)]
    # the splitter kernel's two branches, and the sample cap (four samples a bucket instead of eight)
    assert S.splitter_branch(S.four_launch_geometry(131072)[1]) == "rank"
    for n in S.FOUR_RANDOM_SIZES:
        nb, ns = S.four_launch_geometry(n)
        assert S.splitter_branch(ns) == "bitonic" and ns % nb == 0
        print(f"four launches, n_pos {n}: {nb} buckets, {ns} samples ({ns // nb} a bucket)")
    assert {S.four_launch_geometry(n)[1] // S.four_launch_geometry(n)[0] for n in S.FOUR_RANDOM_SIZES} == {8, 4}
    for n in S.ONE_SIZES:
        nb, ns = S.one_launch_geometry(n)
        assert ns == 4 * nb <= S.SORT_THREADS and np.unique(S.sample_positions(n, ns)).size == ns


def test_capacity_is_the_librarys():
    from pcgnn_amd import _lib
    lib = _lib.load()
    sizes = [0, 1, 4095, 4096, 4097, 16384, 16385, 30720, 30721, 32000, 32768, 40000, 63488, 63489, 65537, 129024, 129025, 131072,
             131073, 262145, 524289, 1048577]
    for n in sizes:
        assert int(lib.pcg_pos_sort_capacity(n)) == S.capacity(n), n
        assert int(lib.pcg_pos_sort_one_launch(n)) == int(S.RANK_MAX < n <= S.BK1_MAX), n
    # up to 16384 keys the half is front_ref's; above, the 2048 scratch entries can raise it a power of two
    assert all(S.half_capacity(n) == F.sort_capacity(n) for n in (1, 4096, 4097, 16384))
    n = S.SCRATCH_RAISES_CAPACITY
    assert F.sort_capacity(n) == 32768 and S.half_capacity(n) == 65536
    assert S.half_capacity(30720) == 32768 and S.half_capacity(30721) == 65536
    for n in S.ONE_SIZES + S.FOUR_RANDOM_SIZES + S.FOUR_CRAFTED_SIZES + S.PERIODIC_SIZES + [n]:
        # what pcg_pos_sort lays out behind the sorted half: n_pos scattered keys, then 1024 splitters, then counts and cursors
        assert S.half_capacity(n) >= n + S.BK_SCRATCH and S.capacity(n) < 2 ** 31


def test_splitters_and_bucket_of_are_the_plain_rule():
    rs = np.random.RandomState(5)
    keys = S.raw_keys(np.round(rs.randn(20000), 1))
    for geometry in ((32, 256), (64, 256), (16, 128)):
        nb, ns = geometry
        spl = S.splitters(keys, geometry)
        samp = sorted(int(keys[(j * keys.size) // ns]) for j in range(ns))
        assert int(spl[0]) == 0 and [int(v) for v in spl[1:]] == [samp[b * (ns // nb)] for b in range(1, nb)]
        assert np.all(spl[1:] > spl[:-1])
        got = S.bucket_of(spl, keys[:500])
        for key, b in zip(keys[:500], got):
            want = max(j for j in range(nb) if int(spl[j]) <= int(key))
            assert b == want
        counts = S.bucket_counts(keys, geometry)
        assert counts.sum() == keys.size and counts.min() >= ns // nb       # (a bucket holds at least its own samples)
    # a key equal to a splitter belongs to that splitter's bucket; below every splitter and above: the first, the last
    spl = np.array([0, 10, 20], dtype=np.uint64)
    assert list(S.bucket_of(spl, np.array([0, 9, 10, 19, 20, 2 ** 63], dtype=np.uint64))) == [0, 0, 1, 1, 2, 2]


def test_raw_keys_are_front_refs():
    s = S.gaussian(5000)
    s0 = np.zeros(9000, dtype=np.float32)
    tp = np.random.RandomState(3).permutation(9000)[:5000]
    s0[tp] = s
    assert np.array_equal(S.raw_keys(s), F.pos_keys(s0, tp))
    assert np.array_equal(S.sorted_with_padding(S.raw_keys(s), 8192), F.sorted_keys(s0, tp, 8192))
    assert int(S.ALL_ONES) != S.SENTINEL and (S.SENTINEL & 0xFFFFFFFF) > 2 ** 21 and S.SENTINEL < 2 ** 63


def _crafted_figures(n_pos, geometry, K):
    s = S.crafted(n_pos, geometry, K)
    assert np.unique(s).size == n_pos and np.all(np.round(s / S.UNIT) * S.UNIT == s)      # distinct, exact multiples of UNIT
    counts = S.bucket_counts(S.raw_keys(s), geometry)
    return counts


@pytest.mark.parametrize("K", S.CRAFTED_K)
@pytest.mark.parametrize("n_pos", S.ONE_SIZES)
def test_crafted_bucket_sizes_one_launch(n_pos, K):
    geometry = S.one_launch_geometry(n_pos)
    counts = _crafted_figures(n_pos, geometry, K)
    print(f"one launch, n_pos {n_pos}, K {K}: bucket 0 = {counts[0]}, the others {counts[1:].min()} .. {counts[1:].max()}")
    assert counts[0] == K and S.tiles(K) == {4096: 1, 4097: 2, 8193: 3}[K]
    assert counts[1:].max() <= S.TILE and counts[1:].min() >= 1                 # only bucket 0 can overflow
    extent = S.overflow_extent(S.raw_keys(S.crafted(n_pos, geometry, K)), geometry)
    assert extent == (None if K <= S.TILE else (0, K))


@pytest.mark.parametrize("K", S.CRAFTED_K)
@pytest.mark.parametrize("n_pos", [16385, 131072, 131073, 262145, 524289, 1048577])
def test_crafted_bucket_sizes_four_launches(n_pos, K):
    geometry = S.four_launch_geometry(n_pos)
    counts = _crafted_figures(n_pos, geometry, K)
    print(f"four launches, n_pos {n_pos}, K {K}: bucket 0 = {counts[0]} ({S.tiles(K)} tile(s)), "
          f"the others {counts[1:].min()} .. {counts[1:].max()}")
    assert counts[0] == K
    assert counts[1:].max() <= S.TILE                                           # the tile loop runs in bucket 0 alone
    assert set(S.FOUR_CRAFTED_SIZES) <= {16385, 131072, 131073, 262145, 524289, 1048577}


def test_periodic_bucket_sizes():
    for n_pos in S.PERIODIC_SIZES:
        for name, geometry in (("one launch", S.one_launch_geometry(n_pos)), ("four launches", S.four_launch_geometry(n_pos))):
            nb, ns = geometry
            keys = S.raw_keys(S.periodic(n_pos, ns))
            counts = S.bucket_counts(keys, geometry)
            print(f"{name}, n_pos {n_pos}, periodic: bucket 0 = {counts[0]}, the others {counts[1:].min()} .. {counts[1:].max()}")
            assert counts[0] == n_pos - ns + ns // nb and np.all(counts[1:] == ns // nb)
            assert S.overflow_extent(keys, geometry) == (0, int(counts[0]))
    assert S.bucket_counts(S.raw_keys(S.periodic(16385, 256)), S.one_launch_geometry(16385))[0] == 16133


@pytest.mark.parametrize("n_pos", S.ONE_SIZES)
def test_no_natural_layout_comes_near_the_tile(n_pos):
    worst = 0
    for name, make in S.NATURAL.items():
        s = make(n_pos)
        assert s.dtype == np.float32 and s.size == n_pos
        for geometry in (S.one_launch_geometry(n_pos), S.four_launch_geometry(n_pos)):
            counts = S.bucket_counts(S.raw_keys(s), geometry)
            print(f"n_pos {n_pos}, {name}, {geometry[0]} buckets: largest {counts.max()}")
            assert counts.max() <= S.TILE, (name, geometry)
            if geometry == S.one_launch_geometry(n_pos):
                worst = max(worst, int(counts.max()))
    assert worst <= S.TILE // 2              # (the one-launch sort, where the tile is a limit: representative samples stay here)


def test_random_sizes_stay_in_one_tile():
    """the four-launch sort's random cases: they are about the splitter branches and the sample cap, not about long buckets"""
    for n_pos in S.FOUR_RANDOM_SIZES + [S.SCRATCH_RAISES_CAPACITY]:
        counts = S.bucket_counts(S.raw_keys(S.gaussian(n_pos)), S.four_launch_geometry(n_pos))
        print(f"four launches, n_pos {n_pos}, gaussian: largest bucket {counts.max()}")
        assert counts.max() <= S.TILE
