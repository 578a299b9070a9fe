"""Both bucket sorts of the train-pos keys (csrc/sort.hip) on layouts that decide what their evenly spaced sample sees
(tests/sort_ref.py; tests/test_sort_ref_host.py shows on the CPU which bucket sizes each case reaches).  Run with ``pytest -m gpu``.

pcg_pos_sort (four launches): every splitter branch and sample cap (131073 .. 1048577 keys), a bucket of exactly one LDS tile, of
two and of three (rank_sort_body<BK_TILE>'s tile loop over already formed keys), almost the whole array in one bucket, and a size
where the scratch entries raise the capacity.
pcg_pos_sort_raw (one launch): raw keys in layout order; a bucket of exactly 4096 keys sorts clean, one of 4097 and the periodic
layout give exactly what the header promises for PCG_ST_SORT_OVERFLOW - and damage nothing but the dropped entries.

Every comparison is exact, against np.sort of the host keys with all-ones padding to the capacity; the whole key buffer is
prefilled with a sentinel word, so an entry nobody wrote shows.  The four-launch sort's order does not depend on its splitters
(bucket_of is monotone in the key over any array), so the splitters and bucket sizes it leaves in the scratch half are compared
with the host restatement as well: that is what holds bk_splitters' two sample sorts to account."""
import numpy as np
import pytest
import torch

from tests import sort_ref as S

pytestmark = pytest.mark.gpu

_GRAPHS = {}


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def P():
    import pcgnn_amd
    from pcgnn_amd import ops  # noqa: F401  (fails loudly if the .so is missing)
    return pcgnn_amd


def graph(P, n_pos):
    """n_pos + 7 isolated nodes of 4 features; train positive i is node n - 1 - i (train_pos order is not id order)"""
    if n_pos not in _GRAPHS:
        n = n_pos + 7
        tp = n - 1 - np.arange(n_pos, dtype=np.int64)
        csr = (np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int32))
        _GRAPHS.clear()                                        # (one graph at a time: the largest is a million nodes)
        _GRAPHS[n_pos] = (P.DeviceGraph(np.zeros((n, 4), np.float32), [csr], tp, dev()), tp, n)
    return _GRAPHS[n_pos]


def fresh_keys(n_pos):
    from pcgnn_amd import _lib
    total = int(_lib.load().pcg_pos_sort_capacity(n_pos))
    assert total == S.capacity(n_pos)
    return torch.full((total,), S.SENTINEL, dtype=torch.int64, device=dev()), total // 2


def host(t):
    return t.cpu().numpy().view(np.uint64)


def four_launches(P, n_pos, scores, what):
    g, tp, n = graph(P, n_pos)
    s0 = np.zeros(n, dtype=np.float32)
    s0[tp] = scores
    keys, cap = fresh_keys(n_pos)
    P.ops.pos_sort(g, torch.from_numpy(s0).to(dev()), keys)
    torch.cuda.synchronize()
    got = host(keys)
    want = S.sorted_with_padding(S.raw_keys(scores), cap)
    bad = np.flatnonzero(got[:cap] != want)
    assert bad.size == 0, f"{what}: {bad.size} entries differ, first at {bad[0]}: {int(got[bad[0]]):#x} for {int(want[bad[0]]):#x}"
    # behind the scatter buffer, the splitters, the counts and the cursors nothing is written
    assert np.all(got[cap + n_pos + S.BK_SCRATCH:] == np.uint64(S.SENTINEL)), what
    # The sorted order cannot show a wrong sample sort: bucket_of's bisection is monotone in the key over ANY splitter array, so
    # the buckets are ordered ranges whatever bk_splitters leaves - only their sizes change.  What it left is still in the
    # scratch half (sort.hip: [cap, cap + n_pos) scattered keys | 1024 splitters | 1024 counts, 1024 cursors, uint32): the
    # splitters and the bucket sizes are the host restatement's, entry for entry.
    geometry = S.four_launch_geometry(n_pos)
    nb = geometry[0]
    raw = S.raw_keys(scores)
    at = cap + n_pos
    assert np.array_equal(got[at:at + nb], S.splitters(raw, geometry)), f"{what}: splitters"
    words = got[at + S.BK_MAX:at + S.BK_SCRATCH].view(np.uint32)
    counts = S.bucket_counts(raw, geometry)
    assert np.array_equal(words[:nb], counts) and np.array_equal(words[S.BK_MAX:S.BK_MAX + nb], counts), f"{what}: bucket sizes"


# ---- pcg_pos_sort -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pos", S.FOUR_RANDOM_SIZES)
def test_four_launches_every_splitter_branch(P, n_pos):
    four_launches(P, n_pos, S.gaussian(n_pos), f"gaussian {n_pos}")


@pytest.mark.parametrize("K", S.CRAFTED_K)
@pytest.mark.parametrize("n_pos", S.FOUR_CRAFTED_SIZES)
def test_four_launches_long_bucket(P, n_pos, K):
    scores = S.crafted(n_pos, S.four_launch_geometry(n_pos), K)
    four_launches(P, n_pos, scores, f"crafted {n_pos} K {K} ({S.tiles(K)} tiles)")


@pytest.mark.parametrize("n_pos", S.PERIODIC_SIZES)
def test_four_launches_periodic(P, n_pos):
    four_launches(P, n_pos, S.periodic(n_pos, S.four_launch_geometry(n_pos)[1]), f"periodic {n_pos}")


def test_four_launches_where_the_scratch_raises_the_capacity(P):
    n_pos = S.SCRATCH_RAISES_CAPACITY
    assert S.half_capacity(n_pos) == 65536
    for name in ("gaussian", "descending"):
        four_launches(P, n_pos, S.NATURAL[name](n_pos), f"{name} {n_pos}")


# ---- pcg_pos_sort_raw -------------------------------------------------------------------------------------------------------------
def one_launch(P, n_pos, scores, status):
    """-> (the whole key buffer after the call, cap, the raw keys)"""
    from pcgnn_amd import _lib
    ops, lib = P.ops, _lib.load()
    g, _, _ = graph(P, n_pos)
    raw = S.raw_keys(scores)
    keys, cap = fresh_keys(n_pos)
    keys[cap:cap + n_pos] = torch.from_numpy(raw.view(np.int64)).to(dev())           # in layout order
    _lib.check(lib.pcg_pos_sort_raw(g.desc_ref(), ops._p(keys), ops._p(status), ops._stream(dev())), "pcg_pos_sort_raw")
    torch.cuda.synchronize()
    return host(keys), cap, raw


def assert_clean(got, cap, raw, status, what):
    n_pos = raw.size
    want = S.sorted_with_padding(raw, cap)
    bad = np.flatnonzero(got[:cap] != want)
    assert bad.size == 0, f"{what}: {bad.size} entries differ, first at {bad[0]}: {int(got[bad[0]]):#x} for {int(want[bad[0]]):#x}"
    assert int(status.item()) == 0, what
    assert np.array_equal(got[cap:cap + n_pos], raw) and np.all(got[cap + n_pos:] == np.uint64(S.SENTINEL)), what


@pytest.mark.parametrize("n_pos", S.ONE_SIZES)
def test_one_launch_layouts(P, n_pos):
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    geometry = S.one_launch_geometry(n_pos)
    cases = [(name, make(n_pos)) for name, make in S.NATURAL.items()] + [("crafted 4096", S.crafted(n_pos, geometry, S.TILE))]
    for name, scores in cases:
        got, cap, raw = one_launch(P, n_pos, scores, status)
        assert_clean(got, cap, raw, status, f"{name} {n_pos}")


@pytest.mark.parametrize("layout", ["crafted 4097", "periodic"])
@pytest.mark.parametrize("n_pos", S.ONE_SIZES)
def test_one_launch_overflow_contract(P, n_pos, layout):
    """include/pcgnn.h: a bucket of more than 4096 keys sets PCG_ST_SORT_OVERFLOW, its surplus keys are dropped"""
    geometry = S.one_launch_geometry(n_pos)
    scores = S.crafted(n_pos, geometry, S.TILE + 1) if layout == "crafted 4097" else S.periodic(n_pos, geometry[1])
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    got, cap, raw = one_launch(P, n_pos, scores, status)
    what = f"{layout} {n_pos}"
    begin, end = S.overflow_extent(raw, geometry)
    assert begin == 0 and end > S.TILE
    assert int(status.item()) == S.ST_SORT_OVERFLOW, what                            # that bit and no other
    want = S.sorted_with_padding(raw, cap)
    assert np.all(got[n_pos:cap] == S.ALL_ONES), what                                # the padding
    # a bucket's offset comes from an exact count: everything behind the overflowed bucket is where it belongs
    assert np.array_equal(got[end:n_pos], want[end:n_pos]), what
    head = got[:S.TILE]
    assert np.all(head[1:] > head[:-1]) and np.all(np.isin(head, want[:end])), what  # 4096 of bucket 0's keys, in order
    assert np.all(got[S.TILE:end] == np.uint64(S.SENTINEL)), what                    # the surplus: dropped, nothing stored
    assert np.array_equal(got[cap:cap + n_pos], raw), what                           # the raw keys are only read
    assert np.all(got[cap + n_pos:] == np.uint64(S.SENTINEL)), what                  # the scratch half behind them: untouched
    # the next sort, the status word zeroed: clean
    status.zero_()
    got, cap, raw = one_launch(P, n_pos, S.gaussian(n_pos), status)
    assert_clean(got, cap, raw, status, f"gaussian {n_pos} after {layout}")
