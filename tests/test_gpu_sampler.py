"""The device sampler (segmean_pick.hip: pcg_pick, pcg_pick_shuffled_epochs - Philox4x32-10 draws, the 16-lane search, the keyed
shuffle, several epochs per launch, the device epoch counter) against the plain host reference of tests/sampler_ref.py.
Every comparison is exact: the draws are integers and the search is over float64 values both sides hold bit for bit.
Run with ``pytest -m gpu`` on an MI355X."""
import numpy as np
import pytest
import torch

from tests import sampler_ref as S

pytestmark = pytest.mark.gpu

SEED_EPOCH = [(0, 0), (11, 100), (2 ** 32 + 5, 3), (2 ** 63 + 1, 2 ** 32 + 7), (5, 2 ** 40)]     # the high words of both arguments
N_TRAIN = [1, 2, 3, 15, 16, 17, 18, 255, 256, 257, 4095, 4096, 4097, 65537]                       # around the powers of 16
K_SHUFFLE = [1, 2, 3, 15, 16, 17, 31, 32, 33, 255, 256, 257, 4095, 4096, 4097, 5346]
K_SEARCH = 2000


@pytest.fixture(scope="module")
def ops():
    import pcgnn_amd  # noqa: F401
    from pcgnn_amd import ops
    return ops


def dev():
    return torch.device("cuda", 0)


def full(k, value=-1):
    return torch.full((k,), value, dtype=torch.int32, device=dev())


@pytest.fixture(scope="module")
def plain():
    """n_train = 18000, strictly increasing cumulative weights (the set-up of test_pick_shuffled_is_a_shuffle_of_pick), with
    idx_train[p] = p so that a pick names its position"""
    rs = np.random.RandomState(3)
    n = 18000
    cum = np.cumsum(S.positive_weights(n, rs))
    idx = np.arange(n, dtype=np.int32)
    labels = (rs.rand(n) < 0.15).astype(np.int32)
    return dict(n=n, cum=cum, idx=idx, labels=labels, cum_d=torch.from_numpy(cum).to(dev()), idx_d=torch.from_numpy(idx).to(dev()),
                lab_d=torch.from_numpy(labels).to(dev()), ref={})


def plain_ref(plain, seed, epoch, k, upto=0):
    """the reference picks of (seed, epoch), computed once per key (upto: as many as any test asks of it), shared and read-only:
    draw i does not depend on how many are drawn"""
    have = plain["ref"].get((seed, epoch))
    if have is None or len(have) < k:
        have = plain["ref"][(seed, epoch)] = S.picks(plain["cum"], plain["idx"], seed, epoch, max(k, upto))
        have.setflags(write=False)
    return have[:k]


@pytest.mark.parametrize("seed,epoch", SEED_EPOCH)
def test_pick_equals_reference(ops, plain, seed, epoch):
    """pcg_pick with device draws == idx_train[bisect_right(cum, uniform(seed, epoch, i) * cum[-1], 0, n - 1)], draw by draw"""
    out = ops.pick(plain["cum_d"], plain["idx_d"], 1000, None, seed, epoch)
    assert out.cpu().numpy().tolist() == plain_ref(plain, seed, epoch, 1000).tolist()


@pytest.fixture(scope="module", params=N_TRAIN)
def sized(request):
    """one upload per n_train: idx_train (distinct ids, 3 p + 1), and both weight vectors' cumulative sums"""
    n = request.param
    rs = np.random.RandomState(1000 + n)
    idx = (np.arange(n, dtype=np.int64) * 3 + 1).astype(np.int32)
    ws = {"positive": S.positive_weights(n, rs), "zero_runs": S.weights_with_zero_runs(n, rs)}
    return dict(n=n, idx=idx, idx_d=torch.from_numpy(idx).to(dev()), w=ws,
                cum={k: np.cumsum(w) for k, w in ws.items()},
                cum_d={k: torch.from_numpy(np.cumsum(w)).to(dev()) for k, w in ws.items()})


@pytest.mark.parametrize("weights", ["positive", "zero_runs"])
def test_pick_shuffled_search_equals_reference(ops, sized, weights):
    """The 16-lane search (bisect16) against Python's bisect_right: sorted, the shuffled picks are the sorted reference picks -
    at sizes around the powers of 16 where the probe step changes, n = 1 and 2, and over cumulative weights with runs of equal
    values (zero-weight entries, at both ends too).  No entry of weight zero is picked, except where the reference itself
    returns one: nothing positive at all (n <= 2), where the hi = n - 1 clip gives the last index."""
    n, seed, epoch = sized["n"], 7, 1
    cum, w, idx = sized["cum"][weights], sized["w"][weights], sized["idx"]
    ref_pos = S.positions(cum, seed, epoch, K_SEARCH)
    out = full(K_SEARCH)
    ops.pick_shuffled(sized["cum_d"][weights], sized["idx_d"], K_SEARCH, seed, epoch, out)
    got = out.cpu().numpy()
    assert np.array_equal(np.sort(got), np.sort(idx[ref_pos]))
    got_pos = (got.astype(np.int64) - 1) // 3
    assert np.array_equal(idx[got_pos], got)
    allowed_zero = set(ref_pos[w[ref_pos] == 0].tolist())            # what the reference itself returns of weight zero
    assert allowed_zero <= {n - 1} and (not allowed_zero or not w.any())
    assert set(got_pos[w[got_pos] == 0].tolist()) <= allowed_zero
    # ... and pcg_pick's two-way search on the same cumulative weights, draw by draw
    assert ops.pick(sized["cum_d"][weights], sized["idx_d"], K_SEARCH, None, seed, epoch).cpu().numpy().tolist() == idx[ref_pos].tolist()


def sigma_of(shuffled: np.ndarray, ref: np.ndarray):
    """where the shuffle put draw i, for the draws whose pick occurs once (picks are drawn with replacement): i -> position"""
    vals, first, counts = np.unique(ref, return_index=True, return_counts=True)
    once = counts == 1
    where = {int(v): p for p, v in enumerate(shuffled.tolist())}
    return {int(i): where[int(v)] for v, i in zip(vals[once], first[once])}


@pytest.mark.parametrize("k", K_SHUFFLE)
def test_shuffle_is_a_bijection_with_its_labels(ops, plain, k):
    """Every output slot is written exactly once (pre-filled with -1: none is left, and the output is a permutation of the
    reference picks), out_labels == labels_all[out_ids], and from k = 256 on the order is neither the draw order nor the same in
    two epochs.  (Order: for draws whose pick occurs once the position sigma(i) is known.  Two independent uniform permutations
    agree at a given i with probability 1 / k, so the number of agreements is about Poisson(1): more than half of at least
    100 known positions agreeing cannot happen by chance.)"""
    seed, sig = 11, []
    for epoch in (100, 101):
        out, lab = full(k), full(k)
        ops.pick_shuffled(plain["cum_d"], plain["idx_d"], k, seed, epoch, out, plain["lab_d"], lab)
        got, ref = out.cpu().numpy(), plain_ref(plain, seed, epoch, k, upto=max(K_SHUFFLE))
        assert (got >= 0).all() and np.array_equal(np.sort(got), np.sort(ref))
        assert np.array_equal(lab.cpu().numpy(), plain["labels"][got])
        sig.append(sigma_of(got, ref))
    if k >= 256:
        for s in sig:
            assert len(s) >= 100 and sum(p == i for i, p in s.items()) < len(s) // 2, "the order is the draw order"
        both = set(sig[0]) & set(sig[1])
        assert len(both) >= 100 and sum(sig[0][i] == sig[1][i] for i in both) < len(both) // 2, "two epochs, one order"


def test_several_epochs_in_one_launch(ops, plain):
    """n_epochs = 3 in one launch, k = 517, epoch_base = 100, the device counter at 7: epoch e's block is the single-epoch launch
    at epoch 107 + e, element by element (the shuffle key depends on the epoch: the order is that epoch's too) and a shuffle of
    the reference picks of that epoch; bump=True moves the counter to 10, bump=False leaves it; its second word stays 0."""
    k, seed = 517, 11
    counter = torch.tensor([7, 0], dtype=torch.int64, device=dev())
    out, lab = full(3 * k), full(3 * k)
    ops.pick_shuffled(plain["cum_d"], plain["idx_d"], k, seed, 100, out, plain["lab_d"], lab, counter, bump=False, n_epochs=3)
    assert counter.cpu().tolist() == [7, 0]
    out2, lab2 = full(3 * k), full(3 * k)
    ops.pick_shuffled(plain["cum_d"], plain["idx_d"], k, seed, 100, out2, plain["lab_d"], lab2, counter, bump=True, n_epochs=3)
    assert counter.cpu().tolist() == [10, 0]
    assert torch.equal(out, out2) and torch.equal(lab, lab2)
    got, got_lab = out.cpu().numpy(), lab.cpu().numpy()
    assert np.array_equal(got_lab, plain["labels"][got])
    for e in range(3):
        one = full(k)
        ops.pick_shuffled(plain["cum_d"], plain["idx_d"], k, seed, 107 + e, one)
        assert np.array_equal(got[e * k:(e + 1) * k], one.cpu().numpy()), e
        assert np.array_equal(np.sort(got[e * k:(e + 1) * k]), np.sort(plain_ref(plain, seed, 107 + e, k))), e
    # the counter is read on the device: the next launch starts at 10
    one, nxt = full(k), full(k)
    ops.pick_shuffled(plain["cum_d"], plain["idx_d"], k, seed, 100, nxt, None, None, counter, bump=True)
    ops.pick_shuffled(plain["cum_d"], plain["idx_d"], k, seed, 110, one)
    assert torch.equal(nxt, one) and counter.cpu().tolist() == [11, 0]
