"""tests/ranked_train_ref.py - the oracle of the train-mode ranked-selection GPU tests - against the reference's own
``samp_score_diff`` (tests/golden/ranked_train.npz, recorded from the imported reference by make_golden_ranked_train.py), and the
host side of the feature: ``ops.minority_counts`` and the minority accessors of ``graph.ChosenLists``.  CPU only."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.ranked_train_ref import compare_train_with_golden, golden_scores, minority_tail, ranked_train_ref
from tests.util import GOLDEN, GoldenCase

CASES = ["yelp_small", "single_rel", "five_rel"]
RHOS = [0.2, 0.5, 2.0]


@pytest.fixture(scope="module")
def ranked_train():
    return np.load(os.path.join(GOLDEN, "ranked_train.npz"))


@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("name", CASES)
def test_ranked_train_ref_reproduces_reference(ranked_train, name, rho):
    c = GoldenCase(name)
    z = ranked_train
    assert np.array_equal(z[f"{name}_nodes"], np.asarray(c.nodes)) and np.array_equal(z[f"{name}_labels"], c.batch_labels)
    assert np.array_equal(z[f"{name}_train_pos"], np.asarray(c.train_pos))
    thresholds = [0.5] * c.R
    s0, center = golden_scores(z, c)
    neigh, minor = ranked_train_ref(c.csr, c.nodes, c.batch_labels, s0, thresholds, rho, c.train_pos, center=center)
    compare_train_with_golden(z, c, rho, neigh, minor, thresholds)
    # every row of a positive centre is a prefix of the centre's longest one: the order does not depend on the relation
    moff, mids, _ = minor
    for b in np.flatnonzero(c.batch_labels == 1).tolist():
        rows = [mids[moff[r, b]:moff[r, b + 1]] for r in range(c.R)]
        longest = max(rows, key=len)
        assert all(np.array_equal(row, longest[:len(row)]) for row in rows)


def test_fixture_has_no_tie_at_a_minority_cut(ranked_train):
    for name in CASES:
        assert float(ranked_train[f"{name}_min_minor_gap"]) > 0


def test_minority_tail_ties_go_to_the_smaller_position():
    s = torch.tensor([0.5, 0.25, 0.75, 0.25, 0.5, 0.75], dtype=torch.float32)
    pos, d = minority_tail(torch.tensor(0.5), s, 4)
    assert pos.tolist() == [0, 4, 1, 2] and d.tolist() == [0.0, 0.0, 0.25, 0.25]


# ---- ops.minority_counts / sel_capacity ----------------------------------------------------------------------------------------
def host_graph(deg_rows, n_pos):
    """what minority_counts and sel_capacity read of a DeviceGraph"""
    return SimpleNamespace(R=len(deg_rows), deg_host=[np.asarray(d, dtype=np.int64) for d in deg_rows], n_pos=n_pos)


@pytest.mark.parametrize("n_pos", [0, 7, 100000])
def test_minority_counts_against_sel_capacity_row(n_pos):
    import pcgnn_amd
    from pcgnn_amd import _lib, ops
    pcgnn_amd.build_library()
    lib = _lib.load()
    degs = np.arange(0, 60)
    g = host_graph([degs, degs[::-1].copy(), degs * 37], n_pos)
    thr, rho = [0.2, 0.5, 1.0], [0.2, 0.5, 2.0]
    nodes = np.random.RandomState(0).randint(0, len(degs), size=200)
    labels = np.random.RandomState(1).randint(0, 2, size=200)
    m = ops.minority_counts(g, nodes, labels, thr, rho)
    assert m.shape == (3, 200) and m.dtype == np.int64
    for r in range(3):
        for b, v in enumerate(nodes.tolist()):
            deg = int(g.deg_host[r][v])
            with_m = lib.pcg_sel_capacity_row(deg, thr[r], rho[r], int(labels[b]), n_pos, 0)
            without = lib.pcg_sel_capacity_row(deg, thr[r], 0.0, 0, n_pos, 0)
            assert m[r, b] == with_m - without, (r, b)
            k = math.ceil(deg * thr[r])
            assert m[r, b] == (min(int(k * rho[r]), n_pos) if labels[b] == 1 else 0)
    # sel_capacity is the same sum as before, a scalar rho is every relation's, and test mode has no minority term
    caps = ops.sel_capacity(g, nodes, labels, thr, rho, True, add_self=True)
    for r in range(3):
        want = [lib.pcg_sel_capacity_row(int(g.deg_host[r][v]), thr[r], rho[r], int(labels[b]), n_pos, 1)
                for b, v in enumerate(nodes.tolist())]
        assert caps[r].tolist() == want
    assert np.array_equal(ops.minority_counts(g, nodes, labels, thr, 0.5), ops.minority_counts(g, nodes, labels, thr, [0.5] * 3))
    assert np.array_equal(ops.sel_capacity(g, nodes, None, thr, rho, False),
                          ops.sel_capacity(g, nodes, labels, thr, 0.0, True))


# ---- graph.ChosenLists -----------------------------------------------------------------------------------------------------------
def lists(with_minority):
    from pcgnn_amd.graph import ChosenLists
    R, n = 2, 3
    flat = torch.tensor([0, 2, 2, 5, 6, 8, 9], dtype=torch.int64)
    ids = torch.tensor([4, 9, 1, 2, 3, 7, 5, 6, 8], dtype=torch.int32)
    dist = torch.tensor([.5, .25, .125, .25, .5, 1., 2., 4., 8.], dtype=torch.float32)
    if not with_minority:
        return ChosenLists(flat, ids, dist, R, n)
    mflat = torch.tensor([0, 2, 2, 2, 3, 3, 3], dtype=torch.int64)
    mids = torch.tensor([9, 30, 30], dtype=torch.int32)
    mdist = torch.tensor([.25, 16., 16.], dtype=torch.float32)
    return ChosenLists(flat, ids, dist, R, n, minor_flat_offsets=mflat, minor_ids=mids, minor_dist=mdist)


def test_chosen_lists_minority_accessors():
    ch = lists(True)
    assert ch.has_minority and ch.minor_offsets.shape == (2, 4)
    assert ch.minor_offsets.tolist() == [[0, 2, 2, 2], [2, 3, 3, 3]]
    i, d = ch.minor_row(0, 0)
    assert i.tolist() == [9, 30] and d.tolist() == [.25, 16.]
    assert ch.minor_row(0, 1)[0].numel() == 0 and ch.minor_row(1, 0)[0].tolist() == [30] and ch.minor_row(1, 2)[1].numel() == 0
    # the neighbour part keeps its meaning
    assert ch.row(0, 0)[0].tolist() == [4, 9] and ch.row(1, 0)[1].tolist() == [1.]
    off, ids, dist = ch
    assert off.shape == (2, 4) and ids.numel() == 9 and dist.numel() == 9
    # the reference's train-mode shape: set union (9 is a neighbour and a minority pick), neighbour then minority distances
    sets, scores = ch.to_reference(0)
    assert sets == [{4, 9, 30}, set(), {1, 2, 3}] and scores == [[.5, .25, .25, 16.], [], [.125, .25, .5]]
    sets, scores = ch.to_reference(1)
    assert sets == [{7, 30}, {5, 6}, {8}] and scores == [[1., 16.], [2., 4.], [8.]]
    md = ch.mean_dist()
    assert md[0, 0].item() == .375 and math.isnan(md[0, 1].item())
    mdm = ch.mean_dist(include_minority=True)
    assert mdm[0, 0].item() == (.5 + .25 + .25 + 16.) / 4 and mdm[1, 0].item() == 8.5 and mdm[1, 1].item() == 3.
    assert torch.equal(md[1, 1:], mdm[1, 1:]) and md[0, 2].item() == mdm[0, 2].item()


def test_chosen_lists_without_minority_is_unchanged():
    ch, full = lists(False), lists(True)
    assert not ch.has_minority and ch.minor_offsets is None and ch.minor_ids is None and ch.minor_dist is None
    with pytest.raises(ValueError):
        ch.minor_row(0, 0)
    sets, scores = ch.to_reference(0)
    assert sets == [{4, 9}, set(), {1, 2, 3}] and scores == [[.5, .25], [], [.125, .25, .5]]
    assert torch.equal(ch.mean_dist(include_minority=True).nan_to_num(-1), ch.mean_dist().nan_to_num(-1))
    assert torch.equal(ch.mean_dist().nan_to_num(-1), full.mean_dist().nan_to_num(-1))
    assert ch.row(1, 1)[0].tolist() == full.row(1, 1)[0].tolist() == [5, 6]
