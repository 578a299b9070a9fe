"""The CPU reference of FusedPCGNN.attribute (tests/attr_ref.py) checked against itself, without a GPU: autograd against the
kernel's three hand-written phases, Euler's completeness, the chosen neighbours' shares against their relation's, and the
ReLU-kink condition of every case tests/test_gpu_attribute.py compares (test-mode sets from the oracle)."""
import numpy as np
import pytest
import torch

from tests import attr_ref as A

KEYS = ("logits", "d_self", "d_agg", "self_contrib", "rel_contrib", "neigh_contrib")


@pytest.fixture(scope="module")
def cases():
    out = {}
    for shape in A.SHAPES:
        c = A.GradCase.of(shape)
        whole = A.sets_to_index(A.host_test_sets(c, np.arange(c.n)))
        out[shape] = (c, whole)
    return out


def index_of(whole, ids):
    """the whole graph's index restricted to ids (row b <- node ids[b]): per relation (rows, cols, counts)"""
    out = []
    for rows, cols, cnt in whole:
        start = torch.cat((torch.zeros(1, dtype=torch.long), cnt.long().cumsum(0)))
        pick = [torch.arange(int(start[v]), int(start[v + 1])) for v in ids]
        sel = torch.cat(pick) if pick else torch.zeros(0, dtype=torch.long)
        c = cnt[torch.as_tensor(np.asarray(ids)).long()]
        out.append((torch.repeat_interleave(torch.arange(len(ids)), c.long()), cols[sel], c))
    return out


@pytest.mark.parametrize("shape", list(A.SHAPES))
def test_reference_is_consistent_and_the_cases_keep_the_kink_condition(cases, shape):
    c, whole = cases[shape]
    assert all(float(cnt.min()) >= 1 for _, _, cnt in whole), "no row of these graphs has an empty set"
    for name, ids in A.id_sets(c).items():
        index = index_of(whole, ids)
        for target in A.TARGETS:
            r64 = A.attr_ref(c.X, ids, index, c.params(), target, torch.float64)
            man = A.attr_manual(c.X, ids, index, c.params(), target, torch.float64)
            for k in KEYS:
                assert A.rel_err(man[k], r64[k]) <= 1e-12, (name, target, k)
            assert A.residual(r64, target) <= 1e-12, (name, target)
            start = 0
            for r, (rows, _, _) in enumerate(index):
                sums = torch.zeros(len(ids), dtype=torch.float64).index_add_(0, rows, r64["neigh_contrib"][start:start + rows.numel()])
                start += rows.numel()
                assert A.rel_err(sums, r64["rel_contrib"][r]) <= 1e-12, (name, target, r)
        r64 = A.attr_ref(c.X, ids, index, c.params(), A.TARGETS[0], torch.float64)
        r32 = A.attr_ref(c.X, ids, index, c.params(), A.TARGETS[0], torch.float32)
        keep, share = A.kept_rows(r64["pre"], r32["pre"])
        # the margin: the batches keep the condition with the band doubled, the whole graph with a quarter added
        wide = A.kept_rows(r64["pre"], r32["pre"], widen=1.25 if name == "whole" else 2.0)[1]
        assert wide <= A.ROW_CAP, f"{shape} {name}: {wide:.2%} of the rows are ambiguous in the widened band"
        print(f"{shape} {name}: {int((~keep).sum())}/{len(ids)} rows left out; e_f32 d_self {A.rel_err(r32['d_self'][keep], r64['d_self'][keep]):.2e} "
              f"residual_f32 {A.residual(r32, A.TARGETS[0]):.2e}")
        assert share <= A.ROW_CAP, f"{shape} {name}: {share:.2%} of the rows have an ambiguous pre-activation - change the seed"


def test_a_dropped_neighbour_moves_the_result_beyond_the_tolerance(cases):
    """the bound the GPU test applies tells a wrong selection from rounding: one chosen row dropped from one set"""
    c, whole = cases[(32, 64, 3)]
    ids = c.batch(17)[0]
    index = index_of(whole, ids)
    r64 = A.attr_ref(c.X, ids, index, c.params(), A.TARGETS[0], torch.float64)
    r32 = A.attr_ref(c.X, ids, index, c.params(), A.TARGETS[0], torch.float32)
    rows, cols, cnt = index[1]
    b = int(torch.argmax(cnt))
    drop = int((rows == b).nonzero()[0])
    keep = torch.ones(rows.numel(), dtype=torch.bool)
    keep[drop] = False
    cnt2 = cnt.clone()
    cnt2[b] -= 1
    bad = A.attr_ref(c.X, ids, [index[0], (rows[keep], cols[keep], cnt2), index[2]], c.params(), A.TARGETS[0], torch.float64)
    for k in ("d_agg", "rel_contrib"):
        assert A.rel_err(bad[k], r64[k]) > 10 * A.tolerance(A.rel_err(r32[k], r64[k])), k


def test_long_row_case_keeps_the_kink_condition():
    """the explicit long-row graph: the kept counts it is built for, no ambiguous row among the 24 the GPU test compares
    (2 % of 24 rows is less than one row)"""
    c = A.LongRowCase()
    ids = c.long_ids()
    assert len(ids) % 16 != 0 and A.ISOLATED not in ids
    sets = A.host_test_sets(c, ids)
    for r in range(3):
        assert [len(s) for s in sets[r][:4]] == A.LONG_KEPT
    index = A.sets_to_index(sets)
    r64 = A.attr_ref(c.X, ids, index, c.params(), A.TARGETS[0], torch.float64)
    r32 = A.attr_ref(c.X, ids, index, c.params(), A.TARGETS[0], torch.float32)
    keep, share = A.kept_rows(r64["pre"], r32["pre"], widen=2.0)
    assert share <= A.ROW_CAP, f"{int((~keep).sum())} of {len(ids)} rows ambiguous in the doubled band - change the seed"
    assert A.residual(r64, A.TARGETS[0]) <= 1e-12
    iso = A.host_test_sets(c, c.tile_with_isolated())
    assert [len(s) for s in iso[1]].count(0) == 1 and len(iso[1][7]) == 0
