"""tests/nearest_ref.py against a brute-force sort of explicit (score, position) tuples - random and tie-heavy inputs, the id
exclusion, the padding, the metrics' definitions on hand-made rows.  No GPU, no oracle."""
import math

import numpy as np
import pytest

from tests import nearest_ref as N


def brute(Q, bank, k, metric, q_ids=None, bank_ids=None):
    """python floats (float64), one pair at a time, sorted() on (-score, position)"""
    out_p, out_s = [], []
    for i, q in enumerate(Q):
        rows = []
        for c, b in enumerate(bank):
            if q_ids is not None and int(q_ids[i]) == int(bank_ids[c]):
                continue
            dot = math.fsum(float(x) * float(y) for x, y in zip(q, b))
            qn2 = math.fsum(float(x) * float(x) for x in q)
            cn2 = math.fsum(float(y) * float(y) for y in b)
            if metric == "dot":
                s = dot
            elif metric == "l2":
                s = min(0.0, 2.0 * dot - qn2 - cn2)
            else:
                s = dot / (math.sqrt(qn2) * math.sqrt(cn2)) if qn2 > 0 and cn2 > 0 else 0.0
            rows.append((-s, c))
        rows.sort()
        rows = rows[:k]
        out_p.append([c for _, c in rows] + [-1] * (k - len(rows)))
        out_s.append([-s for s, _ in rows] + [-math.inf] * (k - len(rows)))
    return np.array(out_p, dtype=np.int32).reshape(len(Q), k), np.array(out_s, dtype=np.float64).reshape(len(Q), k)


@pytest.mark.parametrize("metric", N.METRICS)
@pytest.mark.parametrize("n,M,E,k", [(1, 1, 16, 1), (7, 33, 16, 5), (5, 3, 32, 8), (3, 0, 16, 4), (9, 40, 16, 40)])
def test_random_inputs(metric, n, M, E, k):
    rs = np.random.RandomState(n * 100 + M)
    Q, bank = rs.randn(n, E).astype(np.float32), rs.randn(M, E).astype(np.float32)
    pos, sc = N.topk_similar_ref(Q, bank, k, metric)
    bp, bs = brute(Q, bank, k, metric)
    assert np.array_equal(pos, bp)
    assert np.allclose(sc, bs, rtol=1e-12, atol=1e-12)
    assert pos.shape == (n, k) and pos.dtype == np.int32 and sc.dtype == np.float64
    assert ((pos == -1) == np.isneginf(sc)).all()
    assert (pos[:, min(M, k):] == -1).all() and (pos[:, :min(M, k)] >= 0).all()


@pytest.mark.parametrize("metric", N.METRICS)
def test_tie_heavy_integer_inputs(metric):
    """values in {-1, 0, 1}: many equal scores, duplicated bank rows, all-zero rows - every score exact in float64"""
    rs = np.random.RandomState(5)
    Q = rs.randint(-1, 2, size=(12, 16)).astype(np.float32)
    bank = rs.randint(-1, 2, size=(50, 16)).astype(np.float32)
    bank[10:30] = bank[10]                      # a block of duplicates
    bank[40] = 0
    Q[3] = 0
    for k in (1, 7, 50, 64):
        pos, sc = N.topk_similar_ref(Q, bank, k, metric)
        bp, bs = brute(Q, bank, k, metric)
        assert np.array_equal(pos, bp) and np.array_equal(sc, bs)
    pos, sc = N.topk_similar_ref(Q, bank, 50, metric)
    for i in range(12):                          # sorted, ties by position
        for j in range(49):
            assert sc[i, j] > sc[i, j + 1] or (sc[i, j] == sc[i, j + 1] and pos[i, j] < pos[i, j + 1])
    if metric == "cosine":
        assert (N.scores(Q, bank, metric)[3] == 0).all() and (N.scores(Q, bank, metric)[:, 40] == 0).all()
        assert np.array_equal(pos[3], np.arange(50))            # all scores equal: order by position


def test_exclusion_and_padding():
    rs = np.random.RandomState(2)
    bank = rs.randn(6, 16).astype(np.float32)
    Q = bank[[4, 1]].copy()
    q_ids, bank_ids = np.array([104, 101]), 100 + np.arange(6)
    pos, sc = N.topk_similar_ref(Q, bank, 3, "cosine")
    assert pos[0, 0] == 4 and pos[1, 0] == 1 and np.allclose(sc[:, 0], 1.0)
    pos, sc = N.topk_similar_ref(Q, bank, 3, "cosine", q_ids, bank_ids)
    assert 4 not in pos[0] and 1 not in pos[1]
    bp, bs = brute(Q, bank, 3, "cosine", q_ids, bank_ids)
    assert np.array_equal(pos, bp)
    # fewer eligible rows than k: every bank row carries the query's id but two
    ids = np.array([7, 7, 7, 8, 7, 9])
    pos, sc = N.topk_similar_ref(Q[:1], bank, 4, "dot", np.array([7]), ids)
    assert sorted(pos[0, :2].tolist()) == [3, 5] and pos[0, 2:].tolist() == [-1, -1] and np.isneginf(sc[0, 2:]).all()
    with pytest.raises(ValueError):
        N.topk_similar_ref(Q, bank, 3, "dot", q_ids, None)
    with pytest.raises(ValueError):
        N.scores(Q, bank, "manhattan")


def test_metric_definitions():
    Q = np.array([[3.0, 4.0] + [0.0] * 14], dtype=np.float32)
    bank = np.array([[3.0, 4.0] + [0.0] * 14, [4.0, -3.0] + [0.0] * 14, [0.0] * 16, [6.0, 8.0] + [0.0] * 14], dtype=np.float32)
    assert N.scores(Q, bank, "dot").tolist() == [[25.0, 0.0, 0.0, 50.0]]
    assert N.scores(Q, bank, "cosine").tolist() == [[1.0, 0.0, 0.0, 1.0]]
    assert N.scores(Q, bank, "l2").tolist() == [[0.0, -50.0, -25.0, -25.0]]
    pos, _ = N.topk_similar_ref(Q, bank, 4, "l2")
    assert pos.tolist() == [[0, 2, 3, 1]]
