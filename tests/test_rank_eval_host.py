"""The host side of the ranking metrics (utils.average_precision, precision_recall_at_k, conf_gmean, ranking_from_counts), the
numpy restatement the GPU tests compare against (tests/rank_eval_ref.py), and the argument checks of pcg_pr_counts /
pcg_topk_alerts, which return before any launch.  No GPU."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from tests.rank_eval_ref import alerts_numpy, average_precision_numpy, pr_counts_numpy, scores

EPS = 2.0 ** -53


def exact_ap(prob, y) -> Fraction:
    """sum over the distinct positive scores u of (#{y = 1, p1 == u} / n1) * (#{y = 1, p1 >= u} / #{p1 >= u}), exactly -
    counted directly, not through the functions under test"""
    p = prob[:, 1].astype(np.float64)
    pos = p[y == 1]
    n1 = len(pos)
    total = Fraction(0)
    al = np.sort(p)
    ps = np.sort(pos)
    for u in np.unique(pos):
        tp = n1 - int(np.searchsorted(ps, u, side="left"))
        same = int(np.searchsorted(ps, u, side="right")) - int(np.searchsorted(ps, u, side="left"))
        npred = len(al) - int(np.searchsorted(al, u, side="left"))
        total += Fraction(same * tp, n1 * npred)
    return total


AP_CASES = [(1, 1.0, "continuous"), (2, 0.5, "continuous"), (65, 0.3, "tied"), (1000, 0.145, "continuous"), (1000, 0.9, "edges"),
            (5000, 0.5, "tied"), (5000, 0.145, "equal"), (27573, 0.01, "continuous"), (70_000, 0.02, "continuous"),
            (70_000, 0.145, "tied"), (70_000, 0.5, "edges")]


@pytest.mark.parametrize("n,share,kind", AP_CASES)
def test_average_precision_is_the_exact_sum(n, share, kind):
    from pcgnn_amd import utils as U
    prob, y = scores(n, share, n % 997 + 3, kind)
    if n == 1:
        y[:] = 1
    exact = exact_ap(prob, y)
    ref, got = average_precision_numpy(prob, y), U.average_precision(y, prob[:, 1])
    gap = abs(Fraction(got) - exact) / exact
    print(f"n {n} {kind}: AP {got!r}, G {int(pr_counts_numpy(prob, y)[0][6])}, relative gap {float(gap) / EPS:.3f} * 2^-53")
    assert got == ref                                              # (the same statement on the same integers)
    assert gap <= 5 * Fraction(EPS)                                # three roundings per term, one for the sum


@pytest.mark.parametrize("n,share,kind", AP_CASES[1:])
def test_average_precision_against_sklearn(n, share, kind):
    metrics = pytest.importorskip("sklearn.metrics")
    from pcgnn_amd import utils as U
    prob, y = scores(n, share, n % 997 + 3, kind)
    want = float(metrics.average_precision_score(y, prob[:, 1]))
    got = U.average_precision(y, prob[:, 1])
    G = int(pr_counts_numpy(prob, y)[0][6])
    assert abs(got - want) <= (G + 4) * EPS * want, (got, want, G)   # any summation order over non-negative terms


def test_pr_points_equal_the_reference_and_need_a_positive():
    from pcgnn_amd import utils as U
    for n, share, kind in AP_CASES[1:8]:
        prob, y = scores(n, share, 7, kind)
        hdr, tp, npred = pr_counts_numpy(prob, y)
        n1, tp2, npred2 = U.pr_points(y, prob[:, 1])
        assert n1 == int(hdr[4]) and np.array_equal(tp2, tp) and np.array_equal(npred2, npred)
        assert int(hdr[6]) == len(tp) <= n1 and np.all(np.diff(tp.astype(np.int64)) > 0) and np.all(tp <= npred)
    with pytest.raises(ValueError):
        U.average_precision(np.zeros(5, int), np.linspace(0, 1, 5))
    with pytest.raises(ValueError):
        U.average_precision([0, 1, 2], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError):
        U.average_precision([0, 1, 1], [0.1, np.nan, 0.3])


def test_conf_gmean_is_the_references_expression():
    from pcgnn_amd import utils as U
    for tn, fp, fn, tp in ((5, 1, 2, 7), (90, 10, 3, 1), (1, 0, 0, 1), (3, 4, 5, 0), (0, 8, 1, 6), (123456, 789, 1011, 1213)):
        conf = np.array([[tn, fp], [fn, tp]])
        assert U.conf_gmean(conf) == (tp * tn / ((tp + fn) * (tn + fp))) ** 0.5
    for conf in ([[0, 0], [2, 3]], [[4, 1], [0, 0]]):
        with pytest.raises(ValueError, match="Only one class"):
            U.conf_gmean(np.array(conf))


def test_precision_recall_at_k_resolves_ties_by_position():
    from pcgnn_amd import utils as U
    #            0    1    2    3    4    5    6    7
    s = np.array([0.5, 0.9, 0.5, 0.5, 0.1, 0.5, 0.9, -0.0], dtype=np.float32)
    y = np.array([0, 1, 1, 0, 1, 1, 0, 0])
    assert U.alert_order(s).tolist() == [1, 6, 0, 2, 3, 5, 4, 7]       # (0.9: 1 before 6; 0.5: 0, 2, 3, 5 by position)
    prec, rec = U.precision_recall_at_k(y, s, (1, 2, 3, 4, 5, 6, 8, 20))
    # the tie group 0.5 straddles k = 3, 4, 5: row 0 (y = 0) enters before row 2 (y = 1) although both score 0.5
    assert prec == {1: 1 / 1, 2: 1 / 2, 3: 1 / 3, 4: 2 / 4, 5: 2 / 5, 6: 3 / 6, 8: 4 / 8, 20: 4 / 8}
    assert rec == {1: 1 / 4, 2: 1 / 4, 3: 1 / 4, 4: 2 / 4, 5: 2 / 4, 6: 3 / 4, 8: 4 / 4, 20: 4 / 4}
    # the same scores in another input order: another list at the cut (that is the rule), the same totals
    flip = np.arange(8)[::-1]
    prec2, _ = U.precision_recall_at_k(y[flip], s[flip], (3, 8))
    assert prec2 == {3: 2 / 3, 8: 4 / 8}
    # -0.0 ties with +0.0: position decides
    z = np.array([0.0, -0.0, 0.0], dtype=np.float32)
    assert U.alert_order(z).tolist() == [0, 1, 2] and alerts_numpy(z, 5)[0].tolist() == [0, 1, 2, -1, -1]
    pos, sc = alerts_numpy(s, 3)
    assert pos.tolist() == [1, 6, 0] and sc.tolist() == [s[1], s[6], s[0]]
    with pytest.raises(ValueError):
        U.precision_recall_at_k(y, s, (0,))
    with pytest.raises(ValueError):
        U.precision_recall_at_k(np.zeros(8, int), s, (3,))


def test_host_ranking_and_ranking_from_counts_agree():
    from pcgnn_amd import utils as U
    for n, share, kind in ((1000, 0.145, "continuous"), (5000, 0.5, "tied"), (3000, 0.3, "edges"), (2000, 0.2, "equal")):
        prob, y = scores(n, share, 21, kind)
        hdr, tp, npred = pr_counts_numpy(prob, y)
        m = U.ranking_from_counts(hdr, tp, npred)
        h = U.host_ranking(y, prob, (1, 10, 100, n + 3))
        tpc, fpc, fnc, tnc = (int(v) for v in hdr[:4])
        assert m["average_precision"] == h["average_precision"] == U.average_precision(y, prob[:, 1])
        assert m["gmean"] == h["gmean"] == U.conf_gmean([[tnc, fpc], [fnc, tpc]])
        assert (m["n_pos"], m["n_neg"], m["n_points"]) == (int(y.sum()), n - int(y.sum()), len(tp)) and h["n_points"] == len(tp)
        assert (h["precision_at"], h["recall_at"]) == U.precision_recall_at_k(y, prob[:, 1], (1, 10, 100, n + 3))


def test_ranking_from_counts_rejects_an_inconsistent_header():
    from pcgnn_amd import utils as U
    tp = np.array([1, 2, 3], np.uint32)
    npred = np.array([1, 3, 6], np.uint32)
    good = np.array([2, 1, 1, 4, 3, 5, 3, 0], np.uint64)
    assert U.ranking_from_counts(good, tp, npred)["n_points"] == 3
    more = good.copy()
    more[6] = 4                                                       # G > n1
    with pytest.raises(ValueError, match="4 points for 3 positives"):
        U.ranking_from_counts(more, np.arange(1, 5), np.arange(1, 5))
    with pytest.raises(ValueError):
        U.ranking_from_counts(good, tp[:2], npred[:2])                # fewer entries than G
    with pytest.raises(ValueError):
        U.ranking_from_counts(good[:7], tp, npred)
    one = np.array([0, 0, 0, 0, 0, 0, 0, 0], np.uint64)
    with pytest.raises(ValueError, match="Only one class"):
        U.ranking_from_counts(one, tp[:0], npred[:0])


def test_argument_errors_before_any_launch():
    from pcgnn_amd import _lib
    lib = _lib.load()
    E, K = _lib.PCG_E_ARG, _lib.PCG_ALERTS_MAX_K
    assert K >= 4096
    assert lib.pcg_pr_workspace_bytes(-1) == E and lib.pcg_pr_workspace_bytes(1 << 31) == E
    assert lib.pcg_pr_workspace_bytes(0) > 0 and lib.pcg_pr_workspace_bytes((1 << 31) - 1) > 0
    assert lib.pcg_topk_alerts_workspace_bytes(-1, 10) == E and lib.pcg_topk_alerts_workspace_bytes(1 << 31, 10) == E
    assert lib.pcg_topk_alerts_workspace_bytes(100, 0) == E and lib.pcg_topk_alerts_workspace_bytes(100, K + 1) == E
    assert lib.pcg_topk_alerts_workspace_bytes(0, 1) > 0 and lib.pcg_topk_alerts_workspace_bytes((1 << 31) - 1, K) > 0
    buf = (C.c_uint64 * 64)()                                         # a valid, aligned host address: nothing may touch it
    a = C.addressof(buf)
    N = None
    assert lib.pcg_pr_counts(N, N, 5, 5, N, N, N, N, N, N) == E
    assert lib.pcg_pr_counts(a, a, -1, 5, a, a, a, a, a, N) == E
    assert lib.pcg_pr_counts(a, a, 1 << 31, 5, a, a, a, a, a, N) == E
    assert lib.pcg_pr_counts(a, a, 5, -1, a, a, a, a, a, N) == E
    for hole in (0, 1, 4, 5, 6, 7, 8):
        args = [a, a, 5, 5, a, a, a, a, a]
        args[hole] = N
        assert lib.pcg_pr_counts(*args, N) == E, f"NULL argument {hole}"
    assert lib.pcg_pr_counts(a + 4, a, 5, 5, a, a, a, a, a, N) == E    # prob is read as float2
    assert lib.pcg_topk_alerts(N, 1, 5, 3, N, N, N, N, N) == E
    assert lib.pcg_topk_alerts(a, 1, -1, 3, a, a, a, a, N) == E
    assert lib.pcg_topk_alerts(a, 1, 1 << 31, 3, a, a, a, a, N) == E
    assert lib.pcg_topk_alerts(a, 1, 5, 0, a, a, a, a, N) == E
    assert lib.pcg_topk_alerts(a, 1, 5, K + 1, a, a, a, a, N) == E
    assert lib.pcg_topk_alerts(a, 0, 5, 3, a, a, a, a, N) == E
    for hole in (0, 4, 5, 6, 7):
        args = [a, 1, 5, 3, a, a, a, a]
        args[hole] = N
        assert lib.pcg_topk_alerts(*args, N) == E, f"NULL argument {hole}"
    assert all(v == 0 for v in buf)


def test_ops_reject_the_cpu_and_bad_shapes():
    import torch
    from pcgnn_amd import _lib, ops
    with pytest.raises(_lib.PcgnnLibraryError):
        ops.pr_counts(torch.zeros(4, 2), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(_lib.PcgnnLibraryError):
        ops.topk_alerts(torch.zeros(4, 2), 2)
