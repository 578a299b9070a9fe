"""utils.metrics_from_counts (pure host): from the integer counts of an evaluation pass to every reported metric, ``==``
(float equality, no tolerance) the host functions that work on the probabilities themselves."""
import numpy as np
import pytest

from tests.eval_ref import counts_numpy, scores

CASES = {
    "yelp_share": dict(n=27573, pos_share=0.145, seed=1, kind="continuous"),
    "heavy_ties": dict(n=27573, pos_share=0.145, seed=2, kind="tied"),
    "all_equal": dict(n=5000, pos_share=0.3, seed=3, kind="equal"),
    "positives_majority": dict(n=20000, pos_share=0.9, seed=4, kind="continuous"),
    "edges": dict(n=4000, pos_share=0.5, seed=5, kind="edges"),
}


def _host(prob, y, th=None):
    from pcgnn_amd import utils as U
    m = U.binary_metrics(y, prob.argmax(axis=1), prob[:, 1])
    best = U.get_best_f1(y, prob[:, 1], th)
    return m, best


@pytest.mark.parametrize("name", sorted(CASES))
def test_metrics_from_counts_equal_host_functions(name):
    from pcgnn_amd import utils as U
    prob, y = scores(**CASES[name])
    got = U.metrics_from_counts(counts_numpy(prob, y))
    want, (best_f1, best_t) = _host(prob, y)
    for k, v in want.items():
        assert got[k] == v, (k, got[k], v)
    assert got["auc"] == U.roc_auc(y, prob[:, 1])
    assert (got["best_f1"], got["best_threshold"]) == (best_f1, best_t)
    th = np.linspace(0.01, 0.99, 100)
    assert (got["best_index"] >= 0 and th[got["best_index"]] == best_t) or (got["best_index"] == -1 and best_t == 0.0)
    for i in (0, 17, 49, 99):                                        # test_f1's F1-macro at a threshold
        preds = (prob[:, 1] > th[i]).astype(np.int64)
        assert got["f1_macro_at"][i] == 0.5 * (U._prf(y, preds, 1)[2] + U._prf(y, preds, 0)[2]), i
    if name == "all_equal":
        assert got["auc"] == 0.5


def test_single_threshold():
    from pcgnn_amd import utils as U
    prob, y = scores(27573, 0.145, 6)
    for cut in (0.37, 0.0, 1.0):
        got = U.metrics_from_counts(counts_numpy(prob, y, [cut]), [cut])
        preds = (prob[:, 1] > cut).astype(np.int64)
        assert got["f1_macro_at"] == [0.5 * (U._prf(y, preds, 1)[2] + U._prf(y, preds, 0)[2])]
        assert (got["best_f1"], got["best_threshold"]) == U.get_best_f1(y, prob[:, 1], [cut])
        assert got["auc"] == U.roc_auc(y, prob[:, 1])


def test_one_class_absent_raises_like_roc_auc():
    from pcgnn_amd import utils as U
    prob, _ = scores(500, 0.5, 7)
    for y in (np.zeros(500, np.int32), np.ones(500, np.int32)):
        with pytest.raises(ValueError) as host:
            U.binary_metrics(y, prob.argmax(axis=1), prob[:, 1])
        with pytest.raises(ValueError) as dev:
            U.metrics_from_counts(counts_numpy(prob, y))
        assert str(dev.value) == str(host.value)


def test_word_count_is_checked():
    from pcgnn_amd import utils as U
    with pytest.raises(ValueError):
        U.metrics_from_counts(np.zeros(12, np.uint64))
