"""The yardstick of the baselines' whole-set tests (tests/baseline_ref.py) reproduces the reference's own outputs - the ``s1_*``
arrays of every golden fixture that has them - within the tolerances tests/test_gpu_parity.py uses for the same arrays.  No GPU."""
import numpy as np
import pytest

from tests import baseline_ref as BR
from tests.baseline_ref import FEAT_TOL, GCN_ENC_TOL
from tests.util import GoldenCase

CASES = BR.s1_cases()


def test_fixtures_found():
    assert {"yelp_small", "amazon_small", "single_rel", "yelp_emb128", "feat100", "five_rel"} <= set(CASES)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_outputs(name, dtype):
    c = GoldenCase(name)
    z, sub = c.z, c.z["s1_nodes"]
    for key, add_self, norm in (("s1_mean", False, 0), ("s1_mean_gcn", True, 0), ("s1_gcn", True, 1)):
        got = BR.aggregate(c.X, c.homo_csr, sub, add_self, norm, dtype)
        np.testing.assert_allclose(got, z[key], rtol=0, atol=FEAT_TOL, err_msg=key)
    # Encoder(gcn=True) over MeanAggregator(gcn=False): what the fixture generator built; GCNEncoder over GCNAggregator
    head = np.zeros((2, c.emb), np.float32)
    for key, shape, tol in (("s1_sage_enc", "sage", FEAT_TOL), ("s1_gcn_enc", "gcn", GCN_ENC_TOL)):
        _, h, _ = BR.forward(c.X, c.homo_csr, sub, z[key + "_w"], head, dtype=dtype, **BR.SHAPES[shape])
        np.testing.assert_allclose(h.T, z[key], rtol=0, atol=tol, err_msg=key)


def test_empty_set_is_nan_and_union_counts_once():
    X = np.arange(12, dtype=np.float32).reshape(4, 3) + 1
    indptr, indices = np.array([0, 0, 2, 3, 4], np.int64), np.array([1, 2, 0, 3], np.int32)   # row 0 empty, rows 1 and 3 hold themselves
    a = BR.aggregate(X, (indptr, indices), [0, 1, 2, 3], False, 0)
    assert np.isnan(a[0]).all() and np.array_equal(a[1], (X[1] + X[2]) / 2) and np.array_equal(a[2], X[0])
    u = BR.aggregate(X, (indptr, indices), [0, 1, 2, 3], True, 1)
    assert np.array_equal(u[0], X[0]) and np.array_equal(u[1], (X[1] + X[2]) / np.sqrt(2.0))
    assert np.array_equal(u[2], (X[0] + X[2]) / np.sqrt(2.0)) and np.array_equal(u[3], X[3])
    W = np.ones((16, 3), np.float32)
    logits, h, _ = BR.forward(X, (indptr, indices), [0, 1], W, np.ones((2, 16), np.float32), False, False, 0)
    assert np.isnan(h[0]).all() and np.isnan(logits[0]).all() and np.isfinite(logits[1]).all()
