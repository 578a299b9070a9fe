"""tests/ranked_ref.py - the oracle of the ranked-selection GPU tests - against the reference's own ``samp_scores``
(tests/golden/ranked.npz, recorded from the imported reference by make_golden_ranked.py).  CPU only."""
import os

import numpy as np
import pytest

from tests.ranked_ref import compare_with_golden, ranked_ref
from tests.util import GOLDEN, GoldenCase

CASES = ["yelp_small", "single_rel", "five_rel"]


@pytest.fixture(scope="module")
def ranked():
    return np.load(os.path.join(GOLDEN, "ranked.npz"))


@pytest.mark.parametrize("name", CASES)
def test_ranked_ref_reproduces_reference(ranked, name):
    c = GoldenCase(name)
    assert np.array_equal(ranked[f"{name}_nodes"], np.asarray(c.nodes))
    thresholds = [0.5] * c.R
    s0 = np.ascontiguousarray(c.z["table_scores"][:, 0])
    offsets, ids, dist = ranked_ref(c.csr, c.nodes, s0, thresholds)
    compare_with_golden(ranked, c, offsets, ids, dist, thresholds)
