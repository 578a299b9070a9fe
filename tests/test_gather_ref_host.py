"""CPU-only tests of the oracle the gather geometry matrix is checked with (tests/gather_ref.py): the matrix covers every
geometry edge, the integer data cannot round, a lost, doubled or chunk-wise lost list entry is far outside the Gaussian bound,
and a table wider than the gather kernels' 512 floats is refused on the host."""
import numpy as np
import pytest
import torch

from tests import dense_ref as D
from tests import gather_ref as G


@pytest.fixture(scope="module")
def graph():
    return G.geometry_graph()


@pytest.fixture(scope="module")
def data():
    return G.tables()


def test_matrix_covers_every_geometry_edge(graph):
    indptr, idx = graph
    deg = np.diff(indptr)
    assert deg[:len(G.DEG)].tolist() == G.DEG and len(set(G.DEG)) == len(G.DEG)
    for v in range(G.N_NODES):
        row = idx[indptr[v]:indptr[v + 1]]
        assert v in row and np.all(np.diff(row) > 0) and row[0] >= 0 and row[-1] < G.N_NODES
    tiers = {}
    for F in G.WIDTHS:
        stride = (F + 3) // 4 * 4
        tiers.setdefault((G.lanes_per_row(stride), 2 if stride > 256 else 1), []).append(F)
    assert sorted(tiers) == [(8, 1), (16, 1), (32, 1), (64, 1), (64, 2)]
    for (lpr, _), widths in tiers.items():
        per_iter = 64 // lpr * 8
        assert {per_iter - 1, per_iter, per_iter + 1} <= set(G.DEG), lpr
        assert any(F % 4 == 0 for F in widths) and any(F % 4 != 0 for F in widths), lpr
    chunks = {(d + G.CHUNK - 1) // G.CHUNK for d in G.DEG}
    assert {1, 2, 3, 8, 9, 16, 17, 18} <= chunks           # CB = 8 and 16 on both sides, a tail of one and of two chunks
    nodes = G.batch_nodes()
    assert sorted(set(nodes.tolist())) == list(range(len(G.DEG))) and len(nodes) == len(G.DEG) + 3


def test_integer_sums_stay_exact(graph, data):
    indptr, idx = graph
    xi, _ = data
    sets = [set(idx[indptr[v]:indptr[v + 1]].tolist()) for v in range(len(G.DEG))]
    sums, cnt = G.int_sums(xi, sets)
    assert cnt.tolist() == G.DEG
    assert int(np.abs(sums).max()) < 2 ** 24 and max(G.DEG) * G.INT_RANGE < 2 ** 24
    # any partial sum too: a subset's sum is bounded by the sum of the absolute values
    assert int(np.stack([np.abs(xi[sorted(s)]).astype(np.int64).sum(0) for s in sets]).max()) < 2 ** 24
    for norm in (0, 1):
        m = G.exact_mean(sums, cnt, norm)
        assert m.dtype == np.float32
        # the same quotient through float64: 53 bits >= 2 * 24 + 2, so rounding it again to float32 is the float32 quotient
        # (the divisor of norm 1 is sqrtf's float32 value, as on the device)
        den = np.sqrt(cnt.astype(np.float32)).astype(np.float64) if norm else cnt.astype(np.float64)
        assert np.array_equal(m, (sums / den[:, None]).astype(np.float32))


@pytest.mark.parametrize("deg", [2177, 129])
def test_a_wrong_list_is_ten_tolerances_away(graph, data, deg):
    """one entry dropped, one counted twice, one chunk's partial sum lost (the first and the last chunk), each with the count
    left as it was: rel_err of the row moves by more than ten times the bound the GPU test allows it"""
    indptr, idx = graph
    _, xg = data
    v = G.DEG.index(deg)
    row = idx[indptr[v]:indptr[v + 1]].astype(np.int64)
    assert len(row) == deg
    X = xg[:, :G.MAX_WIDTH]
    ref = G.mean_f64(X, row)
    e_32 = D.rel_err(G.mean_f32_sequential(X, row), ref)
    tol = D.tolerance(e_32)
    total = X[row].astype(np.float64).sum(0)
    last0 = (deg - 1) // G.CHUNK * G.CHUNK
    variants = {"one entry dropped": total - X[row[deg // 2]],
                "one entry twice": total + X[row[deg // 3]],
                "first chunk lost": total - X[row[:G.CHUNK]].astype(np.float64).sum(0),
                "last chunk lost": total - X[row[last0:]].astype(np.float64).sum(0)}
    for what, s in variants.items():
        moved = D.rel_err(s / deg, ref)
        print(f"deg {deg} {what:18s} moved {moved:.3e}  e_f32 {e_32:.3e}  tolerance {tol:.3e}  x{moved / tol:.0f}")
        assert moved > 10 * tol, what
    assert e_32 < 1e-5                                      # (the yardstick itself is a float32 rounding, not a defect)


def test_table_wider_than_512_is_refused_on_the_host():
    """stride > 512: DeviceGraph raises before anything is allocated or launched"""
    import pcgnn_amd
    from pcgnn_amd import _lib
    indptr = np.arange(5, dtype=np.int64)
    with pytest.raises(_lib.PcgnnLibraryError, match="513"):
        pcgnn_amd.DeviceGraph(np.zeros((4, 513), dtype=np.float32), [(indptr, np.arange(4, dtype=np.int32))], [],
                              torch.device("cuda", 0))
