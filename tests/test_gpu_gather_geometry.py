"""The gather + combine geometry matrix: every row geometry of the aggregation path (csrc/gather.hip) against an exact oracle
and against float64.  Run with ``pytest -m gpu`` on an MI355X.

One hand-built relation of 2300 nodes (tests/gather_ref.py) whose 25 centre rows have exactly the degrees at which the path
changes: per_iter +- 1 of every lanes-per-row tier (7 8 9, 15 16 17, 31 32 33, 63 64 65), the 128-entry chunk edges (127 128 129,
255 256 257), the combine-batch edges (1024 | 1025: 8 | 9 chunks, 2048 | 2049: 16 | 17, 2176 | 2177: 17 | 18) and degree 1; the
batch is every centre once, shuffled, and three of them again.  Test mode with threshold 1.0 keeps every neighbour (the keep-all
rule), so a row's list is its neighbour row and ``cnt == DEG`` is asserted.  Eighteen feature widths - both sides of every tier
edge (stride 32 | 64 | 128 | 256 | 512), each with a ragged and a full last float4 -, so gather_chunks<1> / <2>, combine_rows<1>
/ <2> with CB = 16 / 8, store_row's ragged tail and the partial layout all meet a reference at every width.

Two data sets per width:
  exact     X holds integers in [-8, 8]: every partial and total sum (<= 2177 * 8) is exact in float32 in any order, so the mean
            must be ``float32(sum) / float32(cnt)`` BIT FOR BIT (one correctly rounded division; no fast-math flag in the build).
            The same through norm = 1 (``/ sqrtf(cnt)``) and norm = 0 with add_self (the centre is in its row already: the
            set and its count stay, the row's list capacity is one entry more) at F = 32, 100, 260, 512.  No relaxation was
            needed: the device's division and square root are IEEE.
  Gaussian  X ~ N(0, 1): per row e = max|x - x64| / max|x64| against the float64 mean over the device's own set;
            e_kernel <= 8 * e_f32 + 2^-20 (tests/dense_ref.tolerance - the project's bound, not fitted), e_f32 the same mean
            summed entry by entry in float32.  A lost or doubled entry or a lost chunk is more than ten such tolerances away
            (tests/test_gather_ref_host.py).
The output is written into a buffer with a row stride a few floats above F and more rows than the batch, filled with a sentinel:
columns >= F and the rows behind the batch keep it.

The status word: two entries of a multi-chunk row's list overwritten with ``table_rows`` and ``table_rows + 7``
(pcg_aggregate_lists, F = 32 and 260): PCG_ST_LIST_ID_RANGE is set, the row's mean is the exact sum without the two entries over
the unchanged count, every other row keeps its bits; restored, the status is zero and the bits are the clean run's.

Measured on an MI355X (profiles/r17/wide_f64_ratios.txt), Gaussian data, maximised over the 28 rows: `ratio` = e_kernel / e_f32
over the rows with e_f32 >= 2^-24, `of bound` = e_kernel / (8 * e_f32 + 2^-20):

    F     stride  lanes per row  accumulators  ratio  of bound
    1     4       8              1             1.95   0.23
    3     4       8              1             1.12   0.09
    4     4       8              1             1.10   0.07
    5     8       8              1             1.00   0.06
    29    32      8              1             1.00   0.06
    32    32      8              1             1.00   0.06
    33    36      16             1             1.21   0.08
    61    64      16             1             1.29   0.08
    64    64      16             1             1.18   0.08
    65    68      32             1             1.72   0.08
    125   128     32             1             1.17   0.06
    128   128     32             1             1.17   0.06
    129   132     64             1             1.00   0.09
    253   256     64             1             1.00   0.09
    256   256     64             1             1.00   0.09
    257   260     64             2             1.00   0.09
    509   512     64             2             1.00   0.10
    512   512     64             2             1.00   0.10

Every integer-data comparison, at all 18 widths x 28 rows and through both norms with add_self, was bit-exact, and so were the
status-word cases at one and at two accumulators.
"""
import numpy as np
import pytest
import torch

from tests import gather_ref as G

pytestmark = pytest.mark.gpu

PAD_COLS, PAD_ROWS, SENTINEL = 5, 2, -12345.0


@pytest.fixture(scope="module")
def P():
    import pcgnn_amd
    from pcgnn_amd import ops  # noqa: F401  (fails loudly if the .so is missing)
    return pcgnn_amd


@pytest.fixture(scope="module")
def world():
    """the graph, the batch and the two tables, built once"""
    xi, xg = G.tables()
    return dict(csr=G.geometry_graph(), nodes=G.batch_nodes(), int=xi, gauss=xg)


def dev():
    return torch.device("cuda", 0)


def scores():
    return torch.randn(G.N_NODES, generator=torch.Generator().manual_seed(5)).to(dev())


def run(P, world, kind, F, norm=0, add_self=False):
    """test-mode keep-all selection + aggregation of the batch at width F -> (graph, X [n, F], sets, agg [B, F] numpy, cnt)"""
    ops = P.ops
    X = np.ascontiguousarray(world[kind][:, :F])
    g = P.DeviceGraph(X, [world["csr"]], [], dev())
    nodes = torch.from_numpy(world["nodes"]).to(dev())
    sets, agg, cnt = ops.chosen_sets(g, nodes, None, scores(), None, [1.0], 0.5, False, norm=norm, add_self=add_self)
    return g, X, sets[0], agg[0].cpu().numpy(), cnt[0].cpu().numpy()


def assert_sets(world, sets, cnt):
    indptr, idx = world["csr"]
    want = [set(idx[indptr[v]:indptr[v + 1]].tolist()) for v in world["nodes"]]
    assert cnt.tolist() == [G.DEG[v] for v in world["nodes"]], "list length == degree: the matrix must not shrink"
    assert sets == want


def assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    same = got.view(np.uint32) == want.view(np.uint32)
    if not same.all():
        rows = np.flatnonzero(~same.all(axis=1))
        r = int(rows[0])
        cols = np.flatnonzero(~same[r])
        raise AssertionError(f"{what}: {len(rows)} rows differ, first batch row {r} columns {cols[:8].tolist()} "
                             f"got {got[r, cols[:4]].tolist()} want {want[r, cols[:4]].tolist()}")


@pytest.mark.parametrize("F", G.WIDTHS)
def test_integer_data_bit_exact(P, world, F):
    g, X, sets, agg, cnt = run(P, world, "int", F)
    assert_sets(world, sets, cnt)
    sums, n = G.int_sums(X, sets)
    assert agg.shape == (len(world["nodes"]), F)
    assert_bits(agg, G.exact_mean(sums, n), f"F={F}")


@pytest.mark.parametrize("norm", [1, 0])
@pytest.mark.parametrize("F", G.NORM_WIDTHS)
def test_integer_data_bit_exact_with_self_and_norm(P, world, F, norm):
    """choose_aggregate(norm, add_self=True), the GraphSAGE aggregators' call: the self row joins the expected set (it is in
    it already: set and count stay what they were), the sum is divided by sqrt(cnt) (norm 1) or cnt (norm 0)"""
    ops = P.ops
    X = np.ascontiguousarray(world["int"][:, :F])
    g = P.DeviceGraph(X, [world["csr"]], [], dev())
    nodes = torch.from_numpy(world["nodes"]).to(dev())
    agg, cnt = ops.choose_aggregate(g, nodes, None, scores(), None, [1.0], 0.0, False, norm=norm, add_self=True)
    indptr, idx = world["csr"]
    want = [set(idx[indptr[v]:indptr[v + 1]].tolist()) | {int(v)} for v in world["nodes"]]
    assert cnt[0].cpu().tolist() == [len(s) for s in want] == [G.DEG[v] for v in world["nodes"]]
    sums, n = G.int_sums(X, want)
    assert_bits(agg[0].cpu().numpy(), G.exact_mean(sums, n, norm), f"F={F} norm={norm} add_self")


@pytest.mark.parametrize("F", G.WIDTHS)
def test_gaussian_data_against_float64(P, world, F):
    g, X, sets, agg, cnt = run(P, world, "gauss", F)
    assert_sets(world, sets, cnt)
    ratio, of_bound, misses = 0.0, 0.0, []
    for b, s in enumerate(sets):
        e_k, e_32, tol = G.gaussian_row_check(agg[b], X, s)
        if e_32 >= 2.0 ** -24:
            ratio = max(ratio, e_k / e_32)
        of_bound = max(of_bound, e_k / tol)
        print(f"F={F} row {b} deg {len(s)}: e_kernel {e_k:.3e}  e_f32 {e_32:.3e}  bound {tol:.3e}" + ("" if e_k <= tol else "  MISS"))
        if not e_k <= tol:
            misses.append((b, len(s), e_k, e_32, tol))
    print(f"RATIO gather F={F}: ratio {ratio:.2f}  of bound {of_bound:.2f}")
    assert not misses, misses


@pytest.mark.parametrize("F", G.WIDTHS)
def test_output_outside_the_rows_is_untouched(P, world, F):
    """agg with a row stride of F + 5 and two rows behind the batch, a sentinel everywhere first: the kernels write columns
    < F of the batch's rows (the same bits as into a dense output) and nothing else"""
    ops = P.ops
    g, X, sets, dense, cnt0 = run(P, world, "int", F)
    nodes = torch.from_numpy(world["nodes"]).to(dev())
    B = nodes.numel()
    buf = torch.full((1, B + PAD_ROWS, F + PAD_COLS), SENTINEL, dtype=torch.float32, device=dev())
    agg = buf[:, :B, :F]
    assert agg.stride(-2) == F + PAD_COLS and agg.data_ptr() == buf.data_ptr()
    cnt = torch.empty(1, B, dtype=torch.int32, device=dev())
    ws = ops.ChooseWorkspace(g, B, list_capacity=int(sum(G.DEG[v] for v in world["nodes"])))
    ops.choose_aggregate(g, nodes, None, scores(), None, [1.0], 0.5, False, ws=ws, agg=agg, cnt=cnt)
    torch.cuda.synchronize()
    ws.check()
    out = buf[0].cpu().numpy()
    assert cnt[0].cpu().tolist() == cnt0.tolist()
    assert_bits(out[:B, :F], dense, f"F={F} strided output")
    assert np.all(out[:B, F:] == SENTINEL), "columns >= F"
    assert np.all(out[B:] == SENTINEL), "rows behind the batch"


@pytest.mark.parametrize("F", [32, 260])
def test_list_entry_outside_the_table_sets_the_status_word(P, world, F):
    from pcgnn_amd import _lib
    ops = P.ops
    X = np.ascontiguousarray(world["int"][:, :F])
    g = P.DeviceGraph(X, [world["csr"]], [], dev())
    nodes = torch.from_numpy(world["nodes"]).to(dev())
    B = nodes.numel()
    ws = ops.ChooseWorkspace(g, B, list_capacity=int(sum(G.DEG[v] for v in world["nodes"])))
    cnt = torch.empty(B, dtype=torch.int32, device=dev())
    ops.choose_select(g, nodes, None, scores(), None, [1.0], 0.5, False, ws, cnt)
    sets = ops.read_sets(g, B, ws)[0]
    assert_sets(world, sets, cnt.cpu().numpy())

    def aggregate():
        agg = torch.full((1, B, F), SENTINEL, dtype=torch.float32, device=dev())
        ops.aggregate_lists(g, g.X, B, ws, cnt, agg)
        torch.cuda.synchronize()
        st = int(ws.status.item())
        ws.status.zero_()
        return agg[0].cpu().numpy(), st

    clean, st = aggregate()
    assert st == 0
    sums, n = G.int_sums(X, sets)
    assert_bits(clean, G.exact_mean(sums, n), f"F={F} clean")
    # the list of the 2177-entry row (its first occurrence in the batch), laid out as read_sets reads it
    b = int(np.flatnonzero(world["nodes"] == G.DEG.index(2177))[0])
    begin = ws.view(0, torch.int64, B + 1).cpu().numpy()
    length = ws.view(1, torch.int32, B).cpu().numpy()
    assert int(length[b]) == 2177
    lst = ws.view(2, torch.int32, int(begin[-1]))
    at = [int(begin[b]) + 5, int(begin[b]) + 3 * G.CHUNK + 77]               # in the first and in the fourth chunk
    saved = lst[at].clone()
    gone = saved.cpu().tolist()
    assert all(v in sets[b] for v in gone) and len(set(gone)) == 2
    table_rows = g.X.shape[0]
    lst[at] = torch.tensor([table_rows, table_rows + 7], dtype=torch.int32, device=dev())    # just past the end, no further
    bad, st = aggregate()
    assert st & _lib.PCG_ST_LIST_ID_RANGE, "PCG_ST_LIST_ID_RANGE"
    assert st == _lib.PCG_ST_LIST_ID_RANGE
    want = sums.copy()
    want[b] -= X[gone].astype(np.int64).sum(0)
    want = G.exact_mean(want, n)                                             # (the count is the select kernel's: unchanged)
    assert_bits(bad[b:b + 1], want[b:b + 1], f"F={F} the row with two entries outside the table")
    others = np.arange(B) != b
    assert_bits(bad[others], clean[others], f"F={F} the other rows")
    lst[at] = saved
    again, st = aggregate()
    assert st == 0
    assert_bits(again, clean, f"F={F} restored")
