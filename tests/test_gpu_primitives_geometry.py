"""The stand-alone primitives at every row geometry: pcg_segment_mean, pcg_gather_rows, pcg_score_rows and pcg_gather_lists.

pcg_segment_mean (one wave per output row, 64 / lpr list entries per wave-instruction, four in flight: p = 4 * 64 / lpr entries
per loop turn; one float4 accumulator per lane up to a stride of 256 floats, two above): the 18 widths of the gather matrix
(tests/gather_ref.py), lists of 1, p - 1, p, p + 1, 3p + 1 and 1000 entries with duplicate ids, 1 / 4 / 5 output rows (a
workgroup takes four), two rows naming the same segment, out_stride = F + 5 and two spare rows.  On the integer table the mean is
gather_ref.exact_mean bit for bit for both norms; on the Gaussian table it keeps gather_ref.gaussian_row_check's bound
(8 * e_f32 + 2^-20 against float64, e_f32 from the sequential float32 sum of the same entries); the sentinel survives in the pad
columns and the spare rows.

pcg_gather_rows / pcg_score_rows: n_ids = 1 and a workgroup's row count - 1, + 0, + 1, ids with duplicates, a padded out_stride;
the rows are X[ids] bit for bit, the scores pcg_score_table's (column 1: the table scored with the classifier's rows swapped).

pcg_gather_lists (the gather half without the combine launch) on the geometry graph at F = 32 and 260: rows of at most 128
entries are pcg_aggregate_lists' bits, and for longer rows the per-chunk partial sums it leaves in the workspace add up, on the
integer table, to the exact row sum.

Measured on an MI355X (the RATIO lines of -s): pcg_segment_mean on the Gaussian table at most 1.31 x e_f32 and 0.12 of the bound
over the 18 widths; everything else in the file is a bit-exact comparison and was bit-exact.
"""
import numpy as np
import pytest
import torch

from tests import dense_ref as D
from tests import front_ref as R
from tests import gather_ref as G

pytestmark = pytest.mark.gpu

PAD_COLS, PAD_ROWS, SENTINEL = 5, 2, -12345.0


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def P():
    import pcgnn_amd
    from pcgnn_amd import ops  # noqa: F401  (fails loudly if the .so is missing)
    return pcgnn_amd


@pytest.fixture(scope="module")
def world():
    xi, xg = G.tables()
    return dict(csr=G.geometry_graph(), nodes=G.batch_nodes(), int=xi, gauss=xg)


def self_loop_graph(P, X):
    n = X.shape[0]
    return P.DeviceGraph(X, [(np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32))], [], dev())


def assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = got.view(np.uint32) == want.view(np.uint32)
    if not same.all():
        rows = np.flatnonzero(~same.reshape(same.shape[0], -1).all(axis=1))
        raise AssertionError(f"{what}: {len(rows)} rows differ, first row {int(rows[0])}: got {got[rows[0]].ravel()[:4].tolist()} "
                             f"want {want[rows[0]].ravel()[:4].tolist()}")


def segment_cases(F, seed):
    """name -> (begin int64 [n_rows], count int32 [n_rows], idx int32): the row sets of 5, 4 and 1 output rows"""
    p = 4 * (64 // G.lanes_per_row(R.stride_of(F)))
    rs = np.random.RandomState(seed)
    out = {}
    for name, lengths, share in (("5 rows", [1, p - 1, p, p + 1, 3 * p + 1], None), ("4 rows", [1000, 3 * p + 1, p + 1, p + 1], (2, 3)),
                                 ("1 row", [1000], None), ("1 row of 1", [1], None)):
        lists = [rs.randint(0, G.N_NODES, size=k).astype(np.int32) for k in lengths]      # (with replacement: duplicate ids)
        for l in lists:
            if l.size >= 3:
                l[-1] = l[0]
        begin, at, parts = [], 7, [rs.randint(0, G.N_NODES, size=7).astype(np.int32)]     # (the first segment does not start at 0)
        for i, l in enumerate(lists):
            if share and i == share[1]:
                begin.append(begin[share[0]])                  # two rows, one segment
                lists[i] = lists[share[0]]
                continue
            begin.append(at)
            parts.append(l)
            at += l.size
        out[name] = (np.array(begin, dtype=np.int64), np.array([l.size for l in lists], dtype=np.int32), np.concatenate(parts), lists)
    return out, p


@pytest.mark.parametrize("F", G.WIDTHS)
def test_segment_mean_every_geometry(P, world, F):
    ops = P.ops
    cases, p = segment_cases(F, 300 + F)
    assert p == {8: 32, 16: 16, 32: 8, 64: 4}[G.lanes_per_row(R.stride_of(F))]
    ratio, of_bound = 0.0, 0.0
    for kind in ("int", "gauss"):
        X = np.ascontiguousarray(world[kind][:, :F])
        g = P.DeviceGraph(X, [world["csr"]], [], dev())
        for name, (begin, count, idx, lists) in cases.items():
            n_rows = len(lists)
            for norm in ((0, 1) if kind == "int" else (0,)):
                buf = torch.full((n_rows + PAD_ROWS, F + PAD_COLS), SENTINEL, device=dev())
                out = buf[:n_rows, :F]
                assert out.stride(0) == F + PAD_COLS
                ops.segment_mean(g, torch.from_numpy(begin).cuda(), torch.from_numpy(count).cuda(), torch.from_numpy(idx).cuda(), norm, out)
                torch.cuda.synchronize()
                got = buf.cpu().numpy()
                assert np.all(got[:n_rows, F:] == SENTINEL), f"F {F} {name}: pad columns"
                assert np.all(got[n_rows:] == SENTINEL), f"F {F} {name}: spare rows"
                for i, l in enumerate(lists):
                    assert np.array_equal(idx[begin[i]:begin[i] + count[i]], l)
                if kind == "int":
                    sums = np.stack([X.astype(np.int64)[l].sum(0) for l in lists])
                    cnt = np.array([l.size for l in lists], dtype=np.int64)
                    assert_bits(got[:n_rows, :F], G.exact_mean(sums, cnt, norm), f"F {F} {name} norm {norm}")
                else:
                    for i, l in enumerate(lists):
                        li = l.astype(np.int64)
                        ref = G.mean_f64(X, li)
                        e32 = D.rel_err(G.mean_f32_sequential(X, li), ref)
                        e = D.rel_err(got[i, :F], ref)
                        tol = D.tolerance(e32)
                        of_bound = max(of_bound, e / tol)
                        if e32 >= 2.0 ** -24:
                            ratio = max(ratio, e / e32)
                        assert e <= tol, (F, name, i, l.size, e, e32, tol)
    print(f"RATIO pcg_segment_mean F={F}: ratio {ratio:.2f}  of bound {of_bound:.2f}")


@pytest.mark.parametrize("F", G.WIDTHS)
def test_gather_rows_and_score_rows_round_a_workgroup(P, world, F):
    from pcgnn_amd import _lib
    lib, ops = _lib.load(), P.ops
    _p, st = ops._p, ops._stream(dev())
    X = np.ascontiguousarray(world["gauss"][:, :F])
    g = self_loop_graph(P, X)
    n = g.n_nodes
    W_np, b_np = R.weights(F, 4)
    W, b = torch.from_numpy(W_np).cuda(), torch.from_numpy(b_np).cuda()
    Wx, bx = torch.from_numpy(W_np[::-1].copy()).cuda(), torch.from_numpy(b_np[::-1].copy()).cuda()
    col0, col1 = ops.score_table(g, W, b), ops.score_table(g, Wx, bx)
    rw = R.rows_per_workgroup_launch(F)
    for n_ids in (1, rw - 1, rw, rw + 1, 3 * rw + 1):
        ids_np = R.shuffled_ids(n, n_ids, 7 * F + n_ids)
        ids_np[0] = n - 1                                      # (the table's last row)
        if n_ids >= 3:
            ids_np[2] = ids_np[1]
            assert np.unique(ids_np).size < n_ids
        ids = torch.from_numpy(ids_np).cuda()
        buf = torch.full((n_ids + PAD_ROWS, F + PAD_COLS), SENTINEL, device=dev())
        _lib.check(lib.pcg_gather_rows(g.desc_ref(), _p(ids), n_ids, _p(buf), F + PAD_COLS, st), "pcg_gather_rows")
        sc = torch.full((n_ids + PAD_ROWS, 2), SENTINEL, device=dev())
        _lib.check(lib.pcg_score_rows(g.desc_ref(), _p(W), _p(b), _p(ids), n_ids, _p(sc), st), "pcg_score_rows")
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert_bits(got[:n_ids, :F], X[ids_np], f"F {F} n_ids {n_ids}: X[ids]")
        assert np.all(got[:n_ids, F:] == SENTINEL) and np.all(got[n_ids:] == SENTINEL), f"F {F} n_ids {n_ids}: pad columns, spare rows"
        assert_bits(sc[:n_ids, 0:1].cpu().numpy(), col0[ids.long()].view(-1, 1).cpu().numpy(), f"F {F} n_ids {n_ids}: column 0")
        assert_bits(sc[:n_ids, 1:2].cpu().numpy(), col1[ids.long()].view(-1, 1).cpu().numpy(), f"F {F} n_ids {n_ids}: column 1")
        assert bool((sc[n_ids:] == SENTINEL).all())


@pytest.mark.parametrize("F", [32, 260])
def test_gather_lists_rows_and_partial_sums(P, world, F):
    from pcgnn_amd import _lib
    lib, ops = _lib.load(), P.ops
    _p, st = ops._p, ops._stream(dev())
    nodes_np = world["nodes"]
    nodes = torch.from_numpy(nodes_np).to(dev())
    B = nodes.numel()
    indptr, idx = world["csr"]
    lists = [idx[indptr[v]:indptr[v + 1]].astype(np.int64) for v in nodes_np]
    deg = np.array([l.size for l in lists])
    short = deg <= G.CHUNK
    assert short.any() and (~short).any() and {129, 2177} <= set(deg.tolist())
    s0 = torch.randn(G.N_NODES, generator=torch.Generator().manual_seed(5)).to(dev())
    for kind in ("int", "gauss"):
        X = np.ascontiguousarray(world[kind][:, :F])
        g = P.DeviceGraph(X, [world["csr"]], [], dev())
        ws = ops.ChooseWorkspace(g, B, list_capacity=int(deg.sum()))
        cnt = torch.empty(B, dtype=torch.int32, device=dev())
        ops.choose_select(g, nodes, None, s0, None, [1.0], 0.5, False, ws, cnt)
        ref = torch.full((1, B, F), SENTINEL, device=dev())
        ops.aggregate_lists(g, g.X, B, ws, cnt, ref)
        buf = torch.full((B + PAD_ROWS, F + PAD_COLS), SENTINEL, device=dev())
        _lib.check(lib.pcg_gather_lists(_p(g.X), g.feat_dim, g.feat_stride, g.n_nodes, B, _p(cnt), g.desc_ref(), B, _p(ws.buf),
                                        ws.list_capacity, _p(buf), F + PAD_COLS, _p(ws.status), st), "pcg_gather_lists")
        torch.cuda.synchronize()
        ws.check()
        assert int(ws.status.item()) == 0 and cnt.cpu().tolist() == deg.tolist()
        got, want = buf.cpu().numpy(), ref[0].cpu().numpy()
        assert_bits(got[:B, :F][short], want[short], f"F {F} {kind}: rows of one chunk are pcg_aggregate_lists' bits")
        assert np.all(got[:B, F:] == SENTINEL) and np.all(got[B:] == SENTINEL), "pad columns, spare rows"
        if kind != "int":
            continue
        cb = ws.view(3, torch.int32, B + 1).cpu().numpy()
        assert np.array_equal(np.diff(cb), (deg + G.CHUNK - 1) // G.CHUNK), "a chunk per 128 list entries"
        part = ws.view(6, torch.float32, int(cb[-1]) * g.feat_stride).view(int(cb[-1]), g.feat_stride).cpu().numpy()
        xi = X.astype(np.int64)
        begin = ws.view(0, torch.int64, B + 1).cpu().numpy()
        lst = ws.view(2, torch.int32, int(begin[-1])).cpu().numpy()
        for r in np.flatnonzero(~short):
            mine = lst[begin[r]:begin[r] + deg[r]].astype(np.int64)        # (the device's own list: the order the chunks cut)
            assert np.array_equal(np.sort(mine), lists[r])
            chunks = part[cb[r]:cb[r + 1], :F]
            for c in range(chunks.shape[0]):                  # every chunk's own sum, then the row's
                assert np.array_equal(chunks[c].astype(np.int64), xi[mine[c * G.CHUNK:(c + 1) * G.CHUNK]].sum(0)), (F, r, c)
            assert np.array_equal(chunks.astype(np.int64).sum(0), xi[lists[r]].sum(0)), (F, r)
        # the complete means of those rows: the exact quotient of the exact sum
        sums = np.stack([xi[l].sum(0) for l in lists])
        assert_bits(want, G.exact_mean(sums, deg.astype(np.int64)), f"F {F}: pcg_aggregate_lists")
