"""The neighbour selection (select.hip) on crafted score tables (tests/select_ref.py): every histogram round, both ways out of the
round loop and every shape of tie across the cut, at every tier limit +-1; the minority window's branches at the sizes of its
64-ary search.  The centre's score is +0.0, so a neighbour's distance key is the bit pattern of its score and the oracle is exact.
tests/test_select_ref_host.py shows (on the CPU) that the cases reach what they are meant for.  Run with ``pytest -m gpu``.

Bars: chosen sets, counts and list lengths exact; aggregated rows within 5e-5 (test_hub_rows_block_and_scratch_paths' bar)."""
import numpy as np
import pytest
import torch

from oracle import pcgnn_oracle as O
from tests import select_ref as S

pytestmark = pytest.mark.gpu

N, FEAT = 34000, 32
AGG_TOL = 5e-5
KEY_CENTRE = {d: S.POOL + i for i, d in enumerate(S.LENGTHS)}                        # centre of the row of length d
MIN_CENTRE = {d: S.POOL + len(S.LENGTHS) + i for i, d in enumerate(S.MINORITY_ROWS)}
ROW_LEN = {**{v: d for d, v in KEY_CENTRE.items()}, **{v: d for d, v in MIN_CENTRE.items()}}


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def P():
    import pcgnn_amd
    from pcgnn_amd import ops  # noqa: F401  (fails loudly if the .so is missing)
    return pcgnn_amd


@pytest.fixture(scope="module")
def world():
    """X and the one relation: a centre's row is the first d nodes of the shared pool 0 .. POOL - 1, ids ascending"""
    X = np.random.RandomState(20).randn(N, FEAT).astype(np.float32)
    deg = np.zeros(N, dtype=np.int64)
    for v, d in ROW_LEN.items():
        deg[v] = d
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = np.concatenate([np.arange(ROW_LEN[v], dtype=np.int32) for v in sorted(ROW_LEN)])
    return X, (indptr, indices), torch.from_numpy(X)


def select(ops, g, nodes, labels, s0, keys, thr, rho, train, add_self=False):
    """ops.chosen_sets with a list capacity well above the exact need (+ the sum of the row lengths), keeping the workspace:
    -> sets[b], agg [B, F], cnt [B], len [B], the raw list segment of every row (with its -1 holes)"""
    nodes_h = np.asarray(nodes, dtype=np.int64)
    labels_h = None if labels is None else np.asarray(labels, dtype=np.int64)
    cap = int(ops.sel_capacity(g, nodes_h, labels_h, [thr], rho, train, add_self).sum()) + int(sum(ROW_LEN[v] for v in nodes))
    ws = ops.ChooseWorkspace(g, len(nodes), list_capacity=cap)
    nodes_d = torch.tensor(nodes, dtype=torch.int32, device=dev())
    labels_d = None if labels is None else torch.tensor(labels, dtype=torch.int32, device=dev())
    agg, cnt = ops.choose_aggregate(g, nodes_d, labels_d, s0, keys, [thr], rho, train, add_self=add_self, ws=ws)
    sets = ops.read_sets(g, len(nodes), ws)[0]
    begin = ws.view(0, torch.int64, len(nodes) + 1).cpu().numpy()
    length = ws.view(1, torch.int32, len(nodes)).cpu().numpy()
    lst = ws.view(2, torch.int32, max(int(begin[-1]), 1)).cpu().numpy()
    segs = [lst[begin[b]:begin[b] + length[b]] for b in range(len(nodes))]
    return sets, agg[0].cpu().numpy(), cnt[0].cpu().numpy(), length, segs


# ---------------------------------------------------------------------------------------------------------------------------
# selection: key families x {inference, training with every centre negative}
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def key_graph(P, world):
    X, csr, _ = world
    return P.DeviceGraph(X, [csr], S.minority_train_pos(64), dev())


_expected = {}       # (family, d, thr) -> (the oracle's set, its aggregated row): computed once, shared by both modes


def expected_rows(fam, tables, lengths, thr, Xt):
    out = []
    for d in lengths:
        key = (fam.name, d, thr)
        if key not in _expected:
            sc = torch.from_numpy(tables[d].view(np.float32).copy())
            want = O.choose_sets(torch.zeros(1), None, [range(d)], [sc], [], torch.zeros(0), thr, 0.5, False)
            _expected[key] = (want[0], O.sparse_aggregate(want, Xt).numpy()[0])
        out.append(_expected[key])
    return out


def score_table_of(keys):
    s0 = np.zeros(N, dtype=np.float32)            # (the centres: +0.0)
    s0[:S.POOL] = 1.0
    s0[:keys.size] = keys.view(np.float32)
    return s0


@pytest.mark.parametrize("train", [False, True], ids=["infer", "train"])
@pytest.mark.parametrize("name", [f.name for f in S.KEY_FAMILIES])
def test_selection_on_crafted_keys(P, world, key_graph, name, train):
    ops, g = P.ops, key_graph
    _, _, Xt = world
    fam = S.KEY_FAMILY[name]
    tables = S.family_tables(fam)
    # a prefix family: one table, every length in one batch; otherwise a table and a batch per length
    groups = [(tables[max(tables)], list(fam.lengths))] if fam.prefix else \
             [(tables[d], [d]) for d in fam.lengths]
    for table, lengths in groups:
        s0 = torch.from_numpy(score_table_of(table)).to(dev())
        keys = ops.pos_sort(g, s0) if train else None
        rev = lengths[::-1]
        # the same centres in reversed order, with duplicates: other waves / workgroups pull the rows
        for batch in (lengths, rev + rev[::3] + lengths[:2]):
            nodes = [KEY_CENTRE[d] for d in batch]
            labels = [0] * len(nodes) if train else None
            for thr in S.family_thresholds(fam, tables):
                want = expected_rows(fam, tables, batch, thr, Xt)
                sets, agg, cnt, length, segs = select(ops, g, nodes, labels, s0, keys, thr, 0.5, train)
                for b, d in enumerate(batch):
                    assert sets[b] == want[b][0], f"{name} d {d} thr {thr}: {len(sets[b] ^ want[b][0])} ids differ"
                    assert cnt[b] == len(sets[b]) == length[b], f"{name} d {d} thr {thr}"
                    assert (segs[b] >= 0).all()
                np.testing.assert_allclose(agg, np.stack([w[1] for w in want]), rtol=0, atol=AGG_TOL)


# ---------------------------------------------------------------------------------------------------------------------------
# the minority window: every family at every size of the sorted train-pos keys it makes sense for
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pos", S.MINORITY_P)
def test_minority_window_on_crafted_scores(P, world, n_pos):
    ops = P.ops
    X, csr, Xt = world
    tp = S.minority_train_pos(n_pos)
    g = P.DeviceGraph(X, [csr], tp, dev())
    cases = S.minority_cases(n_pos)
    self_family = "interior" if "interior" in cases else "all"
    for name, (scores, c, m) in cases.items():
        rng = np.random.default_rng([20, n_pos, len(name)])
        s0_h = S.minority_score_table(N, tp, scores, c, list(ROW_LEN), rng)
        s0 = torch.from_numpy(s0_h).to(dev())
        keys = ops.pos_sort(g, s0)
        s0_t = torch.from_numpy(s0_h)
        picks = [tp[i] for i in S.minority_picks(scores, c, m).tolist()]
        for d in S.MINORITY_ROWS:
            node, k = MIN_CENTRE[d], S.sample_count(d, 0.5)
            rho = (m + 0.5) / k                                   # int(k * rho) == m
            assert int(ops.minority_counts(g, np.array([node]), np.array([1]), [0.5], rho)[0, 0]) == min(m, n_pos)
            kept = O.choose_sets(s0_t[[node]], [0], [range(d)], [s0_t[:d]], tp, s0_t[tp], 0.5, rho, True)[0]
            want = O.choose_sets(s0_t[[node]], [1], [range(d)], [s0_t[:d]], tp, s0_t[tp], 0.5, rho, True)
            assert want[0] == kept | set(picks) and len(kept) == k
            n_dup = len(kept & set(picks))
            if name == "in_row":
                assert n_dup >= 2, "the case is about picks that are kept neighbours too"
            for add_self in ((False, True) if name == self_family else (False,)):
                sets, agg, cnt, length, segs = select(ops, g, [node], [1], s0, keys, 0.5, rho, True, add_self)
                full = want[0] | ({node} if add_self else set())
                tag = f"{name} P {n_pos} d {d} m {m} self {add_self}"
                assert sets[0] == full, f"{tag}: {sorted(sets[0] ^ full)[:8]}"
                assert cnt[0] == len(full), tag
                assert length[0] == k + min(m, n_pos) + int(add_self), tag            # kept + m slots (+ the centre)
                assert int((segs[0] < 0).sum()) == n_dup, tag                          # a -1 hole per duplicate pick
                ref = O.sparse_aggregate([full], Xt).numpy()
                np.testing.assert_allclose(agg, ref, rtol=0, atol=AGG_TOL, err_msg=tag)
