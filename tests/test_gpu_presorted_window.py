"""Positive centres' minority window in launches whose train-pos keys were sorted by an EARLIER launch (select.hip, the presorted
instantiation): the search index built at the workgroup's entry, the window search staged beside a single-wave row's own loads,
the workgroup rows' early window - with many positive rows per launch, at the sizes of tests/presorted_ref.py
(tests/test_presorted_window_host.py shows on the CPU which boundaries they reach).  Run with ``pytest -m gpu``.

Part 1 (select_rows, eight waves): ops.pos_sort + ops.choose_aggregate(train=True) against O.choose_sets on the same float32
scores - exact.  Bars: sets, counts, list lengths and -1 holes exact; aggregated rows within 5e-5 (the bar of that path in
tests/test_gpu_select_keys.py).  The same at the bucket-sorted sizes, 16384 .. 262145 keys (index strides of 32 .. 1024): the
crafted centre positions, both sides of the staging switch, brackets of three probe rounds, whole-buffer windows, and runs of 100
equal scores across the window's edge.
Part 2 (the fused launch, sixteen waves): sequences of 3 and 4 steps with the classifier two batches ahead against the same steps
as three launches: bit for bit."""
import numpy as np
import pytest
import torch

from oracle import pcgnn_oracle as O
from tests import presorted_ref as R

pytestmark = pytest.mark.gpu

N, FEAT, POOL = 20000, 32, 600
POS_BASE, CENTRE_BASE = 1000, 10000
AGG_TOL = 5e-5
POSITIONS = list(R.centre_scores(64))                         # eight centre positions
KINDS = POSITIONS + ["neg0", "neg1"]                          # per degree: eight positive centres, two negative ones
CENTRES = [(d, kind) for d in R.DEGREES for kind in KINDS]    # centre i is node CENTRE_BASE + i


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def P():
    import pcgnn_amd
    from pcgnn_amd import ops  # noqa: F401  (fails loudly if the .so is missing)
    return pcgnn_amd


@pytest.fixture(scope="module")
def world():
    """X and the one relation: the row of a centre of degree d is the first d nodes of the pool 0 .. POOL - 1"""
    X = np.random.RandomState(22).randn(N, FEAT).astype(np.float32)
    deg = np.zeros(N, dtype=np.int64)
    for i, (d, _) in enumerate(CENTRES):
        deg[CENTRE_BASE + i] = d
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = np.concatenate([np.arange(d, dtype=np.int32) for d, _ in CENTRES])
    return X, (indptr, indices), torch.from_numpy(X)


def train_pos_of(n_pos):
    """a few of the training positives are pool nodes (kept neighbours that are picked too leave -1 holes), the others nobody's"""
    head = [0, 2, 4, 6][:min(4, n_pos // 3)]
    return head + list(range(POS_BASE, POS_BASE + n_pos - len(head)))


def score_table(n_pos, tp):
    rng = np.random.default_rng([22, n_pos])
    keys = R.key_scores(n_pos)
    s0 = np.zeros(N, dtype=np.float32)
    s0[:POOL] = rng.uniform(0.0, float(keys[-1]) + 1.0, size=POOL).astype(np.float32)
    s0[np.asarray(tp)] = keys[rng.permutation(n_pos)]          # (train_pos order is not score order: ties go by position)
    cs = R.centre_scores(n_pos)
    for i, (d, kind) in enumerate(CENTRES):
        s0[CENTRE_BASE + i] = cs[kind] if kind in cs else cs[POSITIONS[(i + d) % len(POSITIONS)]]
    return s0


def select(ops, g, nodes, labels, s0, keys, rho):
    nodes_h, labels_h = np.asarray(nodes, dtype=np.int64), np.asarray(labels, dtype=np.int64)
    cap = int(ops.sel_capacity(g, nodes_h, labels_h, [R.THR], rho, True, False).sum()) + sum(CENTRES[v - CENTRE_BASE][0] for v in nodes)
    ws = ops.ChooseWorkspace(g, len(nodes), list_capacity=cap)
    nodes_d = torch.tensor(nodes, dtype=torch.int32, device=dev())
    labels_d = torch.tensor(labels, dtype=torch.int32, device=dev())
    agg, cnt = ops.choose_aggregate(g, nodes_d, labels_d, s0, keys, [R.THR], rho, True, add_self=False, ws=ws)
    sets = ops.read_sets(g, len(nodes), ws)[0]
    begin = ws.view(0, torch.int64, len(nodes) + 1).cpu().numpy()
    length = ws.view(1, torch.int32, len(nodes)).cpu().numpy()
    lst = ws.view(2, torch.int32, max(int(begin[-1]), 1)).cpu().numpy()
    segs = [lst[begin[b]:begin[b] + length[b]] for b in range(len(nodes))]
    return sets, agg[0].cpu().numpy(), cnt[0].cpu().numpy(), length, segs


@pytest.mark.parametrize("n_pos", R.SIZES + [R.PLAIN_SIZE])
def test_many_positive_rows_per_launch(P, world, n_pos):
    ops = P.ops
    X, csr, Xt = world
    tp = train_pos_of(n_pos)
    g = P.DeviceGraph(X, [csr], tp, dev())
    s0_h = score_table(n_pos, tp)
    s0_t = torch.from_numpy(s0_h)
    s0 = s0_t.to(dev())
    keys = ops.pos_sort(g, s0)
    pos_s0 = s0_t[tp]
    order = list(range(len(CENTRES)))
    rev = order[::-1]
    label_of = [0 if kind.startswith("neg") else 1 for _, kind in CENTRES]
    for m_star, d_star, rho in R.gpu_cases(n_pos):
        # the oracle, once per centre
        want = O.choose_sets(s0_t[CENTRE_BASE:CENTRE_BASE + len(CENTRES)], label_of, [range(d) for d, _ in CENTRES],
                             [s0_t[:d] for d, _ in CENTRES], tp, pos_s0, R.THR, rho, True)
        kept = O.choose_sets(s0_t[CENTRE_BASE:CENTRE_BASE + len(CENTRES)], [0] * len(CENTRES), [range(d) for d, _ in CENTRES],
                             [s0_t[:d] for d, _ in CENTRES], tp, pos_s0, R.THR, rho, True)
        ref = O.sparse_aggregate(want, Xt).numpy()
        # the same centres in two row orders (the second with repeats): other waves / workgroups pull the rows, and one
        # workgroup's waves are on positive rows with different centre scores at the same time
        for batch in (order, rev + rev[::3] + order[:2]):
            nodes = [CENTRE_BASE + i for i in batch]
            labels = [label_of[i] for i in batch]
            sets, agg, cnt, length, segs = select(ops, g, nodes, labels, s0, keys, rho)
            for b, i in enumerate(batch):
                d, kind = CENTRES[i]
                k = R.sample_count(d)
                m = R.row_m(d, rho, n_pos) if label_of[i] else 0
                tag = f"P {n_pos} m* {m_star} at d {d_star}: centre d {d} {kind} m {m}"
                assert len(kept[i]) == k and kept[i] <= want[i] and len(want[i]) <= k + m, tag
                assert sets[b] == want[i], f"{tag}: {sorted(sets[b] ^ want[i])[:8]}"
                assert cnt[b] == len(want[i]), tag
                assert length[b] == k + m, tag                                            # kept + m slots
                assert int((segs[b] < 0).sum()) == k + m - len(want[i]), tag              # a -1 hole per pick that is kept too
            np.testing.assert_allclose(agg, ref[batch], rtol=0, atol=AGG_TOL, err_msg=f"P {n_pos} m* {m_star} at d {d_star}")


# ---------------------------------------------------------------------------------------------------------------------------
# Part 1 at the bucket-sorted sizes (16384 .. 262145 keys: index strides of 32 .. 1024) and with long runs of equal scores
# ---------------------------------------------------------------------------------------------------------------------------
N_L = POS_BASE + max(R.LARGE_SIZES) + 200
CENTRE_BASE_L = POS_BASE + max(R.LARGE_SIZES) + 50            # (behind the last training positive of the largest size)


@pytest.fixture(scope="module")
def large_world():
    """the construction of `world` with room for 262145 training positives"""
    X = np.random.RandomState(23).randn(N_L, FEAT).astype(np.float32)
    deg = np.zeros(N_L, dtype=np.int64)
    for i, (d, _) in enumerate(CENTRES):
        deg[CENTRE_BASE_L + i] = d
    indptr = np.zeros(N_L + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = np.concatenate([np.arange(d, dtype=np.int32) for d, _ in CENTRES])
    return X, (indptr, indices), torch.from_numpy(X)


def large_score_table(n_pos, tp, keys, centre_of_kind, seed):
    """score_table's construction: `keys` are the sorted scores of the positives, shuffled over train_pos; centre i of kind
    POSITIONS[j] gets centre_of_kind[j]"""
    rng = np.random.default_rng([seed, n_pos])
    s0 = np.zeros(N_L, dtype=np.float32)
    s0[:POOL] = rng.uniform(0.0, float(keys[-1]) + 1.0, size=POOL).astype(np.float32)
    s0[np.asarray(tp)] = keys[rng.permutation(n_pos)]
    for i, (d, kind) in enumerate(CENTRES):
        j = POSITIONS.index(kind) if kind in POSITIONS else (i + d) % len(POSITIONS)
        s0[CENTRE_BASE_L + i] = centre_of_kind[j]
    return s0


def oracle_large(centres, labels, s0_t, tp, pos_s0, rho):
    """O.choose_sets, one centre at a time; a positive centre's minority picks are looked for among R.nearest_candidates (every
    positive at most the m-th distance away, in train_pos order) instead of among all P"""
    pos_np, tp_np = pos_s0.numpy(), np.asarray(tp)
    out = []
    for i, lab in zip(centres, labels):
        d = CENTRES[i][0]
        c = s0_t[CENTRE_BASE_L + i:CENTRE_BASE_L + i + 1]
        m = int(R.sample_count(d) * rho)
        ids, sc = tp, pos_s0
        if lab and 0 < m < len(tp):
            cand = R.nearest_candidates(c.numpy()[0], pos_np, m)
            ids, sc = tp_np[cand].tolist(), pos_s0[torch.from_numpy(cand)]
        out.append(O.choose_sets(c, [lab], [range(d)], [s0_t[:d]], ids, sc, R.THR, rho, True)[0])
    return out


def select_large(ops, g, nodes, labels, s0, keys, rho):
    nodes_h, labels_h = np.asarray(nodes, dtype=np.int64), np.asarray(labels, dtype=np.int64)
    cap = int(ops.sel_capacity(g, nodes_h, labels_h, [R.THR], rho, True, False).sum()) + sum(CENTRES[v - CENTRE_BASE_L][0] for v in nodes)
    ws = ops.ChooseWorkspace(g, len(nodes), list_capacity=cap)
    nodes_d = torch.tensor(nodes, dtype=torch.int32, device=dev())
    labels_d = torch.tensor(labels, dtype=torch.int32, device=dev())
    agg, cnt = ops.choose_aggregate(g, nodes_d, labels_d, s0, keys, [R.THR], rho, True, add_self=False, ws=ws)
    sets = ops.read_sets(g, len(nodes), ws)[0]
    begin = ws.view(0, torch.int64, len(nodes) + 1).cpu().numpy()
    length = ws.view(1, torch.int32, len(nodes)).cpu().numpy()
    lst = ws.view(2, torch.int32, max(int(begin[-1]), 1)).cpu().numpy()
    segs = [lst[begin[b]:begin[b] + length[b]] for b in range(len(nodes))]
    ws.check()
    return sets, agg[0].cpu().numpy(), cnt[0].cpu().numpy(), length, segs


def run_large(P, large_world, n_pos, key_scores, centre_of_kind, cases, seed):
    ops = P.ops
    X, csr, Xt = large_world
    tp = train_pos_of(n_pos)
    g = P.DeviceGraph(X, [csr], tp, dev())
    s0_h = large_score_table(n_pos, tp, key_scores, centre_of_kind, seed)
    s0_t = torch.from_numpy(s0_h)
    s0 = s0_t.to(dev())
    keys = ops.pos_sort(g, s0)
    pos_s0 = s0_t[tp]
    label_of = [0 if kind.startswith("neg") else 1 for _, kind in CENTRES]
    for m_star, d_star, rho, degrees in cases:
        sel = [i for i, (d, _) in enumerate(CENTRES) if degrees is None or d in degrees]
        want = oracle_large(sel, [label_of[i] for i in sel], s0_t, tp, pos_s0, rho)
        kept = oracle_large(sel, [0] * len(sel), s0_t, tp, pos_s0, rho)
        ref = O.sparse_aggregate(want, Xt).numpy()
        order = list(range(len(sel)))
        rev = order[::-1]
        for batch in (order, rev + rev[::3] + order[:2]):      # (the two row orders of test_many_positive_rows_per_launch)
            nodes = [CENTRE_BASE_L + sel[j] for j in batch]
            labels = [label_of[sel[j]] for j in batch]
            sets, agg, cnt, length, segs = select_large(ops, g, nodes, labels, s0, keys, rho)
            for b, j in enumerate(batch):
                d, kind = CENTRES[sel[j]]
                k = R.sample_count(d)
                m = R.row_m(d, rho, n_pos) if labels[b] else 0
                tag = f"P {n_pos} m* {m_star} at d {d_star}: centre d {d} {kind} m {m}"
                assert len(kept[j]) == k and kept[j] <= want[j] and len(want[j]) <= k + m, tag
                assert sets[b] == want[j], f"{tag}: {sorted(sets[b] ^ want[j])[:8]}"
                assert cnt[b] == len(want[j]), tag
                assert length[b] == k + m, tag                                            # kept + m slots
                assert int((segs[b] < 0).sum()) == k + m - len(want[j]), tag              # a -1 hole per pick that is kept too
            np.testing.assert_allclose(agg, ref[batch], rtol=0, atol=AGG_TOL, err_msg=f"P {n_pos} m* {m_star} at d {d_star}")


@pytest.mark.parametrize("n_pos", R.LARGE_SIZES)
def test_many_positive_rows_per_launch_large(P, large_world, n_pos):
    """the crafted centre positions, both sides of the staging switch stride - 1 + m <= 4096 and a bracket of three probe rounds
    at every index stride from 32 to 1024 (tests/test_presorted_window_host.py: which boundaries each size reaches)"""
    cs = R.centre_scores(n_pos)
    run_large(P, large_world, n_pos, R.key_scores(n_pos), [cs[kind] for kind in POSITIONS], R.large_cases(n_pos), 24)


@pytest.mark.parametrize("n_pos,run", [(n, "runs") for n in R.TIE_SIZES] + [(R.TIE_SIZES[0], "all_equal")])
def test_ties_across_the_window_edge_large(P, large_world, n_pos, run):
    """runs of 100 equal scores under strides of 64 and 512 (and, at the smaller size - the oracle sorts every key there - one
    run of all the keys): the m-th distance falls inside a run left of the centre, right of it, or inside one on either side; of
    more than 64 ties the earliest in train_pos are taken"""
    length = R.TIE_RUN if run == "runs" else n_pos
    cs = R.tie_centre_scores(n_pos, length)
    run_large(P, large_world, n_pos, R.tie_key_scores(n_pos, length), [cs[kind] for kind in R.TIE_KINDS], R.tie_cases(n_pos), 25)


# ---------------------------------------------------------------------------------------------------------------------------
# Part 2: the fused launch's select half (sixteen waves), keys sorted a launch earlier
# ---------------------------------------------------------------------------------------------------------------------------
NAMES = ("theta", "m", "v", "step_counter", "clf_next", "row_loss")
_WORK = {}


def workload(n_pos):
    """20000 nodes, three relations; exactly n_pos training positives, six of them hubs of the last relation (workgroup rows)
    and six hubs of the second (wave rows); every batch has hub, mid and ordinary positive centres and negative ones"""
    if n_pos in _WORK:
        return _WORK[n_pos]
    from pcgnn_amd import synth
    w = synth.make_workload("mini", 20000, 32, (12000, 90000, 270000), 0.12, seed=3, train_ratio=0.6)
    rs = np.random.RandomState(11)
    base_pos = np.asarray(w.train_pos)
    hubs = rs.choice(base_pos, size=6, replace=False)
    mids = rs.choice(np.setdiff1d(base_pos, hubs), size=6, replace=False)
    for rel, who, extra in ((2, hubs, 600), (1, mids, 150)):
        indptr, idx = w.csr[rel]
        src = np.repeat(np.arange(w.n, dtype=np.int64), np.diff(indptr))
        hs = np.repeat(who.astype(np.int64), extra)
        hd = np.concatenate([rs.choice(w.n, size=extra, replace=False) for _ in who]).astype(np.int64)
        w.csr[rel] = synth._csr_from_pairs(w.n, np.concatenate([src, hs]), np.concatenate([idx.astype(np.int64), hd]))
    w.homo_deg = synth._homo_degree(w.n, w.csr)
    # exactly n_pos training positives: the hubs, the mids, other positives, then (relabelled) other training nodes
    rest_pos = np.setdiff1d(base_pos, np.concatenate([hubs, mids]))
    others = np.setdiff1d(w.idx_train, base_pos)
    chosen = np.concatenate([hubs, mids, rest_pos, others])[:n_pos]
    assert chosen.size == n_pos
    w.labels = w.labels.copy()
    w.labels[chosen] = 1
    w.train_pos = sorted(int(v) for v in chosen)
    B = 128 if n_pos <= 1024 else 640                        # (the sort riders of 8193 keys need the tiles of a larger batch)
    ordinary = chosen[12:] if n_pos > 12 else chosen
    ids = []
    for _ in range(4):
        part = np.concatenate([rs.choice(hubs, size=3, replace=False), rs.choice(mids, size=3, replace=False),
                               rs.choice(ordinary, size=30), rs.choice(w.idx_train, size=B - 36)])
        ids.append(rs.permutation(part))
    ids = np.concatenate(ids).astype(np.int32)
    degs = [np.diff(ip) for ip, _ in w.csr]
    for b in range(4):
        pos_ids = [i for i in ids[b * B:(b + 1) * B] if w.labels[i] == 1]
        dd = np.concatenate([dg[pos_ids] for dg in degs])
        assert (dd > 512).any() and ((dd > 64) & (dd <= 512)).any() and ((dd > 16) & (dd <= 64)).any(), "three tiers"
    _WORK[n_pos] = (w, ids, B)
    return _WORK[n_pos]


def _engine(w, B, pipeline, ahead):
    import torch.nn as nn
    from pcgnn_amd.graph import DeviceGraph
    from pcgnn_amd.layers import InterAgg, IntraAgg
    from pcgnn_amd.model import PCALayer
    from pcgnn_amd.fused import FusedPCGNN
    torch.manual_seed(5)
    g = DeviceGraph(w.X, w.csr, w.train_pos, dev())
    f = w.X.shape[1]
    feats = nn.Embedding(w.n, f)
    feats.weight = nn.Parameter(torch.from_numpy(w.X), requires_grad=False)
    intras = [IntraAgg(feats, f, 64, w.train_pos, 0.5, cuda=True) for _ in w.csr]
    inter = InterAgg(feats, f, 64, w.train_pos, g, intras, cuda=True)
    model = PCALayer(2, inter, 2.0).to(dev())
    return FusedPCGNN(model, 0.01, 0.001, max_batch=B, pipeline=pipeline, clf_ahead=ahead)


def _run_pair(n_pos, n_steps, expect_ahead):
    w, ids, B = workload(n_pos)
    a, b = _engine(w, B, True, True), _engine(w, B, False, False)
    assert a.g.n_pos == n_pos
    b.theta.copy_(a.theta)
    b.params_changed()
    ids_d = torch.from_numpy(ids).to(dev())
    lab_d = torch.from_numpy(w.labels[ids].astype(np.int32)).to(dev())
    for fz in (a, b):
        fz.begin_epoch(ids_d, lab_d, B)
    steps = [(None, None, Bb, 0) for _, Bb in a._ep_batches][:n_steps]
    assert a._pipelines([(0, s[2]) for s in steps]) and not b._pipelines([(0, s[2]) for s in steps])
    assert a._ahead(steps) == expect_ahead, "the schedule this case is about"
    for fz in (a, b):
        fz.epoch_run(n_steps=n_steps, flush=False)
    torch.cuda.synchronize()
    for fz in (a, b):
        fz.check()                                           # (no overflow, no time-out)
    what = f"P {n_pos}, {n_steps} steps"
    for name in NAMES:
        assert torch.equal(getattr(a, name), getattr(b, name)), f"{name} ({what}, update pending)"
    assert torch.equal(a.last_counts, b.last_counts), f"last counts ({what})"
    assert int(a.step_counter[0]) == n_steps
    for fz in (a, b):
        fz.flush()
    torch.cuda.synchronize()
    for name in NAMES:
        assert torch.equal(getattr(a, name), getattr(b, name)), f"{name} ({what}, flushed)"


@pytest.mark.parametrize("n_steps", [3, 4])
@pytest.mark.parametrize("n_pos", [16, 17, 1024, 8192, 8193])
def test_fused_presorted_equals_three_launches(n_pos, n_steps):
    _run_pair(n_pos, n_steps, True)


def test_fused_in_launch_sort_equals_three_launches(monkeypatch):
    """presort off: the fused launch sorts its keys itself - the in-launch-sort instantiation, which behaves as before"""
    monkeypatch.setenv("PCG_PRESORT", "0")
    _run_pair(1024, 4, False)
