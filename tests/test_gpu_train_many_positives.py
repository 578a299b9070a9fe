"""Training steps of the engine with more than 16384 train positives, in both sort regimes, against the oracle.  Run with
``pytest -m gpu``.

Above 16384 keys the select launch no longer sorts: the first step's score launch is followed by pcg_pos_sort's four launches,
and every step's gather launch - which scores the table for the NEXT step and forms its raw keys - by the one-launch sort
(16385 .. 131072 keys) or by the four launches (above).  So steps 2 and 3 of a sequence select from keys a previous step's
launches sorted.  Two small graphs with exactly 16385 and 131073 train positives, three consecutive train_step calls each,
launched kernel by kernel and as one captured graph per step (epoch_step); after every step

  * the key buffer is exactly front_ref.sorted_keys of the score table the step left (what the next step selects from),
  * every centre's list, read back from the workspace, is O.choose_sets on the scores the select launch read,
  * the status word is 0 and theta is finite.

And one step whose follow-up sort overflows (tests/sort_ref.periodic through the label classifier): check() names the sort."""
import numpy as np
import pytest
import torch

from oracle import pcgnn_oracle as O
from tests import front_ref as F
from tests import presorted_ref as R
from tests import sort_ref as S

pytestmark = pytest.mark.gpu

FEAT, EMB, B, N_STEPS = 32, 64, 64, 3
POOL, N_CENTRES = 700, 48                                   # neighbours come from the first POOL nodes; centres of each label
DEGREES = [17, 60, 64, 65, 130, 500, 512, 513, 600]         # both sides of 64 (lane / wave rows) and of 512 (wave / workgroup rows)
THR, RHO = 0.5, 0.5
_WORLDS = {}


def dev():
    return torch.device("cuda", 0)


def world(n_pos, n_rel, periodic_column=False):
    """nodes: [0, 100) negatives | [100, 100 + n_pos) the train positives | 200 negatives.  The pool (the first POOL nodes) holds
    100 negatives and 600 positives; the centres are the last N_CENTRES positives and the first N_CENTRES negatives behind them,
    with a row in every relation; every other node is isolated.  Three batches of B centres, half of them positive."""
    key = (n_pos, n_rel, periodic_column)
    if key in _WORLDS:
        return _WORLDS[key]
    rs = np.random.RandomState(n_pos % 1000 + n_rel)
    n = 100 + n_pos + 200
    X = rs.randn(n, FEAT).astype(np.float32)
    labels = np.zeros(n, dtype=np.int64)
    labels[100:100 + n_pos] = 1
    train_pos = rs.permutation(np.arange(100, 100 + n_pos))                  # (not in id order: ties go by position)
    if periodic_column:
        X[train_pos, 0] = S.periodic(n_pos, S.one_launch_geometry(n_pos)[1])
    pos_c = np.arange(100 + n_pos - N_CENTRES, 100 + n_pos)
    neg_c = np.arange(100 + n_pos, 100 + n_pos + N_CENTRES)
    csr = []
    for r in range(n_rel):
        deg = np.zeros(n, dtype=np.int64)
        rows = {}
        for j, v in enumerate(np.concatenate([pos_c, neg_c])):
            d = DEGREES[(j + 2 * r) % len(DEGREES)]
            rows[int(v)] = np.sort(rs.choice(POOL, size=d, replace=False)).astype(np.int32)
            deg[v] = d
        indptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(deg, out=indptr[1:])
        csr.append((indptr, np.concatenate([rows[v] for v in sorted(rows)])))
    ids = np.concatenate([rs.permutation(np.concatenate([rs.choice(pos_c, B // 2, replace=False), rs.choice(neg_c, B // 2, replace=False)]))
                          for _ in range(N_STEPS)]).astype(np.int32)
    _WORLDS.clear()
    _WORLDS[key] = (X, labels, [int(v) for v in train_pos], csr, ids)
    return _WORLDS[key]


def engine(X, train_pos, csr, lr=0.01):
    import torch.nn as nn
    from pcgnn_amd.graph import DeviceGraph
    from pcgnn_amd.layers import InterAgg, IntraAgg
    from pcgnn_amd.model import PCALayer
    from pcgnn_amd.fused import FusedPCGNN
    torch.manual_seed(7)
    g = DeviceGraph(X, csr, train_pos, dev())
    feats = nn.Embedding(X.shape[0], FEAT)
    feats.weight = nn.Parameter(torch.from_numpy(X), requires_grad=False)
    intras = [IntraAgg(feats, FEAT, EMB, train_pos, RHO, cuda=True) for _ in csr]
    inter = InterAgg(feats, FEAT, EMB, train_pos, g, intras, cuda=True)
    model = PCALayer(2, inter, 2.0).to(dev())
    fz = FusedPCGNN(model, lr, 0.001, max_batch=B)
    assert fz.thresholds == [THR] * len(csr) and fz.rho == [RHO] * len(csr) and not fz.touched_on
    return fz


def assert_keys_sorted(fz, train_pos, what):
    """the sorted half of the key buffer against the score table beside it"""
    cap = S.half_capacity(fz.g.n_pos)
    got = fz.keys[:cap].cpu().numpy().view(np.uint64)
    want = F.sorted_keys(fz.s0.cpu().numpy(), train_pos, cap)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} key entries differ, first at {bad[0]}"


def assert_lists(fz, b, ids, labels, csr, train_pos, s0_read, what):
    """batch b's lists in the workspace against O.choose_sets on the scores its select launch read (the minority picks looked
    for among R.nearest_candidates: tests/test_presorted_window_host.py shows that this loses no pick)"""
    sets = fz.read_batch_lists(b)
    s0_t = torch.from_numpy(s0_read)
    tp = np.asarray(train_pos)
    pos_s0 = s0_t[torch.from_numpy(tp)]
    pos_np = pos_s0.numpy()
    cnt = fz.last_counts.cpu().numpy()
    seen_m = set()
    for r, (indptr, idx) in enumerate(csr):
        for i, v in enumerate(ids):
            row = idx[indptr[v]:indptr[v + 1]].tolist()
            k = R.sample_count(len(row), THR)
            m = int(k * RHO)
            cand_ids, cand_s = train_pos, pos_s0
            if labels[i] == 1 and 0 < m < tp.size:
                cand = R.nearest_candidates(s0_read[v], pos_np, m)
                cand_ids, cand_s = tp[cand].tolist(), pos_s0[torch.from_numpy(cand)]
                seen_m.add(len(row))
            want = O.choose_sets(s0_t[v:v + 1], [int(labels[i])], [row], [s0_t[torch.as_tensor(row, dtype=torch.long)]],
                                 cand_ids, cand_s, THR, RHO, True)[0]
            assert sets[r][i] == want, f"{what}: relation {r} centre {i} (node {v}, degree {len(row)}, label {labels[i]})"
            assert cnt[r][i] == len(want), what
    assert min(seen_m) <= 64 and any(64 < d <= 512 for d in seen_m) and max(seen_m) > 512, (what, "positive rows of three tiers")


@pytest.mark.parametrize("mode", ["eager", "graph"])
@pytest.mark.parametrize("n_pos,n_rel", [(16385, 2), (131073, 1)])
def test_three_steps_select_from_keys_the_previous_step_sorted(n_pos, n_rel, mode):
    from pcgnn_amd import _lib
    X, labels, train_pos, csr, ids = world(n_pos, n_rel)
    fz = engine(X, train_pos, csr)
    g = fz.g
    assert g.n_pos == n_pos and bool(_lib.load().pcg_pos_sort_one_launch(n_pos)) == (n_pos <= S.BK1_MAX)
    assert fz.keys.numel() == S.capacity(n_pos)
    ids_d = torch.from_numpy(ids).to(dev())
    lab_d = torch.from_numpy(labels[ids].astype(np.int32)).to(dev())
    fz.begin_epoch(ids_d, lab_d, B)
    assert len(fz._ep_batches) == N_STEPS
    fz._enqueue_refresh()                                    # the scores of the current classifier, their keys by pcg_pos_sort
    if mode == "graph":
        # one graph per step, captured at its first use (a capture leaves the scores stale: those steps refresh first); the
        # steps that are checked are the replays of the second round
        for b in range(N_STEPS):
            fz.epoch_step(b)
        torch.cuda.synchronize()
        fz.check()
        assert fz._fresh
    theta0 = fz.theta.clone()
    for b in range(N_STEPS):
        what = f"{n_pos} positives, {mode}, step {b + 1}"
        assert fz._fresh, what                               # (no score launch of its own: steps 2 and 3 use the previous step's keys)
        torch.cuda.synchronize()
        s0_read = fz.s0.cpu().numpy().copy()
        assert_keys_sorted(fz, train_pos, what + ", before")
        if mode == "eager":                                  # train_step on the staged batch's plan slot (where its lists are read back)
            fz.train_step(ids_d[b * B:(b + 1) * B], lab_d[b * B:(b + 1) * B], plan=fz._ep_plan(b))
        else:                                                # the same call as one captured graph
            fz.epoch_step(b)
        torch.cuda.synchronize()
        batch = ids[b * B:(b + 1) * B]
        assert_lists(fz, b, batch.astype(np.int64), labels[batch], csr, train_pos, s0_read, what)
        assert_keys_sorted(fz, train_pos, what)
        assert not np.array_equal(fz.s0.cpu().numpy(), s0_read), what        # (the step scored the table for the next one)
        assert int(fz.status.item()) == 0, what
        fz.check()
        assert bool(torch.isfinite(fz.theta).all()), what
    fz.flush()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(fz.theta).all()) and not torch.equal(theta0, fz.theta)


def test_an_overflowing_sort_is_reported_by_check():
    """the label classifier set to score = column 0 + bias, column 0 of the train positives laid out as sort_ref.periodic: the
    one-launch sort behind the step's gather launch meets a bucket of ~16 K keys; check() names it, once"""
    from pcgnn_amd import _lib
    n_pos = 16385
    X, labels, train_pos, csr, ids = world(n_pos, 1, periodic_column=True)
    fz = engine(X, train_pos, csr, lr=1e-4)                  # (a small step: the next classifier still separates the two scores)
    clf = torch.zeros(2 * FEAT + 2, device=dev())
    clf[0] = 1.0
    fz.theta[fz.n_rest:].copy_(clf)
    fz.params_changed()
    batch = torch.from_numpy(ids[:B]).to(dev())
    fz.train_step(batch, torch.from_numpy(labels[ids[:B]].astype(np.int32)).to(dev()))
    torch.cuda.synchronize()
    assert int(fz.status.item()) == S.ST_SORT_OVERFLOW
    with pytest.raises(_lib.PcgnnLibraryError, match="one-launch sort of the train positives"):
        fz.check()
    fz.check()                                               # the word was cleared
