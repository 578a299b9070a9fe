"""Nearest labelled examples (pcg_topk_similar through ops.topk_similar, FusedPCGNN.nearest, utils.similar_examples) on the GPU.

Exact cases: small-integer-valued float32 inputs, so every dot product, squared norm and squared distance is exact in float32
whatever the summation order - positions AND scores must equal tests/nearest_ref.py (numpy float64), for every size at which
the kernel takes another path (a partial candidate tile, fewer candidates than k, several query tiles, two waves per workgroup
at E = 512 would be the same code) and for several bank-slice counts.

Real embeddings: the returned scores against float64 scores of the device's own embeddings, within the worst-case bound of an
E-term float32 dot product, u = 2^-24:  dot  u (E + 8) sum_i |q_i c_i|;  l2  the same over all terms of 2 q.c - |q|^2 - |c|^2;
cosine  u (2 E + 16) (|score| <= 1; two normalisations).  No candidate left out may beat the returned k-th by more than twice
the bound."""
import numpy as np
import pytest
import torch

from tests import nearest_ref as NR
from tests.util import GoldenCase

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
_ENGINES = {}


def dev():
    return torch.device("cuda", 0)


def to_dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev())


def run(Q, bank, k, metric, q_ids=None, bank_ids=None, slices=0):
    from pcgnn_amd import ops
    pos, score = ops.topk_similar(to_dev(Q), to_dev(bank), k, metric, None if q_ids is None else to_dev(q_ids, torch.int32),
                                  None if bank_ids is None else to_dev(bank_ids, torch.int32), _slices=slices)
    assert pos.dtype == torch.int32 and score.dtype == torch.float32 and pos.shape == score.shape == (len(Q), k)
    return pos.cpu().numpy(), score.cpu().numpy()


def assert_exact(Q, bank, k, metric, q_ids=None, bank_ids=None, slices=0, what=""):
    want_pos, want_score = NR.topk_similar_ref(Q, bank, k, metric, q_ids, bank_ids)
    pos, score = run(Q, bank, k, metric, q_ids, bank_ids, slices)
    assert np.array_equal(pos, want_pos), f"{what}: positions differ"
    assert np.array_equal(score.astype(np.float64), want_score), f"{what}: scores differ"
    return pos, score


def ints(rs, n, E, lo=-3, hi=4):
    return rs.randint(lo, hi, size=(n, E)).astype(np.float32)


# ---- exact cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["dot", "l2"])
@pytest.mark.parametrize("M", [0, 1, 15, 16, 17, 1000])
def test_exact_sizes(M, metric):
    rs = np.random.RandomState(M + 1)
    for n, E in ((1, 16), (16, 64), (17, 128), (100, 64)):
        Q, bank = ints(rs, n, E), ints(rs, M, E)
        for k in (1, 5, 64):
            assert_exact(Q, bank, k, metric, what=f"n {n} E {E} M {M} k {k}")
    # every id excluded somewhere
    Q, bank = ints(rs, 17, 64), ints(rs, M, 64)
    q_ids, bank_ids = rs.randint(0, 8, size=17), rs.randint(0, 8, size=M)
    assert_exact(Q, bank, 5, metric, q_ids, bank_ids, what=f"M {M} with exclusions")


@pytest.mark.parametrize("E,k", [(256, 5), (512, 5), (512, 62), (512, 63), (512, 64)])
def test_exact_wide_rows(E, k):
    """the widest rows: more than 64 KiB of LDS per workgroup, and at E = 512, k >= 63 four Q tiles and their lists no longer
    fit in 160 KiB - the launch has two waves per workgroup instead of four (k = 62 is the last size with four)"""
    rs = np.random.RandomState(E + k)
    Q, bank = ints(rs, 100, E), ints(rs, 300, E)
    for metric in ("dot", "l2"):
        for s in (0, 3):
            assert_exact(Q, bank, k, metric, slices=s, what=f"E {E} k {k} {metric} slices {s}")


@pytest.mark.parametrize("metric", ["dot", "l2", "cosine"])
def test_slice_count_does_not_matter(metric):
    """the same inputs with the bank in 1, 2, 3, 7 and 64 slices and the kernel's own choice: the same bits"""
    rs = np.random.RandomState(3)
    for n, M, E, k in ((16, 1000, 64, 5), (100, 1000, 16, 64), (17, 4099, 128, 8)):
        Q, bank = ints(rs, n, E, -2, 3), ints(rs, M, E, -2, 3)          # (few distinct scores: ties across slices)
        q_ids, bank_ids = rs.randint(0, 50, size=n), rs.randint(0, 50, size=M)
        base = run(Q, bank, k, metric, q_ids, bank_ids, slices=1)
        if metric != "cosine":
            assert_exact(Q, bank, k, metric, q_ids, bank_ids, slices=1, what=f"{metric} one slice")
        for s in (0, 2, 3, 7, 64):
            pos, score = run(Q, bank, k, metric, q_ids, bank_ids, slices=s)
            assert np.array_equal(pos, base[0]) and np.array_equal(score, base[1]), f"{metric} n {n} M {M}: {s} slices"


def test_crafted_orders():
    rs = np.random.RandomState(9)
    E = 16
    # all scores equal: order by position, in one slice and in many
    Q, bank = np.ones((5, E), np.float32), np.ones((200, E), np.float32)
    for metric in ("dot", "l2", "cosine"):
        for s in (1, 5):
            pos, score = run(Q, bank, 64, metric, slices=s)
            assert np.array_equal(pos, np.tile(np.arange(64, dtype=np.int32), (5, 1))), metric
            assert (score == {"dot": 16.0, "l2": 0.0, "cosine": 1.0}[metric]).all()
    # blocks of duplicated bank rows straddling a 16-candidate tile edge (rows 10 .. 21 and 30 .. 33), the best for row 0
    Q, bank = ints(rs, 3, E), ints(rs, 64, E)
    bank[10:22] = 3 * np.sign(Q[0]) + (Q[0] == 0)
    bank[30:34] = bank[10]
    pos, _ = assert_exact(Q, bank, 20, "dot", what="duplicates")
    assert pos[0, :16].tolist() == list(range(10, 22)) + [30, 31, 32, 33]
    # the true top-k all in the last (partial) tile
    Q, bank = ints(rs, 20, E), ints(rs, 1000, E)
    bank[995:] = 3 * np.sign(Q[7]) + (Q[7] == 0)
    for s in (0, 1, 4):
        pos, _ = assert_exact(Q, bank, 5, "dot", slices=s, what="last tile")
        assert pos[7].tolist() == [995, 996, 997, 998, 999]
    # exclude_self removes the best candidate (the row itself), and only it
    bank = ints(rs, 40, E)
    bank[:, 0] = np.arange(40) + 5                                       # distinct rows, each its own nearest under l2
    sel = np.array([33, 0, 15, 16, 39])
    ids = 1000 + np.arange(40)
    free, _ = assert_exact(bank[sel], bank, 3, "l2", what="no exclusion")
    assert free[:, 0].tolist() == sel.tolist()
    pos, _ = assert_exact(bank[sel], bank, 3, "l2", ids[sel], ids, what="exclude self")
    assert not (pos == sel[:, None]).any() and (pos >= 0).all()
    # exclude_self leaving fewer than k candidates: padding is -1 / -inf
    bank_ids = np.full(40, 7)
    bank_ids[[3, 38]] = (8, 9)
    pos, score = assert_exact(bank[sel], bank, 5, "dot", np.full(5, 7), bank_ids, what="padding")
    assert (np.sort(pos[:, :2], axis=1) == [3, 38]).all() and (pos[:, 2:] == -1).all() and np.isneginf(score[:, 2:]).all()
    pos, score = run(bank[sel], bank, 5, "cosine", np.full(5, 7), np.full(40, 7))
    assert (pos == -1).all() and np.isneginf(score).all()


# ---- real embeddings ---------------------------------------------------------------------------------------------------------
def engine_of(name):
    from tests.test_gpu_infer_new import engine
    if name not in _ENGINES:
        c = GoldenCase(name)
        _ENGINES[name] = (c, engine(c.X, c.csr, c.train_pos, c.emb, [0.5] * c.R, c.params(), c.alpha))
    return _ENGINES[name]


def bound_of(Q, bank, metric):
    """[n, M] float64: the worst-case float32 error of every pair's score (module docstring)"""
    E = Q.shape[1]
    A = np.abs(Q) @ np.abs(bank).T
    if metric == "dot":
        return U * (E + 8) * A
    if metric == "l2":
        return U * (E + 8) * (2 * A + (Q * Q).sum(1)[:, None] + (bank * bank).sum(1)[None, :])
    return np.full(A.shape, U * (2 * E + 16))


def check_rows(near_pos, near_score, Q, bank, metric, ok, k):
    s64, bnd = NR.scores(Q, bank, metric), bound_of(Q, bank, metric)
    n, M = s64.shape
    worst = 0.0
    for i in range(n):
        p, s = near_pos[i], near_score[i].astype(np.float64)
        n_ok = int(ok[i].sum())
        assert (p[:min(k, n_ok)] >= 0).all() and (p[min(k, n_ok):] == -1).all()
        p = p[p >= 0]
        assert len(set(p.tolist())) == len(p) and ok[i, p].all()
        err = np.abs(s[:len(p)] - s64[i, p])
        worst = max(worst, float((err / np.maximum(bnd[i, p], 1e-300)).max()) if len(p) else 0.0)
        assert (err <= bnd[i, p]).all(), f"row {i}: score error {err.max():.3e} above the bound"
        for j in range(len(p) - 1):                                     # sorted, ties by position
            assert s[j] > s[j + 1] or (s[j] == s[j + 1] and p[j] < p[j + 1])
        if len(p) == k:
            out = ok[i].copy()
            out[p] = False
            kth = s64[i, p[-1]]
            slack = 2 * np.maximum(bnd[i], bnd[i, p[-1]])
            assert (s64[i, out] <= kth + slack[out]).all(), f"row {i}: a better candidate was left out"
    return worst


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
@pytest.mark.parametrize("name", ["yelp_small", "yelp_emb128"])
def test_real_embeddings(name, metric):
    c, fz = engine_of(name)
    rs = np.random.RandomState(4)
    ids = np.concatenate([rs.choice(c.n, size=90, replace=False), np.asarray(c.train_pos[:10])])     # some are in the bank
    near = fz.nearest(ids, k=8, metric=metric)
    among = np.asarray(c.train_pos, dtype=np.int64)
    assert near.metric == metric and near.k == 8 and near.n == len(ids)
    assert np.array_equal(near.among.cpu().numpy(), among)
    e_ids, e_pos, e_score = near.to_numpy()
    assert e_ids.dtype == np.int32 and e_pos.dtype == np.int32 and e_score.dtype == np.float32
    assert np.array_equal(e_ids, np.where(e_pos >= 0, among[np.maximum(e_pos, 0)], -1))
    Q = fz.embed(ids).cpu().numpy().astype(np.float64)
    bank = fz.embed(among).cpu().numpy().astype(np.float64)
    ok = ids[:, None] != among[None, :]
    worst = check_rows(e_pos, e_score, Q, bank, metric, ok, 8)
    print(f"{name} {metric}: worst score error / bound = {worst:.3f}")
    assert not (e_ids == ids[:, None]).any()                            # exclude_self
    r_ids, r_pos, r_score = near.row(3)
    assert torch.equal(r_ids, near.ids[3][near.pos[3] >= 0]) and r_score.numel() == r_pos.numel()
    # exclude_self=False: a node of the bank may be its own example (cosine 1, l2 0 - up to the rounding the bound allows: the
    # norms and the dot product are summed in different orders)
    free = fz.nearest(ids[-10:], k=8, metric=metric, exclude_self=False)
    check_rows(free.pos.cpu().numpy(), free.score.cpu().numpy(), Q[-10:], bank, metric, np.ones((10, len(among)), bool), 8)
    if metric != "dot":
        assert (free.ids == torch.as_tensor(ids[-10:], device=dev())[:, None]).any(1).all()
    # rows searched in chunks: the same result
    parts = fz.nearest(ids, k=8, metric=metric, chunk=33)
    assert torch.equal(parts.pos, near.pos) and torch.equal(parts.score, near.score) and torch.equal(parts.ids, near.ids)
    # among given explicitly, k larger than the bank
    few = fz.nearest(ids[:5], k=8, among=among[:3], metric=metric, exclude_self=False)
    assert (few.pos[:, :3] >= 0).all() and (few.pos[:, 3:] == -1).all() and torch.isneginf(few.score[:, 3:]).all()
    fz.check()


def test_zero_rows_score_zero_under_cosine():
    """all-zero embedding rows (possible after ReLU): cosine is 0, not NaN - for a zero query row and for a zero bank row"""
    from pcgnn_amd import ops
    c, fz = engine_of("yelp_small")
    among = np.asarray(c.train_pos, dtype=np.int64)
    Q, bank = fz.embed(np.arange(20)).clone(), fz.embed(among).clone()
    Q[4] = 0
    bank[2] = 0
    pos, score = ops.topk_similar(Q, bank, len(among) if len(among) <= 64 else 64, "cosine")
    pos, score = pos.cpu().numpy(), score.cpu().numpy()
    assert np.isfinite(score).all()
    assert (score[4] == 0).all() and np.array_equal(pos[4], np.arange(pos.shape[1]))
    s64 = NR.scores(Q.cpu().numpy(), bank.cpu().numpy(), "cosine")
    assert (s64[:, 2] == 0).all()
    for i in range(20):
        hit = np.nonzero(pos[i] == 2)[0]
        assert all(score[i, j] == 0 for j in hit)
    check_rows(pos, score, Q.cpu().numpy().astype(np.float64), bank.cpu().numpy().astype(np.float64), "cosine",
               np.ones(s64.shape, bool), pos.shape[1])


def test_bank_cache_follows_the_parameters():
    from tests.test_gpu_infer_new import mini, same_theta
    w, mk, _ = mini()
    a = mk()
    fz = a.fused
    ids = np.arange(50, 150)
    first = fz.nearest(ids, k=8)
    bank0 = fz._inf["bank"]["emb"]
    again = fz.nearest(ids, k=8)
    assert fz._inf["bank"]["emb"] is bank0 and torch.equal(again.pos, first.pos) and torch.equal(again.score, first.score)
    other = fz.nearest(ids, k=8, among=np.arange(300))                  # another `among`: rebuilt
    assert fz._inf["bank"]["emb"] is not bank0 and other.among.numel() == 300
    tr = torch.as_tensor(w.idx_train[:256], dtype=torch.int32, device=dev())
    lab = torch.as_tensor(w.labels[w.idx_train[:256]], dtype=torch.int32, device=dev())
    fz.nearest(ids, k=8)
    bank1 = fz._inf["bank"]["emb"]
    fz.train_step(tr, lab)
    after = fz.nearest(ids, k=8)
    assert fz._inf["bank"]["emb"] is not bank1 and not torch.equal(fz._inf["bank"]["emb"], bank1)
    b = mk()
    same_theta(b.fused, fz)
    want = b.fused.nearest(ids, k=8)
    assert torch.equal(after.pos, want.pos) and torch.equal(after.score, want.score) and torch.equal(after.ids, want.ids)
    fz.check()


# ---- queries and the helper ---------------------------------------------------------------------------------------------------
def test_nearest_of_query_rows_and_similar_examples():
    from pcgnn_amd import utils as Ut
    from pcgnn_amd.graph import QueryBatch
    from tests.test_gpu_infer_new import append_rows, engine, split
    c = GoldenCase("yelp_small")
    rs = np.random.RandomState(12)
    nq, N = 24, c.n
    # directed rows behind the graph (the base rows - and with them the bank's embeddings - are the fixture's own): each new
    # node lists itself, base nodes and another new node
    rows = [[[N + i, N + (i + 1) % nq] + rs.choice(N, size=6, replace=False).tolist() for i in range(nq)] for _ in range(c.R)]
    Xf, full_csr = append_rows(c.X, c.csr, rs.randn(nq, c.f), rows)
    Xb, base_csr, Xq, q_pairs = split(Xf, full_csr, N)
    thr = [0.5] * c.R
    full = engine(Xf, full_csr, c.train_pos, c.emb, thr, c.params(), c.alpha)
    base = engine(Xb, base_csr, c.train_pos, c.emb, thr, c.params(), c.alpha)
    query = QueryBatch(Xq, q_pairs, base.g)
    assert torch.equal(full.embed(c.train_pos), base.embed(c.train_pos))
    local = np.array([3, 3, 23, 0, 11])
    for ids in (None, local):
        want = full.nearest(N + (np.arange(nq) if ids is None else ids), k=6)
        got = base.nearest(ids, k=6, query=query)
        assert torch.equal(got.pos, want.pos) and torch.equal(got.score, want.score) and torch.equal(got.ids, want.ids)
    # the helper: examples, probabilities, and the labels of the examples
    labels = np.asarray(c.labels).reshape(-1)
    ids = rs.choice(N, size=30, replace=False)
    near, prob, ex = Ut.similar_examples(base, ids, k=6, labels=labels)
    want = base.nearest(ids, k=6)
    assert torch.equal(near.ids, want.ids) and torch.equal(near.score, want.score)
    assert torch.equal(prob, torch.sigmoid(base.infer(ids)).float())
    e_ids = near.ids.cpu().numpy()
    assert np.array_equal(ex.cpu().numpy(), np.where(e_ids >= 0, labels[np.maximum(e_ids, 0)], -1))
    two = Ut.similar_examples(base, local, k=6, query=query)
    assert len(two) == 2 and torch.equal(two[0].pos, got.pos) and torch.equal(two[1], torch.sigmoid(base.infer_new(query, ids=local)).float())
    base.check()
