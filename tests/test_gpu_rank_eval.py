"""Ranking counts and the alert list on the GPU (pcg_pr_counts, pcg_topk_alerts) and what is built on them (ops.pr_counts,
ops.topk_alerts, utils.device_ranking, FusedPCGNN.evaluate_ranking / alerts, utils.test_ranking with on_device=True): the
integers and the positions == numpy's (tests/rank_eval_ref.py), bit-stable across runs and graph replays, and every metric ==
the host functions'.  Sizes are the smallest that cross each boundary of the kernels.  -m gpu."""
import numpy as np
import pytest
import torch

from tests.rank_eval_ref import alerts_numpy, pr_counts_numpy, scores

pytestmark = pytest.mark.gpu

KINDS = ("continuous", "tied", "edges", "equal")
SHARES = (0.001, 0.145, 0.9)
ROWS_PER_ITER = 256 * 8                      # rows a count-pass workgroup takes per iteration
SORT_LIMIT = 65536                           # positives one workgroup sorts
BIN_WINDOW = 16384                           # bins a bin-pass workgroup counts in LDS
BIN_WINDOWS_MAX = 32 * BIN_WINDOW            # positives up to which the bin pass is windowed
GRID_TURN = 2048 * ROWS_PER_ITER + 1         # the grid-stride loops take a second turn (and the alert tiles double)
SMALL_N = (0, 1, 2, 63, 64, 65, ROWS_PER_ITER - 1, ROWS_PER_ITER, ROWS_PER_ITER + 1)


def dev():
    return torch.device("cuda", 0)


def device_pr(prob, y, cap=None, expect_status=0):
    from pcgnn_amd import ops
    status = ops.eval_status(dev())
    hdr, tp, npred = ops.pr_counts(torch.from_numpy(prob).to(dev()), torch.from_numpy(y.astype(np.int32)).to(dev()), cap)
    got = hdr.cpu().numpy().view(np.uint64), tp.cpu().numpy().view(np.uint32), npred.cpu().numpy().view(np.uint32)
    st = int(status.item())
    status.zero_()
    assert st == expect_status, f"status word {st}"
    return got


def assert_pr(prob, y, what):
    want_hdr, want_tp, want_np = pr_counts_numpy(prob, y)
    hdr, tp, npred = device_pr(prob, y)
    G = int(want_hdr[6])
    print(f"{what}: hdr {hdr[:7].tolist()} (numpy {want_hdr[:7].tolist()})")
    assert np.array_equal(hdr, want_hdr), what
    assert np.array_equal(tp[:G], want_tp) and np.array_equal(npred[:G], want_np), what


def with_positives(n, n1, kind, seed):
    """scores of n rows of which exactly n1, at random positions, are positives"""
    prob, _ = scores(n, 0.5, seed, kind)
    y = np.zeros(n, dtype=np.int32)
    y[np.random.RandomState(seed).choice(n, size=n1, replace=False)] = 1
    return prob, y


# ---- pcg_pr_counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SMALL_N)
def test_pr_counts_small(n):
    for kind in KINDS:
        for share in SHARES:
            prob, y = scores(n, share, n + int(share * 1000), kind)
            assert_pr(prob, y, f"n {n} {kind} share {share}")


@pytest.mark.parametrize("n1", (SORT_LIMIT - 1, SORT_LIMIT, SORT_LIMIT + 1))
@pytest.mark.parametrize("kind", ("continuous", "tied"))
def test_pr_counts_at_the_one_workgroup_sort_limit(n1, kind):
    prob, y = with_positives(70_000, n1, kind, 5)
    assert int(y.sum()) == n1
    assert_pr(prob, y, f"n 70000 {kind} n1 {n1}")


@pytest.mark.parametrize("n,n1", [(20_000, BIN_WINDOW - 1), (20_000, BIN_WINDOW), (20_000, BIN_WINDOW + 1), (40_000, 2 * BIN_WINDOW + 1),
                                  (600_000, BIN_WINDOWS_MAX - 1), (600_000, BIN_WINDOWS_MAX), (600_000, BIN_WINDOWS_MAX + 1)])
def test_pr_counts_at_the_bin_pass_limits(n, n1):
    """one window of LDS bins / two; the windowed bin pass / one global add per row"""
    for kind in ("continuous", "tied"):
        prob, y = with_positives(n, n1, kind, 53)
        assert_pr(prob, y, f"n {n} {kind} n1 {n1}")


@pytest.mark.parametrize("kind", KINDS)
def test_pr_counts_above_the_sort_limit_and_all_but_one_positive(kind):
    prob, y = scores(131_073, 0.9, 17, kind)
    assert int(y.sum()) > SORT_LIMIT
    assert_pr(prob, y, f"n 131073 {kind} share 0.9")
    prob, y = with_positives(SORT_LIMIT + 1, SORT_LIMIT, kind, 19)      # share 1.0 minus one negative
    assert_pr(prob, y, f"n 65537 {kind} n1 65536")


@pytest.mark.parametrize("kind,share", (("tied", 0.145), ("continuous", 0.001), ("equal", 0.9)))
def test_pr_counts_second_grid_turn(kind, share):
    prob, y = scores(GRID_TURN, share, 23, kind)
    assert_pr(prob, y, f"n {GRID_TURN} {kind} share {share}")


def test_pr_counts_one_class():
    prob, y = scores(5000, 0.3, 3, "tied")
    hdr, tp, npred = device_pr(prob, np.zeros_like(y))                  # all labels 0: G = 0
    assert np.array_equal(hdr, pr_counts_numpy(prob, np.zeros_like(y))[0]) and int(hdr[6]) == 0 and int(hdr[4]) == 0
    assert_pr(prob, np.ones_like(y), "all labels 1")
    assert int(pr_counts_numpy(prob, np.ones_like(y))[0][5]) == 0


def test_pr_counts_cap_below_G_sets_the_overflow_bit_and_writes_nothing_past_cap():
    from pcgnn_amd import _lib, ops
    prob, y = scores(5000, 0.3, 29, "continuous")
    want_hdr, want_tp, want_np = pr_counts_numpy(prob, y)
    G, cap = int(want_hdr[6]), 100
    assert G > cap + 50
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    p, l = torch.from_numpy(prob).to(dev()), torch.from_numpy(y).to(dev())
    # the outputs are views of sentinel-filled arrays that extend past cap: ops.pr_counts allocates its own, so call the library
    lib = _lib.load()
    ws = torch.empty(int(lib.pcg_pr_workspace_bytes(len(y))), dtype=torch.uint8, device=dev())
    hdr = torch.empty(8, dtype=torch.int64, device=dev())
    tp = torch.full((cap + 64,), -7, dtype=torch.int32, device=dev())
    npred = torch.full((cap + 64,), -7, dtype=torch.int32, device=dev())
    _lib.check(lib.pcg_pr_counts(ops._p(p), ops._p(l), len(y), cap, ops._p(ws), ops._p(hdr), ops._p(tp), ops._p(npred), ops._p(status),
                                 ops._stream(dev())), "pcg_pr_counts")
    assert int(status.item()) == _lib.PCG_ST_PR_OVERFLOW
    assert np.array_equal(hdr.cpu().numpy().view(np.uint64), want_hdr)  # (G itself is reported)
    assert np.array_equal(tp.cpu().numpy()[:cap].view(np.uint32), want_tp[:cap])
    assert np.array_equal(npred.cpu().numpy()[:cap].view(np.uint32), want_np[:cap])
    assert bool((tp[cap:] == -7).all()) and bool((npred[cap:] == -7).all())
    hdr2, tp2, np2 = device_pr(prob, y, cap=G)                          # cap == G: everything, no bit
    assert np.array_equal(tp2, want_tp) and np.array_equal(np2, want_np)
    device_pr(prob, y, cap=G - 1, expect_status=_lib.PCG_ST_PR_OVERFLOW)


# ---- pcg_topk_alerts -------------------------------------------------------------------------------------------------------
def max_k():
    from pcgnn_amd import _lib
    return _lib.PCG_ALERTS_MAX_K


def assert_alerts(prob, ks, what, strides=(1, 2)):
    from pcgnn_amd import ops
    status = ops.eval_status(dev())
    p1 = np.ascontiguousarray(prob[:, 1])
    want_pos, want_score = alerts_numpy(p1, max(ks))
    inputs = {2: torch.from_numpy(prob).to(dev()), 1: torch.from_numpy(p1).to(dev())}
    for k in ks:
        ke = min(k, len(p1))
        for stride in strides:
            pos, score = ops.topk_alerts(inputs[stride], k)
            pos, score = pos.cpu().numpy(), score.cpu().numpy()
            assert pos.shape == (k,) and score.shape == (k,)
            assert np.array_equal(pos[:ke], want_pos[:ke]), f"{what} k {k} stride {stride}: first difference at " \
                                                            f"{np.nonzero(pos[:ke] != want_pos[:ke])[0][:5].tolist()}"
            assert np.array_equal(score[:ke].view(np.uint32), want_score[:ke].view(np.uint32)), f"{what} k {k} stride {stride}"
            assert np.all(pos[ke:] == -1) and np.all(np.isneginf(score[ke:])), f"{what} k {k}: padding"
    assert int(status.item()) == 0, "status word"
    return want_pos


def all_ks():
    return (1, 2, 63, 64, 65, 1000, 4096, max_k())


@pytest.mark.parametrize("n", SMALL_N + (4096,))
def test_alerts_small(n):
    for kind in KINDS:
        prob, _ = scores(n, 0.145, n + 7, kind)
        assert_alerts(prob, all_ks(), f"n {n} {kind}")                  # (n < k: padding; 64 == 64, 4096 == 4096: n == k)


@pytest.mark.parametrize("n", (70_000, 131_073))
@pytest.mark.parametrize("kind", KINDS)
def test_alerts_medium(n, kind):
    prob, _ = scores(n, 0.145, 31, kind)
    pos = assert_alerts(prob, all_ks(), f"n {n} {kind}")
    if kind == "equal":
        assert np.array_equal(pos, np.arange(max_k()))


def test_alerts_exactly_max_k_rows():
    prob, _ = scores(max_k(), 0.145, 37, "tied")
    assert_alerts(prob, (max_k(), 4096), "n == MAX_K")


@pytest.mark.parametrize("kind", ("continuous", "tied", "equal"))
def test_alerts_second_grid_turn(kind):
    prob, _ = scores(GRID_TURN, 0.145, 41, kind)
    pos = assert_alerts(prob, (1, 1000, max_k()), f"n {GRID_TURN} {kind}", strides=(2,))
    if kind == "equal":
        assert np.array_equal(pos, np.arange(max_k()))


def test_alerts_cut_inside_a_tie_group():
    prob, _ = scores(27_573, 0.145, 43, "tied")
    p1 = prob[:, 1]
    srt = np.sort(p1)[::-1]
    ks = [k for k in (63, 64, 65, 1000, 4096) if srt[k - 1] == srt[k]]
    assert len(ks) >= 3, "the tied input has no tie group at these cuts"
    pos = assert_alerts(prob, ks, "tied, cut inside a group")
    for k in ks:                                                        # the group's members beyond the cut come later in the input
        cut = srt[k - 1]
        taken = np.sort(pos[:k][p1[pos[:k]] == cut])
        group = np.nonzero(p1 == cut)[0]
        assert len(group) > len(taken) and np.array_equal(taken, group[:len(taken)])


# ---- determinism -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(27_573, 1000), (200_000, 4096)])
def test_graph_replay_and_repeat_are_bitwise(n, k):
    from pcgnn_amd import ops
    prob, y = scores(n, 0.7 if n > 100_000 else 0.145, 11, "tied")     # (200 000 at 0.7: the tiled sort)
    p, l = torch.from_numpy(prob).to(dev()), torch.from_numpy(y).to(dev())
    G = int(pr_counts_numpy(prob, y)[0][6])

    def run():
        hdr, tp, npred = ops.pr_counts(p, l)
        pos, score = ops.topk_alerts(p, k)
        return hdr, tp, npred, pos, score

    eager = [t.clone() for t in run()]
    again = [t.clone() for t in run()]
    for a, b in zip(eager, again):
        assert torch.equal(a[:G] if a.numel() == n else a, b[:G] if b.numel() == n else b)
    want_hdr, want_tp, want_np = pr_counts_numpy(prob, y)
    assert np.array_equal(eager[0].cpu().numpy().view(np.uint64), want_hdr)
    assert np.array_equal(eager[1].cpu().numpy().view(np.uint32)[:G], want_tp)
    assert np.array_equal(eager[3].cpu().numpy(), alerts_numpy(prob[:, 1], k)[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = run()
    for _ in range(2):
        for t in captured:
            t.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a[:G] if a.numel() == n else a, b[:G] if b.numel() == n else b)
    assert int(ops.eval_status(dev()).item()) == 0


# ---- bad inputs ---------------------------------------------------------------------------------------------------------------
def test_bad_inputs_raise_through_the_status_bit():
    from pcgnn_amd import _lib, ops, utils as U
    prob, y = scores(5000, 0.2, 13)
    p = torch.from_numpy(prob).to(dev())
    want = U.host_ranking(y, prob, (10, 100))
    assert U.device_ranking(p, y, (10, 100)) == want
    bad = y.copy()
    bad[1234] = 2
    with pytest.raises(_lib.PcgnnLibraryError, match="label outside"):
        U.device_ranking(p, bad, (10,))
    assert int(ops.eval_status(dev()).item()) == 0               # (read and cleared)
    nan = prob.copy()
    nan[77, 1] = np.nan
    with pytest.raises(_lib.PcgnnLibraryError, match="NaN"):
        U.device_ranking(torch.from_numpy(nan).to(dev()), y, (10,))
    assert int(ops.eval_status(dev()).item()) == 0
    assert U.device_ranking(p, y, (10, 100), cap=int(y.sum())) == want
    assert int(ops.eval_status(dev()).item()) == 0


@pytest.mark.parametrize("n,share,kind", [(1, 0.5, "continuous"), (2, 0.5, "continuous"), (2049, 0.145, "edges"), (70_001, 0.145, "tied"),
                                          (70_001, 0.9, "equal")])
def test_device_ranking_equals_host_ranking(n, share, kind):
    from pcgnn_amd import utils as U
    prob, y = scores(n, share, 47, kind)
    ks = (1, 2, 100, 4096, n, n + 5)
    p = torch.from_numpy(prob).to(dev())
    if n == 1:
        with pytest.raises(ValueError, match="Only one class"):
            U.device_ranking(p, y, ks)
        return
    want = U.host_ranking(y, prob, ks)
    assert U.device_ranking(p, y, ks) == want
    assert U.device_ranking(p, y, ks, cap=int(y.sum())) == want
    assert U.device_ranking(p, y) == U.host_ranking(y, prob)


# ---- the engines ---------------------------------------------------------------------------------------------------------------
def trained(w, B):
    from pcgnn_amd.handler import PCGNNTrainer
    t = PCGNNTrainer(w, dict(engine="graph", seed=5, batch_size=B), dev())
    for _ in range(3):
        t.run_epoch_one_graph()
    return t


def check_engine(w, B, capsys=None):
    from pcgnn_amd import utils as U
    fz = trained(w, B).fused
    held = np.setdiff1d(np.arange(w.n), w.idx_train)
    lab = w.labels[held]
    ks = (1, 100, 1000, len(held) + 5)
    prob = U.predict_proba(held, fz, B)
    assert len(np.unique(prob[:, 1])) > 100 and 0.0 < U.roc_auc(lab, prob[:, 1]) < 1.0, "degenerate scores"
    want = U.host_ranking(lab, prob, ks)
    got = fz.evaluate_ranking(held, lab, ks=ks)
    print(got)
    assert set(got) == {"average_precision", "gmean", "precision_at", "recall_at", "n_pos", "n_points"}
    for key, v in want.items():
        assert got[key] == v, (key, got[key], v)
    assert got["average_precision"] == U.average_precision(lab, prob[:, 1])
    assert (got["precision_at"], got["recall_at"]) == U.precision_recall_at_k(lab, prob[:, 1], ks)
    assert fz.evaluate_ranking(held, lab, ks=ks, chunk=1500) == want
    assert fz.evaluate_ranking(held, torch.from_numpy(lab).to(dev()), ks=ks) == want       # labels on the device: cap = n
    assert U.test_ranking(held, lab, fz, B, ks=(100, 1000), on_device=True, print_line=False) == \
        U.test_ranking(held, lab, fz, B, ks=(100, 1000), print_line=False)
    # the alert list: every node, and a shuffled id set with duplicates
    whole = U.predict_proba(np.arange(w.n), fz, B)
    rs = np.random.RandomState(2)
    ids = np.concatenate([held, held[:300]])
    rs.shuffle(ids)
    for sel, pr, k in ((None, whole, 1000), (ids, U.predict_proba(ids, fz, B), 777)):
        want_pos, want_score = alerts_numpy(pr[:, 1], k)
        ids_np = np.arange(w.n) if sel is None else sel
        y_sel = w.labels[ids_np]
        for chunk in (None, 1300):
            al = fz.alerts(sel, k=k, chunk=chunk, labels=y_sel)
            a_ids, a_pos, a_prob, a_hits = al.to_numpy()
            assert np.array_equal(a_pos, want_pos) and np.array_equal(a_prob.view(np.uint32), want_score.view(np.uint32))
            assert np.array_equal(a_ids, ids_np[want_pos]) and np.array_equal(a_hits, np.cumsum(y_sel[want_pos]))
            assert al.n == len(ids_np) and al.k == k
    assert fz.alerts(held[:50], k=64).to_numpy()[1].tolist() == alerts_numpy(U.predict_proba(held[:50], fz, B)[:, 1], 64)[0].tolist()
    fz.check()
    return fz


def test_engine_yelp_like():
    from pcgnn_amd import synth
    check_engine(synth.yelp_like(0), 1024)


def test_engine_mini_and_query_alerts(capsys):
    from pcgnn_amd import utils as U
    from tests.test_gpu_infer_new import mini
    w, mk, mkq = mini()
    fz = check_engine(w, 256)
    t = type("Trainer", (), {"fused": fz})                              # (mkq reads the engine's graph)
    q = mkq(t)
    pq = U.predict_proba_new(q, t.fused)
    assert len(np.unique(pq)) > 100
    want_pos, want_score = alerts_numpy(pq, 100)
    al = t.fused.alerts(k=100, query=q)
    assert np.array_equal(al.pos.cpu().numpy(), want_pos) and np.array_equal(al.ids.cpu().numpy(), want_pos)
    assert np.array_equal(al.prob.cpu().numpy().view(np.uint32), want_score.view(np.uint32))
    ids = np.array([5, 5, 499, 0, 17, 250, 5])
    al = t.fused.alerts(ids, k=10, query=q, chunk=3)
    want_pos, want_score = alerts_numpy(U.predict_proba_new(q, t.fused, ids=ids), 10)
    assert np.array_equal(al.pos.cpu().numpy(), want_pos) and np.array_equal(al.prob.cpu().numpy().view(np.uint32), want_score.view(np.uint32))
    assert np.array_equal(al.ids.cpu().numpy()[:7], ids[want_pos[:7]]) and np.all(al.ids.cpu().numpy()[7:] == -1)
    # the printed line
    held = np.setdiff1d(np.arange(w.n), w.idx_train)
    capsys.readouterr()
    U.test_ranking(held, w.labels[held], fz, 256, ks=(100,), on_device=True)
    line = capsys.readouterr().out
    assert "AveragePrecision" in line and "G-mean" in line and "P@100" in line and "R@100" in line
