"""CPU-only tests of the host side of the front / score / optimizer entry-point tests (tests/front_ref.py): the chosen widths
reach every row geometry, the chosen train_pos lengths straddle every tier's grid-stride turn of the key group, a score that
lost a column or took the neighbouring row is far outside the bound the GPU test allows, the optimizer inputs keep the
cancellation cap - and a feature table wider than 512 floats is refused by every entry point that scores it, before anything is
enqueued."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import adam_ref as A
from tests import dense_ref as D
from tests import front_ref as R


def test_widths_cover_every_geometry():
    for widths, want_ragged in ((R.SCORE_WIDTHS, True), (R.KEY_WIDTHS, False)):
        geo = {}
        for F in widths:
            stride = R.stride_of(F)
            geo.setdefault((R.lanes_per_row(stride), 2 if stride > 256 else 1), []).append(F)
        assert sorted(geo) == [(8, 1), (16, 1), (32, 1), (64, 1), (64, 2)], widths
        if want_ragged:
            for tier, ws in geo.items():
                assert any(F % 4 == 0 for F in ws) and any(F % 4 != 0 for F in ws), tier
            assert 256 in geo[(64, 1)] and {257, 260} <= set(geo[(64, 2)]) and 512 in geo[(64, 2)]
    assert len(R.KEY_WIDTHS) == 5                           # one per tier
    # every width's table sizes lie on both sides of a workgroup's rows per iteration, and the large table gives the capped
    # grid a second turn of its grid-stride loop with a ragged tail
    for F in R.SCORE_WIDTHS:
        rb = R.rows_per_block(F)
        assert rb == {8: 256, 16: 128, 32: 64, 64: 32}[R.lanes_per_row(R.stride_of(F))]
        assert {1, rb - 1, rb, rb + 1, R.TABLE_ROWS} == set(R.table_sizes(F)) and R.TABLE_ROWS > rb + 1
    F, n = R.SECOND_TURN
    per_turn = R.SCORE_BLOCKS_MAX * R.rows_per_block(F)
    assert R.lanes_per_row(R.stride_of(F)) == 64 and per_turn < n < 2 * per_turn and (n - per_turn) % R.rows_per_block(F) != 0
    assert n * R.stride_of(F) * 4 <= 35 * 2 ** 20


def test_n_pos_lists_straddle_every_turn():
    turns = {}
    for F in R.KEY_WIDTHS:
        T = R.keys_per_turn(F)
        turns[R.lanes_per_row(R.stride_of(F))] = T
        ns = R.n_pos_list(F)
        assert ns[0] == 1 and T - 1 in ns and T in ns and T + 1 in ns, F
        assert min(ns) <= T < max(ns) <= R.RANK_MAX, F          # a key on both sides of the turn, none beyond the rank sort
        assert max(ns) + 500 == R.key_table(F)[1]
        for n_pos in ns:
            tp = R.train_pos_list(R.key_table(F)[1], n_pos, n_pos)
            assert np.unique(tp).size == n_pos
            assert n_pos <= 2 or np.any(np.diff(tp) < 0), "not ascending"
    assert turns == {8: 8192, 16: 4096, 32: 2048, 64: 1024}
    # the copied rows make equal scores among the train positives of the longest list
    for F in R.KEY_WIDTHS:
        X, n = R.key_table(F)
        W, b = R.weights(F, 1)
        s = R.scores_f32(X, W[0], b[0])
        tp = R.train_pos_list(n, max(R.n_pos_list(F)), max(R.n_pos_list(F)))
        assert np.unique(s[tp]).size < tp.size, F


def test_orderable_key_orders_like_the_floats():
    s = np.array([-np.inf, -2.5, -1e-30, -0.0, 0.0, 1e-30, 1.0, 1.0, np.inf], dtype=np.float32)
    o = R.orderable(s)
    assert np.all(np.diff(o.astype(np.int64))[[0, 1, 2, 3, 4, 5, 7]] > 0) and o[6] == o[7]
    k = R.pos_keys(s, np.arange(s.size))
    assert np.all(np.diff(k.astype(object)) > 0)                # equal scores: the position decides
    cap = R.sort_capacity(s.size)
    out = R.sorted_keys(s[::-1].copy(), np.arange(s.size), cap)
    assert cap == 4096 and out.size == cap and np.all(out[s.size:] == np.uint64(0xFFFFFFFFFFFFFFFF))
    assert (out[:s.size] & np.uint64(0xFFFFFFFF)).tolist() == [8, 7, 6, 5, 4, 3, 1, 2, 0]       # (equal scores: by position)
    assert R.sort_capacity(4097) == 8192 and R.sort_capacity(16384) == 16384


@pytest.mark.parametrize("F", sorted(set(R.SCORE_WIDTHS + R.KEY_WIDTHS)))
def test_a_wrong_score_is_ten_tolerances_away(F):
    """a column left out of the dot (the last one, column 4, one at or past 256) or the neighbouring row's score: rel_err
    against float64 moves by more than ten times the bound the GPU test allows the kernels, at every table size used"""
    X = R.table()[:, :F]
    W, b = R.weights(F, 0)
    assert np.all(np.abs(W) >= 0.5) and np.all(np.abs(W) <= 1.5) and ((W < 0).any() or F < 3) and np.all(np.abs(b) >= 0.5)
    for col in (0, 1):
        ref = R.scores_f64(X, W[col], b[col])
        for n in R.table_sizes(F):
            _, e32, tol = R.score_check(R.scores_f32(X[:n], W[col], b[col]), X[:n], W[col], b[col])
            assert e32 <= tol and tol < 1e-4
            for c in R.dropped_columns(F):
                wrong = ref[:n] - X[:n, c].astype(np.float64) * float(W[col, c])
                moved = D.rel_err(wrong, ref[:n])
                assert moved > 10 * tol, (F, n, col, c, moved, tol)
            if n > 1:
                moved = D.rel_err(np.roll(ref[:n], 1), ref[:n])
                assert moved > 10 * tol, (F, n, col, "neighbouring row", moved, tol)
    # a single-row table is a well-conditioned score: nothing the bound's floor could not hold
    assert abs(R.scores_f64(X[:1], W[0], b[0])[0]) >= 2.0 ** -4 * np.sqrt(F)


def test_optimizer_inputs_keep_the_cancellation_cap():
    """CANCEL_CAP is a condition on the inputs, not a measurement: the float64 reference alone leaves out at most that share of
    the parameters for every (n_slabs, t) the GPU test runs, and its own float32 restatement passes adam_figures"""
    F, E, Rn = R.OPT_SHAPE
    n_params, o_clf = R.opt_n_params(F, E, Rn), R.opt_clf_offset(F, E, Rn)
    assert o_clf % 64 != 0 and n_params % 64 != 0 and n_params - o_clf == 2 * F + 2
    from pcgnn_amd import _lib
    lib = _lib.load()
    assert int(lib.pcg_dense_n_params(F, E, Rn)) == n_params and int(lib.pcg_dense_param_offset(F, E, Rn, 3, 0)) == o_clf
    for n_slabs in R.OPT_SLABS:
        for t in R.OPT_T:
            x = R.opt_inputs(n_params, n_slabs, t)
            assert x["slabs"].shape == (n_slabs, n_params) and float(x["v"].min()) >= 0.0
            g = R.slab_sum_f64(x["slabs"])
            share = float(A.cancelled(x["theta"], g, R.OPT_WD).double().mean())
            assert share <= A.CANCEL_CAP, (n_slabs, t, share)
            g32 = R.slab_sum_f32(x["slabs"])
            assert D.rel_err(g32, g) <= D.tolerance(0.0) + 1e-6
            ref = A.adam_ref(x["theta"], x["m"], x["v"], g, t, R.OPT_LR, R.OPT_BETAS, R.OPT_EPS, R.OPT_WD)
            step = float((ref[0] - torch.from_numpy(x["theta"]).double()).abs().max())
            assert step <= R.OPT_STEP_CAP and float(ref[0].abs().max()) <= R.OPT_THETA_CAP, (n_slabs, t, step)
            got = [y.float() for y in A.adam_ref(x["theta"], x["m"], x["v"], g32, t, R.OPT_LR, R.OPT_BETAS, R.OPT_EPS, R.OPT_WD)]
            fig = A.adam_figures(got, x["theta"], x["m"], x["v"], g32, t, R.OPT_LR, R.OPT_BETAS, R.OPT_EPS, R.OPT_WD)
            assert fig["theta"] <= 1 and fig["m"] <= 1 and fig["v"] <= 1 and fig["excluded"] <= A.CANCEL_CAP, fig
    assert R.opt_inputs(64, 0, 1)["slabs"].shape == (0, 64)


# ---- a table wider than 512 floats ---------------------------------------------------------------------------------------------
def test_a_table_wider_than_512_floats_is_refused_before_any_launch():
    """feat_dim = feat_stride = 516: score_table_body / score_marked_body give a lane two float4 chunks of a row - the columns
    from 512 on would be left out of s0 while the raw keys and pcg_score_rows kept them.  Every entry point that takes plain
    arguments and scores the table answers PCG_E_UNSUPPORTED before it enqueues anything (the pointers here are host memory: a
    launch would not get as far as reading them - there is no device in this test), pcg_segment_mean as before."""
    from pcgnn_amd import _lib
    lib = _lib.load()
    raw = C.create_string_buffer(1 << 16)
    base = (C.addressof(raw) + 255) // 256 * 256
    ptr = lambda k: C.c_void_p(base + 4096 * k)              # non-NULL, 16-byte aligned dummies
    g = _lib.GraphDesc()
    g.n_nodes, g.feat_dim, g.feat_stride, g.n_rel, g.n_pos, g.max_degree = 64, 516, 516, 1, 8, 1
    g.X, g.train_pos = ptr(0), ptr(1)
    g.indptr[0], g.indices[0] = ptr(2), ptr(3)
    W, b, s0, keys, nodes, labels, ws, status, sync = (ptr(k) for k in range(4, 13))
    thr, rho = (C.c_double * 1)(0.5), (C.c_double * 1)(0.5)
    U = _lib.PCG_E_UNSUPPORTED
    gr = C.byref(g)
    assert lib.pcg_score_table(gr, W, b, 0, 64, s0, None) == U
    assert lib.pcg_score_table(gr, W, b, 5, 5, s0, None) == U          # (an empty range too: the shape is what is refused)
    assert lib.pcg_step_front(gr, W, b, s0, keys, nodes, labels, 4, thr, rho, 1, 0, ws, 1024, status, None) == U
    assert lib.pcg_step_front(gr, W, b, s0, keys, nodes, labels, 0, thr, rho, 1, 0, ws, 1024, status, None) == U
    assert lib.pcg_step_front_a(gr, W, b, 0, 64, s0, None, keys, nodes, labels, 4, thr, rho, 1, 0, ws, 1024, status, None) == U
    assert lib.pcg_step_front_a(gr, W, b, 0, 64, s0, ptr(13), None, nodes, None, 4, thr, rho, 0, 0, ws, 1024, status, None) == U
    assert lib.pcg_step_scores(gr, W, b, 0, 64, s0, None, keys, -1, sync, None, None) == U
    assert lib.pcg_step_scores(gr, W, b, 0, 64, s0, None, keys, -1, sync, ptr(13), None) == U      # (a touched map: the same answer)
    assert lib.pcg_step_scores(gr, W, b, 0, 64, s0, ptr(13), None, -1, sync, None, None) == U
    assert lib.pcg_segment_mean(gr, ptr(5), ptr(6), ptr(7), 4, 0, ptr(8), 520, None) == U
    # the struct-taking fronts: the same check sits behind their own argument checks
    st = _lib.TrainState(theta=ptr(4), m=ptr(5), v=ptr(6), step_counter=ptr(7), sync_words=sync, slabs=ptr(8), emb=16,
                         hyper=_lib.AdamHyper(0.01, 0.9, 0.999, 1e-8, 0.0))
    batch = _lib.Batch(ids=nodes, labels=labels, cnt=ptr(9), plan=None, B=4, inv_count=0.25)
    sel = _lib.SelectWs(thresholds=thr, rho=rho, workspace=ws, status=status, list_capacity=1024, add_self=0)
    assert lib.pcg_step_scores_train(gr, C.byref(st), s0, keys, None, None) == U
    assert lib.pcg_step_front_train(gr, C.byref(st), s0, keys, C.byref(batch), C.byref(sel), None) == U
    g.feat_dim = 510                                          # pcg_step_scores_dist looked at feat_dim only: stride 516 passed
    assert lib.pcg_step_scores_dist(gr, C.byref(st), ptr(9), ptr(10), 0, 64, s0, None, None, -1, None) == U
    # the widest supported stride is not refused for its shape (an argument error instead: rows beyond the table)
    g.feat_dim = g.feat_stride = 512
    assert lib.pcg_score_table(gr, W, b, 0, 65, s0, None) == _lib.PCG_E_ARG
