"""CPU-only tests of the edge-shape table (tests/dense_ref.py: EDGE_SHAPES and the lists beside it) the GPU tests of
tests/test_gpu_edge_shapes.py, tests/test_gpu_grad_f64.py and tests/test_gpu_custom_loss.py run:

* which of its six instantiations each of the four users of dense_tile_body - training, the seeded backward, whole-set inference,
  attribution - picks for every shape, from the host's dispatch rules restated in Python, and that the 24 instantiations are
  each launched by a shape some GPU test runs;
* the same for the fifth user, the fused launch of the pipelined step (twelve instantiations: the six times the select half's
  presorted variant), conditioned on what dense_select_blocks accepts and on when the classifier runs two batches ahead;
* the attribution's LDS overlay: every combination is in the table - the fourth (dcat over, dx0 appended), which only the padding
  of K2 makes reachable and only at R = 1, included;
* the attribution's shape limit through the C ABI (fake descriptors, n = 0: nothing is launched), against the restated rule;
* every new case keeps the ReLU-kink caps of its test with the oracle's sets, on the CPU;
* mistakes planted in the reference - relation 8 ignored, output columns 256 .. 271 zero, feature columns >= 256 left out of a
  neighbour's dot product - move every affected tensor by at least ten of the GPU tests' tolerances."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import attr_ref as A
from tests import dense_ref as D
from tests import vjp_ref as V
from tests.test_attr_ref_host import index_of
from tests.test_gpu_embed import AMBIGUOUS_SHARE, bounds, forward_refs
from tests.util import PARAM_KEYS

WAVES = 16
# (F, E, R) -> (the weights' LDS copy in training / the seeded backward, in inference / attribution)
EXPECTED = {
    (16, 64, 4): (True, True), (30, 64, 3): (True, True), (20, 128, 1): (True, True), (20, 32, 7): (True, True),
    (17, 32, 8): (True, True), (32, 64, 8): (False, False), (64, 64, 3): (False, False), (16, 272, 1): (False, False),
}


def kparts(E):
    return WAVES // (E // 16) if E // 16 <= WAVES else 1


def run_time_kernel(user, wlds):
    tail = ", false>" if user in ("infer", "attr") else ">"
    return f"{D.USERS[user]}<{str(wlds).lower()}, 0, 0, 0{tail}"


# ---- dispatch -------------------------------------------------------------------------------------------------------------------
def test_each_user_picks_the_kernel_the_table_says():
    assert set(EXPECTED) == set(D.EDGE_SHAPES)
    for shape, (train_wlds, infer_wlds) in EXPECTED.items():
        assert D.dense_wlds(*shape) == train_wlds and D.infer_wlds(*shape) == infer_wlds, shape
        assert D.EDGE_SHAPES[shape][0] == D.kernel_of("train", *shape) == run_time_kernel("train", train_wlds), shape
        assert D.kernel_of("vjp", *shape) == run_time_kernel("vjp", train_wlds), shape
        assert D.kernel_of("infer", *shape) == run_time_kernel("infer", infer_wlds), shape
        assert D.kernel_of("attr", *shape) == run_time_kernel("attr", infer_wlds), shape
        assert D.dense_smem_bytes(*shape, train_wlds) <= 160 * 1024 and D.attr_smem_bytes(*shape) <= 160 * 1024, shape
        assert shape not in D.FIXED and shape not in D.SHAPES and shape not in D.WIDE_SHAPES
    # what each shape is in the table for
    assert kparts(64) == 4 and kparts(128) == 2 and kparts(32) == 8 and kparts(272) == 1
    F, E, R = 30, 64, 3                                                   # next to the fixed shapes; a padded feature stride
    assert (32, E, R) in D.FIXED and (25, E, R) in D.FIXED and F % 4 != 0 and (F + 3) // 4 * 4 == 32
    assert (17 + 3) // 4 * 4 == 20 and 17 % 2 == 1
    assert 8 * 64 // 16 == 2 * WAVES                                      # (32, 64, 8): two turns of the h_r wave loop
    assert 272 // 16 == WAVES + 1 and 1024 % (272 // 4) != 0              # (16, 272, 1): no LDS copy whatever its size
    assert 16 * 64 <= 1024 < 16 * 65                                      # F = 64: the last width a thread per self element covers
    # three of the LDS-weight shapes leave less than 4 KiB of the 160 KiB free
    for shape in [(16, 64, 4), (30, 64, 3), (17, 32, 8)]:
        assert 160 * 1024 - D.dense_smem_bytes(*shape, True) < 4096, shape
    # the fixed-shape kernels, by the same function (dense_ref.SHAPES names the training kernels)
    for shape, (kernel, _, _) in list(D.SHAPES.items()) + list(D.WIDE_SHAPES.items()):
        assert D.kernel_of("train", *shape) == kernel, shape


def launched():
    """user -> the shapes some GPU test launches it with: tests/test_gpu_grad_f64.py (train), tests/test_gpu_custom_loss.py over
    vjp_ref.SHAPES (vjp), tests/test_gpu_attribute.py over attr_ref.SHAPES (attr, and infer: its logits are compared with
    infer's) and tests/test_gpu_edge_shapes.py (infer, attr)"""
    return {"train": list(D.SHAPES) + list(D.WIDE_SHAPES) + list(D.EDGE_SHAPES), "vjp": list(V.SHAPES),
            "infer": list(A.SHAPES) + D.EDGE_INFER_SHAPES, "attr": list(A.SHAPES) + D.EDGE_ATTR_SHAPES}


def test_every_instantiation_is_launched_by_a_gpu_test_shape():
    want = {u: {f"{k}<{str(w).lower()}, {F}, {E}, {R}" + ((", true>" if F else ", false>") if u in ("infer", "attr") else ">")
                for w, F, E, R in D.INSTANTIATIONS} for u, k in D.USERS.items()}
    assert sum(len(v) for v in want.values()) == 24
    for user, shapes in launched().items():
        got = {D.kernel_of(user, *s) for s in shapes}
        assert None not in got, (user, [s for s in shapes if D.kernel_of(user, *s) is None])
        assert got == want[user], (user, want[user] - got)
    # the run-time LDS-weight inference and attribution kernels: by the edge table alone (no other table reaches them)
    for user in ("infer", "attr"):
        assert run_time_kernel(user, True) in {D.kernel_of(user, *s) for s in D.EDGE_SHAPES}
        others = list(D.SHAPES) + list(D.WIDE_SHAPES)
        assert run_time_kernel(user, True) not in {D.kernel_of(user, *s) for s in others}
    # the run-time LDS-weight training and vjp kernels at E = 32, 64 and 128
    for user in ("train", "vjp"):
        embs = {s[1] for s in launched()[user] if D.kernel_of(user, *s) == run_time_kernel(user, True)}
        assert {16, 64, 128} <= embs and (user == "vjp" or 32 in embs), (user, embs)
    # the fixed F = 25 vjp kernels, and the vjp on wide rows
    assert {(25, 64, 3), (25, 128, 3)} <= set(V.SHAPES) and max(s[0] for s in V.SHAPES) > 64
    assert D.REL_DEG.keys() >= {4, 7, 8} and all(len(D.REL_DEG[R]) == R for R in D.REL_DEG)


# ---- the fifth user: the fused launch of the pipelined step -------------------------------------------------------------------------
def graph_of(w):
    """(F, R, train positives, maximum degree): what the fused launch's host rules read of a workload"""
    return w.X.shape[1], len(w.csr), len(w.train_pos), max(int(np.diff(ip).max()) for ip, _ in w.csr)


def fused_kernels(w, E, B, switch, lengths):
    """the fused launch's instantiations that sequences of `lengths` steps over batches of B rows launch, the engine's clf_ahead
    switch as given (None: its default, on from 1024 train positives); a sequence is pipelined from two steps (_pipelines)"""
    F, R, P, deg = graph_of(w)
    switch = P >= 1024 if switch is None else switch
    got = {D.fused_kernel_of(F, E, R, B, P, deg, D.fused_steps_ahead(F, E, R, B, P, deg, switch, n)) for n in lengths if n >= 2}
    return got - {None}


def compared_lengths(w, B):
    """the sequences of test_gpu_pipelined_step._run_and_compare: two epochs, one epoch, batches 0 .. mid"""
    nb = -(-2 * len(w.train_pos) // B)
    return 2 * nb, nb, nb // 2 + 1


def test_every_fused_launch_instantiation_is_launched_by_a_gpu_test():
    """tests/test_gpu_pipelined_step.py (but for its other shapes), tests/test_gpu_clf_ahead.py and
    tests/test_gpu_launch_sequences.py train at emb 64 on F = 32 and F = 25 only, and the F = 25 graph has too few train positives
    for the classifier to run ahead: three of the twelve kernels.  The other shapes of test_gpu_pipelined_step.py reach the other
    nine, each case the kernel it is there for."""
    from pcgnn_amd import synth
    from tests import test_gpu_clf_ahead as CA
    from tests import test_gpu_launch_sequences as LS
    from tests import test_gpu_pipelined_step as PS
    name = lambda w, F, E, R, pre: f"{D.FUSED_KERNEL}<{str(w).lower()}, {F}, {E}, {R}, {str(pre).lower()}>"
    want = {name(*inst, pre) for inst in D.INSTANTIATIONS for pre in (True, False)}
    assert len(want) == 12
    mini = lambda feat: synth.make_workload("mini", PS.MINI["n"], feat, PS.MINI["rel_edges"], PS.MINI["pos_rate"], seed=PS.MINI["seed"])
    old = set()
    for w, batches in ((mini(32), [256]), (synth.yelp_like(0), [1024, 2048]), (synth.amazon_like(0), [256])):
        for B in batches:
            got = fused_kernels(w, 64, B, None, compared_lengths(w, B))
            assert got, (w.name, B)                                       # (pipelined, as the tests assert on the device)
            old |= got
    assert D.dense_select_blocks(32, 64, 3, 2064, 1000, 100) == 0         # test_above_threshold_falls_back: 129 tiles
    for with_pos in (True, False):                                        # test_gpu_clf_ahead.py: both engines of a pair
        w = CA.workload(with_pos)[0]
        for switch in (True, False):
            old |= fused_kernels(w, 64, CA.B, switch, (1, 2, 3, 4, 5, 6, 7))
    for switch in (None, True, False):                                    # test_gpu_launch_sequences.py: new_trainer(ahead=...)
        old |= fused_kernels(mini(32), 64, LS.BATCH, switch, (2, 3, 6))
    assert old == {name(True, 32, 64, 3, True), name(True, 32, 64, 3, False), name(True, 25, 64, 3, False)}, old
    new = set()
    for feat, emb, ahead in PS.OTHER_SHAPES:
        w = mini(feat)
        got = fused_kernels(w, emb, PS.MINI["B"], ahead, compared_lengths(w, PS.MINI["B"]))
        wlds = D.dense_wlds(feat, emb, 3)
        shape = (feat, emb, 3) if D.FIXED.get((feat, emb, 3)) == wlds else (0, 0, 0)
        mine = name(wlds, *shape, ahead)
        assert mine in got and mine not in old and mine not in new, (feat, emb, ahead, got)
        new.add(mine)
    assert new == want - old and len(new) == len(PS.OTHER_SHAPES) == 9
    # the two run-time-shape cases are the edge table's (30, 64, 3), weights in LDS, and (64, 64, 3), weights streamed
    assert EXPECTED[(30, 64, 3)][0] and not EXPECTED[(64, 64, 3)][0]


def test_the_table_has_the_maximum_relation_count_and_more_column_tiles_than_waves():
    rels = {s[2] for s in D.EDGE_SHAPES}
    assert {4, 7, 8} <= rels
    assert {D.dense_wlds(*s) for s in D.EDGE_SHAPES if s[2] == 8} == {True, False}      # R = 8 with the copy and without
    assert any(s[1] // 16 > WAVES for s in D.EDGE_SHAPES)
    assert set(D.EDGE_TRAIN_SHAPES) <= set(D.EDGE_SHAPES) and {s[2] for s in D.EDGE_TRAIN_SHAPES} >= {4, 8}
    assert any(s[1] // 16 > WAVES for s in D.EDGE_TRAIN_SHAPES)
    assert any(s[0] > 256 for s in D.EDGE_ATTR_SHAPES) and (260, 16, 1) in D.EDGE_INFER_SHAPES


# ---- the attribution's LDS overlay ------------------------------------------------------------------------------------------------
def overlay(shape):
    return D.attr_dcat_over_cat(*shape), D.attr_dx0_over_comb(shape[0], shape[1])


def test_the_table_has_every_reachable_overlay_combination():
    seen = {}
    for shape in D.EDGE_ATTR_SHAPES:
        seen.setdefault(overlay(shape), []).append(shape)
    assert set(seen) == {(True, True), (False, True), (False, False), (True, False)}, seen
    # dcat appended with dx0 over `combined`: with the weights' LDS copy and without
    assert {D.infer_wlds(*s) for s in seen[False, True]} == {True, False}
    assert overlay((20, 32, 7)) == overlay((64, 64, 3)) == (False, True)
    assert seen[True, False] == list(D.ATTR_OVERLAY_SHAPES) == [(24, 16, 1)]
    # what the older attribution tests run: (over, over) and (appended, appended) only
    assert {overlay(s) for s in A.SHAPES} == {(True, True), (False, False)}


def test_dcat_over_with_dx0_appended_needs_one_relation_and_the_k_padding():
    """The fourth combination - dcat over the [self | h] tile, dx0 appended - needs F > E and R (2F + 1) <= K2p + 1.  Without
    the padding of K2 = F + R E to a multiple of 16 the two contradict each other (R (2F + 1) > F + R E + 1 whenever F > E); with
    it they do not: an exhaustive scan finds the combination at R = 1, E < F <= E + 8, 2F <= K2p and nowhere else.  The
    attribution accepts those shapes, so attr_tile_backward's address expression for them is live code, and (24, 16, 1) runs it
    with dcat [16][2F + 1] filling the tile [16][K2p + 1] to the float."""
    found = [(F, E, R) for E in range(16, 513, 16) for R in range(1, 9) for F in range(1, 513)
             if D.attr_dcat_over_cat(F, E, R) and not D.attr_dx0_over_comb(F, E)]
    rule = [(F, E, 1) for E in range(16, 513, 16) for F in range(E + 1, min(E + 8, 512) + 1) if 2 * F <= (F + E + 15) // 16 * 16]
    assert found == rule and found, (found[:5], rule[:5])
    assert not [s for s in found if s[2] > 1]
    F, E, R = (24, 16, 1)
    assert (F, E, R) in found and D.attr_shape_ok(F, E, R) and R * (2 * F + 1) == (F + R * E + 15) // 16 * 16 + 1
    assert sum(D.attr_shape_ok(*s) for s in found) > 100                   # (accepted shapes, not a corner the host refuses)


# ---- the attribution's shape limit, through the C ABI --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import pcgnn_amd
    from pcgnn_amd import _lib
    pcgnn_amd.build_library()
    return _lib.load()


def attr_set_rc(lib, F, E, R):
    """pcg_attr_set over a host-only descriptor with dummy addresses that are never dereferenced, n = 0: PCG_OK or the refusal"""
    from tests.test_query_batch_host import host_desc
    g = host_desc(1000, feat_dim=F, n_rel=R)
    g.X = 0x1000
    thr = (C.c_double * R)(*[0.5] * R)
    at = C.c_void_p(0x1000)
    return lib.pcg_attr_set(C.byref(g), at, E, at, 0, 16, at, thr, at, 100, 0.0, 1.0, at, at, at, at, at, at, None)


def explain_new_rc(lib, F, E, R):
    from tests.test_explain_new_host import ATTR, CHOSEN, explain_out
    from tests.test_query_batch_host import host_desc
    g, q = host_desc(1000, feat_dim=F, n_rel=R), host_desc(10, feat_dim=F, n_rel=R)
    thr = (C.c_double * R)(*[0.5] * R)
    out = explain_out(*ATTR, *CHOSEN, neigh=True)
    return lib.pcg_explain_new(C.byref(g), C.byref(q), None, E, None, 0, 4, None, 1, thr, None, 100, 0.0, 1.0, C.byref(out), None, None)


def test_attribution_limit_through_the_c_abi(lib):
    from pcgnn_amd import _lib
    assert D.ATTR_LIMITS[0] == tuple(D.ATTR_LIMIT_SHAPES)
    for last, first_refused in D.ATTR_LIMITS:
        assert first_refused == (last[0] + 1,) + last[1:]
        assert D.attr_smem_bytes(*last) <= 160 * 1024 < D.attr_smem_bytes(*first_refused)
        assert D.kernel_of("attr", *last) is not None and D.kernel_of("attr", *first_refused) is None
        assert D.kernel_of("infer", *first_refused) is not None              # inference itself has room
        for call in (attr_set_rc, explain_new_rc):
            assert call(lib, *last) == _lib.PCG_OK, (call.__name__, last)
            assert call(lib, *first_refused) == _lib.PCG_E_UNSUPPORTED, (call.__name__, first_refused)
    # the restated rule is the library's: every edge shape, and every width around the two limits
    shapes = D.EDGE_ATTR_SHAPES + [(F, 16, 1) for F in range(340, 381)] + [(F, 64, 3) for F in range(110, 135)]
    for shape in shapes:
        want = _lib.PCG_OK if D.attr_shape_ok(*shape) else _lib.PCG_E_UNSUPPORTED
        assert attr_set_rc(lib, *shape) == want and explain_new_rc(lib, *shape) == want, shape


# ---- the ReLU-kink caps, with the oracle's sets ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    shapes = list(dict.fromkeys(list(D.EDGE_SHAPES) + D.EDGE_INFER_SHAPES + D.EDGE_ATTR_SHAPES))
    return {shape: D.GradCase.of(shape) for shape in shapes}


@pytest.fixture(scope="module")
def whole_sets(cases):
    """shape -> the index of the oracle's test-mode selection over the whole graph"""
    return {shape: A.sets_to_index(A.host_test_sets(c, np.arange(c.n))) for shape, c in cases.items()}


@pytest.fixture(scope="module")
def grad_refs(cases):
    """(shape, B) -> (ref64, ref32, share of ambiguous activations, index of the oracle's train-mode sets) for the batches of
    the gradient and train-step tests"""
    out = {}
    for shape, (_, batches, _) in D.EDGE_SHAPES.items():
        c = cases[shape]
        for B in sorted(set(batches)):
            ids, lab = c.batch(B)
            index = D.sets_to_index(c.host_sets(ids, lab))
            out[shape, B] = D.reference_pair(c, ids, lab, index)[:3] + (index,)
    return out


def test_gradient_cases_keep_the_ambiguous_cap(grad_refs):
    over = {k: v[2] for k, v in grad_refs.items() if v[2] > D.AMBIGUOUS_CAP}
    assert not over, f"ambiguous ReLU pre-activations above {D.AMBIGUOUS_CAP}: {over} - change the seed"
    assert all((s, B) in grad_refs for s in D.EDGE_TRAIN_SHAPES for B in (17, 1025))
    assert set(V.SHAPES) <= set(D.SHAPES) | set(D.WIDE_SHAPES) | set(D.EDGE_SHAPES)     # (tests/test_vjp_host.py checks the vjp cases)


def attr_pair(c, ids, index, target=A.TARGETS[0]):
    return tuple(A.attr_ref(c.X, ids, index, c.params(), target, dt) for dt in (torch.float64, torch.float32))


def test_attribution_cases_keep_the_row_cap(cases, whole_sets):
    for shape in D.EDGE_ATTR_SHAPES:
        c, whole = cases[shape], whole_sets[shape]
        assert all(float(cnt.min()) >= 1 for _, _, cnt in whole)
        sets = {k: v for k, v in A.id_sets(c).items() if k != "whole"}
        assert len(np.unique(sets["n65"])) < 65, f"{shape}: the batch of 65 has no node twice - change the salt"
        if shape == (260, 16, 1):
            sets["hubs"] = A.hub_ids(c)
        for name, ids in sets.items():
            r64, r32 = attr_pair(c, ids, index_of(whole, ids))
            # (the margin of tests/test_attr_ref_host.py: the batches keep the condition with the band doubled)
            wide = A.kept_rows(r64["pre"], r32["pre"], widen=2.0)[1]
            assert wide <= A.ROW_CAP, f"{shape} {name}: {wide:.2%} of the rows are ambiguous in the doubled band - change the salt"
            assert A.residual(r64, A.TARGETS[0]) <= 1e-12, (shape, name)
        # the lone row's inner products do not cancel (attr_ref.COND_CAP: its tensors have one element)
        ids = sets["n1"]
        for target in A.TARGETS:
            cond = A.contrib_condition(c.X, ids, index_of(whole, ids), attr_pair(c, ids, index_of(whole, ids), target)[0])
            assert cond <= A.COND_CAP, f"{shape} target {target}: the lone row has a product of condition {cond:.1f} - change the salt"


def test_hub_rows_run_the_tail_slices_with_two_chunks_per_lane(cases, whole_sets):
    """(260, 16, 1): a chosen list of more than 128 entries among the ids (the neighbour kernel's tail slices), on rows of
    stride > 256 (a lane's second float4 chunk)"""
    c = cases[(260, 16, 1)]
    ids = A.hub_ids(c)
    assert list(ids[:2]) == c.hubs(2) and len(ids) == 65
    kept = index_of(whole_sets[(260, 16, 1)], ids)[0][2]
    assert float(kept.max()) > 128 and (c.f + 3) // 4 * 4 > 256
    assert max(int(np.diff(ip).max()) for ip, _ in c.csr) > 128                       # (max_degree: the launch has tail slices)


def test_embed_cases_keep_the_ambiguous_share(cases, whole_sets):
    for shape in D.EDGE_INFER_SHAPES:
        c = cases[shape]
        sets = D.edge_id_sets(c)
        assert sorted(sets) == [1, 17, 16 * D.EDGE_CUS + 17]
        for n, ids in sets.items():
            r64, r32 = forward_refs(c, ids, index_of(whole_sets[shape], ids))
            for t, (v64, p64, tol, amb) in enumerate(bounds(r64, r32)):
                assert float(amb.double().mean()) <= AMBIGUOUS_SHARE, (shape, n, t)
                assert float((torch.relu(r32["pre"][t]).double() - v64).abs().max()) <= tol


# ---- planted mistakes --------------------------------------------------------------------------------------------------------------
GNN_KEYS = lambda R: [k for k in PARAM_KEYS(R) if "label_clf" not in k]      # (the label classifier's path has no gnn weight in it)


def too_close(tag, rows, short):
    """rows: (name, planted, ref64, ref32); a tensor that moved by less than ten tolerances goes into `short`"""
    for name, bad, ref64, ref32 in rows:
        tol = D.tolerance(D.rel_err(ref32, ref64))
        moved = D.rel_err(bad, ref64)
        print(f"{tag} {name:32s} moved {moved:.3e}  tolerance {tol:.3e}  x{moved / tol:.1f}")
        if moved < 10 * tol:
            short.append((tag, name, moved, tol))


def planted_everywhere(c, shape, params_bad, grad_refs, whole, what, short):
    """a parameter set with a mistake planted in it, through every reference the GPU tests compare with: the training gradients
    (B = 17 and 1025, masks held), the attribution (n = 17, the rows kept) and the embeddings (n = 17)"""
    for B in (17, 1025):
        ids, lab = c.batch(B)
        r64, r32, _, index = grad_refs[shape, B]
        masks = [(t > 0).double() for t in r64["pre"]]
        bad = D.dense_ref(c.X, ids, lab, index, params_bad, c.alpha, masks=masks)
        rows = [(f"grad {k}", bad["grads"][k], r64["grads"][k], r32["grads"][k]) for k in GNN_KEYS(c.R)]
        rows += [(k, bad[k], r64[k], r32[k]) for k in ("loss", "logits")]
        too_close(f"{shape} {what} B={B}", rows, short)
    ids = A.id_sets(c)["n17"]
    index = index_of(whole, ids)
    r64, r32 = attr_pair(c, ids, index)
    keep, _ = A.kept_rows(r64["pre"], r32["pre"])
    bad = A.attr_ref(c.X, ids, index, params_bad, A.TARGETS[0], torch.float64)
    pick = lambda res, k: res[k][keep] if res[k].shape[0] == len(ids) else res[k][:, keep]
    too_close(f"{shape} {what} attribute", [(k, pick(bad, k), pick(r64, k), pick(r32, k))
                                            for k in ("d_self", "d_agg", "self_contrib", "rel_contrib")], short)
    ids = D.edge_id_sets(c)[17]
    index = index_of(whole, ids)
    e64, e32 = forward_refs(c, ids, index)
    ebad = D.dense_ref(c.X, ids, np.zeros(17, np.int64), index, params_bad, 1.0, torch.float64)
    act = lambda res: torch.cat([torch.relu(p) for p in res["pre"]], dim=1)
    too_close(f"{shape} {what} embed", [("h | emb", act(ebad), act(e64), act(e32)), ("logits", ebad["logits"], e64["logits"], e32["logits"])], short)


def test_relation_eight_ignored_is_ten_tolerances_away(cases, grad_refs, whole_sets):
    """the last relation's weight matrix replaced by zeros (its h_8 never computed) and by relation 1's (a relation index that
    wraps), at R = 8"""
    short = []
    for shape in [(17, 32, 8), (32, 64, 8)]:
        c = cases[shape]
        for what, value in (("W_8 = 0", lambda p: torch.zeros_like(p["inter1.intra_agg8.weight"])),
                            ("W_8 = W_1", lambda p: p["inter1.intra_agg1.weight"].clone())):
            bad = c.params()
            bad["inter1.intra_agg8.weight"] = value(bad)
            planted_everywhere(c, shape, bad, grad_refs, whole_sets[shape], what, short)
    assert not short, short


def test_output_columns_beyond_256_zero_is_ten_tolerances_away(cases, grad_refs, whole_sets):
    """E = 272: the seventeenth column tile of h_1 and of `combined` left at zero (a wave loop that takes one turn only)"""
    shape = (16, 272, 1)
    c = cases[shape]
    bad = c.params()
    for k in ("inter1.weight", "inter1.intra_agg1.weight"):
        bad[k][:, 256:] = 0.0
    short = []
    planted_everywhere(c, shape, bad, grad_refs, whole_sets[shape], "columns 256 .. 271 zero", short)
    assert not short, short


def test_feature_columns_beyond_256_left_out_is_ten_tolerances_away(cases, whole_sets):
    """F = 260: a neighbour's dot product over its first 256 features only (a lane's second float4 chunk dropped) - through
    attribute(neighbours=True) and on a random d_agg (ops.neighbour_contrib)"""
    shape = (260, 16, 1)
    c = cases[shape]
    ids = A.hub_ids(c)
    index = index_of(whole_sets[shape], ids)
    r64, r32 = attr_pair(c, ids, index)
    keep, _ = A.kept_rows(r64["pre"], r32["pre"])
    rows, cols, cnt = index[0]
    ekeep = keep[rows]
    X = torch.from_numpy(c.X).double()
    sums = lambda v: torch.zeros(len(ids), dtype=torch.float64).index_add_(0, rows, v.double())[keep]
    cut = (X[cols, :256] * r64["d_agg"][0][rows, :256]).sum(1) / cnt[rows]
    short = []
    too_close(f"{shape} attribute", [("neigh_contrib", cut[ekeep], r64["neigh_contrib"][ekeep], r32["neigh_contrib"][ekeep]),
                                     ("neigh row sums", sums(cut), r64["rel_contrib"][0][keep], sums(r32["neigh_contrib"]))], short)
    d = torch.randn(1, len(ids), c.f, generator=torch.Generator().manual_seed(3))
    ref = {t: (X.to(t)[cols] * d.to(t)[0][rows]).sum(1) / cnt.to(t)[rows] for t in (torch.float64, torch.float32)}
    cut = (X[cols, :256] * d.double()[0][rows, :256]).sum(1) / cnt[rows]
    too_close(f"{shape} random d_agg", [("neigh_contrib", cut, ref[torch.float64], ref[torch.float32])], short)
    assert not short, short
