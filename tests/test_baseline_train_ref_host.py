"""The training reference of the GraphSAGE / GCN baselines (tests/baseline_train_ref.py) on the CPU: its float64 statement against
torch autograd in float64, and the two conditions the GPU tests (tests/test_gpu_baseline_train.py) rely on, asserted for the
reference alone on every case and batch they use - the ambiguous share of pre-activations within ``dense_ref.AMBIGUOUS_CAP``, the
cancelled share of every Adam step within ``adam_ref.CANCEL_CAP`` - and, for the training steps, that the float32 yardstick's own Adam
keeps ``YARDSTICK_THETA`` of theta's tolerance (no entry where Adam amplifies a rounding of the gradient beyond it)."""
import numpy as np
import pytest

from tests import adam_ref as A
from tests import baseline_ref as BR
from tests import baseline_train_ref as T
from tests import dense_ref as D


def test_the_cases_cover_both_dense_variants_and_every_part_count():
    for F, E, shape in T.CASES:
        assert BR.w_enc_in_lds(F, E, BR.SHAPES[shape]["concat_self"]) == ((F, E) not in T.STREAMED), (F, E, shape)
    assert any((F, E) in T.STREAMED for F, E, _ in T.CASES) and any((F, E) in T.STREAMED for F, E, _ in T.STEP_CASES)
    for F, E in T.FE_ALL:
        assert {s for f, e, s in T.CASES if (f, e) == (F, E)} == set(BR.SHAPES)
    assert [T.kparts(B) for B in (1, 1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097, 100000)] == [1, 1, 2, 2, 3, 3, 4, 4, 4, 4]
    for B in (1024, 2048, 3072):                       # both sides of every threshold, and the sizes the issue names
        assert B in T.BATCHES and B + 1 in T.BATCHES
    assert {1, 15, 16, 17, 1025} <= set(T.BATCHES)


def test_every_batch_holds_the_rows_it_should():
    indptr, indices, _ = T.csr_spec()
    deg = np.diff(indptr)
    assert deg[T.EMPTY_NODE] == 0
    for B, salt in [(B, s) for B in T.BATCHES + (40,) for s in sorted({0} | set(T.SALTS.values()))]:
        ids, labels = T.batch(B, salt)
        assert len(ids) == B and T.EMPTY_NODE not in ids and set(np.unique(labels)) <= {0, 1}
        if B < 15:
            assert deg[ids[0]] == 5000
            continue
        in_row = [v in indices[indptr[v]:indptr[v + 1]] for v in ids[:7]]
        assert (deg[ids] > 512).sum() >= 4 and any(in_row) and not all(in_row) and len(np.unique(ids)) < B
    assert T.EMPTY_NODE in T.nan_batch()[0]
    for case in range(len(T.STEP_CASES)):
        steps = T.step_batches(case)
        assert [len(i) for i, _ in steps] == [B for _, _, B in T.STEPS] and len(steps) == len(A.STEPS) == 12
        assert [B < T.STEP_BATCH for _, _, B in T.STEPS] == [B < A.BATCH for _, _, B in A.STEPS]      # adam_ref.STEPS' pattern
        assert all(T.EMPTY_NODE not in i for i, _ in steps)


@pytest.mark.parametrize("F,E,shape", T.CASES)
def test_float64_statement_against_autograd(F, E, shape):
    W_enc, W_cls = T.model_weights(F, E, shape)
    for B in (1, 17, 1025):
        ids, labels = T.batch(B)
        r = T.loss_and_grad(F, shape, ids, labels, W_enc, W_cls)
        loss, d_enc, d_cls = T.autograd_f64(F, shape, ids, labels, W_enc, W_cls)
        # (a row's term is lse - logit: its absolute error is an ulp of the logits, whatever is left after the subtraction)
        np.testing.assert_allclose(r["loss"], loss, rtol=1e-12, atol=1e-14 * np.abs(r["logits"]).max())
        np.testing.assert_allclose(r["d_enc"], d_enc, rtol=0, atol=1e-12 * np.abs(d_enc).max())
        np.testing.assert_allclose(r["d_cls"], d_cls, rtol=0, atol=1e-12 * np.abs(d_cls).max())
        # the masked statement with the float64 sign as the mask is the same function
        m = T.loss_and_grad(F, shape, ids, labels, W_enc, W_cls, mask=(r["pre"] > 0).astype(np.float64))
        for k in ("loss", "d_enc", "d_cls", "logits"):
            np.testing.assert_array_equal(m[k], r[k])
        # and its unmasked logits are baseline_ref.forward's
        s = BR.SHAPES[shape]
        fw = BR.forward(T.features(F), T.csr(), ids, W_enc, W_cls, **s)[0]
        np.testing.assert_allclose(r["logits"], fw, rtol=0, atol=1e-12 * np.abs(fw).max())


def test_nan_goes_through_as_in_autograd():
    F, E = 25, 64
    ids, labels = T.nan_batch()
    for shape, finite in (("sage", False), ("sage_concat", False), ("gcn", True)):
        W_enc, W_cls = T.model_weights(F, E, shape)
        r = T.loss_and_grad(F, shape, ids, labels, W_enc, W_cls)
        loss, d_enc, d_cls = T.autograd_f64(F, shape, ids, labels, W_enc, W_cls)
        assert bool(np.isfinite(loss)) == finite
        for mine, theirs in ((r["loss"], loss), (r["d_enc"], d_enc), (r["d_cls"], d_cls)):
            assert np.array_equal(np.isnan(mine), np.isnan(theirs))


@pytest.mark.parametrize("F,E,shape", T.CASES)
def test_the_gradient_batches_keep_the_ambiguous_cap(F, E, shape):
    W_enc, W_cls = T.model_weights(F, E, shape)
    for B in T.BATCHES:
        ids, labels = T.batch(B, T.salt_of(F, E, shape))
        _, _, share, wrong = T.reference_pair(F, shape, ids, labels, W_enc, W_cls)
        assert share <= D.AMBIGUOUS_CAP and wrong == 0, (B, share)


@pytest.mark.parametrize("case", range(len(T.STEP_CASES)))
def test_the_training_steps_keep_both_caps(case):
    F, E, shape = T.STEP_CASES[case]
    W_enc, W_cls = T.model_weights(F, E, shape)
    seen = 0
    for k, _, share, out, _, yard in T.adam_steps_f64(F, shape, T.step_batches(case), W_enc, W_cls):
        assert share <= D.AMBIGUOUS_CAP, (k, share)
        assert out <= A.CANCEL_CAP, (k, out)
        # no entry where Adam turns a float32 rounding of the gradient into a move of theta (T.WARM_V)
        assert yard["theta"] <= T.YARDSTICK_THETA and yard["m"] <= 1 and yard["v"] <= 1, (k, yard)
        seen += 1
    assert seen == 12
