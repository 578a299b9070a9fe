"""CPU-only tests of the custom-loss entry point and of its reference: pcg_dense_vjp is exported with a prototype, rejects NULL
structs and members before any launch (there is no device here), accepts an empty batch, and leaves the ABI version alone;
tests/vjp_ref.py with the built-in loss is tests/dense_ref.py exactly, and the cases the GPU test runs keep the ReLU-kink cap."""
import ctypes as C

import pytest
import torch

from tests import dense_ref as D
from tests import vjp_ref as V
from tests.util import PARAM_KEYS


@pytest.fixture(scope="module")
def lib():
    import pcgnn_amd
    from pcgnn_amd import _lib
    pcgnn_amd.build_library()
    return _lib.load()


def structs(B=4, members=False):
    """(g, st, sel, batch, out, seeds); members: theta / acts / ids point at host arrays (never read: no launch happens here)"""
    from pcgnn_amd import _lib
    g = _lib.GraphDesc(n_nodes=64, feat_dim=8, feat_stride=8, n_rel=1, n_pos=0, max_degree=4)     # every pointer NULL
    thr = (C.c_double * 1)(0.5)
    buf = (C.c_float * 64)()
    at = C.cast(buf, C.c_void_p)
    hyper = _lib.AdamHyper(0.01, 0.9, 0.999, 1e-8, 0.0)
    st = _lib.TrainState(emb=64, act_ld=16, lambda_1=2.0, hyper=hyper)
    b = _lib.Batch(None, None, None, None, B, 0.25)
    if members:
        st.theta, st.acts, b.ids = at, at, at
    sel = _lib.SelectWs(thr, thr, None, None, 100, 0)
    return g, st, sel, b, _lib.DenseOut(), at, (thr, buf)


def test_entry_point_is_exported_with_a_prototype(lib):
    from pcgnn_amd import _lib
    assert hasattr(lib, "pcg_dense_vjp")
    res, args = _lib.PROTOTYPES["pcg_dense_vjp"]
    assert res is C.c_int and len(args) == 10 <= 16
    assert lib.pcg_abi_version() == _lib.ABI_VERSION == 13
    assert _lib.ABI_STRUCTS[-1] is _lib.ExplainOut          # no new parameter struct


def test_rejects_null_structs_and_members(lib):
    from pcgnn_amd import _lib
    g, st, sel, b, out, at, _keep = structs(members=True)
    N = None
    full = dict(g=g, st=st, b=b, sel=sel, dl=at, dc=at)
    call = lambda a: lib.pcg_dense_vjp(a["g"], a["st"], a["b"], N, 8, a["sel"], a["dl"], a["dc"], out, N)
    assert call(dict.fromkeys(full)) == _lib.PCG_E_ARG, "NULL struct pointers"
    for k in full:                                           # each one alone
        assert call({**full, k: N}) == _lib.PCG_E_ARG, f"NULL {k}"
    # structs with NULL members
    g0, st0, sel0, b0, _, _, _keep0 = structs()
    assert call({**full, "st": st0, "b": b0}) == _lib.PCG_E_ARG, "every member NULL"
    for member in ("theta", "acts"):
        _, st1, _, _, _, _, _keep1 = structs(members=True)
        setattr(st1, member, N)
        assert call({**full, "st": st1}) == _lib.PCG_E_ARG, f"NULL st->{member}"
    assert call({**full, "b": b0}) == _lib.PCG_E_ARG, "NULL ids with B >= 1"
    _, _, _, bneg, _, _, _keep2 = structs(B=-1, members=True)
    assert call({**full, "b": bneg}) == _lib.PCG_E_ARG, "B < 0"
    # with every required member given the call gets as far as pcg_train_dense(adam_clf = 4)'s own checks (X, agg: NULL here)
    assert call(full) == _lib.PCG_E_ARG


def test_empty_batch_is_ok_and_enqueues_nothing(lib):
    from pcgnn_amd import _lib
    g, st, sel, b, out, at, _keep = structs(B=0, members=True)
    assert lib.pcg_dense_vjp(g, st, b, None, 8, sel, at, at, out, None) == _lib.PCG_OK
    assert lib.pcg_dense_vjp(g, st, b, None, 8, sel, at, at, None, None) == _lib.PCG_OK      # out may be NULL
    b.ids = None                                              # (ids are required only with B >= 1)
    assert lib.pcg_dense_vjp(g, st, b, None, 8, sel, at, at, out, None) == _lib.PCG_OK


@pytest.fixture(scope="module")
def host_cases():
    """(shape, B) -> (case, ids, labels, index of the oracle's sets), for exactly the pairs the GPU test runs"""
    out = {}
    for shape in V.SHAPES:
        c = D.GradCase.of(shape)
        for B in V.BATCHES:
            ids, lab = c.batch(B)
            out[shape, B] = (c, ids, lab, D.sets_to_index(c.host_sets(ids, lab)))
    return out


def test_builtin_loss_is_dense_ref_exactly(host_cases):
    """float64, plain and masked: loss, logits and every parameter's gradient are dense_ref's, bit for bit"""
    for (shape, B), (c, ids, lab, index) in host_cases.items():
        if B == 1025 and shape != (32, 64, 3):
            continue
        want = D.dense_ref(c.X, ids, lab, index, c.params(), c.alpha)
        got = V.vjp_ref(c.X, ids, lab, index, c.params(), V.builtin_loss(c.alpha))
        masks = [(t > 0).double() for t in want["pre"]]
        want_m = D.dense_ref(c.X, ids, lab, index, c.params(), c.alpha, masks=masks)
        got_m = V.vjp_ref(c.X, ids, lab, index, c.params(), V.builtin_loss(c.alpha), masks=masks)
        for w, g in ((want, got), (want_m, got_m)):
            assert torch.equal(w["loss"], g["loss"]) and torch.equal(w["logits"], g["logits"]) and torch.equal(w["center"], g["center"])
            for k in PARAM_KEYS(c.R):
                assert torch.equal(w["grads"][k], g["grads"][k]), (shape, B, k)


def test_a_loss_of_the_gnn_logits_leaves_the_label_classifier_alone(host_cases):
    c, ids, lab, index = host_cases[(10, 16, 1), 17]
    got = V.vjp_ref(c.X, ids, lab, index, c.params(), V.gnn_only_loss())
    assert not got["grads"]["inter1.label_clf.weight"].any() and not got["grads"]["inter1.label_clf.bias"].any()
    assert got["grads"]["weight"].abs().max() > 0


def test_gpu_cases_keep_the_ambiguous_cap(host_cases):
    over = {}
    for (shape, B), (c, ids, lab, index) in host_cases.items():
        share = V.reference_pair(c, ids, lab, index, V.focal_loss(c.alpha))[2]
        if share > D.AMBIGUOUS_CAP:
            over[shape, B] = share
    assert not over, f"ambiguous ReLU pre-activations above {D.AMBIGUOUS_CAP}: {over}"
