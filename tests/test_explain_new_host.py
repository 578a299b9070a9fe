"""The host side of pcg_explain_new (FusedPCGNN.chosen_new / attribute_new): the exports and their ctypes prototypes, ABI 13,
the layout of pcg_explain_out, the arguments the entry point rejects before any launch, its workspace size, and the host
arithmetic of the output offsets.  Host-only descriptors and dummy addresses that are never dereferenced: nothing here needs a
GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.test_infer_workspace_host import PAIRS
from tests.test_query_batch_host import host_desc

EMB = 64
ATTR = ("logits", "d_self", "d_agg", "self_contrib", "rel_contrib")
CHOSEN = ("out_begin", "out_ids", "out_dist")


def test_exports_prototypes_and_abi_version():
    from pcgnn_amd import _lib
    lib = _lib.load()
    for name in ("pcg_explain_new", "pcg_explain_new_workspace_bytes"):
        assert hasattr(lib, name), f"libpcgnn_hip.so does not export {name}"
        assert name in _lib.PROTOTYPES, f"ctypes prototype missing for {name}"
    assert lib.pcg_abi_version() == 13 and _lib.ABI_VERSION == 13
    assert len(_lib.PROTOTYPES["pcg_explain_new"][1]) == 17
    assert _lib.PROTOTYPES["pcg_explain_new_workspace_bytes"] == _lib.PROTOTYPES["pcg_infer_new_workspace_bytes"]


def test_explain_out_layout_is_the_mirrors():
    from pcgnn_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_STRUCTS[-1] is _lib.ExplainOut                    # appended last: the older structs keep their numbers
    assert [n for n, _ in _lib.ExplainOut._fields_] == list(ATTR + CHOSEN + ("neigh_contrib",))
    out = (C.c_int64 * 64)()
    which = len(_lib.ABI_STRUCTS) - 1
    n = lib.pcg_abi_layout(which, out, 64)
    assert n == 1 + len(_lib.ExplainOut._fields_)
    assert out[0] == C.sizeof(_lib.ExplainOut)
    for i, (name, _) in enumerate(_lib.ExplainOut._fields_):
        assert out[1 + i] == getattr(_lib.ExplainOut, name).offset, name
    assert lib.pcg_abi_layout(which + 1, out, 64) == _lib.PCG_E_ARG


def explain_out(*groups, neigh=False):
    """a pcg_explain_out whose named members hold a dummy non-NULL address (a rejected call dereferences none)"""
    from pcgnn_amd import _lib
    o = _lib.ExplainOut()
    for name in groups:
        setattr(o, name, 0x1000)
    if neigh:
        o.neigh_contrib = 0x1000
    return o


def test_rejected_before_any_launch():
    from pcgnn_amd import _lib
    lib = _lib.load()
    thr = (C.c_double * 3)(0.5, 0.5, 0.5)
    g, q = host_desc(1000), host_desc(10)
    gp, qp = C.byref(g), C.byref(q)

    def call(out, g=gp, q=qp, w=(0.0, 1.0), n=4):
        o = None if out is None else C.byref(out)
        return lib.pcg_explain_new(g, q, None, EMB, None, n, 4, None, 1, thr, None, 100, w[0], w[1], o, None, None)

    both = explain_out(*ATTR, *CHOSEN, neigh=True)
    # (what an accepted struct meets next: the NULL table / theta / ids of these host-only descriptors - still no launch)
    assert call(both) == _lib.PCG_E_ARG
    assert call(None) == _lib.PCG_E_ARG                               # NULL struct
    assert call(explain_out()) == _lib.PCG_E_ARG                      # no group requested
    assert call(explain_out(), n=0) == _lib.PCG_E_ARG                 # ... whatever n
    for k in range(1, len(ATTR)):                                     # a half-filled attribution group
        assert call(explain_out(*ATTR[:k]), n=0) == _lib.PCG_E_ARG, ATTR[:k]
        assert call(explain_out(*ATTR[k:], *CHOSEN), n=0) == _lib.PCG_E_ARG, ATTR[k:]
    for k in range(1, len(CHOSEN)):                                   # a half-filled chosen group
        assert call(explain_out(*CHOSEN[:k]), n=0) == _lib.PCG_E_ARG, CHOSEN[:k]
        assert call(explain_out(*ATTR, *CHOSEN[k:]), n=0) == _lib.PCG_E_ARG, CHOSEN[k:]
    # neigh_contrib needs both other groups
    assert call(explain_out(neigh=True), n=0) == _lib.PCG_E_ARG
    assert call(explain_out(*ATTR, neigh=True), n=0) == _lib.PCG_E_ARG
    assert call(explain_out(*CHOSEN, neigh=True), n=0) == _lib.PCG_E_ARG
    # every complete request is accepted (n == 0: nothing is enqueued, PCG_OK)
    for ok in (both, explain_out(*ATTR), explain_out(*CHOSEN), explain_out(*ATTR, *CHOSEN)):
        assert call(ok, n=0) == _lib.PCG_OK
    # a non-finite weight
    for w in ((math.nan, 1.0), (0.0, math.inf), (-math.inf, 0.0)):
        assert call(both, w=w, n=0) == _lib.PCG_E_ARG, w
    assert call(both, n=-1) == _lib.PCG_E_ARG
    # descriptors that disagree on feat_dim / n_rel (and the rest of pcg_infer_new's descriptor checks)
    assert call(both, g=None, n=0) == _lib.PCG_E_ARG and call(both, q=None, n=0) == _lib.PCG_E_ARG
    assert call(both, q=C.byref(host_desc(10, feat_dim=25)), n=0) == _lib.PCG_E_ARG
    assert call(both, q=C.byref(host_desc(10, n_rel=2)), n=0) == _lib.PCG_E_ARG
    assert call(both, q=C.byref(host_desc(10, feat_stride=64)), n=0) == _lib.PCG_E_ARG
    qpos = host_desc(10)
    qpos.n_pos = 3
    assert call(both, q=C.byref(qpos), n=0) == _lib.PCG_E_ARG
    # the shapes the attribution's dense launch has no room for are UNSUPPORTED, as pcg_attr_set's
    assert lib.pcg_explain_new(gp, qp, None, 60, None, 0, 4, None, 1, thr, None, 100, 0.0, 1.0, C.byref(both), None, None) == \
        _lib.PCG_E_UNSUPPORTED


@pytest.mark.parametrize("R", (1, 3))
@pytest.mark.parametrize("F", (25, 32))
def test_workspace_is_infer_news(R, F):
    from pcgnn_amd import _lib
    lib = _lib.load()
    g, q = host_desc(100000, feat_dim=F, n_rel=R, max_degree=5000), host_desc(1000, feat_dim=F, n_rel=R, max_degree=300)
    for chunk, cap in PAIRS + ((0, 100), (16, 0), (16, 1 << 31)):
        want = lib.pcg_infer_new_workspace_bytes(C.byref(g), C.byref(q), EMB, chunk, cap)
        assert lib.pcg_explain_new_workspace_bytes(C.byref(g), C.byref(q), EMB, chunk, cap) == want
    assert lib.pcg_explain_new_workspace_bytes(C.byref(g), C.byref(q), EMB, 16, 100) > 0
    assert lib.pcg_explain_new_workspace_bytes(None, C.byref(q), EMB, 16, 100) == _lib.PCG_E_ARG
    assert lib.pcg_explain_new_workspace_bytes(C.byref(g), C.byref(host_desc(1000, feat_dim=F + 4, n_rel=R)), EMB, 16, 100) == \
        _lib.PCG_E_ARG
    assert lib.pcg_explain_new_workspace_bytes(C.byref(g), C.byref(q), 60, 16, 100) == _lib.PCG_E_UNSUPPORTED


@pytest.mark.parametrize("thr", (0.2, 0.5, 1.0))
def test_host_offsets_follow_the_per_row_rule(thr):
    """the output offsets chosen_new forms - ops.sel_capacity / ops.rank_offsets over the QUERY's degrees - against the rule
    spelled out row by row: a test-mode row keeps deg > k + 1 ? k : deg entries, k = ceil(deg * threshold)"""
    from pcgnn_amd import _lib, ops
    from pcgnn_amd.graph import BaseShape, QueryBatch
    lib = _lib.load()
    N, R = 50, 2
    rs = np.random.RandomState(3)
    degs = [0, 1, 2, 3, 4, 5, 16, 17, 33, 40]
    nq = len(degs)
    csr = []
    for r in range(R):
        rows = [rs.choice(N + nq, size=d if r == 0 else max(d - 1, 0), replace=False) for d in degs]
        rows[3] = np.concatenate([rows[3], rows[3]])                    # duplicates are dropped before anything is counted
        ip = np.zeros(nq + 1, np.int64)
        np.cumsum([len(x) for x in rows], out=ip[1:])
        csr.append((ip, np.concatenate(rows)))
    q = QueryBatch(rs.randn(nq, 8).astype(np.float32), csr, BaseShape(N, 8, R))
    assert q.deg_host[0].tolist() == degs
    ids = np.array([9, 0, 3, 3, 7, 1, 2, 4, 5, 6, 8, 9], dtype=np.int64)
    caps = ops.sel_capacity(q, ids, None, [thr] * R, 0.0, False)
    assert caps.shape == (R, len(ids))
    off = ops.rank_offsets(caps)
    want = [0]
    for r in range(R):
        for j in ids:
            deg = int(q.deg_host[r][j])
            k = math.ceil(deg * thr)
            kept = k if deg > k + 1 else deg
            assert kept == lib.pcg_sel_capacity_row(deg, thr, 0.0, 0, 0, 0)
            want.append(want[-1] + kept)
    assert off.dtype == np.int64 and off.tolist() == want
