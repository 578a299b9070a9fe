"""Host-side checks of the embedding and nearest-example entry points (pcg_embed_set, pcg_embed_new, pcg_topk_similar,
pcg_topk_similar_workspace_bytes): exported and prototyped, the ABI version and struct list unchanged, every documented argument
rejection returned before any launch (there is no GPU here: a call that got as far as a launch could not return these codes
for these reasons), the workspace size function's shape."""
import ctypes as C

import pytest

from pcgnn_amd import _lib

NEW = ("pcg_embed_set", "pcg_embed_new", "pcg_topk_similar", "pcg_topk_similar_workspace_bytes")
E_ARG, E_UNS = _lib.PCG_E_ARG, _lib.PCG_E_UNSUPPORTED


@pytest.fixture(scope="module")
def lib():
    import pcgnn_amd
    pcgnn_amd.build_library()
    return _lib.load()


def fake(n=64):
    """a host buffer standing in for a device pointer: its address is looked at, never its contents (the calls below are all
    rejected before a launch)"""
    buf = (C.c_char * n)()
    return buf, C.c_void_p((C.addressof(buf) + 15) & ~15)


def desc(ptr, n_nodes=64, n_pos=0):
    g = _lib.GraphDesc(n_nodes=n_nodes, feat_dim=8, feat_stride=8, n_rel=1, n_pos=n_pos, max_degree=4)
    g.X = ptr
    return g


def test_symbols_version_and_structs(lib):
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    assert lib.pcg_abi_version() == 13 and _lib.ABI_VERSION == 13
    assert _lib.ABI_STRUCTS[-1] is _lib.ExplainOut and len(_lib.ABI_STRUCTS) == 6
    # the embed calls are the infer calls plus two outputs
    assert len(_lib.PROTOTYPES["pcg_embed_set"][1]) == len(_lib.PROTOTYPES["pcg_infer_set"][1]) + 2
    assert len(_lib.PROTOTYPES["pcg_embed_new"][1]) == len(_lib.PROTOTYPES["pcg_infer_new"][1]) + 2


def test_embed_set_rejections(lib):
    keep, p = fake()
    g = desc(p)
    thr = (C.c_double * 1)(0.5)
    call = lambda g_, theta, emb, n, outs: lib.pcg_embed_set(g_, theta, emb, p, n, 16, p, thr, p, 100, *outs, p, None)
    one = (None, None, p, None)
    assert call(None, p, 64, 4, one) == E_ARG                           # NULL graph
    assert call(C.byref(g), None, 64, 4, one) == E_ARG                  # NULL theta
    assert call(C.byref(desc(None)), p, 64, 4, one) == E_ARG            # NULL table
    assert call(C.byref(g), p, 64, -1, one) == E_ARG                    # negative n
    # all four outputs NULL: PCG_E_ARG; the same call with any one output gets past the pointer checks (to the shape check,
    # which refuses emb 24 - still before a launch)
    assert call(C.byref(g), p, 24, 4, (None, None, None, None)) == E_ARG
    for i in range(4):
        outs = tuple(p if j == i else None for j in range(4))
        assert call(C.byref(g), p, 24, 4, outs) == E_UNS, i
    assert call(C.byref(g), p, 8, 4, one) == E_UNS                      # emb 8
    # pcg_infer_set still insists on its logits
    assert lib.pcg_infer_set(C.byref(g), p, 24, p, 4, 16, p, thr, p, 100, None, p, p, None) == E_ARG
    assert lib.pcg_infer_set(C.byref(g), p, 24, p, 4, 16, p, thr, p, 100, p, None, p, None) == E_UNS


def test_embed_new_rejections(lib):
    keep, p = fake()
    g, q = desc(p), desc(p, n_nodes=5)
    thr = (C.c_double * 1)(0.5)
    call = lambda g_, q_, theta, emb, n, outs: lib.pcg_embed_new(g_, q_, theta, emb, p, n, 16, p, 1, thr, p, 100, *outs, p, None)
    one = (None, None, p, None)
    assert call(None, C.byref(q), p, 64, 4, one) == E_ARG               # NULL graph
    assert call(C.byref(g), None, p, 64, 4, one) == E_ARG               # NULL query
    assert call(C.byref(g), C.byref(q), None, 64, 4, one) == E_ARG      # NULL theta
    assert call(C.byref(g), C.byref(q), p, 64, -1, one) == E_ARG        # negative n
    q_bad = desc(p, n_nodes=5)
    q_bad.feat_dim = 9
    assert call(C.byref(g), C.byref(q_bad), p, 64, 4, one) == E_ARG     # tables of different shapes
    assert call(C.byref(g), C.byref(q), p, 24, 4, (None, None, None, None)) == E_ARG
    for i in range(4):
        outs = tuple(p if j == i else None for j in range(4))
        assert call(C.byref(g), C.byref(q), p, 24, 4, outs) == E_UNS, i
    assert call(C.byref(g), C.byref(q), p, 8, 4, one) == E_UNS


def test_topk_similar_rejections(lib):
    keep, p = fake()
    call = lambda n, M, emb, k, metric=1, q_ids=None, bank_ids=None: lib.pcg_topk_similar(p, n, p, M, emb, k, metric, q_ids, bank_ids,
                                                                                       p, p, p, p, None)
    assert call(4, 9, 64, 0) == E_ARG and call(4, 9, 64, 65) == E_ARG and call(4, 9, 64, -3) == E_ARG
    assert call(4, 9, 8, 5) == E_UNS and call(4, 9, 24, 5) == E_UNS and call(4, 9, 528, 5) == E_UNS and call(4, 9, 0, 5) == E_UNS
    assert call(-1, 9, 64, 5) == E_ARG and call(4, -1, 64, 5) == E_ARG
    assert call(4, 9, 64, 5, 1, p, None) == E_ARG and call(4, 9, 64, 5, 1, None, p) == E_ARG
    assert call(4, 9, 64, 5, 3) == E_ARG and call(4, 9, 64, 5, -1) == E_ARG
    # NULL pointers (n > 0), a misaligned table
    assert lib.pcg_topk_similar(None, 4, p, 9, 64, 5, 1, None, None, p, p, p, p, None) == E_ARG
    assert lib.pcg_topk_similar(p, 4, None, 9, 64, 5, 1, None, None, p, p, p, p, None) == E_ARG
    assert lib.pcg_topk_similar(p, 4, p, 9, 64, 5, 1, None, None, None, p, p, p, None) == E_ARG
    assert lib.pcg_topk_similar(p, 4, p, 9, 64, 5, 1, None, None, p, None, p, p, None) == E_ARG
    assert lib.pcg_topk_similar(p, 4, p, 9, 64, 5, 1, None, None, p, p, None, p, None) == E_ARG
    assert lib.pcg_topk_similar(C.c_void_p(p.value + 4), 4, p, 9, 64, 5, 1, None, None, p, p, p, p, None) == E_ARG
    # n == 0: nothing to do, nothing enqueued (no pointer is looked at)
    assert lib.pcg_topk_similar(None, 0, None, 9, 64, 5, 1, None, None, None, None, None, None, None) == _lib.PCG_OK


def test_topk_workspace_bytes(lib):
    ws = lib.pcg_topk_similar_workspace_bytes
    assert ws(4, 9, 64, 0) == E_ARG and ws(4, 9, 64, 65) == E_ARG
    assert ws(4, 9, 8, 5) == E_UNS and ws(4, 9, 24, 5) == E_UNS
    assert ws(-1, 9, 64, 5) == E_ARG and ws(4, -1, 64, 5) == E_ARG
    assert ws(0, 0, 16, 1) > 0
    ns = [0, 1, 15, 16, 17, 100, 511, 512, 513, 2047, 2048, 2049, 32767, 32768, 32769, 40000, 1 << 20, 3_000_000]
    for k in (1, 5, 64):
        for M in (0, 1, 1000, 100_000):
            sizes = [ws(n, M, 64, k) for n in ns]
            assert all(s > 0 for s in sizes)
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), (k, M, sizes)
        for n in (0, 1, 100, 40000):
            sizes = [ws(n, M, 64, k) for M in ns]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), (k, n, sizes)
    # the norms of both tables fit
    assert ws(1000, 5000, 64, 5) >= 4 * (1000 + 5000)
