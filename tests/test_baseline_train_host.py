"""Host side of the baselines' training call (pcg_baseline_train, pc-gnn_amd/baseline.py): the new exports are in the header, the
binding and the built library, the ABI version is what it was, every argument check returns its code before anything is launched
(there is no GPU here), and the workspace is a function of the batch size and the shapes only.  No GPU."""
import ctypes as C
import os
import re

import pytest

NEW = ("pcg_baseline_train_workspace_bytes", "pcg_baseline_train")


@pytest.fixture(scope="module")
def L():
    import pcgnn_amd
    from pcgnn_amd import _lib
    pcgnn_amd.build_library()
    return _lib, _lib.load()


class Args:
    """a complete, valid argument set over host memory that no call may touch: every call below breaks exactly one thing"""

    def __init__(self, _lib, lib, F=25, E=64, n_nodes=1000, concat_self=1):
        self._lib, self.lib = _lib, lib
        self.mem = (C.c_byte * 4096)()
        base = (C.addressof(self.mem) + 255) // 256 * 256
        self.ptr = base
        self.g = _lib.GraphDesc(n_nodes=n_nodes, feat_dim=F, feat_stride=(F + 3) // 4 * 4, n_rel=1, n_pos=0, max_degree=9)
        self.g.X = base
        self.g.indptr[0] = base
        self.g.indices[0] = base
        self.m = _lib.BaselineModel(rel=0, norm=0, add_self=0, concat_self=concat_self, emb=E, W_enc=base, W_cls=base)
        self.opt = _lib.BaselineOpt(m_enc=base, v_enc=base, m_cls=base, v_cls=base, first_step=1, apply=1,
                                    hyper=_lib.AdamHyper(0.01, 0.9, 0.999, 1e-8, 0.001))
        self.kw = dict(g=C.byref(self.g), m=C.byref(self.m), opt=C.byref(self.opt), ids=base, labels=base, n=40, batch=16, ws=base,
                       ws_bytes=None, loss=base, grad=None, status=base, stream=None)

    def size(self, batch=None):
        return self.lib.pcg_baseline_train_workspace_bytes(C.byref(self.g), C.byref(self.m), self.kw["batch"] if batch is None else batch)

    def call(self, **over):
        kw = dict(self.kw, **over)
        if kw["ws_bytes"] is None:
            kw["ws_bytes"] = max(int(self.size(kw["batch"])), 0)
        return self.lib.pcg_baseline_train(kw["g"], kw["m"], kw["opt"], kw["ids"], kw["labels"], kw["n"], kw["batch"], kw["ws"],
                                           kw["ws_bytes"], kw["loss"], kw["grad"], kw["status"], kw["stream"])

    def opt_with(self, **members):
        o = self._lib.BaselineOpt.from_buffer_copy(self.opt)
        for k, v in members.items():
            setattr(o, k, v)
        return C.byref(o)


def test_exports_header_binding_and_library(L):
    _lib, lib = L
    here = os.path.dirname(os.path.abspath(__file__))
    header = open(os.path.join(here, "..", "include", "pcgnn.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) <= 16
        assert getattr(lib, name) is not None
    assert "typedef struct pcg_baseline_opt" in header
    assert len(_lib.PROTOTYPES["pcg_baseline_train"][1]) == 13 and len(_lib.PROTOTYPES["pcg_baseline_train_workspace_bytes"][1]) == 3
    assert lib.pcg_abi_version() == _lib.ABI_VERSION == 13 and _lib.ABI_STRUCTS[-1] is _lib.ExplainOut and len(_lib.ABI_STRUCTS) == 6
    O = _lib.BaselineOpt
    assert (O.m_enc.offset, O.v_enc.offset, O.m_cls.offset, O.v_cls.offset, O.first_step.offset, O.apply.offset, O.hyper.offset) == \
        (0, 8, 16, 24, 32, 40, 48) and C.sizeof(O) == 88


def test_every_rejection_returns_its_code(L):
    _lib, lib = L
    a = Args(_lib, lib)
    ARG, UNS = _lib.PCG_E_ARG, _lib.PCG_E_UNSUPPORTED
    for k in ("g", "m", "opt", "ids", "labels", "ws", "status", "loss"):
        assert a.call(**{k: None}) == ARG, k
    for member in ("W_enc", "W_cls"):
        m = _lib.BaselineModel.from_buffer_copy(a.m)
        setattr(m, member, None)
        assert a.call(m=C.byref(m)) == ARG, member
    assert a.call(n=-1) == ARG and a.call(batch=0) == ARG and a.call(batch=-5) == ARG
    # apply == 1: the state pointers and a 1-based step
    for member in ("m_enc", "v_enc", "m_cls", "v_cls"):
        assert a.call(opt=a.opt_with(**{member: None})) == ARG, member
    assert a.call(opt=a.opt_with(first_step=0)) == ARG and a.call(opt=a.opt_with(first_step=-3)) == ARG
    # apply == 0: one batch and somewhere to put its gradient; the state is not looked at
    grads_only = dict(apply=0, m_enc=None, v_enc=None, m_cls=None, v_cls=None, first_step=0)
    assert a.call(opt=a.opt_with(**grads_only), n=17, batch=16, grad=a.ptr) == ARG
    assert a.call(opt=a.opt_with(**grads_only), n=16, batch=16, grad=None) == ARG
    assert a.call(opt=a.opt_with(**grads_only), n=0, batch=16, grad=a.ptr) == _lib.PCG_OK
    assert a.call(ws_bytes=a.size() - 1) == ARG and a.call(ws_bytes=0) == ARG
    assert a.call(ws=a.ptr + 4) == ARG                        # not 16-byte aligned
    for emb in (0, 8, 15, 17, 40, -16):                      # E % 16 != 0
        m = _lib.BaselineModel.from_buffer_copy(a.m)
        m.emb = emb
        assert a.call(m=C.byref(m)) == UNS, emb
        assert lib.pcg_baseline_train_workspace_bytes(C.byref(a.g), C.byref(m), 16) == UNS
    for stride, feat in ((26, 25), (516, 516), (24, 25), (0, 0)):
        g = _lib.GraphDesc.from_buffer_copy(a.g)
        g.feat_stride, g.feat_dim = stride, feat
        assert a.call(g=C.byref(g)) == UNS, (stride, feat)
    assert lib.pcg_baseline_train_workspace_bytes(None, C.byref(a.m), 16) == ARG
    assert lib.pcg_baseline_train_workspace_bytes(C.byref(a.g), None, 16) == ARG
    assert lib.pcg_baseline_train_workspace_bytes(C.byref(a.g), C.byref(a.m), 0) == ARG
    assert a.call(n=0) == _lib.PCG_OK
    assert bytes(a.mem) == bytes(4096)                       # (nothing wrote the host memory the pointers name)


def test_workspace_is_monotone_in_the_batch_and_knows_no_edges(L):
    _lib, lib = L
    a, b = Args(_lib, lib), Args(_lib, lib)
    b.g.max_degree = 1 << 20
    b.g.n_pos = 77
    b.g.n_nodes = 5_000_000                                  # (more rows, more edges: the same batch costs the same)
    for batch in (1, 15, 16, 17, 1024, 1025, 4096, 4097, 1 << 20):
        assert a.size(batch) == b.size(batch) > 0
        assert a.size(batch) % 256 == 0
        assert a.size(batch) > lib.pcg_baseline_workspace_bytes(C.byref(a.g), C.byref(a.m), batch)    # inference's parts and more
    sizes = [a.size(c) for c in range(1, 5000, 7)]
    assert all(x <= y for x, y in zip(sizes, sizes[1:]))
    # the activations: (K + 2 E + 2) rows of the batch rounded up to 16 - and it grows with the model's shape
    K, E = 50, 64
    assert a.size(1 << 16) >= 4 * (K + 2 * E + 2) * (1 << 16)
    wide, gcn = Args(_lib, lib, E=128), Args(_lib, lib, concat_self=0)
    assert wide.size(4096) > a.size(4096) > gcn.size(4096)
