"""Host side of the baselines' whole-set call (pcg_baseline_infer, pc-gnn_amd/baseline.py): the workspace size depends on the
chunk and the table's row pitch only, every argument check returns its code before anything is launched (there is no GPU
here), and the five model shapes are read off the classes.  No GPU."""
import ctypes as C

import pytest

from tests import baseline_ref as BR


@pytest.fixture(scope="module")
def L():
    import pcgnn_amd
    from pcgnn_amd import _lib
    pcgnn_amd.build_library()
    return _lib, _lib.load()


class Args:
    """a complete, valid argument set over host memory that no call may touch: every call below breaks exactly one thing"""

    def __init__(self, _lib, lib, F=25, E=64, n_nodes=1000, n_rel=1):
        self._lib, self.lib = _lib, lib
        self.mem = (C.c_byte * 4096)()
        base = (C.addressof(self.mem) + 255) // 256 * 256
        self.ptr = base
        self.g = _lib.GraphDesc(n_nodes=n_nodes, feat_dim=F, feat_stride=(F + 3) // 4 * 4, n_rel=n_rel, n_pos=0, max_degree=9)
        self.g.X = base
        for r in range(n_rel):
            self.g.indptr[r] = base
            self.g.indices[r] = base
        self.m = _lib.BaselineModel(rel=0, norm=0, add_self=0, concat_self=1, emb=E, W_enc=base, W_cls=base)
        self.kw = dict(g=C.byref(self.g), m=C.byref(self.m), ids=base, n=10, chunk=16, ws=base, ws_bytes=None, logits=base, emb=None,
                       agg=None, status=base, stream=None)

    def size(self, chunk=None):
        return self.lib.pcg_baseline_workspace_bytes(C.byref(self.g), C.byref(self.m), self.kw["chunk"] if chunk is None else chunk)

    def call(self, **over):
        kw = dict(self.kw, **over)
        if kw["ws_bytes"] is None:
            kw["ws_bytes"] = max(int(self.size(kw["chunk"])), 0)
        return self.lib.pcg_baseline_infer(kw["g"], kw["m"], kw["ids"], kw["n"], kw["chunk"], kw["ws"], kw["ws_bytes"], kw["logits"],
                                           kw["emb"], kw["agg"], kw["status"], kw["stream"])


def test_prototypes_and_struct(L):
    _lib, lib = L
    assert len(_lib.PROTOTYPES["pcg_baseline_infer"][1]) == 12 and len(_lib.PROTOTYPES["pcg_baseline_workspace_bytes"][1]) == 3
    assert C.sizeof(_lib.BaselineModel) == 40 and _lib.BaselineModel.W_enc.offset == 24 and _lib.BaselineModel.W_cls.offset == 32
    assert lib.pcg_abi_version() == 13 and _lib.ABI_STRUCTS[-1] is _lib.ExplainOut       # additions only


def test_workspace_depends_on_chunk_and_pitch_only(L):
    _lib, lib = L
    a, b = Args(_lib, lib), Args(_lib, lib)
    b.g.max_degree = 1 << 20
    b.g.n_pos = 77
    b.g.n_nodes = 5_000_000                                  # (more rows, more edges: the same chunk costs the same)
    for chunk in (1, 15, 16, 17, 1000, 4096, 1 << 20):
        assert a.size(chunk) == b.size(chunk) > 0
    for emb in (16, 128, 512):                               # nor on the encoder
        b.m.emb = emb
        b.m.concat_self = 0
        assert a.size(4096) == b.size(4096)
    sizes = [a.size(c) for c in range(1, 3000, 7)]
    assert all(x <= y for x, y in zip(sizes, sizes[1:]))     # non-decreasing in chunk_rows
    assert a.size(1 << 20) >= (1 << 20) * a.g.feat_stride * 4
    assert a.size(1) % 256 == 0
    wide = Args(_lib, lib, F=100)
    assert wide.size(4096) > a.size(4096)


def test_every_rejection_returns_its_code(L):
    _lib, lib = L
    a = Args(_lib, lib)
    ARG, UNS = _lib.PCG_E_ARG, _lib.PCG_E_UNSUPPORTED
    for k in ("g", "m", "ids", "ws", "status", "logits"):
        assert a.call(**{k: None}) == ARG, k
    for member in ("W_enc", "W_cls"):
        m = _lib.BaselineModel.from_buffer_copy(a.m)
        setattr(m, member, None)
        assert a.call(m=C.byref(m)) == ARG, member
    g = _lib.GraphDesc.from_buffer_copy(a.g)
    g.X = None
    assert a.call(g=C.byref(g)) == ARG
    g = _lib.GraphDesc.from_buffer_copy(a.g)
    g.X = a.ptr + 4                                          # not 16-byte aligned
    assert a.call(g=C.byref(g)) == ARG
    assert a.call(n=-1) == ARG and a.call(chunk=0) == ARG and a.call(chunk=-5) == ARG
    for rel in (-1, 1, 8, 99):
        m = _lib.BaselineModel.from_buffer_copy(a.m)
        m.rel = rel
        assert a.call(m=C.byref(m)) == ARG, rel
    for norm in (-1, 2):
        m = _lib.BaselineModel.from_buffer_copy(a.m)
        m.norm = norm
        assert a.call(m=C.byref(m)) == ARG, norm
    assert a.call(ws_bytes=a.size() - 1) == ARG and a.call(ws_bytes=0) == ARG
    for emb in (0, 8, 15, 17, 40, -16):
        m = _lib.BaselineModel.from_buffer_copy(a.m)
        m.emb = emb
        assert a.call(m=C.byref(m)) == UNS, emb
        assert lib.pcg_baseline_workspace_bytes(C.byref(a.g), C.byref(m), 16) == UNS
    for stride, feat in ((26, 25), (516, 516), (24, 25), (0, 0)):   # what infer_table_ok rejects
        g = _lib.GraphDesc.from_buffer_copy(a.g)
        g.feat_stride, g.feat_dim = stride, feat
        assert a.call(g=C.byref(g)) == UNS, (stride, feat)
    assert lib.pcg_baseline_workspace_bytes(None, C.byref(a.m), 16) == ARG
    assert lib.pcg_baseline_workspace_bytes(C.byref(a.g), None, 16) == ARG
    assert lib.pcg_baseline_workspace_bytes(C.byref(a.g), C.byref(a.m), 0) == ARG
    # rel inside a multi-relation graph is fine as far as the checks go: the last thing checked is the size
    b = Args(_lib, lib, n_rel=3)
    b.m.rel = 2
    assert b.call(ws_bytes=b.size() - 1) == ARG and b.call(n=0) == _lib.PCG_OK


def test_n_zero_is_ok_and_launches_nothing(L):
    _lib, lib = L
    a = Args(_lib, lib)
    assert a.call(n=0) == _lib.PCG_OK
    assert a.call(n=0, emb=a.ptr, agg=a.ptr) == _lib.PCG_OK
    assert bytes(a.mem) == bytes(4096)                       # (nothing wrote the host memory the pointers name)


@pytest.mark.parametrize("name", sorted(BR.SHAPES))
def test_shapes_are_read_off_the_classes(name):
    from pcgnn_amd import _lib, baseline, graphsage as GS
    model = BR.build_model(GS, {}, 25, 64, name, device=None)
    want = BR.SHAPES[name]
    got = baseline.model_shape(model)
    assert got == dict(add_self=want["add_self"], norm=want["norm"], concat_self=want["concat_self"], emb=64)
    assert (_lib.PCG_NORM_COUNT, _lib.PCG_NORM_SQRT_COUNT) == (BR.NORM_COUNT, BR.NORM_SQRT_COUNT)
    assert tuple(model.enc.weight.shape) == (64, 50 if want["concat_self"] else 25)
    assert model.eval_by_infer is False                      # the default stays the per-batch loop


def test_model_shape_rejects_other_models():
    import torch
    from pcgnn_amd import baseline
    with pytest.raises(TypeError):
        baseline.model_shape(torch.nn.Linear(3, 2))
