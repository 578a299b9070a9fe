"""The workspace sizes of the whole-set calls (pcg_infer_workspace_bytes, pcg_infer_dist_workspace_bytes,
pcg_chosen_workspace_bytes, pcg_infer_new_workspace_bytes) as sums of the parts their one layout has - two plan slots (the
partitioned chunk: one), the data part, and agg / cnt / centre logits (the chosen call: cnt only) - and the arguments they
reject.  Host-only descriptors: nothing here needs a GPU."""
import ctypes as C

import pytest

from tests.test_query_batch_host import host_desc

EMB = 64
PAIRS = ((1, 1), (17, 900), (1000, 250000), (16384, 1 << 22))


def a(x):
    return (x + 255) // 256 * 256


@pytest.mark.parametrize("R", (1, 3))
@pytest.mark.parametrize("F", (25, 32))
def test_sizes_are_the_sums_of_their_parts(R, F):
    from pcgnn_amd import _lib
    lib = _lib.load()
    g, q = host_desc(100000, feat_dim=F, n_rel=R, max_degree=5000), host_desc(1000, feat_dim=F, n_rel=R, max_degree=300)
    for d in (g, q):
        for chunk, cap in PAIRS:
            P = lib.pcg_choose_plan_bytes(C.byref(d), chunk, cap)
            D = lib.pcg_choose_data_bytes(C.byref(d), chunk, cap)
            assert P > 0 and D > 0 and P % 256 == 0
            whole = 2 * P + a(D) + a(4 * R * chunk * F) + a(4 * R * chunk) + a(8 * chunk)
            assert lib.pcg_infer_workspace_bytes(C.byref(d), EMB, chunk, cap) == whole
            assert lib.pcg_infer_dist_workspace_bytes(C.byref(d), EMB, chunk, cap) == whole - P
            assert lib.pcg_chosen_workspace_bytes(C.byref(d), chunk, cap) == 2 * P + a(D) + a(4 * R * chunk)
    for chunk, cap in PAIRS:             # the query's rows are what is planned: its descriptor sizes the workspace
        assert lib.pcg_infer_new_workspace_bytes(C.byref(g), C.byref(q), EMB, chunk, cap) == \
            lib.pcg_infer_workspace_bytes(C.byref(q), EMB, chunk, cap)


def test_rejected_arguments():
    from pcgnn_amd import _lib
    lib = _lib.load()
    g, q = host_desc(100000), host_desc(1000)
    sizes = {
        "infer": lambda d, emb, chunk, cap: lib.pcg_infer_workspace_bytes(d, emb, chunk, cap),
        "dist": lambda d, emb, chunk, cap: lib.pcg_infer_dist_workspace_bytes(d, emb, chunk, cap),
        "chosen": lambda d, emb, chunk, cap: lib.pcg_chosen_workspace_bytes(d, chunk, cap),
        "new": lambda d, emb, chunk, cap: lib.pcg_infer_new_workspace_bytes(C.byref(g), d, emb, chunk, cap),
    }
    for name, size in sizes.items():
        assert size(C.byref(q), EMB, 16, 100) > 0, name
        assert size(None, EMB, 16, 100) == _lib.PCG_E_ARG, name
        assert size(C.byref(q), EMB, 0, 100) == _lib.PCG_E_ARG, name
        assert size(C.byref(q), EMB, 16, 0) == _lib.PCG_E_ARG, name
        assert size(C.byref(q), EMB, 16, 1 << 31) == _lib.PCG_E_ARG, name
        assert size(C.byref(q), EMB, 16, (1 << 31) - 1) > 0, name
        # emb is the dense parts' business: the chosen size has none
        if name == "chosen":
            assert size(C.byref(q), 60, 16, 100) == size(C.byref(q), EMB, 16, 100), name
        else:
            assert size(C.byref(q), 60, 16, 100) == _lib.PCG_E_UNSUPPORTED, name
        # R * chunk must stay below 2^31 (R = 3: 715827883 rows reach it, one fewer does not)
        assert size(C.byref(q), EMB, 715827883, 100) == _lib.PCG_E_ARG, name
        assert size(C.byref(q), EMB, 715827882, 100) > 0, name
    assert lib.pcg_infer_new_workspace_bytes(None, C.byref(q), EMB, 16, 100) == _lib.PCG_E_ARG
