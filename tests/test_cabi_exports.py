"""CPU checks of the drop-in boundary: the shared library builds/loads and exports
every symbol include/pcgnn.h declares; host-side helpers agree with the oracle.
No compute calls (there is no GPU here)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "pcgnn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pcg_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    import pcgnn_amd
    from pcgnn_amd import _lib
    pcgnn_amd.build_library()
    lib = _lib.load()
    syms = declared_symbols()
    assert len(syms) >= 10
    for s in syms:
        assert hasattr(lib, s), f"libpcgnn_hip.so does not export {s}"
        assert s in _lib.PROTOTYPES, f"ctypes prototype missing for {s}"
    assert lib.pcg_abi_version() == _lib.ABI_VERSION
    assert lib.pcg_version().startswith(b"pcgnn_hip gfx950")


def test_host_helpers_and_argument_checks():
    from pcgnn_amd import _lib
    lib = _lib.load()
    # pcg_sel_capacity_row == the oracle's counting rule (layers.py:260-262, 662, 681)
    import math
    for deg in range(0, 40):
        for thr in (0.2, 0.5, 0.8, 1.0):
            for rho in (0.0, 0.5, 2.0):
                k = math.ceil(deg * thr)
                want = (k if deg > k + 1 else deg) + min(int(k * rho), 7)
                assert lib.pcg_sel_capacity_row(deg, thr, rho, 1, 7, 0) == want
                assert lib.pcg_sel_capacity_row(deg, thr, rho, 0, 7, 1) == (k if deg > k + 1 else deg) + 1
    assert lib.pcg_pos_sort_capacity(0) == 8192 and lib.pcg_pos_sort_capacity(4097) == 16384 and lib.pcg_pos_sort_capacity(20000) == 65536
    # null / inconsistent arguments are rejected before any launch
    assert lib.pcg_score_table(None, None, None, 0, 0, None, None) == _lib.PCG_E_ARG
    assert lib.pcg_pick(None, None, 0, None, 0, 0, 1, None, None) == _lib.PCG_E_ARG
    assert lib.pcg_choose_workspace_bytes(None, 4, 10) == _lib.PCG_E_ARG


def test_param_struct_mirrors_match_the_header():
    """every ctypes mirror of a parameter struct: size, member count and every member's offset are what the library was
    compiled with (pcg_abi_layout)"""
    import ctypes as C
    from pcgnn_amd import _lib
    lib = _lib.load()
    out = (C.c_int64 * 64)()
    for which, T in enumerate(_lib.ABI_STRUCTS):
        n = lib.pcg_abi_layout(which, out, 64)
        assert n == 1 + len(T._fields_), f"{T.__name__}: {n - 1} members in the header, {len(T._fields_)} in the mirror"
        assert out[0] == C.sizeof(T), T.__name__
        for i, (name, _) in enumerate(T._fields_):
            assert out[1 + i] == getattr(T, name).offset, f"{T.__name__}.{name}"
    assert lib.pcg_abi_layout(len(_lib.ABI_STRUCTS), out, 64) == _lib.PCG_E_ARG
    assert lib.pcg_abi_layout(-1, out, 64) == _lib.PCG_E_ARG
    assert lib.pcg_abi_layout(0, None, 64) == _lib.PCG_E_ARG
    assert lib.pcg_abi_layout(1, out, 3) == _lib.PCG_E_ARG and out[0] == C.sizeof(_lib.ABI_STRUCTS[-1])   # (nothing written)


def test_training_entry_points_reject_null_structs_and_members():
    """Each of the thirteen entry points that take parameter structs returns PCG_E_ARG - before any launch: there is no device
    here - for NULL struct pointers, and for structs whose required members are NULL (theta, sync_words, step_counter, ids
    with B >= 1, slabs, acts ...)."""
    import ctypes as C
    from pcgnn_amd import _lib
    lib = _lib.load()
    g = _lib.GraphDesc(n_nodes=64, feat_dim=8, feat_stride=8, n_rel=1, n_pos=0, max_degree=4)     # every pointer NULL
    thr = (C.c_double * 1)(0.5)
    hyper = _lib.AdamHyper(0.01, 0.9, 0.999, 1e-8, 0.0)
    st = _lib.TrainState(emb=64, act_ld=16, lambda_1=2.0, hyper=hyper)                             # every pointer NULL
    sel = _lib.SelectWs(thr, thr, None, None, 100, 0)
    b = _lib.Batch(None, None, None, None, 4, 0.25)
    out = _lib.DenseOut()
    N = None
    calls = {
        "pcg_choose_gather_train": lambda st, sel, b, out, h: (g, b, N, N, sel, N, 8, st, 1, N, 0, N),
        "pcg_choose_train_part": lambda st, sel, b, out, h: (1, g, b, N, N, sel, N, 8, st, 1, N, 0, N, N),
        "pcg_dense_select_train": lambda st, sel, b, out, h: (g, st, sel, b, b, N, 8, N, out, N, N, N, N),
        "pcg_dense_select_ahead": lambda st, sel, b, out, h: (g, st, sel, b, b, b, N, 8, N, out, N, N, N, N, N),
        "pcg_clf_step": lambda st, sel, b, out, h: (g, b, st, N, 1, N),
        "pcg_step_scores_train": lambda st, sel, b, out, h: (g, st, N, N, N, N),
        "pcg_train_dense": lambda st, sel, b, out, h: (g, st, b, N, 8, sel, out, 3, N, N),
        "pcg_step_front_train": lambda st, sel, b, out, h: (g, st, N, N, b, sel, N),
        "pcg_adam_apply_pending": lambda st, sel, b, out, h: (N, N, N, N, 100, N, N, 0, h, N),
        "pcg_adam_flush": lambda st, sel, b, out, h: (st, 0, 100, 50, 8, 1, N),
        "pcg_wgrad": lambda st, sel, b, out, h: (st, 4, 8, 1, N, 1, 1, N, N),
        "pcg_step_scores_dist": lambda st, sel, b, out, h: (g, st, N, N, 0, 64, N, N, N, -1, N),
        "pcg_adam_step": lambda st, sel, b, out, h: (N, N, N, N, 1, 100, N, h, N, 1, N),
    }
    for name, args in calls.items():
        fn = getattr(lib, name)
        assert fn(*args(N, N, N, N, N)) == _lib.PCG_E_ARG, f"{name}: NULL struct pointers"
        assert fn(*args(st, sel, b, out, hyper)) == _lib.PCG_E_ARG, f"{name}: structs with NULL members"
        assert len(_lib.PROTOTYPES[name][1]) <= 16, name


def test_product_path_refuses_cpu():
    """No CPU fallback: building a graph on a CPU device must raise."""
    import torch
    import pcgnn_amd
    with pytest.raises(pcgnn_amd.PcgnnLibraryError):
        pcgnn_amd.DeviceGraph(np.zeros((4, 8), np.float32), [(np.zeros(5, np.int64), np.zeros(0, np.int32))], [],
                              torch.device("cpu"))


def test_adj_to_csr_matches_oracle():
    from oracle import pcgnn_oracle as O
    from pcgnn_amd.graph import adj_to_csr
    rs = np.random.RandomState(0)
    n = 200
    adj = {v: {v} | set(rs.randint(0, n, size=rs.randint(0, 9)).tolist()) for v in range(n)}
    a, b = adj_to_csr(adj, n)
    c, d = O.adj_to_csr(adj, n)
    assert np.array_equal(a, c) and np.array_equal(b, d)
