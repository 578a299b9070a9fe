"""The host side of alert cases: the reference the GPU tests compare against (tests/cases_ref.py) checked against scipy's
connected_components and a brute-force link count, graph.CaseList on CPU tensors, and the C ABI's prototypes and argument checks,
which return before any launch.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import cases_ref as R


def random_case(seed):
    rs = np.random.RandomState(seed)
    n = int(rs.randint(2, 60))
    n_rel = int(rs.randint(1, 4))
    csr = R.random_csr(rs, n, n_rel, avg_deg=rs.choice([0.3, 1.0, 2.5]), symmetric=bool(rs.rand() < 0.2))
    m = int(rs.randint(0, 80))
    members = rs.randint(0, n, size=m)                                   # (with replacement: duplicates)
    members[rs.rand(m) < 0.15] = -1                                      # padding anywhere
    relations = None if rs.rand() < 0.4 else sorted(rs.choice(n_rel, size=rs.randint(1, n_rel + 1), replace=False).tolist())
    labels = rs.randint(0, 2, size=m)
    return csr, n, members, relations, labels


@pytest.mark.parametrize("block", range(4))
def test_reference_matches_scipy_and_the_definitions(block):
    for seed in range(block * 75, block * 75 + 75):                       # 300 random cases in all
        csr, n, members, relations, labels = random_case(seed)
        out = R.group(csr, members, n, relations, labels)
        ok = R.valid_slots(members, n)
        assert R.same_partition(out["case_of"], R.scipy_partition(csr, members, n, relations)), seed
        C_ = out["n_cases"]
        assert out["head"].size == C_ and out["offsets"].size == C_ + 1 and out["offsets"][-1] == ok.sum() == out["order"].size
        for c in range(C_):
            slots = np.nonzero(out["case_of"] == c)[0]
            assert out["head"][c] == slots.min(), seed                   # the head is the lowest slot
            assert np.array_equal(out["order"][out["offsets"][c]:out["offsets"][c + 1]], slots), seed
            assert out["hits"][c] == int((labels[slots] == 1).sum()), seed
        assert np.all(np.diff(out["head"]) > 0)                          # numbered by ascending head
        assert np.all(out["case_of"][~ok] == -1)
        assert np.array_equal(out["links"], R.brute_links(csr, members, n, relations, out["case_of"], C_)), seed


def test_reference_on_crafted_lists():
    # relation 0: 0 -> 1 stored one way; relation 1: 2 <-> 3; 4 shares neighbour 9 with 5 (9 is no member): not linked
    csr = [R.csr_from_pairs(10, [0, 4, 5], [1, 9, 9]), R.csr_from_pairs(10, [2, 3], [3, 2])]
    out = R.group(csr, [1, 0, 3, 2, 4, 5, -1, 4, 10, -2], 10)
    assert out["case_of"].tolist() == [0, 0, 1, 1, 2, 3, -1, 2, -1, -1]
    assert out["head"].tolist() == [0, 2, 4, 5] and out["offsets"].tolist() == [0, 2, 4, 6, 7]
    assert out["order"].tolist() == [0, 1, 2, 3, 4, 7, 5] and out["links"].tolist() == [1, 2, 0, 0]
    only0 = R.group(csr, [1, 0, 3, 2], 10, relations=[0])
    assert only0["case_of"].tolist() == [0, 0, 1, 2] and only0["links"].tolist() == [1, 0, 0]
    empty = R.group(csr, [-1, -1], 10)
    assert empty["n_cases"] == 0 and empty["offsets"].tolist() == [0] and empty["order"].size == 0


def test_case_list_methods_on_cpu_tensors():
    import torch
    from pcgnn_amd.graph import AlertList, CaseList
    csr = [R.csr_from_pairs(8, [0, 2, 2], [1, 3, 5])]
    ids = np.array([1, 2, 0, 5, 7, 3, -1], dtype=np.int32)
    prob = np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, -np.inf], dtype=np.float32)
    ref = R.group(csr, ids, 8)
    al = AlertList(torch.from_numpy(ids), torch.arange(7, dtype=torch.int32), torch.from_numpy(prob), 6)
    t = lambda k: torch.from_numpy(ref[k])
    cl = CaseList(t("case_of"), t("head"), t("offsets"), t("order"), t("links"), None, ref["n_cases"], torch.from_numpy(ids), al)
    assert ref["case_of"].tolist() == [0, 1, 0, 1, 2, 1, -1]
    assert cl.n_cases == 3 and cl.size().tolist() == [2, 3, 1]
    slots, cids, cprob = cl.case(1)
    assert slots.tolist() == [1, 3, 5] and cids.tolist() == [2, 5, 3] and cprob.tolist() == [prob[1], prob[3], prob[5]]
    with pytest.raises(IndexError):
        cl.case(3)
    want = [float(prob[0]) + float(prob[2]), (float(prob[1]) + float(prob[3])) + float(prob[5]), float(prob[4])]
    eh = cl.expected_hits()
    assert eh.dtype == torch.float64 and eh.tolist() == want              # slot order inside every case
    arrays = cl.to_numpy()
    assert len(arrays) == 5 and all(np.array_equal(a, ref[k]) for a, k in zip(arrays, ("case_of", "head", "offsets", "order", "links")))
    bare = CaseList(t("case_of"), t("head"), t("offsets"), t("order"), t("links"), t("links"), ref["n_cases"], torch.from_numpy(ids))
    assert bare.case(0).tolist() == [0, 2] and len(bare.to_numpy()) == 6
    with pytest.raises(ValueError):
        bare.expected_hits()
    none = CaseList(torch.full((2,), -1, dtype=torch.int32), t("head")[:0], torch.zeros(1, dtype=torch.int32), t("order")[:0],
                    t("links")[:0], None, 0, torch.full((2,), -1, dtype=torch.int32), AlertList(torch.full((2,), -1, dtype=torch.int32),
                    torch.full((2,), -1, dtype=torch.int32), torch.full((2,), -np.inf), 0))
    assert none.size().numel() == 0 and none.expected_hits().numel() == 0


def test_prototypes_and_abi_version():
    from pcgnn_amd import _lib
    for name in ("pcg_alert_cases_workspace_bytes", "pcg_alert_cases"):
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) <= 16, name
    assert len(_lib.PROTOTYPES["pcg_alert_cases"][1]) == 16
    assert _lib.ABI_VERSION == 13 and _lib.load().pcg_abi_version() == 13


def test_argument_checks_return_before_any_launch():
    """every rejected call is made with addresses that are not device memory: a launch would not return PCG_E_ARG"""
    from pcgnn_amd import _lib
    lib = _lib.load()
    E = _lib.PCG_E_ARG
    assert lib.pcg_alert_cases_workspace_bytes(1000, -1) == E and lib.pcg_alert_cases_workspace_bytes(1000, 65537) == E
    assert lib.pcg_alert_cases_workspace_bytes(0, 10) == E
    small, big = lib.pcg_alert_cases_workspace_bytes(1000, 0), lib.pcg_alert_cases_workspace_bytes(1000, 65536)
    assert 4 * 1000 <= small < big and small % 256 == 0 and big % 256 == 0
    assert lib.pcg_alert_cases_workspace_bytes(2_000_000, 100) >= 8_000_000           # the position map: 4 bytes per node

    g = _lib.GraphDesc()
    g.n_nodes, g.feat_dim, g.feat_stride, g.n_rel = 1000, 4, 4, 3
    for r in range(3):
        g.indptr[r] = g.indices[r] = 0x1000
    a = C.c_void_p(0x10000)                                               # 256-byte aligned, never dereferenced
    need = lib.pcg_alert_cases_workspace_bytes(1000, 10)

    def call(gd=g, members=a, m=10, mask=7, labels=None, ws=a, nbytes=need, case_of=a, head=a, offsets=a, order=a, links=a, hits=None,
             hdr=a, status=a):
        return lib.pcg_alert_cases(C.byref(gd) if gd is not None else None, members, m, mask, labels, ws, nbytes, case_of, head, offsets,
                                   order, links, hits, hdr, status, None)

    assert call(gd=None) == E
    for name in ("members", "ws", "case_of", "head", "offsets", "order", "links", "hdr", "status"):
        assert call(**{name: None}) == E, name
    assert call(m=-1) == E and call(m=65537, nbytes=1 << 40) == E
    assert call(mask=0) == E and call(mask=8) == E and call(mask=0xF) == E             # empty / a relation the graph has not
    assert call(nbytes=need - 1) == E and call(ws=C.c_void_p(0x10010)) == E           # too small / misaligned
    assert call(labels=a) == E and call(hits=a) == E                                   # labels and hits go together
