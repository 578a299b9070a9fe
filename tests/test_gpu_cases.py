"""Alert cases on an MI355X (pcg_alert_cases, ops.group_members, EvalCalls.cases): every integer ``==`` the host reference
(tests/cases_ref.py) on crafted graphs - list sizes around every block size, chains (the deepest parent paths), a clique (every
union contends for one root), stars around the row-length thresholds, one-directional edges, relation masks, duplicates, padding,
bad ids and labels - on random hub graphs with two runs and a graph replay bit for bit, inside a guarded arena at exactly the
documented sizes, and end to end through the engines.  Run with ``pytest -m gpu``."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cases_ref as R
from tests.guarded import GuardedArena
from tests.util import synth_graph

pytestmark = pytest.mark.gpu

# the kernels' geometry (pc-gnn_amd/csrc/cases.hip)
CS_THREADS = 256          # workgroup of the per-slot passes; link: 4 waves = 4 (slot, relation) rows per workgroup
CS_ROW_MAX = 512          # longest row one wave walks; longer rows are queued
CS_PARTS = 16             # workgroups a queued row is spread over
CS_SCAN_THREADS = 1024    # the one workgroup of the numbering / offsets scans: thread t owns ceil(m / 1024) slots
MAX_M = 65536
SIZES = sorted({0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, CS_SCAN_THREADS - 1, CS_SCAN_THREADS, CS_SCAN_THREADS + 1,
                2 * CS_SCAN_THREADS - 1, 2 * CS_SCAN_THREADS, 2 * CS_SCAN_THREADS + 1, MAX_M - 1, MAX_M})
# hub rows: around the wave / queue threshold, and around the length at which a part outgrows one pass of its workgroup
STAR_ROWS = (CS_ROW_MAX - 1, CS_ROW_MAX, CS_ROW_MAX + 1, CS_PARTS * CS_THREADS - 1, CS_PARTS * CS_THREADS, CS_PARTS * CS_THREADS + 1, 5000)
KEYS = ("case_of", "head", "offsets", "order", "links")

_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def dev():
    return torch.device("cuda", 0)


def graph(csr, n):
    import pcgnn_amd as P
    return P.DeviceGraph(np.zeros((n, 1), dtype=np.float32), csr, [], dev())


def run(g, members, relations=None, labels=None):
    """-> (CaseList, status word); the word is the caller's, so nothing raises"""
    from pcgnn_amd import ops
    st = torch.zeros(1, dtype=torch.int32, device=dev())
    cl = ops.group_members(g, np.asarray(members, dtype=np.int32), relations=relations, labels=labels, status=st)
    return cl, int(st.item())


def assert_same(cl, ref, what=""):
    got = cl.to_numpy()
    assert cl.n_cases == ref["n_cases"], (what, cl.n_cases, ref["n_cases"])
    for k, a in zip(KEYS, got):
        assert a.dtype == np.int32 and np.array_equal(a, ref[k]), (what, k)
    if ref["hits"] is not None:
        assert np.array_equal(got[5], ref["hits"]), (what, "hits")
    else:
        assert cl.hits is None


def check(g, csr, n, members, relations=None, labels=None, status=0, what=""):
    cl, st = run(g, members, relations, labels)
    assert st == status, (what, st)
    ref = R.group(csr, members, n, relations, labels)
    assert_same(cl, ref, what)
    return cl, ref


# ---- sizes ---------------------------------------------------------------------------------------------------------------------
def sparse():
    n = 70000
    rs = np.random.RandomState(1)
    csr = R.random_csr(rs, n, 2, 0.6)
    return n, csr, graph(csr, n)


@pytest.mark.parametrize("m", SIZES)
def test_sizes(m):
    n, csr, g = memo("sparse", sparse)
    rs = np.random.RandomState(m + 7)
    members = rs.randint(0, n, size=m)
    members[rs.rand(m) < 0.05] = -1
    labels = rs.randint(0, 2, size=m)
    cl, ref = check(g, csr, n, members, labels=labels, what=f"m {m}")
    if m >= 1000:
        assert 1 < ref["n_cases"] < m and ref["links"].sum() > 0 and (np.diff(ref["offsets"]) > 1).any()    # not a degenerate input


def test_rejected_with_no_launch():
    from pcgnn_amd import _lib, ops
    n, csr, g = memo("sparse", sparse)
    with pytest.raises(ValueError):
        ops.group_members(g, np.zeros(MAX_M + 1, dtype=np.int32))
    for bad in ([], [2], [-1], [0, 5]):
        with pytest.raises(ValueError):
            ops.group_members(g, [1, 2, 3], relations=bad)
    lib = _lib.load()
    t = torch.zeros(MAX_M + 8, dtype=torch.int32, device=dev())
    nbytes = lib.pcg_alert_cases_workspace_bytes(n, 16)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    p = lambda x: C.c_void_p(x.data_ptr())
    call = lambda m, mask: lib.pcg_alert_cases(g.desc_ref(), p(t), m, mask, None, p(ws), nbytes, p(t), p(t), p(t), p(t), p(t), None, p(t),
                                               p(t), None)
    assert call(MAX_M + 1, 3) == _lib.PCG_E_ARG and call(16, 0) == _lib.PCG_E_ARG and call(16, 4) == _lib.PCG_E_ARG
    torch.cuda.synchronize()
    assert int(t.abs().sum().item()) == 0                                 # nothing ran


# ---- chains, clique, stars -----------------------------------------------------------------------------------------------------
def chain(m):
    i = np.arange(m - 1)
    csr = [R.csr_from_pairs(m, np.concatenate([i, i + 1, np.arange(m)]), np.concatenate([i + 1, i, np.arange(m)]))]
    return csr, graph(csr, m)


@pytest.mark.parametrize("m", [4096, MAX_M])
@pytest.mark.parametrize("how", ["in order", "reversed", "permuted"])
def test_chain(m, how):
    csr, g = memo(("chain", m), lambda: chain(m))
    members = {"in order": np.arange(m), "reversed": np.arange(m)[::-1].copy(),
               "permuted": np.random.RandomState(m).permutation(m)}[how]
    cl, st = run(g, members)
    assert st == 0
    case_of, head, offsets, order, links = cl.to_numpy()
    assert cl.n_cases == 1 and head.tolist() == [0] and offsets.tolist() == [0, m] and links.tolist() == [2 * (m - 1)]
    assert not case_of.any() and np.array_equal(order, np.arange(m))
    if m == 4096:
        assert_same(cl, R.group(csr, members, m), how)


def test_clique():
    n, k = 400, 300
    a, b = np.meshgrid(np.arange(k), np.arange(k))
    csr = [R.csr_from_pairs(n, np.concatenate([a.ravel(), np.arange(n)]), np.concatenate([b.ravel(), np.arange(n)]))]
    g = graph(csr, n)
    members = np.random.RandomState(0).permutation(k)
    cl, ref = check(g, csr, n, members)
    assert cl.n_cases == 1 and ref["links"].tolist() == [k * (k - 1)]


def star(L):
    """node 0's row holds itself and the L leaves 1 .. L; the leaves' rows hold themselves only (the edges are stored one way)"""
    n = L + 3
    csr = [R.csr_from_pairs(n, np.concatenate([np.zeros(L, dtype=np.int64), np.arange(n)]), np.concatenate([np.arange(1, L + 1), np.arange(n)]))]
    return n, csr, graph(csr, n)


@pytest.mark.parametrize("row", STAR_ROWS)
def test_star(row):
    L = row - 1                                                            # the hub's row: itself and L leaves
    n, csr, g = memo(("star", L), lambda: star(L))
    assert csr[0][0][1] - csr[0][0][0] == L + 1
    leaves = np.arange(1, L + 1)
    for where, members in (("first", np.concatenate([[0], leaves])), ("last", np.concatenate([leaves, [0]]))):
        cl, ref = check(g, csr, n, members, what=f"hub {where}")
        assert cl.n_cases == 1 and ref["links"].tolist() == [L] and ref["head"].tolist() == [0]
    cl, ref = check(g, csr, n, leaves, what="hub not listed")              # a shared neighbour that is no member does not link
    assert cl.n_cases == L and not ref["links"].any() and np.array_equal(ref["order"], np.arange(L))
    # the hub's row with few members in it, and the hub twice
    few = np.array([L, 0, 1, L + 1, 0, L // 2])
    cl, ref = check(g, csr, n, few, what="few")
    assert ref["case_of"].tolist() == [0, 0, 0, 1, 0, 0] and ref["links"].tolist() == [6, 0]


# ---- the definitions on small lists ---------------------------------------------------------------------------------------------
def small():
    n = 12
    loops = np.arange(n)
    csr = [R.csr_from_pairs(n, np.concatenate([[0, 4, 5], loops]), np.concatenate([[1, 9, 9], loops])),       # 0 -> 1 one way
           R.csr_from_pairs(n, np.concatenate([[2, 3, 6, 7, 7], loops]), np.concatenate([[3, 2, 7, 6, 8], loops])),
           R.csr_from_pairs(n, np.concatenate([[0, 1], loops]), np.concatenate([[1, 0], loops]))]
    return n, csr, graph(csr, n)


def test_one_directional_edges():
    n, csr, g = memo("small", small)
    for members in ([0, 1], [1, 0]):                                       # stored in the row of p only / of q only
        cl, ref = check(g, csr, n, members, relations=[0])
        assert cl.n_cases == 1 and ref["links"].tolist() == [1]
    cl, ref = check(g, csr, n, [4, 5], relations=[0])                      # both point at 9, which is no member
    assert cl.n_cases == 2 and ref["links"].tolist() == [0, 0]
    cl, ref = check(g, csr, n, [4, 5, 9], relations=[0])
    assert cl.n_cases == 1 and ref["links"].tolist() == [2]
    cl, ref = check(g, csr, n, [0, 1])                                     # relation 0 one way + relation 2 both ways
    assert ref["links"].tolist() == [3]


def test_relations():
    n, csr, g = memo("small", small)
    members = [8, 6, 7, 2, 3]                                              # linked through relation 1 only
    for rel in ([1], None):
        cl, ref = check(g, csr, n, members, relations=rel)
        assert ref["case_of"].tolist() == [0, 0, 0, 1, 1] and ref["links"].tolist() == [3, 2]
    cl, ref = check(g, csr, n, members, relations=[0, 2])
    assert cl.n_cases == 5 and not ref["links"].any()
    cl, ref = check(g, csr, n, members, relations=(2, 1, 1))
    assert cl.n_cases == 2


def test_duplicates_and_padding():
    n, csr, g = memo("small", small)
    cl, ref = check(g, csr, n, [10, 11, 10, -1, 10, 11, -1, -1], labels=[1, 0, 1, 1, 0, 1, 1, 1])
    assert ref["case_of"].tolist() == [0, 1, 0, -1, 0, 1, -1, -1] and ref["hits"].tolist() == [2, 1] and not ref["links"].any()
    assert ref["order"].tolist() == [0, 2, 4, 1, 5]
    cl, ref = check(g, csr, n, [-1, 2, -1, 3, 3, -1])
    assert ref["case_of"].tolist() == [-1, 0, -1, 0, 0, -1] and ref["head"].tolist() == [1] and ref["links"].tolist() == [3]
    for m in (1, 5, 300):
        cl, ref = check(g, csr, n, np.full(m, -1), labels=np.ones(m, dtype=np.int64))
        assert cl.n_cases == 0 and cl.offsets.tolist() == [0] and cl.order.numel() == 0 and cl.hits.numel() == 0


def test_bad_inputs():
    from pcgnn_amd import _lib, ops
    n, csr, g = memo("small", small)
    for bad in (n, -2, 2 ** 31 - 1, -2 ** 31):
        members = [0, bad, 1, 2, bad, 3]
        cl, ref = check(g, csr, n, members, status=_lib.PCG_ST_LIST_ID_RANGE, what=f"id {bad}")
        padded = R.group(csr, [0, -1, 1, 2, -1, 3], n)
        assert_same(cl, padded)
        assert ref["case_of"].tolist() == [0, -1, 0, 1, -1, 1]
    cl, st = run(g, [0, 1, -1, 2], labels=[0, 2, 2, 1])                    # (a label on a padding slot is not looked at)
    assert st == _lib.PCG_ST_EVAL_INPUT
    cl, st = run(g, [0, 1, -1, 2], labels=[0, 1, 7, 1])
    assert st == 0 and cl.hits.tolist() == [1, 1]
    with pytest.raises(_lib.PcgnnLibraryError):                            # without a status word of the caller's it raises
        ops.group_members(g, [0, n])
    with pytest.raises(ValueError):
        ops.group_members(g, [0, 1], labels=[1])


def test_all_isolated():
    n, csr, g = memo("sparse", sparse)
    deg = sum(np.diff(ip) for ip, _ in csr)
    lone = np.nonzero(deg == 2)[0][:3000]                                  # self-loops only
    members = np.concatenate([lone[:1500], [-1, -1], lone[1500:]])
    cl, ref = check(g, csr, n, members)
    assert cl.n_cases == 3000 and np.array_equal(ref["order"], np.nonzero(members >= 0)[0]) and not ref["links"].any()


# ---- random hub graphs: two runs and a replay ------------------------------------------------------------------------------------
def hubs():
    n = 6000
    _, _, csr = synth_graph(5, n, 4, [3, 6, 12], 0.1)
    return n, csr, graph(csr, n)


@pytest.mark.parametrize("m", [100, 1000, 6000])
def test_random_graph_two_runs_and_a_replay(m):
    from pcgnn_amd import ops
    n, csr, g = memo("hubs", hubs)
    assert max(int(np.diff(ip).max()) for ip, _ in csr) > CS_ROW_MAX
    rs = np.random.RandomState(m)
    members = rs.permutation(n)[:m] if m < n else rs.permutation(n)
    members[:8] = 7                                                        # the hub, more than once
    labels = rs.randint(0, 2, size=m)
    refs = {}
    for rel in (None, [0, 2]):
        cl, ref = check(g, csr, n, members, relations=rel, labels=labels, what=f"relations {rel}")
        refs[str(rel)] = ref
        again, st = run(g, members, rel, labels)
        assert st == 0 and all(np.array_equal(a, b) for a, b in zip(cl.to_numpy(), again.to_numpy()))
    # the stand-alone call is capture-safe up to its final read: one replay, the whole of every buffer bit for bit
    mem = torch.from_numpy(members.astype(np.int32)).to(dev())
    lab = torch.from_numpy(labels.astype(np.int32)).to(dev())
    st = torch.zeros(1, dtype=torch.int32, device=dev())
    eager = ops.group_members_enqueue(g, mem, 7, lab, st)
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_):
        out = ops.group_members_enqueue(g, mem, 7, lab, st)
    for t in out:
        t.fill_(-5)
    graph_.replay()
    torch.cuda.synchronize()
    C_, valid = int(out[6][0]), int(out[6][1])
    assert out[6].tolist() == eager[6].tolist() == [refs["None"]["n_cases"], m, 0, 0] and int(st.item()) == 0
    for a, b, upto in zip(out[:6], eager[:6], (m, C_, C_ + 1, valid, C_, C_)):
        assert torch.equal(a[:upto], b[:upto])


# ---- extents ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 257, MAX_M])
def test_extents(m):
    from pcgnn_amd import _lib
    lib = _lib.load()
    n, csr, g = memo("hubs", hubs) if m < MAX_M else memo("sparse", sparse)
    rs = np.random.RandomState(m + 1)
    members = rs.randint(0, n, size=m)
    members[rs.rand(m) < 0.1] = -1
    labels = rs.randint(0, 2, size=m)
    nbytes = int(lib.pcg_alert_cases_workspace_bytes(n, m))
    arena = GuardedArena(nbytes + 8 * 4 * (m + 1) + (1 << 20), dev())
    i32 = lambda count, name: arena.take(count, torch.int32, name=name)
    mem, lab = i32(m, "members"), i32(m, "labels")
    mem.copy_(torch.from_numpy(members.astype(np.int32)))
    lab.copy_(torch.from_numpy(labels.astype(np.int32)))
    ws = arena.take(nbytes, torch.uint8, name="workspace")
    ws.fill_(0xA5)                                                         # contents irrelevant on entry
    case_of, head, offsets, order, links, hits = (i32(c, k) for c, k in ((m, "case_of"), (m, "head"), (m + 1, "offsets"), (m, "order"),
                                                                         (m, "links"), (m, "hits")))
    hdr, st = i32(4, "hdr"), i32(1, "status")
    p = lambda x: C.c_void_p(x.data_ptr())
    rc = lib.pcg_alert_cases(g.desc_ref(), p(mem), m, (1 << g.R) - 1, p(lab), p(ws), nbytes, p(case_of), p(head), p(offsets), p(order), p(links), p(hits),
                             p(hdr), p(st), C.c_void_p(torch.cuda.current_stream(dev()).cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    arena.check(f"pcg_alert_cases m {m}")
    ref = memo(("extent ref", m), lambda: R.group(csr, members, n, None, labels))
    C_, valid = ref["n_cases"], int((members >= 0).sum())
    assert hdr.tolist() == [C_, valid, 0, 0] and st.item() == 0
    for t, k, upto in ((case_of, "case_of", m), (head, "head", C_), (offsets, "offsets", C_ + 1), (order, "order", valid), (links, "links", C_),
                       (hits, "hits", C_)):
        assert np.array_equal(t[:upto].cpu().numpy(), ref[k]), k
    assert np.array_equal(order[valid:].cpu().numpy(), np.nonzero(members < 0)[0])     # the padding slots, ascending
    assert not links[C_:].any() and not hits[C_:].any()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def check_cases(model, cl, csr, n, labels_rows, relations=None):
    """a CaseList made by an engine: the reference on its own alert list's ids, hits, expected_hits"""
    al = cl.alerts
    ids, pos, prob = al.to_numpy()[:3]
    lab_slots = None if labels_rows is None else np.where(pos >= 0, np.asarray(labels_rows)[np.maximum(pos, 0)], 0)
    ref = R.group(csr, ids, n, relations, lab_slots)
    assert_same(cl, ref)
    assert np.array_equal(cl.members.cpu().numpy(), ids)
    if lab_slots is not None:
        for c in range(ref["n_cases"]):
            slots = ref["order"][ref["offsets"][c]:ref["offsets"][c + 1]]
            assert ref["hits"][c] == int((lab_slots[slots] == 1).sum())
    eh = cl.expected_hits()
    assert eh.dtype == torch.float64 and eh.numel() == ref["n_cases"]
    eh = eh.cpu().numpy()
    for c in range(ref["n_cases"]):
        slots = ref["order"][ref["offsets"][c]:ref["offsets"][c + 1]]
        want = prob[slots].astype(np.float64).sum()
        assert abs(eh[c] - want) <= (len(slots) - 1) * 2.0 ** -53 * want, (c, eh[c], want)
        if c < 20:
            s, i, p = cl.case(c)
            assert np.array_equal(s.cpu().numpy(), slots) and np.array_equal(i.cpu().numpy(), ids[slots])
            assert np.array_equal(p.cpu().numpy().view(np.uint32), prob[slots].view(np.uint32))
    return ref


def test_engine_cases():
    from pcgnn_amd import utils as U
    from tests.test_gpu_infer_new import mini
    w, mk, mkq = mini()
    t = mk()
    for _ in range(2):
        t.run_epoch_one_graph()
    fz = t.fused
    held = np.setdiff1d(np.arange(w.n), w.idx_train)
    lab = w.labels[held]
    sizes = []
    for k in (1, 100, len(held) + 5):
        cl = fz.cases(held, k=k, labels=lab)
        ref = check_cases(fz, cl, w.csr, w.n, lab)
        assert cl.alerts.k == k and np.array_equal(cl.alerts.to_numpy()[0], fz.alerts(held, k=k).to_numpy()[0])
        sizes.append(ref["n_cases"])
    assert sizes[0] == 1 and sizes[1] <= 100 and sizes[2] < len(held)                      # rings, not k separate rows and not one blob
    one = fz.cases(held, k=100, relations=[0])
    check_cases(fz, one, w.csr, w.n, None, relations=[0])
    assert one.hits is None and one.n_cases >= sizes[1]
    via = U.alert_cases(fz, held, k=100, labels=lab)
    assert all(np.array_equal(a, b) for a, b in zip(via.to_numpy(), fz.cases(held, k=100, labels=lab).to_numpy()))
    whole = fz.cases(k=64)                                                 # ids None: every node
    check_cases(fz, whole, w.csr, w.n, None)
    with pytest.raises(ValueError):
        fz.cases(k=10, query=mkq(t))
    with pytest.raises(ValueError):
        fz.cases(held, k=10, relations=[3])
    with pytest.raises(ValueError):
        fz.cases(held, k=10, labels=lab[:-1])
    fz.check()


@pytest.mark.parametrize("shape", ["sage", "gcn"])
def test_baseline_model_cases(shape):
    import pcgnn_amd as P
    from pcgnn_amd import graphsage as GS, utils as U
    from tests import baseline_ref as BR
    n, F, E = 1500, 25, 64
    X, _, csrs = memo("synth", lambda: synth_graph(3, n, F, [6], 0.1))
    labels = (np.random.RandomState(8).rand(n) < 0.2).astype(np.int64)
    g = memo("synth_g", lambda: P.DeviceGraph(X, csrs, [], dev()))
    model = BR.build_model(GS, g, F, E, shape, seed=6)
    ids = np.random.RandomState(4).permutation(n)[:1100]
    y = labels[ids]
    for k in (1, 100, len(ids) + 5):
        cl = model.cases(ids, k=k, labels=y)
        check_cases(model, cl, csrs, n, y)
        via = U.alert_cases(model, ids, k=k, labels=y)
        assert all(np.array_equal(a, b) for a, b in zip(via.to_numpy(), cl.to_numpy()))
    eng = U.alert_cases(model.engine(), ids, k=100, labels=y)
    assert all(np.array_equal(a, b) for a, b in zip(eng.to_numpy(), model.cases(ids, k=100, labels=y).to_numpy()))
    with pytest.raises(ValueError):
        model.cases(ids, k=8, query=object())
