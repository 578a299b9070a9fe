"""The chunk loop the whole-set calls share (pcg_infer_set, pcg_chosen_set, pcg_infer_new: plan -> select -> their own stage per
chunk of ids, two plan slots): every layout of chunks a call can have - chunks of one row, full chunks plus a shorter tail, a
tail equal to the chunk, one chunk, a chunk larger than the set - gives bit for bit what one chunk gives, and what the per-batch
``predict`` loop gives; the status word is left zero, and a call after an overflow works."""
import numpy as np
import pytest
import torch

from tests.util import synth_graph

pytestmark = pytest.mark.gpu

N, F, EMB, NQ = 600, 32, 64, 50
CHUNKS = (1, 7, 25, 49, 50, 55)         # n = 50: 50 x 1 | 7 x 7 + 1 | 25 + 25 | 49 + 1 | one chunk | a chunk beyond the set
HUB = 7                                 # synth_graph's hub row


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def case():
    import pcgnn_amd as P
    from pcgnn_amd.fused import FusedPCGNN
    from pcgnn_amd.graph import QueryBatch
    X, labels, csrs = synth_graph(4, N, F, (3, 10, 40), 0.15)
    train_pos = [int(v) for v in np.nonzero(labels[:N // 2])[0]]
    torch.manual_seed(0)
    g = P.DeviceGraph(X, csrs, train_pos, dev())
    hub_deg = max(int(ip[HUB + 1] - ip[HUB]) for ip, _ in csrs)
    assert g.max_degree == hub_deg > 128            # more than 64 kept at threshold 0.5: the rank launch for long rows runs
    feats = torch.nn.Embedding(N, F)
    feats.weight = torch.nn.Parameter(torch.from_numpy(X), requires_grad=False)
    intras = [P.IntraAgg(feats, F, EMB, train_pos, 0.5, cuda=True) for _ in csrs]
    inter = P.InterAgg(feats, F, EMB, train_pos, g, intras, cuda=True)
    fz = FusedPCGNN(P.PCALayer(2, inter, 2.0).cuda(), 0.01, 0.001, max_batch=256)
    rs = np.random.RandomState(5)
    ids = np.concatenate([rs.randint(0, N, size=NQ - 5), [HUB, HUB, N - 1, 0, HUB]])
    rs.shuffle(ids)
    assert ids.size == NQ and np.unique(ids).size < NQ
    # a query batch of NQ unseen nodes: lists into the base graph, among themselves, the node itself
    pairs = []
    for _ in csrs:
        rows = [np.concatenate([rs.randint(0, N + NQ, size=rs.randint(0, 30)), [N + j]]) for j in range(NQ)]
        pairs.append((np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64), np.concatenate(rows).astype(np.int64)))
    query = QueryBatch(rs.randn(NQ, F).astype(np.float32), pairs, g)
    # the references, computed once: the per-batch predict loop, and each call with its default single chunk
    idt = torch.from_numpy(ids.astype(np.int32)).to(dev())
    parts = [fz.predict(idt[b:b + 16], None, False) for b in range(0, NQ, 16)]
    want = dict(gnn=torch.cat([p[0] for p in parts]), center=torch.cat([p[1] for p in parts]),
                chosen=fz.chosen(ids), new=fz.infer_new(query, want_center=True))
    return fz, ids, query, want


def status_word(fz) -> int:
    return int(fz._inf["status"].item())


@pytest.mark.parametrize("chunk", CHUNKS)
def test_infer_equals_the_predict_loop(case, chunk):
    fz, ids, _, want = case
    gnn, center = fz.infer(ids, chunk=chunk, want_center=True)
    assert torch.equal(gnn, want["gnn"]) and torch.equal(center, want["center"])
    assert status_word(fz) == 0


@pytest.mark.parametrize("chunk", CHUNKS)
def test_chosen_equals_one_chunk(case, chunk):
    fz, ids, _, want = case
    ch = fz.chosen(ids, chunk=chunk)
    assert np.array_equal(ch.host_offsets(), want["chosen"].host_offsets())
    assert torch.equal(ch.ids, want["chosen"].ids) and torch.equal(ch.dist, want["chosen"].dist)
    assert status_word(fz) == 0


@pytest.mark.parametrize("chunk", CHUNKS)
def test_infer_new_equals_one_chunk(case, chunk):
    fz, _, query, want = case
    gnn, center = fz.infer_new(query, chunk=chunk, want_center=True)
    assert torch.equal(gnn, want["new"][0]) and torch.equal(center, want["new"][1])
    assert status_word(fz) == 0


def test_a_call_after_an_overflow_works(case):
    from pcgnn_amd import PcgnnLibraryError
    fz, ids, query, want = case
    with pytest.raises(PcgnnLibraryError, match="selection list overflow"):
        fz.infer_new(query, _list_capacity=5)
    assert status_word(fz) == 0                       # (read once and cleared)
    assert torch.equal(fz.infer_new(query), want["new"][0])
    assert torch.equal(fz.infer(ids, chunk=7), want["gnn"])
    assert status_word(fz) == 0
    fz.check()
