"""The chunk loop the whole-set calls share (pcg_infer_set, pcg_chosen_set, pcg_infer_new: plan -> select -> their own stage per
chunk of ids, two plan slots): every layout of chunks a call can have - chunks of one row, full chunks plus a shorter tail, a
tail equal to the chunk, one chunk, a chunk larger than the set - gives bit for bit what one chunk gives, and what the per-batch
``predict`` loop gives; the status word is left zero, and a call after an overflow works."""
from unittest import mock

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


def status_reads(fz, call) -> int:
    """the number of times `call` reads the whole-set status word - its host synchronisations"""
    with mock.patch.object(fz, "_infer_status", wraps=fz._infer_status) as reads:
        call()
    return reads.call_count


@pytest.mark.parametrize("chunk", [7, None])
def test_every_public_call_synchronises_as_often_as_documented(case, chunk):
    """"Synchronises once (the status word; once more per ``chosen`` call)", whatever the number of chunks: 7 = seven chunks and
    a tail of one row.  ``nearest`` embeds the bank once (while it is cold) and then the requested rows ``chunk`` at a time."""
    fz, ids, query, _ = case
    labels = (ids % 2).astype(np.int64)
    once = {
        "infer": lambda: fz.infer(ids, chunk=chunk),
        "chosen": lambda: fz.chosen(ids, chunk=chunk),
        "chosen(train)": lambda: fz.chosen(ids, chunk=chunk, train_flag=True, labels=labels),
        "attribute": lambda: fz.attribute(ids, chunk=chunk),
        "infer_new": lambda: fz.infer_new(query, chunk=chunk),
        "chosen_new": lambda: fz.chosen_new(query, chunk=chunk),
        "attribute_new": lambda: fz.attribute_new(query, chunk=chunk),
        "attribute_new(neighbours)": lambda: fz.attribute_new(query, chunk=chunk, neighbours=True),
        "embed": lambda: fz.embed(ids, chunk=chunk),
        "embed_new": lambda: fz.embed_new(query, chunk=chunk),
        "evaluate": lambda: fz.evaluate(ids, labels, chunk=chunk),
    }
    for what, call in once.items():
        assert status_reads(fz, call) == 1, what
    assert status_reads(fz, lambda: fz.attribute(ids, chunk=chunk, neighbours=True)) == 2
    parts = 1 if chunk is None else -(-NQ // chunk)          # (nearest searches `chunk` rows at a time: one embed each)
    fz._inf.pop("bank", None)                                # a cold bank: its embed, then the parts'
    assert status_reads(fz, lambda: fz.nearest(ids, chunk=chunk)) == 1 + parts
    assert status_reads(fz, lambda: fz.nearest(ids, chunk=chunk)) == parts
    assert status_word(fz) == 0

    # an empty id list: the empty result, nothing launched, nothing read
    empty = {
        "infer": lambda: fz.infer([], chunk=chunk),
        "chosen": lambda: fz.chosen([], chunk=chunk),
        "chosen(train)": lambda: fz.chosen([], chunk=chunk, train_flag=True, labels=[]),
        "attribute": lambda: fz.attribute([], chunk=chunk),
        "attribute(neighbours)": lambda: fz.attribute([], chunk=chunk, neighbours=True),     # (through chosen, which returns early)
        "infer_new": lambda: fz.infer_new(query, [], chunk=chunk),
        "chosen_new": lambda: fz.chosen_new(query, [], chunk=chunk),
        "attribute_new": lambda: fz.attribute_new(query, [], chunk=chunk),
        "attribute_new(neighbours)": lambda: fz.attribute_new(query, [], chunk=chunk, neighbours=True),
        "embed": lambda: fz.embed([], chunk=chunk),
        "embed_new": lambda: fz.embed_new(query, [], chunk=chunk),
        "nearest": lambda: fz.nearest([], chunk=chunk),                                      # (the bank is warm)
    }
    sizes = {}
    for what, call in empty.items():
        assert status_reads(fz, lambda: sizes.__setitem__(what, call())) == 0, what
    assert sizes["infer"].shape == (0, 2) and sizes["infer_new"].shape == (0, 2)
    assert sizes["embed"].shape == (0, EMB) and sizes["embed_new"].shape == (0, EMB)
    assert sizes["chosen"].n == sizes["chosen(train)"].n == sizes["chosen_new"].n == 0
    for what in ("attribute", "attribute(neighbours)", "attribute_new", "attribute_new(neighbours)"):
        assert sizes[what].logits.shape == (0, 2), what
    assert sizes["attribute(neighbours)"].chosen.n == 0 and sizes["attribute_new(neighbours)"].chosen.n == 0
    assert sizes["nearest"].ids.shape == (0, 5)
    # (evaluate has no empty result - no metric is defined without labels -: its infer returns early all the same)
    with mock.patch.object(fz, "_infer_status", wraps=fz._infer_status) as reads:
        with pytest.raises(ValueError, match="Only one class present"):
            fz.evaluate([], [], chunk=chunk)
    assert reads.call_count == 0
