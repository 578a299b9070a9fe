"""No whole-set call writes - or depends on a read - outside the sizes include/pcgnn.h documents: ``infer``, ``chosen``,
``attribute``, ``infer_new``, ``chosen_new``, ``attribute_new`` and ``evaluate`` on an engine built inside a guarded arena
(tests/guarded.py), so that their workspaces (pcg_infer_workspace_bytes, pcg_chosen_workspace_bytes,
pcg_infer_new_workspace_bytes / pcg_explain_new_workspace_bytes, pcg_eval_workspace_bytes), score tables and outputs
(logits [n, 2], the ranked lists at their exact host-computed totals, d_self [n, F], d_agg [R, n, F] ...) have exactly the
documented size, start at an address that is 256 mod 512 and lie between guard words.  After every call (a) the whole arena
outside the buffers handed out still holds the guard pattern, and (b) every output is ``torch.equal`` to what a plain engine
returns for the same call (the guarded engine runs first: a call that oversteps fails there, before it runs without bands).

The case is tests/test_gpu_whole_set_driver.py's: 600 nodes with a hub row of more than 128 neighbours, 50 ids with duplicates
(a last dense tile of 2 rows), a query batch of 50 unseen nodes; chunks None (one chunk), 7 (seven and a tail of one) and 50.  A
new engine per chunk: a workspace only ever grows, so a second chunk size on the same engine would run inside the first one's.
One more run at (F, E, R) = (24, 16, 5): the forward-only dense kernel streams its weights there while the training kernel
stages them in LDS.

Run with ``pytest -m gpu`` on an MI355X."""
from unittest import mock

import numpy as np
import pytest
import torch

from tests.guarded import GuardedArena, guarded_allocations
from tests.util import synth_graph

pytestmark = pytest.mark.gpu

N, NQ, HUB = 600, 50, 7
PROJECT = (32, 64, (3, 10, 40))
STREAMED = (24, 16, (3, 10, 40, 6, 2))
MIB = 1 << 20


def dev():
    return torch.device("cuda", 0)


class Case:
    """the host side of a case: graph, parameters, the id list, the query batch's rows and lists, labels for ``evaluate``"""

    def __init__(self, F, emb, rel_deg):
        self.F, self.emb = F, emb
        self.X, self.labels, self.csrs = synth_graph(4, N, F, rel_deg, 0.15)
        self.train_pos = [int(v) for v in np.nonzero(self.labels[:N // 2])[0]]
        rs = np.random.RandomState(5)
        ids = np.concatenate([rs.randint(0, N, size=NQ - 5), [HUB, HUB, N - 1, 0, HUB]])
        rs.shuffle(ids)
        assert ids.size == NQ and np.unique(ids).size < NQ and NQ % 16 == 2
        self.ids = ids
        self.pairs = []
        for _ in self.csrs:
            rows = [np.concatenate([rs.randint(0, N + NQ, size=rs.randint(0, 30)), [N + j]]) for j in range(NQ)]
            self.pairs.append((np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64),
                               np.concatenate(rows).astype(np.int64)))
        self.qX = rs.randn(NQ, F).astype(np.float32)
        self.theta = None

    def engine(self):
        """(engine, query batch): new device objects over the same host data, the same parameters every time"""
        import pcgnn_amd as P
        from pcgnn_amd.fused import FusedPCGNN
        from pcgnn_amd.graph import QueryBatch
        g = P.DeviceGraph(self.X, self.csrs, self.train_pos, dev())
        assert g.max_degree > 128
        feats = torch.nn.Embedding(N, self.F)
        feats.weight = torch.nn.Parameter(torch.from_numpy(self.X), requires_grad=False)
        intras = [P.IntraAgg(feats, self.F, self.emb, self.train_pos, 0.5, cuda=True) for _ in self.csrs]
        inter = P.InterAgg(feats, self.F, self.emb, self.train_pos, g, intras, cuda=True)
        fz = FusedPCGNN(P.PCALayer(2, inter, 2.0).cuda(), 0.01, 0.001, max_batch=16)
        if self.theta is None:
            self.theta = fz.theta.clone()
        fz.theta.copy_(self.theta)
        fz.params_changed()
        return fz, QueryBatch(self.qX, self.pairs, g)


_CASES = {}


def case_of(shape):
    if shape not in _CASES:
        _CASES[shape] = Case(*shape)
    return _CASES[shape]


def chosen_tensors(out, tag, ch):
    out[f"{tag}: offsets"], out[f"{tag}: ids"], out[f"{tag}: dist"] = ch.flat_offsets, ch.ids, ch.dist


def attribution_tensors(out, tag, a):
    for name in ("logits", "d_self", "d_agg", "self_contrib", "rel_contrib", "neigh_contrib"):
        out[f"{tag}: {name}"] = getattr(a, name)
    chosen_tensors(out, f"{tag}: chosen", a.chosen)


def whole_set_calls(case, fz, query, chunk, check):
    out = {}
    ids = case.ids
    out["infer: gnn"], out["infer: center"] = fz.infer(ids, chunk=chunk, want_center=True)
    check("infer")
    chosen_tensors(out, "chosen", fz.chosen(ids, chunk=chunk))
    check("chosen")
    attribution_tensors(out, "attribute", fz.attribute(ids, chunk=chunk, neighbours=True))
    check("attribute(neighbours=True)")
    out["infer_new: gnn"], out["infer_new: center"] = fz.infer_new(query, chunk=chunk, want_center=True)
    check("infer_new")
    chosen_tensors(out, "chosen_new", fz.chosen_new(query, chunk=chunk))
    check("chosen_new")
    attribution_tensors(out, "attribute_new", fz.attribute_new(query, chunk=chunk, neighbours=True))
    check("attribute_new(neighbours=True)")
    metrics = fz.evaluate(ids, case.labels[ids], chunk=chunk)
    check("evaluate")
    assert int(fz._inf["status"].item()) == 0
    fz.check()
    return {k: v.clone() for k, v in out.items()}, metrics


def run_both(shape, chunk):
    from pcgnn_amd import ops
    case = case_of(shape)
    arena = GuardedArena(96 * MIB, dev())
    # (ops.eval_counts keeps one workspace per device: an empty cache for the guarded run, the old one back afterwards)
    with guarded_allocations(arena) as log, mock.patch.dict(ops._EVAL_CACHE, clear=True):
        fz, query = case.engine()
        arena.check("building the engine")
        got, got_metrics = whole_set_calls(case, fz, query, chunk, arena.check)
        inf, g, lib = fz._inf, fz.g, fz.lib
        c = NQ if chunk is None else chunk
        caps = lambda deg: int(np.add.reduceat(_row_caps(deg, fz.thresholds, case.ids), np.arange(0, NQ, c)).max())
        cap = caps(g.deg_host)
        # attribute's launches share infer's workspace, chosen has its own: each exactly what its size function says
        assert inf["ws"].untyped_storage().nbytes() == int(lib.pcg_infer_workspace_bytes(g.desc_ref(), fz.E, c, cap))
        assert inf["chosen_ws"].untyped_storage().nbytes() == int(lib.pcg_chosen_workspace_bytes(g.desc_ref(), c, cap))
        for t in (inf["ws"], inf["chosen_ws"], inf["new_ws"], inf["s0"], inf["new_s0"], inf["status"], fz.theta, g.X, query.X,
                  ops._EVAL_CACHE[("cuda", 0)]["ws"]):
            assert 0 < arena.offset_of(t) < arena.nbytes and t.data_ptr() % 512 == 256
        assert ops._EVAL_CACHE[("cuda", 0)]["ws"].numel() == int(lib.pcg_eval_workspace_bytes(NQ, 100))
        assert inf["s0"].numel() == N
    assert len(log) >= 20
    # (the plain engine second: a call that oversteps has failed above, between guard words, before it runs without them)
    want, want_metrics = whole_set_calls(case, *case.engine(), chunk, lambda what: None)
    assert list(got) == list(want)
    for k in want:
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), f"{k}: the guarded engine's bits differ from the plain engine's"
    assert got_metrics == want_metrics


def _row_caps(deg_host, thresholds, ids):
    from pcgnn_amd.fused import infer_row_caps
    return infer_row_caps(deg_host, thresholds, ids)


@pytest.mark.parametrize("chunk", [None, 7, 50])
def test_whole_set_calls_keep_their_extents(chunk):
    run_both(PROJECT, chunk)


def test_whole_set_calls_with_streamed_weights():
    """(24, 16, 5): infer_wlds is false while dense_wlds is true"""
    from tests import dense_ref as D
    assert D.dense_wlds(24, 16, 5)
    run_both(STREAMED, 7)
