"""Workspaces and output buffers may start dirty.  Run with ``pytest -m gpu`` on an MI355X.

``wholeset.py``, ``baseline.py``, ``ops.py`` and ``fused._alloc`` take their workspaces and outputs from ``torch.empty``.  In the
rest of the suite those are mostly fresh pages that read as zero; in a long-lived process they are recycled blocks that hold the
plans, look-back tags, tickets and partial sums of another call, chunk size or graph.  include/pcgnn.h promises "no initial
contents required" / "contents irrelevant on entry" for them ("What a call needs of the memory it starts from", is the
region-by-region reading of that promise).  Here every such call runs on memory that tests/dirty.py has filled:

  WORD3  the 32-bit word 3: a valid index, a denormal float, a value a look-back tag or a ticket really takes
  A5     bytes 0xA5: a negative int32, a tiny negative float
  NAN    float32 quiet NaN - only on buffers and regions that hold nothing but floats (outputs, s0, agg, slabs, clf_slots,
         acts, the per-chunk partial sums of a data part)

and every comparison is ``torch.equal`` on the raw bits with the same call on an engine whose workspace was zero-filled
("clean").  Each clean result is held once to the reference the suite already has for that call - float64 through
``dense_ref.tolerance`` (embed, attribute, the baselines, the training step), the exact host references (``ranked_ref``,
``eval_ref``, ``rank_eval_ref``, ``nearest_ref``) or the rebuilt graph (the query calls) - with the tolerances those tests use; no
tolerance is introduced here.

The whole-set calls run on ONE crafted graph (``DirtyCase``: 3001 nodes, R = 3): a hub whose chosen list has 350 entries (three
gather chunks: the dense launch adds up partial sums), an isolated node (count 0 in every relation), a node that is its own only
neighbour.  3003 ids at chunk 700 are four full chunks and a tail of 203 (both plan slots, plan tags 1 .. 4 in slot 0, n % 16
!= 0); feature widths 25 (stride 28), 32 and 260 (stride above 256), embedding sizes 16 and 64.  (260, 16, 3) leaves the
calls behind pcg_attr_set / pcg_explain_new out BY NAME (attribute, attribute_new, chosen_new): both return PCG_E_UNSUPPORTED
where the attribution tile's LDS does not fit (include/pcgnn.h) - rows of 260 floats fit at R = 1 only.

What these tests can and cannot see of the whole-set fronts' own zeroing (``infer_zero_regions``; profiles/r34/findings.txt has
the mutation runs).  The counters | heads region: seen, through ``heads_left`` - the plan sequence a call leaves counts from
whatever the word held, and at 36036 rows in one chunk (the only size at which the select launch pulls work units and touches
its shard heads and arrival counter) the fill's trace stays in those words - though the OUTPUTS are the same bits even then: a
unit handed out twice is selected twice, to the same list.  The PlanTotals look-back words: NOT seen.  A stale tag passes for a
published total only if a workgroup polls its predecessor before that predecessor has stored under the same tag, and it stores
before it polls anything itself; the word 3 meets the tag of the third plan into slot 0, but the window never opened.  For that
region the promise rests on the reading in DESIGN.md, not on a test.

Order: the WORD3 tests and the recycled sequences of a section come first, A5 after them, the NaN / -7 output tests last.
A test never passes vacuously: the buffer the second call used IS the one that was dirtied (``is`` and ``data_ptr()``), the
allocation log of a ``dirty_allocations`` block is non-empty with nothing unfilled, and no case is skipped at run time.
"""
import copy

import numpy as np
import pytest
import torch

from tests import baseline_ref as BR
from tests import baseline_train_ref as BTR
from tests import dense_ref as D
from tests import nearest_ref as NR
from tests import test_gpu_attribute as TA
from tests import test_gpu_embed as TE
from tests import train_adam_ref as T
from tests.dirty import A5, NAN, WORD3, dirty_, dirty_allocations, holds
from tests.eval_ref import counts_numpy, scores
from tests.grad_check import Tally
from tests.rank_eval_ref import alerts_numpy, pr_counts_numpy
from tests.ranked_ref import ranked_ref
from tests.util import build_model, synth_graph

pytestmark = pytest.mark.gpu

WS_FILLS = {"WORD3": WORD3, "A5": A5}
INT_OUT = -7                                     # what integer outputs start from in the output tests


def dev():
    return torch.device("cuda", 0)


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(got, want, what):
    """two dicts of tensors: the same keys, shapes, types and BITS (keys that start with "_" are not tensors)"""
    assert [k for k in got if k[0] != "_"] == [k for k in want if k[0] != "_"], what
    for k, w in want.items():
        if k[0] == "_":
            continue
        g = got[k]
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {k} is {tuple(g.shape)} {g.dtype}, clean {tuple(w.shape)} {w.dtype}"
        if not torch.equal(bits(g), bits(w)):
            bad = (bits(g) != bits(w)).reshape(-1).nonzero().flatten()
            raise AssertionError(f"{what}: {k} differs from clean in {bad.numel()} of {w.numel()} elements, first at {bad[:8].tolist()}")


def soil(buffers, fill):
    """every buffer zero-filled (fill None: the clean run) or dirtied; -> what `used` is checked against afterwards"""
    for b in buffers:
        if fill is None:
            b.zero_()
        else:
            dirty_(b, fill)
            assert bool(holds(b.view(-1)[:4096], fill).all())
    return [(b, b.data_ptr()) for b in buffers]


def used(marks, now):
    """the buffers a call used are the very objects that were dirtied: no silent reallocation"""
    assert len(marks) == len(now)
    for (b, ptr), n in zip(marks, now):
        assert n is b and n.data_ptr() == ptr, "the workspace was reallocated between the fill and the call"


def logged(log, at_least=1):
    """the allocation log of a dirty_allocations block: something was filled, nothing on the device went unfilled"""
    assert len(log) >= at_least, f"only {len(log)} device allocations were filled"
    assert not log.unfilled, f"device allocations that were not filled: {log.unfilled}"


# =====================================================================================================================================
# a. the whole-set calls on the crafted graph
# =====================================================================================================================================
N, HUB, ISOLATED, LONER, HUB_DEG, NQ = 3001, 7, 30, 31, 700, 333
CHUNK, CHUNK_NEW = 700, 100                      # 3003 ids: 4 x 700 + 203;  333 query rows: 3 x 100 + 33
A_SHAPES = [(25, 64, 3), (32, 16, 3), (260, 16, 3)]
IDS = lambda s: "x".join(map(str, s))


class DirtyCase(D.GradCase):
    """``synth_graph`` over 3001 nodes with three crafted rows: HUB keeps 350 of 700 neighbours in relation 1 (three gather
    chunks), ISOLATED has an empty row in every relation, LONER's only neighbour is itself"""

    def __init__(self, F, E, R=3, seed=11):
        super().__init__(F, E, R, seed=seed)
        self.n = N
        self.X, self.labels, csrs = synth_graph(seed + 1, N, F, D.REL_DEG[R], 0.15)
        self.train_pos = [int(v) for v in range(N // 2) if self.labels[v] == 1]
        rs = np.random.RandomState(seed + 5)
        self.csr = []
        for r, (indptr, idx) in enumerate(csrs):
            rows = [idx[indptr[v]:indptr[v + 1]] for v in range(N)]
            rows[ISOLATED] = np.zeros(0, np.int32)
            rows[LONER] = np.array([LONER], np.int32)
            if r == 1:
                rows[HUB] = np.sort(rs.choice(N, size=HUB_DEG, replace=False)).astype(np.int32)
            ip = np.zeros(N + 1, dtype=np.int64)
            np.cumsum([len(x) for x in rows], out=ip[1:])
            self.csr.append((ip, np.concatenate(rows).astype(np.int32)))

    def main_ids(self):
        """every node once, shuffled, and the hub twice more: 3003 ids"""
        return np.concatenate([np.random.RandomState(3).permutation(N), [HUB, HUB]]).astype(np.int64)

    def other_ids(self):
        """another set: 1500 draws with replacement and the isolated node, 2 x 700 + 101"""
        return np.concatenate([np.random.RandomState(4).randint(0, N, size=1500), [ISOLATED]]).astype(np.int64)


def new_engine(c, max_batch=256, **kw):
    import pcgnn_amd as P
    from pcgnn_amd.fused import FusedPCGNN
    m = build_model(P, c, c.rho, graph=P.DeviceGraph(c.X, c.csr, c.train_pos, dev()))
    return FusedPCGNN(m, c.lr, c.wd, betas=c.betas, max_batch=max_batch, **kw)


class Setup:
    """one case per shape: a clean and a dirty engine on the crafted graph, a query batch of NQ unseen nodes for each, and the
    engine of the graph rebuilt with the query rows appended (the query calls' reference)"""

    def __init__(self, shape):
        from pcgnn_amd.graph import QueryBatch
        from tests.test_gpu_infer_new import append_rows, split
        c = self.c = DirtyCase(*shape)
        # NQ unseen nodes, directed rows (the crafted rows stay what they are): lists into the graph, among themselves and the
        # node itself; query row 0 is empty, row 1 keeps 300 of 600 (three gather chunks)
        rs = np.random.RandomState(21)
        rows = []
        for r in range(c.R):
            rel = [np.concatenate([rs.randint(0, N + NQ, size=rs.randint(0, 30)), [N + j]]) for j in range(NQ)]
            rel[0] = np.zeros(0, np.int64)
            if r == 1:
                rel[1] = rs.choice(N + NQ, size=600, replace=False)
            rows.append(rel)
        Xf, full_csr = append_rows(c.X, c.csr, rs.randn(NQ, c.f), rows)
        _, base_csr, Xq, q_pairs = split(Xf, full_csr, c.n)
        for (ip, ix), (bp, bx) in zip(c.csr, base_csr):
            assert np.array_equal(ip, bp) and np.array_equal(ix, bx), "the base rows of the rebuilt graph are the crafted graph's"
        full = copy.copy(c)
        full.n, full.X, full.csr = c.n + NQ, Xf, full_csr
        self.engine = {role: new_engine(c) for role in ("clean", "dirty")}
        self.full = new_engine(full)
        self.query = {role: QueryBatch(Xq, q_pairs, fz.g) for role, fz in self.engine.items()}
        self.ids = {"main": c.main_ids(), "other": c.other_ids(), "big": np.tile(c.main_ids(), BIG_REPEAT)}
        self.qids = {"main": None, "other": np.arange(NQ)[::-1][:200].copy()}
        self.clean, self.held = {}, False
        hub_kept = -(-HUB_DEG // 2)
        assert hub_kept > 256 and -(-hub_kept // 128) >= 3 and len(self.ids["main"]) % 16 != 0 and len(self.ids["main"]) % CHUNK != 0


_SETUPS = {}


def setup_of(shape):
    if shape not in _SETUPS:
        _SETUPS[shape] = Setup(shape)
    return _SETUPS[shape]


def _chosen(ch, prefix=""):
    return {prefix + "offsets": torch.from_numpy(np.asarray(ch.host_offsets()).astype(np.int64)), prefix + "ids": ch.ids,
            prefix + "dist": ch.dist, "_" + prefix + "lists": ch}


def _attribution(at):
    out = {k: getattr(at, k) for k in ("logits",) + TA.KEYS}
    out.update(_chosen(at.chosen, "chosen "))
    out["neigh_contrib"] = at.neigh_contrib
    out["_attribution"] = at
    return out


def _resident(method):
    def call(s, role, which, chunk):
        ids = s.ids[which]
        return method(s.engine[role], ids, (len(ids) if which == "big" else CHUNK) if chunk is None else chunk)   # ("big": ONE chunk)
    return call


def _query(method):
    def call(s, role, which, chunk):
        return method(s.engine[role], s.query[role], s.qids[which], CHUNK_NEW if chunk is None else chunk)
    return call


# name -> (the keys of FusedPCGNN._inf the call's workspaces live under, the call -> a dict of its outputs)
CALLS = {
    "infer": (("ws",), _resident(lambda fz, ids, ch: dict(zip(("gnn", "center"), fz.infer(ids, chunk=ch, want_center=True))))),
    "embed": (("ws",), _resident(lambda fz, ids, ch: dict(zip(("emb", "h", "logits"),
                                                             fz.embed(ids, chunk=ch, relations=True, want_logits=True))))),
    "chosen": (("chosen_ws",), _resident(lambda fz, ids, ch: _chosen(fz.chosen(ids, chunk=ch)))),
    "attribute": (("ws", "chosen_ws"), _resident(lambda fz, ids, ch: _attribution(fz.attribute(ids, chunk=ch, neighbours=True)))),
    "infer_new": (("new_ws",), _query(lambda fz, q, ids, ch: dict(zip(("gnn", "center"),
                                                                      fz.infer_new(q, ids=ids, chunk=ch, want_center=True))))),
    "embed_new": (("new_ws",), _query(lambda fz, q, ids, ch: dict(zip(("emb", "h", "logits"),
                                                                      fz.embed_new(q, ids=ids, chunk=ch, relations=True, want_logits=True))))),
    "chosen_new": (("new_ws",), _query(lambda fz, q, ids, ch: _chosen(fz.chosen_new(q, ids=ids, chunk=ch)))),
    "attribute_new": (("new_ws",), _query(lambda fz, q, ids, ch: _attribution(fz.attribute_new(q, ids=ids, chunk=ch, neighbours=True)))),
}
# left out by name, not skipped: the attribution tile of rows of 260 floats does not fit the LDS at R = 3 - pcg_attr_set returns
# PCG_E_UNSUPPORTED, and so does pcg_explain_new, whichever of its output groups is asked for (chosen_new goes through it)
NOT_SUPPORTED = {(260, 16, 3): ("attribute", "attribute_new", "chosen_new")}
A_CASES = [(shape, name) for shape in A_SHAPES for name in CALLS if name not in NOT_SUPPORTED.get(shape, ())]
A_IDS = [f"{IDS(shape)}-{name}" for shape, name in A_CASES]


def settled(fz):
    """the status word of the whole-set calls is zero and the engine's own check passes"""
    assert int(fz._inf["status"].item()) == 0, "the whole-set status word"
    fz.check()


def clean_of(shape, name, which="main"):
    """the call on the clean engine with its workspaces zero-filled, computed once"""
    s = setup_of(shape)
    if (name, which) not in s.clean:
        fz = s.engine["clean"]
        keys, call = CALLS[name]
        call(s, "clean", which, None)                                  # (the workspaces exist at the size the call needs)
        marks = soil([fz._inf[k] for k in keys], None)
        s.clean[(name, which)] = call(s, "clean", which, None)
        used(marks, [fz._inf[k] for k in keys])
        settled(fz)
    return s.clean[(name, which)]


def hold_to_references(shape):
    """the clean results of a shape against what the suite holds these calls to, once"""
    s = setup_of(shape)
    if s.held:
        return
    c, fz, ids = s.c, s.engine["clean"], s.ids["main"]
    n = len(ids)
    tally = Tally(f"{shape} clean whole-set calls")
    # chosen: the exact host reference on the scores the call selected by
    ch = clean_of(shape, "chosen")
    off, ref_ids, ref_dist = ranked_ref(c.csr, ids, fz._inf["s0"].cpu().numpy(), fz.thresholds)
    lists = ch["_lists"]
    assert np.array_equal(lists.offsets.cpu().numpy(), off) and np.array_equal(ch["ids"].cpu().numpy(), ref_ids)
    assert np.array_equal(ch["dist"].cpu().numpy().view(np.uint32), ref_dist.view(np.uint32))
    h_off = np.asarray(lists.host_offsets())
    at = int(np.nonzero(ids == HUB)[0][0])
    assert h_off[n + at + 1] - h_off[n + at] == -(-HUB_DEG // 2) > 256, "the hub's chosen list spans three gather chunks"
    for v, want in ((ISOLATED, 0), (LONER, 1)):
        at = int(np.nonzero(ids == v)[0][0])
        assert all(h_off[r * n + at + 1] - h_off[r * n + at] == want for r in range(c.R)), (v, want)
    # embed / infer: float64 with the device's lists as the selection; the isolated node's rows (0 / 0 aggregates) are left out
    emb = clean_of(shape, "embed")
    inf = clean_of(shape, "infer")
    keep = torch.from_numpy(ids != ISOLATED)
    assert torch.equal(bits(inf["gnn"]), bits(emb["logits"]))
    assert bool(torch.isfinite(emb["emb"][keep.to(dev())]).all())
    r64, r32 = TE.forward_refs(c, ids, TE.index_of(lists))
    r64, r32 = ({"pre": [p[keep] for p in r["pre"]], "logits": r["logits"][keep]} for r in (r64, r32))
    b = TE.bounds(r64, r32)
    for t, got in enumerate([emb["h"][:, r, :] for r in range(c.R)] + [emb["emb"]]):
        TE.check_activation(f"{shape} " + (f"h_{t + 1}" if t < c.R else "emb"), got.cpu()[keep], *b[t])
    tally.check("logits", emb["logits"].cpu()[keep], r64["logits"], r32["logits"])
    p = c.params()
    x = torch.from_numpy(c.X[ids])
    center = {dt: x.to(dt) @ p["inter1.label_clf.weight"].to(dt).t() + p["inter1.label_clf.bias"].to(dt) for dt in (torch.float64, torch.float32)}
    tally.check("centre logits", inf["center"], center[torch.float64], center[torch.float32])
    # attribute: float64 on a tile-ragged subset (hub, loner and ordinary rows), whose rows are the whole call's bit for bit
    if "attribute" not in NOT_SUPPORTED.get(shape, ()):
        whole = clean_of(shape, "attribute")
        assert torch.equal(bits(whole["logits"]), bits(inf["gnn"]))
        at = np.concatenate([np.nonzero(ids == HUB)[0][:1], np.nonzero(ids == LONER)[0], np.nonzero(ids != ISOLATED)[0][:63]])
        sub = ids[at]
        res = fz.attribute(sub, neighbours=True)
        rows = torch.from_numpy(at).to(dev())
        for k in ("logits", "d_self", "self_contrib"):
            assert torch.equal(bits(getattr(res, k)), bits(whole[k][rows])), k
        for k in ("d_agg", "rel_contrib"):
            assert torch.equal(bits(getattr(res, k)), bits(whole[k][:, rows])), k
        for target in ((0.0, 1.0),):
            _, index, a64, a32, kept, share = TA.references(c, fz, sub, target)
            TA.check_against_float64(tally, f"target {target}", res, a64, a32, kept, share, target)
            TA.check_neighbours(tally, f"target {target}", res, index, a64, a32, kept)
    # the query calls: the rebuilt graph's rows N .. N + NQ - 1, bit for bit
    gids = torch.arange(c.n, c.n + NQ, dtype=torch.int32, device=dev())
    new = clean_of(shape, "infer_new")
    gnn, cen = s.full.infer(gids, want_center=True)
    assert torch.equal(bits(new["gnn"]), bits(gnn)) and torch.equal(bits(new["center"]), bits(cen))
    enew = clean_of(shape, "embed_new")
    e, h, lg = s.full.embed(gids, relations=True, want_logits=True)
    assert torch.equal(bits(enew["emb"]), bits(e)) and torch.equal(bits(enew["h"]), bits(h)) and torch.equal(bits(enew["logits"]), bits(lg))
    if "attribute_new" not in NOT_SUPPORTED.get(shape, ()):
        cnew = clean_of(shape, "chosen_new")
        fch = s.full.chosen(gids)
        assert np.array_equal(np.asarray(fch.host_offsets()), cnew["offsets"].numpy())
        assert torch.equal(cnew["ids"], fch.ids) and torch.equal(bits(cnew["dist"]), bits(fch.dist))
        anew = clean_of(shape, "attribute_new")
        fat = s.full.attribute(gids, neighbours=True)
        for k in ("logits",) + TA.KEYS + ("neigh_contrib",):
            assert torch.equal(bits(anew[k]), bits(getattr(fat, k))), k
        assert torch.equal(anew["chosen ids"], fch.ids)
    settled(fz)
    settled(s.full)
    tally.done()
    s.held = True


def nan_partial_sums(fz, ws, ids_host, chunk):
    """the per-chunk partial sums of a resident call's data part - floats only (pcg_choose_workspace_offset(..., 6)) - as NaN on
    top of the integer fill: a float of 3 or 0xA5A5A5A5 vanishes in any sum, a NaN does not.  ws = [plan slot | plan slot |
    data part: list, partial sums [chunks][stride], .. | agg | cnt | centre]; the tail chunk's partial sums start at the same
    byte (the list in front of them has the call's capacity whatever the rows)"""
    from pcgnn_amd import wholeset as WS
    g, lib = fz.g, fz.lib
    _, cap = WS.infer_chunks(WS.infer_row_caps(g.deg_host, fz.thresholds, ids_host), chunk)
    plan = int(lib.pcg_choose_plan_bytes(g.desc_ref(), chunk, cap))
    lo = plan + int(lib.pcg_choose_workspace_offset(g.desc_ref(), chunk, cap, 6))          # (2 * plan + (offset - plan))
    nbytes = 4 * (cap // 128 + g.R * chunk + 1) * g.X.stride(0)
    assert plan > 0 and lo % 256 == 0 and lo + nbytes < ws.numel()
    dirty_(ws[lo:lo + nbytes], NAN)


def heads_left(ws, n, chunk, what):
    """What a call leaves in the words of plan slot 0 that no plan launch rewrites (csrc/choose.h: `heads`, the 128 words at
    byte 256 of the slot, which is the first thing in the workspace): the select launches' shard heads, cursor and arrival
    counters back at zero, and heads[12] - the plan sequence - equal to the number of full chunks planned into the slot.  The
    front launch zeroes these words; a call that started from whatever they held leaves the fill's trace here."""
    h = ws[256:768].view(torch.int32).cpu().numpy()
    full = -(-n // chunk) - (1 if n % chunk else 0)
    assert h[12] == full, f"{what}: plan sequence {h[12]} after {full} plans into slot 0"
    assert not h[0::16].any() and not h[13:16].any(), f"{what}: heads {h[0::16].tolist()}, counters {h[13:16].tolist()} left behind"


def dirtied_call(shape, name, fill, which="main"):
    """call -> dirty_ its workspaces -> call again -> equal to clean"""
    hold_to_references(shape)
    s = setup_of(shape)
    fz = s.engine["dirty"]
    keys, call = CALLS[name]
    want = clean_of(shape, name, which)
    same(call(s, "dirty", which, None), want, f"{name}, first call")
    marks = soil([fz._inf[k] for k in keys], fill)
    if name in ("infer", "embed", "attribute"):
        nan_partial_sums(fz, fz._inf["ws"], s.ids[which], len(s.ids[which]) if which == "big" else CHUNK)
    got = call(s, "dirty", which, None)
    used(marks, [fz._inf[k] for k in keys])
    same(got, want, f"{name} on a workspace filled with {fill.hex()}")
    n, chunk = (NQ, CHUNK_NEW) if name.endswith("_new") else (len(s.ids[which]), len(s.ids[which]) if which == "big" else CHUNK)
    for k in keys:
        heads_left(fz._inf[k], n, chunk, f"{name}, {k}, fill {fill.hex()}")
    settled(fz)


@pytest.mark.parametrize("shape,name", A_CASES, ids=A_IDS)
def test_whole_set_call_on_a_workspace_of_word3(shape, name):
    dirtied_call(shape, name, WORD3)


@pytest.mark.parametrize("shape", A_SHAPES, ids=IDS)
def test_whole_set_calls_on_recycled_workspaces(shape):
    """no fill at all: what one call leaves is what the next one finds - another chunk size (another layout over the same
    bytes), another id set, another entry point on the same workspace, the same call five times"""
    hold_to_references(shape)
    s = setup_of(shape)
    fz = s.engine["dirty"]
    names = [n for n in CALLS if n not in NOT_SUPPORTED.get(shape, ())]
    run = lambda name, which="main", chunk=None: CALLS[name][1](s, "dirty", which, chunk)
    for name in names:                                                # chunk 700 -> 64 -> 700 (query rows: 100 -> 64 -> 100)
        for chunk in (None, 64, None):
            same(run(name, chunk=chunk), clean_of(shape, name), f"{name}, chunk {chunk}")
            settled(fz)
    for name in ("infer", "chosen", "infer_new"):                     # another id set in between
        same(run(name, "other"), clean_of(shape, name, "other"), f"{name}, the other ids")
        same(run(name), clean_of(shape, name), f"{name}, after the other ids")
        settled(fz)
    order = [n for n in ("infer", "chosen", "attribute", "embed", "infer") if n in names]
    for name in order:                                                # entry points that share a workspace, one after the other
        same(run(name), clean_of(shape, name), f"{name} in {order}")
    for name in [n for n in ("infer_new", "chosen_new", "embed_new", "infer_new") if n in names]:
        same(run(name), clean_of(shape, name), f"{name} among the query calls")
    settled(fz)
    for name in ("infer", "chosen", "infer_new"):                     # five times in a row
        for k in range(5):
            same(run(name, chunk=64), clean_of(shape, name), f"{name}, call {k + 1} of five")
    settled(fz)


@pytest.mark.parametrize("shape,name", A_CASES, ids=A_IDS)
def test_whole_set_call_on_a_workspace_of_a5(shape, name):
    dirtied_call(shape, name, A5)


# ---- one chunk of many rows: the select launch has more work units than workgroups and PULLS them -----------------------------------
# The crafted graph's 3003 ids four times over in ONE chunk: 36036 rows.  Only then does the select launch touch the words of the
# plan slot that no plan rewrites - its shard heads are advanced by atomics and heads[15] counts the workgroups out, the last of
# which puts them all back to zero (select_rows_body) - so only here does a call START from whatever those words hold.  Its
# outputs do not depend on them (an early reset hands units out twice: the same lists twice); what it LEAVES there does
# (heads_left).
BIG_REPEAT, BIG_SHAPE, BIG_CALLS, SEL_GRID = 4, (32, 16, 3), ("infer", "chosen"), 768


def select_units(c, ids):
    """select_rows_body's count of work units for one chunk of test-mode rows, restated: rows of up to 16 neighbours go four
    to an item, up to 512 one each, eight items at most to a unit; longer rows are units of their own"""
    deg = np.concatenate([np.diff(ip)[ids] for ip, _ in c.csr])
    n_wg, n_items = int((deg > 512).sum()), int(((deg > 16) & (deg <= 512)).sum()) + (int((deg <= 16).sum()) + 3) // 4
    avail = max(SEL_GRID - n_wg, SEL_GRID // 4)
    per_unit = min(max(-(-n_items // avail), 1), 8)
    return n_wg + -(-n_items // per_unit)


def big_clean(name):
    """the one-chunk call on the clean engine, zero-filled workspace; tied to the referenced results: a row's values do not depend
    on its position or company, so the result is the main set's four times over"""
    s = setup_of(BIG_SHAPE)
    first = (name, "big") not in s.clean
    want, small = clean_of(BIG_SHAPE, name, "big"), clean_of(BIG_SHAPE, name)
    if first:
        assert select_units(s.c, s.ids["big"]) > SEL_GRID, "the select launch of this chunk pulls its units"
        if name == "infer":
            for k in ("gnn", "center"):
                assert torch.equal(bits(want[k]), bits(small[k].repeat(BIG_REPEAT, 1))), k
        else:
            n, off_b, off_s = len(s.ids["main"]), want["offsets"].numpy(), small["offsets"].numpy()
            for r in range(s.c.R):
                lo_b, hi_b = int(off_b[r * BIG_REPEAT * n]), int(off_b[(r + 1) * BIG_REPEAT * n])
                lo_s, hi_s = int(off_s[r * n]), int(off_s[(r + 1) * n])
                for k in ("ids", "dist"):
                    assert torch.equal(bits(want[k][lo_b:hi_b]), bits(small[k][lo_s:hi_s].repeat(BIG_REPEAT))), (k, r)
    return want


@pytest.mark.parametrize("name", BIG_CALLS)
def test_one_chunk_of_many_rows_on_a_workspace_of_word3(name):
    big_clean(name)
    dirtied_call(BIG_SHAPE, name, WORD3, "big")


def test_one_chunk_of_many_rows_on_recycled_workspaces():
    """no fill: the large chunk, chunk 700 over the same bytes, the large chunk again; twice in a row; the other entry point"""
    hold_to_references(BIG_SHAPE)
    s = setup_of(BIG_SHAPE)
    fz = s.engine["dirty"]
    for name in BIG_CALLS:
        want = big_clean(name)
        run = lambda chunk=None: CALLS[name][1](s, "dirty", "big", chunk)
        for chunk in (None, CHUNK, None, None):
            same(run(chunk), want, f"{name}, {len(s.ids['big'])} ids, chunk {chunk}")
            settled(fz)
    same(CALLS["infer"][1](s, "dirty", "big", None), big_clean("infer"), "infer behind chosen")
    settled(fz)


@pytest.mark.parametrize("name", BIG_CALLS)
def test_one_chunk_of_many_rows_on_a_workspace_of_a5(name):
    big_clean(name)
    dirtied_call(BIG_SHAPE, name, A5, "big")


# =====================================================================================================================================
# b. the GraphSAGE / GCN baselines
# =====================================================================================================================================
B_CASES = [(25, 64, "sage_concat"), (32, 128, "gcn")]               # GraphSAGE, GCN
B_STEPS = (1025, 17, 2049)                                           # two weight-GEMM parts, one ragged tile, three parts
_BASELINE_CLEAN = {}


def baseline_ids():
    """the crafted rows (the empty one and the 5000-row among them) and 1500 draws: 2 x 700 + 160"""
    return np.concatenate([np.arange(60), np.random.RandomState(8).randint(0, BTR.N, size=1500)]).astype(np.int64)


def baseline_run(F, E, shape, fill, hold=False):
    """infer, embed(aggregates=True), loss_and_grad and three train_steps of a fresh model, the engine's two workspaces
    zero-filled (fill None) or dirtied before every call; hold: the clean results against float64"""
    from tests import test_gpu_baseline_train as BT
    model = BT.trainable(F, E, shape)
    eng = model.engine()
    ids = baseline_ids()
    model.infer(ids, chunk=CHUNK)
    model.loss_and_grad(*BTR.batch(max(B_STEPS), 1))                  # (both workspaces exist at their largest size)
    buffers = [eng._inf["ws"], eng._inf["train_ws"]]
    out = {}
    marks = soil(buffers, fill)
    now = lambda: [eng._inf["ws"], eng._inf["train_ws"]]
    out["infer"] = model.infer(ids, chunk=CHUNK)
    used(marks, now())
    marks = soil(buffers, fill)
    out["h"], out["logits"], out["agg"] = model.embed(ids, chunk=CHUNK, want_logits=True, aggregates=True)
    used(marks, now())
    g_ids, g_lab = BTR.batch(1025, BTR.salt_of(F, E, shape))           # (test_gradients_against_float64's batch of 1025)
    mask = model.embed(g_ids, chunk=CHUNK) > 0                          # (chunk: within the workspace at hand)
    marks = soil(buffers, fill)
    out["loss"], out["d_enc"], out["d_cls"] = model.loss_and_grad(g_ids, g_lab)
    out["d_enc"], out["d_cls"] = out["d_enc"].clone(), out["d_cls"].clone()
    used(marks, [eng._inf["ws"], eng._inf["train_ws"]])
    if hold:
        W_enc, W_cls = BTR.model_weights(F, E, shape)
        tally = Tally(f"baseline F={F} E={E} {shape} clean")
        empty = ids == BTR.EMPTY_NODE if not BR.SHAPES[shape]["add_self"] else np.zeros(len(ids), bool)   # (add_self: it has itself)
        ok = ~empty
        r64 = BR.forward(BTR.features(F), BTR.csr(), ids, W_enc, W_cls, dtype=np.float64, **BR.SHAPES[shape])
        r32 = BR.forward(BTR.features(F), BTR.csr(), ids, W_enc, W_cls, dtype=np.float32, **BR.SHAPES[shape])
        assert bool(torch.isnan(out["agg"][torch.from_numpy(empty).to(dev())]).all()), "the empty row's aggregate is 0 / 0"
        for k, j in (("logits", 0), ("h", 1), ("agg", 2)):
            tally.check(k, out[k].cpu()[ok], torch.from_numpy(r64[j][ok]), torch.from_numpy(r32[j][ok]))
        assert torch.equal(bits(out["infer"]), bits(out["logits"]))
        g64, g32, share, wrong = BTR.reference_pair(F, shape, g_ids, g_lab, W_enc, W_cls, mask)
        assert share <= D.AMBIGUOUS_CAP and wrong == 0, (share, wrong)
        for k in ("loss", "d_enc", "d_cls"):
            tally.check(k, out[k], torch.as_tensor(g64[k]), torch.as_tensor(g32[k]))
        tally.done()
    for k, B in enumerate(B_STEPS):
        marks = soil(buffers, fill)
        out[f"step {k + 1} loss"] = model.train_step(*BTR.batch(B, 3 + k)).clone()
        used(marks, [eng._inf["ws"], eng._inf["train_ws"]])
    state, step = BT.state_of(model)
    assert step == len(B_STEPS)
    for name, t in zip(("W_enc", "W_cls", "m_enc", "v_enc", "m_cls", "v_cls"), state):
        out[name] = t
    model.check()
    return out


def baseline_clean(case):
    if case not in _BASELINE_CLEAN:
        _BASELINE_CLEAN[case] = baseline_run(*case, None, hold=True)
    return _BASELINE_CLEAN[case]


@pytest.mark.parametrize("case", B_CASES, ids=IDS)
def test_baseline_calls_on_workspaces_of_word3(case):
    same(baseline_run(*case, WORD3), baseline_clean(case), f"baseline {case}, WORD3")


@pytest.mark.parametrize("case", B_CASES, ids=IDS)
def test_baseline_calls_on_workspaces_of_a5(case):
    same(baseline_run(*case, A5), baseline_clean(case), f"baseline {case}, A5")


# =====================================================================================================================================
# c. device metrics and search: sizes on both sides of each kernel's one-workgroup limit, k > n and M < k
# =====================================================================================================================================
def _on_dev(prob, y):
    return torch.from_numpy(prob).to(dev()), torch.from_numpy(y.astype(np.int32)).to(dev())


def _eval_case(n):
    from pcgnn_amd import ops
    prob, y = scores(n, 0.145, n % 1000 + 7, "tied")
    p, l = _on_dev(prob, y)
    want = counts_numpy(prob, y, None)
    return dict(key="ws", cache=lambda: ops._eval_cache(dev()), run=lambda: {"out": ops.eval_counts(p, l)},
                hold=lambda got: np.array_equal(got["out"].cpu().numpy().view(np.uint64), want))


def _pr_case(n, n1):
    from pcgnn_amd import ops
    from tests.test_gpu_rank_eval import with_positives
    prob, y = with_positives(n, n1, "tied", 5)
    p, l = _on_dev(prob, y)
    w_hdr, w_tp, w_np = pr_counts_numpy(prob, y)
    G = int(w_hdr[6])

    def run():
        hdr, tp, npred = ops.pr_counts(p, l)
        # written: hdr and the first G entries; past G the header documents nothing ("_tail": what the output test looks at)
        return {"hdr": hdr, "tp": tp[:G], "npred": npred[:G], "_tail": (tp[G:], npred[G:])}

    def hold(got):
        return (np.array_equal(got["hdr"].cpu().numpy().view(np.uint64), w_hdr) and np.array_equal(got["tp"].cpu().numpy().view(np.uint32), w_tp)
                and np.array_equal(got["npred"].cpu().numpy().view(np.uint32), w_np) and 0 < G < n)
    return dict(key="pr_ws", cache=lambda: ops._eval_cache(dev()), run=run, hold=hold)


def _alerts_case(n, k):
    from pcgnn_amd import ops
    prob, _ = scores(n, 0.145, n + 7, "tied")
    p = torch.from_numpy(prob).to(dev())
    w_pos, w_score = alerts_numpy(np.ascontiguousarray(prob[:, 1]), k)
    ke = min(n, k)

    def hold(got):
        pos, score = got["pos"].cpu().numpy(), got["score"].cpu().numpy()
        return (np.array_equal(pos[:ke], w_pos[:ke]) and np.array_equal(score[:ke].view(np.uint32), w_score[:ke].view(np.uint32))
                and bool(np.all(pos[ke:] == -1)) and bool(np.all(np.isneginf(score[ke:]))))
    return dict(key="alerts_ws", cache=lambda: ops._eval_cache(dev()), run=lambda: dict(zip(("pos", "score"), ops.topk_alerts(p, k))), hold=hold)


def _similar_case(n, M, E, k):
    from pcgnn_amd import ops
    rs = np.random.RandomState(n + M + k)
    Q, bank = (rs.randint(-3, 4, size=(r, E)).astype(np.float32) for r in (n, M))
    q, b = torch.from_numpy(Q).to(dev()), torch.from_numpy(bank).to(dev())
    w_pos, w_score = NR.topk_similar_ref(Q, bank, k, "dot", None, None)

    def hold(got):
        return (np.array_equal(got["pos"].cpu().numpy(), w_pos) and np.array_equal(got["score"].cpu().numpy().astype(np.float64), w_score)
                and (M >= k or bool((got["pos"][:, M:] == -1).all())))
    return dict(key="ws", cache=lambda: ops._TOPK_CACHE[("cuda", 0)], run=lambda: dict(zip(("pos", "score"), ops.topk_similar(q, b, k, "dot"))),
                hold=hold)


C_CASES = {
    "eval_counts n=1000": lambda: _eval_case(1000),
    "eval_counts n=131073": lambda: _eval_case(131_073),             # past 2 x 65536: the tiled sort
    "pr_counts n=2049": lambda: _pr_case(2049, 300),
    "pr_counts n=70000": lambda: _pr_case(70_000, 65_537),            # one more positive than one workgroup sorts
    "topk_alerts n=65 k=1000": lambda: _alerts_case(65, 1000),        # k > n: padding entries
    "topk_alerts n=70000 k=1000": lambda: _alerts_case(70_000, 1000),
    "topk_similar M=15 k=20": lambda: _similar_case(100, 15, 64, 20),  # M < k: padding entries, one slice
    "topk_similar M=4099 k=8": lambda: _similar_case(17, 4099, 128, 8),  # several slices and the merge launch
}
_C_MADE = {}


def metric_case(name):
    """the case's inputs, its clean result (workspace zero-filled) held to the exact host reference; made once"""
    if name not in _C_MADE:
        case = C_CASES[name]()
        case["run"]()                                                  # (the cached workspace exists at this size)
        ws = case["cache"]()[case["key"]]
        marks = soil([ws], None)
        case["clean"] = case["run"]()
        used(marks, [case["cache"]()[case["key"]]])
        assert case["hold"](case["clean"]), f"{name}: the clean result is not the host reference's"
        _C_MADE[name] = case
    return _C_MADE[name]


def metric_on(name, fill):
    from pcgnn_amd import ops
    case = metric_case(name)
    case["run"]()                                                      # (another case may have grown the workspace since)
    marks = soil([case["cache"]()[case["key"]]], fill)
    got = case["run"]()
    used(marks, [case["cache"]()[case["key"]]])
    same(got, case["clean"], f"{name} on a workspace filled with {fill.hex()}")
    status = ops.eval_status(dev())
    assert int(status.item()) == 0, "the metrics' status word"


@pytest.mark.parametrize("name", list(C_CASES))
def test_metric_call_on_a_workspace_of_word3(name):
    metric_on(name, WORD3)


@pytest.mark.parametrize("name", list(C_CASES))
def test_metric_call_on_a_workspace_of_a5(name):
    metric_on(name, A5)


# =====================================================================================================================================
# e. the training engine: every torch.empty buffer of _alloc dirty, the zeroed-once buffers never zeroed again
# =====================================================================================================================================
STATE = ("theta", "m", "v", "clf_next", "step_counter")
TRAIN_SHAPE = (10, 16, 1)                                             # train_adam_ref's small case
# train_adam_ref.SEQUENCE rotated by one, on an engine of max_batch 1025: _alloc runs again at 2048 and at 2049, mid-sequence
TRAIN_ORDER = (1, 2, 3, 4, 5, 6, 7, 8, 9, 0)


def on_dev(ids, lab):
    return torch.from_numpy(np.asarray(ids).astype(np.int32)).to(dev()), torch.from_numpy(np.asarray(lab).astype(np.int32)).to(dev())


def soil_engine(fz):
    """what the header says needs no initial contents and ``_alloc`` zeroes all the same: the data part (the selection list is
    int32: WORD3) and the transposed activations (floats: NaN)"""
    dirty_(fz.data, WORD3)
    # ... its partial sums (floats only; behind them: the reserved row tickets and - rows beyond 32768 neighbours only - key scratch)
    g = fz.g
    assert g.max_degree <= 32768
    lo = int(fz.lib.pcg_choose_workspace_offset(g.desc_ref(), fz.maxB, fz.list_capacity, 6)) - fz._plan_bytes(fz.maxB)
    assert 0 < lo < fz.data.numel() and lo % 256 == 0
    dirty_(fz.data[lo:], NAN)
    dirty_(fz.acts, NAN)


def state_same(a, b, what):
    torch.cuda.synchronize()
    for fz in (a, b):
        fz.check()
    for name in STATE:
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(bits(x), bits(y)), f"{what}: {name} differs in {int((bits(x) != bits(y)).sum())} entries"


def test_train_steps_on_a_dirty_engine():
    """ten train_step(defer=True) and a flush, _alloc twice on the way, everything inside the block"""
    c = D.GradCase.of(TRAIN_SHAPE)
    batches = [on_dev(*T.step_batch(c, "sequence", k)) for k in TRAIN_ORDER]
    assert [b[0].numel() for b in batches].index(2048) == 4

    def run(fz, soiled):
        grown = []
        for ids, lab in batches:
            if ids.numel() > fz.maxB:                                  # (_alloc runs here: flush, every buffer anew)
                fz._fit(ids.numel())
                grown.append(ids.numel())
                if soiled:
                    soil_engine(fz)
            fz.train_step(ids, lab, defer=True)
        fz.flush()
        return grown

    clean = new_engine(c, 1025)
    hold_first_step(c, on_dev(*T.step_batch(c, "sequence", 0)))
    assert run(clean, False) == [2048, 2049]
    with dirty_allocations(NAN, int_fill=WORD3) as log:
        dirty = new_engine(c, 1025)
        soil_engine(dirty)
        grown = run(dirty, True)
    logged(log, at_least=24)                                           # (_alloc's eleven torch.empty buffers, three times)
    assert grown == [2048, 2049] and dirty.maxB == 2049
    state_same(dirty, clean, "ten steps")
    assert int(dirty.step_counter.item()) == len(batches)


def hold_first_step(c, batch):
    """a clean engine's first step (the sequence's own: 2049 rows) against float64 Adam: test_gpu_train_adam_f64's check"""
    import pcgnn_amd as P
    from pcgnn_amd.fused import FusedPCGNN
    from tests.test_gpu_train_adam_f64 import state
    m = build_model(P, c, c.rho, graph=P.DeviceGraph(c.X, c.csr, c.train_pos, dev()))
    fz = FusedPCGNN(m, c.lr, c.wd, betas=c.betas, max_batch=2049)
    ids, lab = batch
    B = ids.numel()
    before, _ = state(fz)
    sets = m.inter1.chosen_sets(ids, lab, True)
    fz.train_step(ids, lab, defer=True)
    fz.flush()
    after, _ = state(fz)
    masks = D.device_masks(fz.acts, c.f, c.emb, c.R, B)
    r64, r32, share, wrong = D.reference_pair(c, ids.cpu().numpy().astype(np.int64), lab.cpu().numpy().astype(np.int64), sets,
                                              params=before["theta"], dev_masks=masks)
    assert share <= D.AMBIGUOUS_CAP and wrong == 0, (share, wrong)
    fig = T.step_figures(c, 0, before, after, r64, r32, tag=f"clean first step B={B}")
    assert not T.misses([fig]), T.misses([fig])
    fz.check()


@pytest.mark.parametrize("ahead", [False, True], ids=["pipelined", "classifier-ahead"])
def test_pipelined_sequences_on_a_dirty_engine(ahead):
    """test_gpu_clf_ahead's workload (seven batches of 128, the last one 40 rows): two groups back to back through epoch_run,
    the engine built inside the block"""
    from tests import test_gpu_clf_ahead as CA
    w, ids = CA.workload()
    ids_d = torch.from_numpy(ids).to(dev())
    lab_d = torch.from_numpy(w.labels[ids].astype(np.int32)).to(dev())
    clean = CA._engine(w, ahead)
    with dirty_allocations(NAN, int_fill=WORD3) as log:
        dirty = CA._engine(w, ahead)
    logged(log, at_least=8)
    soil_engine(dirty)
    dirty.theta.copy_(clean.theta)
    dirty.params_changed()
    for fz in (clean, dirty):
        fz.begin_epoch(ids_d, lab_d, CA.B)
        steps = [(None, None, Bb, 0) for _, Bb in fz._ep_batches]
        assert fz._pipelines(fz._ep_batches) and fz._ahead(steps) == ahead, "the schedule this case is for"
        fz.epoch_run(flush=False)
        fz.epoch_run(n_steps=5, flush=False)
        fz.flush()
    CA._same(dirty, clean, "two groups")
    assert int(dirty.step_counter.item()) == 12


def test_whole_epoch_launch_on_a_dirty_engine():
    """run_epoch_one_graph, two epochs in one launch, a shorter last batch: the trainer built inside the block"""
    from pcgnn_amd import synth
    from pcgnn_amd.handler import PCGNNTrainer
    w = synth.make_workload("mini", 6000, 32, (4000, 30000, 90000), 0.12, seed=3)
    cfg = dict(engine="graph", batch_size=256, seed=5)
    clean = PCGNNTrainer(w, dict(cfg), dev())
    with dirty_allocations(NAN, int_fill=WORD3) as log:
        dirty = PCGNNTrainer(w, dict(cfg), dev())
    logged(log, at_least=8)
    soil_engine(dirty.fused)
    dirty.fused.theta.copy_(clean.fused.theta)
    dirty.fused.params_changed()
    for t in (clean, dirty):
        assert t.pick_size % 256 != 0
        assert t.run_epoch_one_graph(n_epochs=2) == 2 * t.pick_size
    state_same(dirty.fused, clean.fused, "two epochs in one launch")
    assert torch.equal(dirty.fused._ep_ids, clean.fused._ep_ids)
    assert int(dirty.fused.step_counter.item()) == 2 * -(-clean.pick_size // 256)


TWELVE = (64, 1000, 64, 257, 1000, 17, 257, 64, 1, 1000, 257, 64)


def step_lists(fz, B):
    """the selection lists of the last train_step of B rows, from that batch size's plan slot and the shared data part: per row
    the sorted chosen ids (``epoch.read_batch_lists``'s reading), every row's number of gather chunks, and the partial sums
    [chunks, F] of the rows of several chunks (the gather leaves those rows so; the dense launch adds them up in chunk order)"""
    g, lib = fz.g, fz.lib
    rows = g.R * B
    torch.cuda.synchronize()
    off = lambda which: int(lib.pcg_choose_workspace_offset(g.desc_ref(), B, fz.list_capacity, which))
    slot = fz._plans[B]
    begin = slot[off(0):off(0) + 8 * (rows + 1)].view(torch.int64).cpu().numpy()
    length = slot[off(1):off(1) + 4 * rows].view(torch.int32).cpu().numpy()
    d0 = off(2) - fz._plan_bytes(B)
    lst = fz.data[d0:d0 + 4 * max(int(begin[-1]), 1)].view(torch.int32).cpu().numpy()
    chunk_begin = slot[off(3):off(3) + 4 * (rows + 1)].view(torch.int32).cpu().numpy()
    out = []
    for r in range(rows):
        seg = lst[begin[r]:begin[r] + length[r]]
        out.append(np.sort(seg[seg >= 0]))
    nch = np.diff(chunk_begin)
    d6, stride, total = off(6) - fz._plan_bytes(B), g.X.stride(0), int(chunk_begin[-1])
    partial = fz.data[d6:d6 + 4 * max(total, 1) * stride].view(torch.float32).view(-1, stride)[:total, :g.feat_dim]
    several = torch.from_numpy(np.repeat(nch > 1, nch)).to(partial.device)
    return out, nch, partial[several].clone()


def test_zeroed_once_buffers_across_batch_sizes():
    """twelve steps over batch sizes 64, 1000, 64, 257, ... on ONE engine built dirty and never zeroed again; every step also
    runs on a FRESH engine (its buffers as fused._alloc makes them) given the state the one engine had before the step: the
    lists, counts and aggregates of the step - rows of one chunk in agg, longer rows as their partial sums - and the state after
    it.  (Each batch size has a plan slot of its own; the data part is shared by all of them.)"""
    c = D.GradCase.of((32, 64, 3))
    with dirty_allocations(NAN, int_fill=WORD3) as log:
        dirty = new_engine(c, 1000)
    logged(log, at_least=8)
    soil_engine(dirty)
    several = 0
    for k, B in enumerate(TWELVE):
        ids, lab = on_dev(*c.batch(B, salt=50 + k))
        fresh = new_engine(c, 1000)
        for name in ("theta", "m", "v", "step_counter"):
            getattr(fresh, name).copy_(getattr(dirty, name))
        fresh.params_changed()
        figs = []
        for fz in (fresh, dirty):
            fz.train_step(ids, lab)
            figs.append((step_lists(fz, B), fz.last_counts.clone(), fz._agg_of(B).clone()))
        ((l0, n0, p0), c0, a0), ((l1, n1, p1), c1, a1) = figs
        assert torch.equal(c0, c1), f"step {k} B={B}: counts"
        assert np.array_equal(n0, n1) and all(np.array_equal(x, y) for x, y in zip(l0, l1)), f"step {k} B={B}: lists"
        one = torch.from_numpy(n0 == 1).to(dev()).view(c.R, B)
        assert bool(one.any()) and torch.equal(bits(a0)[one], bits(a1)[one]), f"step {k} B={B}: aggregates of one-chunk rows"
        assert torch.equal(bits(p0), bits(p1)), f"step {k} B={B}: partial sums of the rows of several chunks"
        several += p0.shape[0]
        state_same(dirty, fresh, f"step {k} B={B}")
    assert several > 0, "no batch held a row of several chunks"
    assert sorted(dirty._plans) == sorted(set(TWELVE)) and int(dirty.step_counter.item()) == len(TWELVE)


CHOOSE_SIZES = (1000, 64, 257, 1000, 17)


@pytest.mark.parametrize("train", [True, False], ids=["train", "test"])
def test_choose_workspace_across_batch_sizes(train):
    """ops.choose_aggregate on ONE ChooseWorkspace (zeroed once, as the header asks; its data part - the selection list, the
    partial sums - dirtied: no initial contents required) while B changes between calls, against a fresh workspace per call; the
    clean aggregates against float64 means over the device's own lists"""
    import pcgnn_amd as P
    from pcgnn_amd import _lib, ops
    c = D.GradCase.of((32, 64, 3))
    m = build_model(P, c, c.rho, graph=P.DeviceGraph(c.X, c.csr, c.train_pos, dev()))
    inter = m.inter1
    g = inter.graph()
    lib = _lib.load()
    s0 = ops.score_table(g, inter.label_clf.weight, inter.label_clf.bias)
    keys = ops.pos_sort(g, s0) if train else None
    thr, rho = inter.thresholds, [a.rho for a in inter.intra_aggs]
    one = ops.ChooseWorkspace(g, max(CHOOSE_SIZES))
    assert not bool(one.buf.any())
    plan_bytes = int(lib.pcg_choose_plan_bytes(g.desc_ref(), max(CHOOSE_SIZES), one.list_capacity))
    dirty_(one.buf[plan_bytes:], WORD3)
    tally = Tally(f"choose_aggregate {'train' if train else 'test'} clean")
    for k, B in enumerate(CHOOSE_SIZES):
        ids, lab = on_dev(*c.batch(B, salt=70 + k))
        fresh = ops.ChooseWorkspace(g, B, list_capacity=one.list_capacity)
        want_agg, want_cnt = ops.choose_aggregate(g, ids, lab if train else None, s0, keys, thr, rho, train, ws=fresh)
        one.B = B                                                      # (the same bytes, carved for this call's B)
        with dirty_allocations(NAN, int_fill=INT_OUT) as log:
            agg, cnt = ops.choose_aggregate(g, ids, lab if train else None, s0, keys, thr, rho, train, ws=one)
        logged(log, at_least=2)
        assert torch.equal(cnt, want_cnt), f"call {k} B={B}: counts"
        assert torch.equal(bits(agg), bits(want_agg)), f"call {k} B={B}: aggregates"
        one.check()
        fresh.check()
        if k == 0:
            sets = inter.chosen_sets(ids, lab if train else None, train)
            X = c.X
            ref = {dt: np.stack([np.stack([X[sorted(sets[r][i])].astype(dt).mean(0) for i in range(B)]) for r in range(c.R)])
                   for dt in (np.float64, np.float32)}
            tally.check(f"B={B} aggregates", want_agg, torch.from_numpy(ref[np.float64]), torch.from_numpy(ref[np.float32]))
            assert np.array_equal(want_cnt.cpu().numpy(), np.array([[len(sets[r][i]) for i in range(B)] for r in range(c.R)]))
    tally.done()


# =====================================================================================================================================
# d. outputs: a - c once more with every torch.empty output starting as NaN (floats) or -7 (integers)
# =====================================================================================================================================
@pytest.mark.parametrize("shape,name", A_CASES, ids=A_IDS)
def test_whole_set_outputs_start_dirty(shape, name):
    """every element of every output is documented as written - rows of count 0 and the holes of a chosen list included"""
    hold_to_references(shape)
    s = setup_of(shape)
    fz = s.engine["dirty"]
    want = clean_of(shape, name)
    CALLS[name][1](s, "dirty", "main", None)                           # (the workspaces exist: the block fills the outputs alone)
    with dirty_allocations(NAN, int_fill=INT_OUT) as log:
        got = CALLS[name][1](s, "dirty", "main", None)
    logged(log, at_least=2)
    same(got, want, f"{name} into outputs of NaN / -7")
    settled(fz)


@pytest.mark.parametrize("case", B_CASES, ids=IDS)
def test_baseline_outputs_start_dirty(case):
    with dirty_allocations(NAN, int_fill=INT_OUT) as log:
        got = baseline_run(*case, A5)
    logged(log, at_least=10)
    same(got, baseline_clean(case), f"baseline {case} into outputs of NaN")


@pytest.mark.parametrize("name", list(C_CASES))
def test_metric_outputs_start_dirty(name):
    """what the header documents as written equals clean; pcg_pr_counts past G keeps the fill"""
    case = metric_case(name)
    case["run"]()
    with dirty_allocations(NAN, int_fill=INT_OUT) as log:
        got = case["run"]()
    logged(log, at_least=1)
    same(got, case["clean"], f"{name} into outputs of NaN / -7")
    if "_tail" in got:
        for t in got["_tail"]:
            assert t.numel() > 0 and bool((t == INT_OUT).all()), f"{name}: an entry past G was written"
