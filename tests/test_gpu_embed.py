"""Node embeddings from the whole-set pass (FusedPCGNN.embed / embed_new; pcg_embed_set / pcg_embed_new) on the GPU.

Identities, not tolerances: ``embed`` against the ``predict(..., want_combined=True)`` loop, its logits against ``infer``,
``embed_new`` against ``embed`` of N + j on the graph rebuilt with the query rows appended - all ``torch.equal``.
One tolerance: h and emb against tests/dense_ref.py in float64, fed the device's own chosen lists; the bound is
``dense_ref.tolerance`` of the same reference in float32 (8 * e_f32 + 2^-20, relative to the tensor's largest element).  An
element whose float64 pre-activation lies within that bound of zero may sit on either side of the ReLU: for those the
magnitude is compared (|got| <= |pre| + bound), and at most 1 % of a tensor's elements may be of that kind - which
``test_f32_reference_ambiguous_share`` checks on the CPU, with the fixtures' own test-mode sets.

Shapes: yelp_small (R 3, the fixed WLDS kernel), yelp_emb128 (streamed weights), five_rel and feat100 (the run-time,
non-persistent kernels), amazon_small (the fixed F = 25 kernel)."""
import numpy as np
import pytest
import torch

from tests import dense_ref as D
from tests.util import GoldenCase

gpu = pytest.mark.gpu
CASES = ["yelp_small", "yelp_emb128", "five_rel", "feat100", "amazon_small"]
AMBIGUOUS_SHARE = 0.01
_ENGINES = {}


def dev():
    return torch.device("cuda", 0)


def engine_of(name):
    from tests.test_gpu_infer_new import engine
    if name not in _ENGINES:
        c = GoldenCase(name)
        _ENGINES[name] = (c, engine(c.X, c.csr, c.train_pos, c.emb, [0.5] * c.R, c.params(), c.alpha))
    return _ENGINES[name]


def as_dev(ids):
    return torch.as_tensor(np.asarray(ids), dtype=torch.int32, device=dev())


def predict_loop(fz, ids, B):
    """(combined, logits) of the per-batch path, B rows at a time"""
    ids = as_dev(ids)
    comb, logits = [], []
    for b in range(0, ids.numel(), B):
        lg, _, cb = fz.predict(ids[b:b + B], want_combined=True)
        comb.append(cb.clone())
        logits.append(lg)
    return torch.cat(comb), torch.cat(logits)


def id_sets(c):
    """n = 1, 15, 16, 17 (shuffled, with duplicates) and 16 * CUs + 17 (ids repeat: a persistent workgroup runs a second tile)"""
    rs = np.random.RandomState(7)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = {}
    for n in (1, 15, 16, 17):
        ids = rs.choice(c.n, size=n, replace=False)
        if n >= 15:
            ids[3], ids[n - 1] = ids[0], ids[0]                       # duplicates, one of them the last row
        out[n] = ids
    out[16 * cus + 17] = rs.randint(0, c.n, size=16 * cus + 17)
    return out


@gpu
@pytest.mark.parametrize("name", CASES)
def test_embed_is_the_predict_loop(name):
    c, fz = engine_of(name)
    for n, ids in id_sets(c).items():
        want, want_logits = predict_loop(fz, ids, 256 if n > 17 else (7 if n == 17 else n))
        one = fz.embed(ids)
        assert one.shape == (n, c.emb) and one.dtype == torch.float32
        assert torch.equal(one, want), f"n {n}: one chunk"
        if n > 1:
            assert torch.equal(fz.embed(ids, chunk=n - 1), want), f"n {n}: a last chunk of one row"
        emb, h, lg = fz.embed(as_dev(ids), chunk=max(n // 3, 1), relations=True, want_logits=True)
        assert torch.equal(emb, want) and torch.equal(lg, want_logits), f"n {n}: three chunks, all outputs"
        assert h.shape == (n, c.R, c.emb)
        # a row's values depend on the row alone: a permuted list gives the same bits per node
        perm = np.random.RandomState(n).permutation(n)
        assert torch.equal(fz.embed(ids[perm]), want[torch.as_tensor(perm, device=dev())])
    assert fz.embed([]).shape == (0, c.emb)
    e0, h0, l0 = fz.embed(np.zeros(0, np.int64), relations=True, want_logits=True)
    assert e0.shape == (0, c.emb) and h0.shape == (0, c.R, c.emb) and l0.shape == (0, 2)
    fz.check()


@gpu
@pytest.mark.parametrize("name", CASES)
def test_logits_are_infers_and_state_is_untouched(name):
    c, fz = engine_of(name)
    ids = id_sets(c)[17]
    before = fz.infer(ids, want_center=True)
    p_before = fz.predict(as_dev(ids))
    theta, s0 = fz.theta.clone(), fz.s0.clone()
    emb, lg = fz.embed(ids, want_logits=True)
    emb2, h = fz.embed(ids, relations=True)
    assert torch.equal(lg, before[0]) and torch.equal(emb, emb2)
    whole_e, whole_l = fz.embed(None, want_logits=True)
    assert whole_e.shape == (c.n, c.emb) and torch.equal(whole_l, fz.infer(None))
    assert torch.equal(whole_e[torch.as_tensor(ids, device=dev())], emb)
    after = fz.infer(ids, want_center=True)
    p_after = fz.predict(as_dev(ids))
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert torch.equal(p_before[0], p_after[0]) and torch.equal(p_before[1], p_after[1])
    assert torch.equal(fz.theta, theta) and torch.equal(fz.s0, s0)
    fz.check()


# ---- float64 ------------------------------------------------------------------------------------------------------------
def index_of(ch):
    """a ChosenLists -> per relation (rows, cols, counts), entries in the device's order"""
    h = torch.from_numpy(np.asarray(ch.host_offsets()))
    ids = ch.ids.cpu().long()
    out = []
    for r in range(ch.R):
        off = h[r * ch.n:(r + 1) * ch.n + 1]
        cnt = off[1:] - off[:-1]
        out.append((torch.repeat_interleave(torch.arange(ch.n), cnt), ids[int(off[0]):int(off[-1])], cnt.double()))
    return out


def forward_refs(c, ids, index):
    """(float64, float32) runs of the reference forward on the given selection"""
    y = np.zeros(len(ids), np.int64)
    return tuple(D.dense_ref(c.X, ids, y, index, c.params(), 1.0, dt) for dt in (torch.float64, torch.float32))


def bounds(r64, r32):
    """per activation tensor (h_1 .. h_R, combined): (float64 values, float64 pre-activations, absolute bound, ambiguous mask)"""
    out = []
    for p64, p32 in zip(r64["pre"], r32["pre"]):
        v64, v32 = torch.relu(p64), torch.relu(p32)
        tol = D.tolerance(D.rel_err(v32, v64)) * float(v64.abs().max())
        out.append((v64, p64, tol, p64.abs() < tol))
    return out


def check_activation(what, got, v64, p64, tol, amb):
    got = got.detach().cpu().double()
    share = float(amb.double().mean())
    err = float((got - v64)[~amb].abs().max())
    print(f"{what}: max error {err:.3e}  bound {tol:.3e}  ambiguous {share:.3%}")
    assert share <= AMBIGUOUS_SHARE, f"{what}: {share:.2%} of the elements lie within the bound of the ReLU's kink"
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"
    assert bool((got[amb].abs() <= p64[amb].abs() + tol).all()), f"{what}: an element at the kink is not small"


@pytest.mark.parametrize("name", CASES)
def test_f32_reference_ambiguous_share(name):
    """CPU: with the fixtures' own test-mode sets, the elements treated as 'at the kink' stay under 1 % of every tensor"""
    c = GoldenCase(name)
    r64, r32 = forward_refs(c, c.nodes, [c.sel("test", r) for r in range(c.R)])
    for t, (v64, p64, tol, amb) in enumerate(bounds(r64, r32)):
        assert float(amb.double().mean()) <= AMBIGUOUS_SHARE, (name, t)
        assert float((torch.relu(r32["pre"][t]).double() - v64).abs().max()) <= tol


@gpu
@pytest.mark.parametrize("name", CASES)
def test_against_float64(name):
    c, fz = engine_of(name)
    ids = np.asarray(c.nodes, dtype=np.int64)
    emb, h, lg = fz.embed(ids, relations=True, want_logits=True)
    r64, r32 = forward_refs(c, ids, index_of(fz.chosen(ids)))
    b = bounds(r64, r32)
    for r in range(c.R):
        check_activation(f"{name} h_{r + 1}", h[:, r, :], *b[r])
    check_activation(f"{name} emb", emb, *b[c.R])
    # emb @ W_cls^T is the logits
    e32 = D.rel_err(r32["logits"], r64["logits"])
    tol = D.tolerance(e32) * float(r64["logits"].abs().max())
    mine = emb.cpu().double() @ c.params()["weight"].double().t()
    err = float((mine - lg.cpu().double()).abs().max())
    err64 = float((lg.cpu().double() - r64["logits"]).abs().max())
    print(f"{name} logits: |emb W_cls^T - logits| {err:.3e}  |logits - float64| {err64:.3e}  bound {tol:.3e}")
    assert err <= tol and err64 <= tol


# ---- unseen nodes ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", CASES)
def test_embed_new_is_embed_on_the_rebuilt_graph(name):
    from pcgnn_amd.graph import QueryBatch
    from tests.test_gpu_infer_new import engine, grow, split
    c = GoldenCase(name)
    nq = 40
    Xf, full_csr = grow(c.X, c.csr, nq, seed=21)
    Xb, base_csr, Xq, q_pairs = split(Xf, full_csr, c.n)
    # query rows point at base nodes, at each other and at themselves
    ip, ix = q_pairs[0]
    rows = np.repeat(np.arange(nq), np.diff(ip))
    assert (ix < c.n).any() and ((ix >= c.n) & (ix != c.n + rows)).any() and (ix == c.n + rows).sum() == nq
    thr = [0.5] * c.R
    full = engine(Xf, full_csr, c.train_pos, c.emb, thr, c.params(), c.alpha)
    base = engine(Xb, base_csr, c.train_pos, c.emb, thr, c.params(), c.alpha)
    query = QueryBatch(Xq, q_pairs, base.g)
    want = full.embed(as_dev(c.n + np.arange(nq)), relations=True, want_logits=True)
    cold = base.embed_new(query, relations=True, want_logits=True)
    assert base._new_scored_base
    warm = base.embed_new(query, relations=True, want_logits=True, chunk=nq - 1)
    assert not base._new_scored_base
    for a, b, w in zip(cold, warm, want):
        assert a.shape == w.shape and torch.equal(a, w) and torch.equal(b, w)
    assert torch.equal(cold[2], base.infer_new(query))
    ids = np.array([5, 5, 39, 0, 17])
    assert torch.equal(base.embed_new(query, ids=ids), want[0][torch.as_tensor(ids, device=dev())])
    assert base.embed_new(query, ids=[]).shape == (0, c.emb)
    base.check()


# ---- extents ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", CASES)
def test_nothing_is_written_outside_the_outputs(name):
    """n = 17: a second tile with one row; out_emb is [17][E] and out_rel [17][R * E] to the byte"""
    from tests.guarded import GuardedArena, guarded_allocations
    c, fz = engine_of(name)
    ids = id_sets(c)[17]
    want = fz.embed(ids, relations=True, want_logits=True)           # (the call's workspace exists from here on)
    arena = GuardedArena(32 << 20, dev())
    with guarded_allocations(arena) as log:
        got = fz.embed(ids, relations=True, want_logits=True)
        torch.cuda.synchronize()
    arena.check("embed")
    sizes = sorted(nbytes for _, _, _, nbytes in log)
    assert 17 * c.emb * 4 in sizes and 17 * c.R * c.emb * 4 in sizes and 17 * 2 * 4 in sizes
    for a, b in zip(got, want):
        assert torch.equal(a, b)
