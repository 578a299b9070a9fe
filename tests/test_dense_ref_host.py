"""CPU-only tests of the float64 reference the GPU gradient tests compare the kernels with (tests/dense_ref.py): it is the
model's plain autograd, its cases keep the ReLU-kink cap, and the tolerance it yields is far below what one batch row dropped
or counted twice does to every parameter's gradient."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from tests import dense_ref as D
from tests.util import PARAM_KEYS


@pytest.fixture(scope="module")
def cases():
    return {shape: D.GradCase.of(shape) for shape in D.SHAPES}


@pytest.fixture(scope="module")
def host_refs(cases):
    """(shape, B) -> (ref64, ref32, share of ambiguous activations, index of the sets), computed once, with the oracle's sets"""
    out = {}
    for shape, (_, batches, _) in D.SHAPES.items():
        c = cases[shape]
        for B in sorted(set(batches)):
            ids, lab = c.batch(B)
            index = D.sets_to_index(c.host_sets(ids, lab))
            r64, r32, share, _ = D.reference_pair(c, ids, lab, index)
            out[shape, B] = (r64, r32, share, index)
    return out


@pytest.fixture(scope="module")
def wide_refs():
    """host_refs for the wide shapes, whose batches have the hub rows pinned into them: (shape, B, salt) -> (share of ambiguous
    activations, the oracle's sets); salt 1: the second batch of the deferred-update test"""
    out = {}
    for shape, (_, batches, _) in D.WIDE_SHAPES.items():
        c = D.GradCase.of(shape)
        for B, salt in [(B, 0) for B in sorted(set(batches))] + [(1025, 1)]:
            ids, lab = c.wide_batch(B, salt)
            sets = c.host_sets(ids, lab)
            out[shape, B, salt] = (D.reference_pair(c, ids, lab, D.sets_to_index(sets))[2], sets)
    return out


def test_wlds_rule_of_the_shapes():
    """which dense kernel each shape runs (the templated ones by their exact shape, the others by the shared-memory rule)"""
    for (F, E, R), (kernel, _, _) in list(D.SHAPES.items()) + list(D.WIDE_SHAPES.items()):
        assert D.dense_wlds(F, E, R) == kernel.startswith("dense_step_kernel<true"), (F, E, R)
    for (F, E, R), (kernel, _, _) in D.WIDE_SHAPES.items():
        assert kernel.endswith("<true, 0, 0, 0>") or kernel.endswith("<false, 0, 0, 0>")     # no templated instantiation
        assert D.dense_smem_bytes(F, E, R, D.dense_wlds(F, E, R)) == D.WIDE_LDS_BYTES[F, E, R] <= 160 * 1024
        assert F > 64 and (F + 3) // 4 * 4 <= 512
    assert not set(D.SHAPES) & set(D.WIDE_SHAPES)


def test_pins_change_their_positions_only():
    c = D.GradCase.of((260, 16, 1))
    for B in (1, 17, 1025, 2049):
        pins = c.wide_pins(B)
        (plain, _), (ids, lab) = c.batch(B), c.wide_batch(B)
        other = np.array([b not in pins for b in range(B)])
        assert np.array_equal(ids[other], plain[other]) and all(ids[b] == v for b, v in pins.items())
        assert np.array_equal(lab, c.labels[ids])
        assert 0 in pins and (B < 16 or 15 in pins) and (B % 16 == 0 or B < 16 or B // 16 * 16 in pins)
    assert c.hubs(1) == [7]                                     # synth_graph's hub


def test_wide_batches_stage_rows_of_several_chunks_in_both_loops(wide_refs):
    """with the oracle's sets (the device's are asserted again on the GPU): every wide batch of a whole tile has a pinned set of
    more than 128 entries among the first 2048 staged aggregate elements and one in the loop beyond"""
    cases = {shape: D.GradCase.of(shape) for shape in D.WIDE_SHAPES}
    for (shape, B, salt), (_, sets) in wide_refs.items():
        pins = cases[shape].wide_pins(B)
        direct, beyond = D.staged_multi_chunk_rows(sets, shape[0], B)
        assert [x for x in direct if x[1] in pins], (shape, B, salt)
        assert B < D.TILE_ROWS or [x for x in beyond if x[1] in pins], (shape, B, salt)


@pytest.mark.parametrize("shape,B", [((25, 64, 3), 65), ((16, 48, 5), 17), ((32, 128, 3), 1)])
def test_masked_reference_is_plain_autograd(cases, shape, B):
    """(a) no ambiguous entry forced: the masked float64 reference == straightforward float64 autograd with F.relu, written
    out independently here (per-row means, nn-style layers, the mean-reduction loss)"""
    c = cases[shape]
    ids, lab = c.batch(B)
    sets = c.host_sets(ids, lab)
    X = torch.from_numpy(c.X).double()
    p = {k: v.double().requires_grad_(True) for k, v in c.params().items()}
    self_feats = X[torch.as_tensor(ids)]
    feats = [self_feats]
    for r in range(c.R):
        agg = torch.stack([X[sorted(s)].mean(0) for s in sets[r]])
        feats.append(Fn.relu(torch.cat((self_feats, agg), 1) @ p[f"inter1.intra_agg{r + 1}.weight"]))
    comb = Fn.relu(torch.cat(feats, 1) @ p["inter1.weight"])
    y = torch.as_tensor(lab)
    logits = comb @ p["weight"].t()
    center = self_feats @ p["inter1.label_clf.weight"].t() + p["inter1.label_clf.bias"]
    loss = Fn.cross_entropy(logits, y) + c.alpha * Fn.cross_entropy(center, y)
    loss.backward()
    r64, _, share, wrong = D.reference_pair(c, ids, lab, sets)
    assert wrong == 0
    assert abs(float(r64["loss"]) - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    assert D.rel_err(r64["logits"], logits.detach()) <= 1e-12
    for k in PARAM_KEYS(c.R):
        assert D.rel_err(r64["grads"][k], p[k].grad) <= 1e-12, k


def test_every_case_keeps_the_ambiguous_cap(host_refs, wide_refs):
    over = {k: v[2] for k, v in host_refs.items() if v[2] > D.AMBIGUOUS_CAP}
    over.update({k: v[0] for k, v in wide_refs.items() if v[0] > D.AMBIGUOUS_CAP})
    assert not over, f"ambiguous ReLU pre-activations above {D.AMBIGUOUS_CAP}: {over} - change the seed or the weight scale"


@pytest.mark.parametrize("B", [17, 1025, 2049])
def test_one_row_wrong_is_ten_tolerances_away(cases, host_refs, B):
    """(b) the last batch row dropped, and row 1024 counted twice where it exists: every parameter's float64 gradient moves by
    at least 10 x the tolerance the GPU test allows for that case (8 * e_f32 + 2^-20, relative to the largest element)"""
    short = []
    for shape in D.SHAPES:
        c = cases[shape]
        ids, lab = c.batch(B)
        r64, r32, _, index = host_refs[shape, B]
        masks = [(t > 0).double() for t in r64["pre"]]
        variants = {"last row dropped": np.r_[np.ones(B - 1), 0.0]}
        if B > 1024:
            variants["row 1024 twice"] = np.r_[np.ones(1024), 2.0, np.ones(B - 1025)]
        for what, w in variants.items():
            bad = D.dense_ref(c.X, ids, lab, index, c.params(), c.alpha, masks=masks, row_weight=w)
            for k in PARAM_KEYS(c.R):
                tol = D.tolerance(D.rel_err(r32["grads"][k], r64["grads"][k]))
                moved = D.rel_err(bad["grads"][k], r64["grads"][k])
                print(f"{shape} B={B} {what:16s} {k:28s} moved {moved:.3e}  tolerance {tol:.3e}  x{moved / tol:.1f}")
                if moved < 10 * tol:
                    short.append((shape, B, what, k, moved, tol))
    assert not short, short
