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


def test_wlds_rule_of_the_shapes():
    """which dense kernel each shape runs (the templated ones by their exact shape, the others by the shared-memory rule)"""
    for (F, E, R), (kernel, _, _) in D.SHAPES.items():
        assert D.dense_wlds(F, E, R) == kernel.startswith("dense_step_kernel<true"), (F, E, R)


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


def test_every_case_keeps_the_ambiguous_cap(host_refs):
    over = {k: v[2] for k, v in host_refs.items() if v[2] > D.AMBIGUOUS_CAP}
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
