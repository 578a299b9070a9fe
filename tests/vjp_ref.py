"""The CPU reference of the custom-loss path (FusedPCGNN.forward / vjp / train_step_custom): ``dense_ref``'s forward
(tests/dense_ref.py - the selection an input, the same masked-ReLU option) with the LOSS a parameter,
``loss_fn(gnn_logits, center_logits, labels) -> scalar``, autograd for every parameter; float64 is the reference, float32 - the
same code - the yardstick.  A parameter the loss does not reach gets a zero gradient.  With ``builtin_loss`` the gradients are
``dense_ref``'s, exactly (tests/test_vjp_host.py).

The three losses of tests/test_gpu_custom_loss.py are here too, written for any dtype and device; ``labels`` may be the int32
tensor the engine hands on.  The cases are dense_ref's: ``GradCase.batch(B)`` with salt 0, for the shapes and batch sizes below.
"""
import numpy as np
import torch
import torch.nn.functional as Fn

from tests import dense_ref as D

# dense_ref.SHAPES' two fixed-shape kernels (with / without the weights' LDS copy) and the two run-time-shape ones (without / with)
SHAPES = [(32, 64, 3), (32, 128, 3), (10, 16, 1), (24, 16, 5)]
# the other two fixed-shape kernels (F = 25), a wide row (the F > 64 staging loops), and dense_ref.EDGE_SHAPES' run-time-shape
# kernels with the weights' LDS copy at E = 64 (R = 4) and E = 128, and without it at E = 272 (17 column tiles for 16 waves)
SHAPES += [(25, 64, 3), (25, 128, 3), (100, 64, 3), (16, 64, 4), (20, 128, 1), (16, 272, 1)]
# a lone row, a full tile, a ragged tile, the first size at which pcg_wgrad shares a weight tile between workgroups
BATCHES = [1, 16, 17, 1025]
FOCAL_GAMMA, FOCAL_WEIGHT = 2.0, (0.25, 0.75)
SMOOTHING = 0.1


def builtin_loss(lambda_1):
    """CE(gnn) + lambda_1 * CE(label), mean reduction - operation by operation what dense_ref forms"""
    def loss(gnn, center, labels):
        y = labels.long()
        rows = Fn.cross_entropy(gnn, y, reduction="none") + lambda_1 * Fn.cross_entropy(center, y, reduction="none")
        return rows.sum() / y.numel()
    return loss


def focal_loss(lambda_1, gamma=FOCAL_GAMMA, weight=FOCAL_WEIGHT):
    """class-weighted focal loss on the gnn logits + lambda_1 * CE on the label-aware logits, SUM reduction"""
    def loss(gnn, center, labels):
        y = labels.long()
        logp = Fn.log_softmax(gnn, dim=1).gather(1, y[:, None])[:, 0]
        w = torch.tensor(weight, dtype=gnn.dtype, device=gnn.device)[y]
        return -(w * (1.0 - logp.exp()) ** gamma * logp).sum() + lambda_1 * Fn.cross_entropy(center, y, reduction="sum")
    return loss


def gnn_only_loss():
    """label-smoothed CE of the gnn logits alone: the label classifier gets no gradient"""
    def loss(gnn, center, labels):
        return Fn.cross_entropy(gnn, labels.long(), label_smoothing=SMOOTHING)
    return loss


LOSSES = {"builtin": builtin_loss, "focal": focal_loss, "gnn_only": lambda lambda_1: gnn_only_loss()}


def vjp_ref(X, ids, labels, sets, params, loss_fn, dtype=torch.float64, masks=None):
    """dense_ref with ``loss_fn`` in place of the built-in loss (no row weights).  Returns dict(loss, logits, center, pre,
    grads), everything in ``dtype``, detached."""
    X = torch.as_tensor(X).to(dtype)
    ids = torch.as_tensor(np.asarray(ids)).long()
    y = torch.as_tensor(np.asarray(labels)).long()
    B, R = ids.numel(), len(sets)
    index = D.sets_to_index(sets)
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    self_feats = X[ids]
    act = (lambda r, pre: Fn.relu(pre)) if masks is None else (lambda r, pre: pre * masks[r].to(dtype))
    feats, pre = [self_feats], []
    for r, (rows, cols, cnt) in enumerate(index):
        agg = torch.zeros(B, X.shape[1], dtype=dtype).index_add_(0, rows, X[cols]) / cnt.to(dtype)[:, None]
        pre.append(torch.cat((self_feats, agg), dim=1).mm(p[f"inter1.intra_agg{r + 1}.weight"]))
        feats.append(act(r, pre[-1]))
    pre.append(torch.cat(feats, dim=1).mm(p["inter1.weight"]))
    comb = act(R, pre[-1])
    logits = comb.mm(p["weight"].t())
    center = Fn.linear(self_feats, p["inter1.label_clf.weight"], p["inter1.label_clf.bias"])
    loss = loss_fn(logits, center, y)
    names = list(p)
    grads = torch.autograd.grad(loss, [p[k] for k in names], allow_unused=True)
    return dict(loss=loss.detach(), logits=logits.detach(), center=center.detach(), pre=[t.detach() for t in pre],
                grads={k: (torch.zeros_like(p[k]) if g is None else g).detach() for k, g in zip(names, grads)})


def reference_pair(case, ids, labels, sets, loss_fn, params=None, dev_masks=None):
    """dense_ref.reference_pair for a custom loss: (ref64, ref32, share of ambiguous activations, non-ambiguous entries where
    the device's mask is not the float64 sign).  The pre-activations - and so the ReLU-kink rule - do not depend on the loss."""
    params = case.params() if params is None else params
    index = D.sets_to_index(sets)
    args = (case.X, ids, labels, index, params, loss_fn)
    plain64, plain32 = vjp_ref(*args, dtype=torch.float64), vjp_ref(*args, dtype=torch.float32)
    _, amb, share = D.ambiguous(plain64["pre"], plain32["pre"])
    masks, wrong = D.resolve_masks(plain64["pre"], amb, dev_masks)
    return vjp_ref(*args, dtype=torch.float64, masks=masks), vjp_ref(*args, dtype=torch.float32, masks=masks), share, wrong
