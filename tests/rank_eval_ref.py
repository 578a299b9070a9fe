"""numpy restatement of what pcg_pr_counts and pcg_topk_alerts form (include/pcgnn.h):
hdr = tp, fp, fn, tn, n1, n0, G, 0 with tp_g / npred_g [G] from (prob [n, 2] float32, labels [n]), and the first k positions /
scores of the alert order (the stable descending sort by p1 + 0.0f) from a score vector."""
import numpy as np

from tests.eval_ref import scores  # noqa: F401  (the tests' inputs: re-exported)


def pr_counts_numpy(prob, labels):
    """-> (hdr uint64 [8], tp_g uint32 [G], npred_g uint32 [G])"""
    prob = np.asarray(prob, dtype=np.float32).reshape(-1, 2)
    y = np.asarray(labels).astype(np.int64).reshape(-1)
    hdr = np.zeros(8, dtype=np.uint64)
    if len(y) == 0:
        return hdr, np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    pred = prob.argmax(axis=1)
    p = prob[:, 1] + np.float32(0.0)
    pos = p[y == 1]
    hdr[:6] = [np.sum((pred == 1) & (y == 1)), np.sum((pred == 1) & (y == 0)), np.sum((pred == 0) & (y == 1)),
               np.sum((pred == 0) & (y == 0)), len(pos), len(p) - len(pos)]
    u = np.unique(pos)[::-1]                                          # u_1 > u_2 > ... > u_G
    hdr[6] = len(u)
    ps, al = np.sort(pos), np.sort(p)
    tp_g = len(ps) - np.searchsorted(ps, u, side="left")              # #{y = 1, p1 >= u_g}
    npred_g = len(al) - np.searchsorted(al, u, side="left")           # #{p1 >= u_g}
    return hdr, tp_g.astype(np.uint32), npred_g.astype(np.uint32)


def average_precision_numpy(prob, labels) -> float:
    """the specification's float64 statement on the integers above"""
    import math
    hdr, tp, npred = pr_counts_numpy(prob, labels)
    n1 = int(hdr[4])
    d = np.diff(np.concatenate([[0], tp.astype(np.int64)]))
    terms = (d.astype(np.float64) / np.float64(n1)) * (tp.astype(np.float64) / npred.astype(np.float64))
    return math.fsum(terms)


def alerts_numpy(p1, k):
    """-> (pos int32 [k], score float32 [k]): the first min(k, n) positions of the stable descending sort, then -1 / -inf"""
    p1 = np.asarray(p1, dtype=np.float32).reshape(-1)
    order = np.argsort(-(p1 + np.float32(0.0)), kind="stable")[:k]
    pos = np.full(k, -1, dtype=np.int32)
    score = np.full(k, -np.inf, dtype=np.float32)
    pos[:len(order)] = order
    score[:len(order)] = p1[order]
    return pos, score
