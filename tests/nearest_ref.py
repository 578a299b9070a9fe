"""A plain numpy float64 reference of pcg_topk_similar (ops.topk_similar, FusedPCGNN.nearest): scores of every (query, bank) pair,
then per query row the k best by (score descending, bank position ascending), with the id exclusion and the padding.

metric - always maximised: "dot" q.c | "cosine" q.c / (|q| |c|), 0 when either norm is 0 | "l2" min(0, 2 q.c - |q|^2 - |c|^2).
Reads nothing but its arguments."""
import numpy as np

METRICS = ("dot", "cosine", "l2")


def scores(Q, bank, metric):
    """[n, M] float64"""
    Q, bank = np.asarray(Q, dtype=np.float64), np.asarray(bank, dtype=np.float64)
    if metric not in METRICS:
        raise ValueError(metric)
    dot = Q @ bank.T
    if metric == "dot":
        return dot
    qn2, cn2 = (Q * Q).sum(1), (bank * bank).sum(1)
    if metric == "l2":
        return np.minimum(0.0, 2.0 * dot - qn2[:, None] - cn2[None, :])
    den = np.sqrt(qn2)[:, None] * np.sqrt(cn2)[None, :]
    ok = (qn2[:, None] > 0) & (cn2[None, :] > 0)
    return np.where(ok, dot / np.where(ok, den, 1.0), 0.0)


def eligible(n, M, q_ids=None, bank_ids=None):
    """[n, M] bool: bank row c may be returned for query row i (exclude_self: bank_ids[c] != q_ids[i])"""
    if (q_ids is None) != (bank_ids is None):
        raise ValueError("q_ids and bank_ids go together")
    if q_ids is None:
        return np.ones((n, M), dtype=bool)
    return np.asarray(q_ids).reshape(-1, 1) != np.asarray(bank_ids).reshape(1, -1)


def topk_of_scores(s, k, ok=None):
    """s [n, M] -> (pos [n, k] int32, score [n, k] float64): per row the k eligible columns with the highest score, ties by the
    lower column; slots beyond the number of eligible columns hold -1 / -inf"""
    s = np.asarray(s, dtype=np.float64)
    n, M = s.shape
    pos = np.full((n, k), -1, dtype=np.int32)
    out = np.full((n, k), -np.inf, dtype=np.float64)
    for i in range(n):
        cols = np.arange(M) if ok is None else np.nonzero(ok[i])[0]
        order = cols[np.argsort(-s[i, cols], kind="stable")][:k]          # (stable: equal scores keep ascending position)
        pos[i, :len(order)] = order
        out[i, :len(order)] = s[i, order]
    return pos, out


def topk_similar_ref(Q, bank, k, metric="cosine", q_ids=None, bank_ids=None):
    Q, bank = np.asarray(Q), np.asarray(bank)
    return topk_of_scores(scores(Q, bank, metric), k, eligible(Q.shape[0], bank.shape[0], q_ids, bank_ids))
