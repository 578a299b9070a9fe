"""numpy restatement of what pcg_eval_counts forms (include/pcgnn.h): the integer vector
tp, fp, fn, tn, n1, n0, 2U, 0, tp_t[T], npred_t[T] from (prob [n, 2] float32, labels [n], thresholds [T])."""
import numpy as np


def default_thresholds():
    return np.linspace(0.01, 0.99, 100)


def counts_numpy(prob, labels, thresholds=None) -> np.ndarray:
    prob = np.asarray(prob, dtype=np.float32).reshape(-1, 2)
    y = np.asarray(labels).astype(np.int64).reshape(-1)
    th = default_thresholds() if thresholds is None else np.asarray(thresholds, dtype=np.float64)
    T = len(th)
    out = np.zeros(8 + 2 * T, dtype=np.uint64)
    if len(y) == 0:
        return out
    pred = prob.argmax(axis=1)
    p = prob[:, 1]
    pos, neg = p[y == 1], p[y == 0]
    n1, n0 = len(pos), len(neg)
    out[:6] = [np.sum((pred == 1) & (y == 1)), np.sum((pred == 1) & (y == 0)), np.sum((pred == 0) & (y == 1)),
               np.sum((pred == 0) & (y == 0)), n1, n0]
    ps = np.sort(pos)
    lb = np.searchsorted(ps, neg, side="left").astype(np.int64)      # positives below a negative
    ub = np.searchsorted(ps, neg, side="right").astype(np.int64)     # positives below or equal
    out[6] = int(np.sum(n1 - lb) + np.sum(n1 - ub))                  # 2 #{pos > neg} + #{pos == neg}, over all pairs
    all_sorted = np.sort(p.astype(np.float64))
    pos_sorted = ps.astype(np.float64)
    out[8:8 + T] = n1 - np.searchsorted(pos_sorted, th, side="right")
    out[8 + T:] = len(p) - np.searchsorted(all_sorted, th, side="right")
    return out


def scores(n, pos_share, seed, kind="continuous"):
    """seeded (prob [n, 2] float32, labels [n] int32): sigmoid of logits that carry some signal.
    kind: continuous | tied (logits rounded to quarters, 50 saturated rows) | edges (exact 0.0 and 1.0 rows, +-0.0) | equal"""
    rs = np.random.RandomState(seed)
    y = (rs.rand(n) < pos_share).astype(np.int32)
    if n >= 2:
        y[0], y[1] = 1, 0                                            # both classes present
    z = rs.randn(n, 2).astype(np.float32)
    z[:, 1] += 1.5 * y - 0.5
    if kind == "tied":
        z = np.round(z * 4) / 4
        sat = rs.choice(n, size=min(50, n), replace=False)
        z[sat[::2], 1], z[sat[1::2], 1] = 40.0, -120.0
    if kind == "equal":
        z[:] = 0.25
    with np.errstate(over="ignore"):
        prob = (1.0 / (1.0 + np.exp(-z.astype(np.float64)))).astype(np.float32)
    if kind == "edges":
        k = max(1, n // 20)
        idx = rs.choice(n, size=min(4 * k, n), replace=False)
        prob[idx[0::4], 1], prob[idx[1::4], 1] = 0.0, 1.0
        prob[idx[2::4], 1], prob[idx[3::4], 1] = -0.0, 0.5            # (-0.0 ties with 0.0; 0.5 ties with column 0 below)
        prob[idx[3::4], 0] = 0.5
    return prob, y
