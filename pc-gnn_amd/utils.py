"""Host-side helpers around the hot path, mirroring the reference's src/utils.py where the
training / evaluation loop touches them: ``test`` (:280-333), ``pos_neg_split`` (:256-271),
``normalize`` (:212-222), ``sparse_to_adjlist_for_train`` / graph ingestion (:226-254), ``set_seeds``.

``test`` keeps the reference's signature and return value; predictions stay on the device for the
whole pass and come back in ONE copy (the reference copies every batch, :305), and the
degenerate empty trailing batch its ``int(len/B)+1`` produces is not run.  A fused engine's pass is
one ``FusedPCGNN.infer`` call (``predict_proba``); a partitioned model's (``DistributedPCGNN``) is a
collective ``infer_global`` call on every rank, with global test node ids.  Metrics are computed
with numpy restatements of the sklearn functions the reference calls (checked against sklearn in
the tests), so evaluation does not depend on sklearn being installed.
"""
import random
from typing import Optional, Tuple

import numpy as np
import torch


# ---- metrics (sklearn.metrics.{accuracy,f1,precision,recall,roc_auc}_score restated) --------------
def _prf(y, p, cls):
    tp = float(np.sum((p == cls) & (y == cls)))
    fp = float(np.sum((p == cls) & (y != cls)))
    fn = float(np.sum((p != cls) & (y == cls)))
    prec = tp / (tp + fp) if tp + fp > 0 else 0.0         # zero_division=0 (utils.py:319)
    rec = tp / (tp + fn) if tp + fn > 0 else 0.0
    f1 = 2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0
    return prec, rec, f1


def binary_metrics(y_true, y_pred, y_score) -> dict:
    y = np.asarray(y_true).astype(np.int64)
    p = np.asarray(y_pred).astype(np.int64)
    p1, r1, f1 = _prf(y, p, 1)
    p0, r0, f0 = _prf(y, p, 0)
    return {"accuracy": float(np.mean(y == p)), "f1": f1, "f1_macro": (f1 + f0) / 2, "precision": p1,
            "precision_macro": (p1 + p0) / 2, "recall": r1, "recall_macro": (r1 + r0) / 2, "auc": roc_auc(y, y_score)}


def roc_auc(y_true, score) -> float:
    """Area under the ROC curve = Mann-Whitney U with average ranks for ties."""
    y = np.asarray(y_true).astype(bool)
    s = np.asarray(score, dtype=np.float64)
    n1, n0 = int(y.sum()), int((~y).sum())
    if n1 == 0 or n0 == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    order = np.argsort(s, kind="mergesort")
    ranks = np.empty(len(s), dtype=np.float64)
    sorted_s = s[order]
    i = 0
    while i < len(s):
        j = i
        while j + 1 < len(s) and sorted_s[j + 1] == sorted_s[i]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    return float((ranks[y].sum() - n1 * (n1 + 1) / 2.0) / (n1 * n0))


def _prf_counts(tp, fp, fn):
    """_prf from the three counts (the same statements)."""
    tp, fp, fn = float(tp), float(fp), float(fn)
    prec = tp / (tp + fp) if tp + fp > 0 else 0.0
    rec = tp / (tp + fn) if tp + fn > 0 else 0.0
    f1 = 2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0
    return prec, rec, f1


def metrics_from_counts(counts, thresholds=None) -> dict:
    """PURE HOST.  Every metric ``binary_metrics`` / ``roc_auc`` / ``get_best_f1`` / ``test_f1`` report, from the integer
    vector ``pcg_eval_counts`` forms (ops.eval_counts): counts [8 + 2 T] = tp, fp, fn, tn, n1, n0, 2U, 0, tp_t[T], npred_t[T].
    The float64 arithmetic from the integers on is the statements of those functions, so the values are ``==`` theirs:
    the keys of binary_metrics (same ValueError when a class is absent), plus ``best_f1`` / ``best_threshold`` (get_best_f1's
    rule: the first threshold wins, it must beat 0), ``best_index`` (its position, -1 if none) and ``f1_macro_at`` (a list:
    test_f1's F1-macro of the prediction ``p > thresholds[i]``)."""
    c = [int(v) & 0xFFFFFFFFFFFFFFFF for v in np.asarray(counts).reshape(-1).tolist()]
    th = np.linspace(0.01, 0.99, 100) if thresholds is None else np.asarray(thresholds, dtype=np.float64).reshape(-1)
    T = len(th)
    if len(c) != 8 + 2 * T:
        raise ValueError(f"metrics_from_counts: {len(c)} words for {T} thresholds (8 + 2 T expected)")
    tp, fp, fn, tn, n1, n0, two_u = c[:7]
    if n1 == 0 or n0 == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    p1, r1, f1 = _prf_counts(tp, fp, fn)
    p0, r0, f0 = _prf_counts(tn, fn, fp)
    m = {"accuracy": float(np.float64(tp + tn) / (n1 + n0)), "f1": f1, "f1_macro": (f1 + f0) / 2, "precision": p1,
         "precision_macro": (p1 + p0) / 2, "recall": r1, "recall_macro": (r1 + r0) / 2,
         "auc": float((two_u / 2.0) / (n1 * n0))}
    tp_t = np.array(c[8:8 + T], dtype=np.float64)
    n_pred = np.array(c[8 + T:8 + 2 * T], dtype=np.float64)
    denom = n_pred + float(n1)                                         # 2TP + FP + FN
    f1_t = np.where(denom > 0, 2.0 * tp_t / np.maximum(denom, 1.0), 0.0)
    best_f1, best_t, best_i = 0.0, 0.0, -1
    for i, (f, t) in enumerate(zip(f1_t, th)):
        if f > best_f1:
            best_f1, best_t, best_i = float(f), float(t), i
    macro = []
    for i in range(T):
        tpi, npi = c[8 + i], c[8 + T + i]
        fpi, fni = npi - tpi, n1 - tpi
        macro.append(0.5 * (_prf_counts(tpi, fpi, fni)[2] + _prf_counts(n0 - fpi, fni, fpi)[2]))
    m.update(best_f1=best_f1, best_threshold=best_t, best_index=best_i, f1_macro_at=macro)
    return m


def device_metrics(prob_dev, labels, thresholds=None) -> dict:
    """metrics_from_counts of class probabilities that are on the device: ops.eval_counts (HIP) + ONE copy of 8 + 2 T words
    (with the status word) + the host arithmetic.  labels: int32 on the device, or anything ops._i32 takes."""
    from . import _lib, ops
    lab = labels if torch.is_tensor(labels) and labels.dtype == torch.int32 and labels.device == prob_dev.device \
        else ops._i32(labels, prob_dev.device)
    th = ops.eval_thresholds(thresholds)
    status = ops.eval_status(prob_dev.device)
    counts = ops.eval_counts(prob_dev, lab.view(-1), None if thresholds is None else th)
    words = torch.cat([counts, status.to(torch.int64)]).cpu().numpy()
    if int(words[-1]):
        status.zero_()
        if int(words[-1]) & _lib.PCG_ST_EVAL_INPUT:
            raise _lib.PcgnnLibraryError("evaluation input: a label outside {0, 1} or a NaN probability")
        raise _lib.PcgnnLibraryError(f"device status {int(words[-1])}")
    return metrics_from_counts(words[:-1], th)


def _device_eval(test_nodes, labels, model, batch_size: int, thresholds=None) -> dict:
    """The on_device evaluation of ``test`` / ``test_f1``: a model that has ``evaluate`` (FusedPCGNN, DistributedPCGNN) runs it;
    the others' batch probabilities are concatenated on the device and go through device_metrics."""
    nodes = np.asarray(test_nodes)
    if hasattr(model, "evaluate") and (getattr(model, "eval_by_infer", True)):
        return model.evaluate(nodes, labels, thresholds=thresholds)
    y = np.asarray(labels)
    with torch.no_grad():
        outs = []
        fused = hasattr(model, "predict")
        ids_dev = torch.as_tensor(nodes, dtype=torch.int32, device=model.dev) if fused else None
        for start in range(0, len(nodes), batch_size):
            if fused:
                outs.append(torch.sigmoid(model.predict(ids_dev[start:start + batch_size], None, False)[0]))
            else:
                outs.append(model.to_prob(nodes[start:start + batch_size].tolist(), y[start:start + batch_size], train_flag=False)[0])
        if not outs:
            raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
        prob = torch.cat(outs).float()
    if hasattr(model, "check"):
        model.check()
    return device_metrics(prob, y, thresholds)


# ---- ranking metrics: average precision, G-mean, precision / recall at k ---------------------------------------------------------
# A row's key is its positive-class score p1 compared as a number (-0.0 ties with +0.0).  The ALERT ORDER is the stable sort of the
# rows by key, descending: among equal keys the lower position in the input comes first.
_ONE_CLASS = "Only one class present in y_true. ROC AUC score is not defined in that case."


def _ranking_inputs(labels, score):
    y = np.asarray(labels).astype(np.int64).reshape(-1)
    s = np.asarray(score).reshape(-1)
    if s.dtype.kind != "f":
        s = s.astype(np.float64)
    if len(y) != len(s):
        raise ValueError(f"{len(y)} labels for {len(s)} scores")
    if np.any((y != 0) & (y != 1)) or np.any(np.isnan(s)):
        raise ValueError("evaluation input: a label outside {0, 1} or a NaN probability")
    return y, s


def pr_points(labels, score):
    """(n1, tp_g, npred_g): with u_1 > ... > u_G the distinct scores of the rows with label 1 - the only points at which recall
    changes - tp_g = #{y = 1, p1 >= u_g} and npred_g = #{p1 >= u_g}, int64, in descending score order (what pcg_pr_counts
    forms on the device)."""
    y, s = _ranking_inputs(labels, score)
    ps = np.sort(s[y == 1])
    n1 = len(ps)
    u, head = np.unique(ps, return_index=True)                         # ascending; head = first index of each value
    tp = (n1 - head).astype(np.int64)[::-1]
    npred = (len(s) - np.searchsorted(np.sort(s), u, side="left")).astype(np.int64)[::-1]
    return n1, tp, npred


def _average_precision_from_points(n1: int, tp, npred) -> float:
    import math
    tp = np.asarray(tp, dtype=np.int64)
    d = np.diff(np.concatenate([np.zeros(1, np.int64), tp]))
    terms = (d.astype(np.float64) / np.float64(n1)) * (tp.astype(np.float64) / np.asarray(npred).astype(np.float64))
    return math.fsum(terms.tolist())                                   # (exactly rounded: independent of any order)


def average_precision(labels, score) -> float:
    """Average precision (sklearn.metrics.average_precision_score's definition: the sum over the points where recall changes of
    (recall step) * precision), from integers: terms (d tp / n1) * (tp / npred) in float64, added with math.fsum.  ValueError
    when there is no positive."""
    n1, tp, npred = pr_points(labels, score)
    if n1 == 0:
        raise ValueError(_ONE_CLASS)
    return _average_precision_from_points(n1, tp, npred)


def conf_gmean(conf) -> float:
    """The reference's G-mean of a 2 x 2 confusion matrix [[tn, fp], [fn, tp]] (src/utils.py:454-456), on Python ints.
    ValueError when a class is absent."""
    tn, fp, fn, tp = (int(v) for v in np.asarray(conf).ravel())
    if tp + fn == 0 or tn + fp == 0:
        raise ValueError(_ONE_CLASS)
    return (tp * tn / ((tp + fn) * (tn + fp))) ** 0.5


def alert_order(score) -> np.ndarray:
    """Positions of the rows in alert order: the stable sort by score, descending (equal scores: the lower position first)."""
    s = np.asarray(score).reshape(-1)
    return np.argsort(-(s + s.dtype.type(0)), kind="stable")


def _rates_at_k(hits_at, ks, n: int, n1: int):
    """precision_at / recall_at from hits_at(ke) = positives among the first ke alerts (int / int in Python)."""
    if n == 0 or n1 == 0:
        raise ValueError(_ONE_CLASS if n else "precision / recall at k of an empty set")
    prec, rec = {}, {}
    for k in ks:
        k = int(k)
        if k < 1:
            raise ValueError("precision / recall at k: k >= 1")
        ke = min(k, n)
        h = int(hits_at(ke))
        prec[k], rec[k] = h / ke, h / n1
    return prec, rec


def precision_recall_at_k(labels, score, ks):
    """(precision_at, recall_at), dicts keyed by k: with hits = the positives among the first ke = min(k, n) rows of the alert
    order, precision_at[k] = hits / ke and recall_at[k] = hits / n1.  A tie at the cut is resolved by input position: among
    equal scores the lower position in the input is ranked first."""
    y, s = _ranking_inputs(labels, score)
    hits = np.cumsum(y[alert_order(s)])
    return _rates_at_k(lambda ke: hits[ke - 1], ks, len(y), int(y.sum()))


def ranking_from_counts(hdr, tp_g, npred_g) -> dict:
    """PURE HOST.  average_precision, gmean, n_pos, n_neg and n_points from what ``pcg_pr_counts`` forms (ops.pr_counts):
    hdr [8] = tp, fp, fn, tn, n1, n0, G, 0 and the first G entries of tp_g / npred_g.  The float64 statements are
    ``average_precision``'s and ``conf_gmean``'s, so the values are ``==`` theirs; the same ValueError when a class is absent."""
    h = [int(v) & 0xFFFFFFFFFFFFFFFF for v in np.asarray(hdr).reshape(-1).tolist()]
    if len(h) != 8:
        raise ValueError(f"ranking_from_counts: a header of {len(h)} words (8 expected)")
    tp, fp, fn, tn, n1, n0, G = h[:7]
    if n1 != tp + fn or n0 != fp + tn:
        raise ValueError("ranking_from_counts: n1 / n0 are not the confusion words' sums")
    if G > n1:
        raise ValueError(f"ranking_from_counts: {G} points for {n1} positives")
    tpg = np.asarray(tp_g).reshape(-1).astype(np.int64) & 0xFFFFFFFF
    npg = np.asarray(npred_g).reshape(-1).astype(np.int64) & 0xFFFFFFFF
    if len(tpg) < G or len(npg) < G:
        raise ValueError(f"ranking_from_counts: {G} points, {min(len(tpg), len(npg))} entries")
    if n1 == 0 or n0 == 0:
        raise ValueError(_ONE_CLASS)
    return {"average_precision": _average_precision_from_points(n1, tpg[:G], npg[:G]),
            "gmean": conf_gmean([[tn, fp], [fn, tp]]), "n_pos": n1, "n_neg": n0, "n_points": G}


def host_ranking(labels, prob, ks=()) -> dict:
    """The ranking metrics of class probabilities [n, 2] that are on the host - what ``device_ranking`` returns: average_precision,
    gmean (of the argmax prediction, p1 > p0), precision_at / recall_at (dicts keyed by k; ties at the cut by input position),
    n_pos, n_points."""
    prob = np.asarray(prob).reshape(-1, 2)
    y, s = _ranking_inputs(labels, prob[:, 1])
    if np.any(np.isnan(prob[:, 0])):
        raise ValueError("evaluation input: a label outside {0, 1} or a NaN probability")
    pred = prob.argmax(axis=1)
    conf = [[int(np.sum((pred == 0) & (y == 0))), int(np.sum((pred == 1) & (y == 0)))],
            [int(np.sum((pred == 0) & (y == 1))), int(np.sum((pred == 1) & (y == 1)))]]
    n1, tp, npred = pr_points(y, s)
    if n1 == 0 or n1 == len(y):
        raise ValueError(_ONE_CLASS)
    prec, rec = precision_recall_at_k(y, s, ks) if len(ks) else ({}, {})
    return {"average_precision": _average_precision_from_points(n1, tp, npred), "gmean": conf_gmean(conf),
            "precision_at": prec, "recall_at": rec, "n_pos": n1, "n_points": len(tp)}


def device_ranking(prob_dev, labels, ks=(), cap: Optional[int] = None) -> dict:
    """``host_ranking`` of class probabilities that are on the device: ops.pr_counts and - for the k below n - ops.topk_alerts, a
    gather of the labels and a cumulative sum (HIP / torch on the device), then the host arithmetic (``ranking_from_counts``).
    cap: the capacity for the precision-recall points; the number of positives suffices.  With a cap ONE copy brings the header,
    the status word, the hit counts and the cap pairs; cap None (n would be needed): the pairs follow in a second copy of
    exactly G.  labels: int32 on the device, or anything ops._i32 takes.  A k below n is at most PCG_ALERTS_MAX_K (65536).  A
    tie at the cut k is resolved by input position."""
    from . import _lib, ops
    dev = prob_dev.device
    lab = labels if torch.is_tensor(labels) and labels.dtype == torch.int32 and labels.device == dev else ops._i32(labels, dev)
    lab = lab.view(-1)
    n = int(prob_dev.shape[0])
    ks = [int(k) for k in ks]
    if any(k < 1 for k in ks):
        raise ValueError("precision / recall at k: k >= 1")
    cut = sorted({k for k in ks if k < n})                             # (k >= n: every row, hits = n1)
    if cut and cut[-1] > _lib.PCG_ALERTS_MAX_K:
        raise ValueError(f"device_ranking: k {cut[-1]} is above PCG_ALERTS_MAX_K {_lib.PCG_ALERTS_MAX_K} and below n {n}")
    status = ops.eval_status(dev)
    hdr, tp_g, npred_g = ops.pr_counts(prob_dev, lab, cap)
    parts = [hdr, status.to(torch.int64)]
    if cut:
        pos, _ = ops.topk_alerts(prob_dev, cut[-1])
        hits = torch.cumsum((lab[pos.long()] != 0).to(torch.int64), 0)
        parts.append(hits[torch.tensor([k - 1 for k in cut], dtype=torch.int64, device=dev)])
    if cap is not None:
        parts += [tp_g.to(torch.int64), npred_g.to(torch.int64)]
    words = torch.cat(parts).cpu().numpy()
    st = int(words[8])
    if st:
        status.zero_()
        if st & _lib.PCG_ST_EVAL_INPUT:
            raise _lib.PcgnnLibraryError("evaluation input: a label outside {0, 1} or a NaN probability")
        if st & _lib.PCG_ST_PR_OVERFLOW:
            raise _lib.PcgnnLibraryError(f"pr_counts: {int(words[6])} precision-recall points do not fit cap {tp_g.numel()}")
        raise _lib.PcgnnLibraryError(f"device status {st}")
    hits_at = {k: int(h) for k, h in zip(cut, words[9:9 + len(cut)])}
    if cap is not None:
        c = tp_g.numel()
        pairs = words[9 + len(cut):]
        m = ranking_from_counts(words[:8], pairs[:c], pairs[c:2 * c])
    else:
        G = min(int(words[6]), tp_g.numel())
        pairs = torch.cat([tp_g[:G], npred_g[:G]]).cpu().numpy()
        m = ranking_from_counts(words[:8], pairs[:G], pairs[G:])
    hits_at[n] = m["n_pos"]
    prec, rec = _rates_at_k(lambda ke: hits_at[ke], ks, n, m["n_pos"]) if ks else ({}, {})
    return {"average_precision": m["average_precision"], "gmean": m["gmean"], "precision_at": prec, "recall_at": rec,
            "n_pos": m["n_pos"], "n_points": m["n_points"]}


def test_ranking(test_nodes, labels, model, batch_size: int, ks=(100, 1000), on_device: bool = False,
                 print_line: Optional[bool] = True) -> dict:
    """The ranking metrics of ``model`` on ``test_nodes``: average_precision, gmean, precision_at / recall_at (dicts keyed by k),
    n_pos, n_points - the same dict both ways.  Host way (every model): ``predict_proba`` -> ``host_ranking``.  on_device: an
    engine that has ``evaluate_ranking`` (FusedPCGNN) keeps the probabilities on the device.  A tie at the cut k is resolved
    by input position.  Prints one line in the style of ``test``."""
    labels = np.asarray(labels)
    if on_device:
        if not hasattr(model, "evaluate_ranking"):
            raise ValueError("test_ranking(on_device=True) needs an engine that has evaluate_ranking")
        m = model.evaluate_ranking(np.asarray(test_nodes), labels, ks=ks)
    else:
        prob = predict_proba(test_nodes, model, batch_size, labels)
        if hasattr(model, "check"):
            model.check()
        m = host_ranking(labels, prob, ks)
    if print_line:
        at = "".join(f"\t- P@{k}: {m['precision_at'][k]:.4f}\t- R@{k}: {m['recall_at'][k]:.4f}" for k in m["precision_at"])
        print(f"- AveragePrecision: {m['average_precision']:.4f}\t- G-mean: {m['gmean']:.4f}{at}\t\n", end="")
    return m


def predict_proba_new(query, model, ids=None, chunk=None) -> np.ndarray:
    """Positive-class probabilities (float32, on the host) of the rows ``ids`` (None = all) of a ``graph.QueryBatch`` - new
    nodes scored against the resident graph by ``FusedPCGNN.infer_new``: column 1 of the same sigmoid statement as
    ``predict_proba``'s, so ``predict_proba_new(q, fz) == predict_proba(N + ids, full, B)[:, 1]`` for an engine ``full``
    whose graph has the query rows appended."""
    with torch.no_grad():
        return np.ascontiguousarray(torch.sigmoid(model.infer_new(query, ids=ids, chunk=chunk)).float().cpu().numpy()[:, 1])


def explain_nodes(engine, ids, labels=None, attribute: bool = False):
    """A flagged node's score and its reason in one call: (``engine.chosen(ids)`` - the neighbours the model listened to, ranked,
    with their distances - , the test-mode class probabilities [n, 2] ``predict_proba`` reports for the same ids), on the device.
    labels (one per id, 0 / 1): the train-mode lists - the training positives a fraud centre is over-sampled with beside its
    neighbours (``engine.chosen(ids, labels=labels, train_flag=True)``); the probabilities stay the test-mode ones.
    attribute=True: a third value, ``engine.attribute(ids, neighbours=True)`` - how much of the fraud logit each of the node's
    own features, each relation and each (test-mode) chosen neighbour accounts for."""
    with torch.no_grad():
        ch = engine.chosen(ids) if labels is None else engine.chosen(ids, labels=labels, train_flag=True)
        prob = torch.sigmoid(engine.infer(ids)).float()
        if not attribute:
            return ch, prob
        return ch, prob, engine.attribute(ids, neighbours=True)


def explain_new(engine, query, ids=None, attribute: bool = False):
    """``explain_nodes`` for nodes that are NOT in the graph - the rows ``ids`` (query-local; None = all) of a
    ``graph.QueryBatch``: (``engine.chosen_new(query, ids)`` - the neighbours the model listened to, ranked, with their
    distances; global ids -, the test-mode class probabilities [n, 2] - sigmoid of ``infer_new``'s logits), on the device.
    attribute=True: a third value, the ``Attribution`` - and then everything comes from ONE
    ``engine.attribute_new(query, ids, neighbours=True)`` call (its ``chosen``, sigmoid of its ``logits``): one selection per
    chunk, one read of the status word."""
    with torch.no_grad():
        if attribute:
            at = engine.attribute_new(query, ids=ids, neighbours=True)
            return at.chosen, torch.sigmoid(at.logits).float(), at
        ch = engine.chosen_new(query, ids=ids)
        return ch, torch.sigmoid(engine.infer_new(query, ids=ids)).float()


def similar_examples(engine, ids, k: int = 5, labels=None, query=None):
    """Example-based explanation in one call: (``engine.nearest(ids, k)`` - the k training positives each node's embedding is
    closest to (cosine), as ``graph.NearestExamples`` -, the test-mode class probabilities [n, 2] of the same ids), on the
    device.  labels (one per graph node, 0 / 1; a tensor, array or list): a third value, the labels of the examples
    [n, k] int64, -1 where a row is padded.  query: the ids are rows of that ``graph.QueryBatch`` (new nodes)."""
    with torch.no_grad():
        near = engine.nearest(ids, k=k, query=query)
        logits = engine.infer(ids) if query is None else engine.infer_new(query, ids=ids)
        prob = torch.sigmoid(logits).float()
        if labels is None:
            return near, prob
        lab = torch.as_tensor(np.asarray(labels.cpu() if torch.is_tensor(labels) else labels)).to(near.ids.device).long().view(-1)
        ex = torch.where(near.ids >= 0, lab[near.ids.clamp(min=0).long()], torch.full_like(near.ids, -1, dtype=torch.long))
        return near, prob, ex


def alert_cases(model_or_engine, ids, k: int = 100, labels=None, relations=None):
    """The k highest-scoring rows of ``ids`` grouped into cases - rings of alerts linked through the graph's relations - as
    ``graph.CaseList``, for any model or engine that has ``alerts`` (FusedPCGNN, BaselineEngine, GraphSage, GCN): its own
    ``cases`` where it has one, else ``alerts`` -> ``ops.group_members`` on the engine's graph.  labels (one per row of ids,
    0 / 1): the positives per case.  relations: None = all.  Out of scope: query batches, partitioned graphs, 2-hop linking."""
    if hasattr(model_or_engine, "cases"):
        return model_or_engine.cases(ids, k=k, relations=relations, labels=labels)
    if not hasattr(model_or_engine, "alerts") or not hasattr(model_or_engine, "g"):
        raise ValueError("alert_cases needs a model or engine that has alerts (and its resident graph)")
    from . import ops
    al = model_or_engine.alerts(ids, k=k)
    slot_labels = None
    if labels is not None:
        lab = torch.as_tensor(np.asarray(labels.cpu() if torch.is_tensor(labels) else labels)).to(al.pos.device).to(torch.int32).view(-1)
        if lab.numel() != al.n:
            raise ValueError(f"alert_cases: {lab.numel()} labels for {al.n} rows")
        slot_labels = lab[al.pos.clamp(min=0).long()] if al.n else torch.zeros_like(al.pos)
    return ops.group_members(model_or_engine.g, al.ids, relations=relations, labels=slot_labels, alerts=al)


def predict_proba(test_nodes, model, batch_size: int, labels=None) -> np.ndarray:
    """Test-mode class probabilities [n, 2] of ``test_nodes`` (sigmoid of the gnn logits, utils.py:305), on the host.
    A FusedPCGNN runs its whole-set pass (``infer``: one call, one score pass) - test-mode results do not depend on how the
    nodes are batched, so this is bit for bit the per-batch ``predict`` loop - unless it was given a selection-list capacity of
    its own (``eval_by_infer`` False): then it is evaluated batch by batch under that capacity, as before.  ``batch_size``
    batches those and the other models (``to_prob``, ``labels`` passed along).  A DistributedPCGNN: COLLECTIVE - every rank
    passes the same global node ids and gets every one's probabilities (``infer_global``)."""
    nodes = np.asarray(test_nodes)
    if len(nodes) == 0:
        return np.zeros((0, 2), np.float32)
    from .dist import DistributedPCGNN
    with torch.no_grad():
        if isinstance(model, DistributedPCGNN):
            return torch.sigmoid(model.infer_global(nodes)).float().cpu().numpy()
        if getattr(model, "eval_by_infer", False):
            ids = torch.as_tensor(nodes, dtype=torch.int32, device=model.dev)
            return torch.sigmoid(model.infer(ids)).float().cpu().numpy()
        fused = hasattr(model, "predict")                                   # FusedPCGNN: ids go to the device ONCE, batches are views
        ids_dev = torch.as_tensor(nodes, dtype=torch.int32, device=model.dev) if fused else None
        outs = []
        for start in range(0, len(nodes), batch_size):                      # :298-303 (no empty trailing batch)
            if fused:
                outs.append(torch.sigmoid(model.predict(ids_dev[start:start + batch_size], None, False)[0]))
            else:
                blab = None if labels is None else np.asarray(labels)[start:start + batch_size]
                outs.append(model.to_prob(nodes[start:start + batch_size].tolist(), blab, train_flag=False)[0])   # :305
    return torch.cat(outs).float().cpu().numpy()


def test(test_nodes, labels, model, batch_size: int, result=None, epoch: Optional[int] = None,
         epoch_best: Optional[int] = None, flag: Optional[str] = None,
         print_line: Optional[bool] = True, on_device: bool = False) -> Tuple[float, float, float, float]:
    """Evaluate ``model`` (PCALayer / GCN / GraphSage mirror, or a FusedPCGNN) on ``test_nodes``:
    batched ``to_prob(..., train_flag=False)`` -> argmax / positive-class confidence -> metrics.
    Returns (auc, recall, f1_macro, precision) like the reference (utils.py:333).  Test-mode results do not depend on the
    batching: a FusedPCGNN evaluates the whole set in one pass (predict_proba); ``batch_size`` batches the other models.
    on_device: the probabilities stay on the device and the metrics come from the integer counts formed there
    (``model.evaluate`` / device_metrics): the same values, the same line, one small copy instead of [n, 2] floats + numpy."""
    labels = np.asarray(labels)
    if on_device:
        m = _device_eval(test_nodes, labels, model, batch_size)
    else:
        prob = predict_proba(test_nodes, model, batch_size, labels)
        if hasattr(model, "check"):
            model.check()          # a batch that overflowed its selection list must not pass for a prediction
        pred = prob.argmax(axis=1)                                               # :306
        m = binary_metrics(labels, pred, prob[:, 1])                             # :308, :316-323
    line = (f"- F1: {m['f1']:.4f}\t- Recall: {m['recall']:.4f}\t- Precision: {m['precision']:.4f}\t"
            f"- Accuracy: {m['accuracy']:.4f}\t- AUC-ROC: {m['auc']:.4f}\t- F1-macro: {m['f1_macro']:.4f}\t"
            f"- Recall-macro: {m['recall_macro']:.4f}\t- AP: {m['precision_macro']:.4f}\t\n")   # :325
    if result is not None:
        args = (m["accuracy"], m["f1"], m["f1_macro"], m["precision"], m["precision_macro"], m["recall"],
                m["recall_macro"], m["auc"], line, print_line)
        if flag == "val":
            result.write_val_log(epoch, epoch_best, *args)
        elif flag == "test":
            result.write_test_log(epoch_best, *args)
    elif print_line:
        print(line, end="")
    return m["auc"], m["recall"], m["f1_macro"], m["precision"]


def get_best_f1(labels, probs, thresholds=None) -> Tuple[float, float]:
    """Best positive-class F1 over the reference's 100 thresholds linspace(0.01, 0.99) and the threshold reaching it
    (the "(f1)" variant, src/utils(f1).py:334-350: one sklearn f1_score call per threshold; the first threshold wins
    ties).  Here: one sort of the confidences, then every threshold's TP / FP by binary search."""
    y = np.asarray(labels).astype(np.int64)
    p = np.asarray(probs, dtype=np.float64)
    th = np.linspace(0.01, 0.99, 100) if thresholds is None else np.asarray(thresholds, dtype=np.float64)
    order = np.argsort(p, kind="stable")
    ps, ys = p[order], y[order]
    pos_from = np.concatenate([np.cumsum(ys[::-1])[::-1], [0]])       # positives among ps[i:]
    first = np.searchsorted(ps, th, side="right")                     # predictions 1: probs > thresh  (:345)
    tp = pos_from[first].astype(np.float64)
    n_pred = (len(ps) - first).astype(np.float64)
    n_pos = float(ys.sum())
    denom = n_pred + n_pos                                             # 2TP + FP + FN
    f1 = np.where(denom > 0, 2.0 * tp / np.maximum(denom, 1.0), 0.0)
    best_f1, best_t = 0.0, 0.0                                         # :342 (a threshold must beat 0 to be taken)
    for f, t in zip(f1, th):
        if f > best_f1:
            best_f1, best_t = float(f), float(t)
    return best_f1, best_t


def test_f1(test_nodes, labels, model, batch_size: int, flag: str = "valid", valid_thresh: Optional[float] = None,
            on_device: bool = False):
    """The "(f1)" evaluation (src/utils(f1).py:280-332): F1-macro at the best validation threshold (flag "valid":
    searched here and returned; otherwise ``valid_thresh`` is applied), the other metrics from the argmax prediction.
    Returns (auc, recall, f1_macro, precision, threshold) like the reference.  Probabilities as ``test`` (predict_proba).
    on_device: as ``test``; flag "valid" takes the best threshold and the F1-macro at it from the 100-threshold sweep's counts,
    otherwise the sweep is the one threshold ``valid_thresh``."""
    y = np.asarray(labels)
    if on_device:
        if flag == "valid":
            m = _device_eval(test_nodes, y, model, batch_size)
            threshold = m["best_threshold"]
            if m["best_index"] >= 0:
                f1_macro = m["f1_macro_at"][m["best_index"]]
            else:                                                     # no threshold beat 0: the cut is get_best_f1's 0.0
                f1_macro = _device_eval(test_nodes, y, model, batch_size, thresholds=[threshold])["f1_macro_at"][0]
            return m["auc"], m["recall"], f1_macro, m["precision"], threshold
        m = _device_eval(test_nodes, y, model, batch_size, thresholds=[valid_thresh])
        return m["auc"], m["recall"], m["f1_macro_at"][0], m["precision"], None
    prob = predict_proba(test_nodes, model, batch_size, y)
    if hasattr(model, "check"):
        model.check()
    threshold = None
    if flag == "valid":
        _, threshold = get_best_f1(y, prob[:, 1])                     # :316-317
        cut = threshold
    else:
        cut = valid_thresh                                            # :320
    preds = (prob[:, 1] > cut).astype(np.int64)
    f1_macro = 0.5 * (_prf(y, preds, 1)[2] + _prf(y, preds, 0)[2])    # :318 / :322
    m = binary_metrics(y, prob.argmax(axis=1), prob[:, 1])            # :324-330
    return m["auc"], m["recall"], f1_macro, m["precision"], threshold


# ---- data helpers ------------------------------------------------------------------------------------
def pos_neg_split(nodes, labels):
    """positive / negative node ids in input order (utils.py:256-271, which is O(n^2) there)."""
    nodes = list(nodes)
    lab = np.asarray(labels)
    pos = [n for n, l in zip(nodes, lab) if l == 1]
    neg = [n for n, l in zip(nodes, lab) if l != 1]
    return pos, neg


def normalize(mx):
    """Row-normalise a dense or scipy-sparse feature matrix: x / (rowsum + 0.01) (utils.py:212-222)."""
    import scipy.sparse as sp
    rowsum = np.array(mx.sum(1)) + 0.01
    r_inv = np.power(rowsum, -1).flatten()
    r_inv[np.isinf(r_inv)] = 0.
    return sp.diags(r_inv).dot(mx)


def sparse_to_csr(sp_matrix):
    """What sparse_to_adjlist_for_train (utils.py:243-254) builds - self-loops added, symmetrised - but
    straight to the device layout: (indptr int64, indices int32 ascending), no dict-of-sets in between."""
    import scipy.sparse as sp
    a = sp.csr_matrix(sp_matrix)
    a = a + a.T + sp.eye(a.shape[0], format="csr")
    a.sum_duplicates()
    a.sort_indices()
    return a.indptr.astype(np.int64), a.indices.astype(np.int32)


def set_seeds(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


# ---- stratified train / valid / test split (src/model_handler.py:36-48) ------------------------------------------------------
def _approximate_mode(class_counts: np.ndarray, n_draws: int, rng: np.random.RandomState) -> np.ndarray:
    """How many of n_draws go to every class: proportional, the remainders settled largest first with random tie-breaks
    (scikit-learn 1.7 ``utils/_approximate_mode``; consumes the generator exactly as it does)."""
    continuous = class_counts / class_counts.sum() * n_draws
    floored = np.floor(continuous)
    need = int(n_draws - floored.sum())
    if need > 0:
        remainder = continuous - floored
        for value in np.sort(np.unique(remainder))[::-1]:
            (inds,) = np.where(remainder == value)
            add_now = min(len(inds), need)
            inds = rng.choice(inds, size=add_now, replace=False)
            floored[inds] += 1
            need -= add_now
            if need == 0:
                break
    return floored.astype(int)


def train_test_split(index, labels, stratify, train_size: Optional[float] = None, test_size: Optional[float] = None,
                     random_state: int = 0, shuffle: bool = True):
    """``sklearn.model_selection.train_test_split(index, labels, stratify=labels, train_size=... | test_size=...,
    random_state=seed, shuffle=True)`` restated (scikit-learn 1.7: one StratifiedShuffleSplit draw) so that the splits
    the reference makes (model_handler.py:42-43, 47-48) can be reproduced without scikit-learn: same generator
    (``np.random.RandomState(seed)``), same order of draws, same outputs - checked against scikit-learn in the tests.
    Returns (idx_train, idx_test, y_train, y_test) as lists / arrays like the reference consumes them."""
    assert shuffle and stratify is not None
    index, labels, y = list(index), np.asarray(labels), np.asarray(stratify)
    n = len(index)
    if test_size is None and train_size is None:
        test_size = 0.25
    # scikit-learn's _validate_shuffle_split for float sizes
    n_test = int(np.ceil(test_size * n)) if test_size is not None else None
    n_train = int(np.floor(train_size * n)) if train_size is not None else None
    if n_train is None:
        n_train = n - n_test
    elif n_test is None:
        n_test = n - n_train
    if n_train + n_test > n or n_train <= 0:
        raise ValueError("train_size / test_size do not fit the number of samples")
    rng = np.random.RandomState(random_state)
    classes, y_indices = np.unique(y, return_inverse=True)
    class_counts = np.bincount(y_indices)
    if class_counts.min() < 2:
        raise ValueError("The least populated class in y has only 1 member, which is too few.")
    if n_train < len(classes) or n_test < len(classes):
        raise ValueError("fewer samples than classes in one side of the split")
    class_indices = np.split(np.argsort(y_indices, kind="mergesort"), np.cumsum(class_counts)[:-1])
    n_i = _approximate_mode(class_counts, n_train, rng)
    t_i = _approximate_mode(class_counts - n_i, n_test, rng)
    train, test = [], []
    for i in range(len(classes)):
        perm = class_indices[i].take(rng.permutation(class_counts[i]), mode="clip")
        train.extend(perm[:n_i[i]])
        test.extend(perm[n_i[i]:n_i[i] + t_i[i]])
    train, test = rng.permutation(train), rng.permutation(test)
    pick = lambda seq, ids: [seq[i] for i in ids]
    return pick(index, train), pick(index, test), labels[train], labels[test]


def split_dataset(labels, train_ratio: float, test_ratio: float, seed: int, first_labeled: int = 0):
    """The reference's train / valid / test split (model_handler.py:36-48): nodes [first_labeled, N) (Amazon: the first 3305 -
    amazon_new: 2013 - are unlabeled), ``train_ratio`` of them for training, ``test_ratio`` of the rest for testing, both
    stratified, both seeded with ``seed``.  Returns idx_train, y_train, idx_valid, y_valid, idx_test, y_test."""
    labels = np.asarray(labels)
    index = list(range(first_labeled, len(labels)))
    lab = labels[first_labeled:]
    idx_train, idx_rest, y_train, y_rest = train_test_split(index, lab, stratify=lab, train_size=train_ratio, random_state=seed)
    idx_valid, idx_test, y_valid, y_test = train_test_split(idx_rest, y_rest, stratify=y_rest, test_size=test_ratio, random_state=seed)
    return idx_train, y_train, idx_valid, y_valid, idx_test, y_test
