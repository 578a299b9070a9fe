"""CPU restatement of the reference's TRAIN-mode choose step with its distances (src/layers.py:633-697) over CSR rows: the
oracle of the train-mode ranked-selection tests.  The neighbour part is tests/ranked_ref.py's (k and the keep-all rule are the
same in both modes); a centre of label 1 is followed by its minority tail - the m = min(int(k * rho), P) training positives
nearest to its score: float32 ``torch.abs``, ``torch.sort(stable=True)`` over train_pos order."""
import math

import numpy as np
import torch

from tests.ranked_ref import ranked_ref


def minority_tail(c, pos_scores, m):
    """One centre: score c (0-dim float32 tensor), the training positives' scores in train_pos order (float32 tensor), m picks.
    Returns (positions in train_pos, distances) of the m nearest, in the reference's order, as numpy arrays."""
    if m <= 0 or len(pos_scores) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    d, order = torch.sort(torch.abs(c - pos_scores), dim=0, descending=False, stable=True)      # layers.py:685-687
    return order[:m].numpy(), d[:m].numpy()


def minority_ref(csr, nodes, labels, s0, thresholds, rho, train_pos, center=None):
    """The minority part of all relations of a batch.  labels: one per node (1 = positive centre); rho: a scalar or one per
    relation; train_pos: the training positives' ids, in order.  Returns (offsets int64 [R, B + 1], ids int32, dist float32)."""
    s0 = torch.as_tensor(np.asarray(s0, dtype=np.float32))
    nodes = np.asarray(nodes, dtype=np.int64).reshape(-1)
    labels = np.asarray(labels).reshape(-1)
    tp = np.asarray(train_pos, dtype=np.int64).reshape(-1)
    pos_scores = s0[torch.from_numpy(tp)]
    cen = s0[torch.from_numpy(nodes)] if center is None else torch.as_tensor(np.asarray(center, dtype=np.float32))
    R, B, P = len(csr), len(nodes), len(tp)
    flat = np.zeros(R * B + 1, dtype=np.int64)
    out_ids, out_dist = [], []
    tails = {}                                                # (centre, m) -> tail: the order does not depend on the relation
    for r, (indptr, _) in enumerate(csr):
        rr = float(rho) if np.isscalar(rho) else float(rho[r])
        for b, v in enumerate(nodes.tolist()):
            deg = int(indptr[v + 1] - indptr[v])
            k = int(math.ceil(deg * float(thresholds[r])))                       # layers.py:260
            m = min(int(k * rr), P) if labels[b] == 1 else 0                      # :675, :681
            if (b, m) not in tails:
                tails[(b, m)] = minority_tail(cen[b], pos_scores, m)
            pos, dist = tails[(b, m)]
            out_ids.append(tp[pos].astype(np.int32))
            out_dist.append(dist.astype(np.float32))
            flat[r * B + b + 1] = flat[r * B + b] + len(pos)
    offsets = np.lib.stride_tricks.as_strided(flat, (R, B + 1), (B * 8, 8)).copy()
    ids = np.concatenate(out_ids).astype(np.int32) if out_ids else np.zeros(0, np.int32)
    dist = np.concatenate(out_dist).astype(np.float32) if out_dist else np.zeros(0, np.float32)
    return offsets, ids, dist


def ranked_train_ref(csr, nodes, labels, s0, thresholds, rho, train_pos, center=None):
    """(neighbour part, minority part): ``ranked_ref``'s and ``minority_ref``'s triples."""
    return (ranked_ref(csr, nodes, s0, thresholds, center=center),
            minority_ref(csr, nodes, labels, s0, thresholds, rho, train_pos, center=center))


# ---- comparison with the reference's own samp_score_diff (tests/golden/ranked_train.npz) ---------------------------------------
def golden_train_rows(z, name, rho, r):
    off, flat = z[f"{name}_rho{rho}_score_off{r}"], z[f"{name}_rho{rho}_scores{r}"]
    return [flat[off[b]:off[b + 1]] for b in range(len(off) - 1)]


def compare_train_with_golden(z, c, rho, neigh, minor, thresholds):
    """Every row of the two parts against the reference: the minority tails bit for bit; of the neighbour part the ranked rows
    bit for bit and the keep-all rows as sorted arrays (the reference returns those in the order of the list it was given);
    the set sizes; the id sets against the golden train-mode selection where the case has one for this rho."""
    (off, ids, dist), (moff, mids, mdist) = neigh, minor
    assert dist.dtype == np.float32 and mdist.dtype == np.float32 and ids.dtype == np.int32 and mids.dtype == np.int32
    labels = z[f"{c.name}_labels"]
    P = len(c.train_pos)
    have_sets = f"rho{rho}_train_sel_off0" in c.z.files
    n_ranked = n_keep = n_minor = 0
    for r in range(c.R):
        want = golden_train_rows(z, c.name, rho, r)
        sets = c.sel(f"rho{rho}_train", r) if have_sets else None
        indptr, _ = c.csr[r]
        for b, v in enumerate(c.nodes):
            lo, hi, mlo, mhi = int(off[r, b]), int(off[r, b + 1]), int(moff[r, b]), int(moff[r, b + 1])
            deg = int(indptr[v + 1] - indptr[v])
            k = int(math.ceil(deg * thresholds[r]))
            assert k == int(z[f"{c.name}_sample_list{r}"][b])
            m = min(int(k * rho), P) if labels[b] == 1 else 0
            assert mhi - mlo == m and len(want[b]) == (hi - lo) + m, (c.name, rho, r, b)
            got_set = set(ids[lo:hi].tolist()) | set(mids[mlo:mhi].tolist())
            assert len(got_set) == int(z[f"{c.name}_rho{rho}_set_len{r}"][b]), (c.name, rho, r, b)
            if sets is not None:
                assert got_set == sets[b], (c.name, rho, r, b)
            head, tail = want[b][:hi - lo], want[b][hi - lo:]
            assert np.array_equal(mdist[mlo:mhi].view(np.uint32), tail.view(np.uint32)), (c.name, rho, r, b)
            n_minor += m > 0
            if deg > k + 1:
                assert np.array_equal(dist[lo:hi].view(np.uint32), head.view(np.uint32)), (c.name, rho, r, b)
                n_ranked += 1
            else:
                assert np.array_equal(np.sort(dist[lo:hi]).view(np.uint32), np.sort(head).view(np.uint32)), (c.name, rho, r, b)
                n_keep += 1
    assert n_ranked > 0 and n_keep > 0 and n_minor > 0, "the fixture must hold ranked, keep-all and minority rows"


def golden_scores(z, c):
    """(s0, centre scores) the reference ranked with: the golden score table with the minority scores the reference used at
    train_pos, and the centres' own"""
    s0 = np.ascontiguousarray(c.z["table_scores"][:, 0]).copy()
    s0[np.asarray(c.train_pos, dtype=np.int64)] = z[f"{c.name}_minor_scores"]
    return s0, z[f"{c.name}_center_scores"]
