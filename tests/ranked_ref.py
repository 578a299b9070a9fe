"""CPU restatement of the reference's test-mode choose step with its distances (src/layers.py:713-736) over CSR rows: the
oracle of the ranked-selection tests.  float32 ``torch.abs``; ``torch.sort(stable=True)`` where the reference ranks
(deg > k + 1: ascending distance, ties by position in the row); the row's own order where it keeps every neighbour."""
import math

import numpy as np
import torch


def ranked_row(c, ids, s, k):
    """One row: centre score c (0-dim float32 tensor), neighbour ids (int array, the row's order), their scores s (float32
    tensor), k = num_sample.  Returns (kept ids, distances) as numpy arrays in the reference's order."""
    ids = np.asarray(ids)
    if len(ids) == 0:
        return ids.astype(np.int32), np.zeros(0, np.float32)
    diff = torch.abs(c - s)                                   # layers.py:721
    if len(ids) > k + 1:                                      # :726
        d, order = torch.sort(diff, dim=0, descending=False, stable=True)
        order = order[:k].numpy()
        return ids[order].astype(np.int32), d[:k].numpy()
    return ids.astype(np.int32), diff.numpy()                 # :730-731


def ranked_ref(csr, nodes, s0, thresholds, center=None):
    """All relations of a batch.  csr: [(indptr, indices)] per relation; nodes: centre ids; s0: float32 scores [n_nodes];
    thresholds: one per relation; center: the centres' scores [B] if they are not s0[nodes].
    Returns (offsets int64 [R, B + 1] into the flat arrays, ids int32, dist float32) - the layout of ``ChosenLists``."""
    s0 = torch.as_tensor(np.asarray(s0, dtype=np.float32))
    nodes = np.asarray(nodes, dtype=np.int64).reshape(-1)
    cen = s0[torch.from_numpy(nodes)] if center is None else torch.as_tensor(np.asarray(center, dtype=np.float32))
    R, B = len(csr), len(nodes)
    flat = np.zeros(R * B + 1, dtype=np.int64)
    out_ids, out_dist = [], []
    for r, (indptr, indices) in enumerate(csr):
        for b, v in enumerate(nodes.tolist()):
            row = np.asarray(indices[indptr[v]:indptr[v + 1]])
            k = int(math.ceil(len(row) * float(thresholds[r])))            # layers.py:260
            ids, dist = ranked_row(cen[b], row, s0[torch.from_numpy(row.astype(np.int64))], k)
            out_ids.append(ids)
            out_dist.append(dist.astype(np.float32))
            flat[r * B + b + 1] = flat[r * B + b] + len(ids)
    offsets = np.lib.stride_tricks.as_strided(flat, (R, B + 1), (B * 8, 8)).copy()
    ids = np.concatenate(out_ids).astype(np.int32) if out_ids else np.zeros(0, np.int32)
    dist = np.concatenate(out_dist).astype(np.float32) if out_dist else np.zeros(0, np.float32)
    return offsets, ids, dist


# ---- comparison with the reference's own samp_scores (tests/golden/ranked.npz) --------------------------------------------
def golden_rows(z, name, r):
    off, flat = z[f"{name}_score_off{r}"], z[f"{name}_scores{r}"]
    return [flat[off[b]:off[b + 1]] for b in range(len(off) - 1)]


def compare_with_golden(z, c, offsets, ids, dist, thresholds):
    """Every row of (offsets, ids, dist) against the reference: ranked rows bit for bit, keep-all rows as sorted arrays (the
    reference returns those in CPython set-iteration order), the id sets against the golden selection."""
    assert dist.dtype == np.float32 and ids.dtype == np.int32
    n_ranked = n_keep = 0
    for r in range(c.R):
        want = golden_rows(z, c.name, r)
        sets = c.sel("test", r)
        indptr, _ = c.csr[r]
        for b, v in enumerate(c.nodes):
            lo, hi = int(offsets[r, b]), int(offsets[r, b + 1])
            deg = int(indptr[v + 1] - indptr[v])
            k = int(math.ceil(deg * thresholds[r]))
            assert k == int(z[f"{c.name}_sample_list{r}"][b])
            assert set(ids[lo:hi].tolist()) == sets[b], (c.name, r, b)
            assert hi - lo == len(want[b]) == int(z[f"{c.name}_set_len{r}"][b])
            if deg > k + 1:
                assert np.array_equal(dist[lo:hi].view(np.uint32), want[b].view(np.uint32)), (c.name, r, b)
                n_ranked += 1
            else:
                assert np.array_equal(np.sort(dist[lo:hi]).view(np.uint32), np.sort(want[b]).view(np.uint32)), (c.name, r, b)
                n_keep += 1
    assert n_ranked > 0 and n_keep > 0, "the fixture must hold both kinds of row"
