"""numpy statement of what pcg_baseline_infer computes (include/pcgnn.h; src/graphsage.py:62-96, 127-150, 167-174, 200-232,
262-275), in float64 and in float32, for the five model shapes the reference's classes can express.

For a centre v: S(v) = its CSR row, united with v when add_self is set and v is not in it; c = |S(v)|;
a(v) = sum(X[u], u in S(v)) / c (norm 0) or / sqrt(c) (norm 1) - c == 0 gives 0 / 0 = NaN -; z = [X[v] | a(v)] or a(v);
h = relu(W_enc z) with a ReLU that lets NaN through; logits = W_cls h.
"""
import glob
import os

import numpy as np

NORM_COUNT, NORM_SQRT_COUNT = 0, 1
FEAT_TOL = 2e-5          # tests/test_gpu_parity.py: aggregated features / activations (s1_mean, s1_mean_gcn, s1_gcn, s1_sage_enc)
GCN_ENC_TOL = 5e-5       # tests/test_gpu_parity.py: s1_gcn_enc


def s1_cases():
    """names of the golden fixtures that hold the reference's GraphSAGE / GCN outputs (the ``s1_*`` arrays)"""
    from tests.util import GOLDEN
    names = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))):
        with np.load(path) as z:
            if "s1_nodes" in z.files:
                names.append(os.path.splitext(os.path.basename(path))[0])
    return names


# name -> what BaselineEngine.from_model must read off the classes
SHAPES = {
    "sage_concat": dict(concat_self=True, add_self=False, norm=NORM_COUNT),        # Encoder(gcn=False), MeanAggregator(gcn=False)
    "sage_concat_self": dict(concat_self=True, add_self=True, norm=NORM_COUNT),    # Encoder(gcn=False), MeanAggregator(gcn=True)
    "sage": dict(concat_self=False, add_self=False, norm=NORM_COUNT),              # Encoder(gcn=True), MeanAggregator(gcn=False): the handler's SAGE
    "sage_self": dict(concat_self=False, add_self=True, norm=NORM_COUNT),          # Encoder(gcn=True), MeanAggregator(gcn=True)
    "gcn": dict(concat_self=False, add_self=True, norm=NORM_SQRT_COUNT),           # GCNEncoder, GCNAggregator
}


def w_enc_in_lds(F, E, concat_self) -> bool:
    """whether the dense launch stages W_enc in LDS (baseline.hip: baseline_wlds) or streams it from L2: the floats of
    z [16][Kp + 1] | K-split parts [kparts][16][E] | h [16][E + 1] | W_cls [2][E] | W_enc [E][Kp + 1] within 160 KB"""
    K = 2 * F if concat_self else F
    Kp = (K + 15) // 16 * 16
    kparts = 4 // (E // 16) if E // 16 <= 4 else 1
    return 4 * (16 * (Kp + 1) + kparts * 16 * E + 16 * (E + 1) + 2 * E + E * (Kp + 1)) <= 160 * 1024


def build_model(GS, graph, F, E, shape_name, seed=0, device="cuda"):
    """the GraphSage / GCN of pcgnn_amd.graphsage (GS) for a shape, over a DeviceGraph, xavier weights under `seed`"""
    import torch
    torch.manual_seed(seed)
    if shape_name == "gcn":
        enc = GS.GCNEncoder(None, F, E, graph, GS.GCNAggregator(None, cuda=True), cuda=True)
        model = GS.GCN(2, enc)
    else:
        s = SHAPES[shape_name]
        enc = GS.Encoder(None, F, E, graph, GS.MeanAggregator(None, cuda=True, gcn=s["add_self"]), gcn=not s["concat_self"], cuda=True)
        model = GS.GraphSage(2, enc)
    return model.to(device) if device is not None else model


def neighbourhoods(csr, ids, add_self):
    """(ptr int64 [n + 1], flat int64): S(v) of every id, ascending ids, the centre united when add_self"""
    indptr, indices = csr
    rows = []
    for v in np.asarray(ids, dtype=np.int64):
        row = np.asarray(indices[indptr[v]:indptr[v + 1]], dtype=np.int64)
        if add_self and not np.any(row == v):
            row = np.sort(np.append(row, v))
        rows.append(row)
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    return ptr, (np.concatenate(rows) if rows else np.zeros(0, np.int64))


def aggregate(X, csr, ids, add_self, norm, dtype=np.float64, hoods=None):
    """a [n, F] in `dtype`: every sum, the count's square root and the division in that type"""
    X = np.asarray(X)
    ptr, flat = neighbourhoods(csr, ids, add_self) if hoods is None else hoods
    n, F = len(ptr) - 1, X.shape[1]
    c = np.diff(ptr)
    gathered = np.concatenate([X[flat].astype(dtype), np.zeros((1, F), dtype)])      # (+ a row for an empty last set)
    sums = np.add.reduceat(gathered, ptr[:-1], axis=0) if n else np.zeros((0, F), dtype)
    sums[c == 0] = 0                                                                 # (reduceat returns the next row there)
    den = c.astype(dtype)
    if norm == NORM_SQRT_COUNT:
        den = np.sqrt(den)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (sums / den[:, None]).astype(dtype)


def forward(X, csr, ids, W_enc, W_cls, concat_self, add_self, norm, dtype=np.float64, hoods=None):
    """-> (logits [n, 2], h [n, E], a [n, F]) in `dtype`"""
    X = np.asarray(X)
    ids = np.asarray(ids, dtype=np.int64)
    a = aggregate(X, csr, ids, add_self, norm, dtype, hoods)
    z = np.concatenate([X[ids].astype(dtype), a], axis=1) if concat_self else a
    with np.errstate(invalid="ignore"):
        pre = z @ np.asarray(W_enc).astype(dtype).T
        h = np.where(pre <= 0, dtype(0), pre)                # (NaN <= 0 is False: NaN goes through, as torch's relu)
        logits = h @ np.asarray(W_cls).astype(dtype).T
    return logits.astype(dtype), h.astype(dtype), a
