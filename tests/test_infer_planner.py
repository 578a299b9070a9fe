"""CPU checks of FusedPCGNN.infer's host-side planner: per-id list capacities (the exact pcg_sel_capacity_row sums of a test-mode
selection), chunk bounds and the ids every whole-set call accepts."""
from types import SimpleNamespace

import numpy as np


def graph(seed=0, n=500, R=3):
    rs = np.random.RandomState(seed)
    deg = [np.concatenate([rs.randint(0, 40, size=n - 3), [0, 1, 5000]]).astype(np.int64) for _ in range(R)]
    return SimpleNamespace(R=R, deg_host=deg, n_pos=17)


def test_row_caps_are_the_exact_sel_capacity_sums():
    from pcgnn_amd import ops
    from pcgnn_amd.fused import infer_row_caps
    g = graph()
    thr = [0.2, 0.5, 0.8]
    rs = np.random.RandomState(1)
    ids = rs.randint(0, 500, size=777)                                  # (any order, duplicates)
    want = ops.sel_capacity(g, ids, None, thr, 0.5, train_flag=False).sum(axis=0)
    assert np.array_equal(infer_row_caps(g.deg_host, thr, ids), want)
    # ids=None: every node, straight from the degree arrays
    want_all = ops.sel_capacity(g, np.arange(500), None, thr, 0.5, train_flag=False).sum(axis=0)
    assert np.array_equal(infer_row_caps(g.deg_host, thr), want_all)


def test_chunks_cover_every_id_once_and_capacity_is_the_largest_chunk():
    from pcgnn_amd.fused import infer_chunks
    rs = np.random.RandomState(2)
    caps = rs.randint(0, 100, size=1001).astype(np.int64)
    for chunk in (1, 16, 333, 1000, 1001, 5000):
        bounds, cap = infer_chunks(caps, chunk)
        covered = np.concatenate([np.arange(lo, hi) for lo, hi in bounds])
        assert np.array_equal(covered, np.arange(len(caps)))
        assert all(hi - lo == chunk for lo, hi in bounds[:-1]) and 0 < bounds[-1][1] - bounds[-1][0] <= chunk
        assert cap == max(int(caps[lo:hi].sum()) for lo, hi in bounds)
    assert infer_chunks(np.zeros(0, np.int64), 16) == ([], 1)
    assert infer_chunks(np.zeros(5, np.int64), 16)[1] == 1               # (a capacity of at least one entry)


def test_default_chunk_keeps_the_workspace_within_its_bound():
    from pcgnn_amd.fused import default_infer_chunk
    caps = np.full(100_000, 10, np.int64)
    ws = lambda c, cap: 100 * c + 4 * cap                               # (a workspace that grows with the chunk)
    assert default_infer_chunk(caps, ws, 1 << 40) == 100_000            # whole set: one chunk
    c = default_infer_chunk(caps, ws, 3_000_000)
    assert 16384 <= c < 100_000 and ws(c, 10 * c) <= 3_000_000
    assert default_infer_chunk(caps, ws, 10) == 16384                   # never under 16384 rows
    assert default_infer_chunk(caps[:1000], ws, 10) == 1000             # (a set smaller than that: one chunk)


def test_ids_helper_accepts_tensor_array_list_and_none():
    import pytest
    import torch
    from pcgnn_amd.fused import whole_set_ids
    dev, rows = torch.device("cpu"), 40
    want = [7, 7, 0, 39, 3, 1]
    got = [whole_set_ids(ids, rows, dev, "infer: ids")
           for ids in (torch.tensor(want), torch.tensor(want, dtype=torch.int32), np.array(want), np.array([want], np.int16), want)]
    for host, on_dev, n in got:
        assert n == len(want) and host.dtype == np.int64 and host.tolist() == want
        assert on_dev.dtype == torch.int32 and on_dev.device == dev and on_dev.tolist() == want
    # None: every row, no host copy; a cached arange of the right length is handed back as it is
    host, on_dev, n = whole_set_ids(None, rows, dev, "infer: ids")
    assert host is None and n == rows and on_dev.dtype == torch.int32 and on_dev.tolist() == list(range(rows))
    assert whole_set_ids(None, rows, dev, "infer: ids", all_ids=on_dev)[1] is on_dev
    assert whole_set_ids(None, rows + 1, dev, "infer: ids", all_ids=on_dev)[1].tolist() == list(range(rows + 1))
    for empty in ([], np.zeros(0, np.int64), torch.zeros(0, dtype=torch.int64)):
        host, on_dev, n = whole_set_ids(empty, rows, dev, "infer: ids")
        assert n == 0 and host.size == 0 and on_dev.numel() == 0
    # the range check: the messages of infer, chosen, infer_new and the partitioned infer
    for bad in (-1, rows):
        with pytest.raises(ValueError, match=r"^infer: ids outside 0 \.\. 39$"):
            whole_set_ids([1, bad], rows, dev, "infer: ids")
        with pytest.raises(ValueError, match=r"^chosen: ids outside 0 \.\. 39$"):
            whole_set_ids(np.array([bad]), rows, dev, "chosen: ids")
        with pytest.raises(ValueError, match=r"^infer_new: ids outside 0 \.\. 39 \(query-local rows\)$"):
            whole_set_ids(torch.tensor([bad]), rows, dev, "infer_new: ids", " (query-local rows)")
        with pytest.raises(ValueError, match=r"^infer: ids_local outside 0 \.\. 39$"):
            whole_set_ids([bad], rows, dev, "infer: ids_local")


# the number of output arguments of each whole-set entry point (include/pcgnn.h): logits, center | + emb, rel | logits, d_self,
# d_agg, self_contrib, rel_contrib | out_begin, out_ids, out_dist | the ExplainOut struct
ENTRY_OUTPUTS = {"pcg_infer_set": 2, "pcg_embed_set": 4, "pcg_attr_set": 5, "pcg_chosen_set": 3,
                 "pcg_infer_new": 2, "pcg_embed_new": 4, "pcg_explain_new": 1}
QUERY_CALLS = {"pcg_infer_new", "pcg_embed_new", "pcg_explain_new"}
WEIGHTED_CALLS = {"pcg_attr_set", "pcg_explain_new"}


def test_argument_tuples_match_the_prototypes():
    from pcgnn_amd import _lib
    from pcgnn_amd.wholeset import whole_set_args
    head = ("g", "theta", "E", "ids", "n", "chunk", "s0")
    for name, n_out in ENTRY_OUTPUTS.items():
        outputs = tuple(f"out{i}" for i in range(n_out))
        args = whole_set_args(head, ("thr", "ws", "cap"), outputs, ("status", "stream"),
                              ("q", "score_base") if name in QUERY_CALLS else None, ("w0", "w1") if name in WEIGHTED_CALLS else ())
        assert len(args) == len(_lib.PROTOTYPES[name][1]), name
        assert len(set(args)) == len(args) and args[0] == "g" and args[-2:] == ("status", "stream"), name
        assert (args[1] == "q") == (name in QUERY_CALLS) == ("q" in args), name
        assert (args[args.index("s0") + 1] == "score_base") == (name in QUERY_CALLS) == ("score_base" in args), name
        cap = args.index("cap")
        assert args[cap - 2:cap + 1] == ("thr", "ws", "cap") and args[args.index("s0") + 1:cap - 2] in ((), ("score_base",)), name
        assert (args[cap + 1:cap + 3] == ("w0", "w1")) == (name in WEIGHTED_CALLS) == ("w0" in args), name
        assert args[-2 - n_out:-2] == outputs, name
        without_q = tuple(a for a in args if a != "q")
        assert without_q[:7] == head, name


def test_workspace_table_covers_the_seven_entry_points():
    from pcgnn_amd import _lib
    from pcgnn_amd.wholeset import WORKSPACES
    assert set(WORKSPACES) == set(ENTRY_OUTPUTS)
    for name, (key, size_fn) in WORKSPACES.items():
        assert key in ("ws", "chosen_ws", "new_ws") and size_fn in _lib.PROTOTYPES and size_fn.endswith("_workspace_bytes"), name
        # the size function takes the call's graph descriptors, (the embedding width,) the chunk and the list capacity
        n_desc = 2 if name in QUERY_CALLS else 1
        assert len(_lib.PROTOTYPES[size_fn][1]) == n_desc + (0 if size_fn == "pcg_chosen_workspace_bytes" else 1) + 2, name
        assert (key == "new_ws") == (name in QUERY_CALLS), name


def test_target_weights_are_two_finite_floats():
    import pytest
    from pcgnn_amd.wholeset import _target_weights
    assert _target_weights("attribute", (0.0, 1.0)) == (0.0, 1.0)
    w = _target_weights("attribute_new", (-1, 1))
    assert w == (-1.0, 1.0) and all(type(v) is float for v in w)
    for what in ("attribute", "attribute_new", "chosen_new"):
        for bad in ((float("nan"), 1), (float("inf"), 0), "ab", (1,), None):
            with pytest.raises(ValueError, match=rf"^{what}: target must be two finite floats, got "):
                _target_weights(what, bad)


def test_fused_keeps_the_planner_names_and_the_alias_imports_the_module():
    import pcgnn_amd.fused as fused
    import pcgnn_amd.wholeset as wholeset
    for name in ("infer_row_caps", "infer_chunks", "default_infer_chunk", "whole_set_ids", "whole_set_workspace", "whole_set_chunk",
                 "whole_set_buffers"):
        assert getattr(fused, name) is getattr(wholeset, name)
    assert issubclass(fused.FusedPCGNN, wholeset.WholeSetCalls)
    assert "__init__" not in vars(wholeset.WholeSetCalls)
