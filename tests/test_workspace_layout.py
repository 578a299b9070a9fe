"""CPU check of the workspace layout (no GPU): the selection list sits at the same place in the data part for every batch size,
ahead of the partial sums, so the list a select launch writes for one batch never overlaps the partial sums that another batch
size's dense tiles read beside it (the pipelined step's fused launch)."""
import ctypes as C


def test_list_before_partial_sums_for_every_batch_size():
    import pcgnn_amd
    from pcgnn_amd import _lib
    pcgnn_amd.build_library()
    lib = _lib.load()
    for feat_stride, max_degree, cap in ((32, 3000, 50_000), (32, 3000, 3_000_000), (28, 40_000, 777_777)):
        g = _lib.GraphDesc()
        g.n_nodes, g.feat_dim, g.feat_stride, g.n_rel, g.n_pos, g.max_degree = 100_000, feat_stride, feat_stride, 3, 500, max_degree
        ref = None
        for B in (1, 64, 255, 256, 1024, 2048, 4096):
            plan = lib.pcg_choose_plan_bytes(C.byref(g), B, cap)
            lst = lib.pcg_choose_workspace_offset(C.byref(g), B, cap, 2) - plan
            part = lib.pcg_choose_workspace_offset(C.byref(g), B, cap, 6) - plan
            assert plan > 0 and lst >= 0 and part >= lst + 4 * cap, (B, plan, lst, part)
            assert ref is None or (lst, part) == ref, "the list and the start of the partial sums move with the batch size"
            ref = (lst, part)
