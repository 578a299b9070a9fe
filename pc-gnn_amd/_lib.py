"""ctypes binding of libpcgnn_hip.so (the C ABI in include/pcgnn.h).

There is NO fallback: if the library is missing or an entry point is absent the
import of the product path raises.  Build it with ``python -m pcgnn_amd.build``
(or ``__graft_entry__.build()``).
"""
import ctypes as C
import os

from .build import lib_path

PCG_MAX_REL = 8
PCG_OK, PCG_E_ARG, PCG_E_UNSUPPORTED, PCG_E_LAUNCH = 0, -1, -2, -3
PCG_ST_SEL_OVERFLOW = 1
PCG_ST_LIST_ID_RANGE = 2
PCG_ST_SYNC_TIMEOUT = 4
PCG_ST_SORT_OVERFLOW = 8
PCG_ST_EVAL_INPUT = 16
PCG_ST_RANK_MISMATCH = 32
PCG_ST_PR_OVERFLOW = 64
PCG_ALERTS_MAX_K = 65536
PCG_NORM_COUNT, PCG_NORM_SQRT_COUNT = 0, 1
ABI_VERSION = 13


class GraphDesc(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_int64),
        ("feat_dim", C.c_int32),
        ("feat_stride", C.c_int32),
        ("n_rel", C.c_int32),
        ("n_pos", C.c_int32),
        ("max_degree", C.c_int32),
        ("_pad", C.c_int32),
        ("X", C.c_void_p),
        ("train_pos", C.c_void_p),
        ("indptr", C.c_void_p * PCG_MAX_REL),
        ("indices", C.c_void_p * PCG_MAX_REL),
    ]


_P, _I32, _I64, _U64, _F64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double
_G = C.POINTER(GraphDesc)


# The parameter structs of the training entry points (include/pcgnn.h documents every member).  They hold raw addresses: whoever
# builds one keeps the tensors and ctypes arrays it points into alive.  tests/test_cabi_exports.py checks each layout against
# pcg_abi_layout.
class AdamHyper(C.Structure):
    _fields_ = [("lr", _F64), ("beta1", _F64), ("beta2", _F64), ("eps", _F64), ("weight_decay", _F64)]


class TrainState(C.Structure):
    _fields_ = [("theta", _P), ("m", _P), ("v", _P), ("step_counter", _P), ("sync_words", _P), ("clf_next", _P), ("slabs", _P),
                ("acts", _P), ("wg_scratch", _P), ("emb", _I32), ("act_ld", _I32), ("lambda_1", C.c_float), ("_pad", _I32),
                ("hyper", AdamHyper)]


class SelectWs(C.Structure):
    _fields_ = [("thresholds", C.POINTER(_F64)), ("rho", C.POINTER(_F64)), ("workspace", _P), ("status", _P),
                ("list_capacity", _I64), ("add_self", _I32), ("_pad", _I32)]


class Batch(C.Structure):
    _fields_ = [("ids", _P), ("labels", _P), ("cnt", _P), ("plan", _P), ("B", _I32), ("inv_count", C.c_float)]


class DenseOut(C.Structure):
    _fields_ = [("logits", _P), ("center", _P), ("combined", _P), ("row_loss", _P)]


class ExplainOut(C.Structure):
    _fields_ = [("logits", _P), ("d_self", _P), ("d_agg", _P), ("self_contrib", _P), ("rel_contrib", _P), ("out_begin", _P),
                ("out_ids", _P), ("out_dist", _P), ("neigh_contrib", _P)]


ABI_STRUCTS = (AdamHyper, TrainState, SelectWs, Batch, DenseOut, ExplainOut)     # pcg_abi_layout's `which`, in order
_H, _ST, _SEL, _B, _OUT, _XOUT = (C.POINTER(t) for t in ABI_STRUCTS)


class BaselineModel(C.Structure):
    """pcg_baseline_model: the shape and the two weight matrices of a GraphSAGE / GCN baseline (pcg_baseline_infer; not one of
    pcg_abi_layout's structs - those are the training entry points')"""
    _fields_ = [("rel", _I32), ("norm", _I32), ("add_self", _I32), ("concat_self", _I32), ("emb", _I32), ("_pad", _I32),
                ("W_enc", _P), ("W_cls", _P)]


class BaselineOpt(C.Structure):
    """pcg_baseline_opt: the Adam state, the first batch's step number and the hyper-parameters of pcg_baseline_train (apply = 0:
    gradients only)"""
    _fields_ = [("m_enc", _P), ("v_enc", _P), ("m_cls", _P), ("v_cls", _P), ("first_step", _I64), ("apply", _I32), ("_pad", _I32),
                ("hyper", AdamHyper)]


_BM, _BO = C.POINTER(BaselineModel), C.POINTER(BaselineOpt)

# name -> (restype, argtypes); must list every symbol include/pcgnn.h declares
PROTOTYPES = {
    "pcg_version": (C.c_char_p, []),
    "pcg_abi_version": (C.c_int, []),
    "pcg_abi_layout": (_I32, [_I32, C.POINTER(_I64), _I32]),
    "pcg_score_table": (C.c_int, [_G, _P, _P, _I64, _I64, _P, _P]),
    "pcg_score_rows": (C.c_int, [_G, _P, _P, _P, _I32, _P, _P]),
    "pcg_pos_sort_capacity": (_I64, [_I32]),
    "pcg_pos_sort": (C.c_int, [_G, _P, _P, _P]),
    "pcg_choose_workspace_bytes": (_I64, [_G, _I32, _I64]),
    "pcg_choose_workspace_offset": (_I64, [_G, _I32, _I64, _I32]),
    "pcg_choose_select": (C.c_int, [_G, _P, _P, _I32, _P, _P, _P, C.POINTER(_F64), C.POINTER(_F64), _I32, _I32,
                                    _P, _P, _I64, _P, _P]),
    "pcg_aggregate_lists": (C.c_int, [_P, _I32, _I32, _I64, _I32, _P, _G, _I32, _P, _I64, _I32, _P, _I32, _P, _P]),
    "pcg_choose_aggregate": (C.c_int, [_G, _P, _P, _I32, _P, _P, _P, C.POINTER(_F64), C.POINTER(_F64), _I32, _I32,
                                       _I32, _P, _I32, _P, _P, _I64, _P, _P]),
    "pcg_step_front": (C.c_int, [_G, _P, _P, _P, _P, _P, _P, _I32, C.POINTER(_F64), C.POINTER(_F64), _I32, _I32, _P, _I64,
                                 _P, _P]),
    "pcg_step_front_a": (C.c_int, [_G, _P, _P, _I64, _I64, _P, _P, _P, _P, _P, _I32, C.POINTER(_F64), C.POINTER(_F64), _I32, _I32,
                                   _P, _I64, _P, _P]),
    "pcg_step_front_b": (C.c_int, [_G, _P, _P, _I32, _P, _P, _I32, C.POINTER(_F64), C.POINTER(_F64), _I32, _I32, _P, _I64, _P,
                                   _P, _I64, _P]),
    "pcg_choose_select_planned": (C.c_int, [_G, _P, _P, _I32, _P, _P, _P, C.POINTER(_F64), C.POINTER(_F64), _I32, _I32,
                                            _P, _P, _P, _I64, _P, _P, _I64, _P]),
    "pcg_step_scores": (C.c_int, [_G, _P, _P, _I64, _I64, _P, _P, _P, _I64, _P, _P, _P]),
    "pcg_choose_gather_train": (C.c_int, [_G, _B, _P, _P, _SEL, _P, _I32, _ST, _I32, _P, _I32, _P]),
    "pcg_choose_train_part": (C.c_int, [_I32, _G, _B, _P, _P, _SEL, _P, _I32, _ST, _I32, _P, _I32, _P, _P]),
    "pcg_dense_select_train": (C.c_int, [_G, _ST, _SEL, _B, _B, _P, _I32, _P, _OUT, _P, _P, _P, _P]),
    "pcg_dense_select_blocks": (_I32, [_G, _I32, _I32]),
    "pcg_dense_select_ahead": (C.c_int, [_G, _ST, _SEL, _B, _B, _B, _P, _I32, _P, _OUT, _P, _P, _P, _P, _P]),
    "pcg_dense_select_ahead_ok": (_I32, [_G, _I32, _I32]),
    "pcg_clf_step": (C.c_int, [_G, _B, _ST, _P, _I32, _P]),
    "pcg_choose_plan_bytes": (_I64, [_G, _I32, _I64]),
    "pcg_choose_data_bytes": (_I64, [_G, _I32, _I64]),
    "pcg_plan_batches": (C.c_int, [_G, _P, _P, _I32, _I32, C.POINTER(_F64), C.POINTER(_F64), _I32, _I32, _P, _I64, _I64, _P, _P,
                                   _P]),
    "pcg_plan_epochs": (C.c_int, [_G, _P, _P, _I32, _I32, _I32, C.POINTER(_F64), C.POINTER(_F64), _I32, _I32, _P, _I64, _I64, _P, _P,
                                  _P]),
    "pcg_pick_shuffled_epochs": (C.c_int, [_P, _P, _I32, _U64, _U64, _P, _I32, _I32, _I32, _P, _P, _P, _P]),
    "pcg_pos_sort_in_select": (_I32, [_I32]),
    "pcg_pos_sort_one_launch": (_I32, [_I32]),
    "pcg_pos_sort_raw": (C.c_int, [_G, _P, _P, _P]),
    "pcg_sync_words_count": (_I32, []),
    "pcg_aggregate_lists_planned": (C.c_int, [_P, _I32, _I32, _I64, _I32, _P, _G, _I32, _P, _P, _I64, _I32, _P, _I32, _P, _P]),
    "pcg_gather_lists_planned": (C.c_int, [_P, _I32, _I32, _I64, _I32, _P, _G, _I32, _P, _P, _I64, _P, _I32, _P, _P]),
    "pcg_step_scores_train": (C.c_int, [_G, _ST, _P, _P, _P, _P]),
    "pcg_touched_bytes": (_I64, [_I64]),
    "pcg_mark_touched": (C.c_int, [_G, _P, _I32, _I32, _P, _I64, _P, _P]),
    "pcg_mark_touched_planned": (C.c_int, [_G, _P, _I32, _I32, _P, _I64, _I64, _P, _I64, _P]),
    "pcg_choose_aggregate_planned": (C.c_int, [_G, _P, _P, _I32, _P, _P, _P, C.POINTER(_F64), C.POINTER(_F64), _I32, _I32,
                                               _I32, _P, _I32, _P, _P, _I64, _P, _P]),
    "pcg_choose_gather_planned": (C.c_int, [_G, _P, _P, _I32, _P, _P, _P, C.POINTER(_F64), C.POINTER(_F64), _I32, _I32,
                                            _P, _I32, _P, _P, _P, _I64, _P, _P, _P]),
    "pcg_gather_lists": (C.c_int, [_P, _I32, _I32, _I64, _I32, _P, _G, _I32, _P, _I64, _P, _I32, _P, _P]),
    "pcg_train_dense": (C.c_int, [_G, _ST, _B, _P, _I32, _SEL, _OUT, _I32, _P, _P]),
    "pcg_dense_sorts_keys": (_I32, [_I32, _I32]),
    "pcg_infer_workspace_bytes": (_I64, [_G, _I32, _I32, _I64]),
    "pcg_infer_set": (C.c_int, [_G, _P, _I32, _P, _I32, _I32, _P, C.POINTER(_F64), _P, _I64, _P, _P, _P, _P]),
    "pcg_infer_blocks": (_I32, [_I32]),
    "pcg_infer_dist_workspace_bytes": (_I64, [_G, _I32, _I32, _I64]),
    "pcg_infer_chunk_dist": (C.c_int, [_G, _P, _I32, _P, _I32, _I32, _P, _I64, _P, _P, _I32, _I32, _I32, _P, _P, _P, _I64, _P, _P,
                                       C.POINTER(_F64), _P, _I32, _I64, _P, _P, _P, _P]),
    "pcg_infer_new_workspace_bytes": (_I64, [_G, _G, _I32, _I32, _I64]),
    "pcg_infer_new": (C.c_int, [_G, _G, _P, _I32, _P, _I32, _I32, _P, _I32, C.POINTER(_F64), _P, _I64, _P, _P, _P, _P]),
    "pcg_embed_set": (C.c_int, [_G, _P, _I32, _P, _I32, _I32, _P, C.POINTER(_F64), _P, _I64, _P, _P, _P, _P, _P, _P]),
    "pcg_embed_new": (C.c_int, [_G, _G, _P, _I32, _P, _I32, _I32, _P, _I32, C.POINTER(_F64), _P, _I64, _P, _P, _P, _P, _P, _P]),
    "pcg_baseline_workspace_bytes": (_I64, [_G, _BM, _I32]),
    "pcg_baseline_infer": (C.c_int, [_G, _BM, _P, _I32, _I32, _P, _I64, _P, _P, _P, _P, _P]),
    "pcg_baseline_train_workspace_bytes": (_I64, [_G, _BM, _I32]),
    "pcg_baseline_train": (C.c_int, [_G, _BM, _BO, _P, _P, _I32, _I32, _P, _I64, _P, _P, _P, _P]),
    "pcg_topk_similar_workspace_bytes": (_I64, [_I32, _I32, _I32, _I32]),
    "pcg_topk_similar": (C.c_int, [_P, _I32, _P, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P]),
    "pcg_debug_set_topk_slices": (None, [_I32]),
    "pcg_explain_new_workspace_bytes": (_I64, [_G, _G, _I32, _I32, _I64]),
    "pcg_explain_new": (C.c_int, [_G, _G, _P, _I32, _P, _I32, _I32, _P, _I32, C.POINTER(_F64), _P, _I64, C.c_float, C.c_float, _XOUT,
                                  _P, _P]),
    "pcg_rank_lists": (C.c_int, [_G, _P, _I32, _P, _P, _P, _I64, _P, _P, _P, _P, _P]),
    "pcg_rank_minority": (C.c_int, [_G, _P, _I32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "pcg_chosen_workspace_bytes": (_I64, [_G, _I32, _I64]),
    "pcg_chosen_set": (C.c_int, [_G, _P, _I32, _P, _I32, _I32, _P, C.POINTER(_F64), _P, _I64, _P, _P, _P, _P, _P]),
    "pcg_attr_set": (C.c_int, [_G, _P, _I32, _P, _I32, _I32, _P, C.POINTER(_F64), _P, _I64, C.c_float, C.c_float, _P, _P, _P, _P, _P,
                               _P, _P]),
    "pcg_attr_neighbours": (C.c_int, [_G, _P, _P, _I32, _I32, _P, _P, _P, _P]),
    "pcg_eval_workspace_bytes": (_I64, [_I64, _I32]),
    "pcg_eval_counts": (C.c_int, [_P, _P, _I64, _P, _I32, _P, _P, _P, _P]),
    "pcg_pr_workspace_bytes": (_I64, [_I64]),
    "pcg_pr_counts": (C.c_int, [_P, _P, _I64, _I64, _P, _P, _P, _P, _P, _P]),
    "pcg_topk_alerts_workspace_bytes": (_I64, [_I64, _I32]),
    "pcg_topk_alerts": (C.c_int, [_P, _I32, _I64, _I32, _P, _P, _P, _P, _P]),
    "pcg_alert_cases_workspace_bytes": (_I64, [_I64, _I32]),
    "pcg_alert_cases": (C.c_int, [_G, _P, _I32, C.c_uint32, _P, _P, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "pcg_step_front_train": (C.c_int, [_G, _ST, _P, _P, _B, _SEL, _P]),
    "pcg_grad_reduce": (C.c_int, [_P, _I32, _I64, _P, _P, _P]),
    "pcg_adam_apply_pending": (C.c_int, [_P, _P, _P, _P, _I64, _P, _P, _I32, _H, _P]),
    "pcg_adam_flush": (C.c_int, [_ST, _I32, _I64, _I64, _I32, _I32, _P]),
    "pcg_wgrad_act_rows": (_I64, [_I32, _I32, _I32]),
    "pcg_wgrad_scratch_bytes": (_I64, [_I32, _I32, _I32, _I32]),
    "pcg_wgrad": (C.c_int, [_ST, _I32, _I32, _I32, _P, _I32, _I32, _P, _P]),
    "pcg_dense_vjp": (C.c_int, [_G, _ST, _B, _P, _I32, _SEL, _P, _P, _OUT, _P]),
    "pcg_step_scores_dist": (C.c_int, [_G, _ST, _P, _P, _I64, _I64, _P, _P, _P, _I64, _P]),
    "pcg_gather_lists_dist": (C.c_int, [_P, _I32, _I32, _I64, _I32, _P, _G, _I32, _P, _P, _I64, _P, _I32, _P, _I32, _I32, _I32, _P, _P,
                                        _I32, _P, _I64, _P, _I32, _I32, _P, _P, _P, _I64, _I32, _P, _P]),
    "pcg_debug_set_stamps": (None, [_P]),
    "pcg_debug_set_dense_stamps": (None, [_P]),
    "pcg_sel_capacity_row": (_I64, [_I64, _F64, _F64, _I32, _I32, _I32]),
    "pcg_segment_mean": (C.c_int, [_G, _P, _P, _P, _I32, _I32, _P, _I32, _P]),
    "pcg_pick": (C.c_int, [_P, _P, _I32, _P, _U64, _U64, _I32, _P, _P]),
    "pcg_pick_shuffled": (C.c_int, [_P, _P, _I32, _U64, _U64, _P, _I32, _I32, _P, _P, _P, _P]),
    "pcg_gather_rows": (C.c_int, [_G, _P, _I32, _P, _I32, _P]),
    "pcg_halo_table_slots": (_I64, [_I32]),
    "pcg_halo_serve": (C.c_int, [_G, _P, _I32, _I32, _I32, _P, _I32, _P]),
    "pcg_halo_collect": (C.c_int, [_G, _P, _I32, _I32, _I32, _I32, _P, _I32, _P, _I32, _P, _I64, _P, _P, _I32, _I32, _I32, _I32,
                                   _P]),
    "pcg_halo_lookup": (C.c_int, [_G, _I32, _P, _P, _I64, _I32, _I32, _I32, _P, _P, _I32, _P, _I64, _P, _I32, _I32, _P]),
    "pcg_dense_n_params": (_I64, [_I32, _I32, _I32]),
    "pcg_dense_param_offset": (_I64, [_I32, _I32, _I32, _I32, _I32]),
    "pcg_dense_n_tiles": (_I32, [_I32]),
    "pcg_dense_step": (C.c_int, [_G, _P, _I32, _P, _P, _I32, _P, _I32, C.c_float, C.c_float, _P, _P, _P, _P, _P, _P,
                                 _P]),
    "pcg_adam_step": (C.c_int, [_P, _P, _P, _P, _I32, _I64, _P, _H, _P, _I32, _P]),
}

_lib = None


class PcgnnLibraryError(RuntimeError):
    pass


def load():
    """Load the shared library once; raise (never fall back) if that fails."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise PcgnnLibraryError(
            f"{path} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (needs hipcc). There is no CPU fallback for the product path.")
    lib = C.CDLL(path)
    for name, (res, args) in PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise PcgnnLibraryError(f"{path} does not export {name}: stale build? rebuild it") from e
        fn.restype = res
        fn.argtypes = args
    if lib.pcg_abi_version() != ABI_VERSION:
        raise PcgnnLibraryError(f"{path}: ABI {lib.pcg_abi_version()} != expected {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


_ERR = {PCG_E_ARG: "bad argument", PCG_E_UNSUPPORTED: "unsupported shape", PCG_E_LAUNCH: "kernel launch failed"}


def check(rc, what):
    if rc != PCG_OK:
        raise PcgnnLibraryError(f"{what} failed: {_ERR.get(rc, rc)} ({rc})")
