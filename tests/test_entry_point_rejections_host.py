"""CPU-only: the return code of every selection / gather entry point (csrc/choose.hip, csrc/gather.hip) for calls that are
refused, or that return early, before anything is enqueued.  The ORDER of the argument checks decides between PCG_E_ARG and
PCG_E_UNSUPPORTED when two of them fail at once, so it is part of the behaviour: ROWS is one table of
(entry point, what differs from a call that would pass, expected code), the codes are literals, and they were recorded from the
library as it was before the host code behind these entry points was restructured.

There is no device here and the pointers are host memory (a 256-byte-aligned dummy buffer, NULL stream): a row that passed its
checks would try to launch.  No row does - PCG_E_LAUNCH is not an expected code anywhere in the table - which is also why
pcg_step_front_a(B = 0) (it scores the table), a NULL `status` of the gather calls (not checked) and the feature-table checks of
pcg_choose_aggregate* (they sit behind the select launch) have no rows.  A `plan` cannot be handed to a non-planned call through
the C ABI (only the *_planned prototypes have the parameter), so that check has no row either."""
import ctypes as C

from pcgnn_amd import _lib

OK, ARG, UNS = 0, -1, -2          # PCG_OK, PCG_E_ARG, PCG_E_UNSUPPORTED (literals on purpose)

_RAW = C.create_string_buffer(1 << 18)
_BASE = (C.addressof(_RAW) + 255) // 256 * 256


def P(k):
    """non-NULL, 256-byte-aligned dummy number k"""
    return _BASE + 4096 * k


THR, RHO = (C.c_double * 8)(*([0.5] * 8)), (C.c_double * 8)(*([0.5] * 8))
HYPER = _lib.AdamHyper(0.01, 0.9, 0.999, 1e-8, 0.0)

# a graph, a state, a batch and a workspace that pass every check (feat_dim 8: n_params = pcg_dense_n_params(8, 16, 1) > 0)
GRAPH = dict(n_nodes=64, feat_dim=8, feat_stride=8, n_rel=1, n_pos=8, max_degree=1, X=P(0), train_pos=P(1), indptr0=P(2), indices0=P(3))
STATE = dict(theta=P(20), m=P(21), v=P(22), step_counter=P(23), sync_words=P(24), clf_next=P(25), slabs=P(26), acts=None,
             wg_scratch=None, emb=16, act_ld=0, lambda_1=2.0)
BATCH = dict(ids=P(30), labels=P(31), cnt=P(32), plan=None, B=4, inv_count=0.25)
SEL = dict(thresholds=THR, rho=RHO, workspace=P(40), status=P(41), list_capacity=1024, add_self=0)
OUT = dict(logits=P(50), center=P(51), combined=None, row_loss=P(52))

_SELECT = dict(g="g", nodes=P(4), labels=P(5), B=4, s0=P(6), center_s0=None, pos_keys=P(7), thresholds=THR, rho=RHO, train_flag=1,
               add_self=0, cnt=P(8), workspace=P(9), list_capacity=1024, status=P(10), stream=None)
_GATHER = dict(X=P(0), feat_dim=8, feat_stride=8, table_rows=64, n_rows=4, cnt=P(8), g="g", B=4, workspace=P(9), list_capacity=1024,
               agg=P(11), agg_stride=8, status=P(10), stream=None)


def _ins(d, after, **new):
    """d with the items of `new` inserted behind key `after` (argument order is the dict's order)"""
    out = {}
    for k, v in d.items():
        out[k] = v
        if k == after:
            out.update(new)
    return out


# entry point -> its arguments in order, for a call that would pass ("g", "st", "sta" - a state that holds activations -, "batch", "next", "clf", "sel", "out": the structs below)
CALLS = {
    "pcg_choose_select": _SELECT,
    "pcg_choose_select_planned": _ins(_ins(_SELECT, "workspace", plan=None), "status", sync_words=P(12), center_id_offset=0),
    "pcg_choose_aggregate": _ins(_ins(_SELECT, "train_flag", norm=0), "add_self", agg=P(11), agg_stride=8),
    "pcg_choose_aggregate_planned": _ins(_ins(_SELECT, "train_flag", norm=0), "add_self", agg=P(11), agg_stride=8),
    "pcg_choose_gather_planned": _ins(_ins(_ins(_SELECT, "add_self", agg=P(11), agg_stride=8), "workspace", plan=None), "status",
                                      sync_words=P(12)),
    "pcg_plan_batches": dict(g="g", nodes=P(4), labels=P(5), n_total=8, B=4, thresholds=THR, rho=RHO, train_flag=1, add_self=0,
                             plans=P(9), plan_stride=1 << 20, list_capacity=1024, status=P(10), bump_counter=None, stream=None),
    "pcg_plan_epochs": dict(g="g", nodes=P(4), labels=P(5), n_total=8, n_epochs=2, B=4, thresholds=THR, rho=RHO, train_flag=1,
                            add_self=0, plans=P(9), plan_stride=1 << 20, list_capacity=1024, status=P(10), bump_counter=None,
                            stream=None),
    "pcg_step_front": dict(g="g", W=P(13), b=P(14), s0=P(6), pos_keys=P(7), nodes=P(4), labels=P(5), B=4, thresholds=THR, rho=RHO,
                           train_flag=1, add_self=0, workspace=P(9), list_capacity=1024, status=P(10), stream=None),
    "pcg_step_front_a": dict(g="g", W=P(13), b=P(14), row_begin=0, row_end=64, s0_out=P(6), row_ids=None, pos_keys=P(7), nodes=P(4),
                             labels=P(5), B=4, thresholds=THR, rho=RHO, train_flag=1, add_self=0, workspace=P(9), list_capacity=1024,
                             status=P(10), stream=None),
    "pcg_step_front_b": dict(g="g", s0=P(6), pos_keys=P(7), raw_keys_ready=1, nodes=P(4), labels=P(5), B=4, thresholds=THR, rho=RHO,
                             train_flag=1, add_self=0, workspace=P(9), list_capacity=1024, status=P(10), center_s0_out=None,
                             center_id_offset=0, stream=None),
    "pcg_step_scores": dict(g="g", W=P(13), b=P(14), row_begin=0, row_end=64, s0_out=P(6), row_ids=None, pos_keys=P(7),
                            pos_row_base=-1, sync_words=P(12), touched=None, stream=None),
    "pcg_aggregate_lists": _ins(_GATHER, "list_capacity", norm=0),
    "pcg_gather_lists": _GATHER,
    "pcg_gather_lists_planned": _ins(_GATHER, "workspace", plan=None),
    "pcg_aggregate_lists_planned": _ins(_ins(_GATHER, "workspace", plan=None), "list_capacity", norm=0),
    "pcg_gather_lists_dist": _ins(_ins(_GATHER, "workspace", plan=None), "status", lo=0, hi=32, n_local=32, pos_ids=P(15), pos_idx=P(16),
                                  n_pos=4, table=P(17), table_slots=1024, counts=P(18), halo_cap=16, halo_base=40, theta=P(20),
                                  m=P(21), v=P(22), clf_offset=0, clf_n=18, snap_dst=P(19)),
    "pcg_step_front_train": dict(g="g", st="st", s0=P(6), pos_keys=P(7), batch="batch", sel="sel", stream=None),
    "pcg_step_scores_train": dict(g="g", st="st", s0=P(6), pos_keys=P(7), touched=None, stream=None),
    "pcg_step_scores_dist": dict(g="g", st="st", grad=P(27), clf_snap=P(28), row_begin=0, row_end=64, s0_out=P(6), row_ids=None,
                                 pos_keys=P(7), pos_row_base=40, stream=None),
    "pcg_choose_gather_train": dict(g="g", batch="batch", s0=P(6), pos_keys=P(7), sel="sel", agg=P(11), agg_stride=8, st="st",
                                    score_next=1, next_touched=None, keys_sorted=0, stream=None),
    "pcg_choose_train_part": dict(part=1, g="g", batch="batch", s0=P(6), pos_keys=P(7), sel="sel", agg=P(11), agg_stride=8, st="st",
                                  score_next=1, next_touched=None, keys_sorted=0, clf_out=None, stream=None),
    "pcg_dense_select_train": dict(g="g", st="sta", sel="sel", batch="batch", next="next", agg=P(11), agg_stride=8, clf_in=P(33), out="out",
                                   clf_out=P(34), s0=P(6), pos_keys=P(7), stream=None),
    "pcg_dense_select_ahead": dict(g="g", st="sta", sel="sel", batch="batch", next="next", clf_batch="clf", agg=P(11), agg_stride=8,
                                   clf_in=P(33), out="out", clf_out=P(34), s0=P(6), pos_keys=P(7), sort_keys=P(35), stream=None),
    "pcg_clf_step": dict(g="g", batch="batch", st="st", clf_out=None, t_ahead=1, stream=None),
}
_STRUCTS = {"g": GRAPH, "st": STATE, "sta": dict(STATE, acts=P(36), act_ld=16, wg_scratch=P(42)), "batch": BATCH, "next": BATCH, "clf": BATCH, "sel": SEL, "out": OUT}
PLAN_BYTES = "one 256-byte step below pcg_choose_plan_bytes(g, B, list_capacity)"

# what every selection call refuses in choose_args, as (override, code); `planned`-only and front-only rows are listed per entry point
_SELECT_ROWS = [
    ({"g": None}, ARG), ({"nodes": None}, ARG), ({"s0": None}, ARG), ({"thresholds": None}, ARG), ({"cnt": None}, ARG),
    ({"workspace": None}, ARG), ({"status": None}, ARG), ({"B": -1}, ARG), ({"B": 0}, OK), ({"list_capacity": 0}, ARG),
    ({"list_capacity": 1 << 31}, ARG), ({"g.n_rel": 0}, ARG), ({"g.n_rel": 9}, ARG), ({"rho": None}, ARG), ({"labels": None}, ARG),
    ({"pos_keys": None}, ARG), ({"g.train_pos": None}, ARG), ({"g.indptr0": None}, ARG), ({"g.indices0": None}, ARG),
    ({"B": 0, "cnt": None, "nodes": None}, OK),               # precedence: the empty batch returns before the pointer checks
    ({"B": -1, "g.feat_stride": 516}, ARG),
]
_AGG_ROWS = [({"g.X": None}, ARG), ({"agg": None}, ARG), ({"B": 0, "agg": None}, OK), ({"agg": None, "list_capacity": 0}, ARG)]
_PLAN_ROWS = [
    ({"g": None}, ARG), ({"nodes": None}, ARG), ({"thresholds": None}, ARG), ({"plans": None}, ARG), ({"status": None}, ARG),
    ({"n_total": -1}, ARG), ({"n_total": 0}, OK), ({"B": 0}, ARG), ({"B": -1}, ARG), ({"plan_stride": -256}, ARG),
    ({"plan_stride": 100}, ARG), ({"plan_stride": PLAN_BYTES}, ARG), ({"plan_stride": 0}, ARG), ({"list_capacity": 0}, ARG),
    ({"list_capacity": 1 << 31}, ARG), ({"g.n_rel": 0}, ARG), ({"g.n_rel": 9}, ARG), ({"rho": None}, ARG), ({"labels": None}, ARG),
    ({"g.indptr0": None}, ARG), ({"n_total": 0, "nodes": None, "status": None}, OK), ({"n_total": 1 << 30, "B": 1}, ARG),
]
# the score / key front: what pcg_step_front, pcg_step_front_a and pcg_step_scores share
_TABLE_FRONT_ROWS = [
    ({"g": None}, ARG), ({"g.X": None}, ARG), ({"W": None}, ARG), ({"b": None}, ARG), ({"g.X": P(0) + 4}, ARG),
    ({"g.feat_stride": 6, "g.feat_dim": 6}, ARG), ({"g.feat_stride": 8, "g.feat_dim": 9}, ARG), ({"g.feat_dim": 0}, ARG),
    ({"g.feat_stride": 516}, UNS), ({"g.feat_stride": 516, "g.feat_dim": 516}, UNS),
    ({"g.feat_stride": 516, "g.X": P(0) + 4}, ARG),            # precedence: alignment outranks the width here
    ({"g.feat_stride": 516, "W": None}, ARG),
]
_TABLE_STATE_ROWS = [(o, c) for o, c in _TABLE_FRONT_ROWS if not {"g", "W", "b"} & set(o)]     # (the classifier comes from the state)
_RANGE_ROWS = [
    ({"row_begin": -1}, ARG), ({"row_end": 65}, ARG), ({"row_begin": 9, "row_end": 8}, ARG), ({"s0_out": None}, ARG),
    ({"g.feat_stride": 516, "row_end": 65}, ARG),              # precedence: the row range outranks the width
]
_FRONT_PLAN_ROWS = [
    ({"nodes": None}, ARG), ({"thresholds": None}, ARG), ({"workspace": None}, ARG), ({"status": None}, ARG), ({"B": -1}, ARG),
    ({"list_capacity": 0}, ARG), ({"list_capacity": 1 << 31}, ARG), ({"g.n_rel": 0}, ARG), ({"g.n_rel": 9}, ARG), ({"rho": None}, ARG),
    ({"labels": None}, ARG), ({"g.indptr0": None}, ARG),
    ({"g.feat_stride": 516, "nodes": None}, UNS),              # precedence: the width outranks the plan's own arguments
    ({"g.feat_stride": 516, "list_capacity": 0}, UNS),
]
_GATHER_ROWS = [
    ({"X": None}, ARG), ({"cnt": None}, ARG), ({"g": None}, ARG), ({"workspace": None}, ARG), ({"agg": None}, ARG), ({"B": -1}, ARG),
    ({"n_rows": -1}, ARG), ({"B": 0, "n_rows": 0}, OK), ({"n_rows": 5}, ARG), ({"g.n_rel": 0}, ARG), ({"g.n_rel": 9}, ARG),
    ({"g.n_rel": 0, "n_rows": 0}, OK), ({"table_rows": 0}, ARG), ({"X": P(0) + 4}, ARG), ({"feat_stride": 6, "feat_dim": 6}, ARG),
    ({"feat_dim": 9}, ARG), ({"feat_stride": 516}, UNS), ({"feat_stride": 516, "feat_dim": 516, "agg_stride": 516}, UNS),
    ({"agg_stride": 7}, ARG),
    # precedence
    ({"feat_stride": 516, "agg": None}, ARG), ({"feat_stride": 516, "n_rows": 5}, ARG), ({"feat_stride": 516, "agg_stride": 7}, ARG),
    ({"feat_stride": 516, "X": P(0) + 4}, UNS),                # the width outranks the alignment here
    ({"feat_stride": 516, "B": 0, "n_rows": 0}, OK), ({"feat_stride": 6, "feat_dim": 6, "B": 0, "n_rows": 0}, OK),
    ({"feat_stride": 516, "feat_dim": 520}, ARG), ({"feat_stride": 516, "table_rows": 0}, ARG),
]
_STATE_NULLS = [({"st." + k: None}, ARG) for k in ("theta", "m", "v", "slabs", "step_counter", "sync_words")]
_TRAIN_ROWS = _STATE_NULLS + [
    ({"g": None}, ARG), ({"batch": None}, ARG), ({"sel": None}, ARG), ({"st": None}, ARG), ({"batch.B": -1}, ARG), ({"batch.B": 0}, OK),
    ({"batch.B": 0, "st.theta": None, "agg": None}, OK), ({"g.X": None}, ARG), ({"agg": None}, ARG), ({"s0": None}, ARG),
    ({"st.clf_next": None}, ARG), ({"batch.labels": None}, ARG), ({"batch.ids": None}, ARG), ({"batch.cnt": None}, ARG),
    ({"sel.thresholds": None}, ARG), ({"sel.rho": None}, ARG), ({"sel.workspace": None}, ARG), ({"sel.status": None}, ARG),
    ({"sel.list_capacity": 0}, ARG), ({"sel.list_capacity": 1 << 31}, ARG), ({"g.n_rel": 0}, ARG), ({"g.n_rel": 9}, ARG),
    ({"pos_keys": None}, ARG), ({"g.train_pos": None}, ARG), ({"g.indptr0": None}, ARG), ({"st.emb": 0}, ARG),
    ({"st.acts": P(36), "st.act_ld": 8}, ARG), ({"st.acts": P(36), "st.act_ld": 24}, ARG), ({"st.acts": P(36) + 4, "st.act_ld": 16}, ARG),
    ({"st.acts": P(36), "st.act_ld": 16, "st.emb": 24}, ARG), ({"g.feat_stride": 516}, UNS),
    # precedence
    ({"g.feat_stride": 516, "agg": None}, ARG), ({"g.feat_stride": 516, "sel.list_capacity": 0}, UNS),
    ({"g.feat_stride": 516, "st.emb": 0}, UNS), ({"g.feat_stride": 516, "batch.cnt": None}, UNS),
]
_DENSE_SELECT_ROWS = [
    ({"g": None}, ARG), ({"st": None}, ARG), ({"sel": None}, ARG), ({"batch": None}, ARG), ({"next": None}, ARG), ({"out": None}, ARG),
    ({"batch.B": 0}, ARG), ({"next.B": 0}, ARG), ({"clf_in": None}, ARG), ({"sta.acts": None}, ARG), ({"batch.cnt": None}, ARG),
    ({"next.cnt": None}, ARG), ({"sel.workspace": None}, ARG), ({"sta.sync_words": None}, ARG), ({"sta.step_counter": None}, ARG),
    ({"clf_out": None}, ARG), ({"sel.list_capacity": 0}, ARG), ({"sel.list_capacity": 1 << 31}, ARG),
    ({"sel.list_capacity": 0, "g.feat_stride": 516}, ARG),
]

ROWS = (
    [("pcg_choose_select", o, c) for o, c in _SELECT_ROWS]
    + [("pcg_choose_select_planned", o, c) for o, c in _SELECT_ROWS]
    + [("pcg_choose_select_planned", o, c) for o, c in [
        ({"center_id_offset": -1}, ARG), ({"center_id_offset": 5, "center_s0": P(6)}, ARG), ({"center_id_offset": -1, "B": 0}, ARG),
        ({"center_id_offset": -1, "g": None}, ARG), ({"plan": P(37), "workspace": None}, ARG), ({"sync_words": None, "cnt": None}, ARG)]]
    + [(n, o, c) for n in ("pcg_choose_aggregate", "pcg_choose_aggregate_planned", "pcg_choose_gather_planned")
       for o, c in _SELECT_ROWS + _AGG_ROWS]
    + [("pcg_choose_gather_planned", {"plan": P(37), "workspace": None}, ARG)]
    + [("pcg_plan_batches", o, c) for o, c in _PLAN_ROWS]
    + [("pcg_plan_epochs", o, c) for o, c in _PLAN_ROWS + [({"n_epochs": 0}, ARG), ({"n_epochs": 1 << 20, "n_total": 8}, ARG)]]
    + [("pcg_step_front", o, c) for o, c in _TABLE_FRONT_ROWS + _FRONT_PLAN_ROWS + [({"s0": None}, ARG)]]
    + [("pcg_step_front_a", o, c) for o, c in _TABLE_FRONT_ROWS + _RANGE_ROWS + _FRONT_PLAN_ROWS + [
        ({"row_ids": P(38)}, ARG), ({"row_ids": P(38), "pos_keys": None, "B": 0}, ARG),
        ({"row_ids": P(38), "g.feat_stride": 516}, ARG), ({"row_ids": P(38), "pos_keys": None, "B": 0, "g.feat_stride": 516}, UNS)]]
    + [("pcg_step_front_b", o, c) for o, c in [
        ({"g": None}, ARG), ({"s0": None}, ARG), ({"B": -1}, ARG), ({"B": 0, "train_flag": 0}, OK), ({"pos_keys": None}, ARG),
        ({"g.train_pos": None}, ARG), ({"center_s0_out": P(39), "center_id_offset": -1}, ARG), ({"nodes": None}, ARG),
        ({"labels": None}, ARG), ({"thresholds": None}, ARG), ({"rho": None}, ARG), ({"workspace": None}, ARG), ({"status": None}, ARG),
        ({"list_capacity": 0}, ARG), ({"list_capacity": 1 << 31}, ARG), ({"g.n_rel": 0}, ARG), ({"g.n_rel": 9}, ARG),
        ({"g.indices0": None}, ARG), ({"B": 0, "train_flag": 0, "nodes": None, "list_capacity": 0}, OK)]]
    + [("pcg_step_scores", o, c) for o, c in _TABLE_FRONT_ROWS + _RANGE_ROWS + [
        ({"sync_words": None}, ARG), ({"row_ids": P(38), "pos_row_base": -1}, ARG), ({"pos_row_base": 60}, ARG),
        ({"touched": P(39), "row_begin": 8}, ARG), ({"touched": P(39), "row_ids": P(38), "pos_row_base": 40}, ARG),
        ({"g.feat_stride": 516, "touched": P(39), "row_begin": 8}, ARG), ({"g.feat_stride": 516, "sync_words": None}, ARG),
        ({"g.feat_stride": 516, "row_ids": P(38), "pos_row_base": -1}, ARG)]]
    + [(n, o, c) for n in ("pcg_aggregate_lists", "pcg_gather_lists", "pcg_gather_lists_planned", "pcg_aggregate_lists_planned",
                           "pcg_gather_lists_dist") for o, c in _GATHER_ROWS]
    + [("pcg_gather_lists_dist", o, c) for o, c in [
        ({"table": None}, ARG), ({"counts": None}, ARG), ({"table_slots": 512}, ARG), ({"table_slots": 1536}, ARG), ({"lo": 33}, ARG),
        ({"n_pos": -1}, ARG), ({"pos_ids": None}, ARG), ({"pos_idx": None}, ARG), ({"theta": None}, ARG), ({"m": None}, ARG),
        ({"v": None}, ARG), ({"clf_n": 0}, ARG), ({"clf_offset": -1}, ARG), ({"feat_stride": 516, "table": None}, UNS),
        ({"feat_stride": 516, "clf_n": 0}, UNS), ({"table": None, "B": 0, "n_rows": 0}, OK)]]
    + [("pcg_step_front_train", o, c) for o, c in _STATE_NULLS + _TABLE_STATE_ROWS + [
        ({"g": None}, ARG), ({"st": None}, ARG), ({"batch": None}, ARG), ({"sel": None}, ARG), ({"batch.B": 0}, ARG), ({"st.emb": 0}, ARG),
        ({"s0": None}, ARG), ({"batch.ids": None}, ARG), ({"batch.labels": None}, ARG), ({"sel.workspace": None}, ARG),
        ({"sel.list_capacity": 0}, ARG), ({"g.feat_stride": 516, "st.theta": None}, ARG), ({"g.feat_stride": 516, "st.emb": 0}, ARG),
        ({"g.feat_stride": 516, "batch.ids": None}, UNS)]]
    + [("pcg_step_scores_train", o, c) for o, c in _STATE_NULLS + _TABLE_STATE_ROWS + [
        ({"g": None}, ARG), ({"st": None}, ARG), ({"pos_keys": None}, ARG), ({"g.train_pos": None}, ARG), ({"st.emb": 0}, ARG),
        ({"s0": None}, ARG), ({"touched": P(39), "g.feat_stride": 516}, UNS), ({"g.feat_stride": 516, "pos_keys": None}, ARG)]]
    + [("pcg_step_scores_dist", o, c) for o, c in [
        ({"g": None}, ARG), ({"st": None}, ARG), ({"g.X": None}, ARG), ({"st.theta": None}, ARG), ({"st.m": None}, ARG), ({"st.v": None}, ARG),
        ({"grad": None}, ARG), ({"clf_snap": None}, ARG), ({"s0_out": None}, ARG), ({"st.step_counter": None}, ARG),
        ({"st.sync_words": None}, ARG), ({"g.feat_dim": 0}, ARG), ({"g.feat_stride": 6, "g.feat_dim": 6}, ARG), ({"g.feat_dim": 9}, ARG),
        ({"g.X": P(0) + 4}, ARG), ({"row_begin": -1}, ARG), ({"row_end": 65}, ARG), ({"pos_row_base": -1}, ARG), ({"pos_row_base": 60}, ARG),
        ({"g.n_pos": 16385, "g.n_nodes": 1 << 20}, ARG), ({"g.feat_stride": 516}, UNS), ({"g.feat_stride": 516, "g.feat_dim": 516}, ARG),
        ({"g.feat_stride": 516, "row_end": 65}, ARG), ({"g.feat_stride": 516, "g.X": P(0) + 4}, ARG),
        ({"g.feat_stride": 516, "pos_row_base": 60}, ARG), ({"g.feat_stride": 516, "st.emb": 0}, UNS), ({"st.emb": 0}, ARG)]]
    + [("pcg_choose_gather_train", o, c) for o, c in _TRAIN_ROWS]
    + [("pcg_choose_train_part", o, c) for o, c in _TRAIN_ROWS + [
        ({"part": 0}, ARG), ({"part": 3}, ARG), ({"part": 0, "batch.B": 0}, ARG), ({"part": 2, "agg": None}, ARG),
        ({"part": 2, "g.feat_stride": 516}, UNS)]]
    + [("pcg_dense_select_train", o, c) for o, c in _DENSE_SELECT_ROWS]
    + [("pcg_dense_select_ahead", o, c) for o, c in _DENSE_SELECT_ROWS + [
        ({"sort_keys": P(7)}, ARG), ({"clf_batch": None}, ARG), ({"clf.labels": None}, ARG), ({"clf.B": 0}, ARG),
        ({"sort_keys": P(7), "g": None}, ARG)]]
    + [("pcg_clf_step", o, c) for o, c in _STATE_NULLS + [
        ({"g": None}, ARG), ({"batch": None}, ARG), ({"st": None}, ARG), ({"g.X": None}, ARG), ({"batch.ids": None}, ARG),
        ({"batch.labels": None}, ARG), ({"batch.B": 0}, ARG), ({"st.clf_next": None}, ARG), ({"t_ahead": 0}, ARG), ({"st.emb": 0}, ARG)]]
)


def _graph(f):
    g = _lib.GraphDesc()
    for k, v in f.items():
        if k == "indptr0":
            g.indptr[0] = v
        elif k == "indices0":
            g.indices[0] = v
        else:
            setattr(g, k, v)
    return g


_MAKE = {"g": _graph, "st": lambda f: _lib.TrainState(hyper=HYPER, **f), "sta": lambda f: _lib.TrainState(hyper=HYPER, **f), "batch": lambda f: _lib.Batch(**f),
         "next": lambda f: _lib.Batch(**f), "clf": lambda f: _lib.Batch(**f), "sel": lambda f: _lib.SelectWs(**f),
         "out": lambda f: _lib.DenseOut(**f)}


def _call(lib, name, over):
    args = dict(CALLS[name])
    fields = {k: dict(_STRUCTS[k]) for k in _STRUCTS}
    for key, val in over.items():
        if "." in key:
            s, f = key.split(".")
            assert s in args.values() and f in fields[s], key
            fields[s][f] = val
        else:
            assert key in args, (name, key)
            args[key] = val
    keep = {k: _MAKE[k](fields[k]) for k in _STRUCTS}          # (alive for the call)
    if args.get("plan_stride") == PLAN_BYTES:
        args["plan_stride"] = int(lib.pcg_choose_plan_bytes(C.byref(keep["g"]), args["B"], args["list_capacity"])) - 256
        assert args["plan_stride"] > 0 and args["plan_stride"] % 256 == 0
    argv = [C.byref(keep[v]) if isinstance(v, str) and v in keep else v for v in args.values()]
    assert len(argv) == len(_lib.PROTOTYPES[name][1]), name
    return getattr(lib, name)(*argv)


def _id(row):
    name, over, _ = row
    return name[4:] + "[" + ",".join(f"{k}={'NULL' if v is None else v if not isinstance(v, int) or abs(v) < 4096 else hex(v - _BASE) if v >= _BASE else hex(v)}" for k, v in over.items()) + "]"


def test_the_table_covers_every_entry_point_and_never_expects_a_launch():
    names = {r[0] for r in ROWS}
    assert names == set(CALLS)
    for must in ("pcg_choose_select", "pcg_choose_select_planned", "pcg_choose_aggregate", "pcg_choose_aggregate_planned",
                 "pcg_choose_gather_planned", "pcg_plan_batches", "pcg_plan_epochs", "pcg_step_front", "pcg_step_front_a",
                 "pcg_step_front_b", "pcg_step_scores", "pcg_aggregate_lists", "pcg_gather_lists", "pcg_gather_lists_planned",
                 "pcg_aggregate_lists_planned", "pcg_gather_lists_dist"):
        assert must in names
    assert all(code in (OK, ARG, UNS) for _, _, code in ROWS)
    assert (OK, ARG, UNS) == (_lib.PCG_OK, _lib.PCG_E_ARG, _lib.PCG_E_UNSUPPORTED) and _lib.PCG_E_LAUNCH not in (OK, ARG, UNS)
    assert len({_id(r) for r in ROWS}) == len(ROWS)            # (no row twice)
    # two checks failing at once: rows that change more than one thing and are still refused
    both = [r for r in ROWS if len(r[1]) >= 2 and 516 in (r[1].get("g.feat_stride"), r[1].get("feat_stride"))]
    assert len({r[0] for r in both}) >= 6 and {r[2] for r in both} == {OK, ARG, UNS}


def test_every_row_answers_its_code():
    lib = _lib.load()
    wrong = []
    for row in ROWS:
        got = _call(lib, row[0], row[1])
        if got != row[2]:
            wrong.append((_id(row), "expected", row[2], "got", got))
    assert not wrong, wrong
