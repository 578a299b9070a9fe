/*
 * pcgnn.h - C ABI of libpcgnn_hip.so: the MI355X (gfx950) PC-GNN hot path.
 *
 * The reference (h22hyeon/PC-GNN) is 100 % Python and has no FFI of its own; its
 * "plugin API" for this path is the forward() of PCALayer / InterAgg* / IntraAgg
 * and pick_step().  This header is what a ctypes binding inside those methods
 * calls instead of the Python set / torch.sort / dense-mask code.  Each entry
 * point names the reference lines it replaces (paths relative to the
 * reference root).  INTEGRATION.md shows the reference-side ctypes stub.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. a torch tensor
 *     that outlives the call) unless the parameter is documented "host";
 *   - work is enqueued on `stream` (a hipStream_t passed as void*); no entry point
 *     synchronises the stream, allocates, or frees device memory;
 *   - return value: 0 = enqueued, <0 = rejected before anything was enqueued
 *     (PCG_E_*).  Conditions only knowable on the device (a selection buffer
 *     too small) are reported through the caller-provided `status` word;
 *   - one host thread per device; re-entrant across devices.
 *
 * Data layout in HBM (built once per graph, resident for the whole run - mirrors
 * the frozen nn.Embedding + adj_lists the reference keeps, model_handler.py:85-87):
 *   X          float  [n_nodes, feat_stride]  row-major, feat_stride % 4 == 0,
 *                     columns feat_dim..feat_stride-1 are zero, 16-byte aligned.
 *                     feat_stride <= 512: every entry point that scores the table (pcg_score_table, pcg_step_front*,
 *                     pcg_step_scores*, the inference and explanation calls), gathers lists from it or takes a segment
 *                     mean returns PCG_E_UNSUPPORTED for a wider one; only pcg_score_rows and pcg_gather_rows take any width
 *   indptr[r]  int64  [n_nodes + 1]           CSR row offsets of relation r
 *   indices[r] int32  [nnz_r]                 neighbour ids, ASCENDING inside a row,
 *                                             self-loops kept (utils.py:226-239)
 *   train_pos  int32  [n_pos]                 ids of training positives, no duplicates
 */
#ifndef PCGNN_H
#define PCGNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCG_MAX_REL 8

enum {
    PCG_OK = 0,
    PCG_E_ARG = -1,        /* null / misaligned pointer, bad size                   */
    PCG_E_UNSUPPORTED = -2,/* shape outside what the kernels handle                 */
    PCG_E_LAUNCH = -3      /* hipLaunchKernel reported an error                     */
};

/* bits of the device-side status word */
enum {
    PCG_ST_SEL_OVERFLOW = 1,  /* sel_indices capacity too small; nothing was written past it */
    PCG_ST_LIST_ID_RANGE = 2, /* a selection-list entry named no row of the table handed to the gather; it was skipped (a hole) */
    PCG_ST_SYNC_TIMEOUT = 4,  /* a bounded in-kernel wait (the select kernel's wait for its own train-pos sort) ran out */
    PCG_ST_SORT_OVERFLOW = 8, /* the one-launch bucket sort of the train positives met a bucket of more than 4096 keys (eight times
                                 the mean): its surplus keys were dropped - minority picks of that step may be wrong */
    PCG_ST_EVAL_INPUT = 16,   /* pcg_eval_counts met a label outside {0, 1} or a NaN probability: its counts describe no valid input */
    PCG_ST_RANK_MISMATCH = 32,/* pcg_rank_lists / pcg_chosen_set: a row's kept count on the device is not the extent the caller's
                                 out_begin gives it (or its list region / extent leaves its array); nothing was written for that row.
                                 pcg_rank_minority: a row's extent is negative, above n_pos or leaves its array; not written */
    PCG_ST_PR_OVERFLOW = 64   /* pcg_pr_counts: more precision-recall points than `cap`; nothing was written past it */
};

enum { PCG_NORM_COUNT = 0, PCG_NORM_SQRT_COUNT = 1 };

typedef struct pcg_graph_desc {
    int64_t n_nodes;
    int32_t feat_dim;
    int32_t feat_stride;
    int32_t n_rel;
    int32_t n_pos;
    int32_t max_degree;                 /* max over relations and rows (host-computed) */
    int32_t _pad;
    const float *X;
    const int32_t *train_pos;
    const int64_t *indptr[PCG_MAX_REL];
    const int32_t *indices[PCG_MAX_REL];
} pcg_graph_desc;

/* library / build identification: "pcgnn_hip gfx950 <abi>" (host pointer, static) */
const char *pcg_version(void);
int pcg_abi_version(void);   /* 13 (added: pcg_explain_out, pcg_explain_new, pcg_explain_new_workspace_bytes; 12: the training entry
                                points take parameter structs, pcg_abi_layout) */

/* ---- parameter structs of the training entry points ------------------------------------------
 * What a training engine owns is handed over as structs, by const pointer: an entry point reads them during the call and keeps
 * no pointer to them (a temporary will do; a captured graph holds the values, not the struct).  A NULL struct pointer is
 * PCG_E_ARG before anything else happens.  Pointers and scalars only; a member an entry point does not name is not read by it.
 * A member that may be NULL means "off" exactly where the entry point says so - a caller that wants it on in one call and off
 * in another keeps two instances.  pcg_abi_layout reports every struct's size and member offsets (a binding's layout check). */

/* torch.optim.Adam's hyper-parameters (coupled weight decay, src/model_handler.py:124); converted to float once, on entry */
typedef struct pcg_adam_hyper {
    double lr, beta1, beta2, eps, weight_decay;
} pcg_adam_hyper;

/* What a training engine allocates once (again when the batch size it was made for grows). */
typedef struct pcg_train_state {
    float *theta, *m, *v;        /* the flat parameter buffer (pcg_dense_param_offset) and Adam's moments, n_params floats each */
    int32_t *step_counter;       /* int32 [1]: Adam's t, counted on the device */
    uint32_t *sync_words;        /* pcg_sync_words_count() words, zero-initialised ONCE by the caller; the launches keep them from
                                    then on: [0] arrival ticket (0 between launches), [1] "an update is waiting" - the pending
                                    word - (1: gradient slabs, 2: activations; 0 once it has been applied), [2] its slab / tile
                                    count, [3] and the words behind it: pcg_choose_gather_planned's in-kernel sort (every launch
                                    leaves them zero) */
    float *clf_next;             /* [2 * feat_dim + 2] (W row-major, then b): the label classifier one step ahead of theta's copy -
                                    the one the next select launch scores by (pcg_choose_gather_train) */
    float *slabs;                /* [max(pcg_dense_n_tiles(B), 8), n_params]: per-tile gradient slabs, and the classifier step's
                                    scratch; no initial contents required (a launch writes the slabs it or its successor reads).
                                    NULL in pcg_train_dense: inference (no gradient, no step counted) */
    float *acts;                 /* [pcg_wgrad_act_rows(...), act_ld], 16-byte aligned: the transposed activations of
                                    pcg_train_dense(adam_clf = 3 / 4) that the weight-gradient GEMMs read; no initial contents
                                    required (a dense launch writes every column of its batch's tiles, the columns beyond the
                                    batch as zeros, and the GEMMs read those tiles only).  NULL: the gradient-slab paths */
    float *wg_scratch;           /* pcg_wgrad_scratch_bytes(...) bytes, zero-initialised ONCE by the caller; every launch leaves
                                    them so (the tiles' arrival counters); may be NULL for act_ld <= 1024 */
    int32_t emb;                 /* embedding width E */
    int32_t act_ld;              /* floats per row of acts: the largest batch rounded up to 16 */
    float lambda_1;              /* weight of the label classifier's loss term (src/model.py:54-61) */
    int32_t _pad;
    pcg_adam_hyper hyper;
} pcg_train_state;

/* The selection settings and the workspace every training call of an engine shares (the arguments of pcg_choose_select). */
typedef struct pcg_select_ws {
    const double *thresholds;    /* HOST double [n_rel] */
    const double *rho;           /* HOST double [n_rel] */
    void *workspace;             /* the DATA part (pcg_choose_data_bytes; no initial contents required) when the batches carry their
                                    plan, else the single buffer (zero-initialised ONCE by the caller; every launch leaves it so) */
    uint32_t *status;            /* the device status word */
    int64_t list_capacity;
    int32_t add_self;
    int32_t _pad;
} pcg_select_ws;

/* One batch. */
typedef struct pcg_batch {
    const int32_t *ids;          /* int32 [B] centre ids (the `nodes` of the selection entry points) */
    const int32_t *labels;       /* int32 [B] */
    int32_t *cnt;                /* int32 [n_rel * B]: |chosen set|, written by the batch's select launch, read by its dense launch */
    const void *plan;            /* the batch's plan part (a slot pcg_plan_batches filled; the slots: zero-initialised ONCE by the
                                    caller; every launch leaves them so); NULL: it lies inside the workspace */
    int32_t B;
    float inv_count;             /* 1 / global batch size: the weight of a row's loss */
} pcg_batch;

/* What a dense launch writes for its batch: logits [B, 2], center [B, 2]; optional combined [B, E] (not written by the fused
 * launches pcg_dense_select_*) and row_loss [B] (see pcg_dense_step). */
typedef struct pcg_dense_out {
    float *logits, *center, *combined, *row_loss;
} pcg_dense_out;

/* What pcg_explain_new writes for its n query rows, in three groups; a group is requested by setting ALL of its pointers and left
 * out by setting none of them (some set, others NULL: PCG_E_ARG).  At least one group must be requested. */
typedef struct pcg_explain_out {
    /* the attribution group (pcg_attr_set's outputs) */
    float *logits;               /* [n][2] */
    float *d_self;               /* [n][feat_dim] */
    float *d_agg;                /* [n_rel][n][feat_dim] */
    float *self_contrib;         /* [n] */
    float *rel_contrib;          /* [n_rel][n] */
    /* the chosen group (pcg_chosen_set's outputs) */
    const int64_t *out_begin;    /* int64 [n_rel * n + 1]: an INPUT, formed on the host as for pcg_chosen_set */
    int32_t *out_ids;            /* [out_begin[n_rel * n]] */
    float *out_dist;             /* [out_begin[n_rel * n]] */
    /* every chosen neighbour's share (pcg_attr_neighbours' output): only with both groups above */
    float *neigh_contrib;        /* [out_begin[n_rel * n]] */
} pcg_explain_out;

/* Layout of struct `which` (0 pcg_adam_hyper, 1 pcg_train_state, 2 pcg_select_ws, 3 pcg_batch, 4 pcg_dense_out, 5 pcg_explain_out)
 * as this library
 * was compiled: out[0] = sizeof, out[1 ..] = offsetof of every member in declaration order (padding members included).
 * Returns the number of values written, or PCG_E_ARG (unknown struct, out NULL, cap too small).  Host only: no device call. */
int32_t pcg_abi_layout(int32_t which, int64_t *out, int32_t cap);

/* ---- label-aware scores -------------------------------------------------------
 * Replaces  batch_scores = self.label_clf(self.features(unique_nodes))
 *           (src/layers.py:230-237) by scoring the whole table once per step.
 * s0[i] = b[0] + sum_f X[i,f] * W[0,f]   (class-0 logit; the only column the
 * choose step reads, layers.py:649-650).  W is label_clf.weight [2, feat_dim]
 * row-major, b is label_clf.bias [2].  Rows [row_begin, row_end). */
int pcg_score_table(const pcg_graph_desc *g, const float *W, const float *b,
                    int64_t row_begin, int64_t row_end, float *s0, void *stream);

/* center_scores = batch_scores[nodes]  (layers.py:243): both logits of the given
 * rows, bit-identical in column 0 to pcg_score_table.  out is [n_ids, 2]. */
int pcg_score_rows(const pcg_graph_desc *g, const float *W, const float *b,
                   const int32_t *ids, int32_t n_ids, float *out, void *stream);

/* Sort the training positives by class-0 logit once per step; replaces the
 * per-centre torch.sort over all of pos_scores (layers.py:683-688).
 * keys [pcg_pos_sort_capacity(n_pos)] uint64; on return its first ceil_pow2(max(n_pos, 4096)) entries hold
 * (orderable(s0[train_pos[p]]) << 32) | p ascending, padded with UINT64_MAX; the capacity is twice that: the second
 * half is scratch (the bucket sort's scatter buffer and splitters for n_pos > 16384; the unsorted keys pcg_step_front forms beside the score pass). */
int64_t pcg_pos_sort_capacity(int32_t n_pos);
int pcg_pos_sort(const pcg_graph_desc *g, const float *s0, uint64_t *keys, void *stream);

/* ---- choose + aggregate (the hot path) ----------------------------------------------
 * Replaces, for every relation r and batch centre b:
 *   neighbour lookup + score slicing            layers.py:217-219, 246-253
 *   num_sample = ceil(deg * threshold[r])        layers.py:260-262
 *   choose_step_neighs / choose_step_test        layers.py:633-738
 *   dense-mask mean  mask.div(n).mm(X[unique])   layers.py:594-624
 * Selection rule: if deg > k+1 keep the k neighbours with the smallest
 * |s0[centre] - s0[j]|, ties by ascending position in the (ascending-id) row;
 * else keep all.  If train_flag and labels[b]==1 additionally take the
 * m = min(int(k*rho[r]), n_pos) training positives nearest in the same metric, ties
 * by position in train_pos; the union is de-duplicated (set(), layers.py:694).
 *
 * pcg_choose_select writes every row's chosen ids into the workspace's selection list
 * (row = r * B + b; region [row_begin[row], row_begin[row] + len[row]); -1 marks a slot
 * whose candidate was a duplicate) and |set| into cnt; pcg_aggregate_lists gathers and
 * averages those lists from a feature table (the graph's X, or on a multi-GPU run a
 * table extended by the rows fetched from other ranks after the list was re-indexed);
 * pcg_choose_aggregate = both, for one GPU.
 *
 *   nodes   int32 [B]   batch centre ids (duplicates allowed)
 *   labels  int32 [B]   batch labels; may be NULL when train_flag == 0
 *   s0      float [n_nodes] from pcg_score_table;  pos_keys from pcg_pos_sort
 *   center_s0 float [B] or NULL: the centres' class-0 logits if they are not to be
 *           read from s0[nodes[b]] (IntraAgg.forward called with explicit
 *           batch_scores, layers.py:562)
 *   thresholds, rho  HOST double [n_rel]
 *   add_self 1: the centre joins its own set (GCN / SAGE-gcn, graphsage.py:78-79, 214)
 *   cnt     int32 [n_rel * B]             |chosen set|
 *   agg     float [n_rel * B, agg_stride] mean of the chosen rows (cols < feat_dim);
 *           norm = PCG_NORM_COUNT | PCG_NORM_SQRT_COUNT (graphsage.py:224-226)
 *   workspace: pcg_choose_workspace_bytes(g, B, list_capacity) bytes, 256-byte aligned,
 *           zero-initialised ONCE by the caller; every launch leaves it so ("Initial contents" below);
 *           list_capacity (< 2^31 entries) bounds sum over rows of
 *           pcg_sel_capacity_row(...); if a batch needs more, nothing is selected and
 *           PCG_ST_SEL_OVERFLOW is OR-ed into *status (uint32 device word; zero it yourself).
 *   pcg_choose_workspace_offset(..., which): byte offset inside the workspace of
 *           0 row_begin int64 [rows+1] | 1 len int32 [rows] | 2 list int32 [list_capacity]
 *           (3 chunk_begin, 4 chunk descriptors, 5 counters, 6 partial: internal, exposed for tests).
 *
 * The workspace has two parts: the PLAN part (what the plan works out for one batch: row records, list / chunk offsets, tier
 * queues, the gather's chunk table - a function of the batch's ids, labels and CSR degrees only) and the DATA part (what a
 * step writes: selection list, per-chunk partial sums, key scratch).  pcg_choose_workspace_bytes = both, the plan part first
 * (the single-buffer layout every entry point without a `plan` argument uses).  pcg_choose_plan_bytes / _data_bytes: the
 * parts on their own, for callers that keep one plan part per batch of an epoch (pcg_plan_batches) and ONE data part.
 *
 * Initial contents.  The PLAN part - of the single buffer, or a slot of pcg_plan_batches / pcg_plan_epochs - is zero-initialised
 * ONCE by the caller; every launch leaves it so: the words the launches count from zero (the 768 bytes at its start: the select
 * launches' queue heads and arrival counters, the plan launch's sequence word) are put back or moved on by the launch that used
 * them, and everything else in it is written by a plan before anything reads it.  A slot stays valid for as long as the same
 * bytes are planned for the SAME B.  Before a slot of pcg_plan_batches / pcg_plan_epochs is planned for another B - another
 * layout over the same bytes, whose look-back tags would sit on whatever the old layout left there - zero it again.  The single
 * buffer of the entry points without a `plan` argument may change B from call to call without being zeroed again: their plan
 * launches publish nothing through look-back words, and the 768 bytes do not move with B.
 * The DATA part: no initial contents required - the selection list, the per-chunk partial sums and the key scratch are written
 * by the step that reads them - and one data part may serve plan slots of any B, in any order, without being zeroed in between.
 * (In the single buffer it lies behind the plan part of the call's B.) */
int64_t pcg_choose_workspace_bytes(const pcg_graph_desc *g, int32_t B, int64_t list_capacity);
int64_t pcg_choose_plan_bytes(const pcg_graph_desc *g, int32_t B, int64_t list_capacity);
int64_t pcg_choose_data_bytes(const pcg_graph_desc *g, int32_t B, int64_t list_capacity);
int64_t pcg_choose_workspace_offset(const pcg_graph_desc *g, int32_t B, int64_t list_capacity, int32_t which);
int pcg_choose_select(const pcg_graph_desc *g, const int32_t *nodes, const int32_t *labels, int32_t B,
                      const float *s0, const float *center_s0, const uint64_t *pos_keys,
                      const double *thresholds, const double *rho, int32_t train_flag, int32_t add_self,
                      int32_t *cnt, void *workspace, int64_t list_capacity, uint32_t *status, void *stream);
/* pcg_aggregate_lists: the gather + mean half on its own, over the lists (and the plan) a pcg_choose_select* call left in
 * `workspace`, reading feature rows from X [table_rows, feat_stride] - g->X, or a table with further rows behind it (the
 * partitioned path's [owned | train-pos | halo] table, whose lists pcg_halo_lookup has re-indexed).  n_rows = the rows of the
 * plan = g->n_rel * B (anything else is rejected).  A list entry outside [0, table_rows) is skipped like a hole and
 * PCG_ST_LIST_ID_RANGE is OR-ed into *status (may be NULL: then only skipped). */
int pcg_aggregate_lists(const float *X, int32_t feat_dim, int32_t feat_stride, int64_t table_rows, int32_t n_rows,
                        const int32_t *cnt, const pcg_graph_desc *g, int32_t B, void *workspace, int64_t list_capacity,
                        int32_t norm, float *agg, int32_t agg_stride, uint32_t *status, void *stream);
int pcg_choose_aggregate(const pcg_graph_desc *g, const int32_t *nodes, const int32_t *labels, int32_t B,
                         const float *s0, const float *center_s0, const uint64_t *pos_keys,
                         const double *thresholds, const double *rho, int32_t train_flag,
                         int32_t norm, int32_t add_self, float *agg, int32_t agg_stride, int32_t *cnt,
                         void *workspace, int64_t list_capacity, uint32_t *status, void *stream);

/* The front of a training step in two launches instead of four.  Equivalent to
 *   pcg_score_table(g, W, b, 0, n_nodes, s0);  pcg_pos_sort(g, s0, pos_keys)  [if train_flag and n_pos > 0];
 *   + the plan (row records, list offsets, tier queues, chunk table) that pcg_choose_select / pcg_choose_aggregate
 *     would compute first for this (nodes, labels, B, thresholds, rho, train_flag, add_self, workspace, list_capacity)
 * with the plan's two passes riding along the score pass and the sort (it needs neither's result; both leave most
 * CUs idle at dataset scale).  Follow it with pcg_choose_aggregate_planned / pcg_choose_select_planned, which take the
 * arguments of their namesakes - the same values as given here - and skip the plan.  Results are bit-identical to the
 * separate calls.  Replaces src/layers.py:230-243 (scores) + :683-688 (sort) + the per-batch bookkeeping of :246-262. */
int pcg_step_front(const pcg_graph_desc *g, const float *W, const float *b, float *s0, uint64_t *pos_keys,
                   const int32_t *nodes, const int32_t *labels, int32_t B, const double *thresholds,
                   const double *rho, int32_t train_flag, int32_t add_self, void *workspace, int64_t list_capacity,
                   uint32_t *status, void *stream);
/* The two halves of pcg_step_front on their own, for callers that need something between them (the partitioned
 * path all-gathers the scores): _a = scores of rows [row_begin, row_end) into s0_out[row] (as pcg_score_table) || plan
 * pass 1;  _b = train-pos sort by s0 || plan pass 2.  Same plan arguments in both.
 * _a with row_ids != NULL (int32 [n_nodes] on the device; pos_keys must be NULL then): row r's score goes to s0_out[row_ids[r]],
 * rows with row_ids[r] < 0 are skipped - the partitioned path, whose table rows are owned / train-pos / halo rows while scores
 * are looked up by global node id (every rank scores the rows it holds; no score all-gather).
 * _b with center_s0_out != NULL (float [B]): also center_s0_out[i] = s0[nodes[i] + center_id_offset] - the centres' own
 * scores for pcg_choose_select_planned's center_s0, when `nodes` are table rows but s0 is indexed by global id (a rank of the
 * partitioned path owns the ids [offset, offset + n_local)).
 * _a with pos_keys != NULL (training, 0 < n_pos <= 16384, every train-pos row present in g->X) also forms the unsorted keys
 * from the feature rows in the scratch half of pos_keys (a third group of workgroups); pass raw_keys_ready = 1 to _b then,
 * and its sort stages them with coalesced loads instead of gathering n_pos scores in every sort workgroup. */
int pcg_step_front_a(const pcg_graph_desc *g, const float *W, const float *b, int64_t row_begin, int64_t row_end,
                     float *s0_out, const int32_t *row_ids, uint64_t *pos_keys, const int32_t *nodes,
                     const int32_t *labels, int32_t B, const double *thresholds, const double *rho, int32_t train_flag,
                     int32_t add_self, void *workspace, int64_t list_capacity, uint32_t *status, void *stream);
int pcg_step_front_b(const pcg_graph_desc *g, const float *s0, uint64_t *pos_keys, int32_t raw_keys_ready,
                     const int32_t *nodes, const int32_t *labels, int32_t B, const double *thresholds,
                     const double *rho, int32_t train_flag, int32_t add_self, void *workspace, int64_t list_capacity,
                     uint32_t *status, float *center_s0_out, int64_t center_id_offset, void *stream);
/* `plan` (here and below): NULL = the plan part lies inside `workspace` (pcg_step_front / _a + _b made it); else `workspace`
 * is a DATA part (pcg_choose_data_bytes) and `plan` the batch's plan part (a slot pcg_plan_batches filled). */
int pcg_choose_select_planned(const pcg_graph_desc *g, const int32_t *nodes, const int32_t *labels, int32_t B,
                              const float *s0, const float *center_s0, const uint64_t *pos_keys,
                              const double *thresholds, const double *rho, int32_t train_flag, int32_t add_self,
                              int32_t *cnt, void *workspace, const void *plan, int64_t list_capacity, uint32_t *status,
                              uint32_t *sync_words, int64_t center_id_offset, void *stream);
/* (sync_words: as pcg_choose_gather_planned - the select kernel sorts the unsorted train-pos keys itself; center_id_offset > 0
 *  with center_s0 == NULL: centre b's score is s0[nodes[b] + center_id_offset] - the partitioned path, whose `nodes` are table rows
 *  of owned nodes while s0 is indexed by global node id) */
/* The plans of ALL batches of an epoch in ONE launch - off every step's critical path (a plan depends on the picked ids, their
 * labels and the CSR degrees, never on a parameter; the reference does this bookkeeping per batch, src/layers.py:217-219,
 * 246-262).  Batch s = nodes[s * B, min((s + 1) * B, n_total)) (the last one may be shorter) is planned into
 * plans + s * plan_stride (plan_stride >= pcg_choose_plan_bytes(g, B, list_capacity), a multiple of 256); thresholds .. add_self
 * and list_capacity as the *_planned calls that follow will be given.  plans: zero-initialised ONCE by the caller; every launch
 * leaves it so - for the same (n_total, B); zero the slots again before another B or epoch size is planned into them ("Initial
 * contents" above: the last, shorter batch's layout moves to another slot).  An overflowing batch sets PCG_ST_SEL_OVERFLOW and
 * selects nothing.  bump_counter (may be NULL): a device uint64 incremented by the launch (the sampler's epoch number -
 * pcg_pick_shuffled with bump = 0 in front of it). */
int pcg_plan_batches(const pcg_graph_desc *g, const int32_t *nodes, const int32_t *labels, int32_t n_total, int32_t B,
                     const double *thresholds, const double *rho, int32_t train_flag, int32_t add_self, void *plans,
                     int64_t plan_stride, int64_t list_capacity, uint32_t *status, uint64_t *bump_counter, void *stream);
/* pcg_plan_batches for n_epochs epochs at once - epoch e's n_total picks at nodes + e * n_total (labels likewise), its batches in
 * slots e * ceil(n_total / B) ..., every epoch's last batch the shorter one: the launch's latency chain (two dependent load
 * levels and a hand-off) is paid once per n_epochs epochs.  bump_counter += n_epochs. */
int pcg_plan_epochs(const pcg_graph_desc *g, const int32_t *nodes, const int32_t *labels, int32_t n_total, int32_t n_epochs, int32_t B,
                    const double *thresholds, const double *rho, int32_t train_flag, int32_t add_self, void *plans,
                    int64_t plan_stride, int64_t list_capacity, uint32_t *status, uint64_t *bump_counter, void *stream);
/* select + gather WITHOUT the combine launch (two launches): rows whose list fits one 128-entry gather chunk are finished
 * (their mean is in agg), longer rows are left as per-chunk partial sums in the workspace; pcg_train_dense, given the same
 * workspace and cnt, adds them up in chunk order (bit-identical to pcg_choose_aggregate_planned's agg) while it stages its
 * tile.  pcg_gather_lists is the gather half on its own (norm = PCG_NORM_COUNT), pcg_gather_lists_planned the same with the
 * plan part outside the workspace.
 * sync_words != NULL (the four words of pcg_train_dense / pcg_step_scores_train): pos_keys' scratch half holds the UNSORTED
 * train-pos keys of this step (pcg_step_scores_train) and - if pcg_pos_sort_in_select(n_pos) - the select kernel sorts them
 * itself, the work shared by its workgroups before they start on the rows (ranks accumulated in the words behind sync_words[3],
 * key groups counted in sync_words[3] - zero on entry; pcg_step_scores_train zeroes it); only a row with minority picks waits
 * for that count (a bounded wait: PCG_ST_SYNC_TIMEOUT if it ever ran out).  The launch also clears sync_words[1].  Results are bit-identical
 * to sorting first (pcg_pos_sort) and passing sync_words = NULL. */
int pcg_choose_gather_planned(const pcg_graph_desc *g, const int32_t *nodes, const int32_t *labels, int32_t B,
                              const float *s0, const float *center_s0, const uint64_t *pos_keys,
                              const double *thresholds, const double *rho, int32_t train_flag, int32_t add_self,
                              float *agg, int32_t agg_stride, int32_t *cnt, void *workspace, const void *plan,
                              int64_t list_capacity, uint32_t *status, uint32_t *sync_words, void *stream);
int32_t pcg_pos_sort_in_select(int32_t n_pos);      /* 1: 0 < n_pos <= 16384 (host helper) */
/* 16384 < n_pos <= 131072 train positives whose UNSORTED keys exist already (pos_keys' scratch half: pcg_choose_gather_train forms
 * them beside the score pass for these sizes too): the bucket sort in ONE launch - workgroup b sorts the same small sample, takes
 * its two splitters, streams all keys once (counting those below its range: the bucket's offset; collecting its own in LDS),
 * ranks them and stores them in place; no counts, no scatter, no hand-off between workgroups (pcg_pos_sort's four launches took
 * 35 us at 40 K keys).  A bucket of more than 4096 keys sets PCG_ST_SORT_OVERFLOW in *status (may be NULL).  src/layers.py:683-691's order. */
int32_t pcg_pos_sort_one_launch(int32_t n_pos);
int pcg_pos_sort_raw(const pcg_graph_desc *g, uint64_t *pos_keys, uint32_t *status, void *stream);
/* scores of rows [row_begin, row_end) (-> s0_out[row], or s0_out[row_ids[row]]) || the UNSORTED train-pos keys into pos_keys'
 * scratch half (pos_keys may be NULL; pos_row_base >= 0: train positive i's feature row is table row pos_row_base + i - required
 * with row_ids -, else row train_pos[i]); zeroes sync_words[3].  ONE launch, no plan, no parameter update.
 * touched (may be NULL; needs row_ids == NULL, row_begin == 0): only the rows the byte map marks (pcg_mark_touched) are scored.
 * Train positives by node id (no row_ids / pos_row_base) and more than 16384 of them: the bucket sort's launches follow and
 * pos_keys is sorted on return. */
int pcg_step_scores(const pcg_graph_desc *g, const float *W, const float *b, int64_t row_begin, int64_t row_end, float *s0_out,
                    const int32_t *row_ids, uint64_t *pos_keys, int64_t pos_row_base, uint32_t *sync_words, const uint8_t *touched,
                    void *stream);
/* select + gather of a TRAINING step with the label classifier stepped on its own: the THREE-launch step
 *       pcg_choose_gather_train (select_rows, gather_train_kernel)  ->  pcg_train_dense(adam_clf = 2).
 * The label classifier (src/layers.py:230-243; its loss term src/model.py:54-61) gets gradient from nothing but the batch
 * centres' feature rows and labels - not from the selection, the aggregates or the GNN weights.  So
 *   - ONE workgroup of the select launch does the classifier's whole step for THIS batch: logits of the centres' rows, the
 *     lambda_1 / global-batch weighted cross-entropy gradient summed over the batch in a fixed order, torch.optim.Adam's update
 *     (t = step_counter[0] + 1; m, v in place at the classifier's offset).  clf_next [2 * feat_dim + 2] (W row-major, then b):
 *     in: the classifier s0 was scored with; out: the updated one.  The in-value is copied to theta's classifier (the dense
 *     kernel computes this step's loss term with it);
 *   - the gather launch carries, in extra workgroups, the previous step's deferred Adam update of every OTHER parameter (from
 *     slabs, if sync_words[1] is set - the dense kernel that follows reads the result) and, if score_next, the NEXT step's score
 *     pass -> s0 and unsorted train-pos keys -> pos_keys' scratch half, computed with the new clf_next (next_touched != NULL:
 *     only the rows that byte map marks; n_pos > 16384: the bucket sort's launches follow).  It zeroes sync_words[3].
 * Nothing waits inside a launch for any of this.  On entry s0 / pos_keys hold THIS step's scores / unsorted keys (from the
 * previous step's call with score_next = 1, or from pcg_step_scores(W = clf_next, b = clf_next + 2 * feat_dim)).
 * pcg_adam_flush(st) afterwards brings theta up to date (deferred update + the stepped classifier).
 * batch: ids, labels, cnt, plan, B, inv_count;  sel: all of it;  st: every member (lambda_1 weighs the classifier's loss).
 * st->acts != NULL (with act_ld; `slabs` is then only the classifier step's scratch, >= 8 * n_params floats): the previous step ran
 * pcg_train_dense(adam_clf = 3) - no gradient slabs exist; the deferred update's workgroups are the weight-gradient GEMMs over
 * that step's batch, each 16 x 16 output tile's workgroup applying Adam to its own parameters (pcg_wgrad below).
 * keys_sorted != 0: pos_keys' first half holds THIS step's train-pos keys SORTED already (the previous step's
 * pcg_train_dense(adam_clf = 3, sort_keys) sorted them on CUs its tiles leave idle, or pcg_pos_sort behind pcg_step_scores): the
 * select launch sorts nothing, no row waits, and a positive hub row's minority window search runs on one of its waves beside the
 * others' key pass.  Same lists either way, bit for bit.
 * Selection, lists and aggregates: exactly pcg_choose_gather_planned(train_flag = 1). */
int pcg_choose_gather_train(const pcg_graph_desc *g, const pcg_batch *batch, float *s0, uint64_t *pos_keys,
                            const pcg_select_ws *sel, float *agg, int32_t agg_stride, const pcg_train_state *st,
                            int32_t score_next, const uint8_t *next_touched, int32_t keys_sorted, void *stream);
/* The same two launches one at a time, for the pipelined step (pcg_dense_select_train): part 1 = the select launch only (clf_out,
 * if not NULL, gets a copy of the classifier's in-value [2 * feat_dim + 2] beside theta's - the dense tiles of a fused launch
 * read it from there), part 2 = the gather launch only (+ the sort of the next step's keys where that is a launch of its own).
 * Arguments otherwise as pcg_choose_gather_train's; the weight-gradient workgroups always ride in the gather launch. */
int pcg_choose_train_part(int32_t part, const pcg_graph_desc *g, const pcg_batch *batch, float *s0, uint64_t *pos_keys,
                          const pcg_select_ws *sel, float *agg, int32_t agg_stride, const pcg_train_state *st,
                          int32_t score_next, const uint8_t *next_touched, int32_t keys_sorted, float *clf_out, void *stream);
/* The pipelined training step.  Batch t + 1's selection needs nothing batch t's dense tiles compute, so a sequence of steps
 * runs as
 *     pcg_choose_train_part(1, batch 0, clf_out = slot 0)
 *     for t:  pcg_choose_train_part(2, batch t)                   gather || Adam of t - 1 || scores + keys of t + 1
 *             pcg_dense_select_train(batch t, batch t + 1)        dense tiles of t || select of t + 1 (classifier step, key sort)
 *     last:   pcg_choose_train_part(2, last), pcg_train_dense(adam_clf = 3, last)
 * and leaves bit for bit what pcg_choose_gather_train + pcg_train_dense(adam_clf = 3) per step leave.  The fused launch: batch
 * t's tiles as pcg_train_dense(adam_clf = 3) (no key sort; the step is counted by the select half's classifier workgroup; the
 * label classifier read from clf_in = the slot batch t's select filled), batch t + 1's select as pcg_choose_train_part(1) with
 * unsorted keys (sorted inside the launch) and clf_out = the other slot.  batch->cnt / next->cnt: two different buffers.
 * batch: batch t (everything);  next: batch t + 1 (everything);  st: every member but wg_scratch (acts: written by the tiles);
 * sel: all of it;  out: logits, center, row_loss.
 * PCG_E_UNSUPPORTED where pcg_dense_select_blocks(g, emb, B) is 0. */
int pcg_dense_select_train(const pcg_graph_desc *g, const pcg_train_state *st, const pcg_select_ws *sel, const pcg_batch *batch,
                           const pcg_batch *next, const float *agg, int32_t agg_stride, const float *clf_in,
                           const pcg_dense_out *out, float *clf_out, float *s0, uint64_t *pos_keys, void *stream);
/* select workgroups of the fused launch for a dense batch of B rows (on the current device), or 0: that batch's steps keep three
 * launches (more than PCG_PIPE_MAX_TILES = 128 tiles of 16 rows by default, rows beyond the select kernel's LDS keys, feature
 * rows of more than 256 floats, a dense shape that does not fit). */
int32_t pcg_dense_select_blocks(const pcg_graph_desc *g, int32_t emb, int32_t B);
/* The pipelined step with the label classifier TWO batches ahead.  The classifier's trajectory needs nothing the gather, the
 * tiles or the weight gradients compute, so the chain classifier step -> table scores -> train-pos keys -> sort of batch t + 2
 * runs one launch earlier than in pcg_dense_select_train's sequence, and every select finds its keys sorted a launch before it
 * (no in-kernel sort, no row waits, a positive hub row's window search beside its key pass):
 *     start:  [scores + sorted keys of batch 0 at hand]  pcg_choose_train_part(1, batch 0, keys_sorted = 1, clf_out = slot 0);
 *             pcg_step_scores + pcg_pos_sort for batch 1 (the other s0 / key buffer);  pcg_clf_step(batch 1, t_ahead = 2, slot 1)
 *     for t:  pcg_choose_train_part(2, batch t, s0 / pos_keys = the buffers of batch t + 2)    gather || Adam of t - 1 || scores +
 *                                                                                               raw keys of t + 2
 *             pcg_dense_select_ahead(batch t, batch t + 1, classifier batch t + 2)
 *     last:   pcg_choose_train_part(2, last, score_next = 0), pcg_train_dense(adam_clf = 3, last, sort_keys = NULL)
 * The fused launch: batch t's tiles (clf_in = slot t % 3), batch t + 1's select as pcg_choose_train_part(1) with keys_sorted = 1
 * (s0 / pos_keys: batch t + 1's buffers), the classifier step of clf_batch (its ids, labels, B, inv_count; Adam's t = count + 3; it
 * counts the step for the tiles; clf_out = slot (t + 2) % 3), and riders that rank-sort sort_keys' raw half - formed by the
 * gather launch in front - into its sorted half (sort_keys != pos_keys; nothing in the launch reads them).  clf_batch->ids == NULL: no
 * classifier step (the end of a sequence) - the tiles count the step; sort_keys == NULL: no riders (n_pos <= 16384 with them).
 * PCG_E_UNSUPPORTED where pcg_dense_select_blocks(g, emb, B) is 0; pcg_dense_select_ahead_ok(g, emb, largest B of the sequence)
 * is the caller's test for choosing this schedule. */
int pcg_dense_select_ahead(const pcg_graph_desc *g, const pcg_train_state *st, const pcg_select_ws *sel, const pcg_batch *batch,
                           const pcg_batch *next, const pcg_batch *clf_batch, const float *agg, int32_t agg_stride,
                           const float *clf_in, const pcg_dense_out *out, float *clf_out, float *s0, uint64_t *pos_keys,
                           uint64_t *sort_keys, void *stream);
/* 1: the fused launch of a batch of B rows has room for the sort riders (a workgroup per 64 train positives, at most four per
 * tile: they start on the CUs the tiles leave) beside the tiles and pcg_dense_select_blocks' select workgroups; a graph
 * without train positives needs none.  0: the sequence keeps pcg_dense_select_train's schedule. */
int32_t pcg_dense_select_ahead_ok(const pcg_graph_desc *g, int32_t emb, int32_t B);
/* The label classifier's step for one batch as a launch of its own (select_rows' classifier workgroup alone): clf_next <- the
 * classifier after the step; theta's classifier and clf_out (if not NULL) <- the one before it; Adam's t = step_counter[0] +
 * t_ahead (>= 1); the count is left as it is.  batch: ids, labels, B, inv_count;  st: theta, m, v, step_counter, clf_next, emb,
 * lambda_1, hyper, and slabs / sync_words as pcg_choose_gather_train uses them (batches of more than 1024 rows). */
int pcg_clf_step(const pcg_graph_desc *g, const pcg_batch *batch, const pcg_train_state *st, float *clf_out, int32_t t_ahead,
                 void *stream);
int32_t pcg_sync_words_count(void);                 /* uint32 words of a `sync_words` buffer (zero-initialised ONCE by the caller; the
                                                        kernels leave every word but [1], [2] zero between launches) */
int pcg_aggregate_lists_planned(const float *X, int32_t feat_dim, int32_t feat_stride, int64_t table_rows, int32_t n_rows,
                                const int32_t *cnt, const pcg_graph_desc *g, int32_t B, void *workspace, const void *plan,
                                int64_t list_capacity, int32_t norm, float *agg, int32_t agg_stride, uint32_t *status,
                                void *stream);       /* pcg_aggregate_lists with the plan part outside the workspace */
int pcg_gather_lists_planned(const float *X, int32_t feat_dim, int32_t feat_stride, int64_t table_rows, int32_t n_rows,
                             const int32_t *cnt, const pcg_graph_desc *g, int32_t B, void *workspace, const void *plan,
                             int64_t list_capacity, float *agg, int32_t agg_stride, uint32_t *status, void *stream);
int pcg_gather_lists(const float *X, int32_t feat_dim, int32_t feat_stride, int64_t table_rows, int32_t n_rows,
                     const int32_t *cnt, const pcg_graph_desc *g, int32_t B, void *workspace, int64_t list_capacity, float *agg,
                     int32_t agg_stride, uint32_t *status, void *stream);
int pcg_choose_aggregate_planned(const pcg_graph_desc *g, const int32_t *nodes, const int32_t *labels, int32_t B,
                                 const float *s0, const float *center_s0, const uint64_t *pos_keys,
                                 const double *thresholds, const double *rho, int32_t train_flag,
                                 int32_t norm, int32_t add_self, float *agg, int32_t agg_stride, int32_t *cnt,
                                 void *workspace, int64_t list_capacity, uint32_t *status, void *stream);

/* diagnostic only: per-row phase timestamps of the select kernels ([rows][8] uint64, 10-ns ticks); NULL = off */
void pcg_debug_set_stamps(void *ptr);
void pcg_debug_set_dense_stamps(void *ptr);   /* [tiles][16] uint64 per dense_step tile */

/* Upper bound on |chosen set| of one row (host helper, pure arithmetic):
 * (deg > k+1 ? k : deg) + m [+1 if add_self]. */
int64_t pcg_sel_capacity_row(int64_t deg, double threshold, double rho, int32_t positive_train,
                             int32_t n_pos, int32_t add_self);

/* ---- segmented mean over explicit index lists -----------------------------------
 * out[i,:] = sum_{j in idx[begin[i] .. begin[i]+count[i])} X[j,:] / norm(count[i])
 * Replaces mask.div(num_neigh).mm(embed_matrix) for a given samp_neighs
 * (layers.py:599-624; graphsage.py:82-95 and, with PCG_NORM_SQRT_COUNT, 216-231). */
int pcg_segment_mean(const pcg_graph_desc *g, const int64_t *begin, const int32_t *count,
                     const int32_t *idx, int32_t n_rows, int32_t norm,
                     float *out, int32_t out_stride, void *stream);

/* ---- pick (label-balanced sampler) ------------------------------------------------
 * Replaces random.choices(idx_train, weights=deg/LF, k) (src/utils.py:274-278):
 * out[i] = idx_train[bisect_right(cum, u[i] * cum[n-1], 0, n-1)].
 * cum is the sequential fp64 running sum of the weights (host-computed once, it
 * is epoch-invariant).  uniforms: fp64 [k] in [0,1); if NULL they are drawn on
 * the device from Philox4x32-10(seed, counter = draw index). */
int pcg_pick(const double *cum, const int32_t *idx_train, int32_t n_train,
             const double *uniforms, uint64_t seed, uint64_t epoch, int32_t k, int32_t *out, void *stream);

/* One epoch's picks, shuffled, with their labels, in one launch: pick (src/utils.py:274-278) + random.shuffle
 * (src/model_handler.py:131-133) + the label lookup of the batch loop (:147).  Draw i is pcg_pick's draw i of
 * (seed, epoch); it is stored at position sigma(i), sigma a keyed pseudo-random permutation of [0, k) (an invertible
 * integer mix on the next power of two, cycle-walked into [0, k)).  epoch = epoch_base + (epoch_counter[0] if given); with
 * bump != 0 a second, one-thread launch increments epoch_counter[0] afterwards, so a captured graph replays a new epoch
 * each time.  epoch_counter points to TWO zero-initialised uint64 words ([1] is reserved).
 * labels_all: int32 label of every node (or NULL with out_labels NULL). */
int pcg_pick_shuffled(const double *cum, const int32_t *idx_train, int32_t n_train, uint64_t seed, uint64_t epoch_base,
                      uint64_t *epoch_counter, int32_t bump, int32_t k, const int32_t *labels_all, int32_t *out_ids,
                      int32_t *out_labels, void *stream);

/* pcg_pick_shuffled for n_epochs consecutive epochs in one launch: epoch e (= epoch_base + epoch_counter[0] + e) is drawn and
 * shuffled exactly as a call of its own would, into out_ids + e * k / out_labels + e * k; bump != 0: epoch_counter[0] += n_epochs. */
int pcg_pick_shuffled_epochs(const double *cum, const int32_t *idx_train, int32_t n_train, uint64_t seed, uint64_t epoch_base,
                             uint64_t *epoch_counter, int32_t bump, int32_t n_epochs, int32_t k, const int32_t *labels_all,
                             int32_t *out_ids, int32_t *out_labels, void *stream);

/* ---- dense tail: relation / inter GEMMs, classifier, loss, backward, Adam ---------------
 * Parameters live in ONE flat f32 buffer `theta` in this order (offsets from
 * pcg_dense_param_offset; shapes are the reference's state-dict shapes, row-major):
 *   which 0  weight                      [2, E]          src/model.py:29
 *   which 1  inter1.weight               [F + R*E, E]    src/layers.py:196
 *   which 2  inter1.intra_agg{rel+1}.weight [2F, E]      src/layers.py:559
 *   which 3  inter1.label_clf.weight     [2, F]          src/layers.py:200
 *   which 4  inter1.label_clf.bias       [2]
 * pcg_dense_step replaces, for one batch (B rows, tiles of 16 rows):
 *   self_feats gather, cat/mm/relu per relation   layers.py:273-277, 625-629
 *   cat/mm/relu of the inter aggregator           layers.py:284-289 ([B,E], not transposed)
 *   scores = W_cls . embeds, label-aware logits   model.py:38, layers.py:236-243
 *   both CrossEntropyLoss terms + loss.backward() model.py:54-61, model_handler.py:152
 * Outputs: logits [B,2], center [B,2]; optional combined [B,E], row_loss [B]
 * (per-row  xent(gnn) + lambda_1*xent(label); the batch loss is inv_count * sum).
 * slabs != NULL (training): labels required; slabs [pcg_dense_n_tiles(B), n_params]
 * receives per-tile partial gradients (already scaled by inv_count = 1/global batch),
 * and *step_counter (int32, may be NULL) is incremented.  slabs == NULL: inference.
 * pcg_adam_step sums the slabs in tile order (bitwise reproducible) and, if `apply`,
 * performs torch.optim.Adam's update with coupled weight decay on theta/m/v using
 * t = *step_counter (model_handler.py:124,153); grad_out [n_params] (optional)
 * receives the summed gradient. */
int64_t pcg_dense_n_params(int32_t feat_dim, int32_t emb, int32_t n_rel);
int64_t pcg_dense_param_offset(int32_t feat_dim, int32_t emb, int32_t n_rel, int32_t which, int32_t rel);
int32_t pcg_dense_n_tiles(int32_t B);
int pcg_dense_step(const pcg_graph_desc *g, const float *theta, int32_t emb,
                   const int32_t *ids, const int32_t *labels, int32_t B,
                   const float *agg, int32_t agg_stride, float lambda_1, float inv_count,
                   float *logits, float *center, float *combined, float *row_loss,
                   float *slabs, int32_t *step_counter, void *stream);
int pcg_adam_step(float *theta, float *m, float *v, const float *slabs, int32_t n_slabs, int64_t n_params,
                  const int32_t *step_counter, const pcg_adam_hyper *hyper, float *grad_out, int32_t apply, void *stream);

/* The training step's tail and front with Adam taken off the critical path (src/model_handler.py:149-153).
 *
 * pcg_train_dense = pcg_dense_step over st (theta, emb, lambda_1, slabs, step_counter), batch and out, plus
 *   - sel->workspace != NULL (with batch->cnt, batch->plan, sel->list_capacity as given to pcg_choose_gather_planned; nothing
 *     else of sel is read): aggregates of rows the gather left as partial sums are added up here (no combine launch);
 *   - adam_clf == 2 (training; slabs, sync_words required): gradient slabs only, marked as waiting (sync_words[1] = 1,
 *     sync_words[2] = #slabs) for the deferred update of the next pcg_choose_gather_train / pcg_adam_flush; the label
 *     classifier's own step is pcg_choose_gather_train's (its share of the slabs is written but not used);
 *   - adam_clf == 3 (training; st->acts, act_ld, sync_words required; slabs unused): NO gradient slabs.  The launch - one workgroup
 *     per 16 batch rows - runs forward, loss and the activation gradients and leaves, TRANSPOSED (one batch row per column,
 *     act_ld floats per row, act_ld >= B rounded up to 16, a multiple of 4; acts 16-byte aligned, pcg_wgrad_act_rows(...) rows):
 *     [self | h_r] , agg_r, dcomb, dh_r, combined, dlogits, dcentre - what every weight gradient is a GEMM over the batch of
 *     (src/layers.py:625-629, 284-289; src/model.py:54-61).  It marks them as waiting (sync_words[1] = 2, sync_words[2] = B / 16
 *     rounded up) for the next pcg_choose_gather_train / pcg_adam_flush over the same acts, whose workgroups run those GEMMs (f32 MFMA,
 *     fixed summation order) and apply Adam tile by tile.  adam_clf == 4: the same without marking (pcg_wgrad follows).
 *     sort_keys != NULL (adam_clf == 3 only; the pos_keys buffer whose scratch half holds the NEXT step's unsorted train-pos keys,
 *     formed by the pcg_choose_gather_train(score_next) before this launch): if pcg_dense_sorts_keys(B, n_pos) the launch carries
 *     ceil(n_pos / 64) more workgroups that rank-sort them into the first half (src/layers.py:683-691's order) - one workgroup
 *     per 16 rows leaves most CUs of a batch of <= ~3000 rows idle; the next pcg_choose_gather_train is then told keys_sorted;
 *   - adam_clf == 1 (training: slabs, m, v, sync_words, hyper required): the workgroup that arrives last (device-scope ticket,
 *     write-through partial gradients) sums the label classifier's gradient over the tiles in tile order and applies
 *     Adam to those 2 * feat_dim + 2 parameters - the only ones the next step's score pass reads - and the launch marks the
 *     slabs as holding a gradient the OTHER parameters have not seen yet: sync_words[1] = 1, sync_words[2] = #slabs.
 * pcg_step_front_train = pcg_step_front(train_flag = 1; batch: ids, labels, B; sel: all of it) reading the label classifier from
 *   st->theta, with that deferred update (st: theta, m, v, emb, slabs, step_counter, sync_words, hyper; pcg_step_scores_train: the same)
 *   (parameters [0, offset of label_clf.weight), same arithmetic and summation order as pcg_adam_step) applied by extra
 *   workgroups beside the score pass when sync_words[1] is set; its second launch clears sync_words[1].
 * pcg_step_scores_train = the front of a training step whose plan exists already (pcg_plan_batches), ONE launch:
 *   [train-pos keys from their feature rows -> pos_keys' scratch half || that deferred update || score pass -> s0]; it zeroes
 *   sync_words[3]; the sort is left to pcg_choose_gather_planned(..., sync_words) (n_pos > 16384: the bucket sort's launches
 *   follow here instead and pos_keys is sorted on return).  Replaces src/layers.py:230-237.
 *   touched (may be NULL = score every row): this batch's byte map from pcg_mark_touched - only rows whose byte is set are
 *   scored (bit for bit the scores pcg_score_table gives them); the other entries of s0 keep whatever they held - the batch's
 *   selection never reads them.  For graphs whose feature table is far larger than what a batch touches.
 * pcg_adam_flush applies a still-deferred update now (two or three small launches) - before parameters are read or saved
 *   (st: every member but lambda_1; slabs may be NULL when acts is given: a step of adam_clf = 3 is applied by the weight-gradient
 *   GEMMs, sync_words[1] == 2); st->clf_next != NULL (the pcg_choose_gather_train step): the stepped label classifier is copied into theta [p_end, n_params) too,
 *   if an update was pending. */
int pcg_step_scores_train(const pcg_graph_desc *g, const pcg_train_state *st, float *s0, uint64_t *pos_keys,
                          const uint8_t *touched, void *stream);
/* Which rows the batches nodes[s * B, min((s + 1) * B, n_total)) can read the score of (src/layers.py:226-237 scores exactly
 * `unique_nodes` = batch + neighbours): one byte map per batch at maps + s * map_stride (map_stride >= pcg_touched_bytes(n_nodes),
 * a multiple of 16; maps 16-byte aligned) - zeroed, then 1 for every centre of the batch, every neighbour it has in any
 * relation, and every train positive (their scores feed pcg_pos_sort when there are more than 16384 of them).  Two launches for ALL batches: per epoch, like pcg_plan_batches - it depends on the picks and the CSR only. */
int64_t pcg_touched_bytes(int64_t n_nodes);
/* queue: uint32 [4 + n_rel * n_total] scratch (may be NULL if g->max_degree <= 4096): rows of more than 4096 neighbours - a
 * hub's - are queued by the per-row pass and marked by the whole grid in a third launch (one wave per row set the duration by
 * the longest row: 1.6 ms per epoch at 10 M nodes / 200 M edges). */
int pcg_mark_touched(const pcg_graph_desc *g, const int32_t *nodes, int32_t n_total, int32_t B, uint8_t *maps,
                     int64_t map_stride, uint32_t *queue, void *stream);
/* pcg_mark_touched from the batches' PLANS (pcg_plan_batches has run on `plans` for the same nodes / n_total / B / list_capacity;
 * an epoch of a pcg_plan_epochs group: pass that epoch's first slot and its n_total): the plan slots hold every row's record and the
 * degree-tier queues, so the hub rows (> 4096 neighbours) are swept, one id range at a time, into LDS bitmaps that are expanded
 * into the byte maps with coalesced stores - which also write every other byte zero (no zeroing pass) - and the other rows, the
 * centres and the train positives are marked afterwards.  Two launches; the same maps as pcg_mark_touched, bit for bit. */
int pcg_mark_touched_planned(const pcg_graph_desc *g, const int32_t *nodes, int32_t n_total, int32_t B, const void *plans,
                             int64_t plan_stride, int64_t list_capacity, uint8_t *maps, int64_t map_stride, void *stream);
int pcg_train_dense(const pcg_graph_desc *g, const pcg_train_state *st, const pcg_batch *batch, const float *agg,
                    int32_t agg_stride, const pcg_select_ws *sel, const pcg_dense_out *out, int32_t adam_clf, uint64_t *sort_keys,
                    void *stream);
int32_t pcg_dense_sorts_keys(int32_t B, int32_t n_pos);   /* 1: the launch above (adam_clf = 3, sort_keys) sorts n_pos keys at batch B */
/* Whole-set inference (test mode, forward only): gnn logits of nodes ids[0 .. n) -> out_logits [n][2] and, if out_center is not
 * NULL, the label-aware (centre) logits -> out_center [n][2].  ONE call enqueues everything: one score pass of theta's label
 * classifier over the whole table into the caller's s0 [n_nodes], then per chunk of chunk_rows ids (the last one may be shorter):
 * plan -> select -> gather (the launches of pcg_plan_epochs and pcg_choose_gather_planned: two to three) -> one persistent
 * forward-only dense launch (pcg_infer_blocks(chunk_rows) workgroups, each staging the weights once and running tile after tile).
 * thresholds: host, [n_rel]; no rho (no minority picks in test mode).  workspace: pcg_infer_workspace_bytes(g, emb, chunk_rows,
 * list_capacity) bytes, no initial contents required, not shared with a concurrent call; list_capacity must cover the largest
 * chunk's sum of pcg_sel_capacity_row(deg, threshold, rho, 0, n_pos, 0) over its rows and relations, else PCG_ST_SEL_OVERFLOW is
 * set in *status and that chunk selects nothing.
 * Parity: every logit is bit for bit what pcg_train_dense (labels = NULL, adam_clf = 0) writes for the same row after
 * pcg_score_table + pcg_plan_batches + pcg_choose_gather_planned in test mode with the same theta, whatever the batch or chunk
 * the row is in and whatever its position there (a row's selection list, gather chunks and dense sums are laid out per row,
 * the dense phases are dense_step_kernel's, with the same MFMA chains, K order, K-split and fma order). */
int64_t pcg_infer_workspace_bytes(const pcg_graph_desc *g, int32_t emb, int32_t chunk_rows, int64_t list_capacity);
int pcg_infer_set(const pcg_graph_desc *g, const float *theta, int32_t emb, const int32_t *ids, int32_t n, int32_t chunk_rows,
                  float *s0, const double *thresholds, void *workspace, int64_t list_capacity, float *out_logits, float *out_center,
                  uint32_t *status, void *stream);
int32_t pcg_infer_blocks(int32_t chunk_rows);   /* workgroups of the dense launch of a chunk of chunk_rows ids (host helper) */
/* Partitioned whole-set inference (pc-gnn_amd/dist.py, DistributedPCGNN.infer): the device work of ONE chunk of a rank's ids,
 * after the chunk's halo exchange (pcg_halo_collect on the inference halo's own table / counts / request list halo_ids, two
 * all-to-alls, pcg_halo_serve) has filled halo_X [halo_cap][feat_stride].  g is the rank's table [owned | train-pos | ...]
 * (hi - lo owned rows, g->n_pos replicated train-pos rows; CSR rows with global neighbour ids); ids [B] are local rows of owned
 * nodes.  Launches: a front (the halo rows' scores -> s0[halo_ids[i]], and when `first` is set also rows [0, n_table_rows) ->
 * s0[row_gid[row]]; s0 is indexed by global node id; the look-back words of the plan slot zeroed) -> plan (test mode) ->
 * select (centre b's score s0[ids[b] + lo]; lists of global ids) -> gather (ids translated with the inference table - owned:
 * id - lo, train-pos: pos_idx, fetched: halo_X row - multi-chunk rows left as partial sums) -> infer_dense_kernel.
 * out_logits / out_center [B][2] (out_center may be NULL).  workspace: pcg_infer_dist_workspace_bytes(g, emb, chunk_rows,
 * list_capacity), B <= chunk_rows; list_capacity must cover the chunk's sum of test-mode row capacities (else
 * PCG_ST_SEL_OVERFLOW in *status); an id in none of owned / train-pos / fetched sets bit 4 of counts[128].  B == 0: nothing.
 * Parity: every logit is bit for bit pcg_infer_set's for the same node on the whole graph with the same theta (scores are the
 * row's own arithmetic; lists, gather chunks and dense sums are laid out per row; the translation changes addresses only). */
int64_t pcg_infer_dist_workspace_bytes(const pcg_graph_desc *g, int32_t emb, int32_t chunk_rows, int64_t list_capacity);
int pcg_infer_chunk_dist(const pcg_graph_desc *g, const float *theta, int32_t emb, const int32_t *ids, int32_t B, int32_t first,
                         const int32_t *row_gid, int64_t n_table_rows, const float *halo_X, const int32_t *halo_ids, int32_t halo_cap,
                         int32_t lo, int32_t hi, const int32_t *pos_ids, const int32_t *pos_idx, const uint32_t *table,
                         int64_t table_slots, uint32_t *counts, float *s0, const double *thresholds, void *workspace,
                         int32_t chunk_rows, int64_t list_capacity, float *out_logits, float *out_center, uint32_t *status,
                         void *stream);
/* Scoring nodes that are NOT in the resident graph (test mode, forward only; FusedPCGNN.infer_new).  g is the BASE graph (N =
 * g->n_nodes >= 1 nodes): nothing of it is modified and the logits of its nodes are not recomputed.  q describes a QUERY BATCH of nq
 * new nodes, query node j having the global id N + j:
 *   q->n_nodes = nq;  q->X = Xq [nq, feat_stride] (16-byte aligned, pad columns zero);  q->indptr[r] int64 [nq + 1];
 *   q->indices[r] int32: GLOBAL ids in [0, N + nq), ascending inside a row - base nodes, other nodes of the batch, the node itself
 *   (a caller mirroring the reference keeps the self-loop: N + j in row j);  q->n_pos = 0, q->train_pos = NULL;
 *   q->max_degree = the query rows' own maximum.  feat_dim, feat_stride and n_rel must equal g's (else PCG_E_ARG); N + nq < 2^31.
 * ids [n]: query-local rows in [0, nq), any order, duplicates allowed.  out_logits [n][2]; out_center [n][2] or NULL.
 * s0 [N + nq] floats, owned by the caller across calls: score_base != 0 - the call first scores the base table into s0[0, N) (the
 * workgroups, rows and fma order of pcg_score_table); score_base == 0 - the caller guarantees that those N entries hold the scores
 * of theta's current label classifier (a previous call's, with theta unchanged since).  Either way the query rows are scored into
 * s0[N, N + nq) (the per-row arithmetic of pcg_score_table).
 * Launches: one front (the scores above || the look-back words of the two plan slots zeroed), then per chunk of chunk_rows ids
 * (the last one may be shorter): plan (test mode, pcg_plan_epochs over q's rows) -> select (pcg_choose_select_planned: centre b's
 * score s0[ids[b] + N], lists of global ids) -> a two-table gather (entry id < N reads row id of g->X, id >= N row id - N of q->X;
 * the chunks and the summation order per row of pcg_choose_gather_planned; rows of several 128-entry chunks left as partial sums)
 * -> the persistent forward-only dense launch of pcg_infer_set with the self rows from q->X.  Never synchronises, never allocates.
 * workspace: pcg_infer_new_workspace_bytes(g, q, emb, chunk_rows, list_capacity) bytes (>= pcg_infer_workspace_bytes of q for the
 * same chunk and capacity; negative = rejected arguments), no initial contents required; list_capacity as pcg_infer_set's, over the
 * QUERY rows' degrees (else PCG_ST_SEL_OVERFLOW in *status and that chunk selects nothing).
 * The caller's contract, as for the base CSR: every entry of q->indices is in [0, N + nq) - the select kernel reads s0[id] for
 * every neighbour before anything checks it.  The gather skips a list entry outside that range like a hole and sets
 * PCG_ST_LIST_ID_RANGE, which is a report, not a guard.  (pc-gnn_amd/graph.py: QueryBatch validates on the host.)
 * n == 0 or nq == 0: nothing is enqueued.
 * Parity: every logit is bit for bit what pcg_infer_set writes for node N + j on a graph built with the query rows appended to
 * the base table and CSR, with the same theta (a node's test-mode logits depend on its own row, its own lists, the scores and
 * rows of those neighbours and the parameters - on nothing else in the graph). */
int64_t pcg_infer_new_workspace_bytes(const pcg_graph_desc *g, const pcg_graph_desc *q, int32_t emb, int32_t chunk_rows,
                                      int64_t list_capacity);
int pcg_infer_new(const pcg_graph_desc *g, const pcg_graph_desc *q, const float *theta, int32_t emb, const int32_t *ids, int32_t n,
                  int32_t chunk_rows, float *s0, int32_t score_base, const double *thresholds, void *workspace,
                  int64_t list_capacity, float *out_logits, float *out_center, uint32_t *status, void *stream);
/* Node embeddings from the whole-set pass (FusedPCGNN.embed, embed_new).  pcg_embed_set / pcg_embed_new are pcg_infer_set /
 * pcg_infer_new - the same arguments, checks, workspace (pcg_infer_workspace_bytes / pcg_infer_new_workspace_bytes) and launches -
 * whose dense launch also stores what the classifier sees:
 *   out_emb [n][emb]          row i = combined = relu([self | h_1 .. h_R] W_inter), the row W_cls multiplies;
 *   out_rel [n][n_rel * emb]  row i = h_1 | .. | h_R, h_r = relu([self | agg_r] W_intra[r]); or NULL.
 * out_logits, out_center and out_emb may each be NULL too; all four NULL is PCG_E_ARG.
 * Parity: out_emb row i is bit for bit what pcg_train_dense (labels NULL) writes to pcg_dense_out.combined for that node, whatever
 * the chunk, tile or position of the row; the logits are bit for bit pcg_infer_set's / pcg_infer_new's; pcg_embed_new's rows equal
 * pcg_embed_set's for node N + j on the graph built with the query rows appended. */
int pcg_embed_set(const pcg_graph_desc *g, const float *theta, int32_t emb, const int32_t *ids, int32_t n, int32_t chunk_rows,
                  float *s0, const double *thresholds, void *workspace, int64_t list_capacity, float *out_logits, float *out_center,
                  float *out_emb, float *out_rel, uint32_t *status, void *stream);
int pcg_embed_new(const pcg_graph_desc *g, const pcg_graph_desc *q, const float *theta, int32_t emb, const int32_t *ids, int32_t n,
                  int32_t chunk_rows, float *s0, int32_t score_base, const double *thresholds, void *workspace,
                  int64_t list_capacity, float *out_logits, float *out_center, float *out_emb, float *out_rel, uint32_t *status,
                  void *stream);
/* Whole-set inference for the GraphSAGE / GCN baselines (BaselineEngine, pc-gnn_amd/baseline.py; src/graphsage.py:62-96, 127-150,
 * 167-174, 200-232, 262-275).  For centre v: S(v) = row v of relation `rel`'s CSR (sorted, distinct), united with v itself when
 * add_self is set and v is not in it; c = |S(v)|;
 *   a(v)   = (sum of X[u], u in S(v)) / den,  den = (float)c (PCG_NORM_COUNT) or sqrtf((float)c) (PCG_NORM_SQRT_COUNT): one float32
 *            division per element; c == 0: 0 / 0 = NaN, through the ReLU into the logits, like the reference;
 *   z      = [X[v] | a(v)] (concat_self; K = 2 * feat_dim) or a(v) (K = feat_dim);
 *   h      = relu(W_enc z), W_enc [emb][K] row-major;   logits = W_cls h, W_cls [2][emb].  No bias.
 * The CSR row is read in place: no plan, no selection, no per-edge list.  pcg_baseline_workspace_bytes depends on chunk_rows and
 * g->feat_stride only, never on degrees or edge counts.  A row's values are a function of the row alone - its summation order is
 * picked by its own degree and fixed, no float atomics - so they are bit for bit the same whatever n, chunk_rows, the row's
 * position in ids or the call.  The dense part is exact float32 (v_mfma_f32_16x16x4_f32).
 * workspace: pcg_baseline_workspace_bytes(g, m, chunk_rows) bytes, no initial contents required (every chunk zeroes the long-row
 * queue's counter itself; the aggregates and the queue are written before they are read).
 *   out_logits [n][2];  out_emb [n][emb] (h) or NULL;  out_agg [n][feat_dim] (a) or NULL.
 * Checks, before any launch: NULL g / g->X / m / W_enc / W_cls / ids / workspace / status / out_logits, n < 0, chunk_rows < 1, rel
 * outside [0, n_rel), a norm other than the two constants, X or workspace not 16-byte aligned, workspace_bytes below
 * pcg_baseline_workspace_bytes(g, m, chunk_rows): PCG_E_ARG; emb < 16, emb % 16 != 0, a table the other whole-set calls reject
 * (feat_stride % 4 != 0 or > 512) or an LDS need above 160 KB: PCG_E_UNSUPPORTED.  n == 0: PCG_OK, nothing is enqueued.
 * An id outside [0, n_nodes) - in ids or in the CSR - is clamped for the read and sets PCG_ST_LIST_ID_RANGE in *status.
 * Three launches and a 4-byte memset per chunk; the weights are read during the call only (pass the live parameters). */
typedef struct pcg_baseline_model {
    int32_t rel, norm, add_self, concat_self, emb, _pad;
    const float *W_enc;   /* [emb][K] */
    const float *W_cls;   /* [2][emb] */
} pcg_baseline_model;
int64_t pcg_baseline_workspace_bytes(const pcg_graph_desc *g, const pcg_baseline_model *m, int32_t chunk_rows);
int pcg_baseline_infer(const pcg_graph_desc *g, const pcg_baseline_model *m, const int32_t *ids, int32_t n, int32_t chunk_rows,
                       void *workspace, int64_t workspace_bytes, float *out_logits, float *out_emb, float *out_agg,
                       uint32_t *status, void *stream);
/* Training steps of the GraphSAGE / GCN baselines (BaselineEngine.train_step / train_epoch / loss_and_grad; src/graphsage.py:37-39,
 * 176-178 with torch.optim.Adam, src/model_handler.py:124, 149-153): ids [n] with labels [n] (int32, 0 / 1) in batches of
 * batch_rows, the last one shorter; batch i is step first_step + i.  Per batch, on the stream, with no host synchronisation:
 *   the aggregation of pcg_baseline_infer -> baseline_train_dense_kernel -> baseline_wgrad_adam_kernel.
 *   forward: pcg_baseline_infer's own tile code - the logits are bit for bit what it returns for those ids;
 *   loss_i = two-class cross entropy of row i;  out_loss[batch] = (sum of loss_i: a tile's 16 rows in row order, the tiles in
 *            tile order) / B - nn.CrossEntropyLoss()'s mean;
 *   dlogits = (softmax - onehot) / B;  dpre = (W_cls^T dlogits) where h > 0 (h <= 0: 0; a NaN h lets it through, as torch's ReLU);
 *   dW_enc[e][k] = sum_t dpre[t][e] z[t][k];  dW_cls[c][e] = sum_t dlogits[t][c] h[t][e]: float32 MFMA sums over the batch in a
 *            fixed order (no float atomics: bitwise the same run to run); batches of more than 1024 rows are shared by up to four
 *            workgroups per 16 x 16 tile (ceil(B / 1024), at most 4), their partial tiles added in part order.
 *   apply != 0: the thread that owns a parameter applies torch.optim.Adam's update (coupled weight decay, step number
 *            first_step + batch) to W_enc / W_cls IN PLACE - through m->W_enc / m->W_cls, which must be writable - and to
 *            m_enc / v_enc [emb][K], m_cls / v_cls [2][emb]; the next batch's dense launch is the first reader.
 *   apply == 0: nothing is updated; grad_out [2 * emb + emb * K] = [dW_cls | dW_enc] of the one batch (n <= batch_rows).
 *            (apply != 0 with grad_out: the last batch's gradient.)
 * A centre without neighbours (no add_self) makes its aggregate, the loss and every gradient NaN, as autograd does.
 * workspace: pcg_baseline_train_workspace_bytes(g, m, batch_rows) bytes, 16-byte aligned; a function of batch_rows,
 * g->feat_dim, g->feat_stride and the model's shape only.  Its contents are irrelevant on entry.
 * Checks, before any launch: pcg_baseline_infer's on g, m, ids, workspace, status; NULL opt / labels / out_loss, n < 0,
 * batch_rows < 1; apply != 0 with a NULL m_enc / v_enc / m_cls / v_cls or first_step < 1; apply == 0 with a NULL grad_out or
 * n > batch_rows; workspace_bytes too small: PCG_E_ARG.  Shapes: PCG_E_UNSUPPORTED exactly where pcg_baseline_infer returns it.
 * n == 0: PCG_OK, nothing is enqueued.  An id outside [0, n_nodes) is clamped for the read and sets PCG_ST_LIST_ID_RANGE; a label
 * outside {0, 1} sets PCG_ST_EVAL_INPUT and its row contributes nothing to the loss or the gradients (it still counts in B). */
typedef struct pcg_baseline_opt {
    float *m_enc, *v_enc;   /* [emb][K] */
    float *m_cls, *v_cls;   /* [2][emb] */
    int64_t first_step;     /* the 1-based number of the first batch's step; by value: the caller owns the count */
    int32_t apply, _pad;
    pcg_adam_hyper hyper;
} pcg_baseline_opt;
int64_t pcg_baseline_train_workspace_bytes(const pcg_graph_desc *g, const pcg_baseline_model *m, int32_t batch_rows);
int pcg_baseline_train(const pcg_graph_desc *g, const pcg_baseline_model *m, const pcg_baseline_opt *opt, const int32_t *ids,
                       const int32_t *labels, int32_t n, int32_t batch_rows, void *workspace, int64_t workspace_bytes,
                       float *out_loss /* [ceil(n / batch_rows)] */, float *grad_out, uint32_t *status, void *stream);
/* The k most similar rows of bank [M][emb] for every row of Q [n][emb] (both float32, row-major, 16-byte aligned), without an
 * [n][M] matrix: exact-f32 MFMA scores and a running top-k (FusedPCGNN.nearest, ops.topk_similar).
 * metric - the score is always MAXIMISED: 0 dot q.c;  1 cosine q.c / (|q| |c|), 0 when either norm is 0;
 *          2 l2 min(0, 2 q.c - |q|^2 - |c|^2).  A NaN score counts as -inf.
 * q_ids [n], bank_ids [M]: both or neither (one alone: PCG_E_ARG); candidate c is skipped for row i when bank_ids[c] == q_ids[i].
 * out_pos [n][k] (bank positions), out_score [n][k]: sorted by score descending, ties by lower position; slots beyond the number of
 * eligible candidates hold position -1 and score -inf.  The result is a function of the scores alone: it does not depend on the
 * grid, on how the bank is sliced over waves (partial lists are merged by the same (score, position) key), nor on any arrival
 * order - there are no atomics.  A pair's score is its own arithmetic whatever tile it is in.
 * Ranges: 1 <= k <= 64 (else PCG_E_ARG); emb % 16 == 0, 16 <= emb <= 512 (else PCG_E_UNSUPPORTED); n, M >= 0 (negative:
 * PCG_E_ARG); n == 0: nothing is enqueued; M == 0: all padding.  workspace: pcg_topk_similar_workspace_bytes(n, M, emb, k) bytes
 * (negative = rejected arguments; non-decreasing in n and M), no initial contents required.  status is reserved: nothing is
 * detected on the device, the word is not written.  Launches: [row norms, metrics 1 and 2] -> scan -> [merge, when the bank was
 * sliced].  Never synchronises, never allocates.
 * pcg_debug_set_topk_slices(s): tests only - s > 0 asks for s bank slices (clamped to what the workspace holds), 0 = choose. */
int64_t pcg_topk_similar_workspace_bytes(int32_t n, int32_t M, int32_t emb, int32_t k);
int pcg_topk_similar(const float *Q, int32_t n, const float *bank, int32_t M, int32_t emb, int32_t k, int32_t metric,
                     const int32_t *q_ids, const int32_t *bank_ids, int32_t *out_pos, float *out_score, void *workspace,
                     uint32_t *status, void *stream);
void pcg_debug_set_topk_slices(int32_t n_slices);
/* The chosen neighbours of test-mode rows in the reference's order, with their distances (choose_step_test's samp_neighs /
 * samp_scores, src/layers.py:713-736; FusedPCGNN.chosen, ops.choose_ranked).
 * pcg_rank_lists: over the lists (and the plan) a pcg_choose_select* call in TEST mode (train_flag = 0, add_self = 0) left in
 * `workspace` (the single-buffer layout of pcg_choose_workspace_bytes(g, B, list_capacity)) for the batch nodes [B].  Row (r, b)
 * is written at out_begin[r * B + b] of out_ids / out_dist:
 *   deg <= k + 1 (keep-all): the list's order (ascending position in the ascending-id row), out_dist[j] = |c - s0[id_j]|;
 *   deg >  k + 1 (ranked)  : ascending distance, ties by list position (torch.sort(stable = True) of the reference's score_diff).
 * c = center_s0 ? center_s0[b] : s0[nodes[b]] - as pcg_choose_select; the distance is one f32 subtract and abs: the bits of
 * torch.abs(c - s), and of the key the select kernel ranked by.
 * out_begin int64 [n_rel * B + 1], ascending from 0: the caller forms it on the host - a test-mode row keeps exactly
 * pcg_sel_capacity_row(deg, threshold, 0, 0, n_pos, 0) entries - and sizes out_ids / out_dist [out_begin[n_rel * B]] with it.
 * A row whose device count differs from out_begin[i + 1] - out_begin[i] (or whose extent leaves [0, out_begin[n_rel * B]]) sets
 * PCG_ST_RANK_MISMATCH in *status and is not written; nothing is ever written outside a row's extent.  A list entry outside
 * [0, n_nodes) is clamped for the score read and sets PCG_ST_LIST_ID_RANGE.  Two launches (rows of <= 64 kept entries: one wave
 * each, the shortest four per wave; longer rows: a workgroup per 2048 entries, every one counting its slice against all of the
 * row's keys); no workgroup waits for another.  Never synchronises, never allocates; B == 0: nothing is enqueued.
 * pcg_chosen_set: ONE call for any id set ids [n] (any order, duplicates allowed): pcg_infer_set's score pass into s0 [n_nodes],
 * then per chunk of chunk_rows ids plan (test mode) -> select (rows beyond the select kernel's LDS key capacity in its long-row
 * launch, as in pcg_infer_set) -> rank; no gather, no dense launch.  Row (r, i) is written at out_begin[r * n + i]
 * (out_begin int64 [n_rel * n + 1]).  theta, emb: the flat parameter buffer of pcg_dense_step - only its label classifier is
 * read.  workspace: pcg_chosen_workspace_bytes(g, chunk_rows, list_capacity) bytes, no initial contents required; list_capacity
 * as pcg_infer_set's (else PCG_ST_SEL_OVERFLOW and that chunk writes nothing).  n == 0: nothing is enqueued. */
int pcg_rank_lists(const pcg_graph_desc *g, const int32_t *nodes, int32_t B, const float *s0, const float *center_s0,
                   const void *workspace, int64_t list_capacity, const int64_t *out_begin, int32_t *out_ids, float *out_dist,
                   uint32_t *status, void *stream);
int64_t pcg_chosen_workspace_bytes(const pcg_graph_desc *g, int32_t chunk_rows, int64_t list_capacity);
int pcg_chosen_set(const pcg_graph_desc *g, const float *theta, int32_t emb, const int32_t *ids, int32_t n, int32_t chunk_rows,
                   float *s0, const double *thresholds, void *workspace, int64_t list_capacity, const int64_t *out_begin,
                   int32_t *out_ids, float *out_dist, uint32_t *status, void *stream);
/* The minority picks of TRAIN-mode rows, ranked, with their distances (choose_step_neighs' tail, src/layers.py:675-691; the
 * minority part of FusedPCGNN.chosen(train_flag=True) / ops.choose_ranked(labels=...)).  The extent of row (r, i),
 * out_begin[r * n + i + 1] - out_begin[r * n + i], IS that row's m = min(int(k * rho), n_pos) - 0 for a negative centre and for
 * int(k * rho) == 0 (the caller forms it on the host: pcg_sel_capacity_row's minority term).  The row receives the m training
 * positives nearest to c = center_s0 ? center_s0[i] : s0[nodes[i]] in ascending order of the unique key
 * (orderable(|c - s_p|) << 32) | p, p = the position in train_pos - torch.sort(stable = True) over train_pos order, and the
 * select kernel's tie rule: out_ids = train_pos[p], out_dist = fabsf(c - s_p) (one f32 subtract and abs, s_p from the sorted
 * key's high word: the bits of torch.abs).  A pick that is also a kept neighbour of the row is reported, not removed (the
 * reference's samp_score_diff keeps it).  pos_keys: what pcg_pos_sort left for the same s0.  A row whose extent is negative,
 * above n_pos or leaves [0, out_begin[n_rel * n]] sets PCG_ST_RANK_MISMATCH in *status and is not written; a position read from
 * a key is clamped below n_pos before train_pos is read, a slot is written only below its row's extent.  One ranking per centre
 * serves every relation (row (r, i) is the prefix of m_r entries).  Two launches (centres of <= 64 candidates: one wave each;
 * more: a workgroup per 2048 candidates, counted against all of the centre's candidates - quadratic in the candidate count, so
 * a tie run of thousands is exact, not fast); no workgroup waits for another.  Never synchronises, never allocates, needs no
 * workspace and no plan; n == 0 or n_pos == 0: nothing is enqueued. */
int pcg_rank_minority(const pcg_graph_desc *g, const int32_t *nodes, int32_t n, const float *s0, const float *center_s0,
                      const uint64_t *pos_keys, const int64_t *out_begin, int32_t *out_ids, float *out_dist, uint32_t *status,
                      void *stream);
/* Exact input attributions of the gnn logits (FusedPCGNN.attribute, ops.neighbour_contrib).  The gnn path has no bias, so with the
 * selection held fixed s = w0 * logit0 + w1 * logit1 is positively homogeneous of degree 1 in (x, a_1 .. a_R) - the centre's own
 * row and the means of its chosen rows - and gradient times input splits it completely:
 *   s[b] = <x_b, d_self[b]> + sum_r <a_r[b], d_agg[r, b]>,   <a_r[b], d_agg[r, b]> = sum_{j in chosen(r, b)} <X[j], d_agg[r, b]> / |chosen|.
 * pcg_attr_set: pcg_infer_set's arguments, checks, workspace (pcg_infer_workspace_bytes) and launches - one front, then per chunk
 * plan (test mode) -> select -> gather -> a dense launch that runs pcg_infer_set's forward phases unchanged (out_logits [n][2] is
 * bit for bit pcg_infer_set's) and from their LDS state the backward to the inputs (three MFMA phases, exact f32):
 *   out_d_self [n][feat_dim] = d s / d x;  out_d_agg [n_rel][n][feat_dim] = d s / d a_r;  out_self_contrib [n] = <x, d_self>;
 *   out_rel_contrib [n_rel][n] = <a_r, d_agg_r>.  w0, w1 must be finite (else PCG_E_ARG).
 * A row's values depend on the row alone (not on its tile, chunk or position); a row with an empty neighbour set has pcg_infer_set's logits
 * (its 0 / 0 aggregate included) and unspecified attributions, and disturbs no other row.  Never synchronises, never allocates; n == 0:
 * nothing is enqueued.
 * pcg_attr_neighbours: for every entry e of row (r, i) of ranked lists (flat_offsets int64 [n_rel * n + 1], ids int32
 * [flat_offsets[n_rel * n]]: pcg_chosen_set's out_begin / out_ids) out[e] = <X[ids[e]], d_agg[r, i]> / row length; d_agg any
 * [n_rel][n][feat_dim] f32 array.  Every dot product is formed by a fixed lane group in a fixed order: the bits do not depend on
 * the launch geometry.  An id outside [0, n_nodes) is clamped for the read and sets PCG_ST_LIST_ID_RANGE; a row whose offsets
 * are not 0 <= begin <= end <= flat_offsets[n_rel * n] sets PCG_ST_RANK_MISMATCH and is not written.  One launch; rows longer
 * than 128 entries are sliced over workgroups.  Never synchronises, never allocates; n == 0: nothing is enqueued. */
int pcg_attr_set(const pcg_graph_desc *g, const float *theta, int32_t emb, const int32_t *ids, int32_t n, int32_t chunk_rows,
                 float *s0, const double *thresholds, void *workspace, int64_t list_capacity, float w0, float w1, float *out_logits,
                 float *out_d_self, float *out_d_agg, float *out_self_contrib, float *out_rel_contrib, uint32_t *status,
                 void *stream);
int pcg_attr_neighbours(const pcg_graph_desc *g, const int64_t *flat_offsets, const int32_t *ids, int32_t n_rel, int32_t n,
                        const float *d_agg, float *out, uint32_t *status, void *stream);
/* Explaining nodes that are NOT in the graph (FusedPCGNN.chosen_new / attribute_new): for the rows ids [n] of a query batch q
 * (pcg_infer_new's descriptor, ids, s0 / score_base, thresholds, workspace and list_capacity contracts, word for word) the chosen
 * neighbours, ranked, with their distances, and / or the exact input attributions of the gnn logits, from ONE selection per chunk.
 * out: the groups of pcg_explain_out - attribution (logits, d_self, d_agg, self_contrib, rel_contrib: pcg_attr_set's outputs for
 * s = w0 * logit0 + w1 * logit1; w0, w1 finite, else PCG_E_ARG), chosen (out_begin - an input: row (r, i) keeps exactly
 * pcg_sel_capacity_row(deg_q, threshold, 0, 0, 0, 0) entries -, out_ids, out_dist: pcg_chosen_set's outputs; the ids are GLOBAL,
 * in [0, N + nq)) and neigh_contrib (pcg_attr_neighbours' output for those lists and d_agg; only beside both other groups).  A
 * NULL struct, no group, a half-filled group or neigh_contrib without both groups is PCG_E_ARG before anything is enqueued.
 * Checks: pcg_infer_new's, and pcg_attr_set's bound on the backward's LDS (PCG_E_UNSUPPORTED).
 * Launches: pcg_infer_new's front (the base table's scores only when score_base != 0, the query rows' scores -> s0[N, N + nq), the
 * look-back words zeroed); per chunk of chunk_rows ids plan (test mode, over q's rows) -> select ONCE (centre b's score
 * s0[ids[b] + N]) -> [chosen] the two rank launches of pcg_rank_lists directly behind it (they only read the lists and the plan)
 * -> [attribution] pcg_infer_new's two-table gather -> pcg_attr_set's dense launch with the self rows from q->X; after the last
 * chunk -> [neigh_contrib] one gather-dot over all R * n ranked rows (entry id < N reads row id of g->X, id >= N row id - N of
 * q->X; its tail slices sized by q->max_degree).  Never synchronises, never allocates.  n == 0 or nq == 0: nothing is enqueued.
 * workspace: pcg_explain_new_workspace_bytes (== pcg_infer_new_workspace_bytes for the same arguments; negative = rejected).
 * Status bits: PCG_ST_SEL_OVERFLOW (list_capacity too small: that chunk selects nothing; its ranked rows are then not written -
 * PCG_ST_RANK_MISMATCH - and what the gather-dot reads in their place is clamped), PCG_ST_LIST_ID_RANGE (a list entry outside
 * [0, N + nq): skipped by the gather like a hole, clamped for the rank's score read and for the gather-dot's row read - a report,
 * not a guard: the caller's contract on q->indices is pcg_infer_new's), PCG_ST_RANK_MISMATCH (a row whose kept count on the device
 * is not its extent in out_begin, or whose extent leaves the arrays, is not written; nothing is written outside a row's extent).
 * Parity: every value is bit for bit what pcg_chosen_set, pcg_attr_set and pcg_attr_neighbours write for node N + j on a graph
 * built with the query rows appended to the base table and CSR, with the same theta - whichever groups are requested, whatever
 * the chunk or the row's position: the table a row is read from changes an address, not a value or an order. */
int64_t pcg_explain_new_workspace_bytes(const pcg_graph_desc *g, const pcg_graph_desc *q, int32_t emb, int32_t chunk_rows,
                                        int64_t list_capacity);
int pcg_explain_new(const pcg_graph_desc *g, const pcg_graph_desc *q, const float *theta, int32_t emb, const int32_t *ids, int32_t n,
                    int32_t chunk_rows, float *s0, int32_t score_base, const double *thresholds, void *workspace,
                    int64_t list_capacity, float w0, float w1, const pcg_explain_out *out, uint32_t *status, void *stream);
int pcg_step_front_train(const pcg_graph_desc *g, const pcg_train_state *st, float *s0, uint64_t *pos_keys, const pcg_batch *batch,
                         const pcg_select_ws *sel, void *stream);
/* The optimizer of a data-parallel / partitioned step, whose gradient passes through an all-reduce: pcg_grad_reduce sums the
 * slabs (tile order) into grad_out and sets flag[0] ("a gradient is waiting"); after the collective, pcg_adam_apply_pending - at
 * the head of the NEXT step's launches, or on its own before parameters are read - applies torch.optim.Adam's update from grad to
 * every parameter if flag[0] is set.  The flag is cleared by a later launch: clear != 0 adds a one-thread launch that does it;
 * clear == 0 leaves it to the caller's next launch (flag = sync_words + 1: pcg_choose_select_planned(sync_words) clears it).
 * flag: one zero-initialised uint32 device word. */
int pcg_grad_reduce(const float *slabs, int32_t n_slabs, int64_t n_params, float *grad_out, uint32_t *flag, void *stream);
int pcg_adam_apply_pending(float *theta, float *m, float *v, const float *grad, int64_t n_params, const int32_t *step_counter,
                           uint32_t *flag, int32_t clear, const pcg_adam_hyper *hyper, void *stream);
/* The partitioned step's front and gather (pc-gnn_amd/dist.py; the reference has no distributed code).
 * pcg_step_scores_dist = pcg_step_scores with the optimizer riding in it (st: theta, m, v, emb, step_counter, sync_words, hyper),
 *   ONE launch behind the gradient all-reduce: if
 *   sync_words[1] == 1 (pcg_wgrad(flag_set) / pcg_grad_reduce) torch.optim.Adam's update from grad [n_params] (the all-reduced
 *   gradient) is applied to EVERY parameter by some workgroups while the others score rows [row_begin, row_end) ->
 *   s0_out[row_ids[row]] and form the train positives' unsorted keys (rows pos_row_base + i; pos_keys may be NULL) with the label
 *   classifier AFTER that update - each works it out for itself from clf_snap [3 * (2 feat_dim + 2)] (the classifier's
 *   parameters, m, v as of the last applied update) and the gradient, same arithmetic, same bits.  The flag is cleared by the
 *   step's select launch (pcg_choose_select_planned(sync_words)); the launch zeroes sync_words[3].
 * pcg_gather_lists_dist = pcg_gather_lists_planned over lists of NODE ids: translated to rows of the extended table
 *   [ owned | train-pos | halo ] as they are read (table / counts / pos_ids / pos_idx as pcg_halo_lookup; the list is left as it
 *   is; an id in none of the three is skipped and sets overflow bit 4 in counts[128]); snap_dst != NULL: the launch also copies
 *   theta / m / v [clf_offset, clf_offset + clf_n) to snap_dst [3 * clf_n] - the snapshot the NEXT step's pcg_step_scores_dist reads. */
int pcg_step_scores_dist(const pcg_graph_desc *g, const pcg_train_state *st, const float *grad, const float *clf_snap,
                         int64_t row_begin, int64_t row_end, float *s0_out, const int32_t *row_ids, uint64_t *pos_keys,
                         int64_t pos_row_base, void *stream);
int pcg_gather_lists_dist(const float *X, int32_t feat_dim, int32_t feat_stride, int64_t table_rows, int32_t n_rows,
                          const int32_t *cnt, const pcg_graph_desc *g, int32_t B, void *workspace, const void *plan,
                          int64_t list_capacity, float *agg, int32_t agg_stride, uint32_t *status, int32_t lo, int32_t hi,
                          int32_t n_local, const int32_t *pos_ids, const int32_t *pos_idx, int32_t n_pos, const uint32_t *table,
                          int64_t table_slots, uint32_t *counts, int32_t halo_cap, int32_t halo_base, const float *theta,
                          const float *m, const float *v, int64_t clf_offset, int32_t clf_n, float *snap_dst, void *stream);
int pcg_adam_flush(const pcg_train_state *st, int32_t n_slabs, int64_t n_params, int64_t p_end, int32_t feat_dim, int32_t n_rel,
                   void *stream);
/* The weight gradients of pcg_train_dense(adam_clf = 3 / 4)'s transposed activations as GEMMs over the batch (B rows; one
 * 256-thread workgroup per 16 x 16 tile of a weight matrix, its four waves a quarter of the batch each, partial tiles added in
 * wave order; st: acts, act_ld, emb, wg_scratch, hyper, and - required only if apply - theta, m, v, step_counter): grad_out
 * [n_params] (may be NULL) gets the gradient, apply != 0 applies torch.optim.Adam's update (coupled weight
 * decay; t = step_counter[0]) to the tile's parameters.  with_clf == 0 leaves the label classifier's 2 * feat_dim + 2 entries
 * alone (its step is pcg_choose_gather_train's).  Batches beyond 1024 rows: a tile is shared by one workgroup per 1024 rows, whose
 * partial tiles meet in wg_scratch (pcg_wgrad_scratch_bytes(feat_dim, emb, n_rel, largest B), zero-initialised ONCE by the caller:
 * arrival tickets, left zero by every launch, then the partial tiles) and are added in part order by the one that arrives last;
 * wg_scratch may be NULL for B <= 1024 (act_ld <= 1024 where the batch size is only known on the device: pcg_adam_flush,
 * pcg_choose_gather_train).  act_ld: a multiple of 16.  flag_set (may be NULL): a device word the launch sets to 1 - "a gradient
 * is waiting" for pcg_step_scores_dist / pcg_adam_apply_pending.  Replaces src/model_handler.py:152-153 for those parameters. */
int64_t pcg_wgrad_act_rows(int32_t feat_dim, int32_t emb, int32_t n_rel);
int64_t pcg_wgrad_scratch_bytes(int32_t feat_dim, int32_t emb, int32_t n_rel, int32_t B);
int pcg_wgrad(const pcg_train_state *st, int32_t B, int32_t feat_dim, int32_t n_rel, float *grad_out, int32_t apply,
              int32_t with_clf, uint32_t *flag_set, void *stream);
/* Custom losses on the fused path: the dense launch of pcg_train_dense(adam_clf = 4) with its backward started from the CALLER's
 * loss gradients instead of the built-in CE(gnn) + lambda_1 * CE(label) (additive since ABI 13; no new struct).  The launch runs
 * the forward for the batch (bit for bit pcg_train_dense's logits), takes row b's seeds d_logits[2b], d_logits[2b + 1] = d loss /
 * d gnn logits and d_center[2b], d_center[2b + 1] = d loss / d label-aware logits (device float [B, 2] each) AS GIVEN - no
 * 1 / count, no lambda_1, no label read, non-finite values propagate - and leaves the transposed activations / activation
 * gradients in st->acts; pcg_wgrad(with_clf = 1) over the same acts then gives every parameter's gradient (apply = 0) or steps
 * every parameter (apply = 1).  Nothing else of the backward depends on the loss, and the selection is not differentiated.
 *   st:    theta, emb, acts, act_ld (what pcg_train_dense(adam_clf = 4) reads); no slabs, no sync words, no Adam state, and
 *          step_counter is not touched
 *   batch: ids, B, cnt, plan; labels and inv_count are ignored
 *   agg, agg_stride, sel: as given to pcg_choose_gather_planned for this batch (sel->workspace != NULL: rows the gather left
 *          as partial sums are added up here, as in pcg_train_dense)
 *   out:   may be NULL; logits / center / combined that are not NULL are written by the launch's own forward; row_loss is ignored
 * PCG_E_ARG before any launch: a NULL g / st / batch / sel / d_logits / d_center, NULL theta or acts, B < 0, NULL ids with
 * B >= 1, and whatever pcg_train_dense(adam_clf = 4) rejects; PCG_E_UNSUPPORTED exactly where that call returns it.  B == 0:
 * PCG_OK, nothing is enqueued.  One 1024-thread workgroup per 16 batch rows, the shape dispatch of the training launch. */
int pcg_dense_vjp(const pcg_graph_desc *g, const pcg_train_state *st, const pcg_batch *batch, const float *agg, int32_t agg_stride,
                  const pcg_select_ws *sel, const float *d_logits, const float *d_center, const pcg_dense_out *out, void *stream);

/* ---- multi-GPU halo exchange helpers (no counterpart in the reference) ----------
 * A rank of a partitioned run holds the table [ owned rows | train-pos rows | halo ]; CSR rows and selection lists hold
 * GLOBAL ids.  Feature rows never change, so a fetched row stays valid: the exchange runs once per WINDOW of steps over every
 * neighbour the window's centres have; a step only looks rows up.  Nothing here is sized by the node-id space.
 *   bounds   int32 [world + 1]: rank r owns ids [bounds[r], bounds[r + 1])          (device)
 *   pos_ids / pos_idx  int32 [n_pos]: the train-pos ids ascending / their row in the replicated block   (device)
 *   table    uint32 [2 * table_slots], table_slots = pcg_halo_table_slots(halo_cap)
 *   counts   uint32 [131], zeroed ONCE by the caller; after a collect [0, world) = unique remote ids per owner, [128] =
 *            overflow bits (1: table full, 2: more unique remote ids than halo_cap / than an owner's pitch, 4: a lookup
 *            missed; STICKY across calls - the caller clears them after looking, so one look per epoch sees every step.
 *            Bit 1 must be CLEARED before the next pcg_halo_collect: while it is set the collect stops walking at once, so
 *            a window collected behind a table-full report - however small - comes out EMPTY: request list all -1, counts
 *            zero, every remote id a hole at look-up),
 *            [129] / [130] = the largest number of unique remote ids a window needed so far / needed from one owner
 *   uniq     int32 [halo_cap]: the request list - the unique remote ids grouped by owner in rank order; it doubles as the
 *            halo rows' id column (row halo_base + i holds node uniq[i], -1 = unused)
 *   owner_pitch  0: packed (owner o's ids start where owner o - 1's end; the all-to-all's split sizes are the counts)
 *                > 0 (halo_cap == max(world - 1, 1) * owner_pitch): the j-th OTHER rank's ids (ranks in order, self_rank left
 *                out) sit at [j * pitch, (j + 1) * pitch), unused entries are -1 - the all-to-alls' split sizes are known in
 *                advance, and no count has to reach the host before they are issued
 * pcg_halo_collect: reset (table, per-window counts, request list) + walk the CSR rows (all relations) of `centres` (local
 *   row numbers [n_centres], duplicates allowed) inserting their remote non-train-pos neighbours + assign slots / fill the
 *   request list (an id that does not fit gets no slot: the overflow bit).  Then all-to-all #1 (ids), pcg_halo_serve on the
 *   owner: out[i, :] = X[req[i] - lo, :] (whole padded rows; req[i] < 0 or not owned: row i untouched), all-to-all #2 (rows).
 * pcg_halo_lookup: per step - the list's global ids -> rows of the table: owned id -> id - lo; train-pos id -> n_local + its
 *   row; remote id -> halo_base + slot; an id the window did not collect becomes a hole (-1) and sets bit 4.
 * A rank then holds the feature row of every node its window can touch and scores them itself (pcg_step_front_a with
 * row_ids): the step needs no score exchange - its only collective is the gradient all-reduce. */
int64_t pcg_halo_table_slots(int32_t halo_cap);
int pcg_halo_collect(const pcg_graph_desc *g, const int32_t *centres, int32_t n_centres, int32_t lo, int32_t hi,
                     int32_t n_local, const int32_t *pos_ids, int32_t n_pos, const int32_t *bounds, int32_t world,
                     uint32_t *table, int64_t table_slots, uint32_t *counts, int32_t *uniq, int32_t halo_cap,
                     int32_t halo_base, int32_t owner_pitch, int32_t self_rank, void *stream);
int pcg_halo_serve(const pcg_graph_desc *g, const int32_t *req, int32_t n_req, int32_t lo, int32_t n_local, float *out,
                   int32_t out_stride, void *stream);
int pcg_halo_lookup(const pcg_graph_desc *g, int32_t B, void *workspace, const void *plan, int64_t list_capacity, int32_t lo, int32_t hi,
                    int32_t n_local, const int32_t *pos_ids, const int32_t *pos_idx, int32_t n_pos, uint32_t *table,
                    int64_t table_slots, uint32_t *counts, int32_t halo_cap, int32_t halo_base, void *stream);

/* gather rows: out[i, :feat_dim] = X[ids[i], :feat_dim]  (self_feats, layers.py:273-277) */
int pcg_gather_rows(const pcg_graph_desc *g, const int32_t *ids, int32_t n_ids,
                    float *out, int32_t out_stride, void *stream);

/* ---- evaluation counts ---------------------------------------------------------
 * Everything the reported metrics (src/utils.py:306-323, src/utils(f1).py:334-350) are functions of, as integers, from the
 * class probabilities of an evaluation pass, without leaving the device:
 *   prob [n, 2] f32 (sigmoid of the gnn logits), labels [n] i32 in {0, 1}, thresholds [n_thresholds] f64 ascending (device),
 *   n <= 2^31 - 1, 1 <= n_thresholds <= 1024;
 *   out [8 + 2 T] u64 = tp, fp, fn, tn (of the argmax prediction: 1 iff p1 > p0), n1, n0, 2U, 0, tp_t[T], npred_t[T]
 *   with tp_t = #{y = 1, (double)p1 > thresholds[t]}, npred_t = #{(double)p1 > thresholds[t]} and
 *   2U = sum over (positive i, negative j) of 2 [p1_i > p1_j] + [p1_i == p1_j]   (auc = (2U / 2) / (n1 n0), average ranks for ties;
 *   -0.0 == +0.0).
 * Launches: zero | count pass | finish | LSD radix sort of the smaller class's keys (one launch up to 65536 keys, three per
 * 8-bit pass above) | rank pass.  Integer sums only: the output is the same bits on every run.  workspace:
 * pcg_eval_workspace_bytes(n, n_thresholds) bytes, 256-byte aligned, contents irrelevant on entry (the call zeroes its counters
 * itself, on the stream: capturable).  A label outside {0, 1} (counted as 1) or a NaN probability sets PCG_ST_EVAL_INPUT in *status.
 * n == 0: out is all zeros. */
int64_t pcg_eval_workspace_bytes(int64_t n, int32_t n_thresholds);
int pcg_eval_counts(const float *prob, const int32_t *labels, int64_t n, const double *thresholds, int32_t n_thresholds,
                    void *workspace, uint64_t *out, uint32_t *status, void *stream);

/* ---- ranking counts and the alert list -----------------------------------------
 * What average precision, precision / recall at k and the top-k alert list are functions of, without leaving the device.
 * Throughout a row's key is p1 + 0.0f compared as a float (-0.0 ties with +0.0), p1 = prob[i, 1].
 *
 * pcg_pr_counts: prob [n, 2] f32, labels [n] i32 in {0, 1}, n <= 2^31 - 1, cap >= 0;
 *   hdr [8] u64 = tp, fp, fn, tn (of the argmax prediction: 1 iff p1 > p0), n1, n0, G, 0 - the first six are pcg_eval_counts';
 *   with u_1 > u_2 > ... > u_G the distinct values of p1 over the rows with y = 1 (the only points at which recall changes; G <= n1):
 *   tp_g [cap] u32 = #{y = 1, p1 >= u_g}, npred_g [cap] u32 = #{p1 >= u_g}; entries [0, min(G, cap)) are written, in descending
 *   score order.  G > cap: nothing is written past cap and PCG_ST_PR_OVERFLOW is set in *status (cap = n1 always suffices; cap = 0:
 *   tp_g / npred_g may be NULL, the header alone).
 * Launches: zero | count pass (confusion words, the positives' keys) | finish | LSD radix sort of the positives' keys (one workgroup
 * up to 65536 keys; for n above that also three launches per 8-bit pass, which return at once unless n1 is above it too) | bin pass
 * (every row: a binary search in the sorted keys, one integer add - in LDS per window of 16384 bins up to 524288 positives) | group heads: tile sums, their scan, the compaction (three).
 * Integer sums only: the output is the same bits on every run.  workspace: pcg_pr_workspace_bytes(n) bytes, 256-byte aligned,
 * contents irrelevant on entry (capturable).  A label outside {0, 1} (counted as 1) or a NaN probability sets PCG_ST_EVAL_INPUT in
 * *status.  n == 0: hdr is all zeros.  The float64 statements (average precision, G-mean) are the host's: pc-gnn_amd/utils.py.
 *
 * pcg_topk_alerts: the alert order is the stable sort of the rows by key, descending - among equal keys the lower position comes
 * first, so a tie at the cut is resolved by input position; the call returns its first min(k, n) positions.
 *   p1: f32, row i at p1[i * stride] (stride 2 with p1 = prob + 1 reads column 1 of [n, 2]; stride 1 a vector), stride >= 1;
 *   1 <= k <= PCG_ALERTS_MAX_K (else PCG_E_ARG), 0 <= n <= 2^31 - 1;
 *   out_pos [k] i32, out_score [k] f32 (p1 at that position, bit for bit) in alert order; slots at and beyond n hold -1 / -inf.
 * Launches: zero | four histogram passes of a radix select of the min(k, n)-th largest key (each picks the previous digit itself) |
 * per-tile counts of the rows above / equal to it | their scan | position-ordered scatter of every row above it and of the first
 * rows equal to it | a stable radix sort of the (key, position) pairs by one workgroup.  Integer sums only; the same bits on every
 * run.  workspace: pcg_topk_alerts_workspace_bytes(n, k) bytes, 256-byte aligned, contents irrelevant on entry (capturable).  A
 * NaN sets PCG_ST_EVAL_INPUT in *status (it is then ranked above +inf or below -inf by its sign bit). */
#define PCG_ALERTS_MAX_K 65536
int64_t pcg_pr_workspace_bytes(int64_t n);
int pcg_pr_counts(const float *prob, const int32_t *labels, int64_t n, int64_t cap, void *workspace, uint64_t *hdr, uint32_t *tp_g,
                  uint32_t *npred_g, uint32_t *status, void *stream);
int64_t pcg_topk_alerts_workspace_bytes(int64_t n, int32_t k);
int pcg_topk_alerts(const float *p1, int32_t stride, int64_t n, int32_t k, void *workspace, int32_t *out_pos, float *out_score,
                    uint32_t *status, void *stream);

/* ---- alert cases ------------------------------------------------------------------
 * The slots of a member list grouped into linked rings, without the list or the CSR leaving the device.
 *   members [m] i32 in alert order, 0 <= m <= PCG_ALERTS_MAX_K: a node id in [0, n_nodes) or -1 (padding: in no case); any other
 *   value sets PCG_ST_LIST_ID_RANGE and is treated as padding.  rel_mask: bit r selects relation r; non-zero, no bit at or
 *   above g->n_rel.  Slot p is linked to slot q != p when members[p] == members[q], or when for a selected relation r members[q]
 *   occurs in row r of members[p] or members[p] in row r of members[q] (an edge stored one way links; there is no 2-hop linking).
 *   A case is a connected component of the valid slots under "linked"; its head is its lowest slot; cases are numbered 0 .. C - 1 by
 *   ascending head.
 *   case_of [m] i32: the slot's case, -1 for padding | head [m] i32: entries [0, C) are written |
 *   offsets [m + 1] i32: entries [0, C] are written, offsets[C] = the number of valid slots | order [m] i32: entries
 *   [offsets[c], offsets[c + 1]) are case c's slots, ascending; the entries from offsets[C] on are the padding slots, ascending |
 *   links [m] i32: entries [0, C) = over the case's slots p and the selected relations, the CSR entries of members[p] whose target is a
 *   member node other than members[p] (directed entries: a symmetric edge counts twice, self-loops count zero); the rest 0 |
 *   hits [m] i32, with labels [m] i32 (one per slot; both or neither NULL): entries [0, C) = the case's slots with label 1; the rest 0.
 *   A label outside {0, 1} on a valid slot sets PCG_ST_EVAL_INPUT |
 *   hdr [4] i32 = C, the number of valid slots, *status as the call's last launch found it, 0.
 * Launches: three memsets (the header, the counters and the position map, 4 n_nodes bytes) | init | link (a wave per slot and relation; rows of
 * more than 512 entries are queued) | long rows (16 workgroups per queued row) | flatten | number (one workgroup) | assign |
 * pcg_topk_alerts over the case numbers (the stable order) | offsets and header (one workgroup).  Lock-free union-find whose root is
 * the component's lowest slot whatever order the unions land in; integer sums only: the same bits on every run.  Every retry loop is
 * bounded by m; one that runs out sets PCG_ST_SYNC_TIMEOUT.  A CSR entry outside [0, n_nodes) is skipped and sets
 * PCG_ST_LIST_ID_RANGE.  workspace: pcg_alert_cases_workspace_bytes(g->n_nodes, m) bytes, 256-byte aligned, contents irrelevant on
 * entry (capturable).  m == 0: C = 0, offsets[0] = 0 and the header are written, nothing else is read or written (members and the
 * other outputs may be NULL).  PCG_E_ARG before any launch: a NULL required pointer, m outside [0, PCG_ALERTS_MAX_K], an empty or
 * out-of-range rel_mask, labels without hits or hits without labels, a workspace too small or misaligned. */
int64_t pcg_alert_cases_workspace_bytes(int64_t n_nodes, int32_t m);
int pcg_alert_cases(const pcg_graph_desc *g, const int32_t *members, int32_t m, uint32_t rel_mask, const int32_t *labels, void *workspace,
                    int64_t workspace_bytes, int32_t *case_of, int32_t *head, int32_t *offsets, int32_t *order, int32_t *links,
                    int32_t *hits, int32_t *hdr, uint32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PCGNN_H */
