// Scoring nodes that are NOT in the resident graph (pcg_infer_new): a query batch of nq new nodes - a feature row each and, per
// relation, a neighbour list of global ids in [0, N + nq) (base nodes, other query nodes, the node itself) - against the base
// graph of N nodes, which is neither modified nor re-scored.
//
//   infer_new_front_kernel : [the base table's score pass (score_table_body over g->X: pcg_score_table's workgroups, rows and fma
//                            order) - only when the caller's s0[0, N) is not current] || the query rows' scores -> s0[N, N + nq)
//                            || the look-back words of the call's two plan slots zeroed
//   per chunk of ids       : plan (test mode, over the QUERY's CSR) -> select (centre score s0[ids[b] + N]; lists of global ids:
//                            ChunkDriver::run, infer.h) -> two-table gather (gather.hip: id < N reads g->X, id >= N reads q->X) -> infer_dense_kernel with
//                            the self rows from q->X
//
// PC-GNN here is one layer and test mode makes no minority picks: a node's logits are a function of its own feature row, its own
// neighbour lists, the class-0 scores and feature rows of those neighbours, and the parameters.  A score is the row's own
// arithmetic (its lanes, fma chain and butterfly - whichever table, workgroup or launch the row is in), a selection list, its
// gather chunks and the dense sums are laid out per row, and the table select changes addresses only.  So every logit is bit for
// bit what pcg_infer_set writes for node N + q on a graph built with the query rows appended.
#include "infer.h"

namespace pcg {

// workgroups [0, n_base) score the base table (n_base == 0: the caller's scores are current), [n_base, n_base + n_query) the
// query rows into s0 + n_base_rows, the rest zero.  n_base = score_table_blocks(n_base_rows): pcg_score_table's grid.
__global__ void __launch_bounds__(256) infer_new_front_kernel(const float *__restrict__ X, int64_t n_base_rows,
                                                              const float *__restrict__ Xq, int64_t n_query_rows, int feat_dim,
                                                              int stride, const float *__restrict__ W,
                                                              const float *__restrict__ bias, float *__restrict__ s0, int n_base,
                                                              int n_query, const ZeroRegions z) {
    int b = (int)blockIdx.x;
    if (b < n_base) {
        score_table_body(X, feat_dim, stride, W, bias, 0, n_base_rows, s0, b, n_base);
        return;
    }
    b -= n_base;
    if (b < n_query) {
        score_table_body(Xq, feat_dim, stride, W, bias, 0, n_query_rows, s0 + n_base_rows, b, n_query);
        return;
    }
    infer_zero_body(z, b - n_query);
}

// what the query entry points check before anything else: the two descriptors describe tables of one shape (infer.h)
int infer_new_descs(const pcg_graph_desc *g, const pcg_graph_desc *q) {
    if (!g || !q) return PCG_E_ARG;
    if (q->feat_dim != g->feat_dim || q->feat_stride != g->feat_stride || q->n_rel != g->n_rel) return PCG_E_ARG;
    if (g->n_nodes < 1 || q->n_nodes < 0 || q->n_pos != 0 || g->n_nodes + q->n_nodes >= (1ll << 31)) return PCG_E_ARG;
    return PCG_OK;
}

// the front launch of a query call (infer.h): d is the call's driver over q
int launch_infer_new_front(const pcg_graph_desc *g, const pcg_graph_desc *q, const float *theta, int32_t emb, float *s0,
                           int32_t score_base, const ChunkDriver &d) {
    const int F = g->feat_dim, E = emb, R = g->n_rel;
    const int64_t N = g->n_nodes, nq = q->n_nodes;
    ZeroRegions z = {};
    infer_zero_regions(z, d);
    const int n_zero = infer_zero_blocks(z);
    const int n_base = score_base ? (int)score_table_blocks(N, g->feat_stride) : 0;
    const int n_query = (int)score_table_blocks(nq, g->feat_stride);
    hipLaunchKernelGGL(infer_new_front_kernel, dim3(n_base + n_query + n_zero), dim3(256), 0, d.st, g->X, N, q->X, nq, F,
                       g->feat_stride, theta + off_clf(F, E, R), theta + off_bias(F, E, R), s0, n_base, n_query, z);
    PCG_LAUNCH_CHECK();
    return PCG_OK;
}

}  // namespace pcg

extern "C" {

int64_t pcg_infer_new_workspace_bytes(const pcg_graph_desc *g, const pcg_graph_desc *q, int32_t emb, int32_t chunk_rows,
                                      int64_t list_capacity) {
    int rc = pcg::infer_new_descs(g, q);
    if (rc != PCG_OK) return rc;
    // plan, select, gather and dense all work on the QUERY's rows: the layout is pcg_infer_set's for that descriptor
    pcg::InferCarve c;
    rc = pcg::infer_carve(q, 2, true, emb, chunk_rows, list_capacity, c);
    return rc != PCG_OK ? rc : c.total;
}

// pcg_infer_new (out_emb, out_rel NULL) and pcg_embed_new: a NULL out_logits / out_center goes to the workspace's centre scratch
static int infer_new_impl(const pcg_graph_desc *g, const pcg_graph_desc *q, const float *theta, int32_t emb, const int32_t *ids,
                          int32_t n, int32_t chunk_rows, float *s0, int32_t score_base, const double *thresholds, void *workspace,
                          int64_t list_capacity, float *out_logits, float *out_center, float *out_emb, float *out_rel,
                          bool need_logits, uint32_t *status, void *stream) {
    int rc = pcg::infer_new_descs(g, q);
    if (rc != PCG_OK) return rc;
    if (n < 0) return PCG_E_ARG;
    if (!need_logits && !out_logits && !out_center && !out_emb && !out_rel) return PCG_E_ARG;
    if (!pcg::infer_table_ok(g)) return PCG_E_UNSUPPORTED;
    pcg::InferCarve c;
    rc = pcg::infer_carve(q, 2, true, emb, chunk_rows, list_capacity, c);
    if (rc != PCG_OK) return rc;
    const int F = g->feat_dim, E = emb, R = g->n_rel;
    if (pcg::dense_smem_bytes(F, E, R, pcg::infer_wlds(F, E, R)) > 160 * 1024) return PCG_E_UNSUPPORTED;
    if (n == 0 || q->n_nodes == 0) return PCG_OK;
    if (!g->X || !q->X || !theta || !ids || !s0 || !thresholds || !workspace || (need_logits && !out_logits) || !status) return PCG_E_ARG;
    if (((reinterpret_cast<uintptr_t>(g->X) | reinterpret_cast<uintptr_t>(q->X)) & 15u) != 0) return PCG_E_ARG;
    const int64_t N = g->n_nodes, nq = q->n_nodes;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    float *agg = reinterpret_cast<float *>(ws + c.agg), *center_scratch = reinterpret_cast<float *>(ws + c.center);
    // the rows are the query's, the scores are indexed by global id (centre b: s0[ids[b] + N])
    const pcg::ChunkDriver d = pcg::infer_driver(q, ids, n, chunk_rows, list_capacity, thresholds, s0, N, 2, workspace, c, status, stream);

    // the front: [base scores] || query scores || the look-back words of both plan slots (as pcg_infer_set zeroes them)
    rc = pcg::launch_infer_new_front(g, q, theta, emb, s0, score_base, d);
    if (rc != PCG_OK) return rc;

    return d.run([&](int64_t off, int32_t B, const int32_t *cid, const pcg::Workspace &w) {
        const int rc = pcg::launch_gather_two(pcg::feat_table(g), q->X, nq, {agg, F, PCG_NORM_COUNT, d.cnt, status}, R * B, w, d.st);
        if (rc != PCG_OK) return rc;
        // dense: the centres are rows of the query table
        return pcg::infer_dense(q, theta, emb, cid, B, w, agg, d.cnt, out_logits ? out_logits + 2 * off : center_scratch,
                                out_center ? out_center + 2 * off : center_scratch, d.st,
                                out_emb ? out_emb + (int64_t)E * off : nullptr, out_rel ? out_rel + (int64_t)R * E * off : nullptr);
    });
}

int pcg_infer_new(const pcg_graph_desc *g, const pcg_graph_desc *q, const float *theta, int32_t emb, const int32_t *ids, int32_t n,
                  int32_t chunk_rows, float *s0, int32_t score_base, const double *thresholds, void *workspace,
                  int64_t list_capacity, float *out_logits, float *out_center, uint32_t *status, void *stream) {
    return infer_new_impl(g, q, theta, emb, ids, n, chunk_rows, s0, score_base, thresholds, workspace, list_capacity, out_logits,
                          out_center, nullptr, nullptr, true, status, stream);
}

int pcg_embed_new(const pcg_graph_desc *g, const pcg_graph_desc *q, const float *theta, int32_t emb, const int32_t *ids, int32_t n,
                  int32_t chunk_rows, float *s0, int32_t score_base, const double *thresholds, void *workspace,
                  int64_t list_capacity, float *out_logits, float *out_center, float *out_emb, float *out_rel, uint32_t *status,
                  void *stream) {
    return infer_new_impl(g, q, theta, emb, ids, n, chunk_rows, s0, score_base, thresholds, workspace, list_capacity, out_logits,
                          out_center, out_emb, out_rel, false, status, stream);
}

}  // extern "C"
