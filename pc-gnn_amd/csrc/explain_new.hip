// Explaining nodes that are NOT in the resident graph (pcg_explain_new): the chosen neighbours of a query batch's rows, ranked,
// with their distances (pcg_chosen_set's output) and the exact input attributions of their gnn logits (pcg_attr_set's and
// pcg_attr_neighbours' output) - from ONE selection per chunk, against the base graph, which is neither modified nor re-scored.
//
//   front (infer_new.hip)  : [the base table's score pass - only when the caller's s0[0, N) is not current] || the query rows'
//                            scores -> s0[N, N + nq) || the look-back words of the call's two plan slots zeroed
//   per chunk of ids       : plan (test mode, over the QUERY's CSR) -> select (centre score s0[ids[b] + N]; lists of global ids:
//                            ChunkDriver::run, infer.h)
//                            -> [chosen group] the two rank launches (rank.hip: centre score s0[ids[b] + N], list scores s0[id])
//                            -> [attribution group] two-table gather (gather.hip) -> attr_dense_kernel with the self rows from
//                               q->X (attr.hip)
//   after the last chunk   : [neigh_contrib] one two-table gather-dot over all ranked rows (attr.hip)
// This file adds no kernel: every launch is one an entry point for resident nodes makes, on other addresses.
//
// A score is the row's own arithmetic, a selection list, its rank keys, its gather chunks, the dense sums, the backward and an
// entry's dot product are laid out per row (or per entry), and choosing the table a row is read from changes an address - not a
// value, not an order.  So every output is bit for bit what pcg_chosen_set, pcg_attr_set and pcg_attr_neighbours write for node
// N + q on a graph built with the query rows appended.
#include "attr.h"

extern "C" {

int64_t pcg_explain_new_workspace_bytes(const pcg_graph_desc *g, const pcg_graph_desc *q, int32_t emb, int32_t chunk_rows,
                                        int64_t list_capacity) {
    int rc = pcg::infer_new_descs(g, q);
    if (rc != PCG_OK) return rc;
    // pcg_infer_new's carve of the query descriptor: two plan slots, the data part and the dense parts
    pcg::InferCarve c;
    rc = pcg::infer_carve(q, 2, true, emb, chunk_rows, list_capacity, c);
    return rc != PCG_OK ? rc : c.total;
}

int pcg_explain_new(const pcg_graph_desc *g, const pcg_graph_desc *q, const float *theta, int32_t emb, const int32_t *ids, int32_t n,
                    int32_t chunk_rows, float *s0, int32_t score_base, const double *thresholds, void *workspace,
                    int64_t list_capacity, float w0, float w1, const pcg_explain_out *out, uint32_t *status, void *stream) {
    int rc = pcg::infer_new_descs(g, q);
    if (rc != PCG_OK) return rc;
    if (n < 0 || !out) return PCG_E_ARG;
    // the output groups: each all or nothing, at least one, neigh_contrib only beside both others
    const int n_attr = !!out->logits + !!out->d_self + !!out->d_agg + !!out->self_contrib + !!out->rel_contrib;
    const int n_chosen = !!out->out_begin + !!out->out_ids + !!out->out_dist;
    if ((n_attr != 0 && n_attr != 5) || (n_chosen != 0 && n_chosen != 3)) return PCG_E_ARG;
    const bool want_attr = n_attr == 5, want_chosen = n_chosen == 3, want_neigh = out->neigh_contrib != nullptr;
    if ((!want_attr && !want_chosen) || (want_neigh && !(want_attr && want_chosen))) return PCG_E_ARG;
    if (!(w0 - w0 == 0.f) || !(w1 - w1 == 0.f)) return PCG_E_ARG;                    // (finite)
    if (!pcg::infer_table_ok(g)) return PCG_E_UNSUPPORTED;
    pcg::InferCarve c;
    rc = pcg::infer_carve(q, 2, true, emb, chunk_rows, list_capacity, c);
    if (rc != PCG_OK) return rc;
    const int F = g->feat_dim, E = emb, R = g->n_rel;
    if (!pcg::attr_shape_ok(F, E, R)) return PCG_E_UNSUPPORTED;
    if (n == 0 || q->n_nodes == 0) return PCG_OK;
    if (!g->X || !q->X || !theta || !ids || !s0 || !thresholds || !workspace || !status) return PCG_E_ARG;
    if (((reinterpret_cast<uintptr_t>(g->X) | reinterpret_cast<uintptr_t>(q->X)) & 15u) != 0) return PCG_E_ARG;
    const int64_t N = g->n_nodes, nq = q->n_nodes;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    float *agg = reinterpret_cast<float *>(ws + c.agg), *center_scratch = reinterpret_cast<float *>(ws + c.center);
    // the rows are the query's, the scores are indexed by global id (centre b: s0[ids[b] + N])
    const pcg::ChunkDriver d = pcg::infer_driver(q, ids, n, chunk_rows, list_capacity, thresholds, s0, N, 2, workspace, c, status, stream);

    rc = pcg::launch_infer_new_front(g, q, theta, emb, s0, score_base, d);
    if (rc != PCG_OK) return rc;
    rc = d.run([&](int64_t off, int32_t B, const int32_t *cid, const pcg::Workspace &w) {
        int rc = PCG_OK;
        if (want_chosen) {         // directly behind the select, as pcg_chosen_set places them (the lists and the plan are only read)
            rc = pcg::launch_rank_lists(q, cid, B, n, off, s0, nullptr, w, out->out_begin, out->out_ids, out->out_dist, status, N,
                                        N + nq, d.st);
            if (rc != PCG_OK) return rc;
        }
        if (want_attr) {
            rc = pcg::launch_gather_two(pcg::feat_table(g), q->X, nq, {agg, F, PCG_NORM_COUNT, d.cnt, status}, R * B, w, d.st);
            if (rc != PCG_OK) return rc;
            // dense: the centres are rows of the query table
            rc = pcg::attr_chunk(q, theta, emb, cid, B, w, agg, d.cnt, off, n, w0, w1, out->logits, center_scratch, out->d_self,
                                 out->d_agg, out->self_contrib, out->rel_contrib, d.st);
        }
        return rc;
    });
    if (rc != PCG_OK || !want_neigh) return rc;
    return pcg::launch_attr_neigh(g->X, N, q->X, nq, F, g->feat_stride, q->max_degree, out->out_begin, out->out_ids, (int64_t)R * n,
                                  out->d_agg, out->neigh_contrib, status, d.st);
}

}  // extern "C"
