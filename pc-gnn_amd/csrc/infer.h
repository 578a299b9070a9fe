// Shared between the whole-set entry points (infer.hip, infer_new.hip, rank.hip, attr.hip, explain_new.hip): the zeroing workgroups of a front kernel, the
// call's workspace layout, the per-chunk plan -> select -> stage loop and the forward-only dense launch.
#pragma once
#include "dense.h"

namespace pcg {

struct ZeroRegions {          // up to four runs of 32-bit words to zero
    uint32_t *p[4];
    int64_t n[4];
};
constexpr int INFER_ZERO_WORDS = 256 * 16;   // words per zeroing workgroup

// zeroing workgroup `b` (256 threads) of a front kernel: words [b * INFER_ZERO_WORDS, + INFER_ZERO_WORDS) of the concatenated regions
__device__ __forceinline__ void infer_zero_body(const ZeroRegions &z, int b) {
    const int64_t w0 = (int64_t)b * INFER_ZERO_WORDS;
    for (int64_t i = w0 + threadIdx.x; i < w0 + INFER_ZERO_WORDS; i += blockDim.x) {
        int64_t j = i;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (j >= 0 && j < z.n[k]) z.p[k][j] = 0u;
            j -= z.n[k];
        }
    }
}

// a call's workspace: [plan slot of full chunks | plan slot of the last, shorter chunk (n_slots == 2: the single-GPU calls; the
// partitioned chunk has one slot) | data part | dense parts: agg [R][chunk][F] | cnt [R][chunk] | dense parts: centre logits
// [chunk][2] (for a caller who wants none)].  A chunk of fewer rows carves its own layout inside the same bytes (every part grows
// with the rows).  Without the dense parts (pcg_chosen_set) agg and center are -1 and emb is not looked at.
struct InferCarve {
    int64_t plan_bytes, data, agg, cnt, center, total;
};
// infer.hip
int infer_carve(const pcg_graph_desc *g, int n_slots, bool dense, int32_t emb, int32_t chunk_rows, int64_t list_capacity, InferCarve &c);
bool infer_wlds(int F, int E, int R);
int launch_infer_dense(const DenseArgs &a, int B, hipStream_t st, float *h_out = nullptr);
// the forward-only dense launch of a chunk whose lists were gathered into agg ([R][B][F]; rows of several chunks: partial sums in
// w): centres `nodes` are rows of g's table -> out_logits, out_center [B][2]; out_emb [B][emb] (`combined`) and out_rel
// [B][n_rel * emb] (h_1 | .. | h_R) where not NULL (pcg_embed_set, pcg_embed_new)
int infer_dense(const pcg_graph_desc *g, const float *theta, int32_t emb, const int32_t *nodes, int32_t B, const Workspace &w,
                float *agg, const int32_t *cnt, float *out_logits, float *out_center, hipStream_t st, float *out_emb = nullptr,
                float *out_rel = nullptr);
// the zeroing workgroups a front kernel needs for z
inline int infer_zero_blocks(const ZeroRegions &z) {
    return (int)((z.n[0] + z.n[1] + z.n[2] + z.n[3] + INFER_ZERO_WORDS - 1) / INFER_ZERO_WORDS);
}
// the front launch of a whole-set call: the table's scores with (W, bias) || the words of z zeroed
int launch_infer_front(const pcg_graph_desc *g, const float *W, const float *bias, float *s0, const ZeroRegions &z, hipStream_t st);
// the feature tables every whole-set call reads: rows of 16-byte groups that one score workgroup's lanes cover
inline bool infer_table_ok(const pcg_graph_desc *g) {
    return g->feat_dim >= 1 && g->feat_stride >= g->feat_dim && g->feat_stride % 4 == 0 && g->feat_stride <= 512;
}

// The chunks of a whole-set call: ids [ch * chunk_rows, + chunk_rows) of n, the last one `tail` rows.  Full chunks plan into slot
// 0, a shorter last chunk into slot 1 (a tail equal to the chunk is a full chunk); the data part, cnt and the status word are
// shared.  The front launch of the call zeroes what infer_zero_regions names: the look-back words (counters, queue heads,
// per-workgroup totals) of every slot as the layouts of the call's chunk sizes place them.  A slot's earlier plans may have laid
// other arrays over those words: zeroed, none of them can pass for a published total (the tags the plan launches count from the
// zeroed sequence word start at 1).
struct ChunkDriver {
    const pcg_graph_desc *g;      // the graph whose rows are planned and selected
    const int32_t *ids;
    int32_t n, chunk_rows;
    int64_t list_capacity;
    const double *thresholds;
    const float *s0;
    int64_t center_off;           // centre b's score is s0[ids[b] + center_off]
    int n_slots;
    unsigned char *slot[2];
    int64_t plan_bytes;
    unsigned char *data;
    int32_t *cnt;
    uint32_t *status;
    hipStream_t st;

    int n_chunks() const { return (int)(((int64_t)n + chunk_rows - 1) / chunk_rows); }
    int32_t tail() const { return n - (n_chunks() - 1) * chunk_rows; }
    // per chunk: plan (test mode) -> select -> stage(off, B, cid, w): the chunk is ids [off, off + B) = cid[0, B), its lists and
    // plan are in w
    template <class Stage>
    int run(Stage &&stage) const {
        const int nc = n_chunks();
        const int32_t last = tail();
        for (int ch = 0; ch < nc; ++ch) {
            const int64_t off = (int64_t)ch * chunk_rows;
            const int32_t B = ch + 1 < nc ? chunk_rows : last;
            unsigned char *plan = slot[B == chunk_rows ? 0 : 1];
            const int32_t *cid = ids + off;
            int rc = pcg_plan_epochs(g, cid, nullptr, B, 1, B, thresholds, nullptr, 0, 0, plan, plan_bytes, list_capacity, status,
                                     nullptr, st);
            if (rc != PCG_OK) return rc;
            rc = pcg_choose_select_planned(g, cid, nullptr, B, s0, nullptr, nullptr, thresholds, nullptr, 0, 0, cnt, data, plan,
                                           list_capacity, status, nullptr, center_off, st);
            if (rc != PCG_OK) return rc;
            Workspace w;
            carve1(g, B, list_capacity, data, &w, plan);
            rc = stage(off, B, cid, w);
            if (rc != PCG_OK) return rc;
        }
        return PCG_OK;
    }
};
// the look-back words of d's n_slots plan slots (see ChunkDriver)
void infer_zero_regions(ZeroRegions &z, const ChunkDriver &d);
// the driver of a call whose workspace was carved as c (n_slots as given to infer_carve)
ChunkDriver infer_driver(const pcg_graph_desc *g, const int32_t *ids, int32_t n, int32_t chunk_rows, int64_t list_capacity,
                         const double *thresholds, const float *s0, int64_t center_off, int n_slots, void *workspace,
                         const InferCarve &c, uint32_t *status, void *stream);


// ---- query batches (pcg_infer_new, pcg_explain_new): rows of a query table q behind the base table g ---------------------------
// infer_new.hip: the two descriptors describe tables of one shape (else PCG_E_ARG)
int infer_new_descs(const pcg_graph_desc *g, const pcg_graph_desc *q);
// infer_new.hip: the front launch of a query call whose driver (over q, center_off = g->n_nodes, two slots) is d: [the base
// table's scores -> s0[0, N), only when score_base] || the query rows' scores -> s0[N, N + nq) || d's look-back words zeroed
int launch_infer_new_front(const pcg_graph_desc *g, const pcg_graph_desc *q, const float *theta, int32_t emb, float *s0,
                           int32_t score_base, const ChunkDriver &d);
// gather.hip: lists of ids in [0, t.rows + query_rows): id < t.rows -> row id of t.X, else row id - t.rows of query_X
int launch_gather_two(const FeatTable &t, const float *query_X, int64_t query_rows, const GatherOut &out, int32_t n_rows,
                      const Workspace &w, hipStream_t st);

// rank.hip: the two rank launches over the lists (and the plan) in `w` - rows (r, b), b < B, of a chunk that is ids
// [b_off, b_off + B) of the call's n_total, written at out_begin[r * n_total + b_off + b].  g: the graph whose rows were planned
// and selected; s0 [n_scores] by list id; centre b's score center_s0 ? center_s0[b] : s0[nodes[b] + center_off]
int launch_rank_lists(const pcg_graph_desc *g, const int32_t *nodes, int32_t B, int64_t n_total, int64_t b_off, const float *s0,
                      const float *center_s0, const Workspace &w, const int64_t *out_begin, int32_t *out_ids, float *out_dist,
                      uint32_t *status, int64_t center_off, int64_t n_scores, hipStream_t st);

}  // namespace pcg
