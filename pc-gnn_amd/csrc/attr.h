// The attribution launches of attr.hip, for the entry points outside it (explain_new.hip).
#pragma once
#include "infer.h"

namespace pcg {

// the backward's LDS beyond the forward's fits a workgroup (else PCG_E_UNSUPPORTED)
bool attr_shape_ok(int F, int E, int R);

// The attribution dense launch of a chunk whose lists were gathered into agg ([R][B][F]; rows of several chunks: partial sums in
// w): the chunk is ids [off, off + B) = cid[0, B) of the call's n, rows of g's table (the self rows are read from g->X).
// out_logits [n][2], out_d_self [n][F], out_d_agg [R][n][F], out_self_contrib [n], out_rel_contrib [R][n]: the call's arrays,
// the chunk writes its rows; center_scratch [B][2].
int attr_chunk(const pcg_graph_desc *g, const float *theta, int32_t emb, const int32_t *cid, int32_t B, const Workspace &w, float *agg,
               const int32_t *cnt, int64_t off, int32_t n, float w0, float w1, float *out_logits, float *center_scratch,
               float *out_d_self, float *out_d_agg, float *out_self_contrib, float *out_rel_contrib, hipStream_t st);

// The gather-dot over `rows` ranked rows: out[e] = <row ids[e], d_agg[row]> / row length.  query_X == NULL: every id names a row of
// X [base_rows]; else id < base_rows reads row id of X and id >= base_rows row id - base_rows of query_X [query_rows] (both
// [.., feat_stride], 16-byte aligned).  An id outside [0, base_rows + query_rows) is clamped for the read and sets
// PCG_ST_LIST_ID_RANGE.  max_degree: the longest row there can be (it sizes the tail slices; the bits do not depend on it).
int launch_attr_neigh(const float *X, int64_t base_rows, const float *query_X, int64_t query_rows, int32_t feat_dim,
                      int32_t feat_stride, int32_t max_degree, const int64_t *flat_offsets, const int32_t *ids, int64_t rows,
                      const float *d_agg, float *out, uint32_t *status, hipStream_t st);

}  // namespace pcg
