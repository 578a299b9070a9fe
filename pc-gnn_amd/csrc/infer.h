// Shared between the whole-set inference entry points (infer.hip) and the query-batch path (infer_new.hip): the zeroing
// workgroups of a front kernel, the call's workspace layout and the forward-only dense launch.
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

// the call's workspace: [plan slot of full chunks | plan slot of the last, shorter chunk | data part | agg [R][chunk][F] |
// cnt [R][chunk] | centre logits [chunk][2] (when the caller wants none)]
struct InferCarve {
    int64_t plan_bytes, data, agg, cnt, center, total;
};
// infer.hip
int infer_carve(const pcg_graph_desc *g, int32_t emb, int32_t chunk_rows, int64_t list_capacity, InferCarve &c);
bool infer_wlds(int F, int E, int R);
int launch_infer_dense(const DenseArgs &a, int B, hipStream_t st);
// the front launch of a whole-set call: the table's scores with (W, bias) || the words of z zeroed
int launch_infer_front(const pcg_graph_desc *g, const float *W, const float *bias, float *s0, const ZeroRegions &z, hipStream_t st);
// the look-back words of a call's two plan slots (full chunks | the shorter last chunk) as the layouts of its chunk sizes place them
void infer_zero_regions(ZeroRegions &z, const pcg_graph_desc *g, int32_t chunk_rows, int32_t tail, int64_t list_capacity,
                        unsigned char *slot0, unsigned char *slot1, unsigned char *data);

}  // namespace pcg
