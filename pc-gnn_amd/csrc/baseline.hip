// Whole-set inference for the GraphSAGE / GCN baselines (src/graphsage.py:62-96, 127-150, 167-174, 200-232, 262-275) on gfx950:
// logits (and embeddings, aggregates) of any node set in large chunks, with no plan, no selection and no per-edge list.
//
//   per chunk: counter = 0  ->  baseline_agg_rows_kernel  ->  baseline_agg_long_kernel  ->  baseline_dense_kernel
//
//   baseline_agg_rows_kernel : one wave per centre, grid-stride.  The centre's neighbourhood is its CSR row, read in place
//                              (g->indices[rel] + g->indptr[rel][v]); with add_self the centre itself is united with it.  A row of
//                              more than BL_ROW_MAX neighbours is not summed here: its chunk position goes into a queue.
//   baseline_agg_long_kernel : a fixed grid of BL_LONG_WAVES-wave workgroups strides over the queue, one workgroup per long row.
//   baseline_dense_kernel    : 16-centre tiles, z = [self | a] or a, h = relu(W_enc z) with v_mfma_f32_16x16x4_f32 (exact float32),
//                              logits = W_cls h.  W_enc is staged in LDS once per workgroup when it fits beside the tile, else it
//                              streams from L2 as the B operand.  Workgroups stride over the tiles: no queue, no atomics.
//
// A row's values are a function of the row alone.  The strategy is picked by the row's CSR degree; within a strategy group q of
// Q (Q lanes-per-row groups of the wave, or of the workgroup's waves) adds the neighbours q, q + Q, ... in that order, the groups
// are added by a butterfly (wave) and in wave order through LDS (workgroup), the united centre comes last, one float32 division
// per element finishes it.  The dense sums are MFMA chains in k order, K-split parts added in part order.  No float atomics and
// no waits between workgroups; the only atomics are the queue's integer counter and the status word.
// A row without neighbours (degree 0, no union) is 0 / 0 = NaN like the reference's; the ReLU lets NaN through.
#include "baseline.h"

namespace pcg {

template <bool WLDS>
__global__ void __launch_bounds__(BL_DENSE_THREADS) baseline_dense_kernel(const BaselineDense a, int n_tiles) {
    extern __shared__ __align__(16) float sm[];
    const BaselineLds s = baseline_lds(sm, a.feat_dim, a.emb, a.concat_self);
    baseline_stage_weights<WLDS>(a, s);
    for (int tile = (int)blockIdx.x; tile < n_tiles; tile += (int)gridDim.x) {
        const int64_t b = (int64_t)tile * TB + (threadIdx.x >> 4);
        float logit0, logit1;
        baseline_tile_forward<WLDS>(a, s, (int64_t)tile * TB, logit0, logit1);
        if ((threadIdx.x & 15) == 0 && b < a.B) {
            a.logits[2 * b] = logit0;
            a.logits[2 * b + 1] = logit1;
        }
    }
}

template <bool WLDS>
static int launch_baseline_dense(const BaselineDense &a, size_t smem, hipStream_t st) {
    if (allow_dynamic_lds(baseline_dense_kernel<WLDS>, 160 * 1024) != PCG_OK) return PCG_E_LAUNCH;
    const int n_tiles = (int)(((int64_t)a.B + TB - 1) / TB);
    hipLaunchKernelGGL(baseline_dense_kernel<WLDS>, dim3(baseline_dense_grid(n_tiles, smem)), dim3(BL_DENSE_THREADS), smem, st, a, n_tiles);
    PCG_LAUNCH_CHECK();
    return PCG_OK;
}

}  // namespace pcg

extern "C" {

int64_t pcg_baseline_workspace_bytes(const pcg_graph_desc *g, const pcg_baseline_model *m, int32_t chunk_rows) {
    pcg::BaselineCarve c;
    const int rc = pcg::baseline_carve(g, m, chunk_rows, c);
    return rc != PCG_OK ? rc : c.total;
}

int pcg_baseline_infer(const pcg_graph_desc *g, const pcg_baseline_model *m, const int32_t *ids, int32_t n, int32_t chunk_rows,
                       void *workspace, int64_t workspace_bytes, float *out_logits, float *out_emb, float *out_agg, uint32_t *status,
                       void *stream) {
    if (!ids || !workspace || !status || !out_logits || n < 0 || chunk_rows < 1 || !pcg::baseline_args_ok(g, m)) return PCG_E_ARG;
    pcg::BaselineCarve c;
    const int rc = pcg::baseline_carve(g, m, chunk_rows, c);
    if (rc != PCG_OK) return rc;
    const int F = g->feat_dim, E = m->emb, concat = m->concat_self != 0;
    const bool wlds = pcg::baseline_wlds(F, E, concat);
    const size_t smem = pcg::baseline_smem_bytes(F, E, concat, wlds);
    if (smem > 160 * 1024) return PCG_E_UNSUPPORTED;
    if (workspace_bytes < c.total || (reinterpret_cast<uintptr_t>(workspace) & 15u) != 0) return PCG_E_ARG;
    if (n == 0) return PCG_OK;

    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    pcg::BaselineAgg a;
    pcg::BaselineDense d;
    pcg::baseline_fill(g, m, reinterpret_cast<float *>(ws + c.agg), reinterpret_cast<int32_t *>(ws + c.queue),
                       reinterpret_cast<uint32_t *>(ws + c.counter), status, a, d);
    for (int64_t off = 0; off < n; off += chunk_rows) {
        const int32_t B = (int32_t)(n - off < chunk_rows ? n - off : chunk_rows);
        a.ids = d.ids = ids + off;
        a.B = d.B = B;
        a.out_agg = out_agg ? out_agg + off * F : nullptr;
        d.logits = out_logits + 2 * off;
        d.out_emb = out_emb ? out_emb + off * E : nullptr;
        const int rc1 = pcg::launch_baseline_agg(a, st);
        if (rc1 != PCG_OK) return rc1;
        const int rc2 = wlds ? pcg::launch_baseline_dense<true>(d, smem, st) : pcg::launch_baseline_dense<false>(d, smem, st);
        if (rc2 != PCG_OK) return rc2;
    }
    return PCG_OK;
}

}  // extern "C"
