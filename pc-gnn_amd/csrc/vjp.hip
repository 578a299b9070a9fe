// The dense tail's backward from CALLER-SUPPLIED loss gradients (custom losses on the fused path): pcg_dense_vjp.
//
//   dense_vjp : the acts-mode dense launch (dense.hip, pcg_train_dense(adam_clf = 4)) with dense_tile_body's EXT flag - one
//               1024-thread workgroup per tile of 16 batch rows runs the forward for its rows, takes the rows' seeds
//               d loss / d gnn logits and d loss / d label-aware logits from the caller instead of from the two cross-entropy
//               terms, and leaves the transposed activations / activation gradients in `acts` (wgrad.h) - what pcg_wgrad turns
//               into every weight gradient, the label classifier's included.  No slabs, no ticket / staged / pending words, no
//               classifier Adam, no sort rider; the step counter is not touched.
//
// Nothing behind the loss phase of the body depends on the loss: dcomb, dh_r and the stored activations are functions of the
// two seed arrays and the forward's LDS state alone.  The selection is not differentiated (nor does the reference: it is
// index-only), so with the seeds supplied the fused path is a differentiable function of the parameters.
//
// Reference lines replaced: loss.backward() of src/model_handler.py:149-153 for any loss of (gnn logits, label-aware logits, labels).
#include "dense.h"

namespace pcg {

template <bool WLDS, int F_, int E_, int R_>
__global__ void __launch_bounds__(DENSE_THREADS) dense_vjp_kernel(const DenseArgs a, const float *__restrict__ d_logits,
                                                                  const float *__restrict__ d_center) {
    extern __shared__ __align__(16) float sm[];
    dense_tile_body<WLDS, F_, E_, R_, false, true, true>(a, (int)blockIdx.x, sm, d_logits, d_center);
}

}  // namespace pcg

extern "C" int pcg_dense_vjp(const pcg_graph_desc *g, const pcg_train_state *st, const pcg_batch *batch, const float *agg,
                             int32_t agg_stride, const pcg_select_ws *sel, const float *d_logits, const float *d_center,
                             const pcg_dense_out *out, void *stream) {
    using namespace pcg;
    if (!g || !st || !batch || !sel || !d_logits || !d_center || batch->B < 0) return PCG_E_ARG;
    if (!st->theta || !st->acts) return PCG_E_ARG;
    const int32_t B = batch->B;
    if (B == 0) return PCG_OK;
    if (!batch->ids) return PCG_E_ARG;
    DenseExtra x;
    if (sel->workspace) {
        if (!batch->cnt || sel->list_capacity < 1) return PCG_E_ARG;
        Workspace w;
        carve1(g, B, sel->list_capacity, static_cast<unsigned char *>(sel->workspace), &w,
               static_cast<unsigned char *>(const_cast<void *>(batch->plan)));
        x.chunk_begin = w.chunk_begin;
        x.partial = w.partial;
        x.cnt = batch->cnt;
        x.partial_stride = g->feat_stride;
    }
    x.acts = st->acts;
    x.act_ld = st->act_ld;
    DenseArgs a;
    int n_sort_blocks = 0;
    // the argument block of pcg_train_dense(adam_clf = 4), with its checks.  dense_args insists on labels and on both logit
    // outputs; the seeded body reads no label and stores logits only where asked: placeholders in, the caller's pointers after
    float *const hold = const_cast<float *>(agg);
    const int rc = dense_args(a, n_sort_blocks, g, st->theta, st->emb, batch->ids, batch->ids, B, agg, agg_stride, 0.f, 0.f, hold, hold,
                              nullptr, nullptr, nullptr, nullptr, x);
    if (rc != PCG_OK) return rc;
    a.labels = nullptr;
    a.logits = out ? out->logits : nullptr;
    a.center = out ? out->center : nullptr;
    a.combined = out ? out->combined : nullptr;
    const int F = g->feat_dim, E = st->emb, R = g->n_rel;
    const bool wlds = dense_wlds(F, E, R);
    const size_t smem = dense_smem_bytes(F, E, R, wlds);
    typedef void (*kern_t)(const DenseArgs, const float *, const float *);
    const kern_t kern = dense_dispatch(F, E, R, wlds, [](auto s) -> kern_t {
        using S = decltype(s);
        return dense_vjp_kernel<S::wlds, S::F, S::E, S::R>;
    });
    if (allow_dynamic_lds(kern, 160 * 1024) != PCG_OK) return PCG_E_LAUNCH;
    // (acts mode: one workgroup per tile - a.n_split is 1)
    hipLaunchKernelGGL(kern, dim3((unsigned)a.n_tile_blocks), dim3(DENSE_THREADS), smem, static_cast<hipStream_t>(stream), a, d_logits,
                       d_center);
    PCG_LAUNCH_CHECK();
    return PCG_OK;
}
