// Dense tail of the PC-GNN step for gfx950: relation GEMMs, inter GEMM, classifier, the two cross-entropy terms,
// their backward and Adam.
//
//   dense_step : one 1024-thread workgroup per tile of 16 batch rows (up to 4 of them when the batch has few tiles: all
//                run the forward pass, the weight-gradient tiles are dealt out among them) does the whole forward for its
//                rows, the loss gradients, and this tile's partial weight gradients (split-K over the batch: one partial
//                "slab" per tile, no atomics => bitwise reproducible).  GEMMs run on the f32 matrix cores
//                (v_mfma_f32_16x16x4_f32: exact fmaf chains).  Rows whose selection list the gather left as several
//                partial sums are summed (in chunk order) while the tile is staged - no combine launch.  Optionally the
//                workgroup whose label-classifier gradient arrives last applies Adam to those 2F + 2 parameters - the only
//                ones the next step's score pass needs - so that the update of all others can ride along that pass.
//   adam_reduce: sums the slabs in tile order and applies torch.optim.Adam's update (coupled L2 weight decay) to a
//                range of the flat parameter buffer.
//
// f32 MFMA runs at the f32 vector rate (256 FLOP / clk / CU): one tile is ~2.6 MFLOP forward + backward, i.e. >= 4 us of
// matrix time on ONE CU, which is why a tile's work is spread over several workgroups rather than several tiles looped
// over by one (the slabs that costs are summed by the Adam pass, beside the next step's score pass).
//
// Reference lines replaced: src/layers.py:273-289, 625-629; src/model.py:34-62;
// src/model_handler.py:124,149-153 (optimizer.zero_grad / loss.backward / optimizer.step).
// Gradients never flow into the gathered features or the selection (features frozen,
// model_handler.py:86; selection is index-only), so backward is dense GEMMs only.
#include "dense.h"

namespace pcg {

template <bool WLDS, int F_, int E_, int R_>
__global__ void __launch_bounds__(DENSE_THREADS) dense_step_kernel(const DenseArgs a) {
    extern __shared__ __align__(16) float sm[];
    if (a.sort_raw && (int)blockIdx.x >= a.n_tile_blocks) {
        // the next step's sorted train-pos keys (pos_rank_sort's body: a workgroup ranks 64 keys against all of them): the select
        // launch that follows finds them sorted - no in-kernel sort, no row waiting for it, and a positive hub row's window
        // search can run beside its key pass
        uint64_t *sh = reinterpret_cast<uint64_t *>(sm);
        int *part = reinterpret_cast<int *>(sh + DENSE_SORT_TILE);
        rank_sort_body<DENSE_SORT_TILE, DENSE_WAVES, false>(nullptr, nullptr, a.sort_n, a.sort_cap, a.sort_out,
                                                            (int)blockIdx.x - a.n_tile_blocks, sh, part, a.sort_raw);
        return;
    }
    dense_tile_body<WLDS, F_, E_, R_>(a, (int)blockIdx.x, sm);
}

__global__ void __launch_bounds__(256) adam_reduce_kernel(float *__restrict__ theta, float *__restrict__ m,
                                                          float *__restrict__ v, const float *__restrict__ slabs,
                                                          int n_slabs, int64_t n_params, int64_t p_begin, int64_t p_end,
                                                          const int32_t *__restrict__ step_counter, AdamHyper h,
                                                          float *__restrict__ grad_out, int apply, const uint32_t *pending) {
    __shared__ float part[4][PCG_WAVE];
    if (pending) {                                    // the deferred update: nothing to do unless a gradient is waiting in the slabs
        if (pending[0] != 1u) return;                 // (wave-uniform: one word; 2 = it waits in `acts`: wgrad_adam_kernel's)
        n_slabs = (int)pending[1];
    }
    adam_reduce_body(theta, m, v, slabs, n_slabs, n_params, p_begin, p_end, step_counter, h, grad_out, apply, (int)blockIdx.x, part);
}

// the weight gradients from the dense kernel's transposed activations + Adam (wgrad.h), as a launch of its own
__global__ void __launch_bounds__(256) wgrad_adam_kernel(const WgradArgs a) {
    __shared__ float red[4][256];
    wgrad_adam_body(a, (int)blockIdx.x, red);
}

__global__ void clear_word_kernel(uint32_t *w) { w[0] = 0u; }
// dst[i] = src[i] if an update is pending (pcg_adam_flush: the stepped label classifier -> the parameter buffer)
__global__ void __launch_bounds__(256) copy_if_pending_kernel(float *__restrict__ dst, const float *__restrict__ src, int n,
                                                              const uint32_t *__restrict__ pending) {
    if (pending[0] == 0u) return;
    for (int i = (int)threadIdx.x; i < n; i += (int)blockDim.x) dst[i] = src[i];
}

// The partitioned path's two optimizer launches (its gradient goes through an all-reduce between them):
//   grad_reduce   : slabs summed in tile order -> grad; marks "a gradient is waiting" (flag[0] = 1)
//   apply_pending : if a gradient is waiting: Adam on every parameter from grad (after the all-reduce, at the head of the NEXT step's
//                   graph - no launch of its own between the collective and the next score pass).  The flag is cleared by a LATER
//                   launch (the step's select kernel: pcg_choose_select_planned(sync_words) clears sync_words[1]; or the
//                   one-thread launch pcg_adam_apply_pending(clear = 1) adds) - a departure ticket in this kernel was 420
//                   same-address atomics, 4.8 us
__global__ void __launch_bounds__(256) grad_reduce_kernel(const float *__restrict__ slabs, int n_slabs, int64_t n_params,
                                                          float *__restrict__ grad_out, uint32_t *flag) {
    __shared__ float part[4][PCG_WAVE];
    if (blockIdx.x == 0 && threadIdx.x == 0) flag[0] = 1u;
    const AdamHyper none = {0.f, 0.f, 0.f, 0.f, 0.f};
    adam_reduce_body(nullptr, nullptr, nullptr, slabs, n_slabs, n_params, 0, n_params, nullptr, none, grad_out, 0, (int)blockIdx.x, part);
}
__global__ void __launch_bounds__(256) apply_pending_kernel(float *__restrict__ theta, float *__restrict__ m, float *__restrict__ v,
                                                            const float *__restrict__ grad, int64_t n_params,
                                                            const int32_t *__restrict__ step_counter, AdamHyper h,
                                                            const uint32_t *__restrict__ flag) {
    __shared__ float part[4][PCG_WAVE];
    if (flag[0] == 0u) return;                                    // (one word, the same for every thread)
    adam_reduce_body(theta, m, v, grad, 1, n_params, 0, n_params, step_counter, h, nullptr, 1, (int)blockIdx.x, part);
}

unsigned long long *g_dense_stamps = nullptr;

}  // namespace pcg
/* 1: pcg_train_dense(adam_clf = 3, sort_keys) for a batch of B rows also sorts the next step's train-pos keys (n_pos of them: the
 * rank sort's sizes) - when its tiles' workgroups and the sort's together leave no CU with two of them (up to ~3000 rows): the
 * sort is then free.  (PCG_PRESORT_MAX_TILES=n also allows batches of up to n tiles, the sorting workgroups running behind the
 * tiles'.  Measured at 256 tiles: power-law 2 M / 8000 keys - where the in-kernel sort publishes 13 us into the select launch and
 * every positive row waits for it - the call 123.3 -> 117.3 us but the step 136.5 -> 142.8: 125 rank-sorting workgroups behind the
 * tiles cost the dense launch more than the select launch gains; emb 128 / 2670 keys: 94.1 -> 93.5.  Off.)  Host helper. */
extern "C" int32_t pcg_dense_sorts_keys(int32_t B, int32_t n_pos) {
    if (B < 1 || n_pos < 1 || n_pos > pcg::RANK_MAX) return 0;
    static int max_tiles = -1;
    if (max_tiles < 0) {
        const char *e = getenv("PCG_PRESORT_MAX_TILES");
        max_tiles = e ? atoi(e) : 0;
    }
    const int tiles = (B + pcg::TB - 1) / pcg::TB;
    if (tiles + (n_pos + PCG_WAVE - 1) / PCG_WAVE <= 256) return 1;
    return tiles <= max_tiles ? 1 : 0;
}
namespace pcg {

int dense_args(DenseArgs &a, int &n_sort_blocks, const pcg_graph_desc *g, const float *theta, int32_t emb, const int32_t *ids,
               const int32_t *labels, int32_t B, const float *agg, int32_t agg_stride, float lambda_1, float inv_count, float *logits,
               float *center, float *combined, float *row_loss, float *slabs, int32_t *step_counter, const DenseExtra &x) {
    if (!g || !g->X || !theta || B < 1) return PCG_E_ARG;
    if (!ids || !agg || !logits || !center) return PCG_E_ARG;
    if (emb < 16 || emb % 16 != 0 || g->n_rel < 1 || g->n_rel > PCG_MAX_REL) return PCG_E_UNSUPPORTED;
    if ((slabs || x.acts) && !labels) return PCG_E_ARG;
    if (x.acts && (x.act_ld < (B + TB - 1) / TB * TB || x.act_ld % 4 != 0 || (reinterpret_cast<uintptr_t>(x.acts) & 15u) != 0)) return PCG_E_ARG;
    if (x.theta_rw && (!slabs || !x.m || !x.v || !x.ticket || !step_counter)) return PCG_E_ARG;
    if (x.chunk_begin && (!x.partial || !x.cnt)) return PCG_E_ARG;
    const int F = g->feat_dim, E = emb, R = g->n_rel;
    if (dense_smem_bytes(F, E, R, dense_wlds(F, E, R)) > 160 * 1024) return PCG_E_UNSUPPORTED;
    a.X = g->X;
    a.feat_dim = F;
    a.feat_stride = g->feat_stride;
    a.n_rel = R;
    a.emb = E;
    a.ids = ids;
    a.labels = labels;
    a.B = B;
    a.agg = agg;
    a.agg_stride = agg_stride;
    a.chunk_begin = x.chunk_begin;
    a.partial = x.partial;
    a.cnt = x.cnt;
    a.partial_stride = x.partial_stride;
    a.W_cls = theta + off_cls(F, E, R);
    a.W_inter = theta + off_inter(F, E, R);
    for (int r = 0; r < PCG_MAX_REL; ++r) a.W_intra[r] = r < R ? theta + off_intra(F, E, R, r) : nullptr;
    a.W_clf = theta + off_clf(F, E, R);
    a.b_clf = theta + off_bias(F, E, R);
    a.lambda_1 = lambda_1;
    a.inv_count = inv_count;
    a.logits = logits;
    a.center = center;
    a.combined = combined;
    a.row_loss = row_loss;
    a.slabs = x.acts ? nullptr : slabs;
    a.acts = x.acts;
    a.act_ld = x.act_ld;
    a.n_params = n_params_of(F, E, R);
    a.step_counter = step_counter;
    a.theta = x.theta_rw;
    a.m = x.m;
    a.v = x.v;
    a.ticket = x.ticket;
    a.staged = x.staged;
    a.pending = x.pending;
    a.h = x.h;
    // few tiles (small batches): up to 4 workgroups per tile, so that the weight-gradient tiles of a 16-row tile are not one
    // CU's serial work while most of the chip idles
    const int n_tiles = (B + TB - 1) / TB;
    // (acts instead of slabs: no weight-gradient tiles to deal out - one workgroup per tile)
    int n_split = (slabs && !x.acts) ? 256 / n_tiles : 1;
    a.n_split = n_split < 1 ? 1 : (n_split > 4 ? 4 : n_split);
    a.stamps = g_dense_stamps;
    a.sort_raw = nullptr;
    a.sort_out = nullptr;
    a.sort_n = a.sort_cap = 0;
    a.n_tile_blocks = n_tiles * a.n_split;
    n_sort_blocks = 0;
    if (x.sort_keys && pcg_dense_sorts_keys(B, g->n_pos)) {
        const int64_t cap = pcg_pos_sort_capacity(g->n_pos) / 2;
        a.sort_out = x.sort_keys;
        a.sort_raw = x.sort_keys + cap;
        a.sort_n = g->n_pos;
        a.sort_cap = (int32_t)cap;
        n_sort_blocks = (g->n_pos + PCG_WAVE - 1) / PCG_WAVE;
    }
    return PCG_OK;
}

static int launch_dense(const pcg_graph_desc *g, const float *theta, int32_t emb, const int32_t *ids, const int32_t *labels,
                        int32_t B, const float *agg, int32_t agg_stride, float lambda_1, float inv_count, float *logits,
                        float *center, float *combined, float *row_loss, float *slabs, int32_t *step_counter,
                        const DenseExtra &x, void *stream) {
    if (!g || !g->X || !theta || B < 0) return PCG_E_ARG;
    if (B == 0) return PCG_OK;
    DenseArgs a;
    int n_sort_blocks = 0;
    const int rc = dense_args(a, n_sort_blocks, g, theta, emb, ids, labels, B, agg, agg_stride, lambda_1, inv_count, logits, center,
                              combined, row_loss, slabs, step_counter, x);
    if (rc != PCG_OK) return rc;
    const int F = g->feat_dim, E = emb, R = g->n_rel;
    const bool wlds = dense_wlds(F, E, R);
    const size_t smem = dense_smem_bytes(F, E, R, wlds);
    const int n_tiles = (B + TB - 1) / TB;
    typedef void (*kern_t)(const DenseArgs);
    const kern_t kern = dense_dispatch(F, E, R, wlds, [](auto s) -> kern_t {
        using S = decltype(s);
        return dense_step_kernel<S::wlds, S::F, S::E, S::R>;
    });
    if (allow_dynamic_lds(kern, 160 * 1024) != PCG_OK) return PCG_E_LAUNCH;
    const dim3 grid(n_tiles * a.n_split + n_sort_blocks), block(DENSE_THREADS);
    const size_t sort_smem = n_sort_blocks ? sizeof(uint64_t) * DENSE_SORT_TILE + sizeof(int) * DENSE_THREADS : 0;
    hipLaunchKernelGGL(kern, grid, block, smem > sort_smem ? smem : sort_smem, static_cast<hipStream_t>(stream), a);
    PCG_LAUNCH_CHECK();
    return PCG_OK;
}

}  // namespace pcg

extern "C" {

void pcg_debug_set_dense_stamps(void *ptr) { pcg::g_dense_stamps = static_cast<unsigned long long *>(ptr); }

int64_t pcg_dense_n_params(int32_t feat_dim, int32_t emb, int32_t n_rel) {
    if (feat_dim < 1 || emb < 1 || n_rel < 1 || n_rel > PCG_MAX_REL) return PCG_E_ARG;
    return pcg::n_params_of(feat_dim, emb, n_rel);
}

int64_t pcg_dense_param_offset(int32_t feat_dim, int32_t emb, int32_t n_rel, int32_t which, int32_t rel) {
    switch (which) {
        case 0: return pcg::off_cls(feat_dim, emb, n_rel);
        case 1: return pcg::off_inter(feat_dim, emb, n_rel);
        case 2: return pcg::off_intra(feat_dim, emb, n_rel, rel);
        case 3: return pcg::off_clf(feat_dim, emb, n_rel);
        case 4: return pcg::off_bias(feat_dim, emb, n_rel);
        default: return PCG_E_ARG;
    }
}

int32_t pcg_dense_n_tiles(int32_t B) { return B < 0 ? PCG_E_ARG : (B + pcg::TB - 1) / pcg::TB; }

int pcg_dense_step(const pcg_graph_desc *g, const float *theta, int32_t emb, const int32_t *ids, const int32_t *labels,
                   int32_t B, const float *agg, int32_t agg_stride, float lambda_1, float inv_count, float *logits,
                   float *center, float *combined, float *row_loss, float *slabs, int32_t *step_counter, void *stream) {
    return pcg::launch_dense(g, theta, emb, ids, labels, B, agg, agg_stride, lambda_1, inv_count, logits, center, combined,
                             row_loss, slabs, step_counter, pcg::DenseExtra(), stream);
}

int pcg_train_dense(const pcg_graph_desc *g, const pcg_train_state *st, const pcg_batch *batch, const float *agg,
                    int32_t agg_stride, const pcg_select_ws *sel, const pcg_dense_out *out, int32_t adam_clf, uint64_t *sort_keys,
                    void *stream) {
    if (!g || !st || !batch || !sel || !out || batch->B < 0) return PCG_E_ARG;
    const int32_t B = batch->B;
    uint32_t *const sync_words = st->sync_words;
    pcg::DenseExtra x;
    if (sel->workspace) {
        if (!batch->cnt || sel->list_capacity < 1) return PCG_E_ARG;
        pcg::Workspace w;
        pcg::carve1(g, B, sel->list_capacity, static_cast<unsigned char *>(sel->workspace), &w,
                    static_cast<unsigned char *>(const_cast<void *>(batch->plan)));
        x.chunk_begin = w.chunk_begin;
        x.partial = w.partial;
        x.cnt = batch->cnt;
        x.partial_stride = g->feat_stride;
    }
    if (adam_clf == 3) {                     // no slabs: transposed activations for the weight-gradient GEMMs of a later launch
        if (!st->acts || !sync_words) return PCG_E_ARG;
        x.pending = sync_words + 1;
        x.acts = st->acts;
        x.act_ld = st->act_ld;
        x.sort_keys = sort_keys;             // (only this mode has one workgroup per tile: CUs to spare for the riding sort)
    } else if (adam_clf == 4) {              // the same without marking anything as waiting (pcg_wgrad follows: gradients only)
        if (!st->acts) return PCG_E_ARG;
        x.acts = st->acts;
        x.act_ld = st->act_ld;
    } else if (adam_clf == 2) {              // the label classifier is stepped elsewhere (pcg_choose_gather_train): slabs + "pending" only
        if (!st->slabs || !sync_words) return PCG_E_ARG;
        x.pending = sync_words + 1;
    } else if (adam_clf) {
        if (!st->slabs || !st->m || !st->v || !sync_words) return PCG_E_ARG;
        x.theta_rw = st->theta;
        x.m = st->m;
        x.v = st->v;
        x.ticket = sync_words;
        x.staged = sync_words + pcg_sync_words_count() - 4;
        x.pending = sync_words + 1;
        x.h = pcg::adam_hyper(st->hyper);
    }
    return pcg::launch_dense(g, st->theta, st->emb, batch->ids, batch->labels, B, agg, agg_stride, st->lambda_1, batch->inv_count,
                             out->logits, out->center, out->combined, out->row_loss, st->slabs, st->step_counter, x, stream);
}

int pcg_adam_step(float *theta, float *m, float *v, const float *slabs, int32_t n_slabs, int64_t n_params,
                  const int32_t *step_counter, const pcg_adam_hyper *hyper, float *grad_out, int32_t apply, void *stream) {
    if (!hyper || !slabs || n_slabs < 0 || n_params < 1) return PCG_E_ARG;
    if (apply && (!theta || !m || !v || !step_counter)) return PCG_E_ARG;
    if (!apply && !grad_out) return PCG_E_ARG;
    const pcg::AdamHyper h = pcg::adam_hyper(*hyper);
    hipLaunchKernelGGL(pcg::adam_reduce_kernel, dim3((unsigned)((n_params + PCG_WAVE - 1) / PCG_WAVE)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), theta, m, v, slabs, n_slabs, n_params, (int64_t)0, n_params,
                       step_counter, h, grad_out, apply, (const uint32_t *)nullptr);
    PCG_LAUNCH_CHECK();
    return PCG_OK;
}

int pcg_grad_reduce(const float *slabs, int32_t n_slabs, int64_t n_params, float *grad_out, uint32_t *flag, void *stream) {
    if (!slabs || n_slabs < 0 || n_params < 1 || !grad_out || !flag) return PCG_E_ARG;
    hipLaunchKernelGGL(pcg::grad_reduce_kernel, dim3((unsigned)((n_params + PCG_WAVE - 1) / PCG_WAVE)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), slabs, n_slabs, n_params, grad_out, flag);
    PCG_LAUNCH_CHECK();
    return PCG_OK;
}

int pcg_adam_apply_pending(float *theta, float *m, float *v, const float *grad, int64_t n_params, const int32_t *step_counter,
                           uint32_t *flag, int32_t clear, const pcg_adam_hyper *hyper, void *stream) {
    if (!hyper || !theta || !m || !v || !grad || n_params < 1 || !step_counter || !flag) return PCG_E_ARG;
    const pcg::AdamHyper h = pcg::adam_hyper(*hyper);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pcg::apply_pending_kernel, dim3((unsigned)((n_params + PCG_WAVE - 1) / PCG_WAVE)), dim3(256), 0, st, theta, m, v,
                       grad, n_params, step_counter, h, flag);
    PCG_LAUNCH_CHECK();
    if (clear) {
        hipLaunchKernelGGL(pcg::clear_word_kernel, dim3(1), dim3(1), 0, st, flag);
        PCG_LAUNCH_CHECK();
    }
    return PCG_OK;
}

// the GEMMs over st->acts and the parameters they may update; what the launch does with them is the caller's to set
static int wgrad_args(pcg::WgradArgs &w, const pcg_train_state *st, int32_t feat_dim, int32_t n_rel, int32_t n_kblocks) {
    const float *const acts = st->acts;
    float *const scratch = st->wg_scratch;
    const int32_t act_ld = st->act_ld, emb = st->emb;
    if (!acts || act_ld < 16 || act_ld % 16 != 0 || (reinterpret_cast<uintptr_t>(acts) & 15u) != 0) return PCG_E_ARG;
    if (feat_dim < 1 || emb < 16 || emb % 16 != 0 || n_rel < 1 || n_rel > PCG_MAX_REL) return PCG_E_UNSUPPORTED;
    if (n_kblocks < 1 || n_kblocks * 16 > act_ld) return PCG_E_ARG;
    w.acts = acts;
    w.ld = act_ld;
    w.F = feat_dim;
    w.E = emb;
    w.R = n_rel;
    w.n_kblocks = n_kblocks;
    w.kparts = pcg::wgrad_kparts(n_kblocks);
    w.tickets = nullptr;
    w.partials = nullptr;
    if (w.kparts > 1) {
        if (!scratch) return PCG_E_ARG;
        const int t = pcg::wgrad_tiles(feat_dim, emb, n_rel, 1);
        w.tickets = reinterpret_cast<uint32_t *>(scratch);
        w.partials = scratch + (t + 63) / 64 * 64;
    }
    w.theta = st->theta; w.m = st->m; w.v = st->v;
    w.step_counter = st->step_counter;
    w.h = pcg::adam_hyper(st->hyper);
    return PCG_OK;
}

int64_t pcg_wgrad_act_rows(int32_t feat_dim, int32_t emb, int32_t n_rel) {
    if (feat_dim < 1 || emb < 1 || n_rel < 1 || n_rel > PCG_MAX_REL) return PCG_E_ARG;
    return pcg::wgrad_act_rows(feat_dim, emb, n_rel);
}

int64_t pcg_wgrad_scratch_bytes(int32_t feat_dim, int32_t emb, int32_t n_rel, int32_t B) {
    if (feat_dim < 1 || emb < 16 || emb % 16 != 0 || n_rel < 1 || n_rel > PCG_MAX_REL || B < 1) return PCG_E_ARG;
    return 4 * pcg::wgrad_scratch_floats(feat_dim, emb, n_rel, (B + 15) / 16);
}

int pcg_wgrad(const pcg_train_state *st, int32_t B, int32_t feat_dim, int32_t n_rel, float *grad_out, int32_t apply,
              int32_t with_clf, uint32_t *flag_set, void *stream) {
    pcg::WgradArgs w;
    if (!st || B < 1) return PCG_E_ARG;
    const int rc = wgrad_args(w, st, feat_dim, n_rel, (B + 15) / 16);
    if (rc != PCG_OK) return rc;
    if (apply && (!st->theta || !st->m || !st->v || !st->step_counter)) return PCG_E_ARG;
    if (!apply && !grad_out) return PCG_E_ARG;
    w.pending = nullptr;
    w.grad_out = grad_out;
    w.flag_set = flag_set;
    w.apply = apply;
    w.with_clf = with_clf ? 1 : 0;
    hipLaunchKernelGGL(pcg::wgrad_adam_kernel, dim3((unsigned)(pcg::wgrad_tiles(feat_dim, st->emb, n_rel, w.with_clf) * w.kparts)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), w);
    PCG_LAUNCH_CHECK();
    return PCG_OK;
}

int pcg_adam_flush(const pcg_train_state *st, int32_t n_slabs, int64_t n_params, int64_t p_end, int32_t feat_dim, int32_t n_rel,
                   void *stream) {
    if (!st || !st->theta || !st->m || !st->v || (!st->slabs && !st->acts) || !st->step_counter || !st->sync_words || n_slabs < 0 ||
        n_params < 1 || p_end < 0 || p_end > n_params)
        return PCG_E_ARG;
    const pcg::AdamHyper h = pcg::adam_hyper(st->hyper);
    uint32_t *const pending = st->sync_words + 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (st->acts) {                          // a step of pcg_train_dense(adam_clf = 3) waiting (sync_words[1] == 2): weight-gradient GEMMs + Adam
        pcg::WgradArgs w;
        const int rc = wgrad_args(w, st, feat_dim, n_rel, st->act_ld / 16);
        if (rc != PCG_OK) return rc;
        if (pcg::n_params_of(feat_dim, st->emb, n_rel) != n_params) return PCG_E_ARG;
        w.pending = pending;
        w.grad_out = nullptr;
        w.flag_set = nullptr;
        w.apply = 1;
        w.with_clf = p_end > pcg::off_clf(feat_dim, st->emb, n_rel) ? 1 : 0;
        hipLaunchKernelGGL(pcg::wgrad_adam_kernel, dim3((unsigned)(pcg::wgrad_tiles(feat_dim, st->emb, n_rel, w.with_clf) * w.kparts)), dim3(256), 0, s, w);
        PCG_LAUNCH_CHECK();
    }
    if (p_end > 0 && st->slabs) {
        hipLaunchKernelGGL(pcg::adam_reduce_kernel, dim3((unsigned)((p_end + PCG_WAVE - 1) / PCG_WAVE)), dim3(256), 0, s, st->theta, st->m,
                           st->v, (const float *)st->slabs, n_slabs, n_params, (int64_t)0, p_end, (const int32_t *)st->step_counter, h,
                           (float *)nullptr, 1, (const uint32_t *)pending);
        PCG_LAUNCH_CHECK();
    }
    if (st->clf_next && p_end < n_params) {  // (pcg_choose_gather_train keeps the stepped label classifier outside theta until now)
        hipLaunchKernelGGL(pcg::copy_if_pending_kernel, dim3(1), dim3(256), 0, s, st->theta + p_end, (const float *)st->clf_next,
                           (int)(n_params - p_end), (const uint32_t *)pending);
        PCG_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(pcg::clear_word_kernel, dim3(1), dim3(1), 0, s, pending);
    PCG_LAUNCH_CHECK();
    return PCG_OK;
}

}  // extern "C"
