// Whole-set inference for gfx950: the logits of any set of nodes (or of the whole graph) in large chunks, with one score pass
// per call instead of one per batch.
//
//   infer_front_kernel : the score pass of the label classifier over the whole table (score_table_body: the same workgroups,
//                        rows and fma order as pcg_score_table) || the look-back words of the call's two plan slots zeroed
//   per chunk          : plan (test mode) -> select -> gather (pcg_plan_epochs, pcg_choose_gather_planned) -> infer_dense_kernel
//   infer_dense_kernel : a persistent grid of dense workgroups (16 waves, 16-row tiles): each stages W_inter | W_intra[r] into
//                        LDS once (when they fit: the emb-128 shapes stream them from L2 as the training kernel does) and then
//                        runs the forward phases of dense_tile_body on tiles blockIdx.x, + gridDim.x, ... - static striding,
//                        no queue, no atomics.  No labels, loss, activations, slabs or optimizer.
//
// In test mode a row's logits depend on nothing but the row (its degree, the score table, the parameters): its selection list
// and gather chunks are laid out per row (RowRec::lbeg, chunk0), the dense phases sum in the same order whatever tile the row
// lands in.  So the chunked pass leaves bit for bit what pcg_train_dense (forward only, labels NULL) leaves batch by batch.
// Reference lines replaced: src/utils.py:298-305 (the batched evaluation loop), src/model.py:34-39 (PCALayer.forward).
#include "infer.h"
#include "halo_map.h"

namespace pcg {

__global__ void __launch_bounds__(256) infer_front_kernel(const float *__restrict__ X, int feat_dim, int stride,
                                                          const float *__restrict__ W, const float *__restrict__ bias,
                                                          int64_t n_nodes, float *__restrict__ s0, int n_score_blocks,
                                                          const ZeroRegions z) {
    const int b = (int)blockIdx.x;
    if (b < n_score_blocks) {
        score_table_body(X, feat_dim, stride, W, bias, 0, n_nodes, s0, b, n_score_blocks);
        return;
    }
    infer_zero_body(z, b - n_score_blocks);   // the zeroing workgroups
}

// the front launch of a whole-set call (pcg_infer_set, pcg_chosen_set): the table's scores with (W, bias) || the words of z zeroed
int launch_infer_front(const pcg_graph_desc *g, const float *W, const float *bias, float *s0, const ZeroRegions &z, hipStream_t st) {
    const int64_t zero_words = z.n[0] + z.n[1] + z.n[2] + z.n[3];
    const int n_zero = (int)((zero_words + INFER_ZERO_WORDS - 1) / INFER_ZERO_WORDS);
    const int n_score = (int)score_table_blocks(g->n_nodes, g->feat_stride);
    hipLaunchKernelGGL(infer_front_kernel, dim3(n_score + n_zero), dim3(256), 0, st, g->X, g->feat_dim, g->feat_stride, W, bias,
                       g->n_nodes, s0, n_score, z);
    PCG_LAUNCH_CHECK();
    return PCG_OK;
}

// PERSIST: tile blockIdx.x, then + gridDim.x, ...; else one tile per workgroup (the run-time shapes: a loop around their
// run-time index arithmetic needs more than the 128 VGPRs a 1024-thread workgroup has - it spilled)
template <bool WLDS, int F_, int E_, int R_, bool PERSIST>
__global__ void __launch_bounds__(DENSE_THREADS) infer_dense_kernel(const DenseArgs a, int n_tiles) {
    extern __shared__ __align__(16) float sm[];
    int tile = (int)blockIdx.x;                       // (gridDim.x <= n_tiles: every workgroup has a first tile)
    dense_tile_body<WLDS, F_, E_, R_, true, true>(a, tile, sm);
    if constexpr (PERSIST) {
        for (tile += (int)gridDim.x; tile < n_tiles; tile += (int)gridDim.x) {
            __syncthreads();                          // (the tile before: its last phase's LDS reads)
            dense_tile_body<WLDS, F_, E_, R_, true, false>(a, tile, sm);
        }
    }
}

// WLDS for a forward-only launch: the training kernel's choice, if the K-split partial tiles fit where dcomb / dh_r live
bool infer_wlds(int F, int E, int R) {
    if (!dense_wlds(F, E, R)) return false;
    const int ntile_e = E / 16, kparts = ntile_e <= DENSE_WAVES ? DENSE_WAVES / ntile_e : 1;
    return (int64_t)kparts * TB * E <= (int64_t)(1 + R) * TB * (E + 1);
}

static int device_cus() {
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cus[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
        cus[dev] = n;
    }
    return cus[dev];
}

static int infer_blocks(int B) {
    const int n_tiles = (B + TB - 1) / TB;
    const int cus = device_cus();
    return n_tiles < cus ? n_tiles : cus;
}

int launch_infer_dense(const DenseArgs &a, int B, hipStream_t st) {
    const int F = a.feat_dim, E = a.emb, R = a.n_rel;
    const bool wlds = infer_wlds(F, E, R);
    const size_t smem = dense_smem_bytes(F, E, R, wlds);
    typedef void (*kern_t)(const DenseArgs, int);
    kern_t kern;
    bool persist = true;
    if (R == 3 && F == 32 && E == 64 && wlds) kern = infer_dense_kernel<true, 32, 64, 3, true>;
    else if (R == 3 && F == 25 && E == 64 && wlds) kern = infer_dense_kernel<true, 25, 64, 3, true>;
    else if (R == 3 && F == 32 && E == 128 && !wlds) kern = infer_dense_kernel<false, 32, 128, 3, true>;
    else if (R == 3 && F == 25 && E == 128 && !wlds) kern = infer_dense_kernel<false, 25, 128, 3, true>;
    else {
        kern = wlds ? infer_dense_kernel<true, 0, 0, 0, false> : infer_dense_kernel<false, 0, 0, 0, false>;
        persist = false;
    }
    static kern_t attr_done[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool seen = false;
    for (kern_t k : attr_done) seen = seen || k == kern;
    if (!seen) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
            hipSuccess)
            return PCG_E_LAUNCH;
        for (kern_t &k : attr_done)
            if (!k) {
                k = kern;
                break;
            }
    }
    const int n_tiles = (B + TB - 1) / TB;
    hipLaunchKernelGGL(kern, dim3(persist ? infer_blocks(B) : n_tiles), dim3(DENSE_THREADS), smem, st, a, n_tiles);
    PCG_LAUNCH_CHECK();
    return PCG_OK;
}

// the call's workspace (InferCarve, infer.h)
int infer_carve(const pcg_graph_desc *g, int32_t emb, int32_t chunk_rows, int64_t list_capacity, InferCarve &c) {
    if (!g || chunk_rows < 1 || list_capacity < 1 || list_capacity >= (1ll << 31)) return PCG_E_ARG;
    if (emb < 16 || emb % 16 != 0 || g->n_rel < 1 || g->n_rel > PCG_MAX_REL || g->feat_dim < 1) return PCG_E_UNSUPPORTED;
    if ((int64_t)g->n_rel * chunk_rows >= (1ll << 31)) return PCG_E_ARG;
    const CarveSizes sz = carve(g, chunk_rows, list_capacity, nullptr, nullptr, nullptr);
    const int64_t R = g->n_rel, B = chunk_rows, F = g->feat_dim;
    c.plan_bytes = sz.plan_bytes;
    c.data = 2 * sz.plan_bytes;
    c.agg = c.data + align256(sz.data_bytes);
    c.cnt = c.agg + align256(4 * R * B * F);
    c.center = c.cnt + align256(4 * R * B);
    c.total = c.center + align256(8 * B);
    return PCG_OK;
}

void infer_zero_regions(ZeroRegions &z, const pcg_graph_desc *g, int32_t chunk_rows, int32_t tail, int64_t list_capacity,
                        unsigned char *slot0, unsigned char *slot1, unsigned char *data) {
    const int32_t slot_B[2] = {chunk_rows, tail};
    unsigned char *slot[2] = {slot0, slot1};
    for (int s = 0; s < 2; ++s) {
        Workspace w;
        carve1(g, slot_B[s], list_capacity, data, &w, slot[s]);
        z.p[2 * s] = w.counters;                                  // counters | heads: contiguous (256 + 512 bytes)
        z.n[2 * s] = (reinterpret_cast<unsigned char *>(w.heads) - reinterpret_cast<unsigned char *>(w.counters) + 4 * 8 * 16) / 4;
        z.p[2 * s + 1] = reinterpret_cast<uint32_t *>(w.plan_totals);
        z.n[2 * s + 1] = 64 * ((int64_t)g->n_rel * slot_B[s] / 256 + 2) / 4;
    }
}

// ---- partitioned inference (pcg_infer_chunk_dist, pc-gnn_amd/dist.py) ------------------------------------------------------
// gather.hip
int launch_gather_infer(const float *X, int32_t feat_dim, int32_t feat_stride, int32_t n_rows, const int32_t *cnt, const Workspace &w,
                        float *agg, int32_t agg_stride, uint32_t *status, const HaloMap &hm, const float *halo_X, hipStream_t st);

// A chunk's front: workgroups [0, n_tab) score the rank's table rows [0, n_tab_rows) (owned | train-pos: the first chunk of a
// call only) -> s0[tab_ids[row]]; [n_tab, n_tab + n_halo) score the inference halo rows -> s0[halo_ids[row]] (-1: unused slot,
// skipped); the rest zero the look-back words of the chunk's plan slot.  score_table_body throughout: a row's score has the
// bits pcg_score_table gives it on one GPU (the arithmetic is the row's alone: its lanes, fma chain and butterfly).
__global__ void __launch_bounds__(256) infer_front_dist_kernel(const float *__restrict__ X, const float *__restrict__ halo_X,
                                                               int feat_dim, int stride, const float *__restrict__ W,
                                                               const float *__restrict__ bias, const int32_t *__restrict__ tab_ids,
                                                               int64_t n_tab_rows, const int32_t *__restrict__ halo_ids,
                                                               int64_t n_halo_rows, float *__restrict__ s0, int n_tab, int n_halo,
                                                               const ZeroRegions z) {
    int b = (int)blockIdx.x;
    if (b < n_tab) {
        score_table_body(X, feat_dim, stride, W, bias, 0, n_tab_rows, s0, b, n_tab, tab_ids);
        return;
    }
    b -= n_tab;
    if (b < n_halo) {
        score_table_body(halo_X, feat_dim, stride, W, bias, 0, n_halo_rows, s0, b, n_halo, halo_ids);
        return;
    }
    infer_zero_body(z, b - n_halo);
}

// the call's workspace: [plan slot (chunk_rows) | data part | agg [R][chunk][F] | cnt [R][chunk] | centre logits [chunk][2]];
// a chunk of fewer rows carves its own layout inside the same bytes (every part grows with the rows)
static int infer_dist_carve(const pcg_graph_desc *g, int32_t emb, int32_t chunk_rows, int64_t list_capacity, InferCarve &c) {
    if (!g || chunk_rows < 1 || list_capacity < 1 || list_capacity >= (1ll << 31)) return PCG_E_ARG;
    if (emb < 16 || emb % 16 != 0 || g->n_rel < 1 || g->n_rel > PCG_MAX_REL || g->feat_dim < 1) return PCG_E_UNSUPPORTED;
    if ((int64_t)g->n_rel * chunk_rows >= (1ll << 31)) return PCG_E_ARG;
    const CarveSizes sz = carve(g, chunk_rows, list_capacity, nullptr, nullptr, nullptr);
    const int64_t R = g->n_rel, B = chunk_rows, F = g->feat_dim;
    c.plan_bytes = sz.plan_bytes;
    c.data = sz.plan_bytes;
    c.agg = c.data + align256(sz.data_bytes);
    c.cnt = c.agg + align256(4 * R * B * F);
    c.center = c.cnt + align256(4 * R * B);
    c.total = c.center + align256(8 * B);
    return PCG_OK;
}

}  // namespace pcg

extern "C" {

int64_t pcg_infer_workspace_bytes(const pcg_graph_desc *g, int32_t emb, int32_t chunk_rows, int64_t list_capacity) {
    pcg::InferCarve c;
    const int rc = pcg::infer_carve(g, emb, chunk_rows, list_capacity, c);
    return rc != PCG_OK ? rc : c.total;
}

int32_t pcg_infer_blocks(int32_t chunk_rows) { return chunk_rows < 1 ? PCG_E_ARG : pcg::infer_blocks(chunk_rows); }

int pcg_infer_set(const pcg_graph_desc *g, const float *theta, int32_t emb, const int32_t *ids, int32_t n, int32_t chunk_rows,
                  float *s0, const double *thresholds, void *workspace, int64_t list_capacity, float *out_logits, float *out_center,
                  uint32_t *status, void *stream) {
    if (!g || !g->X || !theta || !ids || n < 0 || !s0 || !thresholds || !workspace || !out_logits || !status) return PCG_E_ARG;
    if (g->feat_dim < 1 || g->feat_stride < g->feat_dim || g->feat_stride % 4 != 0 || g->feat_stride > 512) return PCG_E_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(g->X) & 15u) != 0) return PCG_E_ARG;
    pcg::InferCarve c;
    int rc = pcg::infer_carve(g, emb, chunk_rows, list_capacity, c);
    if (rc != PCG_OK) return rc;
    const int F = g->feat_dim, E = emb, R = g->n_rel;
    if (pcg::dense_smem_bytes(F, E, R, pcg::infer_wlds(F, E, R)) > 160 * 1024) return PCG_E_UNSUPPORTED;
    if (n == 0) return PCG_OK;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    unsigned char *slot[2] = {ws, ws + c.plan_bytes}, *data = ws + c.data;
    float *agg = reinterpret_cast<float *>(ws + c.agg);
    int32_t *cnt = reinterpret_cast<int32_t *>(ws + c.cnt);
    float *center_scratch = reinterpret_cast<float *>(ws + c.center);
    const int n_chunks = (int)(((int64_t)n + chunk_rows - 1) / chunk_rows);
    const int32_t tail = n - (n_chunks - 1) * chunk_rows;
    hipStream_t st = static_cast<hipStream_t>(stream);

    // the front: scores || the look-back words (counters, queue heads, per-workgroup totals) of both slots as the layouts of this
    // call's chunk sizes place them.  A slot's earlier plans may have laid other arrays over those words: zeroed, none of them
    // can pass for a published total (the tags the plan launches count from the zeroed sequence word start at 1)
    pcg::ZeroRegions z = {};
    pcg::infer_zero_regions(z, g, chunk_rows, tail, list_capacity, slot[0], slot[1], data);
    rc = pcg::launch_infer_front(g, theta + pcg::off_clf(F, E, R), theta + pcg::off_bias(F, E, R), s0, z, st);
    if (rc != PCG_OK) return rc;

    for (int ch = 0; ch < n_chunks; ++ch) {
        const int64_t off = (int64_t)ch * chunk_rows;
        const int32_t B = ch + 1 < n_chunks ? chunk_rows : tail;
        unsigned char *plan = slot[B == chunk_rows ? 0 : 1];
        const int32_t *cid = ids + off;
        rc = pcg_plan_epochs(g, cid, nullptr, B, 1, B, thresholds, nullptr, 0, 0, plan, c.plan_bytes, list_capacity, status, nullptr,
                             stream);
        if (rc != PCG_OK) return rc;
        rc = pcg_choose_gather_planned(g, cid, nullptr, B, s0, nullptr, nullptr, thresholds, nullptr, 0, 0, agg, F, cnt, data, plan,
                                       list_capacity, status, nullptr, stream);
        if (rc != PCG_OK) return rc;
        pcg::Workspace w;
        pcg::carve1(g, B, list_capacity, data, &w, plan);
        pcg::DenseExtra x;
        x.chunk_begin = w.chunk_begin;
        x.partial = w.partial;
        x.cnt = cnt;
        x.partial_stride = g->feat_stride;
        pcg::DenseArgs a;
        int n_sort_blocks = 0;
        rc = pcg::dense_args(a, n_sort_blocks, g, theta, emb, cid, nullptr, B, agg, F, 0.f, 1.f, out_logits + 2 * off,
                             out_center ? out_center + 2 * off : center_scratch, nullptr, nullptr, nullptr, nullptr, x);
        if (rc != PCG_OK) return rc;
        a.stamps = nullptr;
        rc = pcg::launch_infer_dense(a, B, st);
        if (rc != PCG_OK) return rc;
    }
    return PCG_OK;
}

int64_t pcg_infer_dist_workspace_bytes(const pcg_graph_desc *g, int32_t emb, int32_t chunk_rows, int64_t list_capacity) {
    pcg::InferCarve c;
    const int rc = pcg::infer_dist_carve(g, emb, chunk_rows, list_capacity, c);
    return rc != PCG_OK ? rc : c.total;
}

int pcg_infer_chunk_dist(const pcg_graph_desc *g, const float *theta, int32_t emb, const int32_t *ids, int32_t B, int32_t first,
                         const int32_t *row_gid, int64_t n_table_rows, const float *halo_X, const int32_t *halo_ids, int32_t halo_cap,
                         int32_t lo, int32_t hi, const int32_t *pos_ids, const int32_t *pos_idx, const uint32_t *table,
                         int64_t table_slots, uint32_t *counts, float *s0, const double *thresholds, void *workspace,
                         int32_t chunk_rows, int64_t list_capacity, float *out_logits, float *out_center, uint32_t *status,
                         void *stream) {
    if (!g || !g->X || !theta || !ids || B < 0 || B > chunk_rows || !row_gid || !halo_X || !halo_ids || halo_cap < 1 || !table ||
        !counts || !s0 || !thresholds || !workspace || !out_logits || !status)
        return PCG_E_ARG;
    if (g->feat_dim < 1 || g->feat_stride < g->feat_dim || g->feat_stride % 4 != 0 || g->feat_stride > 512) return PCG_E_UNSUPPORTED;
    if (((reinterpret_cast<uintptr_t>(g->X) | reinterpret_cast<uintptr_t>(halo_X)) & 15u) != 0) return PCG_E_ARG;
    const int64_t n_local = (int64_t)hi - lo, halo_base = n_local + g->n_pos;
    if (lo < 0 || n_local < 0 || n_table_rows < 0 || n_table_rows > g->n_nodes || halo_base > g->n_nodes) return PCG_E_ARG;
    if (table_slots < 1024 || (table_slots & (table_slots - 1)) != 0 || (g->n_pos > 0 && (!pos_ids || !pos_idx))) return PCG_E_ARG;
    pcg::InferCarve c;
    int rc = pcg::infer_dist_carve(g, emb, chunk_rows, list_capacity, c);
    if (rc != PCG_OK) return rc;
    const int F = g->feat_dim, E = emb, R = g->n_rel;
    if (pcg::dense_smem_bytes(F, E, R, pcg::infer_wlds(F, E, R)) > 160 * 1024) return PCG_E_UNSUPPORTED;
    if (B == 0) return PCG_OK;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    unsigned char *plan = ws, *data = ws + c.data;
    float *agg = reinterpret_cast<float *>(ws + c.agg);
    int32_t *cnt = reinterpret_cast<int32_t *>(ws + c.cnt);
    float *center_scratch = reinterpret_cast<float *>(ws + c.center);
    hipStream_t st = static_cast<hipStream_t>(stream);
    pcg::Workspace w;
    pcg::carve1(g, B, list_capacity, data, &w, plan);

    // front: halo scores (+ the table's on the first chunk) || the look-back words of this chunk's plan layout
    pcg::ZeroRegions z = {};
    z.p[0] = w.counters;                                          // counters | heads: contiguous (256 + 512 bytes)
    z.n[0] = (reinterpret_cast<unsigned char *>(w.heads) - reinterpret_cast<unsigned char *>(w.counters) + 4 * 8 * 16) / 4;
    z.p[1] = reinterpret_cast<uint32_t *>(w.plan_totals);
    z.n[1] = 64 * ((int64_t)R * B / 256 + 2) / 4;
    const int n_zero = (int)((z.n[0] + z.n[1] + pcg::INFER_ZERO_WORDS - 1) / pcg::INFER_ZERO_WORDS);
    const int64_t tab_rows = first ? n_table_rows : 0;
    const int n_tab = tab_rows > 0 ? (int)pcg::score_table_blocks(tab_rows, g->feat_stride) : 0;
    const int n_halo = (int)pcg::score_table_blocks(halo_cap, g->feat_stride);
    hipLaunchKernelGGL(pcg::infer_front_dist_kernel, dim3(n_tab + n_halo + n_zero), dim3(256), 0, st, g->X, halo_X, g->feat_dim,
                       g->feat_stride, theta + pcg::off_clf(F, E, R), theta + pcg::off_bias(F, E, R), row_gid, tab_rows, halo_ids,
                       (int64_t)halo_cap, s0, n_tab, n_halo, z);
    PCG_LAUNCH_CHECK();
    // plan (test mode) -> select (centre scores by global id: s0[ids[b] + lo]; lists of global ids)
    rc = pcg_plan_epochs(g, ids, nullptr, B, 1, B, thresholds, nullptr, 0, 0, plan, c.plan_bytes, list_capacity, status, nullptr,
                         stream);
    if (rc != PCG_OK) return rc;
    rc = pcg_choose_select_planned(g, ids, nullptr, B, s0, nullptr, nullptr, thresholds, nullptr, 0, 0, cnt, data, plan,
                                   list_capacity, status, nullptr, lo, stream);
    if (rc != PCG_OK) return rc;
    // gather: ids -> owned / train-pos rows of g->X, fetched rows of the inference halo (its own hash table)
    pcg::HaloMap hm;
    hm.keys = table;
    hm.vals = table + table_slots;
    hm.mask = (uint32_t)(table_slots - 1);
    hm.lo = lo; hm.hi = hi; hm.n_local = (int32_t)n_local;
    hm.pos_ids = pos_ids; hm.pos_idx = pos_idx; hm.n_pos = g->n_pos;
    hm.halo_cap = halo_cap; hm.halo_base = (int32_t)halo_base;
    hm.overflow = counts + 128;
    rc = pcg::launch_gather_infer(g->X, F, g->feat_stride, R * B, cnt, w, agg, F, status, hm, halo_X, st);
    if (rc != PCG_OK) return rc;
    // dense: the centres are local table rows
    pcg::DenseExtra x;
    x.chunk_begin = w.chunk_begin;
    x.partial = w.partial;
    x.cnt = cnt;
    x.partial_stride = g->feat_stride;
    pcg::DenseArgs a;
    int n_sort_blocks = 0;
    rc = pcg::dense_args(a, n_sort_blocks, g, theta, emb, ids, nullptr, B, agg, F, 0.f, 1.f, out_logits,
                         out_center ? out_center : center_scratch, nullptr, nullptr, nullptr, nullptr, x);
    if (rc != PCG_OK) return rc;
    a.stamps = nullptr;
    return pcg::launch_infer_dense(a, B, st);
}

}  // extern "C"
