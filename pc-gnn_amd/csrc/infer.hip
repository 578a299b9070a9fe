// Whole-set inference for gfx950: the logits of any set of nodes (or of the whole graph) in large chunks, with one score pass
// per call instead of one per batch.
//
//   infer_front_kernel : the score pass of the label classifier over the whole table (score_table_body: the same workgroups,
//                        rows and fma order as pcg_score_table) || the look-back words of the call's two plan slots zeroed
//   per chunk          : plan (test mode) -> select (ChunkDriver::run, infer.h) -> gather (pcg_gather_lists_planned) -> infer_dense_kernel
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
    const int n_zero = infer_zero_blocks(z);
    const int n_score = (int)score_table_blocks(g->n_nodes, g->feat_stride);
    hipLaunchKernelGGL(infer_front_kernel, dim3(n_score + n_zero), dim3(256), 0, st, g->X, g->feat_dim, g->feat_stride, W, bias,
                       g->n_nodes, s0, n_score, z);
    PCG_LAUNCH_CHECK();
    return PCG_OK;
}

// PERSIST: tile blockIdx.x, then + gridDim.x, ...; else one tile per workgroup (the run-time shapes: a loop around their
// run-time index arithmetic needs more than the 128 VGPRs a 1024-thread workgroup has - it spilled)
// h_out: NULL, or [B][n_rel * emb] for every row's h_1 | .. | h_R (pcg_embed_set, pcg_embed_new; a.combined is their out_emb).
// No instantiation has scratch with the store in, and none lost occupancy (profiles/r26/kernel_resources.txt).
template <bool WLDS, int F_, int E_, int R_, bool PERSIST>
__global__ void __launch_bounds__(DENSE_THREADS) infer_dense_kernel(const DenseArgs a, int n_tiles, float *__restrict__ h_out) {
    extern __shared__ __align__(16) float sm[];
    int tile = (int)blockIdx.x;                       // (gridDim.x <= n_tiles: every workgroup has a first tile)
    dense_tile_body<WLDS, F_, E_, R_, true, true>(a, tile, sm, nullptr, nullptr, h_out);
    if constexpr (PERSIST) {
        for (tile += (int)gridDim.x; tile < n_tiles; tile += (int)gridDim.x) {
            __syncthreads();                          // (the tile before: its last phase's LDS reads)
            dense_tile_body<WLDS, F_, E_, R_, true, false>(a, tile, sm, nullptr, nullptr, h_out);
        }
    }
}

// WLDS for a forward-only launch: the training kernel's choice, if the K-split partial tiles fit where dcomb / dh_r live
bool infer_wlds(int F, int E, int R) {
    if (!dense_wlds(F, E, R)) return false;
    const int ntile_e = E / 16, kparts = ntile_e <= DENSE_WAVES ? DENSE_WAVES / ntile_e : 1;
    return (int64_t)kparts * TB * E <= (int64_t)(1 + R) * TB * (E + 1);
}

static int infer_blocks(int B) {
    const int n_tiles = (B + TB - 1) / TB;
    const int cus = device_cus(256);
    return n_tiles < cus ? n_tiles : cus;
}

int launch_infer_dense(const DenseArgs &a, int B, hipStream_t st, float *h_out) {
    const int F = a.feat_dim, E = a.emb, R = a.n_rel;
    const bool wlds = infer_wlds(F, E, R);
    const size_t smem = dense_smem_bytes(F, E, R, wlds);
    typedef void (*kern_t)(const DenseArgs, int, float *);
    bool persist = false;                             // (the fixed shapes only: see infer_dense_kernel)
    const kern_t kern = dense_dispatch(F, E, R, wlds, [&persist](auto s) -> kern_t {
        using S = decltype(s);
        persist = S::F != 0;
        return infer_dense_kernel<S::wlds, S::F, S::E, S::R, S::F != 0>;
    });
    if (allow_dynamic_lds(kern, 160 * 1024) != PCG_OK) return PCG_E_LAUNCH;
    const int n_tiles = (B + TB - 1) / TB;
    hipLaunchKernelGGL(kern, dim3(persist ? infer_blocks(B) : n_tiles), dim3(DENSE_THREADS), smem, st, a, n_tiles, h_out);
    PCG_LAUNCH_CHECK();
    return PCG_OK;
}

// the call's workspace (InferCarve, infer.h)
int infer_carve(const pcg_graph_desc *g, int n_slots, bool dense, int32_t emb, int32_t chunk_rows, int64_t list_capacity, InferCarve &c) {
    if (!g || chunk_rows < 1 || list_capacity < 1 || list_capacity >= (1ll << 31)) return PCG_E_ARG;
    if ((dense && (emb < 16 || emb % 16 != 0)) || g->n_rel < 1 || g->n_rel > PCG_MAX_REL || g->feat_dim < 1) return PCG_E_UNSUPPORTED;
    if ((int64_t)g->n_rel * chunk_rows >= (1ll << 31)) return PCG_E_ARG;
    const CarveSizes sz = carve(g, chunk_rows, list_capacity, nullptr, nullptr, nullptr);
    const int64_t R = g->n_rel, B = chunk_rows, F = g->feat_dim;
    c.plan_bytes = sz.plan_bytes;
    c.data = n_slots * sz.plan_bytes;
    int64_t off = c.data + align256(sz.data_bytes);
    auto take = [&](bool present, int64_t bytes) {
        const int64_t o = off;
        if (present) off += align256(bytes);
        return present ? o : -1;
    };
    c.agg = take(dense, 4 * R * B * F);
    c.cnt = take(true, 4 * R * B);
    c.center = take(dense, 8 * B);
    c.total = off;
    return PCG_OK;
}

void infer_zero_regions(ZeroRegions &z, const ChunkDriver &d) {
    const int32_t slot_B[2] = {d.chunk_rows, d.tail()};
    for (int s = 0; s < d.n_slots; ++s) {
        Workspace w;
        carve1(d.g, slot_B[s], d.list_capacity, d.data, &w, d.slot[s]);
        z.p[2 * s] = w.counters;                                  // counters | heads: contiguous (256 + 512 bytes)
        z.n[2 * s] = (reinterpret_cast<unsigned char *>(w.heads) - reinterpret_cast<unsigned char *>(w.counters) + 4 * 8 * 16) / 4;
        z.p[2 * s + 1] = reinterpret_cast<uint32_t *>(w.plan_totals);
        z.n[2 * s + 1] = 64 * ((int64_t)d.g->n_rel * slot_B[s] / 256 + 2) / 4;
    }
}

ChunkDriver infer_driver(const pcg_graph_desc *g, const int32_t *ids, int32_t n, int32_t chunk_rows, int64_t list_capacity,
                         const double *thresholds, const float *s0, int64_t center_off, int n_slots, void *workspace,
                         const InferCarve &c, uint32_t *status, void *stream) {
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    ChunkDriver d;
    d.g = g;
    d.ids = ids;
    d.n = n;
    d.chunk_rows = chunk_rows;
    d.list_capacity = list_capacity;
    d.thresholds = thresholds;
    d.s0 = s0;
    d.center_off = center_off;
    d.n_slots = n_slots;
    d.slot[0] = ws;
    d.slot[1] = n_slots > 1 ? ws + c.plan_bytes : nullptr;
    d.plan_bytes = c.plan_bytes;
    d.data = ws + c.data;
    d.cnt = reinterpret_cast<int32_t *>(ws + c.cnt);
    d.status = status;
    d.st = static_cast<hipStream_t>(stream);
    return d;
}

int infer_dense(const pcg_graph_desc *g, const float *theta, int32_t emb, const int32_t *nodes, int32_t B, const Workspace &w,
                float *agg, const int32_t *cnt, float *out_logits, float *out_center, hipStream_t st, float *out_emb, float *out_rel) {
    DenseExtra x;
    x.chunk_begin = w.chunk_begin;
    x.partial = w.partial;
    x.cnt = cnt;
    x.partial_stride = g->feat_stride;
    DenseArgs a;
    int n_sort_blocks = 0;
    const int rc = dense_args(a, n_sort_blocks, g, theta, emb, nodes, nullptr, B, agg, g->feat_dim, 0.f, 1.f, out_logits, out_center,
                              out_emb, nullptr, nullptr, nullptr, x);
    if (rc != PCG_OK) return rc;
    a.stamps = nullptr;
    return launch_infer_dense(a, B, st, out_rel);
}

// ---- partitioned inference (pcg_infer_chunk_dist, pc-gnn_amd/dist.py) ------------------------------------------------------
// gather.hip
int launch_gather_infer(const FeatTable &t, const GatherOut &out, int32_t n_rows, const Workspace &w, const HaloMap &hm,
                        const float *halo_X, hipStream_t st);

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

}  // namespace pcg

extern "C" {

int64_t pcg_infer_workspace_bytes(const pcg_graph_desc *g, int32_t emb, int32_t chunk_rows, int64_t list_capacity) {
    pcg::InferCarve c;
    const int rc = pcg::infer_carve(g, 2, true, emb, chunk_rows, list_capacity, c);
    return rc != PCG_OK ? rc : c.total;
}

int32_t pcg_infer_blocks(int32_t chunk_rows) { return chunk_rows < 1 ? PCG_E_ARG : pcg::infer_blocks(chunk_rows); }

// pcg_infer_set (out_emb, out_rel NULL, out_logits required by its caller) and pcg_embed_set: a NULL out_logits / out_center goes
// to the workspace's centre scratch (the same lane stores both pairs; nobody reads them)
static int infer_set_impl(const pcg_graph_desc *g, const float *theta, int32_t emb, const int32_t *ids, int32_t n, int32_t chunk_rows,
                          float *s0, const double *thresholds, void *workspace, int64_t list_capacity, float *out_logits,
                          float *out_center, float *out_emb, float *out_rel, uint32_t *status, void *stream) {
    if (!g || !g->X || !theta || !ids || n < 0 || !s0 || !thresholds || !workspace || !status) return PCG_E_ARG;
    if (!out_logits && !out_center && !out_emb && !out_rel) return PCG_E_ARG;
    if (!pcg::infer_table_ok(g)) return PCG_E_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(g->X) & 15u) != 0) return PCG_E_ARG;
    pcg::InferCarve c;
    int rc = pcg::infer_carve(g, 2, true, emb, chunk_rows, list_capacity, c);
    if (rc != PCG_OK) return rc;
    const int F = g->feat_dim, E = emb, R = g->n_rel;
    if (pcg::dense_smem_bytes(F, E, R, pcg::infer_wlds(F, E, R)) > 160 * 1024) return PCG_E_UNSUPPORTED;
    if (n == 0) return PCG_OK;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    float *agg = reinterpret_cast<float *>(ws + c.agg), *center_scratch = reinterpret_cast<float *>(ws + c.center);
    const pcg::ChunkDriver d = pcg::infer_driver(g, ids, n, chunk_rows, list_capacity, thresholds, s0, 0, 2, workspace, c, status, stream);

    // the front: scores || the look-back words of both plan slots
    pcg::ZeroRegions z = {};
    pcg::infer_zero_regions(z, d);
    rc = pcg::launch_infer_front(g, theta + pcg::off_clf(F, E, R), theta + pcg::off_bias(F, E, R), s0, z, d.st);
    if (rc != PCG_OK) return rc;
    return d.run([&](int64_t off, int32_t B, const int32_t *cid, const pcg::Workspace &w) {
        // (w.counters: the first part of the chunk's plan slot)
        const int rc = pcg_gather_lists_planned(g->X, F, g->feat_stride, g->n_nodes, R * B, d.cnt, g, B, d.data, w.counters,
                                                list_capacity, agg, F, status, stream);
        if (rc != PCG_OK) return rc;
        return pcg::infer_dense(g, theta, emb, cid, B, w, agg, d.cnt, out_logits ? out_logits + 2 * off : center_scratch,
                                out_center ? out_center + 2 * off : center_scratch, d.st,
                                out_emb ? out_emb + (int64_t)E * off : nullptr, out_rel ? out_rel + (int64_t)R * E * off : nullptr);
    });
}

int pcg_infer_set(const pcg_graph_desc *g, const float *theta, int32_t emb, const int32_t *ids, int32_t n, int32_t chunk_rows,
                  float *s0, const double *thresholds, void *workspace, int64_t list_capacity, float *out_logits, float *out_center,
                  uint32_t *status, void *stream) {
    if (!out_logits) return PCG_E_ARG;
    return infer_set_impl(g, theta, emb, ids, n, chunk_rows, s0, thresholds, workspace, list_capacity, out_logits, out_center, nullptr,
                          nullptr, status, stream);
}

int pcg_embed_set(const pcg_graph_desc *g, const float *theta, int32_t emb, const int32_t *ids, int32_t n, int32_t chunk_rows,
                  float *s0, const double *thresholds, void *workspace, int64_t list_capacity, float *out_logits, float *out_center,
                  float *out_emb, float *out_rel, uint32_t *status, void *stream) {
    return infer_set_impl(g, theta, emb, ids, n, chunk_rows, s0, thresholds, workspace, list_capacity, out_logits, out_center, out_emb,
                          out_rel, status, stream);
}

int64_t pcg_infer_dist_workspace_bytes(const pcg_graph_desc *g, int32_t emb, int32_t chunk_rows, int64_t list_capacity) {
    pcg::InferCarve c;
    const int rc = pcg::infer_carve(g, 1, true, emb, chunk_rows, list_capacity, c);
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
    if (!pcg::infer_table_ok(g)) return PCG_E_UNSUPPORTED;
    if (((reinterpret_cast<uintptr_t>(g->X) | reinterpret_cast<uintptr_t>(halo_X)) & 15u) != 0) return PCG_E_ARG;
    const int64_t n_local = (int64_t)hi - lo, halo_base = n_local + g->n_pos;
    if (lo < 0 || n_local < 0 || n_table_rows < 0 || n_table_rows > g->n_nodes || halo_base > g->n_nodes) return PCG_E_ARG;
    if (table_slots < 1024 || (table_slots & (table_slots - 1)) != 0 || (g->n_pos > 0 && (!pos_ids || !pos_idx))) return PCG_E_ARG;
    pcg::InferCarve c;
    int rc = pcg::infer_carve(g, 1, true, emb, chunk_rows, list_capacity, c);
    if (rc != PCG_OK) return rc;
    const int F = g->feat_dim, E = emb, R = g->n_rel;
    if (pcg::dense_smem_bytes(F, E, R, pcg::infer_wlds(F, E, R)) > 160 * 1024) return PCG_E_UNSUPPORTED;
    if (B == 0) return PCG_OK;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    float *agg = reinterpret_cast<float *>(ws + c.agg), *center_scratch = reinterpret_cast<float *>(ws + c.center);
    // one chunk of B rows in the one slot (the layout is B's own); centre scores by global id: s0[ids[b] + lo]; lists of global ids
    const pcg::ChunkDriver d = pcg::infer_driver(g, ids, B, B, list_capacity, thresholds, s0, lo, 1, workspace, c, status, stream);

    // front: halo scores (+ the table's on the first chunk) || the look-back words of this chunk's plan layout
    pcg::ZeroRegions z = {};
    pcg::infer_zero_regions(z, d);
    const int n_zero = pcg::infer_zero_blocks(z);
    const int64_t tab_rows = first ? n_table_rows : 0;
    const int n_tab = tab_rows > 0 ? (int)pcg::score_table_blocks(tab_rows, g->feat_stride) : 0;
    const int n_halo = (int)pcg::score_table_blocks(halo_cap, g->feat_stride);
    hipLaunchKernelGGL(pcg::infer_front_dist_kernel, dim3(n_tab + n_halo + n_zero), dim3(256), 0, d.st, g->X, halo_X, g->feat_dim,
                       g->feat_stride, theta + pcg::off_clf(F, E, R), theta + pcg::off_bias(F, E, R), row_gid, tab_rows, halo_ids,
                       (int64_t)halo_cap, s0, n_tab, n_halo, z);
    PCG_LAUNCH_CHECK();
    // gather: ids -> owned / train-pos rows of g->X, fetched rows of the inference halo (its own hash table)
    pcg::HaloMap hm;
    hm.keys = table;
    hm.vals = table + table_slots;
    hm.mask = (uint32_t)(table_slots - 1);
    hm.lo = lo; hm.hi = hi; hm.n_local = (int32_t)n_local;
    hm.pos_ids = pos_ids; hm.pos_idx = pos_idx; hm.n_pos = g->n_pos;
    hm.halo_cap = halo_cap; hm.halo_base = (int32_t)halo_base;
    hm.overflow = counts + 128;
    return d.run([&](int64_t, int32_t, const int32_t *, const pcg::Workspace &w) {
        const int rc = pcg::launch_gather_infer(pcg::feat_table(g), {agg, F, PCG_NORM_COUNT, d.cnt, status}, R * B, w, hm, halo_X, d.st);
        if (rc != PCG_OK) return rc;
        // dense: the centres are local table rows
        return pcg::infer_dense(g, theta, emb, ids, B, w, agg, d.cnt, out_logits, out_center ? out_center : center_scratch, d.st);
    });
}

}  // extern "C"
