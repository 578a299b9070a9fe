// Shared between the GraphSAGE / GCN baselines' entry points (baseline.hip: whole-set inference; baseline_train.hip: the training
// step): the aggregation kernels over the CSR rows read in place, the forward of one 16-centre dense tile with its LDS layout,
// the workspace's head (agg | queue | counter) and the launches both calls make.  baseline.hip's head describes the kernels.
#pragma once
#include "infer.h"

namespace pcg {

constexpr int BL_ROW_MAX = 512;        // CSR degree up to which ONE wave sums a row
constexpr int BL_UNROLL = 4;           // neighbour rows a lanes-per-row group has in flight
constexpr int BL_ROWS_THREADS = 256;
constexpr int BL_LONG_WAVES = 8;
constexpr int BL_LONG_THREADS = BL_LONG_WAVES * PCG_WAVE;
constexpr int BL_DENSE_WAVES = 4;
constexpr int BL_DENSE_THREADS = BL_DENSE_WAVES * PCG_WAVE;

typedef float bl_f4 __attribute__((ext_vector_type(4)));

struct BaselineAgg {
    const float *X;
    int32_t feat_dim, feat_stride;
    int64_t n_nodes;
    const int64_t *indptr;
    const int32_t *indices;
    const int32_t *ids;          // the chunk's centres
    int32_t B;
    int32_t norm, add_self;
    float *agg;                  // [B][feat_stride]
    float *out_agg;              // [B][feat_dim] or null
    int32_t *queue;              // [B]: chunk positions of the long rows, in no particular order
    uint32_t *counter;           // entries in the queue
    uint32_t *status;
};

struct BaselineRow {
    int32_t v;                   // the centre, clamped
    const int32_t *row;          // its CSR row
    int32_t deg;
    bool bad;                    // the id named no node
};

// centre b of the chunk: every index read from memory is clamped before it addresses memory
__device__ __forceinline__ BaselineRow baseline_row(const BaselineAgg &a, int64_t b) {
    BaselineRow r;
    const int32_t id = a.ids[b];
    r.bad = id < 0 || (int64_t)id >= a.n_nodes;
    r.v = id < 0 ? 0 : ((int64_t)id >= a.n_nodes ? (int32_t)(a.n_nodes - 1) : id);
    const int64_t nnz = a.indptr[a.n_nodes];
    int64_t beg = a.indptr[r.v], end = a.indptr[r.v + 1];
    beg = beg < 0 ? 0 : (beg > nnz ? nnz : beg);
    end = end < beg ? beg : (end > nnz ? nnz : end);
    const int64_t deg = end - beg;
    r.deg = deg > (1 << 30) ? (1 << 30) : (int32_t)deg;       // (distinct ids: a row is never longer than the table)
    r.row = a.indices + beg;
    return r;
}

// Group q of Q adds the feature rows of neighbours q, q + Q, q + 2Q, ... in that order: lane `sub` of the group's lpr lanes
// holds the float4 chunks sub (and sub + lpr: NV == 2, rows of more than 256 floats).  BL_UNROLL rows are in flight; every
// load is unconditional (index clamped, the value not added).  found: the centre is in the row; bad: an entry named no node.
template <int NV>
__device__ __forceinline__ void baseline_group_sum(const BaselineAgg &a, const BaselineRow &r, int q, int Q, const int (&chc)[NV],
                                                   bl_f4 (&acc)[NV], bool &found, bool &bad) {
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = bl_f4{0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < r.deg; j0 += Q * BL_UNROLL) {              // (uniform over the workgroup)
        int32_t id[BL_UNROLL];
        bool ok[BL_UNROLL];
#pragma unroll
        for (int u = 0; u < BL_UNROLL; ++u) {
            const int j = j0 + u * Q + q;
            ok[u] = j < r.deg;
            id[u] = r.row[ok[u] ? j : r.deg - 1];
        }
        bl_f4 x[BL_UNROLL][NV];
#pragma unroll
        for (int u = 0; u < BL_UNROLL; ++u) {
            const bool out = id[u] < 0 || (int64_t)id[u] >= a.n_nodes;
            bad = bad || (ok[u] && out);
            found = found || (ok[u] && id[u] == r.v);
            const int32_t idc = id[u] < 0 ? 0 : ((int64_t)id[u] >= a.n_nodes ? (int32_t)(a.n_nodes - 1) : id[u]);
            const float *xr = a.X + (size_t)idc * a.feat_stride;
#pragma unroll
            for (int k = 0; k < NV; ++k) x[u][k] = *reinterpret_cast<const bl_f4 *>(xr + 4 * chc[k]);
        }
#pragma unroll
        for (int u = 0; u < BL_UNROLL; ++u)
#pragma unroll
            for (int k = 0; k < NV; ++k) acc[k] = ok[u] ? acc[k] + x[u][k] : acc[k];
    }
}

// the sum over the groups of a wave (every lane of a group position gets it): a butterfly, the same operands on both sides
template <int NV>
__device__ __forceinline__ void baseline_wave_sum(bl_f4 (&acc)[NV], int lpr) {
    for (int o = lpr; o < PCG_WAVE; o <<= 1)
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            acc[k].x += __shfl_xor(acc[k].x, o);
            acc[k].y += __shfl_xor(acc[k].y, o);
            acc[k].z += __shfl_xor(acc[k].z, o);
            acc[k].w += __shfl_xor(acc[k].w, o);
        }
}

// float4 chunk `ch` of centre b's aggregate from the sum over its row: the centre united with the row when it is not in it
// (graphsage.py:78-79, 214), one division per element by |S| or sqrt |S| (:82-95, :224-231); 0 / 0 = NaN for an empty set
__device__ __forceinline__ void baseline_finish(const BaselineAgg &a, int64_t b, const BaselineRow &r, bool found, bl_f4 total, int ch) {
    int32_t c = r.deg;
    if (a.add_self && !found) {
        total = total + *reinterpret_cast<const bl_f4 *>(a.X + (size_t)r.v * a.feat_stride + 4 * ch);
        c += 1;
    }
    const float den = a.norm == PCG_NORM_SQRT_COUNT ? sqrtf((float)c) : (float)c;
    bl_f4 res;
    res.x = total.x / den;
    res.y = total.y / den;
    res.z = total.z / den;
    res.w = total.w / den;
    *reinterpret_cast<bl_f4 *>(a.agg + (size_t)b * a.feat_stride + 4 * ch) = res;
    if (a.out_agg) {
        float *o = a.out_agg + (size_t)b * a.feat_dim;
        const int f = 4 * ch;
        if (f + 0 < a.feat_dim) o[f + 0] = res.x;
        if (f + 1 < a.feat_dim) o[f + 1] = res.y;
        if (f + 2 < a.feat_dim) o[f + 2] = res.z;
        if (f + 3 < a.feat_dim) o[f + 3] = res.w;
    }
}

template <int NV>
__global__ void __launch_bounds__(BL_ROWS_THREADS) baseline_agg_rows_kernel(const BaselineAgg a) {
    const int lane = lane_id();
    const int nch = a.feat_stride >> 2, lpr = lanes_per_row(a.feat_stride);
    const int G = PCG_WAVE / lpr, g = lane / lpr, sub = lane % lpr;
    int chc[NV];
    bool has[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        has[k] = sub + k * lpr < nch;
        chc[k] = has[k] ? sub + k * lpr : nch - 1;
    }
    const int64_t n_waves = (int64_t)gridDim.x * (BL_ROWS_THREADS / PCG_WAVE);
    for (int64_t b = (int64_t)blockIdx.x * (BL_ROWS_THREADS / PCG_WAVE) + (threadIdx.x >> 6); b < a.B; b += n_waves) {
        const BaselineRow r = baseline_row(a, b);
        if (r.deg > BL_ROW_MAX) {                                     // (wave-uniform) a workgroup's row: baseline_agg_long_kernel
            if (lane == 0) {
                const uint32_t slot = atomicAdd(a.counter, 1u);
                if (slot < (uint32_t)a.B) a.queue[slot] = (int32_t)b;
            }
            continue;
        }
        bl_f4 acc[NV];
        bool found = false, bad = r.bad;
        baseline_group_sum<NV>(a, r, g, G, chc, acc, found, bad);
        baseline_wave_sum<NV>(acc, lpr);
        const bool in_row = __ballot(found) != 0ull;
        if (g == 0)
#pragma unroll
            for (int k = 0; k < NV; ++k)
                if (has[k]) baseline_finish(a, b, r, in_row, acc[k], chc[k]);
        if (__ballot(bad) != 0ull && lane == 0) atomicOr(a.status, (uint32_t)PCG_ST_LIST_ID_RANGE);
    }
}

template <int NV>
__global__ void __launch_bounds__(BL_LONG_THREADS) baseline_agg_long_kernel(const BaselineAgg a) {
    __shared__ __align__(16) float s_part[BL_LONG_WAVES][512];       // a wave's sum of its groups, [feat_stride] each
    __shared__ int s_found;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nch = a.feat_stride >> 2, lpr = lanes_per_row(a.feat_stride);
    const int G = PCG_WAVE / lpr, g = lane / lpr, sub = lane % lpr;
    int chc[NV];
    bool has[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        has[k] = sub + k * lpr < nch;
        chc[k] = has[k] ? sub + k * lpr : nch - 1;
    }
    uint32_t n_long = a.counter[0];
    n_long = n_long < (uint32_t)a.B ? n_long : (uint32_t)a.B;
    for (uint32_t qi = blockIdx.x; qi < n_long; qi += gridDim.x) {
        int32_t b = a.queue[qi];
        b = b < 0 ? 0 : (b >= a.B ? a.B - 1 : b);
        const BaselineRow r = baseline_row(a, b);
        if (tid == 0) s_found = 0;
        __syncthreads();
        bl_f4 acc[NV];
        bool found = false, bad = r.bad;
        baseline_group_sum<NV>(a, r, wave * G + g, BL_LONG_WAVES * G, chc, acc, found, bad);
        baseline_wave_sum<NV>(acc, lpr);
        if (g == 0)
#pragma unroll
            for (int k = 0; k < NV; ++k)
                if (has[k]) *reinterpret_cast<bl_f4 *>(&s_part[wave][4 * chc[k]]) = acc[k];
        if (__ballot(found) != 0ull && lane == 0) atomicOr(&s_found, 1);
        if (__ballot(bad) != 0ull && lane == 0) atomicOr(a.status, (uint32_t)PCG_ST_LIST_ID_RANGE);
        __syncthreads();
        for (int ch = tid; ch < nch; ch += BL_LONG_THREADS) {         // the waves' sums, in wave order
            bl_f4 total = *reinterpret_cast<const bl_f4 *>(&s_part[0][4 * ch]);
#pragma unroll
            for (int w = 1; w < BL_LONG_WAVES; ++w) total = total + *reinterpret_cast<const bl_f4 *>(&s_part[w][4 * ch]);
            baseline_finish(a, b, r, s_found != 0, total, ch);
        }
        __syncthreads();                                              // (s_part, s_found: the next row's)
    }
}

struct BaselineDense {
    const float *X;
    int32_t feat_dim, feat_stride;
    int64_t n_nodes;
    const int32_t *ids;
    int32_t B;
    const float *agg;            // [B][feat_stride]
    int32_t concat_self, emb;
    const float *W_enc;          // [emb][K]
    const float *W_cls;          // [2][emb]
    float *logits;               // [B][2]
    float *out_emb;              // [B][emb] or null
};

// K of the encoder, K padded for the MFMA chains, the waves that share one 16-column tile of h
__host__ __device__ inline int baseline_K(int F, int concat_self) { return concat_self ? 2 * F : F; }
__host__ __device__ inline int baseline_Kp(int K) { return (K + KPAD - 1) / KPAD * KPAD; }
__host__ __device__ inline int baseline_kparts(int E) { return E / 16 <= BL_DENSE_WAVES ? BL_DENSE_WAVES / (E / 16) : 1; }

// LDS of a dense workgroup, in floats: z [16][Kp + 1] | K-split parts [kparts][16][E] | h [16][E + 1] | W_cls [2][E]
// (| W_enc [E][Kp + 1] when staged)
static inline size_t baseline_smem_bytes(int F, int E, int concat_self, bool wlds) {
    const int Kp = baseline_Kp(baseline_K(F, concat_self));
    size_t fl = (size_t)TB * (Kp + 1) + (size_t)baseline_kparts(E) * TB * E + (size_t)TB * (E + 1) + 2 * (size_t)E;
    if (wlds) fl += (size_t)E * (Kp + 1);
    return sizeof(float) * fl;
}
static inline bool baseline_wlds(int F, int E, int concat_self) { return baseline_smem_bytes(F, E, concat_self, true) <= 160 * 1024; }

// relu that lets NaN through (torch's; fmaxf(x, 0) would return 0)
__device__ __forceinline__ float baseline_relu(float x) { return x <= 0.f ? 0.f : x; }

// the LDS of a dense workgroup (baseline_smem_bytes), carved
struct BaselineLds {
    float *z;                    // [TB][Kp + 1]: [self | a] or a, pad columns zero
    float *part;                 // [kparts][TB][E]
    float *h;                    // [TB][E + 1]
    float *wc;                   // [2][E]
    float *w;                    // WLDS: [E][Kp + 1] copy of W_enc, pad columns zero
};
__device__ __forceinline__ BaselineLds baseline_lds(float *sm, int F, int E, int concat_self) {
    const int ldz = baseline_Kp(baseline_K(F, concat_self)) + 1;
    BaselineLds s;
    s.z = sm;
    s.part = s.z + TB * ldz;
    s.h = s.part + baseline_kparts(E) * TB * E;
    s.wc = s.h + TB * (E + 1);
    s.w = s.wc + 2 * E;
    return s;
}

// a workgroup's copies of the weights, made once before its tiles (no barrier here: the first tile's staging barrier covers it)
template <bool WLDS>
__device__ __forceinline__ void baseline_stage_weights(const BaselineDense &a, const BaselineLds &s) {
    const int E = a.emb, K = baseline_K(a.feat_dim, a.concat_self), ldz = baseline_Kp(K) + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if constexpr (WLDS) {
        // rows of odd pitch: lanes of consecutive output columns read distinct banks.  A wave copies a row at a time, lane k its
        // columns k, k + 64, ... (coalesced; K need not be a multiple of 4), zeros in the pad columns
        for (int e = wave; e < E; e += BL_DENSE_WAVES) {
            const float *__restrict__ wrow = a.W_enc + (size_t)e * K;
            for (int k = lane; k < ldz; k += PCG_WAVE) s.w[e * ldz + k] = k < K ? wrow[k] : 0.f;
        }
    }
    for (int i = tid; i < 2 * E; i += BL_DENSE_THREADS) s.wc[i] = a.W_cls[i];
}

// The forward of the 16 centres from chunk row row0 on: s.z and s.h hold the tile's z and h afterwards (rows beyond the chunk:
// z = 0), out_emb is written where asked for, and every lane of the 16 that share centre tid >> 4 returns its two logits.
// The callers' barriers: none is needed before the call for the first tile; a later tile's stores to s.h are two barriers away,
// its stores to s.z behind this tile's MFMA barrier - a caller that reads s.z after the call puts a barrier before the next one.
template <bool WLDS>
__device__ __forceinline__ void baseline_tile_forward(const BaselineDense &a, const BaselineLds &s, int64_t row0, float &logit0,
                                                      float &logit1) {
    const int F = a.feat_dim, E = a.emb;
    const int K = baseline_K(F, a.concat_self), Kp = baseline_Kp(K), ldz = Kp + 1, ldE = E + 1;
    const int ntile_e = E / 16, kparts = baseline_kparts(E);
    float *s_z = s.z, *s_part = s.part, *s_h = s.h;
    const float *s_wc = s.wc, *s_w = s.w;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- stage z: the tile's self rows (ids -> rows, clamped) and aggregates; rows beyond the chunk are zero ----
    // 16 lanes per centre, a float4 of the row per lane and turn (X and agg rows are 16-byte aligned, feat_stride floats
    // apart); only the columns below F are stored
    {
        const int t = tid >> 4, l16 = tid & 15, nch = a.feat_stride >> 2;
        const int zoff = a.concat_self ? F : 0;
        const int64_t b = row0 + t;
        const bool live = b < a.B;
        float *zr = s_z + t * ldz;
        if (a.concat_self) {
            int64_t idc = 0;
            if (live) {
                const int32_t id = a.ids[b];
                idc = id < 0 ? 0 : ((int64_t)id >= a.n_nodes ? a.n_nodes - 1 : (int64_t)id);
            }
            const float *xs = a.X + (size_t)idc * a.feat_stride;
            for (int c4 = l16; c4 < nch; c4 += 16) {
                const bl_f4 v = live ? *reinterpret_cast<const bl_f4 *>(xs + 4 * c4) : bl_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * c4 + j < F) zr[4 * c4 + j] = v[j];
            }
        }
        const float *as = a.agg + (size_t)(live ? b : 0) * a.feat_stride;
        for (int c4 = l16; c4 < nch; c4 += 16) {
            const bl_f4 v = live ? *reinterpret_cast<const bl_f4 *>(as + 4 * c4) : bl_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * c4 + j < F) zr[zoff + 4 * c4 + j] = v[j];
        }
        for (int c = K + l16; c < ldz; c += 16) zr[c] = 0.f;
    }
    __syncthreads();
    // ---- h = relu(W_enc z) (graphsage.py:149, :274): tile ct of 16 columns, its K split over kparts waves ----
    {
        const int ksteps = Kp / 4;
        const int per = ((ksteps + kparts - 1) / kparts + MU - 1) / MU * MU;   // steps per part: a multiple of MU
        const int r = lane & 15, kq = lane >> 4;
        for (int item = wave; item < ntile_e * kparts; item += BL_DENSE_WAVES) {
            const int ct = item % ntile_e, kp = item / ntile_e;
            const int k_lo = kp * per * 4, k_hi = (kp + 1) * per * 4 < Kp ? (kp + 1) * per * 4 : Kp;
            const float *ap = s_z + r * ldz + k_lo + kq;
            f32x4 c;
            if constexpr (WLDS) {
                const float *bp = s_w + (ct * 16 + r) * ldz + k_lo + kq;
                c = mfma_chain((k_hi - k_lo) >> 2, [&](int s) { return ap[4 * s]; }, [&](int s) { return bp[4 * s]; });
            } else {
                // columns k >= K of W_enc do not exist: the load is clamped and a zero takes the value's place, as in the LDS
                // copy - a non-finite weight must not reach the sum through a pad column (0 * Inf), whichever variant runs
                const float *__restrict__ wr = a.W_enc + (size_t)(ct * 16 + r) * K;
                c = mfma_chain((k_hi - k_lo) >> 2, [&](int s) { return ap[4 * s]; },
                               [&](int s) {
                                   const int k = k_lo + 4 * s + kq;
                                   const float w = wr[k < K ? k : K - 1];
                                   return k < K ? w : 0.f;
                               });
            }
            const int col = ct * 16 + r, rq = kq * 4;
#pragma unroll
            for (int i = 0; i < 4; ++i) s_part[(kp * TB + rq + i) * E + col] = c[i];
        }
    }
    __syncthreads();
    for (int i = tid; i < TB * E; i += BL_DENSE_THREADS) {
        const int t = i / E, e = i - t * E;
        float acc = s_part[t * E + e];
        for (int kp = 1; kp < kparts; ++kp) acc += s_part[(kp * TB + t) * E + e];
        const float v = baseline_relu(acc);
        s_h[t * ldE + e] = v;
        const int64_t b = row0 + t;
        if (a.out_emb && b < a.B) a.out_emb[(size_t)b * E + e] = v;
    }
    __syncthreads();
    // ---- logits = W_cls h (graphsage.py:28-31, :167-170): 16 lanes per centre, both classes, DPP row sums ----
    {
        const int t = tid >> 4, part = tid & 15;
        float acc0 = 0.f, acc1 = 0.f;
        for (int e = part; e < E; e += 16) {
            const float h = s_h[t * ldE + e];
            acc0 = fmaf(h, s_wc[e], acc0);
            acc1 = fmaf(h, s_wc[E + e], acc1);
        }
        logit0 = row16_sum(acc0);
        logit1 = row16_sum(acc1);
    }
}

// the call's workspace: agg [chunk][feat_stride] | queue [chunk] | counter.  Nothing in it depends on degrees or edge counts.
struct BaselineCarve {
    int64_t agg, queue, counter, total;
};
static int baseline_carve(const pcg_graph_desc *g, const pcg_baseline_model *m, int32_t chunk_rows, BaselineCarve &c) {
    if (!g || !m || chunk_rows < 1) return PCG_E_ARG;
    if (m->emb < 16 || m->emb % 16 != 0 || !infer_table_ok(g)) return PCG_E_UNSUPPORTED;
    int64_t off = 0;
    c.agg = off;
    off += align256(4 * (int64_t)chunk_rows * g->feat_stride);
    c.queue = off;
    off += align256(4 * (int64_t)chunk_rows);
    c.counter = off;
    off += 256;
    c.total = off;
    return PCG_OK;
}

// what both entry points ask of the graph and the model before anything else (PCG_E_ARG otherwise)
static inline bool baseline_args_ok(const pcg_graph_desc *g, const pcg_baseline_model *m) {
    if (!g || !g->X || !m || !m->W_enc || !m->W_cls) return false;
    if (g->n_rel < 1 || g->n_rel > PCG_MAX_REL || m->rel < 0 || m->rel >= g->n_rel) return false;
    if (m->norm != PCG_NORM_COUNT && m->norm != PCG_NORM_SQRT_COUNT) return false;
    if (!g->indptr[m->rel] || !g->indices[m->rel] || g->n_nodes < 1 || g->n_nodes >= (1ll << 31)) return false;
    return (reinterpret_cast<uintptr_t>(g->X) & 15u) == 0;
}

// the two kernels' arguments but for the chunk's own (ids, B, the outputs): agg, queue and counter are the workspace's
static inline void baseline_fill(const pcg_graph_desc *g, const pcg_baseline_model *m, float *agg, int32_t *queue, uint32_t *counter,
                                 uint32_t *status, BaselineAgg &a, BaselineDense &d) {
    a.X = d.X = g->X;
    a.feat_dim = d.feat_dim = g->feat_dim;
    a.feat_stride = d.feat_stride = g->feat_stride;
    a.n_nodes = d.n_nodes = g->n_nodes;
    a.indptr = g->indptr[m->rel];
    a.indices = g->indices[m->rel];
    a.norm = m->norm;
    a.add_self = m->add_self != 0;
    a.agg = agg;
    a.out_agg = nullptr;
    a.queue = queue;
    a.counter = counter;
    a.status = status;
    d.agg = agg;
    d.concat_self = m->concat_self != 0;
    d.emb = m->emb;
    d.W_enc = m->W_enc;
    d.W_cls = m->W_cls;
    d.logits = nullptr;
    d.out_emb = nullptr;
}

// a chunk's aggregation: counter = 0 -> the rows of up to BL_ROW_MAX neighbours -> the queue of the longer ones
static int launch_baseline_agg(const BaselineAgg &a, hipStream_t st) {
    const bool two = a.feat_stride > 256;                // float4 chunks per lane: 1 covers rows of up to 256 floats
    const int cus = device_cus(256);
    if (hipMemsetAsync(a.counter, 0, sizeof(uint32_t), st) != hipSuccess) return PCG_E_LAUNCH;
    const int64_t row_blocks = ((int64_t)a.B + 3) / 4, row_room = (int64_t)cus * 8;
    const dim3 rows_grid((unsigned)(row_blocks < row_room ? row_blocks : row_room));
    if (two) hipLaunchKernelGGL(baseline_agg_rows_kernel<2>, rows_grid, dim3(BL_ROWS_THREADS), 0, st, a);
    else hipLaunchKernelGGL(baseline_agg_rows_kernel<1>, rows_grid, dim3(BL_ROWS_THREADS), 0, st, a);
    PCG_LAUNCH_CHECK();
    // the long rows: how many there are is known on the device only - a fixed grid strides over the queue
    const dim3 long_grid((unsigned)(a.B < 2 * cus ? a.B : 2 * cus));
    if (two) hipLaunchKernelGGL(baseline_agg_long_kernel<2>, long_grid, dim3(BL_LONG_THREADS), 0, st, a);
    else hipLaunchKernelGGL(baseline_agg_long_kernel<1>, long_grid, dim3(BL_LONG_THREADS), 0, st, a);
    PCG_LAUNCH_CHECK();
    return PCG_OK;
}

// the grid of a dense launch over n_tiles tiles: the workgroups that fit the device at once, striding over the tiles
static inline unsigned baseline_dense_grid(int n_tiles, size_t smem) {
    int per_cu = (int)((size_t)160 * 1024 / smem);
    per_cu = per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu);
    const int64_t room = (int64_t)device_cus(256) * per_cu;
    return (unsigned)(n_tiles < room ? n_tiles : room);
}

}  // namespace pcg
