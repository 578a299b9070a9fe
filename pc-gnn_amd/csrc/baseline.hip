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

template <bool WLDS>
__global__ void __launch_bounds__(BL_DENSE_THREADS) baseline_dense_kernel(const BaselineDense a, int n_tiles) {
    extern __shared__ __align__(16) float sm[];
    const int F = a.feat_dim, E = a.emb;
    const int K = baseline_K(F, a.concat_self), Kp = baseline_Kp(K), ldz = Kp + 1, ldE = E + 1;
    const int ntile_e = E / 16, kparts = baseline_kparts(E);
    float *s_z = sm;                                  // [TB][ldz]: [self | a] or a, pad columns zero
    float *s_part = s_z + TB * ldz;                   // [kparts][TB][E]
    float *s_h = s_part + kparts * TB * E;            // [TB][ldE]
    float *s_wc = s_h + TB * ldE;                     // [2][E]
    float *s_w = s_wc + 2 * E;                        // WLDS: [E][ldz] copy of W_enc, pad columns zero
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    if constexpr (WLDS) {
        // rows of odd pitch: lanes of consecutive output columns read distinct banks.  A wave copies a row at a time, lane k its
        // columns k, k + 64, ... (coalesced; K need not be a multiple of 4), zeros in the pad columns
        for (int e = wave; e < E; e += BL_DENSE_WAVES) {
            const float *__restrict__ wrow = a.W_enc + (size_t)e * K;
            for (int k = lane; k < ldz; k += PCG_WAVE) s_w[e * ldz + k] = k < K ? wrow[k] : 0.f;
        }
    }
    for (int i = tid; i < 2 * E; i += BL_DENSE_THREADS) s_wc[i] = a.W_cls[i];

    for (int tile = (int)blockIdx.x; tile < n_tiles; tile += (int)gridDim.x) {
        const int64_t row0 = (int64_t)tile * TB;
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
            acc0 = row16_sum(acc0);
            acc1 = row16_sum(acc1);
            const int64_t b = row0 + t;
            if (part == 0 && b < a.B) {
                a.logits[2 * b] = acc0;
                a.logits[2 * b + 1] = acc1;
            }
        }
        // (the next tile's first store to s_h is two barriers away, its stores to s_z are behind this tile's MFMA barrier)
    }
}

static int baseline_cus() {
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

template <bool WLDS>
static int launch_baseline_dense(const BaselineDense &a, size_t smem, hipStream_t st) {
    static bool attr_done[64] = {false};                      // per device: the attribute belongs to a device's copy of the kernel
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return PCG_E_LAUNCH;
    const bool known = dev >= 0 && dev < 64;
    if (!known || !attr_done[dev]) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(baseline_dense_kernel<WLDS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024) != hipSuccess)
            return PCG_E_LAUNCH;
        if (known) attr_done[dev] = true;
    }
    const int n_tiles = (int)(((int64_t)a.B + TB - 1) / TB);
    int per_cu = (int)((size_t)160 * 1024 / smem);
    per_cu = per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu);
    const int64_t room = (int64_t)baseline_cus() * per_cu;
    hipLaunchKernelGGL(baseline_dense_kernel<WLDS>, dim3((unsigned)(n_tiles < room ? n_tiles : room)), dim3(BL_DENSE_THREADS), smem, st,
                       a, n_tiles);
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
    if (!g || !g->X || !m || !m->W_enc || !m->W_cls || !ids || !workspace || !status || !out_logits) return PCG_E_ARG;
    if (n < 0 || chunk_rows < 1 || g->n_rel < 1 || g->n_rel > PCG_MAX_REL || m->rel < 0 || m->rel >= g->n_rel) return PCG_E_ARG;
    if (m->norm != PCG_NORM_COUNT && m->norm != PCG_NORM_SQRT_COUNT) return PCG_E_ARG;
    if (!g->indptr[m->rel] || !g->indices[m->rel] || g->n_nodes < 1 || g->n_nodes >= (1ll << 31)) return PCG_E_ARG;
    if ((reinterpret_cast<uintptr_t>(g->X) & 15u) != 0) return PCG_E_ARG;
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
    a.X = g->X;
    a.feat_dim = F;
    a.feat_stride = g->feat_stride;
    a.n_nodes = g->n_nodes;
    a.indptr = g->indptr[m->rel];
    a.indices = g->indices[m->rel];
    a.norm = m->norm;
    a.add_self = m->add_self != 0;
    a.agg = reinterpret_cast<float *>(ws + c.agg);
    a.queue = reinterpret_cast<int32_t *>(ws + c.queue);
    a.counter = reinterpret_cast<uint32_t *>(ws + c.counter);
    a.status = status;
    pcg::BaselineDense d;
    d.X = g->X;
    d.feat_dim = F;
    d.feat_stride = g->feat_stride;
    d.n_nodes = g->n_nodes;
    d.agg = a.agg;
    d.concat_self = concat;
    d.emb = E;
    d.W_enc = m->W_enc;
    d.W_cls = m->W_cls;
    const bool two = g->feat_stride > 256;               // float4 chunks per lane: 1 covers rows of up to 256 floats
    const int cus = pcg::baseline_cus();
    for (int64_t off = 0; off < n; off += chunk_rows) {
        const int32_t B = (int32_t)(n - off < chunk_rows ? n - off : chunk_rows);
        a.ids = d.ids = ids + off;
        a.B = d.B = B;
        a.out_agg = out_agg ? out_agg + off * F : nullptr;
        d.logits = out_logits + 2 * off;
        d.out_emb = out_emb ? out_emb + off * E : nullptr;
        if (hipMemsetAsync(a.counter, 0, sizeof(uint32_t), st) != hipSuccess) return PCG_E_LAUNCH;
        const int64_t row_blocks = ((int64_t)B + 3) / 4, row_room = (int64_t)cus * 8;
        const dim3 rows_grid((unsigned)(row_blocks < row_room ? row_blocks : row_room));
        if (two) hipLaunchKernelGGL(pcg::baseline_agg_rows_kernel<2>, rows_grid, dim3(pcg::BL_ROWS_THREADS), 0, st, a);
        else hipLaunchKernelGGL(pcg::baseline_agg_rows_kernel<1>, rows_grid, dim3(pcg::BL_ROWS_THREADS), 0, st, a);
        PCG_LAUNCH_CHECK();
        // the long rows: how many there are is known on the device only - a fixed grid strides over the queue
        const dim3 long_grid((unsigned)(B < 2 * cus ? B : 2 * cus));
        if (two) hipLaunchKernelGGL(pcg::baseline_agg_long_kernel<2>, long_grid, dim3(pcg::BL_LONG_THREADS), 0, st, a);
        else hipLaunchKernelGGL(pcg::baseline_agg_long_kernel<1>, long_grid, dim3(pcg::BL_LONG_THREADS), 0, st, a);
        PCG_LAUNCH_CHECK();
        const int rc2 = wlds ? pcg::launch_baseline_dense<true>(d, smem, st) : pcg::launch_baseline_dense<false>(d, smem, st);
        if (rc2 != PCG_OK) return rc2;
    }
    return PCG_OK;
}

}  // extern "C"
