// Exact input attributions of the gnn logits for gfx950 (FusedPCGNN.attribute).
//
// The gnn path has no bias: h_r = relu([x | a_r] W_r), comb = relu([x | h_1 .. h_R] W_inter), logits = comb W_cls^T.  With the
// selection held fixed every logit is positively homogeneous of degree 1 in (x, a_1 .. a_R), so gradient times input splits the
// attributed scalar s = w0 * logit0 + w1 * logit1 completely (Euler):  s = <x, ds/dx> + sum_r <a_r, ds/da_r>, and - a_r being the
// mean of the chosen rows -  <a_r, ds/da_r> = sum_{j in chosen(r)} <X[j], ds/da_r> / |chosen(r)|.
//
//   pcg_attr_set        : pcg_infer_set's launches (front, then per chunk plan -> select -> gather) with attr_dense_kernel in the
//                         place of infer_dense_kernel: per 16-row tile the forward phases of dense_tile_body, unchanged (the
//                         logits are pcg_infer_set's bit for bit), and - from the LDS state the forward leaves - the backward to
//                         the INPUTS: three phases, a barrier between them
//                           1. dcomb = (w0 W_cls[0] + w1 W_cls[1]) * (comb > 0)
//                           2. dh_r  = (dcomb W_inter[F + rE .., :]^T) * (h_r > 0)   and   dx0 = dcomb W_inter[0 .. F, :]^T
//                           3. dcat_r = dh_r W_r^T   ([16][2F]: columns < F the self part, columns >= F  d s / d a_r)
//                         then d_self = dx0 + sum_r dcat_r[:, :F] (r = 0 .. R-1), d_agg_r = dcat_r[:, F:], and the two inner
//                         products per row, 16 lanes each, a fixed order.  Every GEMM is v_mfma_f32_16x16x4_f32.
//   pcg_attr_neighbours : out[e] = <X[ids[e]], d_agg[r, i]> / len for every entry e of row (r, i) of ranked lists.
// Both launches are exported (attr.h) to pcg_explain_new (explain_new.hip): the dense launch with the self rows of a query
// table, the gather-dot in its two-table form (entry id >= N reads row id - N of the query table: an address, not a value).
//
// A row's results depend on the row alone: no atomics on floats, no workgroup waits for another, every sum in a fixed order.
#include "attr.h"

namespace pcg {

struct AttrArgs {
    float w0, w1;
    float *d_self;              // [B][F]  (the chunk's first row)
    float *d_agg;               // [R][n][F]: relation r of chunk row b at d_agg + r * agg_rstride + b * F
    int64_t agg_rstride;
    float *self_contrib;        // [B]
    float *rel_contrib;         // [R][n]: + r * n_total + b
    int64_t n_total;
};

// floats the backward needs beyond the forward's LDS: dcat [R][TB][2F + 1] lies over the forward's [self | h_r] tile (dead after
// phase 2) and dx0 [TB][F + 1] over `combined` (dead after phase 1) where they fit; what does not fit is appended
__host__ __device__ inline bool attr_dcat_over_cat(int F, int E, int R) {
    const int K2p = (F + R * E + KPAD - 1) / KPAD * KPAD;
    return R * (2 * F + 1) <= K2p + 1;
}
__host__ __device__ inline bool attr_dx0_over_comb(int F, int E) { return F <= E; }
static inline size_t attr_smem_bytes(int F, int E, int R, bool wlds) {
    size_t extra = 0;
    if (!attr_dcat_over_cat(F, E, R)) extra += (size_t)R * TB * (2 * F + 1);
    if (!attr_dx0_over_comb(F, E)) extra += (size_t)TB * (F + 1);
    return dense_smem_bytes(F, E, R, wlds) + sizeof(float) * extra;
}

// out[t][j] = sum_e A[t][e] * W[j][e] for the 16 weight rows this wave's lanes name (lane & 15 -> its row: wl in the LDS copy,
// wg in global memory), e < E: A [TB][lda] in LDS.  E is a multiple of 16.
template <bool WLDS>
__device__ __forceinline__ f32x4 attr_tile_wT(const float *A, int lda, const float *wl, const float *__restrict__ wg, int E, int lane) {
    const int rr = lane & 15, kq = lane >> 4;
    if constexpr (WLDS) {
        const float *ap = A + rr * lda + kq, *bl = wl + kq;
        return mfma_chain(E >> 2, [&](int s) { return ap[4 * s]; }, [&](int s) { return bl[4 * s]; });
    } else {
        // (tile_lds_globT4's k order with four blocks of loads in flight instead of eight: behind the forward's live state the
        //  persistent emb-128 instantiations have no registers for more)
        typedef float f4 __attribute__((ext_vector_type(4)));
        const float *ap = A + rr * lda + 4 * kq, *bp = wg + 4 * kq;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        constexpr int NB = 4;
        const int n_blocks = E >> 4;                                                  // (a multiple of NB or fewer than NB)
        for (int u0 = 0; u0 < n_blocks; u0 += NB) {
            f4 b[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) b[j] = *reinterpret_cast<const f4 *>(bp + 16 * (u0 + j < n_blocks ? u0 + j : n_blocks - 1));
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                if (u0 + j >= n_blocks) break;                                        // (wave-uniform)
                const float *aj = ap + 16 * (u0 + j);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aj[0], b[j].x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aj[1], b[j].y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aj[2], b[j].z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aj[3], b[j].w, acc, 0, 0, 0);
            }
        }
        return acc;
    }
}

// the backward of tile `tile_id`, continuing from the LDS state dense_tile_body<WLDS, F_, E_, R_, true, .> left (and past its
// last barrier)
template <bool WLDS, int F_, int E_, int R_>
__device__ __forceinline__ void attr_tile_backward(const DenseArgs &a, const AttrArgs &x, int tile_id, float *sm) {
    const int F = F_ > 0 ? F_ : a.feat_dim, E = E_ > 0 ? E_ : a.emb, R = R_ > 0 ? R_ : a.n_rel;
    const int K1 = 2 * F, K1p = (K1 + KPAD - 1) / KPAD * KPAD, K2 = F + R * E, K2p = (K2 + KPAD - 1) / KPAD * KPAD;
    const int ld1 = K1p + 1, ld2 = K2p + 1, ldE = E + 1, ldW = E + 4;
    const int ntile_e = E / 16;
    const int kparts = ntile_e <= DENSE_WAVES ? DENSE_WAVES / ntile_e : 1;
    // (the layout of dense_tile_body)
    float *s_wi = sm;
    float *s_wr = s_wi + (WLDS ? K2p * ldW : 0);
    float *s_catr = s_wr + (WLDS ? R * K1p * ldW : kparts * TB * E);
    float *s_cat = s_catr + R * TB * ld1;
    float *s_comb = s_cat + TB * ld2;
    float *s_dcomb = s_comb + TB * ldE;
    float *s_dh = s_dcomb + TB * ldE;
    float *s_wc = s_dh + R * TB * ldE + 4 * TB;
    float *s_end = s_wc + 2 * E + 2 * F + 4 + 4;
    const int ldc = 2 * F + 1, ldx = F + 1;
    const bool dcat_over = attr_dcat_over_cat(F, E, R);
    float *s_dcat = dcat_over ? s_cat : s_end;                                        // [R][TB][ldc]
    float *s_dx0 = attr_dx0_over_comb(F, E) ? s_comb : (dcat_over ? s_end : s_end + R * TB * ldc);   // [TB][ldx]

    // (the thread index through an empty asm: what this function computes from it - per-lane weight row pointers, output
    //  addresses - is then no loop invariant of the persistent tile loop, which would be hoisted out of it and, at 128 VGPRs
    //  per lane, spilled)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = tile_id * TB;
    const int rr = lane & 15, kq = lane >> 4;

    // ---- 1: dcomb = (w0 W_cls[0] + w1 W_cls[1]) * relu'(combined) ----------------------------------------------------------
    for (int i = tid; i < TB * E; i += DENSE_THREADS) {
        const int t = i / E, e = i - t * E;
        const float g = x.w0 * s_wc[e] + x.w1 * s_wc[E + e];
        s_dcomb[t * ldE + e] = s_comb[t * ldE + e] > 0.f ? g : 0.f;
    }
    __syncthreads();
    // ---- 2: dh_r = (dcomb W_inter[F + rE .., :]^T) * relu'(h_r) for every r, and dx0 = dcomb W_inter[0 .. F, :]^T -----------
    {
        const int n_dh = R * ntile_e, ntf = (F + 15) / 16;
        for (int tile = wave; tile < n_dh + ntf; tile += DENSE_WAVES) {
            if (tile < n_dh) {
                const int r = tile / ntile_e, ct = tile - r * ntile_e;
                const int j = F + r * E + ct * 16 + rr;
                const f32x4 acc = attr_tile_wT<WLDS>(s_dcomb, ldE, s_wi + j * ldW, a.W_inter + (size_t)j * E, E, lane);
                const int col = ct * 16 + rr, rq = kq * 4;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    s_dh[(r * TB + rq + i) * ldE + col] = s_cat[(rq + i) * ld2 + F + r * E + col] > 0.f ? acc[i] : 0.f;
            } else {
                const int ct = tile - n_dh;
                const int col = ct * 16 + rr, j = col < F ? col : F - 1;            // (clamped: the surplus is discarded)
                const f32x4 acc = attr_tile_wT<WLDS>(s_dcomb, ldE, s_wi + j * ldW, a.W_inter + (size_t)j * E, E, lane);
                const int rq = kq * 4;
                if (col < F) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) s_dx0[(rq + i) * ldx + col] = acc[i];
                }
            }
        }
    }
    __syncthreads();
    // ---- 3: dcat_r = dh_r W_r^T, [TB][2F] --------------------------------------------------------------------------------------
    {
        const int nt1 = (K1 + 15) / 16;
        const float *w_intra = a.W_inter + (size_t)K2 * E;                              // W_intra[0 .. R): contiguous behind W_inter
        for (int tile = wave; tile < R * nt1; tile += DENSE_WAVES) {
            const int r = tile / nt1, ct = tile - r * nt1;
            const int col = ct * 16 + rr, j = col < K1 ? col : K1 - 1;
            const f32x4 acc = attr_tile_wT<WLDS>(s_dh + r * TB * ldE, ldE, s_wr + (r * K1p + j) * ldW, w_intra + ((size_t)r * K1 + j) * E, E, lane);
            const int rq = kq * 4;
            if (col < K1) {
#pragma unroll
                for (int i = 0; i < 4; ++i) s_dcat[(r * TB + rq + i) * ldc + col] = acc[i];
            }
        }
    }
    __syncthreads();
    // ---- out: d_self = dx0 + sum_r dcat_r[:, :F] (r ascending), d_agg_r = dcat_r[:, F:]; the tile's rows are contiguous ---------
    const int rows_here = a.B - row0 < TB ? a.B - row0 : TB;
    for (int i = tid; i < rows_here * F; i += DENSE_THREADS) {
        const int t = i / F, f = i - t * F;
        float ds = s_dx0[t * ldx + f];
        for (int r = 0; r < R; ++r) ds += s_dcat[(r * TB + t) * ldc + f];
        x.d_self[(size_t)row0 * F + i] = ds;
    }
    for (int i = tid; i < R * rows_here * F; i += DENSE_THREADS) {
        const int r = i / (rows_here * F), j = i - r * rows_here * F, t = j / F, f = j - t * F;
        x.d_agg[(size_t)r * x.agg_rstride + (size_t)row0 * F + j] = s_dcat[(r * TB + t) * ldc + F + f];
    }
    // the inner products: wave t has row t; 16 lanes per product (f = part, part + 16, ..: an fma chain), a DPP row sum
    {
        const int t = wave, part = lane & 15, b = row0 + t;
        for (int q = lane >> 4; q < 1 + R; q += 4) {
            float acc = 0.f;
            if (q == 0) {
                for (int f = part; f < F; f += 16) {
                    float ds = s_dx0[t * ldx + f];
                    for (int r = 0; r < R; ++r) ds += s_dcat[(r * TB + t) * ldc + f];
                    acc = fmaf(s_catr[t * ld1 + f], ds, acc);
                }
            } else {
                const int r = q - 1;
                for (int f = part; f < F; f += 16) acc = fmaf(s_catr[(r * TB + t) * ld1 + F + f], s_dcat[(r * TB + t) * ldc + F + f], acc);
            }
            acc = row16_sum(acc);
            if (part == 0 && b < a.B) {
                if (q == 0) x.self_contrib[b] = acc;
                else x.rel_contrib[(size_t)(q - 1) * x.n_total + b] = acc;
            }
        }
    }
}

// PERSIST as infer_dense_kernel's: tile blockIdx.x, then + gridDim.x, ...; else one tile per workgroup (the run-time shapes)
template <bool WLDS, int F_, int E_, int R_, bool PERSIST>
__global__ void __launch_bounds__(DENSE_THREADS) attr_dense_kernel(const DenseArgs a, const AttrArgs x, int n_tiles) {
    extern __shared__ __align__(16) float sm[];
    int tile = (int)blockIdx.x;
    dense_tile_body<WLDS, F_, E_, R_, true, true>(a, tile, sm);
    attr_tile_backward<WLDS, F_, E_, R_>(a, x, tile, sm);
    if constexpr (PERSIST) {
        for (tile += (int)gridDim.x; tile < n_tiles; tile += (int)gridDim.x) {
            __syncthreads();                          // (the tile before: its last phase's LDS reads)
            dense_tile_body<WLDS, F_, E_, R_, true, false>(a, tile, sm);
            attr_tile_backward<WLDS, F_, E_, R_>(a, x, tile, sm);
        }
    }
}

bool attr_shape_ok(int F, int E, int R) { return attr_smem_bytes(F, E, R, infer_wlds(F, E, R)) <= 160 * 1024; }

static int launch_attr_dense(const DenseArgs &a, const AttrArgs &x, int B, hipStream_t st) {
    const int F = a.feat_dim, E = a.emb, R = a.n_rel;
    const bool wlds = infer_wlds(F, E, R);            // (the forward's own choice: the logits are pcg_infer_set's)
    const size_t smem = attr_smem_bytes(F, E, R, wlds);
    typedef void (*kern_t)(const DenseArgs, const AttrArgs, int);
    bool persist = false;
    const kern_t kern = dense_dispatch(F, E, R, wlds, [&persist](auto s) -> kern_t {
        using S = decltype(s);
        persist = S::F != 0;
        return attr_dense_kernel<S::wlds, S::F, S::E, S::R, S::F != 0>;
    });
    if (allow_dynamic_lds(kern, 160 * 1024) != PCG_OK) return PCG_E_LAUNCH;
    const int n_tiles = (B + TB - 1) / TB;
    const int blocks = persist ? pcg_infer_blocks(B) : n_tiles;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(DENSE_THREADS), smem, st, a, x, n_tiles);
    PCG_LAUNCH_CHECK();
    return PCG_OK;
}

// ---- the chosen neighbours' shares ---------------------------------------------------------------------------------------------
// Row (r, i) of the ranked lists has len = off[row + 1] - off[row] entries; out[e] = <X[ids[e]], d_agg[row]> / len.  An entry's dot
// product is formed by lanes_per_row(feat_stride) lanes: lane `sub` holds the float4 chunks sub, sub + lpr of d_agg[row] in
// registers (zero beyond F) and reads the same chunks of X[id] (16 bytes each), one fma chain over them, score_reduce over the
// group - whatever group, wave or workgroup the entry lands in, the same operations in the same order.
// Geometry: grid (x, y).  y == 0: a lane group per row, its entries [0, SHORT) in turn (the whole row when the launch has no
// tail slices).  y >= 1 (only when the graph's max_degree exceeds SHORT): tail slice y - 1 of n_tail of every row longer than
// SHORT, the wave's groups striding over the slice - a hub's thousands of entries are spread over n_tail workgroups.
constexpr int NEIGH_SHORT = 128, NEIGH_SLICE = 256, NEIGH_MAX_TAIL = 15, NEIGH_THREADS = 256, NEIGH_U = 4;

struct NeighArgs {
    const float *X;
    int32_t F, stride;
    int64_t n_nodes;            // rows an id may name (TWO: base + query rows)
    const float *Xq;            // TWO: the query table, row id - n_base for id >= n_base
    int64_t n_base;
    const int64_t *off;         // [rows + 1]
    const int32_t *ids;         // [off[rows]]
    int64_t rows;               // R * n
    const float *d_agg;         // [rows][F]
    float *out;                 // [off[rows]]
    uint32_t *status;
    int32_t n_tail;
};

// entries first, first + step, .. < last of a row that begins at `lo` and has `len` entries (all uniform over the lane group).
// TWO: ids of the base table and of the query table behind it (gather_chunks_two's form: the clamped id in a register,
// id - n_base >= 0 picks between two addresses formed from it, the row loads unconditional either way)
template <bool TWO>
__device__ __forceinline__ void neigh_span(const NeighArgs &a, const float (&d)[2][4], const bool (&has)[2], const int (&chc)[2],
                                           int64_t lo, int64_t len, int64_t first, int64_t last, int step, int sub, int lpr) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const float flen = (float)len;
    for (int64_t e0 = first; e0 < last; e0 += (int64_t)NEIGH_U * step) {
        int32_t id[NEIGH_U];
        bool bad = false;
        // (every load of the batch is in flight before the first product: indices clamped, the surplus not stored)
#pragma unroll
        for (int u = 0; u < NEIGH_U; ++u) {
            const int64_t e = e0 + (int64_t)u * step;
            id[u] = a.ids[lo + (e < last ? e : last - 1)];
        }
        f4 xv[NEIGH_U][2];
#pragma unroll
        for (int u = 0; u < NEIGH_U; ++u) {
            const bool oob = id[u] < 0 || (int64_t)id[u] >= a.n_nodes;
            bad = bad || (oob && e0 + (int64_t)u * step < last);
            const int64_t idc = id[u] < 0 ? 0 : ((int64_t)id[u] >= a.n_nodes ? a.n_nodes - 1 : (int64_t)id[u]);
            const float *xr = a.X + (size_t)idc * a.stride;
            if constexpr (TWO) {
                const int64_t qr = idc - a.n_base;
                xr = qr >= 0 ? a.Xq + (size_t)qr * a.stride : xr;
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) xv[u][k] = *reinterpret_cast<const f4 *>(xr + 4 * chc[k]);
        }
#pragma unroll
        for (int u = 0; u < NEIGH_U; ++u) {
            float p = 0.f;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (has[k]) {
                    p = fmaf(xv[u][k].x, d[k][0], p);
                    p = fmaf(xv[u][k].y, d[k][1], p);
                    p = fmaf(xv[u][k].z, d[k][2], p);
                    p = fmaf(xv[u][k].w, d[k][3], p);
                }
            }
            p = score_reduce(p, lpr);
            const int64_t e = e0 + (int64_t)u * step;
            if (sub == 0 && e < last) a.out[lo + e] = p / flen;
        }
        if (bad && sub == 0 && a.status) atomicOr(a.status, (uint32_t)PCG_ST_LIST_ID_RANGE);
    }
}

// this lane's chunks of d_agg[row] (row < a.rows)
__device__ __forceinline__ void neigh_load_d(const NeighArgs &a, int64_t row, float (&d)[2][4], const bool (&has)[2], const int (&chc)[2]) {
    const float *dr = a.d_agg + (size_t)row * a.F;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int f = 4 * chc[k] + j;
            const float v = dr[f < a.F ? f : a.F - 1];
            d[k][j] = (has[k] && f < a.F) ? v : 0.f;
        }
}

template <bool TWO>
__global__ void __launch_bounds__(NEIGH_THREADS) attr_neigh_kernel(const NeighArgs a) {
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int lpr = lanes_per_row(a.stride), rpw = PCG_WAVE / lpr;
    const int grp = lane / lpr, sub = lane - grp * lpr;
    const int nch = a.stride >> 2;
    bool has[2];
    int chc[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int ch = sub + k * lpr;
        has[k] = ch < nch;
        chc[k] = has[k] ? ch : nch - 1;
    }
    const int64_t wave_global = (int64_t)blockIdx.x * (NEIGH_THREADS / PCG_WAVE) + wave;
    const int64_t row = wave_global * rpw + grp;
    const bool have = row < a.rows;
    const int64_t rc = have ? row : a.rows - 1;
    // every offset is device data: a row is taken only if 0 <= lo <= hi <= total
    const int64_t total = a.off[a.rows], lo = a.off[rc], hi = a.off[rc + 1];
    const bool ok = have && lo >= 0 && hi >= lo && hi <= total;
    const int64_t len = ok ? hi - lo : 0;
    float d[2][4];
    if (blockIdx.y == 0) {
        if (have && !ok && sub == 0 && a.status) atomicOr(a.status, (uint32_t)PCG_ST_RANK_MISMATCH);
        const int64_t n_e = (a.n_tail > 0 && len > NEIGH_SHORT) ? NEIGH_SHORT : len;
        if (n_e <= 0) return;
        neigh_load_d(a, rc, d, has, chc);
        neigh_span<TWO>(a, d, has, chc, lo, len, 0, n_e, 1, sub, lpr);
        return;
    }
    if (__ballot(len > NEIGH_SHORT) == 0ull) return;
    const int slice = (int)blockIdx.y - 1;
    for (int q = 0; q < rpw; ++q) {
        const int64_t len_q = __shfl(len, q * lpr), lo_q = __shfl(lo, q * lpr);       // (wave-uniform)
        if (len_q <= NEIGH_SHORT) continue;
        const int64_t per = (len_q - NEIGH_SHORT + a.n_tail - 1) / a.n_tail;
        const int64_t first = NEIGH_SHORT + (int64_t)slice * per;
        const int64_t last = first + per < len_q ? first + per : len_q;
        // (a group beyond the slice runs an empty span: no lane leaves the loop body's common path)
        neigh_load_d(a, wave_global * rpw + q, d, has, chc);
        neigh_span<TWO>(a, d, has, chc, lo_q, len_q, first + grp, last > first ? last : first, rpw, sub, lpr);
    }
}

// (attr.h) the attribution dense launch of a chunk
int attr_chunk(const pcg_graph_desc *g, const float *theta, int32_t emb, const int32_t *cid, int32_t B, const Workspace &w, float *agg,
               const int32_t *cnt, int64_t off, int32_t n, float w0, float w1, float *out_logits, float *center_scratch,
               float *out_d_self, float *out_d_agg, float *out_self_contrib, float *out_rel_contrib, hipStream_t st) {
    const int F = g->feat_dim;
    DenseExtra ex;
    ex.chunk_begin = w.chunk_begin;
    ex.partial = w.partial;
    ex.cnt = cnt;
    ex.partial_stride = g->feat_stride;
    DenseArgs a;
    int n_sort_blocks = 0;
    const int rc = dense_args(a, n_sort_blocks, g, theta, emb, cid, nullptr, B, agg, F, 0.f, 1.f, out_logits + 2 * off, center_scratch,
                              nullptr, nullptr, nullptr, nullptr, ex);
    if (rc != PCG_OK) return rc;
    a.stamps = nullptr;
    AttrArgs x;
    x.w0 = w0;
    x.w1 = w1;
    x.d_self = out_d_self + (size_t)off * F;
    x.d_agg = out_d_agg + (size_t)off * F;
    x.agg_rstride = (int64_t)n * F;
    x.self_contrib = out_self_contrib + off;
    x.rel_contrib = out_rel_contrib + off;
    x.n_total = n;
    return launch_attr_dense(a, x, B, st);
}

// (attr.h) the gather-dot launch
int launch_attr_neigh(const float *X, int64_t base_rows, const float *query_X, int64_t query_rows, int32_t feat_dim,
                      int32_t feat_stride, int32_t max_degree, const int64_t *flat_offsets, const int32_t *ids, int64_t rows,
                      const float *d_agg, float *out, uint32_t *status, hipStream_t st) {
    NeighArgs a;
    a.X = X;
    a.F = feat_dim;
    a.stride = feat_stride;
    a.n_nodes = base_rows + query_rows;
    a.Xq = query_X;
    a.n_base = base_rows;
    a.off = flat_offsets;
    a.ids = ids;
    a.rows = rows;
    a.d_agg = d_agg;
    a.out = out;
    a.status = status;
    const int64_t over = (int64_t)max_degree - NEIGH_SHORT;
    const int64_t tail = over > 0 ? (over + NEIGH_SLICE - 1) / NEIGH_SLICE : 0;
    a.n_tail = (int32_t)(tail < NEIGH_MAX_TAIL ? tail : NEIGH_MAX_TAIL);
    const int rows_per_block = (NEIGH_THREADS / PCG_WAVE) * (PCG_WAVE / lanes_per_row(a.stride));
    const int64_t blocks = (a.rows + rows_per_block - 1) / rows_per_block;
    if (blocks >= (1ll << 31)) return PCG_E_ARG;
    const dim3 grid((unsigned)blocks, (unsigned)(1 + a.n_tail));
    if (query_X) hipLaunchKernelGGL(attr_neigh_kernel<true>, grid, dim3(NEIGH_THREADS), 0, st, a);
    else hipLaunchKernelGGL(attr_neigh_kernel<false>, grid, dim3(NEIGH_THREADS), 0, st, a);
    PCG_LAUNCH_CHECK();
    return PCG_OK;
}

}  // namespace pcg

extern "C" {

int pcg_attr_set(const pcg_graph_desc *g, const float *theta, int32_t emb, const int32_t *ids, int32_t n, int32_t chunk_rows,
                 float *s0, const double *thresholds, void *workspace, int64_t list_capacity, float w0, float w1, float *out_logits,
                 float *out_d_self, float *out_d_agg, float *out_self_contrib, float *out_rel_contrib, uint32_t *status,
                 void *stream) {
    if (!g || !g->X || !theta || !ids || n < 0 || !s0 || !thresholds || !workspace || !out_logits || !status) return PCG_E_ARG;
    if (!out_d_self || !out_d_agg || !out_self_contrib || !out_rel_contrib) return PCG_E_ARG;
    if (!(w0 - w0 == 0.f) || !(w1 - w1 == 0.f)) return PCG_E_ARG;                    // (finite)
    if (!pcg::infer_table_ok(g)) return PCG_E_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(g->X) & 15u) != 0) return PCG_E_ARG;
    pcg::InferCarve c;
    int rc = pcg::infer_carve(g, 2, true, emb, chunk_rows, list_capacity, c);
    if (rc != PCG_OK) return rc;
    const int F = g->feat_dim, E = emb, R = g->n_rel;
    if (!pcg::attr_shape_ok(F, E, R)) return PCG_E_UNSUPPORTED;
    if (n == 0) return PCG_OK;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    float *agg = reinterpret_cast<float *>(ws + c.agg), *center_scratch = reinterpret_cast<float *>(ws + c.center);
    const pcg::ChunkDriver d = pcg::infer_driver(g, ids, n, chunk_rows, list_capacity, thresholds, s0, 0, 2, workspace, c, status, stream);

    pcg::ZeroRegions z = {};
    pcg::infer_zero_regions(z, d);
    rc = pcg::launch_infer_front(g, theta + pcg::off_clf(F, E, R), theta + pcg::off_bias(F, E, R), s0, z, d.st);
    if (rc != PCG_OK) return rc;
    return d.run([&](int64_t off, int32_t B, const int32_t *cid, const pcg::Workspace &w) {
        int rc = pcg_gather_lists_planned(g->X, F, g->feat_stride, g->n_nodes, R * B, d.cnt, g, B, d.data, w.counters, list_capacity,
                                          agg, F, status, stream);
        if (rc != PCG_OK) return rc;
        return pcg::attr_chunk(g, theta, emb, cid, B, w, agg, d.cnt, off, n, w0, w1, out_logits, center_scratch, out_d_self, out_d_agg,
                               out_self_contrib, out_rel_contrib, d.st);
    });
}

int pcg_attr_neighbours(const pcg_graph_desc *g, const int64_t *flat_offsets, const int32_t *ids, int32_t n_rel, int32_t n,
                        const float *d_agg, float *out, uint32_t *status, void *stream) {
    if (!g || !g->X || !flat_offsets || n_rel < 1 || n_rel > PCG_MAX_REL || n < 0 || !status) return PCG_E_ARG;
    if (!pcg::infer_table_ok(g) || g->n_nodes < 1) return PCG_E_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(g->X) & 15u) != 0) return PCG_E_ARG;
    if (n == 0) return PCG_OK;
    if (!ids || !d_agg || !out) return PCG_E_ARG;
    return pcg::launch_attr_neigh(g->X, g->n_nodes, nullptr, 0, g->feat_dim, g->feat_stride, g->max_degree, flat_offsets, ids,
                                  (int64_t)n_rel * n, d_agg, out, status, static_cast<hipStream_t>(stream));
}

}  // extern "C"
