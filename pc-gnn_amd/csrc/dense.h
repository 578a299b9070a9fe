// Device side of the dense step: argument block, MFMA tile helpers and the body of one 16-row tile's workgroup.  Shared by
// dense.hip (dense_step_kernel) and select.hip (dense_select_kernel: the tiles of batch t beside the selection of batch t + 1).
#pragma once
#include "choose.h"
#include "launch.h"
#include "wgrad.h"

namespace pcg {


typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TB = 16;          // batch rows per workgroup (one MFMA M-tile)
constexpr int DENSE_WAVES = 16;
constexpr int DENSE_THREADS = DENSE_WAVES * PCG_WAVE;
constexpr int WSTAGE = 8;       // weight float4 loads in flight per thread while staging

struct DenseArgs {
    const float *X;
    int32_t feat_dim, feat_stride, n_rel, emb;
    const int32_t *ids;
    const int32_t *labels;      // null => inference (no loss, no gradients)
    int32_t B;
    const float *agg;           // [R, B, agg_stride]
    int32_t agg_stride;
    // optional: rows of more than one gather chunk are summed here from the gather's partial sums (no combine launch)
    const int32_t *chunk_begin; // [R * B + 1] or null (agg is complete)
    const float *partial;       // [chunks, partial_stride]
    const int32_t *cnt;         // [R * B]
    int32_t partial_stride;
    const float *W_cls;         // [2, E]
    const float *W_inter;       // [F + R*E, E]
    const float *W_intra[PCG_MAX_REL];  // [2F, E]
    const float *W_clf;         // [2, F]
    const float *b_clf;         // [2]
    float lambda_1, inv_count;
    float *logits;              // [B, 2]
    float *center;              // [B, 2]
    float *combined;            // [B, E] or null
    float *row_loss;            // [B] or null
    float *slabs;               // [n_tiles, n_params] or null
    float *acts;                // [wgrad_act_rows][act_ld] or null: the step's activations / activation gradients, transposed
    int32_t act_ld;             //   (wgrad.h) INSTEAD of weight-gradient slabs - the weight gradients are GEMMs of a later launch
    int64_t n_params;
    int32_t *step_counter;      // incremented once per training launch (Adam's t), or null
    int32_t n_split;            // training: workgroups per 16-row tile; they all run the forward pass, the weight-gradient tiles are dealt out
    // optional: Adam for the label classifier's parameters by the workgroup whose gradient arrives last
    float *theta, *m, *v;       // null => off
    uint32_t *ticket;           // device word, 0 between launches
    uint32_t *staged;           // device word, 0 between launches: workgroups that take no ticket (sp != 0) and have read the classifier
    uint32_t *pending;          // two device words: [0] = 1 "the slabs hold a gradient not yet applied to the other parameters", [1] = its slab count
    AdamHyper h;
    unsigned long long *stamps; // diagnostic only (pcg_debug_set_dense_stamps): [tiles][16] wall-clock ticks, else null
    // optional riders: the NEXT step's train-pos sort (rank sort of the unsorted keys the gather launch before this one formed), by
    // workgroups behind the tiles' - only when tiles and sort together leave no CU with two workgroups (a batch of <= ~3000 rows)
    const uint64_t *sort_raw;   // null: off
    uint64_t *sort_out;
    int32_t sort_n, sort_cap, n_tile_blocks;
};
constexpr int DENSE_SORT_TILE = 4096;     // keys per LDS tile of the riding sort (32 KB of the launch's dynamic LDS)
#define DENSE_STAMP(slot) do { if (a.stamps && threadIdx.x == 0 && sp == 0) a.stamps[(size_t)tile_id * 16 + (slot)] = wall_clock64(); } while (0)

// flat parameter / gradient order: W_cls | W_inter | W_intra[0..R) | W_clf | b_clf
__host__ __device__ inline int64_t off_cls(int F, int E, int R) { return 0; }
__host__ __device__ inline int64_t off_inter(int F, int E, int R) { return 2 * (int64_t)E; }
__host__ __device__ inline int64_t off_intra(int F, int E, int R, int r) {
    return off_inter(F, E, R) + (int64_t)(F + R * E) * E + (int64_t)r * 2 * F * E;
}
__host__ __device__ inline int64_t off_clf(int F, int E, int R) { return off_intra(F, E, R, R); }
__host__ __device__ inline int64_t off_bias(int F, int E, int R) { return off_clf(F, E, R) + 2 * (int64_t)F; }
__host__ __device__ inline int64_t n_params_of(int F, int E, int R) { return off_bias(F, E, R) + 2; }

// One accumulator chain of n_steps v_mfma_f32_16x16x4_f32 (n_steps a multiple of MU: every K dimension is padded with
// zeros to a multiple of 4 * MU), software-pipelined by hand: the operands of the next MU steps are requested before the
// MFMAs of the current MU steps issue (two register sets), so that a wave's LDS reads overlap its own matrix work.
// (hipcc does not unroll these chains by itself; one step at a time every MFMA waits for its own two operand reads.  The
// fetched values go into the MFMAs untouched - any arithmetic on them would be scheduled, with its wait, ahead of the
// MFMAs and undo the prefetch.)  fa(s) / fb(s): this lane's A / B operand of step s.
constexpr int MU = 4;
constexpr int KPAD = 4 * MU;
template <class FA, class FB>
__device__ __forceinline__ void mfma_fetch(float (&av)[MU], float (&bv)[MU], int s, FA &fa, FB &fb) {
#pragma unroll
    for (int u = 0; u < MU; ++u) {
        av[u] = fa(s + u);
        bv[u] = fb(s + u);
    }
}
template <class FA, class FB>
__device__ __forceinline__ f32x4 mfma_chain(int n_steps, FA fa, FB fb) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float a0[MU], b0[MU], a1[MU], b1[MU];
    if (n_steps <= 0) return acc;
    mfma_fetch(a0, b0, 0, fa, fb);
    for (int s = 0; s < n_steps; s += 2 * MU) {
        if (s + MU < n_steps) mfma_fetch(a1, b1, s + MU, fa, fb);          // (wave-uniform)
#pragma unroll
        for (int u = 0; u < MU; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[u], b0[u], acc, 0, 0, 0);
        if (s + MU >= n_steps) break;
        if (s + 2 * MU < n_steps) mfma_fetch(a0, b0, s + 2 * MU, fa, fb);
#pragma unroll
        for (int u = 0; u < MU; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[u], b1[u], acc, 0, 0, 0);
    }
    return acc;
}

// C[16x16] = A * Bt^T with Bt in GLOBAL memory, row-major [n][k] (a weight matrix used transposed): lane (n = r, kq) would read
// Bt[n][4s + kq] for step s - 4 bytes from each of 16 rows per load instruction.  Instead a lane reads the float4
// Bt[n][16u + 4kq .. + 3] (16 rows x 64 contiguous bytes per instruction, a quarter of the instructions) and the four MFMA
// steps of block u take k = 16u + 4kq + i, i = 0..3: a permutation of the k order that the A operand (LDS, any pattern is
// cheap there) follows.  All loads of eight blocks are in flight before the first MFMA.
__device__ __forceinline__ f32x4 tile_lds_globT4(const float *ap /* A + r*lda + 4*kq */, const float *__restrict__ bp /* Bt + n*ldb + 4*kq */,
                                                 int n_blocks) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    constexpr int NB = 8;
    for (int u0 = 0; u0 < n_blocks; u0 += NB) {
        f4 b[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int u = u0 + j < n_blocks ? u0 + j : n_blocks - 1;          // (clamped: unconditional loads)
            b[j] = *reinterpret_cast<const f4 *>(bp + 16 * u);
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            if (u0 + j >= n_blocks) break;                                    // (wave-uniform)
            const float *aj = ap + 16 * (u0 + j);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aj[0], b[j].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aj[1], b[j].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aj[2], b[j].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aj[3], b[j].w, acc, 0, 0, 0);
        }
    }
    return acc;
}

// C[16x16] += A[16 x k-steps] (LDS, row-major, leading dim lda) * B (global, ld ldb, column n0..n0+15), k in [k_lo, k_hi)
__device__ __forceinline__ f32x4 tile_lds_glob(const float *A, int lda, const float *__restrict__ Bg, int ldb, int n0,
                                               int K, int k_lo, int k_hi, int lane) {
    const int r = lane & 15, kq = lane >> 4;
    const float *ap = A + r * lda + k_lo + kq;
    // rows k >= K of B do not exist: A's pad columns are zero, so any finite value will do there - the last row's
    return mfma_chain((k_hi - k_lo) >> 2, [&](int s) { return ap[4 * s]; },
                      [&](int s) {
                          const int k = k_lo + 4 * s + kq;
                          return Bg[(size_t)(k < K ? k : K - 1) * ldb + n0 + r];
                      });
}

// the same with B an LDS copy of the weight matrix (leading dim ldb; rows beyond K are zero)
__device__ __forceinline__ f32x4 tile_lds_lds(const float *A, int lda, const float *Bl, int ldb, int n0, int k_lo, int k_hi,
                                              int lane) {
    const int r = lane & 15, kq = lane >> 4;
    const float *ap = A + r * lda + k_lo + kq;
    const float *bp = Bl + (k_lo + kq) * ldb + n0 + r;
    return mfma_chain((k_hi - k_lo) >> 2, [&](int s) { return ap[4 * s]; }, [&](int s) { return bp[4 * s * ldb]; });
}

// C[16x16] = At^T * Bt with both operands row tiles in LDS: C[m][n] = sum_t At[t][m0+m] * Bt[t][n0+n], t < 16
__device__ __forceinline__ f32x4 tile_ldsT_lds(const float *At, int lda, int m0, int M, const float *Bt, int ldb, int n0,
                                               int lane) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int r = lane & 15, kq = lane >> 4;
    const bool mok = m0 + r < M;
    const int mr = mok ? m0 + r : M - 1;
    float av[TB / 4], bv[TB / 4];
#pragma unroll
    for (int j = 0; j < TB / 4; ++j) {
        const int t = 4 * j + kq;
        const float x = At[t * lda + mr];
        av[j] = mok ? x : 0.f;
        bv[j] = Bt[t * ldb + n0 + r];
    }
#pragma unroll
    for (int j = 0; j < TB / 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[j], acc, 0, 0, 0);
    return acc;
}

// sum over the 16 lanes of a DPP row (every lane gets it): quad permutes, then the half-row / row mirrors
__device__ __forceinline__ float row16_sum(float p) {
    p = dpp_add<0xB1>(p);
    p = dpp_add<0x4E>(p);
    p = dpp_add<0x141>(p);
    p = dpp_add<0x140>(p);
    return p;
}

// WLDS: the weight matrices are staged in LDS once per workgroup (when they fit), so every MFMA operand
// is an LDS read; otherwise the B operands stream from global memory / L2.
// Phases (one barrier between them): stage -> h_r for all relations -> combined (K split over the waves) -> logits + loss
// grads -> dcomb + small dW -> {dh_r for all r, dW_inter} -> dW_r for all r.
// F_, E_, R_ > 0: the shape is a compile-time constant (the datasets' shapes are instantiated below): every LDS offset is
// then an immediate and the index arithmetic folds away - with run-time shapes the kernel issues ~1400 vector and ~750
// scalar instructions per wave, most of them address arithmetic, and that issue time (not the matrix cores, 14 % busy,
// nor the LDS, 20 % busy) is what it is bound by.  0: run-time shape (any F, E % 16 == 0, R <= 8).
// INFER: the forward phases only, for a workgroup that may run tile after tile (infer_dense_kernel, infer.hip): the K-split
// partial tiles of `combined` go where the backward's dcomb / dh_r arrays are (the W_intra copy stays live for the next tile),
// and STAGE_W = false skips the weights' LDS copy (the workgroup's first tile made it).  The training launches set neither:
// their code is what it was before these flags existed.
// EXT: the backward starts from the CALLER's loss gradients instead of the built-in loss's (dense_vjp_kernel, vjp.hip; acts mode
// only): row b's seeds are d_logits[2b], d_logits[2b + 1] (d loss / d gnn logits) and d_center[2b], d_center[2b + 1] (d loss / d
// label-aware logits), used as given - no 1 / count, no lambda_1, no label read, no row loss; rows beyond the batch get zeros.
// Everything behind the loss phase reads only s_dlog / s_dcl and the forward's LDS state, so nothing else differs.
// h_out (INFER only, else not looked at; pcg_embed_set / pcg_embed_new): row b's relation embeddings h_1 | .. | h_R -> h_out[b][R * E],
// copied out of s_cat behind the h_r phase's barrier.  The other launches leave it at its default and the copy folds away.
template <bool WLDS, int F_, int E_, int R_, bool INFER = false, bool STAGE_W = true, bool EXT = false>
__device__ __forceinline__ void dense_tile_body(const DenseArgs &a, int bid, float *sm, const float *__restrict__ d_logits = nullptr,
                                                const float *__restrict__ d_center = nullptr, float *__restrict__ h_out = nullptr) {
    // bid: this workgroup's index among the tiles' workgroups (a.n_tile_blocks of them); sm: the launch's dynamic LDS
    const int F = F_ > 0 ? F_ : a.feat_dim, E = E_ > 0 ? E_ : a.emb, R = R_ > 0 ? R_ : a.n_rel;
    const int K1 = 2 * F, K1p = (K1 + KPAD - 1) / KPAD * KPAD, K2 = F + R * E, K2p = (K2 + KPAD - 1) / KPAD * KPAD;
    const int ld1 = K1p + 1, ld2 = K2p + 1, ldE = E + 1, ldW = E + 4;   // ldW: rows stay 16-B aligned (ds_write_b128)
    const int ntile_e = E / 16;
    const int kparts = ntile_e <= DENSE_WAVES ? DENSE_WAVES / ntile_e : 1;      // waves sharing one output tile of `combined`
    float *s_wi = sm;                               // WLDS: [K2p][ldW] copy of W_inter   (first: 16-B aligned)
    float *s_wr = s_wi + (WLDS ? K2p * ldW : 0);    // WLDS: [R][K1p][ldW] copies of W_intra; later the K-split partial tiles
    float *s_part = WLDS ? s_wr : s_wr;             // [kparts][TB][E] partial sums of `combined` (W_intra is dead by then)
    float *s_catr = s_wr + (WLDS ? R * K1p * ldW : kparts * TB * E);   // [R][TB][ld1]  [self | agg_r]
    float *s_cat = s_catr + R * TB * ld1;           // [TB][ld2]  [self | h_1 .. h_R]
    float *s_comb = s_cat + TB * ld2;               // [TB][ldE]
    float *s_dcomb = s_comb + TB * ldE;             // [TB][ldE]
    float *s_dh = s_dcomb + TB * ldE;               // [R][TB][ldE]
    float *s_dlog = s_dh + R * TB * ldE;            // [TB][2] d loss / d gnn logits
    float *s_dcl = s_dlog + TB * 2;                 // [TB][2] d loss / d centre scores (already times lambda_1)
    float *s_wc = s_dcl + TB * 2;                   // [2][E] W_cls, [2][F] W_clf, [2] b_clf
    int *s_flag = reinterpret_cast<int *>(s_wc + 2 * E + 2 * F + 4);   // [4] "this workgroup's classifier gradient arrived last"
    if constexpr (WLDS && INFER) s_part = s_dcomb;  // (host-checked: kparts * TB * E <= (1 + R) * TB * ldE)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.n_split, tile_id = bid / S, sp = bid % S;
    const int row0 = tile_id * TB;
    const bool acts_mode = a.acts != nullptr;
    const bool train = a.slabs != nullptr || acts_mode;
    if (train && bid == 0 && tid == 0) {
        // (an agent-scope atomic: the workgroup that applies the classifier's Adam reads the new count from another XCD)
        if (a.step_counter) __hip_atomic_fetch_add(a.step_counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (a.pending) {
            a.pending[0] = acts_mode ? 2u : 1u;                 // the slabs (1) / acts (2) hold a gradient the other parameters still need
            a.pending[1] = (unsigned)(a.n_tile_blocks / S);           // ... in this many slabs / blocks of 16 batch rows
        }
    }
    // wave t's row of the loss phase: its label is requested now, not when the logits are ready
    const int my_b = row0 + wave;
    const int my_label = (!EXT && a.labels && my_b < a.B) ? a.labels[my_b] : 0;
    // (EXT: its four seeds instead - unconditional loads at a clamped row, the values of rows beyond the batch discarded)
    float seed_g0 = 0.f, seed_g1 = 0.f, seed_c0 = 0.f, seed_c1 = 0.f;
    if constexpr (EXT) {
        const int sb = my_b < a.B ? my_b : a.B - 1;
        seed_g0 = d_logits[2 * sb];
        seed_g1 = d_logits[2 * sb + 1];
        seed_c0 = d_center[2 * sb];
        seed_c1 = d_center[2 * sb + 1];
        if (my_b >= a.B) seed_g0 = seed_g1 = seed_c0 = seed_c1 = 0.f;
    }
    DENSE_STAMP(0);
    if (a.stamps && threadIdx.x == 0 && sp == 0) a.stamps[(size_t)tile_id * 16 + 12] = clock64();     // shader cycles (diagnostic)

    // ---- stage ----------------------------------------------------------------------------------------------------
    // every global load of the prologue is requested before the first LDS store: weights (<= WSTAGE float4 per thread in
    // flight), the tile's self rows (ids -> rows), its aggregated rows (or their partial sums)
    {
        // self rows and aggregates: element e of [TB][F] (self) and [R][TB][F] (agg), one or two per thread.  Every load is
        // unconditional (indices clamped, the value discarded afterwards): a load inside a branch makes the compiler wait
        // for it at the branch's end, which turns the prologue into a chain of L2 round trips
        const int n_self = TB * F, n_agg = R * TB * F;
        const bool do_self = tid < n_self;                                 // (TB * F <= 1024 for F <= 64; a loop covers the rest)
        const int self_i = do_self ? tid : n_self - 1;
        const int self_t = self_i / F, self_f = self_i - self_t * F;
        const int self_b = row0 + self_t;
        const int self_id = a.ids[self_b < a.B ? self_b : a.B - 1];
        constexpr int NAGG = 2;
        float v_agg[NAGG];
        int agg_at[NAGG], agg_nch[NAGG], agg_cb[NAGG];
        size_t agg_row[NAGG];
        int agg_f[NAGG];
        bool agg_ok[NAGG];
#pragma unroll
        for (int u = 0; u < NAGG; ++u) {
            const int i0 = tid + u * DENSE_THREADS;
            const int i = i0 < n_agg ? i0 : n_agg - 1;
            const int r = i / (TB * F), j = i - r * TB * F, t = j / F, f = j - t * F;
            const int b = row0 + t;
            agg_at[u] = i0 < n_agg ? (r * TB + t) * ld1 + F + f : -1;
            agg_ok[u] = i0 < n_agg && b < a.B;
            agg_row[u] = (size_t)r * a.B + (b < a.B ? b : a.B - 1);
            agg_f[u] = f;
            agg_cb[u] = 0;
            agg_nch[u] = 1;
            if (a.chunk_begin) {                                           // (uniform: a kernel argument)
                agg_cb[u] = a.chunk_begin[agg_row[u]];
                agg_nch[u] = a.chunk_begin[agg_row[u] + 1] - agg_cb[u];
            }
            v_agg[u] = a.agg[agg_row[u] * a.agg_stride + f];
        }
        float v_self = a.X[(size_t)self_id * a.feat_stride + self_f];
        if (!do_self || self_b >= a.B) v_self = 0.f;
#pragma unroll
        for (int u = 0; u < NAGG; ++u) {
            if (!agg_ok[u]) v_agg[u] = 0.f;
            else if (agg_nch[u] == 0) v_agg[u] = 0.f / 0.f;       // empty set: 0 / 0 like the reference's mask.div (layers.py:612-614)
            else if (agg_nch[u] > 1) {                             // sum of the gather's partial sums, in chunk order, / |set|  (== combine_rows)
                float acc = 0.f;
                const float *pp = a.partial + (size_t)agg_cb[u] * a.partial_stride + agg_f[u];
                const int nch = agg_nch[u];
                // (eight loads in flight - clamped index, the extra values not added -, the adds in chunk order: a hub row has
                //  dozens of chunks, and this loop sits in front of everything else the workgroup stages)
                for (int jx = 0; jx < nch; jx += 8) {
                    float pv[8];
#pragma unroll
                    for (int x = 0; x < 8; ++x) pv[x] = pp[(size_t)(jx + x < nch ? jx + x : nch - 1) * a.partial_stride];
#pragma unroll
                    for (int x = 0; x < 8; ++x) acc = jx + x < nch ? acc + pv[x] : acc;
                }
                v_agg[u] = acc / (float)a.cnt[agg_row[u]];
            }
        }
        if constexpr (WLDS && STAGE_W) {
            // the weight matrices as one list of rows [W_inter | W_intra[0] | ...] (contiguous in theta); thread -> (row, 16-B column chunk)
            const int c4 = E >> 2;
            const int cc = (tid % c4) * 4, r0 = tid / c4, rstep = DENSE_THREADS / c4;   // DENSE_THREADS % c4 == 0 (host-checked)
            const int n_rows = K2 + R * K1;
            // every workgroup streams the same 100+ KB out of L2 at the same moment: each starts at another row, so that they
            // do not all queue on the same L2 channels in the same order
            const int rot = (int)(((unsigned)bid * 29u) % (unsigned)n_rows);
            for (int base = r0; base < n_rows; base += WSTAGE * rstep) {
                float4 wv[WSTAGE];
                int rows_[WSTAGE];
#pragma unroll
                for (int u = 0; u < WSTAGE; ++u) {
                    const int rl = base + u * rstep;
                    int rr = (rl < n_rows ? rl : n_rows - 1) + rot;
                    rr = rr >= n_rows ? rr - n_rows : rr;
                    rows_[u] = rl < n_rows ? rr : -1;
                    wv[u] = *reinterpret_cast<const float4 *>(a.W_inter + (size_t)rr * E + cc);
                }
#pragma unroll
                for (int u = 0; u < WSTAGE; ++u) {
                    const int rr = rows_[u];
                    if (rr >= 0) {
                        float *dst = rr < K2 ? s_wi + rr * ldW
                                             : s_wr + ((rr - K2) / K1) * K1p * ldW + ((rr - K2) % K1) * ldW;
                        *reinterpret_cast<float4 *>(dst + cc) = wv[u];
                    }
                }
            }
            for (int i = tid; i < (K2p - K2) * E; i += DENSE_THREADS) s_wi[(K2 + i / E) * ldW + i % E] = 0.f;
            const int pad1 = (K1p - K1) * E, pad1_div = pad1 > 0 ? pad1 : 1;   // (no pad rows when 2F is a multiple of KPAD)
            for (int i = tid; i < R * pad1; i += DENSE_THREADS) {
                const int r = i / pad1_div, j = i - r * pad1;
                s_wr[r * K1p * ldW + (K1 + j / E) * ldW + j % E] = 0.f;
            }
        }
        for (int i = tid; i < 2 * E; i += DENSE_THREADS) s_wc[i] = a.W_cls[i];
        for (int i = tid; i < 2 * F; i += DENSE_THREADS) s_wc[2 * E + i] = a.W_clf[i];
        if (tid < 2) s_wc[2 * E + 2 * F + tid] = a.b_clf[tid];
        if (tid == 0) s_flag[0] = 0;
        // activations: self into [self | .] of every concatenation, aggregates, zero pad columns
        if (do_self) {
            s_cat[self_t * ld2 + self_f] = v_self;
            for (int r = 0; r < R; ++r) s_catr[(r * TB + self_t) * ld1 + self_f] = v_self;
        }
        for (int i = tid + DENSE_THREADS; i < n_self; i += DENSE_THREADS) {           // F > 64
            const int t = i / F, f = i - t * F, b = row0 + t;
            const float v = b < a.B ? a.X[(size_t)a.ids[b] * a.feat_stride + f] : 0.f;
            s_cat[t * ld2 + f] = v;
            for (int r = 0; r < R; ++r) s_catr[(r * TB + t) * ld1 + f] = v;
        }
#pragma unroll
        for (int u = 0; u < NAGG; ++u)
            if (agg_at[u] >= 0) s_catr[agg_at[u]] = v_agg[u];
        for (int i = tid + NAGG * DENSE_THREADS; i < n_agg; i += DENSE_THREADS) {     // R * F > 128
            const int r = i / (TB * F), j = i - r * TB * F, t = j / F, f = j - t * F, b = row0 + t;
            float v = 0.f;
            if (b < a.B) {
                const size_t row = (size_t)r * a.B + b;
                int cb = 0, nch = 1;
                if (a.chunk_begin) {
                    cb = a.chunk_begin[row];
                    nch = a.chunk_begin[row + 1] - cb;
                }
                if (nch == 0) v = 0.f / 0.f;
                else if (nch > 1) {
                    float acc = 0.f;
                    for (int jx = 0; jx < nch; ++jx) acc += a.partial[(size_t)(cb + jx) * a.partial_stride + f];
                    v = acc / (float)a.cnt[row];
                } else {
                    v = a.agg[row * a.agg_stride + f];
                }
            }
            s_catr[(r * TB + t) * ld1 + F + f] = v;
        }
        for (int i = tid; i < R * TB * (ld1 - K1); i += DENSE_THREADS) {              // pad columns K1 .. ld1
            const int rt = i / (ld1 - K1), c = K1 + i % (ld1 - K1);
            s_catr[rt * ld1 + c] = 0.f;
        }
        for (int i = tid; i < TB * (ld2 - K2); i += DENSE_THREADS) s_cat[(i / (ld2 - K2)) * ld2 + K2 + i % (ld2 - K2)] = 0.f;
    }
    __syncthreads();
    DENSE_STAMP(1);
    // (a workgroup that takes no ticket says here that it has read the classifier's weights - the last ticket holder overwrites
    //  them.  These arrivals are ~10 us ahead of their only reader: their serialisation on the counter costs nobody anything)
    if (a.theta && sp != 0 && tid == 0) __hip_atomic_fetch_add(a.staged, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

    // ---- forward: h_r = relu([self | agg_r] W_r) for every relation   (layers.py:625-629) ---------
    for (int tile = wave; tile < R * ntile_e; tile += DENSE_WAVES) {
        const int r = tile / ntile_e, ct = tile - r * ntile_e;
        const float *A = s_catr + r * TB * ld1;
        const f32x4 c = WLDS ? tile_lds_lds(A, ld1, s_wr + r * K1p * ldW, ldW, ct * 16, 0, K1p, lane)
                             : tile_lds_glob(A, ld1, a.W_intra[r], E, ct * 16, K1, 0, K1p, lane);
        const int col = ct * 16 + (lane & 15), rq = (lane >> 4) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) s_cat[(rq + i) * ld2 + F + r * E + col] = fmaxf(c[i], 0.f);
    }
    __syncthreads();
    DENSE_STAMP(2);
    if constexpr (INFER) {
        if (h_out) {                                                       // (uniform: a kernel argument)
            // consecutive threads store consecutive floats of a row's R * E (s_cat's columns behind the self columns)
            const int RE = R * E;
            for (int i = tid; i < TB * RE; i += DENSE_THREADS) {
                const int t = i / RE, c = i - t * RE, b = row0 + t;
                if (b < a.B) h_out[(size_t)b * RE + c] = s_cat[t * ld2 + F + c];
            }
        }
    }
    // ---- combined = relu(cat W)   (layers.py:284-289): the K dimension of every output tile split over `kparts` waves,
    //      their partial tiles added in a fixed order ----------------------------------------------------------------
    {
        const int ksteps = K2p / 4;
        const int per = ((ksteps + kparts - 1) / kparts + MU - 1) / MU * MU;      // steps per part: a multiple of MU
        for (int item = wave; item < ntile_e * kparts; item += DENSE_WAVES) {
            const int ct = item % ntile_e, kp = item / ntile_e;
            const int k_lo = kp * per * 4, k_hi = (kp + 1) * per * 4 < K2p ? (kp + 1) * per * 4 : K2p;
            const f32x4 c = WLDS ? tile_lds_lds(s_cat, ld2, s_wi, ldW, ct * 16, k_lo, k_hi, lane)
                                 : tile_lds_glob(s_cat, ld2, a.W_inter, E, ct * 16, K2, k_lo, k_hi, lane);
            const int col = ct * 16 + (lane & 15), rq = (lane >> 4) * 4;
#pragma unroll
            for (int i = 0; i < 4; ++i) s_part[(kp * TB + rq + i) * E + col] = c[i];
        }
        __syncthreads();
        DENSE_STAMP(11);
        for (int i = tid; i < TB * E; i += DENSE_THREADS) {
            const int t = i / E, e = i - t * E;
            float acc = s_part[t * E + e];
            for (int kp = 1; kp < kparts; ++kp) acc += s_part[(kp * TB + t) * E + e];
            const float v = fmaxf(acc, 0.f);
            s_comb[t * ldE + e] = v;
            const int b = row0 + t;
            if (a.combined && b < a.B && sp == 0) a.combined[(size_t)b * E + e] = v;
        }
    }
    __syncthreads();
    DENSE_STAMP(3);
    // ---- logits, centre scores, loss gradients (model.py:38, layers.py:243, model.py:54-61): wave t has row t; its four
    //      dot products run on 16 lanes each and are added with DPP row operations; no LDS, no barrier in between ----
    {
        const int t = wave, which = lane >> 4, part = lane & 15, b = row0 + t;
        float acc = 0.f;
        if (which < 2) {
            const float *wv = s_wc + which * E;
            for (int e = part; e < E; e += 16) acc = fmaf(s_comb[t * ldE + e], wv[e], acc);
        } else {
            const float *wv = s_wc + 2 * E + (which - 2) * F;
            for (int f = part; f < F; f += 16) acc = fmaf(s_cat[t * ld2 + f], wv[f], acc);
        }
        acc = row16_sum(acc);
        const float g0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 0));
        const float g1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 16));
        const float c0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 32)) + s_wc[2 * E + 2 * F];
        const float c1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 48)) + s_wc[2 * E + 2 * F + 1];
        if (lane == 0) {
            float dg0 = 0.f, dg1 = 0.f, dc0 = 0.f, dc1 = 0.f;
            if (b < a.B) {
                if constexpr (EXT) {
                    if (a.logits) {
                        a.logits[2 * b] = g0;
                        a.logits[2 * b + 1] = g1;
                    }
                    if (a.center) {
                        a.center[2 * b] = c0;
                        a.center[2 * b + 1] = c1;
                    }
                } else if (sp == 0) {
                    a.logits[2 * b] = g0;
                    a.logits[2 * b + 1] = g1;
                    a.center[2 * b] = c0;
                    a.center[2 * b + 1] = c1;
                }
                if constexpr (EXT) {
                    dg0 = seed_g0; dg1 = seed_g1;
                    dc0 = seed_c0; dc1 = seed_c1;
                } else if (a.labels) {
                    const int y = my_label;
                    float lg, lc;
                    xent2(g0, g1, y, lg, dg0, dg1);
                    xent2(c0, c1, y, lc, dc0, dc1);
                    if (a.row_loss && sp == 0) a.row_loss[b] = lg + a.lambda_1 * lc;
                    dg0 *= a.inv_count; dg1 *= a.inv_count;
                    dc0 *= a.inv_count * a.lambda_1; dc1 *= a.inv_count * a.lambda_1;
                }
            }
            s_dlog[2 * t] = dg0; s_dlog[2 * t + 1] = dg1;
            s_dcl[2 * t] = dc0; s_dcl[2 * t + 1] = dc1;
        }
    }
    __syncthreads();
    DENSE_STAMP(4);
    if constexpr (INFER) return;
    if (!train) return;

    float *slab = acts_mode ? nullptr : a.slabs + (size_t)tile_id * a.n_params;
    const bool adam_clf = a.theta != nullptr;
    // ---- backward ----------------------------------------------------------------------------------------------------
    // dcomb = (dlogits W_cls) * relu'(combined);  dW_cls, dW_clf, db_clf
    for (int i = tid; i < TB * E; i += DENSE_THREADS) {
        const int t = i / E, e = i - t * E;
        const float g = s_dlog[2 * t] * s_wc[e] + s_dlog[2 * t + 1] * s_wc[E + e];
        s_dcomb[t * ldE + e] = s_comb[t * ldE + e] > 0.f ? g : 0.f;
    }
    DENSE_STAMP(8);
    for (int i = tid; i < ((sp == 0 && !acts_mode) ? 2 * E : 0); i += DENSE_THREADS) {
        const int cidx = i / E, e = i - cidx * E;
        float sacc = 0.f;
        for (int t = 0; t < TB; ++t) sacc = fmaf(s_dlog[2 * t + cidx], s_comb[t * ldE + e], sacc);
        slab[off_cls(F, E, R) + i] = sacc;
    }
    DENSE_STAMP(9);
    // the label classifier's partial gradient, by ONE wave: write-through (sc1) stores when another workgroup of this launch
    // will read it - that wave's own vmcnt wait, a phase later, then covers every one of them.  The wave chosen has no other
    // global store in between (the last of the waves that only compute a dh_r tile in the next phase), so that wait is free.
    const int clf_wave = (R * ntile_e - 1) & (DENSE_WAVES - 1);
    if (wave == clf_wave && sp == 0 && !acts_mode) {
        for (int i = lane; i < 2 * F + 2; i += PCG_WAVE) {
            float sacc = 0.f;
            if (i < 2 * F) {
                const int cidx = i / F, f = i - cidx * F;
                for (int t = 0; t < TB; ++t) sacc = fmaf(s_dcl[2 * t + cidx], s_cat[t * ld2 + f], sacc);
            } else {
                for (int t = 0; t < TB; ++t) sacc += s_dcl[2 * t + (i - 2 * F)];
            }
            float *dst = slab + off_clf(F, E, R) + i;
            if (adam_clf) __hip_atomic_store(dst, sacc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else *dst = sacc;
        }
    }
    DENSE_STAMP(10);
    __syncthreads();
    DENSE_STAMP(5);
    // one phase: dh_r = (dcomb W[F+rE.., :]^T) * relu'(h_r) for every r   and   dW_inter = cat^T dcomb
    {
        const int mt2 = (K2 + 15) / 16;
        const int n_dh = R * ntile_e, n_all = n_dh + mt2 * ntile_e;
        float *dst = slab ? slab + off_inter(F, E, R) : nullptr;
        // every workgroup of the tile needs all of dh_r; the dW_inter tiles are dealt out over the tile's S workgroups
        // (acts_mode: dh_r only - the weight gradients are a later launch's)
        for (int t0 = wave; t0 < (acts_mode ? n_dh : n_dh + (n_all - n_dh + S - 1) / S); t0 += DENSE_WAVES) {
            const int tile = t0 < n_dh ? t0 : n_dh + (t0 - n_dh) * S + sp;
            if (tile >= n_all) continue;
            if (tile < n_dh) {
                const int r = tile / ntile_e, ct = tile - r * ntile_e;
                const float *Wr = a.W_inter + (size_t)(F + r * E) * E;   // rows of W_inter that multiply h_r
                const int rr = lane & 15, kq = lane >> 4;
                const float *ap = s_dcomb + rr * ldE + kq;                 // out[t][j] = sum_e dcomb[t][e] * Wr[j][e]
                const float *bl = s_wi + (F + r * E + ct * 16 + rr) * ldW + kq;
                const float *bg = Wr + (size_t)(ct * 16 + rr) * E + kq;
                // (E is a multiple of 16.  Without the LDS copy the transposed weight rows come from L2 as float4 per lane)
                const f32x4 acc = WLDS ? mfma_chain(E >> 2, [&](int s) { return ap[4 * s]; }, [&](int s) { return bl[4 * s]; })
                                       : tile_lds_globT4(s_dcomb + rr * ldE + 4 * kq, bg + 3 * kq, E >> 4);
                const int col = ct * 16 + rr, rq = kq * 4;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    s_dh[(r * TB + rq + i) * ldE + col] = s_cat[(rq + i) * ld2 + F + r * E + col] > 0.f ? acc[i] : 0.f;
            } else {
                const int tl = tile - n_dh;
                const int m0 = (tl / ntile_e) * 16, n0 = (tl % ntile_e) * 16;
                const f32x4 c = tile_ldsT_lds(s_cat, ld2, m0, K2, s_dcomb, ldE, n0, lane);
                const int col = n0 + (lane & 15), rq = (lane >> 4) * 4;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (m0 + rq + i < K2) dst[(size_t)(m0 + rq + i) * E + col] = c[i];
            }
        }
    }
    __syncthreads();
    DENSE_STAMP(6);
    if (acts_mode) {
        // everything the weight gradients are made of, transposed (a batch row per column: the GEMMs over the batch then read
        // both operands contiguously - wgrad.h); rows beyond the batch in this tile are zero in every array (staged as zeros,
        // no loss gradient).  A thread stores 16-float runs (one act row of this tile: 64 bytes); nothing reads them in this launch.
        const int n_act = K2 + R * F + E + R * E + E + 4;
        float *__restrict__ out = a.acts + row0;
        for (int i = tid; i < n_act * TB; i += DENSE_THREADS) {
            const int rho = i >> 4, t = i & 15;
            int q = rho;
            float v;
            if (q < K2) v = s_cat[t * ld2 + q];
            else if ((q -= K2) < R * F) {
                const int r = q / F, f = q - r * F;
                v = s_catr[(r * TB + t) * ld1 + F + f];
            } else if ((q -= R * F) < E) v = s_dcomb[t * ldE + q];
            else if ((q -= E) < R * E) {
                const int r = q / E, e = q - r * E;
                v = s_dh[(r * TB + t) * ldE + e];
            } else if ((q -= R * E) < E) v = s_comb[t * ldE + q];
            else if ((q -= E) < 2) v = s_dlog[2 * t + q];
            else v = s_dcl[2 * t + (q - 2)];
            out[(size_t)rho * a.act_ld + t] = v;
        }
        DENSE_STAMP(7);
        return;
    }
    // arrival ticket (the workgroup's classifier gradient - its clf wave's stores, issued a phase ago - is write-through and
    // drained; and a workgroup that has arrived has long read the classifier's weights).  The answer is not needed before the
    // end of the kernel, so nobody waits for it here.
    // Only the workgroups that stored a share of the classifier's gradient (sp == 0: one per tile) arrive: the other slab
    // entries are read by the NEXT launch.  (Every workgroup arriving was 256 same-address atomics at B = 1024 - a counter
    // takes ~88 per microsecond, so the last arriver learned that it was the last ~3 us after the first one asked.)
    unsigned ticket_old = 0u;
    if (adam_clf && wave == clf_wave && sp == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) ticket_old = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // dW_r = [self|agg_r]^T dh_r for every r
    {
        const int mt1 = (K1 + 15) / 16, per_r = mt1 * ntile_e;
        for (int tile = sp + S * wave; tile < R * per_r; tile += S * DENSE_WAVES) {
            const int r = tile / per_r, tl = tile - r * per_r;
            const int m0 = (tl / ntile_e) * 16, n0 = (tl % ntile_e) * 16;
            const f32x4 c = tile_ldsT_lds(s_catr + r * TB * ld1, ld1, m0, K1, s_dh + r * TB * ldE, ldE, n0, lane);
            float *dst = slab + off_intra(F, E, R, r);
            const int col = n0 + (lane & 15), rq = (lane >> 4) * 4;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (m0 + rq + i < K1) dst[(size_t)(m0 + rq + i) * E + col] = c[i];
        }
    }
    DENSE_STAMP(7);
    if (a.stamps && threadIdx.x == 0 && sp == 0) a.stamps[(size_t)tile_id * 16 + 13] = clock64();
    // ---- the workgroup whose ticket was the last: sum of every tile's share of the classifier gradient (tile order), Adam
    //      for those 2F + 2 parameters (model_handler.py:153) - the only ones the next step's score pass reads ----------
    if (!adam_clf) return;
    if (wave == clf_wave && lane == 0) s_flag[0] = sp == 0 && ticket_old == (unsigned)a.n_tile_blocks / (unsigned)S - 1u;
    __syncthreads();
    if (s_flag[0]) {
        if (tid == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        DENSE_STAMP(14);
        const int n_tiles = a.n_tile_blocks / S;
        unsigned staged_seen = (tid == 0 && S > 1) ? __hip_atomic_load(a.staged, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        const int64_t oc = off_clf(F, E, R);
        const int NC = 2 * F + 2;
        // G threads per parameter: thread (g, i) adds up the tiles s = g, g + G, ... of parameter i in that order (the loads of
        // a batch of eight are all in flight: one memory round trip per batch instead of one per tile), the G partial sums
        // are added in group order - a fixed order for a given batch size, like everything else here.  s_dh is free by now.
        int G = NC <= DENSE_THREADS ? (DENSE_THREADS / NC < 16 ? DENSE_THREADS / NC : 16) : 1;
        const int room = (R * TB * ldE) / NC;                  // what s_dh can hold
        G = G < room ? G : room;
        G = G < 1 ? 1 : G;
        float *s_red = s_dh;                                   // [G][NC] (only when G > 1)
        for (int i0 = 0; i0 < NC; i0 += DENSE_THREADS) {       // (one pass unless there are more parameters than threads)
            const int g = G > 1 ? tid / NC : 0, i = i0 + (G > 1 ? tid - g * NC : tid);
            float acc = 0.f;
            if (g < G && i < NC) {
                const float *src = a.slabs + oc + i;
                // (every batch of eight loads is issued whole - indices clamped, the surplus not added: at 64 tiles and fifteen
                //  threads per parameter a thread has five tiles, and a loop of single agent-scope loads waited for each of them in
                //  turn: five memory round trips on the step's critical path instead of one)
                for (int s2 = g; s2 < n_tiles; s2 += 8 * G) {
                    float x[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int t2 = s2 + u * G;
                        x[u] = __hip_atomic_load(src + (size_t)(t2 < n_tiles ? t2 : n_tiles - 1) * a.n_params, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) acc = (s2 + u * G < n_tiles) ? acc + x[u] : acc;
                }
            }
            if (G > 1) {
                if (g < G && i < NC) s_red[g * NC + i] = acc;
                __syncthreads();
                if (tid < NC) {
                    acc = s_red[tid];
                    for (int gg = 1; gg < G; ++gg) acc += s_red[gg * NC + tid];
                }
            }
            const int ip = G > 1 ? tid : i;
            if (i0 == 0 && S > 1) {
                // every workgroup without a ticket has long staged the old classifier (it said so ~10 us ago); the count was
                // requested before the gradient's loads, so the check costs nothing in all but pathological schedules; bounded
                if (tid == 0)
                    for (int spins = 0; staged_seen < (unsigned)a.n_tile_blocks - (unsigned)n_tiles && spins < (1 << 20); ++spins) {
                        __builtin_amdgcn_s_sleep(4);
                        staged_seen = __hip_atomic_load(a.staged, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                __syncthreads();
            }
            if (ip < NC) {
                // t: the step this launch counted (block 0 incremented the counter at its start; read it past the L1)
                const float t = (float)__hip_atomic_load(a.step_counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                adam_apply_one(a.theta, a.m, a.v, oc + ip, acc, t, a.h);
            }
        }
        if (tid == 0) {
            __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.staged, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        DENSE_STAMP(15);
    }
}

static inline size_t dense_smem_bytes(int F, int E, int R, bool wlds) {
    const int K1p = (2 * F + KPAD - 1) / KPAD * KPAD, K2p = (F + R * E + KPAD - 1) / KPAD * KPAD;
    const int ntile_e = E / 16, kparts = ntile_e <= DENSE_WAVES ? DENSE_WAVES / ntile_e : 1;
    size_t fl = (size_t)(R * TB * (K1p + 1) + TB * (K2p + 1) + (2 + R) * TB * (E + 1) + 4 * TB + 2 * E + 2 * F + 4 + 4);
    if (wlds) fl += (size_t)(K2p + R * K1p) * (E + 4);
    else fl += (size_t)kparts * TB * E;
    return sizeof(float) * fl;
}

static inline bool dense_wlds(int F, int E, int R) {
    const int K1p = (2 * F + KPAD - 1) / KPAD * KPAD;
    const int ntile_e = E / 16, kparts = ntile_e <= DENSE_WAVES ? DENSE_WAVES / ntile_e : 1;
    // the K-split partial tiles of `combined` live where the W_intra copies were
    return dense_smem_bytes(F, E, R, true) <= 160 * 1024 && DENSE_THREADS % (E / 4) == 0 && (size_t)kparts * TB * E <= (size_t)R * K1p * (E + 4);
}

// The instantiated shapes of dense_tile_body's kernels, listed HERE and nowhere else: YelpChi (F 32) and Amazon (F 25) at emb 64
// (weights in LDS) and emb 128 (weights streamed), three relations; anything else gets the run-time shape <wlds, 0, 0, 0>.
// wlds is the launcher's own rule (dense_wlds; infer_wlds for the forward-only launches); pick is a generic lambda that turns the
// shape's tag into the launcher's kernel pointer, with whatever further template arguments that kernel has.
template <bool WLDS, int F_, int E_, int R_>
struct DenseShape {
    static constexpr bool wlds = WLDS;
    static constexpr int F = F_, E = E_, R = R_;
};
template <class Pick>
static inline auto dense_dispatch(int F, int E, int R, bool wlds, Pick pick) -> decltype(pick(DenseShape<true, 0, 0, 0>())) {
    if (R == 3 && F == 32 && E == 64 && wlds) return pick(DenseShape<true, 32, 64, 3>());
    if (R == 3 && F == 25 && E == 64 && wlds) return pick(DenseShape<true, 25, 64, 3>());
    if (R == 3 && F == 32 && E == 128 && !wlds) return pick(DenseShape<false, 32, 128, 3>());
    if (R == 3 && F == 25 && E == 128 && !wlds) return pick(DenseShape<false, 25, 128, 3>());
    return wlds ? pick(DenseShape<true, 0, 0, 0>()) : pick(DenseShape<false, 0, 0, 0>());
}

struct DenseExtra {          // the optional parts of a launch
    const int32_t *chunk_begin = nullptr;
    const float *partial = nullptr;
    const int32_t *cnt = nullptr;
    int32_t partial_stride = 0;
    float *theta_rw = nullptr, *m = nullptr, *v = nullptr;
    uint32_t *ticket = nullptr, *pending = nullptr, *staged = nullptr;
    float *acts = nullptr;
    int32_t act_ld = 0;
    uint64_t *sort_keys = nullptr;          // the riding sort of the next step's train-pos keys (pcg_train_dense)
    AdamHyper h = {0.f, 0.f, 0.f, 0.f, 0.f};
};

// the argument block of a dense launch (launch_dense; the tiles of dense_select_kernel): n_sort_blocks = workgroups of the riding
// key sort behind the tiles' (x.sort_keys)
int dense_args(DenseArgs &a, int &n_sort_blocks, const pcg_graph_desc *g, const float *theta, int32_t emb, const int32_t *ids,
               const int32_t *labels, int32_t B, const float *agg, int32_t agg_stride, float lambda_1, float inv_count, float *logits,
               float *center, float *combined, float *row_loss, float *slabs, int32_t *step_counter, const DenseExtra &x);
extern unsigned long long *g_dense_stamps;

}  // namespace pcg
