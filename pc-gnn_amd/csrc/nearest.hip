// Nearest rows of a bank for every query row (pcg_topk_similar): exact-f32 similarity on the matrix cores plus a running top-k,
// without ever forming the [n][M] score matrix.
//
//   topk_norms_kernel : |row|^2 of every query and bank row into the workspace (cosine and l2 only; 16 lanes per row)
//   topk_scan_kernel  : a wave owns 16 query rows (its Q tile in LDS, the MFMA A operand) and one SLICE of the bank, which it
//                       walks in 16-candidate tiles: v_mfma_f32_16x16x4_f32 over E (tile_lds_globT4, dense.h: the bank rows come
//                       from global memory / L2 as float4 per lane), the metric applied to the 16x16 tile in registers, each
//                       score compared with its row's current k-th, and the few survivors inserted - one at a time, by the
//                       whole wave - into the row's sorted list in LDS.  The waves of a workgroup (4, or 2 where four Q tiles
//                       do not fit) own neighbouring query tiles and walk the same slice, so the bank tiles they ask for are
//                       in the CU's L1.  No workgroup barrier: a wave's LDS is its own.
//   topk_merge_kernel : only when the bank was sliced (few query tiles): a wave per query row, lane s at the head of slice s's
//                       list, k rounds of a wave-wide arg-best.
//
// Order: a list is sorted by (score descending, bank position ascending) and every insertion and merge compares that whole key,
// positions are unique, so the result is a function of the scores alone - not of the slice count, the grid, or the order in
// which survivors are taken.  A score is the row pair's own arithmetic (the MFMA chain over E in a fixed k order, then the
// metric), whatever tile or slice the pair is in.  No atomics anywhere.  Padding is (position -1, score -inf) and sorts last.
// A NaN score is taken as -inf.
#include "dense.h"

namespace pcg {

constexpr int TOPK_MAX_K = 64;
constexpr int TOPK_MAX_SLICES = 64;            // one lane of the merge wave per slice
constexpr int TOPK_PART_TILES = 2048;          // query tiles x slices the workspace's partial lists can hold
constexpr int TOPK_MIN_SLICE_TILES = 8;        // a slice is at least this many candidate tiles
constexpr int TOPK_SMEM_MAX = 160 * 1024;
static int g_topk_force_slices = 0;            // pcg_debug_set_topk_slices (tests): 0 = choose

__device__ __forceinline__ void wave_lds_sync() {
    // orders this wave's LDS stores before its later LDS loads of other lanes' words (no other wave touches them)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// key order of the lists: a before b
__device__ __forceinline__ bool topk_before(float sa, int pa, float sb, int pb) {
    if (pa < 0) return false;                  // padding is never before anything
    if (pb < 0) return true;
    return sa > sb || (sa == sb && pa < pb);
}

__global__ void __launch_bounds__(256) topk_norms_kernel(const float *__restrict__ Q, int64_t n, const float *__restrict__ bank,
                                                         int64_t M, int E, float *__restrict__ qn2, float *__restrict__ cn2) {
    const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int part = threadIdx.x & 15;
    const bool ok = row < n + M;
    const int64_t rc = ok ? row : n + M - 1;                               // (clamped: unconditional loads)
    const float *src = rc < n ? Q + rc * E : bank + (rc - n) * E;
    float acc = 0.f;
    for (int e = 4 * part; e < E; e += 64) {
        const float4 v = *reinterpret_cast<const float4 *>(src + e);
        acc = fmaf(v.x, v.x, acc);
        acc = fmaf(v.y, v.y, acc);
        acc = fmaf(v.z, v.z, acc);
        acc = fmaf(v.w, v.w, acc);
    }
    acc = row16_sum(acc);
    if (ok && part == 0) {
        if (row < n) qn2[row] = acc;
        else cn2[row - n] = acc;
    }
}

// out_*: [n_slices][row_stride][k]; slice s = candidate tiles [s * slice_tiles, + slice_tiles) of the bank's
__global__ void __launch_bounds__(256) topk_scan_kernel(const float *__restrict__ Q, int n, const float *__restrict__ bank, int M,
                                                        int E, int k, int metric, const int32_t *__restrict__ q_ids,
                                                        const int32_t *__restrict__ bank_ids, const float *__restrict__ qn2,
                                                        const float *__restrict__ cn2, int slice_tiles, int64_t row_stride,
                                                        int32_t *__restrict__ out_pos, float *__restrict__ out_score) {
    extern __shared__ __align__(16) float sm[];
    const int W = (int)blockDim.x >> 6, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ldq = E + 4;                                                 // rows stay 16-byte aligned
    float *s_q = sm + (size_t)wave * 16 * ldq;                             // [16][ldq] this wave's query rows
    float *s_sc = sm + (size_t)W * 16 * ldq + (size_t)wave * 16 * k;       // [16][k] scores, sorted
    int *s_ps = reinterpret_cast<int *>(sm + (size_t)W * 16 * ldq + (size_t)W * 16 * k) + (size_t)wave * 16 * k;   // [16][k] positions
    const int n_qt = (n + 15) >> 4;
    const int qt = (int)blockIdx.x * W + wave;
    if (qt >= n_qt) return;                                                // (wave-uniform; no workgroup barrier below)
    const int slice = (int)blockIdx.y;
    const int row0 = qt * 16;
    const float ninf = -__builtin_inff();

    // ---- stage: the Q tile (rows beyond n: zeros, never written out), empty lists ------------------------------------------
    const int c4n = E >> 2;
    for (int i = lane; i < 16 * c4n; i += PCG_WAVE) {
        const int r = i / c4n, c4 = i - r * c4n;
        const int row = row0 + r;
        float4 v = *reinterpret_cast<const float4 *>(Q + (size_t)(row < n ? row : n - 1) * E + 4 * c4);
        if (row >= n) v = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4 *>(s_q + r * ldq + 4 * c4) = v;
    }
    for (int i = lane; i < 16 * k; i += PCG_WAVE) {
        s_sc[i] = ninf;
        s_ps[i] = -1;
    }
    // this lane's four rows of a score tile: kq * 4 + i (the MFMA's C layout), its column lane & 15
    const int cn_ = lane & 15, kq = lane >> 4;
    float my_qn2[4];
    int my_qid[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = row0 + kq * 4 + i, rc = row < n ? row : n - 1;
        my_qn2[i] = metric != 0 ? qn2[rc] : 0.f;
        my_qid[i] = q_ids ? q_ids[rc] : 0;
    }
    wave_lds_sync();

    const int n_ct = (M + 15) >> 4;
    const int t_lo = slice * slice_tiles, t_hi = t_lo + slice_tiles < n_ct ? t_lo + slice_tiles : n_ct;
    const float *ap = s_q + cn_ * ldq + 4 * kq;
    for (int ct = t_lo; ct < t_hi; ++ct) {                                 // (bounded: slice_tiles)
        const int c = ct * 16 + cn_, cc = c < M ? c : M - 1;               // this lane's candidate (clamped: unconditional loads)
        const float my_cn2 = metric != 0 ? cn2[cc] : 0.f;
        const int my_cid = bank_ids ? bank_ids[cc] : 0;
        const f32x4 dot = tile_lds_globT4(ap, bank + (size_t)cc * E + 4 * kq, E >> 4);
        float thr_s[4];
        int thr_p[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            thr_s[i] = s_sc[(kq * 4 + i) * k + k - 1];
            thr_p[i] = s_ps[(kq * 4 + i) * k + k - 1];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float s = dot[i];
            if (metric == 1) {
                const float den = sqrtf(my_qn2[i]) * sqrtf(my_cn2);
                s = (my_qn2[i] > 0.f && my_cn2 > 0.f) ? s / den : 0.f;
            } else if (metric == 2) {
                s = fminf(0.f, fmaf(2.f, s, -my_qn2[i]) - my_cn2);
            }
            if (!(s == s)) s = ninf;
            const bool eligible = c < M && !(q_ids && my_cid == my_qid[i]);
            const bool cand = eligible && topk_before(s, c, thr_s[i], thr_p[i]);
            unsigned long long mask = __ballot(cand);
            while (mask) {                                                 // (bounded: 64 bits; wave-uniform)
                const int L = __builtin_ctzll(mask);
                mask &= mask - 1;
                const int r = (L >> 4) * 4 + i;
                const float ss = __shfl(s, L);
                const int sp = __shfl(c, L);
                // the whole wave inserts (ss, sp) into row r's list: lane j holds entry j
                const bool in = lane < k;
                const float e_s = in ? s_sc[r * k + lane] : ninf;
                const int e_p = in ? s_ps[r * k + lane] : -1;
                const int p = __builtin_popcountll(__ballot(in && topk_before(e_s, e_p, ss, sp)));   // (a prefix: the list is sorted)
                if (p < k) {
                    if (in && lane >= p && lane + 1 < k) {
                        s_sc[r * k + lane + 1] = e_s;
                        s_ps[r * k + lane + 1] = e_p;
                    }
                    if (lane == p) {
                        s_sc[r * k + p] = ss;
                        s_ps[r * k + p] = sp;
                    }
                }
                wave_lds_sync();
            }
        }
    }
    wave_lds_sync();
    // ---- the lists: consecutive lanes store consecutive entries -----------------------------------------------------------
    for (int i = lane; i < 16 * k; i += PCG_WAVE) {
        const int r = i / k, row = row0 + r;
        if (row < n) {
            const size_t at = ((size_t)slice * row_stride + row) * k + (i - r * k);
            out_score[at] = s_sc[i];
            out_pos[at] = s_ps[i];
        }
    }
}

// a wave per query row: lane s reads slice s's list [k] from its head
__global__ void __launch_bounds__(256) topk_merge_kernel(const int32_t *__restrict__ part_pos, const float *__restrict__ part_score,
                                                         int n, int k, int n_slices, int64_t row_stride,
                                                         int32_t *__restrict__ out_pos, float *__restrict__ out_score) {
    const int lane = threadIdx.x & 63;
    const int row = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;                                                  // (wave-uniform)
    const float ninf = -__builtin_inff();
    const bool mine = lane < n_slices;
    const size_t base = ((size_t)(mine ? lane : 0) * row_stride + row) * k;
    int head = 0;
    for (int j = 0; j < k; ++j) {                                          // (bounded: k <= 64)
        const int h = head < k ? head : k - 1;
        float s = part_score[base + h];
        int p = part_pos[base + h];
        if (!mine || head >= k) {
            s = ninf;
            p = -1;
        }
        float bs = s;
        int bp = p;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float os = __shfl_xor(bs, o);
            const int op = __shfl_xor(bp, o);
            if (topk_before(os, op, bs, bp)) {
                bs = os;
                bp = op;
            }
        }
        // (every lane holds the same best: the order is total over distinct positions, padding loses to everything)
        if (bp >= 0 && p == bp) ++head;
        if (lane == 0) {
            out_score[(size_t)row * k + j] = bp >= 0 ? bs : ninf;
            out_pos[(size_t)row * k + j] = bp;
        }
    }
}

struct TopkCarve {
    int64_t qn2, cn2, part_score, part_pos, total;
    int part_tiles;
};

static int topk_carve(int64_t n, int64_t M, int emb, int k, TopkCarve &c) {
    if (n < 0 || M < 0 || n >= (1ll << 31) - 16 || M >= (1ll << 31) - 16) return PCG_E_ARG;
    if (k < 1 || k > TOPK_MAX_K) return PCG_E_ARG;
    if (emb < 16 || emb > 512 || emb % 16 != 0) return PCG_E_UNSUPPORTED;
    const int64_t n_qt = (n + 15) / 16;
    const int64_t pt = n_qt * TOPK_MAX_SLICES < TOPK_PART_TILES ? n_qt * TOPK_MAX_SLICES : TOPK_PART_TILES;
    c.part_tiles = (int)pt;
    int64_t off = 0;
    c.qn2 = off; off += (4 * n + 255) & ~(int64_t)255;
    c.cn2 = off; off += (4 * M + 255) & ~(int64_t)255;
    c.part_score = off; off += 4 * pt * 16 * k;
    c.part_pos = off; off += 4 * pt * 16 * k;
    c.total = off + 256;
    return PCG_OK;
}

// waves per workgroup of the scan: 4, or 2 where four Q tiles and lists exceed the LDS
static int topk_waves(int emb, int k, size_t &smem) {
    for (int W = 4; W >= 2; W >>= 1) {
        smem = sizeof(float) * ((size_t)W * 16 * (emb + 4) + 2 * (size_t)W * 16 * k);
        if (smem <= (size_t)TOPK_SMEM_MAX) return W;
    }
    return 0;
}

}  // namespace pcg

extern "C" {

void pcg_debug_set_topk_slices(int32_t n_slices) { pcg::g_topk_force_slices = n_slices > 0 ? n_slices : 0; }

int64_t pcg_topk_similar_workspace_bytes(int32_t n, int32_t M, int32_t emb, int32_t k) {
    pcg::TopkCarve c;
    const int rc = pcg::topk_carve(n, M, emb, k, c);
    return rc != PCG_OK ? rc : c.total;
}

int pcg_topk_similar(const float *Q, int32_t n, const float *bank, int32_t M, int32_t emb, int32_t k, int32_t metric,
                     const int32_t *q_ids, const int32_t *bank_ids, int32_t *out_pos, float *out_score, void *workspace,
                     uint32_t *status, void *stream) {
    pcg::TopkCarve c;
    const int rc = pcg::topk_carve(n, M, emb, k, c);
    if (rc != PCG_OK) return rc;
    if (metric < 0 || metric > 2 || (q_ids == nullptr) != (bank_ids == nullptr)) return PCG_E_ARG;
    size_t smem = 0;
    const int W = pcg::topk_waves(emb, k, smem);
    if (W == 0) return PCG_E_UNSUPPORTED;
    if (n == 0) return PCG_OK;
    if (!Q || (M > 0 && !bank) || !out_pos || !out_score || !workspace || !status) return PCG_E_ARG;
    if (M == 0) bank = nullptr;                                             // (an empty table's address means nothing)
    if (((reinterpret_cast<uintptr_t>(Q) | reinterpret_cast<uintptr_t>(bank) | reinterpret_cast<uintptr_t>(workspace)) & 15u) != 0)
        return PCG_E_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    float *qn2 = reinterpret_cast<float *>(ws + c.qn2), *cn2 = reinterpret_cast<float *>(ws + c.cn2);
    float *part_score = reinterpret_cast<float *>(ws + c.part_score);
    int32_t *part_pos = reinterpret_cast<int32_t *>(ws + c.part_pos);

    const int n_qt = (n + 15) / 16, n_ct = (M + 15) / 16;
    // slices of the bank: enough waves to fill the device when the query tiles alone do not, each slice worth its lists' merge
    int S = pcg::g_topk_force_slices > 0 ? pcg::g_topk_force_slices : (2048 + n_qt - 1) / n_qt;
    if (pcg::g_topk_force_slices == 0 && S > n_ct / pcg::TOPK_MIN_SLICE_TILES) S = n_ct / pcg::TOPK_MIN_SLICE_TILES;
    if (S > pcg::TOPK_MAX_SLICES) S = pcg::TOPK_MAX_SLICES;
    if (S > c.part_tiles / n_qt) S = c.part_tiles / n_qt;
    if (S > n_ct) S = n_ct;
    if (S < 1) S = 1;
    const int slice_tiles = n_ct > 0 ? (n_ct + S - 1) / S : 1;
    S = n_ct > 0 ? (n_ct + slice_tiles - 1) / slice_tiles : 1;          // (no empty slice)

    if (metric != 0) {
        const int64_t rows = (int64_t)n + M;
        hipLaunchKernelGGL(pcg::topk_norms_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, Q, (int64_t)n, bank,
                           (int64_t)M, emb, qn2, cn2);
        PCG_LAUNCH_CHECK();
    }
    if (pcg::allow_dynamic_lds(pcg::topk_scan_kernel, pcg::TOPK_SMEM_MAX) != PCG_OK) return PCG_E_LAUNCH;
    const int64_t row_stride = (int64_t)n_qt * 16;
    hipLaunchKernelGGL(pcg::topk_scan_kernel, dim3((n_qt + W - 1) / W, S), dim3(64 * W), smem, st, Q, n, bank, M, emb, k, metric, q_ids,
                       bank_ids, qn2, cn2, slice_tiles, row_stride, S > 1 ? part_pos : out_pos, S > 1 ? part_score : out_score);
    PCG_LAUNCH_CHECK();
    if (S > 1) {
        hipLaunchKernelGGL(pcg::topk_merge_kernel, dim3((n + 3) / 4), dim3(256), 0, st, part_pos, part_score, n, k, S, row_stride,
                           out_pos, out_score);
        PCG_LAUNCH_CHECK();
    }
    return PCG_OK;
}

}  // extern "C"
