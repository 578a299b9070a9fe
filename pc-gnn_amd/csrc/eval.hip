// Device-side evaluation counts (gfx950, wave64): everything the reported metrics are functions of, as integers.
//   out = tp, fp, fn, tn, n1, n0, 2U, 0, tp_t[T], npred_t[T]                                      (uint64)
// from prob f32 [n, 2], labels i32 [n], thresholds f64 [T] ascending:
//   count pass   one stream over the rows: confusion counts of the argmax prediction, the threshold-bin histogram of p1, and
//                every row's orderable key appended to its class's key array (positives from the front of `keys`, negatives
//                from its back: one array of n words holds both);
//   finish       n1, n0, suffix sums of the histogram -> tp_t, npred_t; picks the class to sort (the smaller one);
//   sort         LSD radix sort of that class's keys, 8-bit digits, stable; one workgroup below SMALL_SORT_MAX keys, tiles + a
//                scan of the per-tile digit counts above;
//   rank pass    every key of the other class: lower and upper bound in the sorted keys, summed into 2U.
// All sums are integer sums (LDS / global integer atomics, one global atomic per counter and workgroup): the result does not
// depend on the order anything ran in.  No float atomics, no host round trip, nothing allocated, nothing synchronised.
#include "common.h"

namespace pcg {

constexpr int EVAL_MAX_T = 1024;
constexpr int EVAL_CTR_WORDS = 16;            // ctr[0..3] tp fp fn tn | 4 pos cursor | 5 neg cursor | 6 m | 7 sorted-is-pos
                                              // | 8 sorted offset | 9 other offset | 10 other count; then hist [T + 1][2]
constexpr int EVAL_COUNT_THREADS = 256;
constexpr int EVAL_COUNT_ROWS = 8;            // rows per thread and iteration: a workgroup appends 2048 keys per pair of atomics
constexpr int SMALL_SORT_MAX = 65536;         // keys one workgroup sorts by itself (n <= 2 * SMALL_SORT_MAX takes that path)
constexpr int SMALL_SORT_THREADS = 1024;
constexpr int TILE_SORT_THREADS = 256;
constexpr int64_t TILE_MIN = 4096;
constexpr int64_t TILE_MAX_BLOCKS = 2048;

struct EvalCarve {
    int64_t ctr, keys, tmp, hist, total;      // byte offsets
    int64_t n_max, tile, n_tiles;             // keys the sorted class can have; keys per tile; tiles
};

__host__ inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

__host__ inline void eval_carve(int64_t n, int32_t T, EvalCarve &c) {
    c.n_max = n / 2;                                                   // the smaller class
    int64_t tile = (c.n_max + TILE_MAX_BLOCKS - 1) / TILE_MAX_BLOCKS;
    tile = (tile + 1023) / 1024 * 1024;
    c.tile = tile < TILE_MIN ? TILE_MIN : tile;
    c.n_tiles = c.n_max > SMALL_SORT_MAX ? (c.n_max + c.tile - 1) / c.tile : 0;
    c.ctr = 0;
    c.keys = align256(8 * (int64_t)(EVAL_CTR_WORDS + 2 * (T + 1)));
    c.tmp = c.keys + align256(4 * (n + 1));
    c.hist = c.tmp + align256(4 * (c.n_max + 1));
    c.total = c.hist + align256(4 * 256 * (c.n_tiles + 1));
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;                                                          // (lane 0 holds the wave's sum)
}

__global__ void __launch_bounds__(256) eval_zero_kernel(uint64_t *__restrict__ ctr, int n_ctr, uint64_t *__restrict__ out, int n_out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_ctr + n_out; i += gridDim.x * blockDim.x) {
        if (i < n_ctr) ctr[i] = 0ull;
        else out[i - n_ctr] = 0ull;
    }
}

// ---- count pass ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(EVAL_COUNT_THREADS)
eval_count_kernel(const float *__restrict__ prob, const int32_t *__restrict__ labels, int64_t n, const double *__restrict__ thresholds,
                  int T, uint64_t *__restrict__ ctr, uint32_t *__restrict__ keys, uint32_t *__restrict__ status) {
    __shared__ double th[EVAL_MAX_T];
    __shared__ uint32_t hist[(EVAL_MAX_T + 1) * 2];
    __shared__ uint32_t cur[2];               // this iteration's append cursors (positives, negatives)
    __shared__ uint64_t gbase[2];             // where this iteration's keys start in their class's array
    __shared__ unsigned long long conf[4];
    const int tid = threadIdx.x, lane = lane_id();
    for (int i = tid; i < T; i += blockDim.x) th[i] = thresholds[i];
    for (int i = tid; i < 2 * (T + 1); i += blockDim.x) hist[i] = 0u;
    if (tid < 4) conf[tid] = 0ull;
    if (tid < 2) cur[tid] = 0u;
    __syncthreads();

    uint32_t c_tp = 0, c_fp = 0, c_fn = 0, c_tn = 0;
    bool bad = false;
    const int64_t per_iter = (int64_t)EVAL_COUNT_THREADS * EVAL_COUNT_ROWS;
    for (int64_t base = (int64_t)blockIdx.x * per_iter; base < n; base += (int64_t)gridDim.x * per_iter) {
        float2 p[EVAL_COUNT_ROWS];
        int32_t lab[EVAL_COUNT_ROWS];
#pragma unroll
        for (int r = 0; r < EVAL_COUNT_ROWS; ++r) {                    // (unconditional loads, index clamped)
            const int64_t row = base + (int64_t)r * EVAL_COUNT_THREADS + tid;
            const int64_t rc = row < n ? row : n - 1;
            p[r] = reinterpret_cast<const float2 *>(prob)[rc];
            lab[r] = labels[rc];
        }
        uint32_t key[EVAL_COUNT_ROWS], off[EVAL_COUNT_ROWS];
#pragma unroll
        for (int r = 0; r < EVAL_COUNT_ROWS; ++r) {
            const int64_t row = base + (int64_t)r * EVAL_COUNT_THREADS + tid;
            const bool ok = row < n;
            const float p0 = p[r].x, p1 = p[r].y;
            bad |= ok && ((lab[r] != 0 && lab[r] != 1) || p0 != p0 || p1 != p1);
            const int y = lab[r] != 0 ? 1 : 0;
            const int pred = p1 > p0 ? 1 : 0;                           // numpy argmax: ties (and NaN) to class 0
            c_tp += ok && y && pred;
            c_fp += ok && !y && pred;
            c_fn += ok && y && !pred;
            c_tn += ok && !y && !pred;
            // bin = number of thresholds < p1 (ascending thresholds: a prefix)
            const double pd = (double)p1;
            int lo = 0, hi = T;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (th[mid] < pd) lo = mid + 1;
                else hi = mid;
            }
            if (ok) atomicAdd(&hist[2 * lo + y], 1u);
            key[r] = orderable(p1 + 0.0f);
            // wave-aggregated append into this iteration's cursors
            const uint64_t mpos = __ballot(ok && y), mneg = __ballot(ok && !y);
            uint32_t bp = 0, bn = 0;
            if (lane == 0) {
                if (mpos) bp = atomicAdd(&cur[0], (uint32_t)__popcll(mpos));
                if (mneg) bn = atomicAdd(&cur[1], (uint32_t)__popcll(mneg));
            }
            bp = __shfl(bp, 0);
            bn = __shfl(bn, 0);
            off[r] = !ok ? 0xffffffffu
                         : (y ? bp + (uint32_t)__popcll(mpos & lanemask_lt()) : bn + (uint32_t)__popcll(mneg & lanemask_lt()));
            lab[r] = y;
        }
        __syncthreads();
        if (tid < 2) {
            const uint32_t c = cur[tid];
            gbase[tid] = c ? atomicAdd(reinterpret_cast<unsigned long long *>(&ctr[4 + tid]), (unsigned long long)c) : 0ull;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < EVAL_COUNT_ROWS; ++r) {
            if (off[r] == 0xffffffffu) continue;
            const uint64_t at = gbase[lab[r] ? 0 : 1] + off[r];        // (a counter's value: clamped to the array)
            if (at < (uint64_t)n) keys[lab[r] ? at : (uint64_t)n - 1 - at] = key[r];
        }
        if (tid < 2) cur[tid] = 0u;
        __syncthreads();
    }
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(status, (uint32_t)PCG_ST_EVAL_INPUT);
    const uint64_t s_tp = wave_sum64(c_tp), s_fp = wave_sum64(c_fp), s_fn = wave_sum64(c_fn), s_tn = wave_sum64(c_tn);
    if (lane == 0) {
        atomicAdd(&conf[0], (unsigned long long)s_tp);
        atomicAdd(&conf[1], (unsigned long long)s_fp);
        atomicAdd(&conf[2], (unsigned long long)s_fn);
        atomicAdd(&conf[3], (unsigned long long)s_tn);
    }
    __syncthreads();
    if (tid < 4 && conf[tid]) atomicAdd(reinterpret_cast<unsigned long long *>(&ctr[tid]), conf[tid]);
    uint64_t *ghist = ctr + EVAL_CTR_WORDS;
    for (int i = tid; i < 2 * (T + 1); i += blockDim.x)
        if (hist[i]) atomicAdd(reinterpret_cast<unsigned long long *>(&ghist[i]), (unsigned long long)hist[i]);
}

// ---- finish: the confusion words, the threshold sweep's suffix sums, and which class is sorted --------------------------------
__global__ void __launch_bounds__(1024)
eval_finish_kernel(uint64_t *__restrict__ ctr, int T, int64_t n, int64_t n_max, uint64_t *__restrict__ out) {
    __shared__ uint64_t h[(EVAL_MAX_T + 1) * 2];
    const int tid = threadIdx.x;
    for (int i = tid; i < 2 * (T + 1); i += blockDim.x) h[i] = ctr[EVAL_CTR_WORDS + i];
    __syncthreads();
    for (int t = tid; t < T; t += blockDim.x) {
        uint64_t tp = 0, np = 0;
        for (int b = t + 1; b <= T; ++b) {                             // p > thresholds[t]  <=>  bin > t
            tp += h[2 * b + 1];
            np += h[2 * b] + h[2 * b + 1];
        }
        out[8 + t] = tp;
        out[8 + T + t] = np;
    }
    if (tid == 0) {
        const uint64_t tp = ctr[0], fp = ctr[1], fn = ctr[2], tn = ctr[3];
        const uint64_t n1 = tp + fn, n0 = fp + tn;
        out[0] = tp, out[1] = fp, out[2] = fn, out[3] = tn, out[4] = n1, out[5] = n0;
        const bool pos_sorted = n1 <= n0;
        uint64_t m = pos_sorted ? n1 : n0, others = pos_sorted ? n0 : n1;
        if (m > (uint64_t)n_max) m = (uint64_t)n_max;                  // (cannot happen: n1 + n0 == n; clamped all the same)
        if (others > (uint64_t)n) others = (uint64_t)n;
        ctr[6] = m;
        ctr[7] = pos_sorted ? 1 : 0;
        ctr[8] = pos_sorted ? 0 : (uint64_t)n - m;                     // positives fill keys from the front, negatives from the back
        ctr[9] = pos_sorted ? (uint64_t)n - others : 0;
        ctr[10] = others;
    }
}

// ---- LSD radix sort, 8-bit digits --------------------------------------------------------------------------------------------
// One pass over keys [begin, end) of `in` by a workgroup of W waves: wave w owns the contiguous stretch w of the range, so
// (tile, wave, position in the stretch) is the input order and a key's place is
//     base(digit) + keys of that digit in earlier tiles + in earlier waves' stretches + earlier in this wave's stretch.
// wcnt[w][d] first counts (phase A), then holds the running place (phases B, C).  gbase: where this tile's keys of every digit
// start (the scanned per-tile counts), or null: the range is the whole array and the digit bases are formed here.
template <int W>
__device__ __forceinline__ void radix_pass_body(const uint32_t *in, uint32_t *out, int64_t begin, int64_t end,
                                                int64_t m, int shift, const uint32_t *__restrict__ gbase, int64_t gstride,
                                                uint32_t (*wcnt)[256], uint32_t *tot) {
    const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    for (int i = tid; i < W * 256; i += W * 64) wcnt[i >> 8][i & 255] = 0u;
    __syncthreads();
    const int64_t len = end - begin;
    const int64_t per = ((len + W - 1) / W + 63) & ~(int64_t)63;
    int64_t wb = begin + (int64_t)w * per, we = wb + per;
    if (wb > end) wb = end;
    if (we > end) we = end;
    for (int64_t i = wb + lane; i < we; i += 64) atomicAdd(&wcnt[w][(in[i] >> shift) & 255u], 1u);            // phase A
    __syncthreads();
    if (tid < 256) {                                                                                              // phase B
        uint32_t s = 0;
#pragma unroll
        for (int k = 0; k < W; ++k) s += wcnt[k][tid];
        tot[tid] = s;
    }
    __syncthreads();
    if (tid < 256) {
        uint32_t at;
        if (gbase) {
            at = gbase[(int64_t)tid * gstride];
        } else {
            at = 0;
            for (int d = 0; d < tid; ++d) at += tot[d];
        }
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const uint32_t c = wcnt[k][tid];
            wcnt[k][tid] = at;
            at += c;
        }
    }
    __syncthreads();
    volatile uint32_t *mine = wcnt[w];                                                                            // phase C
    for (int64_t i0 = wb; i0 < we; i0 += 64) {
        const int64_t i = i0 + lane;
        const bool ok = i < we;
        const uint32_t k = ok ? in[i] : 0u;
        const uint32_t d = (k >> shift) & 255u;
        uint64_t peers = __ballot(ok);                                 // the lanes that hold this lane's digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const uint64_t v = __ballot(bit);
            peers &= bit ? v : ~v;
        }
        const uint32_t before = (uint32_t)__popcll(peers & lanemask_lt());
        uint32_t place = 0;
        if (ok) place = mine[d];
        __builtin_amdgcn_wave_barrier();
        if (ok && before == 0) mine[d] = place + (uint32_t)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
        const uint64_t at = (uint64_t)place + before;
        if (ok && at < (uint64_t)m) out[at] = k;                       // (a counter's value: clamped to the array)
    }
    __syncthreads();
}

// the whole sort by ONE workgroup (m <= SMALL_SORT_MAX): four passes keys -> tmp -> keys -> tmp -> keys
__global__ void __launch_bounds__(SMALL_SORT_THREADS)
eval_sort_small_kernel(const uint64_t *__restrict__ ctr, uint32_t *__restrict__ keys, uint32_t *__restrict__ tmp, int64_t n, int64_t n_max) {
    __shared__ uint32_t wcnt[SMALL_SORT_THREADS / 64][256];
    __shared__ uint32_t tot[256];
    int64_t m = (int64_t)ctr[6], off = (int64_t)ctr[8];
    if (m > n_max) m = n_max;
    if (off < 0 || off + m > n) return;
    uint32_t *a = keys + off, *b = tmp;
    for (int pass = 0; pass < 4; ++pass) {
        radix_pass_body<SMALL_SORT_THREADS / 64>(a, b, 0, m, m, 8 * pass, nullptr, 0, wcnt, tot);
        __threadfence_block();
        uint32_t *t = a;
        a = b;
        b = t;
    }
}

// tiled path, three launches per pass: per-tile digit counts -> exclusive scan (digit-major, tile-minor) -> scatter
__global__ void __launch_bounds__(TILE_SORT_THREADS)
eval_sort_hist_kernel(const uint64_t *__restrict__ ctr, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ tmp, int64_t n,
                      int64_t n_max, int64_t tile, int pass, uint32_t *__restrict__ hist) {
    __shared__ uint32_t cnt[256];
    int64_t m = (int64_t)ctr[6], off = (int64_t)ctr[8];
    if (m > n_max) m = n_max;
    if (off < 0 || off + m > n) m = 0;
    const uint32_t *in = (pass & 1) ? tmp : keys + off;
    const int tid = threadIdx.x;
    cnt[tid] = 0u;
    __syncthreads();
    const int64_t begin = (int64_t)blockIdx.x * tile;
    int64_t end = begin + tile;
    if (end > m) end = m;
    for (int64_t i = begin + tid; i < end; i += TILE_SORT_THREADS) atomicAdd(&cnt[(in[i] >> (8 * pass)) & 255u], 1u);
    __syncthreads();
    hist[(int64_t)tid * gridDim.x + blockIdx.x] = cnt[tid];
}

__global__ void __launch_bounds__(1024) eval_sort_scan_kernel(uint32_t *__restrict__ hist, int64_t len) {
    __shared__ uint32_t part[1024];
    const int tid = threadIdx.x;
    const int64_t per = (len + 1023) / 1024;
    int64_t b = (int64_t)tid * per, e = b + per;
    if (b > len) b = len;
    if (e > len) e = len;
    uint32_t s = 0;
    for (int64_t i = b; i < e; ++i) s += hist[i];
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                               // inclusive scan of the 1024 partial sums
        const uint32_t v = tid >= o ? part[tid - o] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint32_t at = part[tid] - s;
    for (int64_t i = b; i < e; ++i) {
        const uint32_t c = hist[i];
        hist[i] = at;
        at += c;
    }
}

__global__ void __launch_bounds__(TILE_SORT_THREADS)
eval_sort_scatter_kernel(const uint64_t *__restrict__ ctr, uint32_t *__restrict__ keys, uint32_t *__restrict__ tmp, int64_t n, int64_t n_max,
                         int64_t tile, int pass, const uint32_t *__restrict__ hist) {
    __shared__ uint32_t wcnt[TILE_SORT_THREADS / 64][256];
    __shared__ uint32_t tot[256];
    int64_t m = (int64_t)ctr[6], off = (int64_t)ctr[8];
    if (m > n_max) m = n_max;
    if (off < 0 || off + m > n) return;
    const int64_t begin = (int64_t)blockIdx.x * tile;
    if (begin >= m) return;                                            // (workgroup-uniform)
    int64_t end = begin + tile;
    if (end > m) end = m;
    const uint32_t *in = (pass & 1) ? tmp : keys + off;
    uint32_t *out = (pass & 1) ? keys + off : tmp;
    radix_pass_body<TILE_SORT_THREADS / 64>(in, out, begin, end, m, 8 * pass, hist + blockIdx.x, gridDim.x, wcnt, tot);
}

// ---- rank pass: 2U = sum over the other class's keys of (lower bound + upper bound) in the sorted class --------------------------
__global__ void __launch_bounds__(256)
eval_rank_kernel(const uint64_t *__restrict__ ctr, const uint32_t *__restrict__ keys, int64_t n, int64_t n_max, uint64_t *__restrict__ out) {
    __shared__ unsigned long long acc;
    int64_t m = (int64_t)ctr[6], s_off = (int64_t)ctr[8], o_off = (int64_t)ctr[9], n_o = (int64_t)ctr[10];
    const bool pos_sorted = ctr[7] != 0ull;
    if (m > n_max) m = n_max;
    if (s_off < 0 || s_off + m > n || o_off < 0 || n_o < 0 || o_off + n_o > n) return;
    if (m == 0 || n_o == 0) return;                                    // (one class absent: 2U stays 0, the host raises)
    const uint32_t *S = keys + s_off, *O = keys + o_off;
    if (threadIdx.x == 0) acc = 0ull;
    __syncthreads();
    uint64_t sum = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_o; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t k = O[i];
        int64_t lo = 0, hi = m;
        while (lo < hi) {                                              // lb = #{S < k}
            const int64_t mid = (lo + hi) >> 1;
            if (S[mid] < k) lo = mid + 1;
            else hi = mid;
        }
        const int64_t lb = lo;
        int64_t ub = lb;
        if (lb < m && S[lb] == k) {                                    // ties: ub = #{S <= k}, searched from lb on
            int64_t step = 1;
            hi = lb + 1;
            while (hi < m && S[hi] == k) {                             // gallop
                lo = hi;
                step <<= 1;
                hi = lb + step;
            }
            if (hi > m) hi = m;
            lo = lo < lb + 1 ? lb + 1 : lo;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (S[mid] <= k) lo = mid + 1;
                else hi = mid;
            }
            ub = lo;
        }
        // positives sorted, k a negative: 2 #{pos > k} + #{pos == k};  negatives sorted, k a positive: 2 #{neg < k} + #{neg == k}
        sum += pos_sorted ? (uint64_t)((m - lb) + (m - ub)) : (uint64_t)(lb + ub);
    }
    sum = wave_sum64(sum);
    if (lane_id() == 0 && sum) atomicAdd(&acc, (unsigned long long)sum);
    __syncthreads();
    if (threadIdx.x == 0 && acc) atomicAdd(reinterpret_cast<unsigned long long *>(&out[6]), acc);
}

}  // namespace pcg

extern "C" {

int64_t pcg_eval_workspace_bytes(int64_t n, int32_t n_thresholds) {
    if (n < 0 || n > 0x7fffffffll || n_thresholds < 1 || n_thresholds > pcg::EVAL_MAX_T) return PCG_E_ARG;
    pcg::EvalCarve c;
    pcg::eval_carve(n, n_thresholds, c);
    return c.total;
}

int pcg_eval_counts(const float *prob, const int32_t *labels, int64_t n, const double *thresholds, int32_t n_thresholds,
                    void *workspace, uint64_t *out, uint32_t *status, void *stream) {
    if (n < 0 || n > 0x7fffffffll || n_thresholds < 1 || n_thresholds > pcg::EVAL_MAX_T) return PCG_E_ARG;
    if (!thresholds || !workspace || !out || !status || (n > 0 && (!prob || !labels))) return PCG_E_ARG;
    if ((reinterpret_cast<uintptr_t>(prob) & 7u) != 0 || (reinterpret_cast<uintptr_t>(workspace) & 7u) != 0 ||
        (reinterpret_cast<uintptr_t>(out) & 7u) != 0 || (reinterpret_cast<uintptr_t>(thresholds) & 7u) != 0)
        return PCG_E_ARG;
    const int T = n_thresholds;
    pcg::EvalCarve c;
    pcg::eval_carve(n, T, c);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    uint64_t *ctr = reinterpret_cast<uint64_t *>(ws + c.ctr);
    uint32_t *keys = reinterpret_cast<uint32_t *>(ws + c.keys), *tmp = reinterpret_cast<uint32_t *>(ws + c.tmp);
    uint32_t *hist = reinterpret_cast<uint32_t *>(ws + c.hist);
    hipStream_t st = static_cast<hipStream_t>(stream);

    const int n_ctr = pcg::EVAL_CTR_WORDS + 2 * (T + 1), n_out = 8 + 2 * T;
    hipLaunchKernelGGL(pcg::eval_zero_kernel, dim3((n_ctr + n_out + 255) / 256), dim3(256), 0, st, ctr, n_ctr, out, n_out);
    PCG_LAUNCH_CHECK();
    if (n == 0) return PCG_OK;

    const int64_t per_iter = (int64_t)pcg::EVAL_COUNT_THREADS * pcg::EVAL_COUNT_ROWS;
    int64_t blocks = (n + per_iter - 1) / per_iter;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(pcg::eval_count_kernel, dim3((unsigned)blocks), dim3(pcg::EVAL_COUNT_THREADS), 0, st, prob, labels, n, thresholds,
                       T, ctr, keys, status);
    PCG_LAUNCH_CHECK();
    hipLaunchKernelGGL(pcg::eval_finish_kernel, dim3(1), dim3(1024), 0, st, ctr, T, n, c.n_max, out);
    PCG_LAUNCH_CHECK();
    if (c.n_max == 0) return PCG_OK;                                   // (n == 1: no pair)

    if (c.n_tiles == 0) {
        hipLaunchKernelGGL(pcg::eval_sort_small_kernel, dim3(1), dim3(pcg::SMALL_SORT_THREADS), 0, st, ctr, keys, tmp, n, c.n_max);
        PCG_LAUNCH_CHECK();
    } else {
        for (int pass = 0; pass < 4; ++pass) {
            hipLaunchKernelGGL(pcg::eval_sort_hist_kernel, dim3((unsigned)c.n_tiles), dim3(pcg::TILE_SORT_THREADS), 0, st, ctr, keys, tmp,
                               n, c.n_max, c.tile, pass, hist);
            PCG_LAUNCH_CHECK();
            hipLaunchKernelGGL(pcg::eval_sort_scan_kernel, dim3(1), dim3(1024), 0, st, hist, 256 * c.n_tiles);
            PCG_LAUNCH_CHECK();
            hipLaunchKernelGGL(pcg::eval_sort_scatter_kernel, dim3((unsigned)c.n_tiles), dim3(pcg::TILE_SORT_THREADS), 0, st, ctr, keys,
                               tmp, n, c.n_max, c.tile, pass, hist);
            PCG_LAUNCH_CHECK();
        }
    }
    int64_t rblocks = (n + 1023) / 1024;
    if (rblocks > 2048) rblocks = 2048;
    hipLaunchKernelGGL(pcg::eval_rank_kernel, dim3((unsigned)rblocks), dim3(256), 0, st, ctr, keys, n, c.n_max, out);
    PCG_LAUNCH_CHECK();
    return PCG_OK;
}

}  // extern "C"
