// Ranking metrics and the top-k alert list on the device (gfx950, wave64), in the style of eval.hip: integers on the device, the
// float64 statements on the host.  A row's key is orderable(p1 + 0.0f) (-0.0 ties with +0.0).
//
// pcg_pr_counts    hdr = tp, fp, fn, tn, n1, n0, G, 0 (uint64) and the G points of the precision-recall curve at which recall
//                  changes, tp_g / npred_g, in descending score order:
//   count pass   one stream over the rows: confusion counts of the argmax prediction, the positives' keys appended to `keys`,
//                every row's bin zeroed;
//   finish       hdr[0..5], m = n1;
//   sort         LSD radix sort of the positives' keys, 8-bit digits, stable (eval.hip's: one workgroup up to SMALL_SORT_MAX
//                keys, tiles + a scan of the per-tile digit counts above - the kernels of the path not taken return at once,
//                because which one it is is known on the device only);
//   bin pass     every row: ub = #{sorted positives <= key} (bisection); bins[ub - 1] += 1 (a row below every positive counts
//                nowhere) - counted in LDS per (row slab, window of 16384 bins) and added with few global atomics up to 524288
//                positives, one global add per row above;
//   heads        a sorted key that differs from its predecessor heads a group: per-tile sums of bins and of heads -> suffix
//                scan of the tile sums (one workgroup; writes G) -> per tile, walked from the top: the g-th head from the top,
//                at index h, gives tp_g = m - h, npred_g = sum of bins[h ..].
// pcg_topk_alerts  the first min(k, n) rows of the stable descending sort by key, as (position, score):
//   select       radix select of the ke-th largest key, 8-bit digits from the top: a histogram launch per digit (LDS histogram per
//                workgroup, global integer atomics); every workgroup of the NEXT launch picks the digit from the finished histogram
//                itself (256 words), so there is no launch between the passes;
//   compact      position-ordered: per-tile counts of the rows above / equal to the ke-th key -> scan (one workgroup) -> scatter of
//                every row above it and of the first (ke - above) rows equal to it by position;
//   sort         stable LSD radix sort of the (~key, position) pairs by one workgroup: equal keys keep position order.
// All sums are integer sums; no float atomics, no host round trip, nothing allocated, no waits between workgroups (launches are
// separated instead).  Every device-side counter that indexes memory is clamped to its array.
#include "common.h"

namespace pcg {
namespace rankeval {

constexpr int CTR_WORDS = 16;                 // u64: ctr[0..3] tp fp fn tn | 4 positives' append cursor | 6 m (= n1, clamped to n)
constexpr int COUNT_THREADS = 256;
constexpr int COUNT_ROWS = 8;                 // rows per thread and iteration: a workgroup takes 2048 rows per iteration
constexpr int SMALL_SORT_MAX = 65536;         // keys one workgroup sorts by itself
constexpr int SMALL_SORT_THREADS = 1024;
constexpr int TILE_THREADS = 256;
constexpr int64_t TILE_MIN = 4096;
constexpr int64_t MAX_TILES = 2048;           // tiles of the sort / the head scan, and of the alert compaction
constexpr int64_t GRID_CAP = 2048;            // workgroups of the grid-stride passes
constexpr int WIN_BINS = 16384;               // bins a workgroup of the bin pass counts in LDS (64 KB)
constexpr int WIN_MAX = 32;                   // windows of the windowed bin pass: up to 524288 positives
constexpr int WIN_SLABS = 8;                  // row slabs per window
constexpr int WIN_THREADS = 1024;
constexpr int64_t AL_TILE_MIN = 2048;
constexpr int AL_CTR_WORDS = 64;              // u32: 0 the ke-th largest key | 1 rows equal to it that are taken

struct PrCarve {
    int64_t ctr, keys, tmp, bins, hist, tot, total;                    // byte offsets
    int64_t tile, n_tiles;                                             // keys per tile; tiles (of the capacity n)
};

struct AlCarve {
    int64_t ctr, hist, tcnt, cand, total;
    int64_t tile, n_tiles;
};

__host__ inline int64_t up256(int64_t x) { return (x + 255) & ~(int64_t)255; }

__host__ inline void pr_carve(int64_t n, PrCarve &c) {
    int64_t tile = (n + MAX_TILES - 1) / MAX_TILES;
    tile = (tile + 1023) / 1024 * 1024;
    c.tile = tile < TILE_MIN ? TILE_MIN : tile;
    c.n_tiles = (n + c.tile - 1) / c.tile;
    c.ctr = 0;
    c.keys = up256(8 * (int64_t)CTR_WORDS);
    c.tmp = c.keys + up256(4 * (n + 1));
    c.bins = c.tmp + up256(4 * (n + 1));
    c.hist = c.bins + up256(4 * (n + 1));
    c.tot = c.hist + up256(4 * 256 * (c.n_tiles + 1));
    c.total = c.tot + up256(4 * 2 * (c.n_tiles + 1));
}

__host__ inline void al_carve(int64_t n, int32_t k, AlCarve &c) {
    int64_t tile = (n + MAX_TILES - 1) / MAX_TILES;
    tile = (tile + AL_TILE_MIN - 1) / AL_TILE_MIN * AL_TILE_MIN;
    c.tile = tile < AL_TILE_MIN ? AL_TILE_MIN : tile;
    c.n_tiles = (n + c.tile - 1) / c.tile;
    c.ctr = 0;
    c.hist = up256(4 * (int64_t)AL_CTR_WORDS);
    c.tcnt = c.hist + up256(4 * 4 * 256);
    c.cand = c.tcnt + up256(4 * 2 * (c.n_tiles + 1));
    c.total = c.cand + 4 * up256(4 * (int64_t)k);                      // keys and positions, each in and out
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;                                                          // (lane 0 holds the wave's sum)
}

__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// One LSD pass (eval.hip's radix_pass_body, restated here so that pcg_eval_counts keeps its code; PAIRS: every key carries a
// 32-bit value along).  Keys [begin, end) of `in` by a workgroup of W waves: wave w owns the contiguous stretch w of the range,
// so (tile, wave, position in the stretch) is the input order and a key's place is
//     base(digit) + keys of that digit in earlier tiles + in earlier waves' stretches + earlier in this wave's stretch.
// gbase: where this tile's keys of every digit start, or null: the range is the whole array and the bases are formed here.
template <int W, bool PAIRS>
__device__ __forceinline__ void radix_pass(const uint32_t *in, uint32_t *out, const uint32_t *in_v, uint32_t *out_v, int64_t begin,
                                           int64_t end, int64_t m, int shift, const uint32_t *__restrict__ gbase, int64_t gstride,
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
        uint32_t v = 0u;
        if constexpr (PAIRS) v = ok ? in_v[i] : 0u;
        const uint32_t d = (k >> shift) & 255u;
        uint64_t peers = __ballot(ok);                                 // the lanes that hold this lane's digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const uint64_t bv = __ballot(bit);
            peers &= bit ? bv : ~bv;
        }
        const uint32_t before = (uint32_t)__popcll(peers & lanemask_lt());
        uint32_t place = 0;
        if (ok) place = mine[d];
        __builtin_amdgcn_wave_barrier();
        if (ok && before == 0) mine[d] = place + (uint32_t)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
        const uint64_t at = (uint64_t)place + before;
        if (ok && at < (uint64_t)m) {                                  // (a counter's value: clamped to the array)
            out[at] = k;
            if constexpr (PAIRS) out_v[at] = v;
        }
    }
    __syncthreads();
}

// ============================================================ pcg_pr_counts ========================================================
__global__ void __launch_bounds__(64) pr_zero_kernel(uint64_t *__restrict__ ctr, uint64_t *__restrict__ hdr) {
    const int i = threadIdx.x;
    if (i < CTR_WORDS) ctr[i] = 0ull;
    if (i < 8) hdr[i] = 0ull;
}

__global__ void __launch_bounds__(COUNT_THREADS)
pr_count_kernel(const float *__restrict__ prob, const int32_t *__restrict__ labels, int64_t n, uint64_t *__restrict__ ctr,
                uint32_t *__restrict__ keys, uint32_t *__restrict__ bins, uint32_t *__restrict__ status) {
    __shared__ uint32_t cur;                  // this iteration's append cursor
    __shared__ uint64_t gbase;                // where this iteration's keys start in `keys`
    __shared__ unsigned long long conf[4];
    const int tid = threadIdx.x, lane = lane_id();
    if (tid < 4) conf[tid] = 0ull;
    if (tid == 0) cur = 0u;
    __syncthreads();

    uint32_t c_tp = 0, c_fp = 0, c_fn = 0, c_tn = 0;
    bool bad = false;
    const int64_t per_iter = (int64_t)COUNT_THREADS * COUNT_ROWS;
    for (int64_t base = (int64_t)blockIdx.x * per_iter; base < n; base += (int64_t)gridDim.x * per_iter) {
        float2 p[COUNT_ROWS];
        int32_t lab[COUNT_ROWS];
#pragma unroll
        for (int r = 0; r < COUNT_ROWS; ++r) {                         // (unconditional loads, index clamped)
            const int64_t row = base + (int64_t)r * COUNT_THREADS + tid;
            const int64_t rc = row < n ? row : n - 1;
            p[r] = reinterpret_cast<const float2 *>(prob)[rc];
            lab[r] = labels[rc];
        }
        uint32_t key[COUNT_ROWS], off[COUNT_ROWS];
#pragma unroll
        for (int r = 0; r < COUNT_ROWS; ++r) {
            const int64_t row = base + (int64_t)r * COUNT_THREADS + tid;
            const bool ok = row < n;
            const float p0 = p[r].x, p1 = p[r].y;
            bad |= ok && ((lab[r] != 0 && lab[r] != 1) || p0 != p0 || p1 != p1);
            const int y = lab[r] != 0 ? 1 : 0;
            const int pred = p1 > p0 ? 1 : 0;                           // numpy argmax: ties (and NaN) to class 0
            c_tp += ok && y && pred;
            c_fp += ok && !y && pred;
            c_fn += ok && y && !pred;
            c_tn += ok && !y && !pred;
            key[r] = orderable(p1 + 0.0f);
            if (ok) bins[row] = 0u;
            const uint64_t mpos = __ballot(ok && y);                   // wave-aggregated append into this iteration's cursor
            uint32_t bp = 0;
            if (lane == 0 && mpos) bp = atomicAdd(&cur, (uint32_t)__popcll(mpos));
            bp = __shfl(bp, 0);
            off[r] = (ok && y) ? bp + (uint32_t)__popcll(mpos & lanemask_lt()) : 0xffffffffu;
        }
        __syncthreads();
        if (tid == 0) {
            const uint32_t c = cur;
            gbase = c ? atomicAdd(reinterpret_cast<unsigned long long *>(&ctr[4]), (unsigned long long)c) : 0ull;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < COUNT_ROWS; ++r) {
            if (off[r] == 0xffffffffu) continue;
            const uint64_t at = gbase + off[r];                        // (a counter's value: clamped to the array)
            if (at < (uint64_t)n) keys[at] = key[r];
        }
        if (tid == 0) cur = 0u;
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
}

__global__ void __launch_bounds__(64) pr_finish_kernel(uint64_t *__restrict__ ctr, int64_t n, uint64_t *__restrict__ hdr) {
    if (threadIdx.x != 0) return;
    const uint64_t tp = ctr[0], fp = ctr[1], fn = ctr[2], tn = ctr[3];
    const uint64_t n1 = tp + fn, n0 = fp + tn;
    hdr[0] = tp, hdr[1] = fp, hdr[2] = fn, hdr[3] = tn, hdr[4] = n1, hdr[5] = n0;
    ctr[6] = n1 > (uint64_t)n ? (uint64_t)n : n1;                     // (cannot exceed n; clamped all the same)
}

__device__ __forceinline__ int64_t pr_m(const uint64_t *ctr, int64_t n) {
    const int64_t m = (int64_t)ctr[6];
    return m < 0 ? 0 : (m > n ? n : m);
}

// the whole sort by ONE workgroup (m <= SMALL_SORT_MAX): four passes keys -> tmp -> keys -> tmp -> keys
__global__ void __launch_bounds__(SMALL_SORT_THREADS)
pr_sort_small_kernel(const uint64_t *__restrict__ ctr, uint32_t *__restrict__ keys, uint32_t *__restrict__ tmp, int64_t n) {
    __shared__ uint32_t wcnt[SMALL_SORT_THREADS / 64][256];
    __shared__ uint32_t tot[256];
    const int64_t m = pr_m(ctr, n);
    if (m > SMALL_SORT_MAX) return;                                    // (the tiled launches sort it)
    uint32_t *a = keys, *b = tmp;
    for (int pass = 0; pass < 4; ++pass) {
        radix_pass<SMALL_SORT_THREADS / 64, false>(a, b, nullptr, nullptr, 0, m, m, 8 * pass, nullptr, 0, wcnt, tot);
        __threadfence_block();
        uint32_t *t = a;
        a = b;
        b = t;
    }
}

// tiled path (m > SMALL_SORT_MAX), three launches per pass: per-tile digit counts -> exclusive scan (digit-major, tile-minor) -> scatter
__global__ void __launch_bounds__(TILE_THREADS)
pr_sort_hist_kernel(const uint64_t *__restrict__ ctr, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ tmp, int64_t n,
                    int64_t tile, int pass, uint32_t *__restrict__ hist) {
    __shared__ uint32_t cnt[256];
    int64_t m = pr_m(ctr, n);
    if (m <= SMALL_SORT_MAX) m = 0;
    const uint32_t *in = (pass & 1) ? tmp : keys;
    const int tid = threadIdx.x;
    cnt[tid] = 0u;
    __syncthreads();
    const int64_t begin = (int64_t)blockIdx.x * tile;
    int64_t end = begin + tile;
    if (end > m) end = m;
    for (int64_t i = begin + tid; i < end; i += TILE_THREADS) atomicAdd(&cnt[(in[i] >> (8 * pass)) & 255u], 1u);
    __syncthreads();
    hist[(int64_t)tid * gridDim.x + blockIdx.x] = cnt[tid];
}

__global__ void __launch_bounds__(1024) pr_sort_scan_kernel(const uint64_t *__restrict__ ctr, int64_t n, uint32_t *__restrict__ hist, int64_t len) {
    __shared__ uint32_t part[1024];
    if (pr_m(ctr, n) <= SMALL_SORT_MAX) return;                        // (the one-workgroup launch sorts it)
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

__global__ void __launch_bounds__(TILE_THREADS)
pr_sort_scatter_kernel(const uint64_t *__restrict__ ctr, uint32_t *__restrict__ keys, uint32_t *__restrict__ tmp, int64_t n, int64_t tile,
                       int pass, const uint32_t *__restrict__ hist) {
    __shared__ uint32_t wcnt[TILE_THREADS / 64][256];
    __shared__ uint32_t tot[256];
    const int64_t m = pr_m(ctr, n);
    if (m <= SMALL_SORT_MAX) return;                                   // (the one-workgroup launch sorted it)
    const int64_t begin = (int64_t)blockIdx.x * tile;
    if (begin >= m) return;                                            // (workgroup-uniform)
    int64_t end = begin + tile;
    if (end > m) end = m;
    const uint32_t *in = (pass & 1) ? tmp : keys;
    uint32_t *out = (pass & 1) ? keys : tmp;
    radix_pass<TILE_THREADS / 64, false>(in, out, nullptr, nullptr, begin, end, m, 8 * pass, hist + blockIdx.x, gridDim.x, wcnt, tot);
}

// ---- bin pass: every row into the bin of the largest sorted positive key that is <= its own ------------------------------------
// ub[row] = #{S <= key(row)} (0: below every positive), by bisection; written over `tmp`, which the sort is done with
__global__ void __launch_bounds__(256)
pr_ub_kernel(const float *__restrict__ prob, int64_t n, const uint64_t *__restrict__ ctr, const uint32_t *__restrict__ keys,
             uint32_t *__restrict__ ub) {
    const int64_t m = pr_m(ctr, n);
    if (m == 0) return;                                                // (no positive: G = 0, nothing reads ub)
    for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n; row += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t k = orderable(prob[2 * row + 1] + 0.0f);
        int64_t lo = 0, hi = m;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (keys[mid] <= k) lo = mid + 1;
            else hi = mid;
        }
        ub[row] = (uint32_t)lo;
    }
}

// arr[b] += 1 for the live lanes, wave-aggregated: the "all scores equal" input puts every row into one bin.  Up to four of the
// wave's bins are added once each with their lane counts; what is left then adds itself.
__device__ __forceinline__ void wave_bin_add(uint32_t *arr, bool live, uint32_t b) {
    const int lane = lane_id();
    uint64_t rest = __ballot(live);
    for (int it = 0; it < 4 && rest != 0ull; ++it) {
        const int leader = __ffsll((long long)rest) - 1;
        const uint32_t lb = __shfl(b, leader);
        const uint64_t same = __ballot(live && b == lb) & rest;
        if (lane == leader) atomicAdd(&arr[lb], (uint32_t)__popcll(same));
        rest &= ~same;
    }
    if ((rest >> lane) & 1ull) atomicAdd(&arr[b], 1u);
}

// Up to WIN_MAX * WIN_BINS positives: workgroup (slab s, window w) counts the rows of its slab whose bin lies in its window of
// WIN_BINS bins in LDS and adds the non-zero counts to `bins`: at most WIN_SLABS global integer atomics per bin instead of one per
// row (device-scope atomics are the expensive part of this pass: 2 M of them took 0.5 ms).  A window at or above m returns at once.
__global__ void __launch_bounds__(WIN_THREADS)
pr_bin_window_kernel(int64_t n, const uint64_t *__restrict__ ctr, const uint32_t *__restrict__ ub, int windows, uint32_t *__restrict__ bins) {
    __shared__ uint32_t h[WIN_BINS];
    const int64_t m = pr_m(ctr, n);
    if (m == 0 || m > (int64_t)WIN_MAX * WIN_BINS) return;             // (the direct launch adds them)
    const int tid = threadIdx.x;
    const int64_t w0 = (int64_t)(blockIdx.x % windows) * WIN_BINS, slab = blockIdx.x / windows;
    if (w0 >= m) return;                                               // (workgroup-uniform)
    for (int i = tid; i < WIN_BINS; i += WIN_THREADS) h[i] = 0u;
    __syncthreads();
    const int64_t per = (n + WIN_SLABS - 1) / WIN_SLABS;
    const int64_t rb = slab * per;
    int64_t re = rb + per;
    if (re > n) re = n;
    for (int64_t base = rb; base < re; base += 4 * WIN_THREADS) {      // (workgroup-uniform; four loads in flight per thread)
        uint32_t u4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {                                  // (unconditional loads, index clamped)
            const int64_t row = base + (int64_t)j * WIN_THREADS + tid;
            u4[j] = ub[row < re ? row : re - 1];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = base + (int64_t)j * WIN_THREADS + tid < re;
            const int64_t u = (int64_t)u4[j];
            const bool live = ok && u > 0 && u - 1 >= w0 && u - 1 < w0 + WIN_BINS;
            wave_bin_add(h, live, live ? (uint32_t)(u - 1 - w0) : 0u);
        }
    }
    __syncthreads();
    for (int i = tid; i < WIN_BINS; i += WIN_THREADS)
        if (h[i] != 0u && w0 + i < m) atomicAdd(&bins[w0 + i], h[i]);
}

// above WIN_MAX * WIN_BINS positives: one global integer add per row
__global__ void __launch_bounds__(256)
pr_bin_direct_kernel(int64_t n, const uint64_t *__restrict__ ctr, const uint32_t *__restrict__ ub, uint32_t *__restrict__ bins) {
    const int64_t m = pr_m(ctr, n);
    if (m <= (int64_t)WIN_MAX * WIN_BINS) return;                      // (the window launch added them)
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = base + threadIdx.x;
        const bool ok = row < n;
        const int64_t u = ok ? (int64_t)ub[row] : 0;
        const bool live = ok && u > 0 && u <= m;                       // (a value read from the workspace: clamped to the array)
        wave_bin_add(bins, live, live ? (uint32_t)(u - 1) : 0u);
    }
}

// ---- heads: group heads of the sorted keys, suffix sums of the bins, compaction to G entries -------------------------------------
__device__ __forceinline__ bool pr_head(const uint32_t *keys, int64_t i) { return i == 0 || keys[i] != keys[i - 1]; }

__global__ void __launch_bounds__(TILE_THREADS)
pr_heads_kernel(const uint64_t *__restrict__ ctr, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ bins, int64_t n,
                int64_t tile, uint32_t *__restrict__ tot_a, uint32_t *__restrict__ tot_h) {
    __shared__ uint32_t acc[2];
    const int64_t m = pr_m(ctr, n);
    const int tid = threadIdx.x;
    if (tid < 2) acc[tid] = 0u;
    __syncthreads();
    const int64_t begin = (int64_t)blockIdx.x * tile;
    int64_t end = begin + tile;
    if (end > m) end = m;
    uint32_t sa = 0, sh = 0;
    for (int64_t i = begin + tid; i < end; i += TILE_THREADS) {
        sa += bins[i];
        sh += pr_head(keys, i) ? 1u : 0u;
    }
    sa = wave_sum32(sa);
    sh = wave_sum32(sh);
    if (lane_id() == 0) {
        atomicAdd(&acc[0], sa);
        atomicAdd(&acc[1], sh);
    }
    __syncthreads();
    if (tid == 0) {
        tot_a[blockIdx.x] = acc[0];
        tot_h[blockIdx.x] = acc[1];
    }
}

// tile sums -> what lies ABOVE each tile (exclusive suffix sums); the number of heads is G
__global__ void __launch_bounds__(1024)
pr_heads_scan_kernel(uint32_t *__restrict__ tot_a, uint32_t *__restrict__ tot_h, int n_tiles, int64_t cap, uint64_t *__restrict__ hdr,
                     uint32_t *__restrict__ status) {
    __shared__ uint32_t pa[1024], ph[1024];
    const int tid = threadIdx.x;
    const int per = (n_tiles + 1023) / 1024;
    int b = tid * per, e = b + per;                                    // (reversed index r: tile n_tiles - 1 - r)
    if (b > n_tiles) b = n_tiles;
    if (e > n_tiles) e = n_tiles;
    uint32_t sa = 0, sh = 0;
    for (int r = b; r < e; ++r) {
        sa += tot_a[n_tiles - 1 - r];
        sh += tot_h[n_tiles - 1 - r];
    }
    pa[tid] = sa;
    ph[tid] = sh;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const uint32_t va = tid >= o ? pa[tid - o] : 0u, vh = tid >= o ? ph[tid - o] : 0u;
        __syncthreads();
        pa[tid] += va;
        ph[tid] += vh;
        __syncthreads();
    }
    uint32_t at_a = pa[tid] - sa, at_h = ph[tid] - sh;
    for (int r = b; r < e; ++r) {
        const int i = n_tiles - 1 - r;
        const uint32_t ca = tot_a[i], ch = tot_h[i];
        tot_a[i] = at_a;
        tot_h[i] = at_h;
        at_a += ca;
        at_h += ch;
    }
    if (tid == 1023) {
        const uint64_t G = ph[1023];
        hdr[6] = G;
        if (G > (uint64_t)cap) atomicOr(status, (uint32_t)PCG_ST_PR_OVERFLOW);
    }
}

// a thread owns a contiguous stretch of its tile and walks it from the top
__global__ void __launch_bounds__(TILE_THREADS)
pr_emit_kernel(const uint64_t *__restrict__ ctr, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ bins, int64_t n,
               int64_t tile, const uint32_t *__restrict__ tot_a, const uint32_t *__restrict__ tot_h, int64_t cap,
               uint32_t *__restrict__ tp_g, uint32_t *__restrict__ npred_g) {
    __shared__ uint32_t pa[TILE_THREADS], ph[TILE_THREADS];
    const int64_t m = pr_m(ctr, n);
    const int tid = threadIdx.x;
    const int64_t begin = (int64_t)blockIdx.x * tile;
    if (begin >= m) return;                                            // (workgroup-uniform)
    int64_t end = begin + tile;
    if (end > m) end = m;
    const int64_t per = tile / TILE_THREADS;
    int64_t b = begin + (int64_t)tid * per, e = b + per;
    if (b > end) b = end;
    if (e > end) e = end;
    uint32_t sa = 0, sh = 0;
    for (int64_t i = b; i < e; ++i) {
        sa += bins[i];
        sh += pr_head(keys, i) ? 1u : 0u;
    }
    const int rt = TILE_THREADS - 1 - tid;                             // (reversed: an inclusive scan from the last thread down)
    pa[rt] = sa;
    ph[rt] = sh;
    __syncthreads();
    for (int o = 1; o < TILE_THREADS; o <<= 1) {
        const uint32_t va = rt >= o ? pa[rt - o] : 0u, vh = rt >= o ? ph[rt - o] : 0u;
        __syncthreads();
        pa[rt] += va;
        ph[rt] += vh;
        __syncthreads();
    }
    uint32_t run_a = tot_a[blockIdx.x] + pa[rt] - sa;                  // bins above this stretch
    uint32_t run_h = tot_h[blockIdx.x] + ph[rt] - sh;                  // heads above this stretch
    for (int64_t i = e - 1; i >= b; --i) {
        run_a += bins[i];
        if (pr_head(keys, i)) {
            if ((int64_t)run_h < cap) {                                // (nothing is written past cap)
                tp_g[run_h] = (uint32_t)(m - i);
                npred_g[run_h] = run_a;
            }
            ++run_h;
        }
    }
}

// ============================================================ pcg_topk_alerts ======================================================
__global__ void __launch_bounds__(256) al_zero_kernel(uint32_t *__restrict__ ctr, int n_words) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += gridDim.x * blockDim.x) ctr[i] = 0u;
}

// The digits of the ke-th largest key that the first `passes` histograms decide, by the whole workgroup (>= 256 threads):
// prefix = those digits in place, r = how many of the rows that match the prefix are still to be taken (>= 1).
// hist[p][d] = rows whose higher digits match and whose digit p is d.  s: 256 words, sel: 2 words of LDS.
__device__ __forceinline__ void al_pick(const uint32_t *__restrict__ hist, int passes, uint32_t ke, uint32_t *s, uint32_t *sel,
                                        uint32_t &prefix, uint32_t &r) {
    const int tid = threadIdx.x;
    prefix = 0u;
    r = ke;
    for (int p = 0; p < passes; ++p) {
        if (tid < 256) s[tid] = hist[256 * p + tid];
        if (tid == 0) sel[0] = 0u, sel[1] = 0u;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {                            // s[d] = rows with digit >= d
            const uint32_t v = (tid < 256 && tid + o < 256) ? s[tid + o] : 0u;
            __syncthreads();
            if (tid < 256) s[tid] += v;
            __syncthreads();
        }
        if (tid < 256) {
            const uint32_t above = tid < 255 ? s[tid + 1] : 0u;
            if (s[tid] >= r && above < r) sel[0] = (uint32_t)tid, sel[1] = r - above;     // (exactly one digit: s falls with d)
        }
        __syncthreads();
        prefix |= sel[0] << (24 - 8 * p);
        r = sel[1];
        __syncthreads();
    }
}

__device__ __forceinline__ uint32_t al_key(const float *__restrict__ p1, int64_t stride, int64_t row) {
    return orderable(p1[row * stride] + 0.0f);
}

__global__ void __launch_bounds__(256)
al_hist_kernel(const float *__restrict__ p1, int64_t stride, int64_t n, uint32_t ke, int pass, uint32_t *__restrict__ hist,
               uint32_t *__restrict__ status) {
    __shared__ uint32_t cnt[256], s[256], sel[2];
    const int tid = threadIdx.x, lane = lane_id();
    uint32_t prefix, r;
    al_pick(hist, pass, ke, s, sel, prefix, r);
    cnt[tid] = 0u;
    __syncthreads();
    const int hi_shift = 32 - 8 * pass, lo_shift = 24 - 8 * pass;      // (hi_shift 32 at pass 0: shifted as 64-bit)
    bool bad = false;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = base + tid;
        const bool ok = row < n;
        const float v = p1[(ok ? row : n - 1) * stride];
        bad |= ok && v != v;
        const uint32_t key = orderable(v + 0.0f);
        const bool match = ok && (uint32_t)((uint64_t)key >> hi_shift) == (uint32_t)((uint64_t)prefix >> hi_shift);
        const uint32_t d = (key >> lo_shift) & 255u;
        const uint64_t mm = __ballot(match);
        if (mm != 0ull) {                                              // one add for a wave whose rows share the digit
            const int leader = __ffsll((long long)mm) - 1;
            const uint32_t ld = __shfl(d, leader);
            const uint64_t same = __ballot(match && d == ld);
            if (same == mm) {
                if (lane == leader) atomicAdd(&cnt[ld], (uint32_t)__popcll(mm));
            } else if (match) {
                atomicAdd(&cnt[d], 1u);
            }
        }
    }
    if (pass == 0 && __ballot(bad) != 0ull && lane == 0) atomicOr(status, (uint32_t)PCG_ST_EVAL_INPUT);
    __syncthreads();
    if (cnt[tid]) atomicAdd(&hist[256 * pass + tid], cnt[tid]);
}

// per tile of rows: how many lie above the ke-th key, how many equal it
__global__ void __launch_bounds__(256)
al_count_kernel(const float *__restrict__ p1, int64_t stride, int64_t n, uint32_t ke, int64_t tile, const uint32_t *__restrict__ hist,
                uint32_t *__restrict__ ctr, uint32_t *__restrict__ tcnt_a, uint32_t *__restrict__ tcnt_e) {
    __shared__ uint32_t s[256], sel[2], acc[2];
    const int tid = threadIdx.x;
    uint32_t T, need;
    al_pick(hist, 4, ke, s, sel, T, need);
    if (blockIdx.x == 0 && tid == 0) ctr[0] = T, ctr[1] = need;
    if (tid < 2) acc[tid] = 0u;
    __syncthreads();
    const int64_t begin = (int64_t)blockIdx.x * tile;
    int64_t end = begin + tile;
    if (end > n) end = n;
    uint32_t a = 0, e = 0;
    for (int64_t row = begin + tid; row < end; row += 256) {
        const uint32_t key = al_key(p1, stride, row);
        a += key > T;
        e += key == T;
    }
    a = wave_sum32(a);
    e = wave_sum32(e);
    if (lane_id() == 0) {
        atomicAdd(&acc[0], a);
        atomicAdd(&acc[1], e);
    }
    __syncthreads();
    if (tid == 0) {
        tcnt_a[blockIdx.x] = acc[0];
        tcnt_e[blockIdx.x] = acc[1];
    }
}

// exclusive scan of v[0 .. len) by 1024 threads, thread t over its `per` consecutive entries; in place
__device__ __forceinline__ void al_scan(uint32_t *v, int len, uint32_t *part) {
    const int tid = threadIdx.x;
    const int per = (len + 1023) / 1024;
    int b = tid * per, e = b + per;
    if (b > len) b = len;
    if (e > len) e = len;
    uint32_t s = 0;
    for (int i = b; i < e; ++i) s += v[i];
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const uint32_t x = tid >= o ? part[tid - o] : 0u;
        __syncthreads();
        part[tid] += x;
        __syncthreads();
    }
    uint32_t at = part[tid] - s;
    for (int i = b; i < e; ++i) {
        const uint32_t c = v[i];
        v[i] = at;
        at += c;
    }
    __syncthreads();
}

// tcnt_e -> equal rows before each tile; tcnt_a -> where each tile's taken rows start in the candidate list
__global__ void __launch_bounds__(1024)
al_scan_kernel(const uint32_t *__restrict__ ctr, uint32_t *__restrict__ tcnt_a, uint32_t *__restrict__ tcnt_e, int n_tiles) {
    __shared__ uint32_t part[1024];
    __shared__ uint32_t eq[MAX_TILES];
    const int tid = threadIdx.x;
    const uint32_t need = ctr[1];
    for (int i = tid; i < n_tiles; i += 1024) eq[i] = tcnt_e[i];
    __syncthreads();
    al_scan(tcnt_e, n_tiles, part);
    for (int i = tid; i < n_tiles; i += 1024) {
        const uint32_t before = tcnt_e[i], left = need > before ? need - before : 0u;
        tcnt_a[i] += eq[i] < left ? eq[i] : left;
    }
    __syncthreads();
    al_scan(tcnt_a, n_tiles, part);
}

__global__ void __launch_bounds__(256)
al_scatter_kernel(const float *__restrict__ p1, int64_t stride, int64_t n, uint32_t ke, int64_t tile, const uint32_t *__restrict__ ctr,
                  const uint32_t *__restrict__ tcnt_a, const uint32_t *__restrict__ tcnt_e, uint32_t *__restrict__ cand_k,
                  uint32_t *__restrict__ cand_v) {
    __shared__ uint32_t we[4], wo[4];
    const int tid = threadIdx.x, w = tid >> 6;
    const uint32_t T = ctr[0], need = ctr[1];
    uint32_t run_e = tcnt_e[blockIdx.x], run_o = tcnt_a[blockIdx.x];
    const int64_t begin = (int64_t)blockIdx.x * tile;
    int64_t end = begin + tile;
    if (end > n) end = n;
    for (int64_t base = begin; base < end; base += 256) {              // (workgroup-uniform)
        const int64_t row = base + tid;
        const bool ok = row < end;
        const uint32_t key = al_key(p1, stride, ok ? row : end - 1);
        const bool ab = ok && key > T, eq = ok && key == T;
        const uint64_t me = __ballot(eq);
        if (lane_id() == 0) we[w] = (uint32_t)__popcll(me);
        __syncthreads();
        uint32_t e_before = run_e + (uint32_t)__popcll(me & lanemask_lt()), e_all = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            e_before += j < w ? we[j] : 0u;
            e_all += we[j];
        }
        const bool take = ab || (eq && e_before < need);               // the first `need` equal rows by position
        const uint64_t mt = __ballot(take);
        if (lane_id() == 0) wo[w] = (uint32_t)__popcll(mt);
        __syncthreads();
        uint32_t slot = run_o + (uint32_t)__popcll(mt & lanemask_lt()), o_all = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            slot += j < w ? wo[j] : 0u;
            o_all += wo[j];
        }
        if (take && slot < ke) {                                       // (a counter's value: clamped to the array)
            cand_k[slot] = ~key;
            cand_v[slot] = (uint32_t)row;
        }
        run_e += e_all;
        run_o += o_all;
        __syncthreads();
    }
}

// stable sort of the ke candidates by ~key ascending (= key descending, equal keys in position order) and the output
__global__ void __launch_bounds__(SMALL_SORT_THREADS)
al_sort_kernel(const float *__restrict__ p1, int64_t stride, int64_t n, int64_t ke, int64_t k, uint32_t *cand_k, uint32_t *cand_v,
               uint32_t *tmp_k, uint32_t *tmp_v, int32_t *__restrict__ out_pos, float *__restrict__ out_score) {
    __shared__ uint32_t wcnt[SMALL_SORT_THREADS / 64][256];
    __shared__ uint32_t tot[256];
    uint32_t *ak = cand_k, *av = cand_v, *bk = tmp_k, *bv = tmp_v;
    for (int pass = 0; pass < 4; ++pass) {
        radix_pass<SMALL_SORT_THREADS / 64, true>(ak, bk, av, bv, 0, ke, ke, 8 * pass, nullptr, 0, wcnt, tot);
        __threadfence_block();
        uint32_t *t = ak;
        ak = bk, bk = t;
        t = av;
        av = bv, bv = t;
    }
    for (int64_t j = threadIdx.x; j < k; j += SMALL_SORT_THREADS) {
        const int64_t pos = j < ke ? (int64_t)av[j] : -1;
        const bool ok = pos >= 0 && pos < n;                           // (a position read from the workspace: checked)
        out_pos[j] = ok ? (int32_t)pos : -1;
        out_score[j] = ok ? p1[pos * stride] : -__builtin_inff();
    }
}

__global__ void __launch_bounds__(256) al_pad_kernel(int64_t k, int32_t *__restrict__ out_pos, float *__restrict__ out_score) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < k; j += (int64_t)gridDim.x * blockDim.x) {
        out_pos[j] = -1;
        out_score[j] = -__builtin_inff();
    }
}

}  // namespace rankeval
}  // namespace pcg

extern "C" {

int64_t pcg_pr_workspace_bytes(int64_t n) {
    if (n < 0 || n > 0x7fffffffll) return PCG_E_ARG;
    pcg::rankeval::PrCarve c;
    pcg::rankeval::pr_carve(n, c);
    return c.total;
}

int pcg_pr_counts(const float *prob, const int32_t *labels, int64_t n, int64_t cap, void *workspace, uint64_t *hdr, uint32_t *tp_g,
                  uint32_t *npred_g, uint32_t *status, void *stream) {
    namespace re = pcg::rankeval;
    if (n < 0 || n > 0x7fffffffll || cap < 0) return PCG_E_ARG;
    if (!workspace || !hdr || !status || (n > 0 && (!prob || !labels)) || (cap > 0 && (!tp_g || !npred_g))) return PCG_E_ARG;
    if ((reinterpret_cast<uintptr_t>(prob) & 7u) != 0 || (reinterpret_cast<uintptr_t>(workspace) & 7u) != 0 ||
        (reinterpret_cast<uintptr_t>(hdr) & 7u) != 0)
        return PCG_E_ARG;
    re::PrCarve c;
    re::pr_carve(n, c);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    uint64_t *ctr = reinterpret_cast<uint64_t *>(ws + c.ctr);
    uint32_t *keys = reinterpret_cast<uint32_t *>(ws + c.keys), *tmp = reinterpret_cast<uint32_t *>(ws + c.tmp);
    uint32_t *bins = reinterpret_cast<uint32_t *>(ws + c.bins), *hist = reinterpret_cast<uint32_t *>(ws + c.hist);
    uint32_t *tot_a = reinterpret_cast<uint32_t *>(ws + c.tot), *tot_h = tot_a + (c.n_tiles + 1);
    hipStream_t st = static_cast<hipStream_t>(stream);

    hipLaunchKernelGGL(re::pr_zero_kernel, dim3(1), dim3(64), 0, st, ctr, hdr);
    PCG_LAUNCH_CHECK();
    if (n == 0) return PCG_OK;

    const int64_t per_iter = (int64_t)re::COUNT_THREADS * re::COUNT_ROWS;
    int64_t blocks = (n + per_iter - 1) / per_iter;
    if (blocks > re::GRID_CAP) blocks = re::GRID_CAP;
    hipLaunchKernelGGL(re::pr_count_kernel, dim3((unsigned)blocks), dim3(re::COUNT_THREADS), 0, st, prob, labels, n, ctr, keys, bins, status);
    PCG_LAUNCH_CHECK();
    hipLaunchKernelGGL(re::pr_finish_kernel, dim3(1), dim3(64), 0, st, ctr, n, hdr);
    PCG_LAUNCH_CHECK();

    const unsigned tiles = (unsigned)c.n_tiles;
    hipLaunchKernelGGL(re::pr_sort_small_kernel, dim3(1), dim3(re::SMALL_SORT_THREADS), 0, st, ctr, keys, tmp, n);
    PCG_LAUNCH_CHECK();
    if (n > re::SMALL_SORT_MAX) {                                      // (more positives than one workgroup sorts are possible)
        for (int pass = 0; pass < 4; ++pass) {
            hipLaunchKernelGGL(re::pr_sort_hist_kernel, dim3(tiles), dim3(re::TILE_THREADS), 0, st, ctr, keys, tmp, n, c.tile, pass, hist);
            PCG_LAUNCH_CHECK();
            hipLaunchKernelGGL(re::pr_sort_scan_kernel, dim3(1), dim3(1024), 0, st, ctr, n, hist, 256 * c.n_tiles);
            PCG_LAUNCH_CHECK();
            hipLaunchKernelGGL(re::pr_sort_scatter_kernel, dim3(tiles), dim3(re::TILE_THREADS), 0, st, ctr, keys, tmp, n, c.tile, pass, hist);
            PCG_LAUNCH_CHECK();
        }
    }
    int64_t bblocks = (n + 255) / 256;
    if (bblocks > re::GRID_CAP) bblocks = re::GRID_CAP;
    hipLaunchKernelGGL(re::pr_ub_kernel, dim3((unsigned)bblocks), dim3(256), 0, st, prob, n, ctr, keys, tmp);
    PCG_LAUNCH_CHECK();
    int64_t windows = (n + re::WIN_BINS - 1) / re::WIN_BINS;
    if (windows > re::WIN_MAX) windows = re::WIN_MAX;
    hipLaunchKernelGGL(re::pr_bin_window_kernel, dim3((unsigned)(windows * re::WIN_SLABS)), dim3(re::WIN_THREADS), 0, st, n, ctr, tmp,
                       (int)windows, bins);
    PCG_LAUNCH_CHECK();
    if (n > (int64_t)re::WIN_MAX * re::WIN_BINS) {                     // (more positives than the windows cover are possible)
        hipLaunchKernelGGL(re::pr_bin_direct_kernel, dim3((unsigned)bblocks), dim3(256), 0, st, n, ctr, tmp, bins);
        PCG_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(re::pr_heads_kernel, dim3(tiles), dim3(re::TILE_THREADS), 0, st, ctr, keys, bins, n, c.tile, tot_a, tot_h);
    PCG_LAUNCH_CHECK();
    hipLaunchKernelGGL(re::pr_heads_scan_kernel, dim3(1), dim3(1024), 0, st, tot_a, tot_h, (int)c.n_tiles, cap, hdr, status);
    PCG_LAUNCH_CHECK();
    hipLaunchKernelGGL(re::pr_emit_kernel, dim3(tiles), dim3(re::TILE_THREADS), 0, st, ctr, keys, bins, n, c.tile, tot_a, tot_h, cap, tp_g,
                       npred_g);
    PCG_LAUNCH_CHECK();
    return PCG_OK;
}

int64_t pcg_topk_alerts_workspace_bytes(int64_t n, int32_t k) {
    if (n < 0 || n > 0x7fffffffll || k < 1 || k > PCG_ALERTS_MAX_K) return PCG_E_ARG;
    pcg::rankeval::AlCarve c;
    pcg::rankeval::al_carve(n, k, c);
    return c.total;
}

int pcg_topk_alerts(const float *p1, int32_t stride, int64_t n, int32_t k, void *workspace, int32_t *out_pos, float *out_score,
                    uint32_t *status, void *stream) {
    namespace re = pcg::rankeval;
    if (n < 0 || n > 0x7fffffffll || k < 1 || k > PCG_ALERTS_MAX_K || stride < 1) return PCG_E_ARG;
    if (!workspace || !out_pos || !out_score || !status || (n > 0 && !p1)) return PCG_E_ARG;
    if ((reinterpret_cast<uintptr_t>(workspace) & 3u) != 0 || (reinterpret_cast<uintptr_t>(p1) & 3u) != 0) return PCG_E_ARG;
    re::AlCarve c;
    re::al_carve(n, k, c);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    uint32_t *ctr = reinterpret_cast<uint32_t *>(ws + c.ctr), *hist = reinterpret_cast<uint32_t *>(ws + c.hist);
    uint32_t *tcnt_a = reinterpret_cast<uint32_t *>(ws + c.tcnt), *tcnt_e = tcnt_a + (c.n_tiles + 1);
    const int64_t kb = re::up256(4 * (int64_t)k);
    uint32_t *cand_k = reinterpret_cast<uint32_t *>(ws + c.cand), *cand_v = reinterpret_cast<uint32_t *>(ws + c.cand + kb);
    uint32_t *tmp_k = reinterpret_cast<uint32_t *>(ws + c.cand + 2 * kb), *tmp_v = reinterpret_cast<uint32_t *>(ws + c.cand + 3 * kb);
    hipStream_t st = static_cast<hipStream_t>(stream);

    if (n == 0) {                                                      // all padding
        hipLaunchKernelGGL(re::al_pad_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, (int64_t)k, out_pos, out_score);
        PCG_LAUNCH_CHECK();
        return PCG_OK;
    }
    const uint32_t ke = (uint32_t)(n < k ? n : k);
    const int zero_words = (int)((c.tcnt - c.ctr) / 4);                // the counters and the four histograms
    hipLaunchKernelGGL(re::al_zero_kernel, dim3((zero_words + 255) / 256), dim3(256), 0, st, ctr, zero_words);
    PCG_LAUNCH_CHECK();
    int64_t blocks = (n + 255) / 256;
    if (blocks > re::GRID_CAP) blocks = re::GRID_CAP;
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(re::al_hist_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p1, (int64_t)stride, n, ke, pass, hist, status);
        PCG_LAUNCH_CHECK();
    }
    const unsigned tiles = (unsigned)c.n_tiles;
    hipLaunchKernelGGL(re::al_count_kernel, dim3(tiles), dim3(256), 0, st, p1, (int64_t)stride, n, ke, c.tile, hist, ctr, tcnt_a, tcnt_e);
    PCG_LAUNCH_CHECK();
    hipLaunchKernelGGL(re::al_scan_kernel, dim3(1), dim3(1024), 0, st, ctr, tcnt_a, tcnt_e, (int)c.n_tiles);
    PCG_LAUNCH_CHECK();
    hipLaunchKernelGGL(re::al_scatter_kernel, dim3(tiles), dim3(256), 0, st, p1, (int64_t)stride, n, ke, c.tile, ctr, tcnt_a, tcnt_e, cand_k,
                       cand_v);
    PCG_LAUNCH_CHECK();
    hipLaunchKernelGGL(re::al_sort_kernel, dim3(1), dim3(re::SMALL_SORT_THREADS), 0, st, p1, (int64_t)stride, n, (int64_t)ke, (int64_t)k,
                       cand_k, cand_v, tmp_k, tmp_v, out_pos, out_score);
    PCG_LAUNCH_CHECK();
    return PCG_OK;
}

}  // extern "C"
