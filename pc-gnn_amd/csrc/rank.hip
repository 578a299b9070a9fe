// The chosen neighbours of test-mode rows in the reference's order, with their distances (gfx950).
//
// After the plan and select launches have written a batch's selection lists (ascending position in the ascending-id row, no
// holes in test mode), rank_lists copies every row (r, b) to the caller's arrays at out_begin[r * n_total + b_off + b]:
//   keep-all rows (deg <= k + 1, layers.py:729-733): list order, dist[j] = |c - s0[list[j]]|;
//   ranked rows   (deg > k + 1,  layers.py:726-728): ascending distance, ties by list position - the order torch.sort(stable)
//                 gives the reference's score_diff.  Key = (orderable(|c - s0[id]|) << 32) | j: unique, so an entry's slot is
//                 the number of smaller keys - ranking by counting, exact and stable, no sort network.
// The distance is one f32 subtract and abs (dist_key's arithmetic: a tie here is a tie in select_rows, bit for bit
// torch.abs(c - s)); orderable() on a non-negative float is dist_key's bit pattern with bit 31 set - the same order.
//
// Tiers by kept count n (the plan's degree-tier queues and counters are READ to enumerate the rows; nothing of the plan is written):
//   rank_short_rows  n <= 64: one wave per row, one key per lane, ranked lane against lane (readlane, as wave_kth); the rows of
//                    the plan's <= 16-neighbour queue four per wave, one per 16-lane row (DPP rotates, as select_four_short_rows)
//   rank_wg_rows     n > 64: work item = (row, slice of RANK_SLICE keys); a workgroup keeps its slice's keys in registers
//                    (RANK_KPT per thread), re-forms ALL of the row's keys tile by tile in LDS (a key is a function of the list
//                    and s0 only: any workgroup can recompute it) and counts the smaller ones.  n <= RANK_SLICE: one workgroup,
//                    its own keys are the only tile.  Longer rows: slices blockIdx.y, + gridDim.y, ... - a 30 000-neighbour row
//                    keeps 15 000 entries = 8 workgroups.
// No workgroup waits for another: no polling, no tickets, no float atomics (the only atomic is the OR into the status word).
// Every index that comes from device data is checked or clamped: a row whose device count differs from the extent the caller
// gave it (out_begin[i + 1] - out_begin[i]), whose list region leaves the list or whose extent leaves [0, out_begin[R * n_total])
// sets PCG_ST_RANK_MISMATCH and writes nothing; list ids are clamped to the score table for the read (PCG_ST_LIST_ID_RANGE);
// a slot is clamped to the row's extent.
// Reference lines replaced: src/layers.py:713-736 (choose_step_test's samp_scores), :630 (IntraAgg.forward's second value).
// The second half of the file ranks the minority picks of train-mode rows (pcg_rank_minority; :675-691).
#include "infer.h"

namespace pcg {

constexpr int RANK_THREADS = 256;
constexpr int RANK_KPT = 8;                               // keys of its slice a thread keeps in registers
constexpr int RANK_SLICE = RANK_THREADS * RANK_KPT;       // the one-workgroup limit: 2048 keys (16 KB of LDS)
constexpr int RANK_SHORT_BLOCKS = 2048;
constexpr int RANK_WG_BLOCKS = 1024;

struct RankArgs {
    Workspace w;                // the plan (recs, queues, counters: read only) and the lists (len, list) of the batch
    const int32_t *nodes;       // [B] the batch's centres
    int32_t B, n_rel;
    int64_t n_nodes, n_total, b_off;   // row (r, b) of the batch is row (r, b_off + b) of the caller's n_total ids; n_nodes: the
                                       // entries of s0 (the table's rows; a query batch: base + query rows)
    int64_t center_off;         // centre b's score is s0[nodes[b] + center_off] (a query batch's rows lie behind the base table's)
    const float *s0, *center_s0;
    const int64_t *out_begin;   // [n_rel * n_total + 1]
    int32_t *out_ids;
    float *out_dist;
    uint32_t *status;
};

struct RankRow {
    int n;                      // kept entries; -1: nothing to do (mismatch reported, or an empty row)
    int lbeg;
    bool keep_all;
    float c;
    int64_t obeg;
};

// what every path needs of a row, checked (wave- / workgroup-uniform: every lane reads the same words)
__device__ __forceinline__ RankRow rank_row(const RankArgs &a, int row) {
    RankRow q;
    const RowRec p = a.w.recs[row];
    const int r = row / a.B, b = row - r * a.B;
    const int64_t i = (int64_t)r * a.n_total + a.b_off + b;
    const int64_t obeg = a.out_begin[i], oend = a.out_begin[i + 1], ocap = a.out_begin[(int64_t)a.n_rel * a.n_total];
    const int n = a.w.len[row];
    q.keep_all = rec_keep_all(p);
    q.lbeg = p.lbeg;
    q.obeg = obeg;
    const bool ok = n >= 0 && (int64_t)n == oend - obeg && obeg >= 0 && oend <= ocap && p.lbeg >= 0 &&
                    (int64_t)p.lbeg + n <= a.w.list_capacity;
    q.n = ok ? (n > 0 ? n : -1) : -1;
    if (!ok && a.status && (threadIdx.x & (PCG_WAVE - 1)) == 0) atomicOr(a.status, (uint32_t)PCG_ST_RANK_MISMATCH);
    int64_t node = a.nodes[b] + a.center_off;
    node = node < 0 ? 0 : (node >= a.n_nodes ? a.n_nodes - 1 : node);
    q.c = a.center_s0 ? a.center_s0[b] : a.s0[node];
    return q;
}

// s0 of a list entry; an id outside the table (a hole, a foreign list) is clamped for the read and reported
__device__ __forceinline__ float rank_score(const RankArgs &a, int32_t id, bool valid) {
    const bool bad = valid && (id < 0 || (int64_t)id >= a.n_nodes);
    if (bad && a.status) atomicOr(a.status, (uint32_t)PCG_ST_LIST_ID_RANGE);
    const int64_t at = id < 0 ? 0 : ((int64_t)id >= a.n_nodes ? a.n_nodes - 1 : (int64_t)id);
    return a.s0[at];
}

// rotate a (key, position) pair by N lanes inside every 16-lane row
#define PCG_RANK_ROR(N)                                                                                      \
    do {                                                                                                     \
        const uint32_t ok = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)key, 0x120 + (N), 0xF, 0xF, false); \
        const int op = __builtin_amdgcn_update_dpp(0, pos, 0x120 + (N), 0xF, 0xF, false);                   \
        rank += (ok < key) || (ok == key && op < pos);                                                       \
    } while (0)

// four rows of the plan's <= 16-neighbour queue, one per 16-lane row of the wave
__device__ __forceinline__ void rank_four_short_rows(const RankArgs &a, int q_first, int na, int lane) {
    const int g = lane >> 4, pos = lane & 15;
    const int qi = q_first + g;
    const bool active = qi < na;
    int row = a.w.qa[active ? qi : na - 1];
    const int rows = a.n_rel * a.B;
    row = row < 0 ? 0 : (row >= rows ? rows - 1 : row);
    const RowRec p = a.w.recs[row];
    const int r = row / a.B, b = row - r * a.B;
    const int64_t i = (int64_t)r * a.n_total + a.b_off + b;
    const int64_t obeg = a.out_begin[i], oend = a.out_begin[i + 1], ocap = a.out_begin[(int64_t)a.n_rel * a.n_total];
    const int n = a.w.len[row];
    const bool ok = n >= 0 && n <= TA_CAP && (int64_t)n == oend - obeg && obeg >= 0 && oend <= ocap && p.lbeg >= 0 &&
                    (int64_t)p.lbeg + n <= a.w.list_capacity;
    if (active && !ok && pos == 0 && a.status) atomicOr(a.status, (uint32_t)PCG_ST_RANK_MISMATCH);
    const bool have = active && ok && pos < n;
    const int32_t id = a.w.list[have ? p.lbeg + pos : 0];                  // unconditional load (clamped)
    int64_t node = a.nodes[b] + a.center_off;
    node = node < 0 ? 0 : (node >= a.n_nodes ? a.n_nodes - 1 : node);
    const float c = a.center_s0 ? a.center_s0[b] : a.s0[node];
    const float dist = fabsf(c - rank_score(a, id, have));
    const uint32_t key = have ? orderable(dist) : 0xFFFFFFFFu;             // (a real distance is never a negative NaN)
    int rank = 0;
    PCG_RANK_ROR(1); PCG_RANK_ROR(2); PCG_RANK_ROR(3); PCG_RANK_ROR(4); PCG_RANK_ROR(5);
    PCG_RANK_ROR(6); PCG_RANK_ROR(7); PCG_RANK_ROR(8); PCG_RANK_ROR(9); PCG_RANK_ROR(10);
    PCG_RANK_ROR(11); PCG_RANK_ROR(12); PCG_RANK_ROR(13); PCG_RANK_ROR(14); PCG_RANK_ROR(15);
    if (have) {
        int slot = rec_keep_all(p) ? pos : rank;
        slot = slot < n ? slot : n - 1;
        a.out_ids[obeg + slot] = id;
        a.out_dist[obeg + slot] = dist;
    }
}

// one row of <= 64 kept entries on one wave: one key per lane, ranked lane against lane in the (key, position) order
__device__ __forceinline__ void rank_lane_row(const RankArgs &a, int row, int lane) {
    const RankRow q = rank_row(a, row);
    if (q.n < 0 || q.n > PCG_WAVE) return;                                 // (longer rows: rank_wg_rows)
    const int n = q.n;
    const bool have = lane < n;
    const int32_t id = a.w.list[q.lbeg + (have ? lane : n - 1)];
    const float dist = fabsf(q.c - rank_score(a, id, have));
    const uint32_t mine = have ? orderable(dist) : 0xFFFFFFFFu;
    int slot = lane;
    if (!q.keep_all) {
        slot = 0;
        for (int j = 0; j < n; ++j) {                                      // n is wave-uniform
            const uint32_t o = (uint32_t)__builtin_amdgcn_readlane((int)mine, j);
            slot += (o < mine) || (o == mine && j < lane);
        }
    }
    if (have) {
        slot = slot < n ? slot : n - 1;
        a.out_ids[q.obeg + slot] = id;
        a.out_dist[q.obeg + slot] = dist;
    }
}

// rows of at most 64 kept entries.  Items: the groups of four of the <= 16-neighbour queue, then every other queued row (the
// <= 64-neighbour queue always, a longer row when it kept no more than 64); one item per wave, wave-strided
__global__ void __launch_bounds__(RANK_THREADS) rank_short_rows(const RankArgs a) {
    const int lane = lane_id();
    const int n_waves = (int)gridDim.x * (RANK_THREADS / PCG_WAVE);
    const int wave = (int)blockIdx.x * (RANK_THREADS / PCG_WAVE) + ((int)threadIdx.x >> 6);
    const int rows = a.n_rel * a.B;
    auto cnt = [&](int which) {
        const int v = (int)a.w.counters[which];
        return v < 0 ? 0 : (v > rows ? rows : v);
    };
    const int na = cnt(C_NA), n0 = cnt(C_N0), n1 = cnt(C_N1), n4 = cnt(C_N4), n16 = cnt(C_N16);
    const int ga = (na + 3) / 4;
    const int n_items = ga + n0 + n1 + n4 + n16;
    for (int u = wave; u < n_items; u += n_waves) {
        if (u < ga) {
            rank_four_short_rows(a, 4 * u, na, lane);
            continue;
        }
        int j = u - ga;
        const int32_t *qq = a.w.q0;
        if (j >= n0) { j -= n0; qq = a.w.q1;
            if (j >= n1) { j -= n1; qq = a.w.q4;
                if (j >= n4) { j -= n4; qq = a.w.q16; } } }
        int row = __builtin_amdgcn_readfirstlane(qq[j]);
        if (row < 0 || row >= rows) continue;
        rank_lane_row(a, row, lane);
    }
}

// #keys of the tile below each of the thread's NU keys
template <int NU>
__device__ __forceinline__ void rank_count_tile(const uint64_t *__restrict__ tile, int tn, const uint64_t (&key)[RANK_KPT],
                                                int (&below)[RANK_KPT]) {
    int t = 0;
    for (; t + 4 <= tn; t += 4) {
        const uint64_t k0 = tile[t], k1 = tile[t + 1], k2 = tile[t + 2], k3 = tile[t + 3];   // (one address per wave: a broadcast)
#pragma unroll
        for (int u = 0; u < NU; ++u) below[u] += (int)(k0 < key[u]) + (int)(k1 < key[u]) + (int)(k2 < key[u]) + (int)(k3 < key[u]);
    }
    for (; t < tn; ++t) {
        const uint64_t k0 = tile[t];
#pragma unroll
        for (int u = 0; u < NU; ++u) below[u] += (int)(k0 < key[u]);
    }
}

// rows of more than 64 kept entries: blockIdx.x strides over the queued rows of more than 64 neighbours, blockIdx.y over a row's
// slices of RANK_SLICE keys
__global__ void __launch_bounds__(RANK_THREADS) rank_wg_rows(const RankArgs a) {
    __shared__ uint64_t tile[RANK_SLICE];
    const int tid = (int)threadIdx.x;
    const int rows = a.n_rel * a.B;
    auto cnt = [&](int which) {
        const int v = (int)a.w.counters[which];
        return v < 0 ? 0 : (v > rows ? rows : v);
    };
    const int n16 = cnt(C_N16), n4 = cnt(C_N4), n1 = cnt(C_N1);
    // a row of <= 512 neighbours has one slice, of <= 4096 two: the workgroups of later slices look at the longer rows only
    const int n_cand = blockIdx.y == 0 ? n16 + n4 + n1 : (blockIdx.y * RANK_SLICE < T4_CAP ? n16 + n4 : n16);
    for (int u = (int)blockIdx.x; u < n_cand; u += (int)gridDim.x) {
        const int row = u < n16 ? a.w.q16[u] : (u < n16 + n4 ? a.w.q4[u - n16] : a.w.q1[u - n16 - n4]);
        if (row < 0 || row >= rows) continue;
        const RankRow q = rank_row(a, row);
        const int n = q.n;
        if (n <= PCG_WAVE) continue;                                       // (rank_short_rows; -1: nothing to do)
        const int32_t *__restrict__ list = a.w.list + q.lbeg;
        for (int64_t base64 = (int64_t)blockIdx.y * RANK_SLICE; base64 < n; base64 += (int64_t)gridDim.y * RANK_SLICE) {
            const int base = (int)base64;
            // the slice's own entries: j = base + u * 256 + tid
            int32_t id[RANK_KPT];
            float dist[RANK_KPT];
            uint64_t key[RANK_KPT];
            int below[RANK_KPT];
#pragma unroll
            for (int x = 0; x < RANK_KPT; ++x) {
                const int j = base + x * RANK_THREADS + tid;
                id[x] = list[j < n ? j : n - 1];                           // unconditional loads (clamped): all in flight together
            }
#pragma unroll
            for (int x = 0; x < RANK_KPT; ++x) {
                const int j = base + x * RANK_THREADS + tid;
                dist[x] = fabsf(q.c - rank_score(a, id[x], j < n));
                key[x] = j < n ? ((uint64_t)orderable(dist[x]) << 32) | (uint32_t)j : ~0ull;
                below[x] = 0;
            }
            if (q.keep_all) {
#pragma unroll
                for (int x = 0; x < RANK_KPT; ++x) {
                    const int j = base + x * RANK_THREADS + tid;
                    if (j < n) {
                        a.out_ids[q.obeg + j] = id[x];
                        a.out_dist[q.obeg + j] = dist[x];
                    }
                }
                continue;
            }
            const int mine = n - base < RANK_SLICE ? n - base : RANK_SLICE;          // entries of this slice
            const int nu = (mine + RANK_THREADS - 1) / RANK_THREADS;                 // key[x], x >= nu: no thread has one
            for (int t0 = 0; t0 < n; t0 += RANK_SLICE) {
                __syncthreads();                                                     // (the tile before: its reads)
                if (t0 == base) {
#pragma unroll
                    for (int x = 0; x < RANK_KPT; ++x) tile[x * RANK_THREADS + tid] = key[x];
                } else {
                    int32_t tile_id[RANK_KPT];
#pragma unroll
                    for (int x = 0; x < RANK_KPT; ++x) {
                        const int j = t0 + x * RANK_THREADS + tid;
                        tile_id[x] = list[j < n ? j : n - 1];
                    }
#pragma unroll
                    for (int x = 0; x < RANK_KPT; ++x) {
                        const int j = t0 + x * RANK_THREADS + tid;
                        const float d = fabsf(q.c - rank_score(a, tile_id[x], j < n));
                        tile[x * RANK_THREADS + tid] = j < n ? ((uint64_t)orderable(d) << 32) | (uint32_t)j : ~0ull;
                    }
                }
                __syncthreads();
                const int tn = n - t0 < RANK_SLICE ? n - t0 : RANK_SLICE;
                if (nu <= 1) rank_count_tile<1>(tile, tn, key, below);
                else if (nu <= 2) rank_count_tile<2>(tile, tn, key, below);
                else if (nu <= 4) rank_count_tile<4>(tile, tn, key, below);
                else rank_count_tile<RANK_KPT>(tile, tn, key, below);
            }
#pragma unroll
            for (int x = 0; x < RANK_KPT; ++x) {
                const int j = base + x * RANK_THREADS + tid;
                if (j < n) {
                    const int slot = below[x] < n ? below[x] : n - 1;
                    a.out_ids[q.obeg + slot] = id[x];
                    a.out_dist[q.obeg + slot] = dist[x];
                }
            }
        }
        __syncthreads();                                                             // (the next row's first tile)
    }
}

// the two launches over the lists (and the plan) in `w`: rows (r, b), b < B, of a batch that is ids [b_off, b_off + B) of n_total
// (declared in infer.h; g: the graph whose rows were planned and selected, s0 [n_scores], centre b's score s0[nodes[b] + center_off])
int launch_rank_lists(const pcg_graph_desc *g, const int32_t *nodes, int32_t B, int64_t n_total, int64_t b_off, const float *s0,
                      const float *center_s0, const Workspace &w, const int64_t *out_begin, int32_t *out_ids, float *out_dist,
                      uint32_t *status, int64_t center_off, int64_t n_scores, hipStream_t st) {
    RankArgs a;
    a.w = w;
    a.nodes = nodes;
    a.B = B;
    a.n_rel = g->n_rel;
    a.n_nodes = n_scores;
    a.center_off = center_off;
    a.n_total = n_total;
    a.b_off = b_off;
    a.s0 = s0;
    a.center_s0 = center_s0;
    a.out_begin = out_begin;
    a.out_ids = out_ids;
    a.out_dist = out_dist;
    a.status = status;
    const int64_t rows = (int64_t)g->n_rel * B;
    const int64_t short_blocks = (rows + 15) / 16;                         // four waves a workgroup, up to four rows a wave
    hipLaunchKernelGGL(rank_short_rows, dim3((int)(short_blocks < RANK_SHORT_BLOCKS ? short_blocks : RANK_SHORT_BLOCKS)),
                       dim3(RANK_THREADS), 0, st, a);
    PCG_LAUNCH_CHECK();
    if (g->max_degree > PCG_WAVE) {                                        // (a row keeps no more than it has)
        int64_t slices = ((int64_t)g->max_degree + RANK_SLICE - 1) / RANK_SLICE;
        slices = slices > 64 ? 64 : slices;                                // (longer rows: a workgroup takes several slices)
        hipLaunchKernelGGL(rank_wg_rows, dim3((int)(rows < RANK_WG_BLOCKS ? rows : RANK_WG_BLOCKS), (int)slices), dim3(RANK_THREADS),
                           0, st, a);
        PCG_LAUNCH_CHECK();
    }
    return PCG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The minority picks of train-mode rows, ranked, with their distances (choose_step_neighs' tail, src/layers.py:675-691).
//
// A positive centre's picks are the m training positives nearest to its score c: a function of c, m, the sorted train-pos
// keys and train_pos - nothing of the row, nothing of the selection list (which stores them in window order, without
// distances, and turns a duplicate of a kept neighbour into a hole).  Row (r, i)'s m is its extent in out_begin; the order
// is the unique key (orderable(|c - s_p|) << 32) | p, p = position in train_pos: torch.sort(stable) over train_pos order, and
// select_rows' tie rule (ties at the m-th distance go to the smallest positions).
//   window      M = max_r m_r.  pc = the first sorted key whose score is >= c.  Left of pc the distances fall with the index,
//               from pc on they rise (rounding is monotone), so the M nearest are in [pc - M, pc + M) - once each end is
//               extended over its run of EQUAL distances (bisected): an element outside then has at least M strictly nearer
//               ones on its own side, whatever its position.  Nothing outside can precede a candidate of rank < M, so a
//               candidate's slot is the number of smaller candidate keys; the order does not depend on the relation: row
//               (r, i) is the prefix slot < m_r, one ranking per centre serves every relation.
//   rank_minor_short   <= 64 candidates: one wave per centre, lane against lane (readlane)
//   rank_minor_wg      more: work item = (centre, slice of RANK_SLICE candidates), counted against all of the centre's
//                      candidates tile by tile in LDS (rank_count_tile).  Quadratic in the candidate count: a tie run of
//                      thousands (constant scores) is exact, not fast.
// The keys come from an earlier launch: plain loads.  No workgroup waits for another; the only atomic is the OR into the
// status word.  Every loop is bounded by P.  A row whose extent is negative, above P or leaves [0, out_begin[R * n]) sets
// PCG_ST_RANK_MISMATCH and is not written; a position read from a key is clamped below P before train_pos is read; a slot is
// written only below its row's extent.
struct MinorArgs {
    const int32_t *nodes;       // [n]
    int32_t n, n_rel, P;
    int64_t n_nodes;
    const float *s0, *center_s0;
    const uint64_t *keys;       // [P] sorted (orderable(score) << 32 | position in train_pos)
    const int32_t *train_pos;   // [P]
    const int64_t *out_begin;   // [n_rel * n + 1]
    int32_t *out_ids;
    float *out_dist;
    uint32_t *status;
};

struct MinorWin {
    int lo, N, M;               // candidates = sorted keys [lo, lo + N); M == 0: nothing to do
    float c;
};

// row (r, i)'s extent, checked: m (-1: rejected) and where it begins
__device__ __forceinline__ int minor_extent(const MinorArgs &a, int r, int i, int64_t &obeg) {
    const int64_t at = (int64_t)r * a.n + i;
    const int64_t b = a.out_begin[at], e = a.out_begin[at + 1], cap = a.out_begin[(int64_t)a.n_rel * a.n];
    obeg = b;
    const bool ok = e >= b && e - b <= (int64_t)a.P && b >= 0 && e <= cap;
    return ok ? (int)(e - b) : -1;
}

__device__ __forceinline__ float minor_score(const MinorArgs &a, int x) { return from_orderable((uint32_t)(a.keys[x] >> 32)); }

// the candidate window of centre i (uniform over the wave / workgroup: every lane reads the same words)
__device__ __forceinline__ MinorWin minor_window(const MinorArgs &a, int i, bool report) {
    MinorWin w;
    w.lo = 0; w.N = 0; w.M = 0; w.c = 0.f;
    bool bad = false;
    for (int r = 0; r < a.n_rel; ++r) {
        int64_t obeg;
        const int m = minor_extent(a, r, i, obeg);
        bad |= m < 0;
        w.M = m > w.M ? m : w.M;
    }
    if (bad && report && a.status && (threadIdx.x & (PCG_WAVE - 1)) == 0) atomicOr(a.status, (uint32_t)PCG_ST_RANK_MISMATCH);
    if (w.M == 0) return w;
    int64_t node = a.nodes[i];
    node = node < 0 ? 0 : (node >= a.n_nodes ? a.n_nodes - 1 : node);
    const float c = a.center_s0 ? a.center_s0[i] : a.s0[node];
    w.c = c;
    const int P = a.P, M = w.M;
    int lo = 0, hi = P;
    while (lo < hi) {                                                      // pc: <= 31 steps
        const int mid = lo + ((hi - lo) >> 1);
        if (minor_score(a, mid) < c) lo = mid + 1; else hi = mid;
    }
    const int pc = lo;
    int wa = pc - M > 0 ? pc - M : 0;
    int wb = (int64_t)pc + M < (int64_t)P ? pc + M : P;
    if (wa > 0 && wa < pc) {                                               // the run of distances equal to the left end's
        const float d = fabsf(c - minor_score(a, wa));
        lo = 0; hi = wa;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (fabsf(c - minor_score(a, mid)) > d) lo = mid + 1; else hi = mid;
        }
        wa = lo;
    }
    if (wb < P && wb > pc) {                                               // ... and to the right end's
        const float d = fabsf(c - minor_score(a, wb - 1));
        lo = wb; hi = P;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (fabsf(c - minor_score(a, mid)) <= d) lo = mid + 1; else hi = mid;
        }
        wb = lo;
    }
    w.lo = wa;
    w.N = wb - wa;
    return w;
}

// candidate t of a window: its ranking key, its id and its distance
__device__ __forceinline__ uint64_t minor_key(const MinorArgs &a, const MinorWin &w, int t, bool valid, int32_t &id, float &dist) {
    const uint64_t k = a.keys[w.lo + (valid ? t : 0)];
    uint32_t p = (uint32_t)k;
    dist = fabsf(w.c - from_orderable((uint32_t)(k >> 32)));
    const uint64_t key = valid ? ((uint64_t)orderable(dist) << 32) | p : ~0ull;
    p = p < (uint32_t)a.P ? p : (uint32_t)a.P - 1;
    id = a.train_pos[p];
    return key;
}

// one centre per wave, wave-strided; reports the rejected extents of EVERY centre (rank_minor_wg does not)
__global__ void __launch_bounds__(RANK_THREADS) rank_minor_short(const MinorArgs a) {
    const int lane = lane_id();
    const int n_waves = (int)gridDim.x * (RANK_THREADS / PCG_WAVE);
    const int wave = (int)blockIdx.x * (RANK_THREADS / PCG_WAVE) + ((int)threadIdx.x >> 6);
    for (int iw = wave; iw < a.n; iw += n_waves) {
        const int i = __builtin_amdgcn_readfirstlane(iw);
        const MinorWin w = minor_window(a, i, true);
        if (w.M == 0 || w.N > PCG_WAVE) continue;                          // (more candidates: rank_minor_wg)
        const bool have = lane < w.N;
        int32_t id;
        float dist;
        const uint64_t mine = minor_key(a, w, lane, have, id, dist);
        const uint32_t mh = (uint32_t)(mine >> 32), ml = (uint32_t)mine;
        int slot = 0;
        for (int j = 0; j < w.N; ++j) {                                    // N is wave-uniform
            const uint32_t oh = (uint32_t)__builtin_amdgcn_readlane((int)mh, j), ol = (uint32_t)__builtin_amdgcn_readlane((int)ml, j);
            slot += (oh < mh) || (oh == mh && ol < ml);
        }
        for (int r = 0; r < a.n_rel; ++r) {
            int64_t obeg;
            const int m = minor_extent(a, r, i, obeg);
            if (have && slot < m) {
                a.out_ids[obeg + slot] = id;
                a.out_dist[obeg + slot] = dist;
            }
        }
    }
}

// centres of more than 64 candidates: blockIdx.x strides over the centres, blockIdx.y over a centre's slices of RANK_SLICE
__global__ void __launch_bounds__(RANK_THREADS) rank_minor_wg(const MinorArgs a) {
    __shared__ uint64_t tile[RANK_SLICE];
    const int tid = (int)threadIdx.x;
    for (int i = (int)blockIdx.x; i < a.n; i += (int)gridDim.x) {
        const MinorWin w = minor_window(a, i, false);
        const int n = w.N;
        if (w.M == 0 || n <= PCG_WAVE) continue;                           // (rank_minor_short)
        for (int64_t base64 = (int64_t)blockIdx.y * RANK_SLICE; base64 < n; base64 += (int64_t)gridDim.y * RANK_SLICE) {
            const int base = (int)base64;
            int32_t id[RANK_KPT];
            float dist[RANK_KPT];
            uint64_t key[RANK_KPT];
            int below[RANK_KPT];
#pragma unroll
            for (int x = 0; x < RANK_KPT; ++x) {
                const int t = base + x * RANK_THREADS + tid;
                key[x] = minor_key(a, w, t, t < n, id[x], dist[x]);
                below[x] = 0;
            }
            const int mine = n - base < RANK_SLICE ? n - base : RANK_SLICE;          // entries of this slice
            const int nu = (mine + RANK_THREADS - 1) / RANK_THREADS;                 // key[x], x >= nu: no thread has one
            for (int t0 = 0; t0 < n; t0 += RANK_SLICE) {
                __syncthreads();                                                     // (the tile before: its reads)
                if (t0 == base) {
#pragma unroll
                    for (int x = 0; x < RANK_KPT; ++x) tile[x * RANK_THREADS + tid] = key[x];
                } else {
#pragma unroll
                    for (int x = 0; x < RANK_KPT; ++x) {
                        const int t = t0 + x * RANK_THREADS + tid;
                        int32_t tid_id;
                        float td;
                        tile[x * RANK_THREADS + tid] = minor_key(a, w, t, t < n, tid_id, td);
                    }
                }
                __syncthreads();
                const int tn = n - t0 < RANK_SLICE ? n - t0 : RANK_SLICE;
                if (nu <= 1) rank_count_tile<1>(tile, tn, key, below);
                else if (nu <= 2) rank_count_tile<2>(tile, tn, key, below);
                else if (nu <= 4) rank_count_tile<4>(tile, tn, key, below);
                else rank_count_tile<RANK_KPT>(tile, tn, key, below);
            }
            for (int r = 0; r < a.n_rel; ++r) {                                      // (uniform: the row's words once)
                int64_t obeg;
                const int m = minor_extent(a, r, i, obeg);
#pragma unroll
                for (int x = 0; x < RANK_KPT; ++x) {
                    const int t = base + x * RANK_THREADS + tid;
                    if (t < n && below[x] < m) {
                        a.out_ids[obeg + below[x]] = id[x];
                        a.out_dist[obeg + below[x]] = dist[x];
                    }
                }
            }
        }
        __syncthreads();                                                             // (the next centre's first tile)
    }
}

}  // namespace pcg

extern "C" {

int pcg_rank_minority(const pcg_graph_desc *g, const int32_t *nodes, int32_t n, const float *s0, const float *center_s0,
                      const uint64_t *pos_keys, const int64_t *out_begin, int32_t *out_ids, float *out_dist, uint32_t *status,
                      void *stream) {
    if (!g || n < 0 || g->n_pos < 0 || g->n_rel < 1 || g->n_rel > PCG_MAX_REL || g->n_nodes < 1) return PCG_E_ARG;
    if ((int64_t)g->n_rel * n >= (1ll << 31)) return PCG_E_ARG;
    if (n == 0 || g->n_pos == 0) return PCG_OK;
    if (!nodes || !s0 || !pos_keys || !g->train_pos || !out_begin || !out_ids || !out_dist || !status) return PCG_E_ARG;
    pcg::MinorArgs a;
    a.nodes = nodes;
    a.n = n;
    a.n_rel = g->n_rel;
    a.P = g->n_pos;
    a.n_nodes = g->n_nodes;
    a.s0 = s0;
    a.center_s0 = center_s0;
    a.keys = pos_keys;
    a.train_pos = g->train_pos;
    a.out_begin = out_begin;
    a.out_ids = out_ids;
    a.out_dist = out_dist;
    a.status = status;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t short_blocks = ((int64_t)n + 3) / 4;                     // four waves a workgroup, one centre a wave
    hipLaunchKernelGGL(pcg::rank_minor_short, dim3((int)(short_blocks < pcg::RANK_SHORT_BLOCKS ? short_blocks : pcg::RANK_SHORT_BLOCKS)),
                       dim3(pcg::RANK_THREADS), 0, st, a);
    PCG_LAUNCH_CHECK();
    if (g->n_pos > PCG_WAVE) {                                             // (a centre has no more candidates than P)
        int64_t slices = ((int64_t)g->n_pos + pcg::RANK_SLICE - 1) / pcg::RANK_SLICE;
        slices = slices > 16 ? 16 : slices;                                // (more: a workgroup takes several slices)
        hipLaunchKernelGGL(pcg::rank_minor_wg, dim3(n < pcg::RANK_WG_BLOCKS ? n : pcg::RANK_WG_BLOCKS, (int)slices),
                           dim3(pcg::RANK_THREADS), 0, st, a);
        PCG_LAUNCH_CHECK();
    }
    return PCG_OK;
}

int pcg_rank_lists(const pcg_graph_desc *g, const int32_t *nodes, int32_t B, const float *s0, const float *center_s0,
                   const void *workspace, int64_t list_capacity, const int64_t *out_begin, int32_t *out_ids, float *out_dist,
                   uint32_t *status, void *stream) {
    if (!g || !nodes || B < 0 || !s0 || !workspace || !out_begin || !out_ids || !out_dist || !status) return PCG_E_ARG;
    if (list_capacity < 1 || list_capacity >= (1ll << 31) || g->n_rel < 1 || g->n_rel > PCG_MAX_REL || g->n_nodes < 1) return PCG_E_ARG;
    if ((int64_t)g->n_rel * B >= (1ll << 31)) return PCG_E_ARG;
    if (B == 0) return PCG_OK;
    pcg::Workspace w;
    pcg::carve1(g, B, list_capacity, static_cast<unsigned char *>(const_cast<void *>(workspace)), &w);
    return pcg::launch_rank_lists(g, nodes, B, B, 0, s0, center_s0, w, out_begin, out_ids, out_dist, status, 0, g->n_nodes,
                                  static_cast<hipStream_t>(stream));
}

int64_t pcg_chosen_workspace_bytes(const pcg_graph_desc *g, int32_t chunk_rows, int64_t list_capacity) {
    // (pcg_infer_set's two plan slots and data part, then cnt [R][chunk]: no dense parts)
    pcg::InferCarve c;
    const int rc = pcg::infer_carve(g, 2, false, 0, chunk_rows, list_capacity, c);
    return rc != PCG_OK ? rc : c.total;
}

int pcg_chosen_set(const pcg_graph_desc *g, const float *theta, int32_t emb, const int32_t *ids, int32_t n, int32_t chunk_rows,
                   float *s0, const double *thresholds, void *workspace, int64_t list_capacity, const int64_t *out_begin,
                   int32_t *out_ids, float *out_dist, uint32_t *status, void *stream) {
    if (!g || !g->X || !theta || !ids || n < 0 || !s0 || !thresholds || !workspace || !out_begin || !out_ids || !out_dist || !status)
        return PCG_E_ARG;
    if (!pcg::infer_table_ok(g)) return PCG_E_UNSUPPORTED;
    if (emb < 16 || emb % 16 != 0) return PCG_E_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(g->X) & 15u) != 0 || g->n_nodes < 1) return PCG_E_ARG;
    pcg::InferCarve c;
    int rc = pcg::infer_carve(g, 2, false, 0, chunk_rows, list_capacity, c);
    if (rc != PCG_OK) return rc;
    if (n == 0) return PCG_OK;
    const int F = g->feat_dim, E = emb, R = g->n_rel;
    const pcg::ChunkDriver d = pcg::infer_driver(g, ids, n, chunk_rows, list_capacity, thresholds, s0, 0, 2, workspace, c, status, stream);

    // pcg_infer_set's front: the score pass || the look-back words of both plan slots zeroed
    pcg::ZeroRegions z = {};
    pcg::infer_zero_regions(z, d);
    rc = pcg::launch_infer_front(g, theta + pcg::off_clf(F, E, R), theta + pcg::off_bias(F, E, R), s0, z, d.st);
    if (rc != PCG_OK) return rc;
    return d.run([&](int64_t off, int32_t B, const int32_t *cid, const pcg::Workspace &w) {
        return pcg::launch_rank_lists(g, cid, B, n, off, s0, nullptr, w, out_begin, out_ids, out_dist, status, 0, g->n_nodes, d.st);
    });
}

}  // extern "C"
