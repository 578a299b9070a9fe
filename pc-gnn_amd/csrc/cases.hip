// Alert cases on the device (gfx950, wave64): the slots of a member list (the alert list's ids, in alert order) grouped into the
// connected components of "linked" - two slots are linked when they name the same node or when, in a selected relation, either
// node occurs in the other's CSR row.  include/pcgnn.h states the outputs; every one is a function of the inputs alone.
//
//   fill      map[0 .. N) = absent (a byte memset: 4 N bytes per call), the queue counter = 0, the header = 0
//   init      per slot: map[id] = min(map[id], slot) (integer atomicMin: the first slot of a node), parent[slot] = slot, the
//             slot's link count and the per-case sums = 0; an id outside [0, N) other than -1 sets PCG_ST_LIST_ID_RANGE, a label
//             outside {0, 1} on a valid slot PCG_ST_EVAL_INPUT
//   link      one wave per (slot, selected relation), grid-stride: the row is walked 64 entries at a time, map[neighbour] is one
//             4-byte read at a random address per entry; where a member other than the slot's own node is found the entry is
//             counted and the two slots are united.  A row of more than CS_ROW_MAX entries is not walked here: (slot, relation)
//             goes into a queue.  The first selected relation's wave also unites a slot with the first slot of its node.
//   long      every queued row is cut into CS_PARTS equal parts, a workgroup per part, grid-stride: no wave walks a hub's row alone.
//   flatten   root[slot] = find(slot)
//   number    one workgroup: the heads (root == slot) are counted below every slot: head[c], the case number of a head, C
//   assign    case_of[slot] = number of its root; size / links / hits of the case += the slot's (integer atomics); the sort key
//   order     pcg_topk_alerts (rank_eval.hip) of the key -case_of, k = n = m: its stable descending sort is the slots by case
//             ascending and by slot ascending inside a case; padding slots (key -inf) come last
//   offsets   one workgroup: exclusive scan of the sizes; the header (C, valid slots, the status word)
//
// The union is lock-free union-find.  parent[] only ever moves towards smaller slots and only a root is hooked
// (atomicCAS(&parent[hi], hi, lo), hi > lo): the root of a component is its lowest slot whatever order the hooks land in.  Every
// access to parent[] inside link / long / flatten is an agent-scope atomic (the loads go to L2, not to a CU's L1), a stale value
// would be an older but valid state, and the CAS decides.  A failed CAS continues from the value it returned.  No wave waits for
// another: at most m - 1 hooks ever succeed and a CAS fails only because another hook succeeded, so a union needs at most m
// attempts and a find at most m steps; either loop gives up after that with PCG_ST_SYNC_TIMEOUT.  All sums are integer sums.
#include "common.h"

namespace pcg {
namespace cases {

constexpr int CS_THREADS = 256;               // workgroup of the per-slot passes, of link (4 waves = 4 rows) and of long
constexpr int CS_ROW_MAX = 512;               // longest row a single wave walks
constexpr int CS_PARTS = 16;                  // workgroups a longer row is spread over
constexpr int CS_SCAN_THREADS = 1024;         // the one workgroup of number / offsets
constexpr int CS_GRID_CAP = 2048;             // workgroups of the grid-stride passes
constexpr int CS_ABSENT = 0x7f7f7f7f;         // map: no slot names this node (what the byte memset writes)
constexpr int CS_MAX_M = PCG_ALERTS_MAX_K;

struct Rels {
    int n;
    int r[PCG_MAX_REL];
};

struct Carve {
    int64_t ctr, map, parent, slot_links, root, cnum, size, key, score, queue, order_ws, total;
};
__host__ inline int64_t up256(int64_t x) { return (x + 255) / 256 * 256; }
__host__ inline void carve(int64_t n_nodes, int32_t m, Carve &c) {
    const int64_t mb = up256(4 * (int64_t)(m > 0 ? m : 1));
    int64_t at = 0;
    c.ctr = at, at += 256;
    c.map = at, at += up256(4 * n_nodes);
    c.parent = at, at += mb;
    c.slot_links = at, at += mb;
    c.root = at, at += mb;
    c.cnum = at, at += mb;
    c.size = at, at += mb;
    c.key = at, at += mb;
    c.score = at, at += mb;
    c.queue = at, at += PCG_MAX_REL * mb;
    c.order_ws = at, at += up256(m > 0 ? pcg_topk_alerts_workspace_bytes(m, m) : 0);
    c.total = at;
}

__device__ __forceinline__ int ld_parent(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x; halves the path on the way (x is no root when it is rewritten and never becomes one again)
__device__ __forceinline__ int find_root(int *parent, int x, int m, bool &ok) {
    for (int i = 0; i <= m; ++i) {
        const int q = ld_parent(parent + x);
        if (q == x) return x;
        const int gq = ld_parent(parent + q);
        if (gq != q) __hip_atomic_fetch_min(parent + x, gq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = gq;
    }
    ok = false;
    return x;
}

// one component out of the components of slots a and b; false: the bounded loops ran out
__device__ __forceinline__ bool unite(int *parent, int a, int b, int m) {
    bool ok = true;
    for (int tries = 0; tries <= m; ++tries) {
        a = find_root(parent, a, m, ok);
        b = find_root(parent, b, m, ok);
        if (!ok) return false;
        if (a == b) return true;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        int seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return true;
        a = seen;                                                          // (hi was hooked by somebody else: go on from where it hangs)
        b = lo;
    }
    return false;
}

__device__ __forceinline__ void or_status(uint32_t *status, uint32_t bits) { atomicOr(status, bits); }

__global__ void __launch_bounds__(CS_THREADS)
init_kernel(const int32_t *__restrict__ members, const int32_t *__restrict__ labels, int m, int64_t n_nodes, int *__restrict__ map,
            int *__restrict__ parent, int *__restrict__ slot_links, int *__restrict__ size, int32_t *__restrict__ links,
            int32_t *__restrict__ hits, uint32_t *__restrict__ status) {
    for (int p = (int)(blockIdx.x * blockDim.x + threadIdx.x); p < m; p += (int)(gridDim.x * blockDim.x)) {
        const int id = members[p];
        const bool valid = id >= 0 && (int64_t)id < n_nodes;
        uint32_t bad = (!valid && id != -1) ? (uint32_t)PCG_ST_LIST_ID_RANGE : 0u;
        if (valid) {
            atomicMin(map + id, p);
            if (labels && (labels[p] < 0 || labels[p] > 1)) bad |= (uint32_t)PCG_ST_EVAL_INPUT;
        }
        if (bad) or_status(status, bad);
        parent[p] = p;
        slot_links[p] = 0;
        size[p] = 0;
        links[p] = 0;
        if (hits) hits[p] = 0;
    }
}

// entries [beg, end) of a row of node `id` (slot p), entry beg + first, beg + first + step, ... by this thread; the whole wave
// runs every iteration (the ballot).  -> the wave's count of entries that name a member other than `id`
__device__ __forceinline__ int walk_row(const int32_t *__restrict__ idx, int64_t beg, int64_t end, int first, int step, int id, int p,
                                        int m, int64_t n_nodes, const int *__restrict__ map, int *parent, uint32_t *status) {
    int count = 0;
    const int64_t len = end - beg;
    for (int64_t j0 = 0; j0 < len; j0 += step) {                           // (wave-uniform trip count)
        const int64_t j = j0 + first;
        int q = CS_ABSENT;
        if (j < len) {
            const int nb = idx[beg + j];
            if (nb < 0 || (int64_t)nb >= n_nodes) or_status(status, PCG_ST_LIST_ID_RANGE);
            else if (nb != id) q = map[nb];
        }
        const bool hit = q != CS_ABSENT;
        count += wave_count(hit);
        if (hit && !unite(parent, p, q, m)) or_status(status, PCG_ST_SYNC_TIMEOUT);
    }
    return count;
}

__global__ void __launch_bounds__(CS_THREADS)
link_kernel(const pcg_graph_desc g, const int32_t *__restrict__ members, int m, const Rels rels, const int *__restrict__ map,
            int *parent, int *slot_links, int32_t *__restrict__ queue, uint32_t *queue_n, uint32_t *status) {
    const int lane = lane_id();
    const int waves = (int)(gridDim.x * (blockDim.x >> 6));
    const int items = m * rels.n;
    for (int item = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); item < items; item += waves) {
        const int p = item / rels.n, ri = item - p * rels.n;
        const int id = members[p];
        if (id < 0 || (int64_t)id >= g.n_nodes) continue;                  // (wave-uniform)
        if (ri == 0 && lane == 0) {
            const int first = map[id];                                      // the same node at a lower slot
            if (first != p && !unite(parent, p, first, m)) or_status(status, PCG_ST_SYNC_TIMEOUT);
        }
        const int r = rels.r[ri];
        const int64_t *ip = static_cast<const int64_t *>(g.indptr[r]);
        const int64_t beg = ip[id], end = ip[id + 1];
        if (end - beg > CS_ROW_MAX) {
            if (lane == 0) queue[atomicAdd(queue_n, 1u)] = p * PCG_MAX_REL + r;     // (at most m * n_rel entries: its capacity)
            continue;
        }
        const int count = walk_row(static_cast<const int32_t *>(g.indices[r]), beg, end, lane, PCG_WAVE, id, p, m, g.n_nodes, map, parent, status);
        if (lane == 0 && count) atomicAdd(slot_links + p, count);
    }
}

__global__ void __launch_bounds__(CS_THREADS)
long_kernel(const pcg_graph_desc g, const int32_t *__restrict__ members, int m, const int *__restrict__ map, int *parent,
            int *slot_links, const int32_t *__restrict__ queue, const uint32_t *__restrict__ queue_n, uint32_t *status) {
    const int64_t cap = (int64_t)m * PCG_MAX_REL, queued = (int64_t)queue_n[0];
    const int64_t items = (queued < cap ? queued : cap) * CS_PARTS;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int e = queue[item / CS_PARTS], part = (int)(item % CS_PARTS);
        const int p = e / PCG_MAX_REL, r = e % PCG_MAX_REL;
        const int id = members[p];
        const int64_t *ip = static_cast<const int64_t *>(g.indptr[r]);
        const int64_t beg = ip[id], end = ip[id + 1];
        const int64_t span = (end - beg + CS_PARTS - 1) / CS_PARTS;
        int64_t b = beg + part * span, t = b + span;
        if (b > end) b = end;
        if (t > end) t = end;
        const int count = walk_row(static_cast<const int32_t *>(g.indices[r]), b, t, (int)threadIdx.x, CS_THREADS, id, p, m, g.n_nodes, map, parent, status);
        if (lane_id() == 0 && count) atomicAdd(slot_links + p, count);
    }
}

__global__ void __launch_bounds__(CS_THREADS)
flatten_kernel(const int32_t *__restrict__ members, int m, int64_t n_nodes, int *parent, int *__restrict__ root, uint32_t *status) {
    for (int p = (int)(blockIdx.x * blockDim.x + threadIdx.x); p < m; p += (int)(gridDim.x * blockDim.x)) {
        const int id = members[p];
        bool ok = true;
        const int rt = (id >= 0 && (int64_t)id < n_nodes) ? find_root(parent, p, m, ok) : -1;
        root[p] = ok ? rt : -1;                                            // (a find that ran out names no head: the slot is left out)
        if (!ok) or_status(status, PCG_ST_SYNC_TIMEOUT);
    }
}

// exclusive scan of one value per thread over the workgroup (CS_SCAN_THREADS threads); sh: 16 ints + 1; -> the total in `total`
__device__ __forceinline__ int block_exclusive_scan(int v, int *sh, int &total) {
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < PCG_WAVE; o <<= 1) {
        const int up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    __syncthreads();                                                       // (sh may still be read from the previous scan)
    if (lane == PCG_WAVE - 1) sh[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < CS_SCAN_THREADS / PCG_WAVE; ++w) {
        const int s = sh[w];
        before += w < wave ? s : 0;
        all += s;
    }
    total = all;
    return before + inc - v;
}

// thread t owns the slots [t * per, (t + 1) * per)
__global__ void __launch_bounds__(CS_SCAN_THREADS)
number_kernel(const int *__restrict__ root, int m, int *__restrict__ cnum, int32_t *__restrict__ head, int32_t *__restrict__ hdr) {
    __shared__ int sh[CS_SCAN_THREADS / PCG_WAVE];
    const int per = (m + CS_SCAN_THREADS - 1) / CS_SCAN_THREADS;
    const int lo = (int)threadIdx.x * per, hi = lo + per < m ? lo + per : m;
    int heads = 0;
    for (int p = lo; p < hi; ++p) heads += root[p] == p;
    int total;
    int c = block_exclusive_scan(heads, sh, total);
    for (int p = lo; p < hi; ++p)
        if (root[p] == p) {
            cnum[p] = c;
            head[c] = p;
            ++c;
        }
    if (threadIdx.x == 0) hdr[0] = total;
}

__global__ void __launch_bounds__(CS_THREADS)
assign_kernel(const int *__restrict__ root, const int *__restrict__ cnum, const int *__restrict__ slot_links,
              const int32_t *__restrict__ labels, int m, int32_t *__restrict__ case_of, int *size, int32_t *links, int32_t *hits,
              float *__restrict__ key) {
    for (int p = (int)(blockIdx.x * blockDim.x + threadIdx.x); p < m; p += (int)(gridDim.x * blockDim.x)) {
        const int rt = root[p];
        if (rt < 0) {
            case_of[p] = -1;
            key[p] = -__builtin_inff();
            continue;
        }
        const int c = cnum[rt];
        case_of[p] = c;
        key[p] = -(float)c;                                                // (exact: c < 2^24)
        atomicAdd(size + c, 1);
        if (slot_links[p]) atomicAdd(links + c, slot_links[p]);
        if (hits && labels[p] == 1) atomicAdd(hits + c, 1);
    }
}

// offsets[0 .. C] from the sizes; hdr = C, valid slots, the status word, 0
__global__ void __launch_bounds__(CS_SCAN_THREADS)
offsets_kernel(const int *__restrict__ size, int32_t *__restrict__ offsets, int32_t *__restrict__ hdr, const uint32_t *__restrict__ status) {
    __shared__ int sh[CS_SCAN_THREADS / PCG_WAVE];
    int n_cases = hdr[0];
    n_cases = n_cases < 0 ? 0 : (n_cases > CS_MAX_M ? CS_MAX_M : n_cases);
    const int per = (n_cases + CS_SCAN_THREADS - 1) / CS_SCAN_THREADS;
    const int lo = (int)threadIdx.x * per, hi = lo + per < n_cases ? lo + per : n_cases;
    int sum = 0;
    for (int c = lo; c < hi; ++c) sum += size[c];
    int total;
    int at = block_exclusive_scan(sum, sh, total);
    for (int c = lo; c < hi; ++c) {
        offsets[c] = at;
        at += size[c];
    }
    if (threadIdx.x == 0) {
        offsets[n_cases] = total;
        hdr[1] = total;
        hdr[2] = (int32_t)status[0];
        hdr[3] = 0;
    }
}

static unsigned grid_for(int64_t threads_wanted) {
    int64_t b = (threads_wanted + CS_THREADS - 1) / CS_THREADS;
    return (unsigned)(b < 1 ? 1 : (b > CS_GRID_CAP ? CS_GRID_CAP : b));
}

}  // namespace cases
}  // namespace pcg

extern "C" {

int64_t pcg_alert_cases_workspace_bytes(int64_t n_nodes, int32_t m) {
    if (n_nodes < 1 || n_nodes > 0x7fffffffll || m < 0 || m > PCG_ALERTS_MAX_K) return PCG_E_ARG;
    pcg::cases::Carve c;
    pcg::cases::carve(n_nodes, m, c);
    return c.total;
}

int pcg_alert_cases(const pcg_graph_desc *g, const int32_t *members, int32_t m, uint32_t rel_mask, const int32_t *labels, void *workspace,
                    int64_t workspace_bytes, int32_t *case_of, int32_t *head, int32_t *offsets, int32_t *order, int32_t *links,
                    int32_t *hits, int32_t *hdr, uint32_t *status, void *stream) {
    namespace cs = pcg::cases;
    if (!g || !workspace || !offsets || !hdr || !status || m < 0 || m > PCG_ALERTS_MAX_K) return PCG_E_ARG;
    if (g->n_nodes < 1 || g->n_nodes > 0x7fffffffll || g->n_rel < 1 || g->n_rel > PCG_MAX_REL) return PCG_E_ARG;
    if (rel_mask == 0 || (g->n_rel < 32 && (rel_mask >> g->n_rel) != 0)) return PCG_E_ARG;
    if ((labels == nullptr) != (hits == nullptr)) return PCG_E_ARG;
    if (m > 0 && (!members || !case_of || !head || !order || !links)) return PCG_E_ARG;
    cs::Carve c;
    cs::carve(g->n_nodes, m, c);
    if (workspace_bytes < c.total || (reinterpret_cast<uintptr_t>(workspace) & 255u) != 0) return PCG_E_ARG;
    cs::Rels rels{};
    for (int r = 0; r < g->n_rel; ++r)
        if ((rel_mask >> r) & 1u) {
            if (!g->indptr[r] || !g->indices[r]) return PCG_E_ARG;
            rels.r[rels.n++] = r;
        }

    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    uint32_t *queue_n = reinterpret_cast<uint32_t *>(ws + c.ctr);
    int *map = reinterpret_cast<int *>(ws + c.map), *parent = reinterpret_cast<int *>(ws + c.parent);
    int *slot_links = reinterpret_cast<int *>(ws + c.slot_links), *root = reinterpret_cast<int *>(ws + c.root);
    int *cnum = reinterpret_cast<int *>(ws + c.cnum), *size = reinterpret_cast<int *>(ws + c.size);
    float *key = reinterpret_cast<float *>(ws + c.key), *score = reinterpret_cast<float *>(ws + c.score);
    int32_t *queue = reinterpret_cast<int32_t *>(ws + c.queue);

    if (hipMemsetAsync(hdr, 0, 16, st) != hipSuccess) return PCG_E_LAUNCH;
    if (m > 0) {
        if (hipMemsetAsync(ws + c.ctr, 0, 256, st) != hipSuccess) return PCG_E_LAUNCH;
        if (hipMemsetAsync(map, 0x7f, (size_t)(4 * g->n_nodes), st) != hipSuccess) return PCG_E_LAUNCH;
        const unsigned slots_grid = cs::grid_for(m);
        hipLaunchKernelGGL(cs::init_kernel, dim3(slots_grid), dim3(cs::CS_THREADS), 0, st, members, labels, (int)m, (int64_t)g->n_nodes, map,
                           parent, slot_links, size, links, hits, status);
        PCG_LAUNCH_CHECK();
        hipLaunchKernelGGL(cs::link_kernel, dim3(cs::grid_for((int64_t)m * rels.n * PCG_WAVE)), dim3(cs::CS_THREADS), 0, st, *g, members,
                           (int)m, rels, map, parent, slot_links, queue, queue_n, status);
        PCG_LAUNCH_CHECK();
        hipLaunchKernelGGL(cs::long_kernel, dim3(cs::CS_GRID_CAP), dim3(cs::CS_THREADS), 0, st, *g, members, (int)m, map, parent, slot_links,
                           queue, queue_n, status);
        PCG_LAUNCH_CHECK();
        hipLaunchKernelGGL(cs::flatten_kernel, dim3(slots_grid), dim3(cs::CS_THREADS), 0, st, members, (int)m, (int64_t)g->n_nodes, parent,
                           root, status);
        PCG_LAUNCH_CHECK();
        hipLaunchKernelGGL(cs::number_kernel, dim3(1), dim3(cs::CS_SCAN_THREADS), 0, st, root, (int)m, cnum, head, hdr);
        PCG_LAUNCH_CHECK();
        hipLaunchKernelGGL(cs::assign_kernel, dim3(slots_grid), dim3(cs::CS_THREADS), 0, st, root, cnum, slot_links, labels, (int)m, case_of,
                           size, links, hits, key);
        PCG_LAUNCH_CHECK();
        const int rc = pcg_topk_alerts(key, 1, m, m, ws + c.order_ws, order, score, status, stream);
        if (rc != PCG_OK) return rc;
    }
    hipLaunchKernelGGL(cs::offsets_kernel, dim3(1), dim3(cs::CS_SCAN_THREADS), 0, st, size, offsets, hdr, status);
    PCG_LAUNCH_CHECK();
    return PCG_OK;
}

}  // extern "C"
