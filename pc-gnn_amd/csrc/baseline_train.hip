// Training steps of the GraphSAGE / GCN baselines (src/graphsage.py:37-39, 176-178; src/model_handler.py:124, 149-153) on gfx950:
// a whole id list in batches, forward, loss, backward and torch.optim.Adam's update on the device, no host synchronisation.
//
//   per batch: counter = 0 -> baseline_agg_rows_kernel -> baseline_agg_long_kernel      (baseline.h: as whole-set inference)
//              -> baseline_train_dense_kernel -> baseline_wgrad_adam_kernel
//
//   baseline_train_dense_kernel : 16-centre tiles; the forward is baseline_tile_forward (baseline.h), the very code of
//                                 baseline_dense_kernel: the logits are bit for bit pcg_baseline_infer's.  Then, per row, the two-class
//                                 cross entropy and dlogits = (softmax - onehot) / B (xent2), dpre = (W_cls^T dlogits) under the
//                                 ReLU's mask, and what the weight GEMMs read is stored TRANSPOSED in `acts` ([rows][ld], a batch row
//                                 per column, the layout at the top of wgrad.h): z [K] | h [E] | dpre [E] | dlogits [2]; the columns
//                                 of a tile beyond the batch are zero.  A tile's 16 loss terms are added in row order -> tile_loss.
//                                 The LDS is the forward's own (baseline_smem_bytes, W_enc staged when it fits, else streamed): the
//                                 16 x 3 floats of dlogits and loss terms lie over the K-split parts, which are dead by then.
//   baseline_wgrad_adam_kernel  : dW_cls [2][E] = dlogits h^T and dW_enc [E][K] = dpre z^T as f32-MFMA GEMMs over the batch, one
//                                 256-thread workgroup per 16 x 16 output tile and part: its four waves take a quarter of the
//                                 part's 16-row blocks each (ascending; inside a block the k order is the permutation 4 kq + i the
//                                 float4 reads imply), their tiles are added in wave order in LDS; with several parts (batches
//                                 beyond 1024 rows: ceil(B / 1024), at most BT_MAX_PARTS) the part that arrives last adds the
//                                 partial tiles in part order.  Thread (row, col) applies adam_update to its parameter, or stores
//                                 the gradient.  One more workgroup adds tile_loss in tile order and divides by B -> out_loss.
//
// No float atomics: every sum has a fixed order and the results are bitwise the same run to run; the only atomics are the
// aggregation queue's counter, the tiles' arrival tickets and the status word.  Stream order is the only synchronisation between
// the launches: the next batch's dense kernel is the first reader of the updated weights.
#include "baseline.h"

namespace pcg {

constexpr int BT_NB = 8;                 // 16-row blocks whose operands a wave has in flight
constexpr int BT_PART_BLOCKS = 8 * BT_NB;// blocks one workgroup covers in two rounds per wave: 1024 batch rows
constexpr int BT_MAX_PARTS = 4;          // (beyond 4096 rows the waves take more rounds)
constexpr int BT_THREADS = 256;

__host__ __device__ inline int bt_kparts(int n_kblocks) {
    const int p = (n_kblocks + BT_PART_BLOCKS - 1) / BT_PART_BLOCKS;
    return p < 1 ? 1 : (p > BT_MAX_PARTS ? BT_MAX_PARTS : p);
}
// acts: z [K] | h [E] | dpre [E] | dlogits [2]
__host__ __device__ inline int bt_act_rows(int K, int E) { return K + 2 * E + 2; }
// the weight GEMMs' output tiles: dW_cls (2 rows: one tile row) | dW_enc (E / 16 tile rows of ceil(K / 16))
__host__ __device__ inline int bt_tiles(int K, int E) { return E / 16 + (E / 16) * ((K + 15) / 16); }

struct BaselineTrainDense {
    BaselineDense d;
    const int32_t *labels;
    float inv_B;
    float *acts;
    int32_t ld;
    float *tile_loss;            // [tiles of the batch]
    uint32_t *status;
};

template <bool WLDS>
__global__ void __launch_bounds__(BL_DENSE_THREADS) baseline_train_dense_kernel(const BaselineTrainDense a, int n_tiles) {
    extern __shared__ __align__(16) float sm[];
    const BaselineDense &d = a.d;
    const BaselineLds s = baseline_lds(sm, d.feat_dim, d.emb, d.concat_self);
    const int E = d.emb, K = baseline_K(d.feat_dim, d.concat_self), ldz = baseline_Kp(K) + 1, ldE = E + 1;
    float *s_dl = s.part;                             // [TB][2] dlogits | [TB] loss terms: over the K-split parts (>= 256 floats)
    float *s_loss = s.part + 2 * TB;
    const int tid = threadIdx.x;
    baseline_stage_weights<WLDS>(d, s);
    for (int tile = (int)blockIdx.x; tile < n_tiles; tile += (int)gridDim.x) {
        const int64_t row0 = (int64_t)tile * TB;
        float logit0, logit1;
        baseline_tile_forward<WLDS>(d, s, row0, logit0, logit1);
        // ---- the row's loss term and dlogits (graphsage.py:37-39): one lane per centre ----
        if ((tid & 15) == 0) {
            const int t = tid >> 4;
            const int64_t b = row0 + t;
            const bool live = b < d.B;
            const int32_t y = live ? a.labels[b] : 0;
            const bool ok = live && (y == 0 || y == 1);            // (a label outside {0, 1} is reported and indexes nothing)
            float loss = 0.f, d0 = 0.f, d1 = 0.f;
            if (ok) {
                xent2(logit0, logit1, y, loss, d0, d1);
                d0 *= a.inv_B;
                d1 *= a.inv_B;
            }
            s_dl[2 * t] = d0;
            s_dl[2 * t + 1] = d1;
            s_loss[t] = loss;
            if (live && !ok) atomicOr(a.status, (uint32_t)PCG_ST_EVAL_INPUT);
        }
        __syncthreads();
        if (tid == 0) {
            float sum = s_loss[0];
#pragma unroll
            for (int t = 1; t < TB; ++t) sum += s_loss[t];
            a.tile_loss[tile] = sum;
        }
        // ---- acts: 16 lanes store the tile's 16 columns of a row (64 contiguous bytes); LDS rows of odd pitch ----
        const int n_rows = bt_act_rows(K, E);
        for (int i = tid; i < n_rows * TB; i += BL_DENSE_THREADS) {
            const int r = i >> 4, t = i & 15;
            float v;
            if (r < K) v = s.z[t * ldz + r];
            else if (r < K + E) v = s.h[t * ldE + (r - K)];
            else if (r < K + 2 * E) {
                const int e = r - K - E;
                const float h = s.h[t * ldE + e];
                const float g = __builtin_fmaf(s.wc[E + e], s_dl[2 * t + 1], s.wc[e] * s_dl[2 * t]);
                v = h <= 0.f ? 0.f : g;                            // (torch's threshold_backward: a NaN h lets g through)
            } else v = s_dl[2 * t + (r - K - 2 * E)];
            a.acts[(size_t)r * a.ld + row0 + t] = row0 + t < d.B ? v : 0.f;
        }
        __syncthreads();                                           // (s.z, s.h and the parts are the next tile's)
    }
}

struct BaselineWgrad {
    const float *acts;
    int32_t ld, K, E;
    int32_t B, n_kblocks, kparts;
    float *W_enc, *W_cls;        // apply: updated in place
    float *m_enc, *v_enc, *m_cls, *v_cls;
    float tstep;
    AdamHyper h;
    int32_t apply;
    float *grad_out;             // [2 E + E K]: dW_cls | dW_enc, or null
    uint32_t *tickets;           // [tiles] arrival counters, zero between launches
    float *partials;             // [tiles][kparts][256]
    const float *tile_loss;
    int32_t n_loss_tiles;
    float *out_loss;             // the batch's mean loss
};

__global__ void __launch_bounds__(BT_THREADS) baseline_wgrad_adam_kernel(const BaselineWgrad a) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    __shared__ float red[4][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K, E = a.E, ne = E / 16, nk = (K + 15) / 16;
    const int KP = a.kparts;
    const int n_tiles = bt_tiles(K, E);
    if ((int)blockIdx.x == n_tiles * KP) {
        // ---- the batch's loss: the tiles' sums in tile order, one division ----
        float acc = 0.f;
        for (int base = 0; base < a.n_loss_tiles; base += BT_THREADS) {
            const int i = base + tid;
            red[0][tid] = a.tile_loss[i < a.n_loss_tiles ? i : a.n_loss_tiles - 1];
            __syncthreads();
            if (tid == 0) {
                const int cnt = a.n_loss_tiles - base < BT_THREADS ? a.n_loss_tiles - base : BT_THREADS;
                for (int j = 0; j < cnt; ++j) acc += red[0][j];
            }
            __syncthreads();
        }
        if (tid == 0) a.out_loss[0] = acc / (float)a.B;
        return;
    }
    const int tile = (int)blockIdx.x / KP, kp = (int)blockIdx.x - tile * KP;
    // ---- which tile (workgroup-uniform): section 0 dW_cls = dlogits h^T, section 1 dW_enc = dpre z^T ----
    const int r_h = K, r_dpre = K + E, r_dlog = K + 2 * E;
    int sec, m0, n0;
    if (tile < ne) { sec = 0; m0 = 0; n0 = 16 * tile; }
    else { sec = 1; m0 = 16 * ((tile - ne) / nk); n0 = 16 * ((tile - ne) % nk); }
    const int M = sec == 0 ? 2 : E, N = sec == 0 ? E : K;
    // the parameter of thread (row, col) of the tile, its optimizer state requested up front
    const int orow = tid >> 4, ocol = tid & 15;
    const int pm = m0 + orow, pn = n0 + ocol;
    const bool pok = pm < M && pn < N;
    const int64_t pidx = (int64_t)pm * N + pn;
    float *theta = sec == 0 ? a.W_cls : a.W_enc, *mom = sec == 0 ? a.m_cls : a.m_enc, *var = sec == 0 ? a.v_cls : a.v_enc;
    float p_old = 0.f, m_old = 0.f, v_old = 0.f;
    if (pok && a.apply) {
        p_old = theta[pidx];
        m_old = mom[pidx];
        v_old = var[pidx];
    }
    // ---- operand rows of this lane (clamped: every load is unconditional; rows / columns beyond the matrix only feed outputs
    //      that are never stored) ----
    const int lr = lane & 15, kq = lane >> 4;
    const int am = m0 + lr < M ? m0 + lr : M - 1;
    const int bn = n0 + lr < N ? n0 + lr : N - 1;
    const int arow = sec == 0 ? r_dlog + am : r_dpre + am;
    const int brow = sec == 0 ? r_h + bn : bn;
    const float *__restrict__ ap = a.acts + (size_t)arow * a.ld + 4 * kq;
    const float *__restrict__ bp = a.acts + (size_t)brow * a.ld + 4 * kq;
    // this wave's blocks: part kp of the batch's blocks, a quarter of that per wave
    const int nkb = a.n_kblocks;
    const int pp = (nkb + KP - 1) / KP, p_lo = kp * pp < nkb ? kp * pp : nkb, p_hi = p_lo + pp < nkb ? p_lo + pp : nkb;
    const int per = (p_hi - p_lo + 3) >> 2;
    const int u_lo = p_lo + wave * per < p_hi ? p_lo + wave * per : p_hi;
    const int u_hi = u_lo + per < p_hi ? u_lo + per : p_hi;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int u0 = u_lo; u0 < u_hi; u0 += BT_NB) {
        f4 av[BT_NB], bv[BT_NB];
#pragma unroll
        for (int j = 0; j < BT_NB; ++j) {
            const int u = u0 + j < u_hi ? u0 + j : u_hi - 1;           // (u_lo < u_hi here: a block of this wave's own range)
            av[j] = *reinterpret_cast<const f4 *>(ap + 16 * u);
            bv[j] = *reinterpret_cast<const f4 *>(bp + 16 * u);
        }
#pragma unroll
        for (int j = 0; j < BT_NB; ++j) {
            if (u0 + j >= u_hi) break;                                 // (wave-uniform)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].x, bv[j].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].y, bv[j].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].z, bv[j].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].w, bv[j].w, acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave][(4 * kq + i) * 16 + lr] = acc[i];
    __syncthreads();
    float g = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    if (KP > 1) {
        // this part's tile -> its slot (write-through: another workgroup of this launch reads it), then the tile's ticket; the
        // part that arrives last adds the parts up in part order (whichever it is: the sum's order is fixed) and goes on
        float *slot = a.partials + ((size_t)tile * KP + kp) * 256;
        __hip_atomic_store(slot + tid, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                               // every thread's store is complete
        int *flag = reinterpret_cast<int *>(&red[0][0]);               // (the waves' tiles have been read)
        if (tid == 0) flag[0] = __hip_atomic_fetch_add(a.tickets + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)KP - 1u;
        __syncthreads();
        if (!flag[0]) return;
        if (tid == 0) __hip_atomic_store(a.tickets + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float *base = a.partials + (size_t)tile * KP * 256 + tid;
        float x[BT_MAX_PARTS];
#pragma unroll
        for (int q = 0; q < BT_MAX_PARTS; ++q) x[q] = __hip_atomic_load(base + (size_t)(q < KP ? q : KP - 1) * 256, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        g = x[0];
#pragma unroll
        for (int q = 1; q < BT_MAX_PARTS; ++q) g = q < KP ? g + x[q] : g;
    }
    if (!pok) return;
    if (a.grad_out) a.grad_out[(sec == 0 ? 0 : 2 * (int64_t)E) + pidx] = g;
    if (!a.apply) return;
    float mi, vi;
    const float p_new = adam_update(p_old, m_old, v_old, g, a.tstep, a.h, mi, vi);     // torch.optim.Adam, coupled weight decay
    mom[pidx] = mi;
    var[pidx] = vi;
    theta[pidx] = p_new;
}

// the call's workspace: [agg | queue | counter: baseline_carve] | acts [rows][ld] | tile_loss [ld / 16] | tickets [tiles] |
// partials [tiles][parts][256].  A function of batch_rows, the table's widths and the model's shape only.
struct BaselineTrainCarve {
    BaselineCarve head;
    int64_t acts, tile_loss, tickets, partials, total;
    int32_t ld;
};
static int baseline_train_carve(const pcg_graph_desc *g, const pcg_baseline_model *m, int32_t batch_rows, BaselineTrainCarve &c) {
    const int rc = baseline_carve(g, m, batch_rows, c.head);
    if (rc != PCG_OK) return rc;
    const int K = baseline_K(g->feat_dim, m->concat_self != 0), E = m->emb;
    const int64_t ld = ((int64_t)batch_rows + 15) / 16 * 16;
    if (ld >= (1ll << 31)) return PCG_E_ARG;
    c.ld = (int32_t)ld;
    const int tiles = bt_tiles(K, E);
    int64_t off = c.head.total;
    c.acts = off;
    off += align256(4 * (int64_t)bt_act_rows(K, E) * ld);
    c.tile_loss = off;
    off += align256(4 * (ld / 16));
    c.tickets = off;
    off += align256(4 * (int64_t)tiles);
    c.partials = off;
    const int parts = bt_kparts((int)(ld / 16));
    off += parts > 1 ? align256(4 * (int64_t)tiles * parts * 256) : 0;
    c.total = off;
    return PCG_OK;
}

template <bool WLDS>
static int launch_baseline_train_dense(const BaselineTrainDense &a, size_t smem, hipStream_t st) {
    if (allow_dynamic_lds(baseline_train_dense_kernel<WLDS>, 160 * 1024) != PCG_OK) return PCG_E_LAUNCH;
    const int n_tiles = (int)(((int64_t)a.d.B + TB - 1) / TB);
    hipLaunchKernelGGL(baseline_train_dense_kernel<WLDS>, dim3(baseline_dense_grid(n_tiles, smem)), dim3(BL_DENSE_THREADS), smem, st, a,
                       n_tiles);
    PCG_LAUNCH_CHECK();
    return PCG_OK;
}

}  // namespace pcg

extern "C" {

int64_t pcg_baseline_train_workspace_bytes(const pcg_graph_desc *g, const pcg_baseline_model *m, int32_t batch_rows) {
    pcg::BaselineTrainCarve c;
    const int rc = pcg::baseline_train_carve(g, m, batch_rows, c);
    return rc != PCG_OK ? rc : c.total;
}

int pcg_baseline_train(const pcg_graph_desc *g, const pcg_baseline_model *m, const pcg_baseline_opt *opt, const int32_t *ids,
                       const int32_t *labels, int32_t n, int32_t batch_rows, void *workspace, int64_t workspace_bytes, float *out_loss,
                       float *grad_out, uint32_t *status, void *stream) {
    if (!opt || !ids || !labels || !workspace || !status || !out_loss || n < 0 || batch_rows < 1 || !pcg::baseline_args_ok(g, m))
        return PCG_E_ARG;
    if (opt->apply) {
        if (!opt->m_enc || !opt->v_enc || !opt->m_cls || !opt->v_cls || opt->first_step < 1) return PCG_E_ARG;
    } else if (!grad_out || n > batch_rows) return PCG_E_ARG;
    pcg::BaselineTrainCarve c;
    const int rc = pcg::baseline_train_carve(g, m, batch_rows, c);
    if (rc != PCG_OK) return rc;
    const int F = g->feat_dim, E = m->emb, concat = m->concat_self != 0, K = pcg::baseline_K(F, concat);
    const bool wlds = pcg::baseline_wlds(F, E, concat);
    const size_t smem = pcg::baseline_smem_bytes(F, E, concat, wlds);
    if (smem > 160 * 1024) return PCG_E_UNSUPPORTED;
    if (workspace_bytes < c.total || (reinterpret_cast<uintptr_t>(workspace) & 15u) != 0) return PCG_E_ARG;
    if (n == 0) return PCG_OK;

    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    pcg::BaselineAgg a;
    pcg::BaselineTrainDense t;
    pcg::baseline_fill(g, m, reinterpret_cast<float *>(ws + c.head.agg), reinterpret_cast<int32_t *>(ws + c.head.queue),
                       reinterpret_cast<uint32_t *>(ws + c.head.counter), status, a, t.d);
    t.acts = reinterpret_cast<float *>(ws + c.acts);
    t.ld = c.ld;
    t.tile_loss = reinterpret_cast<float *>(ws + c.tile_loss);
    t.status = status;
    pcg::BaselineWgrad w;
    w.acts = t.acts;
    w.ld = c.ld;
    w.K = K;
    w.E = E;
    w.W_enc = const_cast<float *>(m->W_enc);
    w.W_cls = const_cast<float *>(m->W_cls);
    w.m_enc = opt->m_enc;
    w.v_enc = opt->v_enc;
    w.m_cls = opt->m_cls;
    w.v_cls = opt->v_cls;
    w.h = pcg::adam_hyper(opt->hyper);
    w.apply = opt->apply != 0;
    w.grad_out = grad_out;
    w.tickets = reinterpret_cast<uint32_t *>(ws + c.tickets);
    w.partials = reinterpret_cast<float *>(ws + c.partials);
    w.tile_loss = t.tile_loss;
    const int tiles = pcg::bt_tiles(K, E);
    if (hipMemsetAsync(w.tickets, 0, sizeof(uint32_t) * (size_t)tiles, st) != hipSuccess) return PCG_E_LAUNCH;
    int64_t batch = 0;
    for (int64_t off = 0; off < n; off += batch_rows, ++batch) {
        const int32_t B = (int32_t)(n - off < batch_rows ? n - off : batch_rows);
        a.ids = t.d.ids = ids + off;
        a.B = t.d.B = B;
        t.labels = labels + off;
        t.inv_B = 1.f / (float)B;
        const int rc1 = pcg::launch_baseline_agg(a, st);
        if (rc1 != PCG_OK) return rc1;
        const int rc2 = wlds ? pcg::launch_baseline_train_dense<true>(t, smem, st) : pcg::launch_baseline_train_dense<false>(t, smem, st);
        if (rc2 != PCG_OK) return rc2;
        w.B = B;
        w.n_kblocks = (B + 15) / 16;
        w.kparts = pcg::bt_kparts(w.n_kblocks);
        w.n_loss_tiles = w.n_kblocks;
        w.tstep = (float)(opt->first_step + batch);
        w.out_loss = out_loss + batch;
        hipLaunchKernelGGL(pcg::baseline_wgrad_adam_kernel, dim3((unsigned)(tiles * w.kparts + 1)), dim3(pcg::BT_THREADS), 0, st, w);
        PCG_LAUNCH_CHECK();
    }
    return PCG_OK;
}

}  // extern "C"
