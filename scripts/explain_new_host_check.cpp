// Host-side argument checks of pcg_explain_new / pcg_explain_new_workspace_bytes under the host sanitizers: a stand-alone program
// (its own main, no Python, no GPU needed - every call below is rejected, or accepted with n == 0, before anything is enqueued).
//
//   cd pc-gnn_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -fno-gpu-rdc -Xarch_host -fsanitize=address,undefined \
//       -I../../include ../../scripts/explain_new_host_check.cpp *.hip -o /tmp/explain_new_host_check && /tmp/explain_new_host_check
//
// Prints one line per check and "ok"; a sanitizer report or a failed check ends it with a non-zero status.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pcgnn.h"

static int failures = 0;
#define CHECK(expr, want)                                                              \
    do {                                                                               \
        const long long got_ = (long long)(expr);                                      \
        const bool ok_ = got_ == (long long)(want);                                    \
        std::printf("%-4s %s -> %lld\n", ok_ ? "ok" : "FAIL", #expr, got_);            \
        failures += ok_ ? 0 : 1;                                                       \
    } while (0)

static pcg_graph_desc desc(int64_t n, int32_t feat_dim = 32, int32_t n_rel = 3, int32_t max_degree = 100) {
    pcg_graph_desc d;
    std::memset(&d, 0, sizeof d);
    d.n_nodes = n;
    d.feat_dim = feat_dim;
    d.feat_stride = (feat_dim + 3) / 4 * 4;
    d.n_rel = n_rel;
    d.max_degree = max_degree;
    return d;
}

int main() {
    const double thr[3] = {0.5, 0.5, 0.5};
    const pcg_graph_desc g = desc(1000), q = desc(10);
    float f[1];
    int32_t i32[1];
    int64_t i64[1];
    pcg_explain_out none;
    std::memset(&none, 0, sizeof none);
    pcg_explain_out attr = none, chosen = none, both = none;
    attr.logits = attr.d_self = attr.d_agg = attr.self_contrib = attr.rel_contrib = f;
    chosen.out_begin = i64;
    chosen.out_ids = i32;
    chosen.out_dist = f;
    both = attr;
    both.out_begin = i64;
    both.out_ids = i32;
    both.out_dist = f;
    both.neigh_contrib = f;
    auto call = [&](const pcg_graph_desc *gg, const pcg_graph_desc *qq, const pcg_explain_out *o, int32_t n, float w0, float w1,
                    int32_t emb = 64) {
        return pcg_explain_new(gg, qq, nullptr, emb, nullptr, n, 4, nullptr, 1, thr, nullptr, 100, w0, w1, o, nullptr, nullptr);
    };
    CHECK(call(&g, &q, nullptr, 0, 0.f, 1.f), PCG_E_ARG);                       // NULL struct
    CHECK(call(&g, &q, &none, 0, 0.f, 1.f), PCG_E_ARG);                         // no group
    pcg_explain_out half = attr;
    half.d_agg = nullptr;
    CHECK(call(&g, &q, &half, 0, 0.f, 1.f), PCG_E_ARG);                         // a half-filled attribution group
    half = both;
    half.out_dist = nullptr;
    CHECK(call(&g, &q, &half, 0, 0.f, 1.f), PCG_E_ARG);                         // a half-filled chosen group
    half = attr;
    half.neigh_contrib = f;
    CHECK(call(&g, &q, &half, 0, 0.f, 1.f), PCG_E_ARG);                         // neigh_contrib without the chosen group
    half = chosen;
    half.neigh_contrib = f;
    CHECK(call(&g, &q, &half, 0, 0.f, 1.f), PCG_E_ARG);                         // ... without the attribution group
    CHECK(call(&g, &q, &both, 0, NAN, 1.f), PCG_E_ARG);                         // non-finite weights
    CHECK(call(&g, &q, &both, 0, 0.f, INFINITY), PCG_E_ARG);
    CHECK(call(&g, &q, &both, -1, 0.f, 1.f), PCG_E_ARG);
    const pcg_graph_desc q25 = desc(10, 25), q2 = desc(10, 32, 2);
    CHECK(call(&g, &q25, &both, 0, 0.f, 1.f), PCG_E_ARG);                       // descriptors that disagree
    CHECK(call(&g, &q2, &both, 0, 0.f, 1.f), PCG_E_ARG);
    CHECK(call(nullptr, &q, &both, 0, 0.f, 1.f), PCG_E_ARG);
    CHECK(call(&g, nullptr, &both, 0, 0.f, 1.f), PCG_E_ARG);
    CHECK(call(&g, &q, &both, 0, 0.f, 1.f, 60), PCG_E_UNSUPPORTED);             // emb not a multiple of 16
    CHECK(call(&g, &q, &both, 4, 0.f, 1.f), PCG_E_ARG);                         // n > 0 with NULL tables: still before any launch
    CHECK(call(&g, &q, &both, 0, 0.f, 1.f), PCG_OK);                            // n == 0: nothing is enqueued
    CHECK(call(&g, &q, &attr, 0, -1.f, 1.f), PCG_OK);
    CHECK(call(&g, &q, &chosen, 0, 0.f, 1.f), PCG_OK);
    CHECK(pcg_explain_new_workspace_bytes(&g, &q, 64, 16, 100) == pcg_infer_new_workspace_bytes(&g, &q, 64, 16, 100), 1);
    CHECK(pcg_explain_new_workspace_bytes(&g, &q, 64, 16, 100) > 0, 1);
    CHECK(pcg_explain_new_workspace_bytes(nullptr, &q, 64, 16, 100), PCG_E_ARG);
    CHECK(pcg_explain_new_workspace_bytes(&g, &q25, 64, 16, 100), PCG_E_ARG);
    CHECK(pcg_explain_new_workspace_bytes(&g, &q, 64, 0, 100), PCG_E_ARG);
    CHECK(pcg_explain_new_workspace_bytes(&g, &q, 60, 16, 100), PCG_E_UNSUPPORTED);
    int64_t layout[16];
    CHECK(pcg_abi_layout(5, layout, 16), 10);
    CHECK(layout[0], (long long)sizeof(pcg_explain_out));
    CHECK(pcg_abi_version(), 13);
    std::printf(failures ? "%d check(s) FAILED\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
