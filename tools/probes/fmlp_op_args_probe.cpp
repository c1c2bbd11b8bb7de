// Host-side argument checking of the dr4sr_fmlp_layer_* / dr4sr_layer_norm_* entry points under the host sanitizers: a stand-alone
// program (CPU build of the host code, no GPU needed — every call below returns before its first launch).  Build and run:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I dr4sr_amd/csrc \
//         dr4sr_amd/csrc/fmlp_op.hip tools/probes/fmlp_op_args_probe.cpp -o tools/probes/fmlp_op_args_probe && tools/probes/fmlp_op_args_probe
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/dr4sr_hip.h"

void big_lds_impl(const void*, size_t) {}                  // step.hip's; never reached: no call below gets as far as a launch

static int failures = 0;
#define EXPECT(expr, want)                                                                        \
    do {                                                                                          \
        const long long got_ = (long long)(expr);                                                 \
        if (got_ != (long long)(want)) { std::printf("FAIL %s = %lld, want %lld\n", #expr, got_, (long long)(want)); ++failures; } \
    } while (0)

int main() {
    float buf[16] = {0};
    float* p = buf;                                        // any non-null pointer: nothing dereferences it on the host
    dr4sr_fmlp_layer_weights w = {p, p, p, p, p, p, p, p, p};
    dr4sr_fmlp_layer_grads g = {p, p, p, p, p, p, p, p, p};
    dr4sr_fmlp_layer_weights w_hole = w;
    w_hole.dense_2_bias = nullptr;
    for (int L = -3; L <= 70; ++L) {
        const bool ok = L >= 2 && L <= 64 && !(L & 1);
        EXPECT(dr4sr_fmlp_layer_saved_floats(3, L, 64, 256), ok ? 3LL * L * 384 : DR4SR_E_SHAPE);
        EXPECT(dr4sr_fmlp_layer_workspace_bytes(3, L, 64, 256, 0), ok ? 16384 : DR4SR_E_SHAPE);
        EXPECT(dr4sr_fmlp_layer_fwd(p, &w, 3, L, 64, 256, 1e-12f, 0.f, 1, 1, 0, p, nullptr, nullptr, 0, nullptr), ok ? DR4SR_E_WS : DR4SR_E_SHAPE);
        EXPECT(dr4sr_fmlp_layer_bwd(p, &w, 3, L, 64, 256, 1e-12f, 0.f, 1, 1, 0, p, p, p, &g, p, 16384, nullptr), ok ? DR4SR_E_WS : DR4SR_E_SHAPE);
    }
    EXPECT(dr4sr_fmlp_layer_saved_floats(3, 50, 128, 512), DR4SR_E_SHAPE);
    EXPECT(dr4sr_fmlp_layer_saved_floats(3, 50, 64, 128), DR4SR_E_SHAPE);
    EXPECT(dr4sr_fmlp_layer_saved_floats(-1, 50, 64, 256), DR4SR_E_ARG);
    EXPECT(dr4sr_fmlp_layer_saved_floats(INT64_C(1) << 40, 64, 64, 256), (INT64_C(1) << 40) * 64 * 384);
    EXPECT(dr4sr_fmlp_layer_workspace_bytes(INT64_C(1) << 40, 50, 64, 256, 1), (16384LL / 4 + 256LL * 37440) * 4);
    EXPECT(dr4sr_fmlp_layer_fwd(p, nullptr, 3, 50, 64, 256, 1e-12f, 0.f, 1, 1, 0, p, p, p, 1 << 20, nullptr), DR4SR_E_ARG);
    EXPECT(dr4sr_fmlp_layer_fwd(p, &w_hole, 3, 50, 64, 256, 1e-12f, 0.f, 1, 1, 0, p, p, p, 1 << 20, nullptr), DR4SR_E_ARG);
    EXPECT(dr4sr_fmlp_layer_fwd(nullptr, &w, 3, 50, 64, 256, 1e-12f, 0.f, 1, 1, 0, p, p, p, 1 << 20, nullptr), DR4SR_E_ARG);
    EXPECT(dr4sr_fmlp_layer_fwd(p, &w, 3, 50, 64, 256, 1e-12f, 0.f, 1, 1, 0, nullptr, p, p, 1 << 20, nullptr), DR4SR_E_ARG);
    EXPECT(dr4sr_fmlp_layer_fwd(p, &w, -1, 50, 64, 256, 1e-12f, 0.f, 1, 1, 0, p, p, p, 1 << 20, nullptr), DR4SR_E_ARG);
    EXPECT(dr4sr_fmlp_layer_fwd(p, &w, 3, 50, 64, 256, -1.f, 0.f, 1, 1, 0, p, p, p, 1 << 20, nullptr), DR4SR_E_ARG);
    EXPECT(dr4sr_fmlp_layer_fwd(p, &w, 3, 50, 64, 256, 1e-12f, 1.f, 1, 1, 0, p, p, p, 1 << 20, nullptr), DR4SR_E_ARG);
    EXPECT(dr4sr_fmlp_layer_fwd(p, &w, 3, 50, 64, 256, 1e-12f, -0.5f, 1, 1, 0, p, p, p, 1 << 20, nullptr), DR4SR_E_ARG);
    EXPECT(dr4sr_fmlp_layer_fwd(p, &w, 3, 50, 64, 256, 1e-12f, 0.f, 1, 1, 1025, p, p, p, 1 << 20, nullptr), DR4SR_E_ARG);
    EXPECT(dr4sr_fmlp_layer_fwd(p, &w, 3, 50, 64, 256, 1e-12f, 0.f, 1, 1, -1, p, p, p, 1 << 20, nullptr), DR4SR_E_ARG);
    EXPECT(dr4sr_fmlp_layer_fwd(p, &w, 3, 50, 64, 256, 1e-12f, 0.f, 1, 1, 0, p, p, p, 16383, nullptr), DR4SR_E_WS);
    EXPECT(dr4sr_fmlp_layer_fwd(nullptr, &w, 0, 50, 64, 256, 1e-12f, 0.f, 1, 1, 0, nullptr, nullptr, nullptr, 0, nullptr), 0);       // B = 0
    EXPECT(dr4sr_fmlp_layer_bwd(p, &w, 3, 50, 64, 256, 1e-12f, 0.f, 1, 1, 0, p, p, p, nullptr, p, 1 << 30, nullptr), DR4SR_E_ARG);
    EXPECT(dr4sr_fmlp_layer_bwd(p, &w, 3, 50, 64, 256, 1e-12f, 0.f, 1, 1, 0, nullptr, p, p, &g, p, 1 << 30, nullptr), DR4SR_E_ARG);
    EXPECT(dr4sr_fmlp_layer_bwd(p, &w, 3, 50, 64, 256, 1e-12f, 0.f, 1, 1, 0, p, p, p, &g, nullptr, 1 << 30, nullptr), DR4SR_E_WS);
    EXPECT(dr4sr_fmlp_layer_bwd(p, &w, 300, 50, 64, 256, 1e-12f, 0.f, 1, 1, 0, p, p, p, &g, p, (4096LL + 256LL * 37440) * 4 - 1, nullptr), DR4SR_E_WS);
    for (int D = -4; D <= 1032; ++D) {
        const bool ok = D >= 4 && D <= 1024 && !(D & 3);
        EXPECT(dr4sr_layer_norm_workspace_bytes(7, D), ok ? 2LL * 2 * D * 4 : DR4SR_E_SHAPE);
        EXPECT(dr4sr_layer_norm_fwd(nullptr, p, p, 7, D, 1e-12f, p, nullptr), ok ? DR4SR_E_ARG : DR4SR_E_SHAPE);
        EXPECT(dr4sr_layer_norm_bwd(p, p, 7, D, 1e-12f, p, p, p, p, nullptr, 0, nullptr), ok ? DR4SR_E_WS : DR4SR_E_SHAPE);
    }
    EXPECT(dr4sr_layer_norm_workspace_bytes(INT64_C(1) << 40, 64), 256LL * 2 * 64 * 4);
    EXPECT(dr4sr_layer_norm_workspace_bytes(-1, 64), DR4SR_E_ARG);
    EXPECT(dr4sr_layer_norm_fwd(p, nullptr, p, 7, 64, 1e-12f, p, nullptr), DR4SR_E_ARG);
    EXPECT(dr4sr_layer_norm_fwd(p, p, p, 7, 64, -1.f, p, nullptr), DR4SR_E_ARG);
    EXPECT(dr4sr_layer_norm_fwd(nullptr, p, p, 0, 64, 1e-12f, nullptr, nullptr), 0);
    EXPECT(dr4sr_layer_norm_bwd(p, p, 7, 64, 1e-12f, p, p, nullptr, p, p, 1 << 20, nullptr), DR4SR_E_ARG);
    EXPECT(dr4sr_layer_norm_bwd(p, p, 7, 64, 1e-12f, p, p, p, p, p, 2 * 2 * 64 * 4 - 1, nullptr), DR4SR_E_WS);
    std::printf(failures ? "%d FAILED\n" : "fmlp_op argument checks: ok\n", failures);
    return failures ? 1 : 0;
}
