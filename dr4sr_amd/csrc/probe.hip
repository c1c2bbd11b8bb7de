// probe.hip — probe entry points (include/dr4sr_hip_probes.h): device primitives run on their own, for tests/
#include "common.h"
#include "kernels.h"
#include "../../include/dr4sr_hip_probes.h"
#include "attn_tile.h"

// the DPP / permlane cross-lane primitives of common.h beside the shuffle forms, on inputs loaded straight into them
__global__ __launch_bounds__(256) void k_lane_probe(const float* __restrict__ in, const uint32_t* __restrict__ in_u, uint32_t* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;         // n is a multiple of 256 and the grid is n / 256: every thread in range
    const float v = in[i];
    const uint32_t u = in_u[i];
    auto put = [&](int q, float a, float b) { out[(2 * q) * n + i] = __float_as_uint(a); out[(2 * q + 1) * n + i] = __float_as_uint(b); };
    put(DR4SR_LP_GROUP16_SUM, lane_group_sum<16>(v), group16_sum(v));
    put(DR4SR_LP_GROUP8_SUM, group8_sum(v), group8_sum_ref(v));
    put(DR4SR_LP_WAVE_SUM, wave_sum_dpp(v), wave_sum(v));
    put(DR4SR_LP_XG_MAX, tattn::xg_max<true>(v), xrow_max_ref(v));
    put(DR4SR_LP_XG_SUM, tattn::xg_sum<true>(v), xrow_sum_ref(v));
    put(DR4SR_LP_FOLD, xrow_sum(v), xrow_sum_ref(v));
    out[(2 * DR4SR_LP_XOR1) * n + i] = lane_xor1_u32(u); out[(2 * DR4SR_LP_XOR1 + 1) * n + i] = lane_xor1_u32_ref(u);
}
extern "C" int dr4sr_lane_probe(const float* in, const uint32_t* in_u, uint32_t* out, int64_t n, void* stream) {
    if (!in || !in_u || !out || n <= 0 || (n & 255) || n > (int64_t)1 << 24) return DR4SR_E_ARG;
    hipLaunchKernelGGL(k_lane_probe, dim3((unsigned)(n / 256)), dim3(256), 0, (hipStream_t)stream, in, in_u, out, n);
    return DR4SR_LAUNCH_CHECK();
}
