// fmlp_conv.h — the sliding-window circular-convolution loop of the FMLP filter kernels (fmlp.hip, fmlp_op.hip)
#pragma once
#include "common.h"

__device__ __forceinline__ void fma4(float4& a, const float4& m, const float4& x) {
    a.x = fmaf(m.x, x.x, a.x); a.y = fmaf(m.y, x.y, a.y); a.z = fmaf(m.z, x.z, a.z); a.w = fmaf(m.w, x.w, a.w);
}

// Four CONSECUTIVE rows per thread and a sliding window: acc[i] += C(s) * V(s + off_i), off_i = i (or 3 - i), s = 0 .. S-1.  Row i at
// step s and row i -/+ 1 at step s + 1 read the same V, so a 4-slot circular register window needs ONE new value per step: 2 LDS
// reads (coefficient + new value) per 16 FMAs instead of 5 with rows 16 apart — these kernels run one wave per SIMD and were bound by
// LDS bandwidth / latency (k_fmlp_filter_fwd 14.4 us, _bwd 28.8 us at B = 256).  V and C must be safe (in bounds, any value) for s up to S + 10.
template <bool REV, class VF, class CF>
__device__ __forceinline__ void conv4(float4 (&acc)[4], const int S, VF V, CF C) {
    float4 w[4], nv[4], nc[4];
    w[0] = V(0); w[1] = V(1); w[2] = V(2);
#pragma unroll
    for (int j = 0; j < 4; ++j) { nv[j] = V(3 + j); nc[j] = C(j); }
    const int S4 = S & ~3;
    for (int s0 = 0; s0 < S4; s0 += 4) {
        float4 cv[4], cc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { cv[j] = nv[j]; cc[j] = nc[j]; }
#pragma unroll
        for (int j = 0; j < 4; ++j) { nv[j] = V(s0 + 7 + j); nc[j] = C(s0 + 4 + j); }   // the next 4 steps' reads fly over these 64 FMAs:
#pragma unroll                                                                          // one wave per SIMD hides no LDS latency itself
        for (int j = 0; j < 4; ++j) {
            w[(j + 3) & 3] = cv[j];
#pragma unroll
            for (int i = 0; i < 4; ++i) fma4(acc[i], cc[j], w[(j + (REV ? 3 - i : i)) & 3]);
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)                    // the S & 3 tail steps (their operands are already in nv / nc)
        if (S4 + j < S) {
            w[(j + 3) & 3] = nv[j];
#pragma unroll
            for (int i = 0; i < 4; ++i) fma4(acc[i], nc[j], w[(j + (REV ? 3 - i : i)) & 3]);
        }
}
