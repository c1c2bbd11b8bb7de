// op_tiles.h — device helpers of the stateless dense-tensor ops (layer_op.hip, fmlp_op.hip): one 256-thread workgroup per sequence, the
// sequence's [64][ld] activation tiles in LDS (zero rows behind L), transposed-A MFMA products for the weight gradients, per-workgroup
// partial slots written with wput (first sequence stores, later ones add).
#pragma once
#include "common.h"

namespace optile {

// rows [0, L) of a global [L][W] matrix -> LDS [64][ld], zero rows behind L
template <int W>
__device__ __forceinline__ void load_rows(float* __restrict__ dst, int ld, const float* __restrict__ src, int lds_, int L) {
    load_tile<W>(dst, ld, src, lds_, 0, L);
}
// LDS [64][ld] rows [0, L) -> global [L][ldg]
template <int W>
__device__ __forceinline__ void store_rows(float* __restrict__ dst, int ldg, const float* __restrict__ src, int ld, int L) {
    constexpr int C4 = W / 4;
    for (int i = threadIdx.x; i < L * C4; i += 256) {
        const int row = i / C4, c = (i % C4) * 4;
        st4(dst + (size_t)row * ldg + c, ld4(src + row * ld + c));
    }
}
// C[32 x 32] = sum over the 64 rows k of A[k][r] B[k][c]: the transposed-A product of the weight gradients and of dK / dV.  A and B point at
// the tile's first column; lane (r, g) takes rows k in [32 g, 32 g + 32).  Result in the 32x32 C layout (row = (q & 3) + 8 (q >> 2) + 4 g).
__device__ __forceinline__ f32x16 mma_tn(const float* __restrict__ A, int lda, const float* __restrict__ Bm, int ldb) {
    const int lane = threadIdx.x & 63, r = lane & 31, g = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    const float* a = A + (g * 32) * lda + r;
    const float* b = Bm + (g * 32) * ldb + r;
#pragma unroll 8
    for (int k = 0; k < 32; ++k) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k * lda], b[k * ldb], acc, 0, 0, 0);
    return acc;
}
// common.h's mma_64xN_wT with the reduction loop unrolled by four float4 steps only: fully unrolled, the compiler hoists every weight load
// of the GEMM in front of the first MFMA (KR / 2 x NTW dwords per lane), which with the accumulators in flight here runs out of registers
// (1 - 2 KB of scratch per lane).  Measured, backward launches of two layers at B = 256, L = 50, d = 64 / 128: full 0.349 / 0.877 ms,
// unroll 2: 0.299 / 0.625, unroll 4: 0.278 / 0.417, unroll 8 (scratch again at d = 64): 0.325 / 0.552 (NOTEBOOK)
template <int KR, int NTW>
__device__ __forceinline__ void mma_wT(const float* __restrict__ As, int lda, const float* __restrict__ W, int ldw, f32x16 (&acc)[NTW]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = lane & 31, g = lane >> 5, rh = w & 1, cg = w >> 1;
    const float* arow = As + (rh * 32 + r) * lda + g * (KR / 2);
    const float* wcol = W + (size_t)(g * (KR / 2)) * ldw + cg * 32 + r;
#pragma unroll 4
    for (int c = 0; c < KR / 2; c += 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(arow + c);
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            const float* wp = wcol + (size_t)c * ldw + 64 * i;
            const float b0 = wp[0], b1 = wp[ldw], b2 = wp[2 * ldw], b3 = wp[3 * ldw];
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0, acc[i], 0, 0, 0);
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1, acc[i], 0, 0, 0);
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b2, acc[i], 0, 0, 0);
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b3, acc[i], 0, 0, 0);
        }
    }
}
__device__ __forceinline__ void wput(float* __restrict__ p, float v, bool first) { *p = first ? v : *p + v; }
// weight-gradient partial  out[M x N] (row stride ldo) = A^T B  over the token rows; 32x32 tiles dealt to the four waves
template <int M, int N>
__device__ __forceinline__ void wgrad_tn(float* __restrict__ out, int ldo, const float* __restrict__ A, int lda, const float* __restrict__ Bm, int ldb,
                                         bool first) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, g = lane >> 5;
    constexpr int NT = N / 32, TILES = (M / 32) * NT;
    for (int t = w; t < TILES; t += 4) {
        const int mt = t / NT, nt = t % NT;
        const f32x16 acc = mma_tn(A + mt * 32, lda, Bm + nt * 32, ldb);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int row = mt * 32 + (q & 3) + 8 * (q >> 2) + 4 * g;
            wput(out + (size_t)row * ldo + nt * 32 + r, acc[q], first);
        }
    }
}
// column sums over rows [0, L) of an LDS matrix, rows added in index order: out[c] for c < W
__device__ __forceinline__ void colsum(float* __restrict__ out, const float* __restrict__ S, int ld, int W, int L, bool first) {
    for (int c = threadIdx.x; c < W; c += 256) {
        float s = 0.f;
        for (int row = 0; row < L; ++row) s += S[row * ld + c];
        wput(out + c, s, first);
    }
}
__device__ __forceinline__ float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// LayerNorm statistics of the rows of U (16 lanes per row) -> st[row] = (mean, rstd)
template <int D>
__device__ __forceinline__ void ln_stats_rows(const float* __restrict__ U, int ld, float* __restrict__ st, int L, float eps) {
    constexpr int NV = D / 64;
    for (int row = threadIdx.x >> 4; row < 64; row += 16) {
        const int j16 = threadIdx.x & 15;
        float4 u[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) u[j] = ld4(U + row * ld + 4 * j16 + 64 * j);
        float mean, rstd;
        ln_stats16<NV>(u, mean, rstd, eps);
        if (j16 == 0) { st[2 * row] = row < L ? mean : 0.f; st[2 * row + 1] = row < L ? rstd : 0.f; }
    }
}
// d gamma[c] = sum_rows dz xhat, d beta[c] = sum_rows dz (rows in index order)
template <int D>
__device__ __forceinline__ void ln_affine_grads(float* __restrict__ dgam, float* __restrict__ dbet, const float* __restrict__ dZ,
                                                const float* __restrict__ U, int ld, const float* __restrict__ st, int L, bool first) {
    for (int c = threadIdx.x; c < D; c += 256) {
        float sg = 0.f, sb = 0.f;
        for (int row = 0; row < L; ++row) {
            const float dz = dZ[row * ld + c];
            sg += dz * (U[row * ld + c] - st[2 * row]) * st[2 * row + 1];
            sb += dz;
        }
        wput(dgam + c, sg, first);
        wput(dbet + c, sb, first);
    }
}

}  // namespace optile
