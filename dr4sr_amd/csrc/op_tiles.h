// op_tiles.h — device helpers of the stateless dense-tensor ops (layer_op.hip, fmlp_op.hip): one 256-thread workgroup per sequence, the
// sequence's [64][ld] activation tiles in LDS (zero rows behind L), transposed-A MFMA products for the weight gradients, per-workgroup
// partial slots written with wput (first sequence stores, later ones add).  Above the tile helpers: the row passes of the post-norm
// residual blocks, the FFN block both layers end with (ffn_fwd / ffn_ln_bwd; the activation dropout that only the encoder layer has is
// the template parameter ACT_DROP), the slot reduction over a table of destinations, and the host checks the entry points share.
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
__device__ __forceinline__ float4 ln_apply(float4 u, float mean, float rstd, float4 gm, float4 bt) {
    return make_float4((u.x - mean) * rstd * gm.x + bt.x, (u.y - mean) * rstd * gm.y + bt.y, (u.z - mean) * rstd * gm.z + bt.z,
                       (u.w - mean) * rstd * gm.w + bt.w);
}

// The row passes below give a row to 16 lanes (lane j16 takes the float4 at columns 4 j16 + 64 j, j < D / 64).  A dropout site of a
// sequence is (rk, drop, site, t0): element (row, c) of its [L][W] tensor is Philox element (t0 + row) * W + c, t0 = b * L.

// u = res + drop(o) -> sv_u (global [L][D], may be null); dst[row] = LN(u) for rows [0, L).  res and o are LDS tiles of row stride ld;
// dst has row stride ldd (an LDS tile, which may be res itself, or global y)
template <int D>
__device__ __forceinline__ void res_drop_ln_rows(float* dst, int ldd, const float* res, const float* o, int ld, const float* gam,
                                                 const float* bet, float* sv_u, const RngKey& rk, bool drop, uint32_t site,
                                                 uint64_t t0, int L, float eps) {
    constexpr int NV = D / 64;
    for (int row = threadIdx.x >> 4; row < L; row += 16) {
        const int j16 = threadIdx.x & 15;
        float4 u[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = 4 * j16 + 64 * j;
            float4 ov = ld4(o + row * ld + c);
            if (drop) ov = mul4(ov, drop4(rk, site, (t0 + row) * D + c));
            u[j] = add4(ld4(res + row * ld + c), ov);
            if (sv_u) st4(sv_u + (size_t)row * D + c, u[j]);
        }
        float mean, rstd;
        ln_stats16<NV>(u, mean, rstd, eps);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = 4 * j16 + 64 * j;
            st4(dst + (size_t)row * ldd + c, ln_apply(u[j], mean, rstd, ld4(gam + c), ld4(bet + c)));
        }
    }
}
// LayerNorm backward of all 64 rows: dZ (upstream gradient) := du, U (the LayerNorm input) := du * mask; du of rows [0, L) also to
// dres (global [L][D]) unless null
template <int D>
__device__ __forceinline__ void ln_bwd_rows(float* dZ, float* U, int ld, const float* st, const float* gam, float* dres,
                                            const RngKey& rk, bool drop, uint32_t site, uint64_t t0, int L) {
    constexpr int NV = D / 64;
    for (int row = threadIdx.x >> 4; row < 64; row += 16) {
        const int j16 = threadIdx.x & 15;
        float4 dz[NV], u[NV], gm[NV], dg[NV], db[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = 4 * j16 + 64 * j;
            dz[j] = ld4(dZ + row * ld + c); u[j] = ld4(U + row * ld + c); gm[j] = ld4(gam + c);
            dg[j] = db[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        ln_bwd_row<NV>(dz, u, st[2 * row], st[2 * row + 1], gm, dg, db);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = 4 * j16 + 64 * j;
            st4(dZ + row * ld + c, dz[j]);
            if (dres && row < L) st4(dres + (size_t)row * D + c, dz[j]);
            float4 dv = dz[j];
            if (drop && row < L) dv = mul4(dv, drop4(rk, site, (t0 + row) * D + c));
            st4(U + row * ld + c, dv);
        }
    }
}
// dst := LN(u) of the saved rows u (global [L][D]; zero rows behind L), st[row] := (mean, rstd)
template <int D>
__device__ __forceinline__ void ln_recompute_rows(float* dst, int ld, const float* sv_u, float* st, const float* gam,
                                                  const float* bet, int L, float eps) {
    constexpr int NV = D / 64;
    for (int row = threadIdx.x >> 4; row < 64; row += 16) {
        const int j16 = threadIdx.x & 15;
        float4 u[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) u[j] = row < L ? ld4(sv_u + (size_t)row * D + 4 * j16 + 64 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
        float mean, rstd;
        ln_stats16<NV>(u, mean, rstd, eps);
        if (j16 == 0) { st[2 * row] = row < L ? mean : 0.f; st[2 * row + 1] = row < L ? rstd : 0.f; }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = 4 * j16 + 64 * j;
            float4 yv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < L) yv = ln_apply(u[j], mean, rstd, ld4(gam + c), ld4(bet + c));
            st4(dst + row * ld + c, yv);
        }
    }
}
// dst [64][F] tile := gelu(src) (GRAD: gelu'(src)) of rows [0, L), times the activation-dropout mask if ACT_DROP; zero rows behind L.
// src (row stride lds_) is the LDS tile itself in the forward, the saved pre-activation in the backward; save (global [L][F]) takes the
// rows of src unless null
template <int F, bool GRAD, bool ACT_DROP>
__device__ __forceinline__ void gelu_sweep(float* dst, int ldd, const float* src, int lds_, float* save, const RngKey& rk, bool drop,
                                           uint32_t site, uint64_t t0, int L) {
    for (int i = threadIdx.x; i < 64 * (F / 4); i += 256) {
        const int row = i / (F / 4), c = (i % (F / 4)) * 4;
        float4 hv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < L) {
            hv = ld4(src + (size_t)row * lds_ + c);
            if (save) st4(save + (size_t)row * F + c, hv);
            hv = GRAD ? make_float4(gelu_erf_grad(hv.x), gelu_erf_grad(hv.y), gelu_erf_grad(hv.z), gelu_erf_grad(hv.w))
                      : make_float4(gelu_erf(hv.x), gelu_erf(hv.y), gelu_erf(hv.z), gelu_erf(hv.w));
            if (ACT_DROP && drop) hv = mul4(hv, drop4(rk, site, (t0 + row) * F + c));
        }
        st4(dst + row * ldd + c, hv);
    }
}
// op(row, col, value) for each accumulator of this lane: the 32x32 C layout of acc_to_lds.  Hand it a lambda that captures BY VALUE:
// with [&] the LDS read-modify-writes below no longer pair into ds_read2 / ds_write2 (FMLP backward launches 0.2419 ms against 0.2394)
template <int NTW, class Op>
__device__ __forceinline__ void acc_each(const f32x16 (&acc)[NTW], Op op) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, g = lane >> 5, rh = w & 1, cg = w >> 1;
#pragma unroll
    for (int i = 0; i < NTW; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) op(rh * 32 + (q & 3) + 8 * (q >> 2) + 4 * g, (cg + 2 * i) * 32 + r, acc[i][q]);
}

// ------------------------------------------------------------------------------------------------------------------ the FFN block
// The second half of a layer, y = LN(x1 + drop_FFN(dense_2(drop_ACT(gelu_erf(dense_1(x1)))))), on the tiles As [64][ldx] (x1),
// Bs [64][ldx], R [64][ldf].  ACT_DROP: the activation dropout exists (the encoder layer has it, FMLP does not).
struct FfnWeights {     // dense 1, dense 2, the closing LayerNorm; ln0: the LayerNorm that produced x1 (the backward recomputes x1)
    const float *w1, *b1, *w2, *b2, *ln_w, *ln_b, *ln0_w, *ln0_b;
};
struct FfnGrads { float *w1, *b1, *w2, *b2, *ln_w, *ln_b; };      // their places in this workgroup's slot

// x1 in As -> y rows [0, L) (global [L][D]); saves the pre-activation and the closing LayerNorm's input (sv_h, sv_u2: both or neither
// null).  Leaves x1 in As; the caller's barrier closes the sequence.
template <int D, int F, bool ACT_DROP>
__device__ __forceinline__ void ffn_fwd(float* As, float* Bs, int ldx, float* R, int ldf, const FfnWeights& w, float* sv_h, float* sv_u2,
                                        float* y, const RngKey& rk, bool drop, uint32_t s_act, uint32_t s_ffn, uint64_t t0, int L, float eps) {
    {
        f32x16 acc[F / 64];
        acc_zero(acc);
        mma_64xN<D, F / 64>(As, ldx, w.w1, acc);
        acc_to_lds<F / 64>(acc, R, ldf, w.b1);
    }
    __syncthreads();
    gelu_sweep<F, false, ACT_DROP>(R, ldf, R, ldf, sv_h, rk, drop, s_act, t0, L);
    __syncthreads();
    {
        f32x16 acc[D / 64];
        acc_zero(acc);
        mma_64xN<F, D / 64>(R, ldf, w.w2, acc);
        acc_to_lds<D / 64>(acc, Bs, ldx, w.b2);
    }
    __syncthreads();
    res_drop_ln_rows<D>(y, D, As, Bs, ldx, w.ln_w, w.ln_b, sv_u2, rk, drop, s_ffn, t0, L, eps);
}
// dy rows (global [L][D]) -> d x1 in As (every branch summed), x1 in Bs, the statistics of the closing LayerNorm in st2 and of ln0 in
// st1 (u_in: ln0's saved input); the six weight-gradient partials go to g by wput.  The caller's barrier follows.
template <int D, int F, bool ACT_DROP>
__device__ __forceinline__ void ffn_ln_bwd(float* As, float* Bs, int ldx, float* R, int ldf, float* st1, float* st2, const FfnWeights& w,
                                           const float* u_in, const float* sv_h, const float* sv_u2, const float* dy, const FfnGrads& g,
                                           const RngKey& rk, bool drop, uint32_t s_act, uint32_t s_ffn, uint64_t t0, int L, float eps,
                                           bool first) {
    load_rows<D>(As, ldx, dy, D, L);
    load_rows<D>(Bs, ldx, sv_u2, D, L);
    __syncthreads();
    ln_stats_rows<D>(Bs, ldx, st2, L, eps);
    __syncthreads();
    ln_affine_grads<D>(g.ln_w, g.ln_b, As, Bs, ldx, st2, L, first);
    __syncthreads();
    ln_bwd_rows<D>(As, Bs, ldx, st2, w.ln_w, nullptr, rk, drop, s_ffn, t0, L);         // du2 -> As, d f2 = du2 * mask -> Bs
    gelu_sweep<F, false, ACT_DROP>(R, ldf, sv_h, F, nullptr, rk, drop, s_act, t0, L);  // hd = drop(gelu(hpre)) -> R
    __syncthreads();
    wgrad_tn<D, F>(g.w2, F, Bs, ldx, R, ldf, first);
    colsum(g.b2, Bs, ldx, D, L, first);
    __syncthreads();
    // R := d hd / d hpre factor = mask * gelu'(hpre); then d hpre = (d f2 W2) * R in place
    gelu_sweep<F, true, ACT_DROP>(R, ldf, sv_h, F, nullptr, rk, drop, s_act, t0, L);
    {
        f32x16 acc[F / 64];
        acc_zero(acc);
        mma_wT<D, F / 64>(Bs, ldx, w.w2, F, acc);
        __syncthreads();                                       // the factor is in R, every wave is done reading d f2 from Bs
        acc_each(acc, [=](int row, int col, float v) { float* pp = R + row * ldf + col; *pp *= v; });
    }
    ln_recompute_rows<D>(Bs, ldx, u_in, st1, w.ln0_w, w.ln0_b, L, eps);                // x1 -> Bs, statistics -> st1
    __syncthreads();
    wgrad_tn<F, D>(g.w1, D, R, ldf, Bs, ldx, first);
    colsum(g.b1, R, ldf, F, L, first);
    {
        f32x16 acc[D / 64];
        acc_zero(acc);
        mma_wT<F, D / 64>(R, ldf, w.w1, D, acc);
        acc_each(acc, [=](int row, int col, float v) { float* pp = As + row * ldx + col; *pp += v; });   // d x1 = d hpre W1 + du2
    }
}

// ------------------------------------------------------------------------------------------------------------------ row-indirect variants
// The same passes for a tile whose rows are tokens of SEVERAL sequences (layer_packed.hip): tok (LDS, 64 ints) is the row table, tok[row] =
// b * L + pos of the token in row < n, n the tile's fill; rows behind n are zero.  Global [B L][ldg] tensors are addressed by tok[row] where
// the passes above use t0 + row, and so is every dropout element: a token draws what it draws in a tile of its own.
template <int W>
__device__ __forceinline__ void load_rows_ix(float* __restrict__ dst, int ld, const float* __restrict__ src, int ldg, const int* __restrict__ tok,
                                             int n) {
    constexpr int C4 = W / 4;
    for (int i = threadIdx.x; i < 64 * C4; i += 256) {
        const int row = i / C4, c = (i % C4) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < n) v = ld4(src + (size_t)tok[row] * ldg + c);
        st4(dst + row * ld + c, v);
    }
}
// LDS [64][ld] rows [0, n), W columns -> global [B L][ldg] (dst points at the first column)
template <int W>
__device__ __forceinline__ void store_rows_ix(float* __restrict__ dst, int ldg, const float* __restrict__ src, int ld, const int* __restrict__ tok,
                                              int n) {
    constexpr int C4 = W / 4;
    for (int i = threadIdx.x; i < n * C4; i += 256) {
        const int row = i / C4, c = (i % C4) * 4;
        st4(dst + (size_t)tok[row] * ldg + c, ld4(src + row * ld + c));
    }
}
// res_drop_ln_rows; sv_u is global [B L][D]; dst is an LDS tile of row stride ldd, or with GLOBAL_DST global [B L][D]
template <int D, bool GLOBAL_DST>
__device__ __forceinline__ void res_drop_ln_rows_ix(float* dst, int ldd, const float* res, const float* o, int ld, const float* gam,
                                                    const float* bet, float* sv_u, const RngKey& rk, bool drop, uint32_t site,
                                                    const int* tok, int n, float eps) {
    constexpr int NV = D / 64;
    for (int row = threadIdx.x >> 4; row < n; row += 16) {
        const int j16 = threadIdx.x & 15;
        const uint64_t t = (uint64_t)tok[row];
        float4 u[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = 4 * j16 + 64 * j;
            float4 ov = ld4(o + row * ld + c);
            if (drop) ov = mul4(ov, drop4(rk, site, t * D + c));
            u[j] = add4(ld4(res + row * ld + c), ov);
            if (sv_u) st4(sv_u + t * D + c, u[j]);
        }
        float mean, rstd;
        ln_stats16<NV>(u, mean, rstd, eps);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = 4 * j16 + 64 * j;
            float* d = GLOBAL_DST ? dst + t * D + c : dst + (size_t)row * ldd + c;
            st4(d, ln_apply(u[j], mean, rstd, ld4(gam + c), ld4(bet + c)));
        }
    }
}
// ln_bwd_rows; dres is global [B L][D] or null
template <int D>
__device__ __forceinline__ void ln_bwd_rows_ix(float* dZ, float* U, int ld, const float* st, const float* gam, float* dres,
                                               const RngKey& rk, bool drop, uint32_t site, const int* tok, int n) {
    constexpr int NV = D / 64;
    for (int row = threadIdx.x >> 4; row < 64; row += 16) {
        const int j16 = threadIdx.x & 15;
        const uint64_t t = row < n ? (uint64_t)tok[row] : 0;
        float4 dz[NV], u[NV], gm[NV], dg[NV], db[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = 4 * j16 + 64 * j;
            dz[j] = ld4(dZ + row * ld + c); u[j] = ld4(U + row * ld + c); gm[j] = ld4(gam + c);
            dg[j] = db[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        ln_bwd_row<NV>(dz, u, st[2 * row], st[2 * row + 1], gm, dg, db);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = 4 * j16 + 64 * j;
            st4(dZ + row * ld + c, dz[j]);
            if (dres && row < n) st4(dres + t * D + c, dz[j]);
            float4 dv = dz[j];
            if (drop && row < n) dv = mul4(dv, drop4(rk, site, t * D + c));
            st4(U + row * ld + c, dv);
        }
    }
}
// ln_recompute_rows; sv_u is global [B L][D]
template <int D>
__device__ __forceinline__ void ln_recompute_rows_ix(float* dst, int ld, const float* sv_u, float* st, const float* gam, const float* bet,
                                                     const int* tok, int n, float eps) {
    constexpr int NV = D / 64;
    for (int row = threadIdx.x >> 4; row < 64; row += 16) {
        const int j16 = threadIdx.x & 15;
        float4 u[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) u[j] = row < n ? ld4(sv_u + (size_t)tok[row] * D + 4 * j16 + 64 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
        float mean, rstd;
        ln_stats16<NV>(u, mean, rstd, eps);
        if (j16 == 0) { st[2 * row] = row < n ? mean : 0.f; st[2 * row + 1] = row < n ? rstd : 0.f; }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = 4 * j16 + 64 * j;
            float4 yv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < n) yv = ln_apply(u[j], mean, rstd, ld4(gam + c), ld4(bet + c));
            st4(dst + row * ld + c, yv);
        }
    }
}
// gelu_sweep; src is the LDS tile itself (row stride lds_), or with GLOBAL_SRC the saved pre-activation, global [B L][F]; save is
// global [B L][F] or null
template <int F, bool GRAD, bool ACT_DROP, bool GLOBAL_SRC>
__device__ __forceinline__ void gelu_sweep_ix(float* dst, int ldd, const float* src, int lds_, float* save, const RngKey& rk, bool drop,
                                              uint32_t site, const int* tok, int n) {
    for (int i = threadIdx.x; i < 64 * (F / 4); i += 256) {
        const int row = i / (F / 4), c = (i % (F / 4)) * 4;
        float4 hv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < n) {
            const uint64_t t = (uint64_t)tok[row];
            hv = ld4(GLOBAL_SRC ? src + t * F + c : src + (size_t)row * lds_ + c);
            if (save) st4(save + t * F + c, hv);
            hv = GRAD ? make_float4(gelu_erf_grad(hv.x), gelu_erf_grad(hv.y), gelu_erf_grad(hv.z), gelu_erf_grad(hv.w))
                      : make_float4(gelu_erf(hv.x), gelu_erf(hv.y), gelu_erf(hv.z), gelu_erf(hv.w));
            if (ACT_DROP && drop) hv = mul4(hv, drop4(rk, site, t * F + c));
        }
        st4(dst + row * ldd + c, hv);
    }
}
// ffn_fwd; y, sv_h and sv_u2 are the whole global tensors ([B L][D], [B L][F], [B L][D])
template <int D, int F, bool ACT_DROP>
__device__ __forceinline__ void ffn_fwd_ix(float* As, float* Bs, int ldx, float* R, int ldf, const FfnWeights& w, float* sv_h, float* sv_u2,
                                           float* y, const RngKey& rk, bool drop, uint32_t s_act, uint32_t s_ffn, const int* tok, int n,
                                           float eps) {
    {
        f32x16 acc[F / 64];
        acc_zero(acc);
        mma_64xN<D, F / 64>(As, ldx, w.w1, acc);
        acc_to_lds<F / 64>(acc, R, ldf, w.b1);
    }
    __syncthreads();
    gelu_sweep_ix<F, false, ACT_DROP, false>(R, ldf, R, ldf, sv_h, rk, drop, s_act, tok, n);
    __syncthreads();
    {
        f32x16 acc[D / 64];
        acc_zero(acc);
        mma_64xN<F, D / 64>(R, ldf, w.w2, acc);
        acc_to_lds<D / 64>(acc, Bs, ldx, w.b2);
    }
    __syncthreads();
    res_drop_ln_rows_ix<D, true>(y, D, As, Bs, ldx, w.ln_w, w.ln_b, sv_u2, rk, drop, s_ffn, tok, n, eps);
}
// ffn_ln_bwd; dy, u_in, sv_h and sv_u2 are the whole global tensors
template <int D, int F, bool ACT_DROP>
__device__ __forceinline__ void ffn_ln_bwd_ix(float* As, float* Bs, int ldx, float* R, int ldf, float* st1, float* st2, const FfnWeights& w,
                                              const float* u_in, const float* sv_h, const float* sv_u2, const float* dy, const FfnGrads& g,
                                              const RngKey& rk, bool drop, uint32_t s_act, uint32_t s_ffn, const int* tok, int n, float eps,
                                              bool first) {
    load_rows_ix<D>(As, ldx, dy, D, tok, n);
    load_rows_ix<D>(Bs, ldx, sv_u2, D, tok, n);
    __syncthreads();
    ln_stats_rows<D>(Bs, ldx, st2, n, eps);
    __syncthreads();
    ln_affine_grads<D>(g.ln_w, g.ln_b, As, Bs, ldx, st2, n, first);
    __syncthreads();
    ln_bwd_rows_ix<D>(As, Bs, ldx, st2, w.ln_w, nullptr, rk, drop, s_ffn, tok, n);                      // du2 -> As, d f2 = du2 * mask -> Bs
    gelu_sweep_ix<F, false, ACT_DROP, true>(R, ldf, sv_h, F, nullptr, rk, drop, s_act, tok, n);         // hd = drop(gelu(hpre)) -> R
    __syncthreads();
    wgrad_tn<D, F>(g.w2, F, Bs, ldx, R, ldf, first);
    colsum(g.b2, Bs, ldx, D, n, first);
    __syncthreads();
    gelu_sweep_ix<F, true, ACT_DROP, true>(R, ldf, sv_h, F, nullptr, rk, drop, s_act, tok, n);
    {
        f32x16 acc[F / 64];
        acc_zero(acc);
        mma_wT<D, F / 64>(Bs, ldx, w.w2, F, acc);
        __syncthreads();                                       // the factor is in R, every wave is done reading d f2 from Bs
        acc_each(acc, [=](int row, int col, float v) { float* pp = R + row * ldf + col; *pp *= v; });
    }
    ln_recompute_rows_ix<D>(Bs, ldx, u_in, st1, w.ln0_w, w.ln0_b, tok, n, eps);                         // x1 -> Bs, statistics -> st1
    __syncthreads();
    wgrad_tn<F, D>(g.w1, D, R, ldf, Bs, ldx, first);
    colsum(g.b1, R, ldf, F, n, first);
    {
        f32x16 acc[D / 64];
        acc_zero(acc);
        mma_wT<F, D / 64>(R, ldf, w.w1, D, acc);
        acc_each(acc, [=](int row, int col, float v) { float* pp = As + row * ldx + col; *pp += v; });   // d x1 = d hpre W1 + du2
    }
}

// ------------------------------------------------------------------------------------------------------------------ slot reduction
// Element e of a slot belongs to the first destination whose end lies behind it; a destination begins where the one before it ends
// (the first at `begin`).  Unused entries end where the last used one does, so end[REDUCE_MAX - 1] is the slot's end.
constexpr int REDUCE_MAX = 12;
struct ReduceTable { float* dst[REDUCE_MAX]; int end[REDUCE_MAX]; int begin; };
// the n destinations of a gradient struct's pointers p with slot offsets off[0 .. n] (off[n]: the end of the last)
static inline ReduceTable reduce_table(float* const* p, const int* off, int n) {
    ReduceTable t{};
    t.begin = off[0];
    for (int i = 0; i < REDUCE_MAX; ++i) { t.dst[i] = i < n ? p[i] : nullptr; t.end[i] = off[i < n ? i + 1 : n]; }
    return t;
}
// sums element e of the n_slots slots in index order and stores it to its destination
__device__ __forceinline__ void reduce_store(const float* __restrict__ slots, int n_slots, size_t stride, int e, const ReduceTable& t) {
    if (e >= t.end[REDUCE_MAX - 1]) return;
    const float s = det_sum(slots + e, n_slots, stride);
    float* dst = t.dst[0];
    int o = t.begin;
#pragma unroll
    for (int i = 1; i < REDUCE_MAX; ++i)
        if (e >= t.end[i - 1]) { dst = t.dst[i]; o = t.end[i - 1]; }
    dst[e - o] = s;
}
static __global__ void k_slot_reduce(const float* __restrict__ slots, int n_slots, int stride, ReduceTable t) {
    reduce_store(slots, n_slots, (size_t)stride, t.begin + blockIdx.x * blockDim.x + threadIdx.x, t);
}

// ------------------------------------------------------------------------------------------------------------------ host
constexpr int MAX_SLOTS = 256;         // workgroups (= weight-gradient partial slots) of a backward launch
static inline int n_slots(int64_t B) { return B < MAX_SLOTS ? (int)B : MAX_SLOTS; }
static inline bool layer_args_ok(int layer, float p_drop, float eps) {
    return !(layer < 0 || layer > 1024 || !(p_drop >= 0.f && p_drop < 1.f) || !(eps >= 0.f));
}
// is s there, and every one of the N pointers it consists of?
template <int N, class T>
static inline bool all_set(const T* s) {
    static_assert(sizeof(T) == N * sizeof(float*), "a struct of N pointers");
    if (!s) return false;
    const void* p[N];
    memcpy(p, s, sizeof p);
    for (int i = 0; i < N; ++i)
        if (!p[i]) return false;
    return true;
}
struct ZeroSpan { float* p; int64_t n; };
static inline int zero_fill(const ZeroSpan* t, int n, hipStream_t st) {
    for (int i = 0; i < n; ++i) {
        const int e = hip_ret(hipMemsetAsync(t[i].p, 0, t[i].n * sizeof(float), st));
        if (e) return e;
    }
    return 0;
}

}  // namespace optile
