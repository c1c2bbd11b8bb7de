// fmlp_op.hip — the stateless FMLP layer op (dr4sr_fmlp_layer_fwd / _bwd) and the LayerNorm op (dr4sr_layer_norm_fwd / _bwd) on dense
// tensors: what torch.ops.dr4sr_hip.fmlp_layer / layer_norm run.  One FMLP `Layer` of the reference (module/layers.py:781-791) on [B, L, 64]:
//     f  = irfft(rfft(x, dim=1, 'ortho') * complex_weight, n=L, dim=1, 'ortho')
//     xf = LayerNorm_f(drop_FILT(f) + x)
//     y  = LayerNorm_i(drop_FFN(dense_2(gelu_erf(dense_1(xf)))) + xf)
// no plan, no device state words.  The filter is computed as fmlp.hip computes it: per feature a circular convolution with the real
// kernel m [L][64], which k_fmlp_op_coef builds from the complex weight ONCE PER CALL into the workspace (DC and Nyquist bins weighted 1,
// the others 2; the imaginary parts of DC and Nyquist contribute nothing).
//
// Work distribution: one 256-thread workgroup per sequence (b = blockIdx.x, + gridDim.x, ...).  Filter: thread (dq = tid & 15,
// rg = tid >> 4) owns the feature quad 4 dq of rows 4 rg .. 4 rg + 3 and runs fmlp_conv.h's sliding-window loop over the sequence tile
// held twice in LDS; FFN: v_mfma_f32_32x32x2_f32 through common.h's 64-row tile helpers (zero rows behind L).  LDS (floats):
//     A [64][68] | B [64][68] | R [64][260] (filter phases: X2 [2 L][64] | DY2 [2 L][64]) | m [64][64] | LayerNorm statistics [2][128]
// = 118 784 bytes of the CU's 160 KB: one workgroup per CU.
//
// The forward saves both LayerNorm inputs and the FFN pre-activation (dr4sr_fmlp_layer_saved_floats = B L (2 D + F)); the backward
// recomputes the LayerNorm statistics, xf, the GELU and the dropout masks (Philox is a pure function of (seed, step, site, element)).
// Weight gradients: every workgroup sums the sequences it owns, in that order, into its own slot of the workspace (dm [L][64] and the
// other eight tensors); a second launch adds the slots in index order and folds dm back to d complex_weight — no float atomics, the same
// bits on every call.
//
// This file holds the filter half of the layer (its first rows pass runs in the convolution's thread layout) and the LayerNorm op; the
// FFN + LayerNorm_i half, forward and backward, and the slot reduction are op_tiles.h's (shared with layer_op.hip).
#include "common.h"
#include "fmlp_conv.h"
#include "op_tiles.h"

namespace fop {
using namespace optile;

constexpr int D = 64, F = 256, LDX = D + 4, LDF = F + 4;
constexpr int M_FLOATS = 64 * D;       // the filter kernel m, L <= 64 rows
constexpr int R_FLOATS = 64 * LDF;     // >= 2 * (2 * 64) * D: X2 and DY2 of the filter phases
constexpr int LDS_FLOATS = 2 * 64 * LDX + R_FLOATS + M_FLOATS + 2 * 128;
static_assert(R_FLOATS >= 4 * 64 * D, "the doubled sequence tiles live in R");
// one slot of weight-gradient partials: dm in place of the complex weight, then the other eight tensors in the flat layout's order
constexpr int O_DM = 0, O_FLNW = O_DM + M_FLOATS, O_FLNB = O_FLNW + D, O_W1 = O_FLNB + D, O_B1 = O_W1 + F * D, O_W2 = O_B1 + F,
              O_B2 = O_W2 + D * F, O_ILNW = O_B2 + D, O_ILNB = O_ILNW + D, NW = O_ILNB + D;
constexpr int FOLD_BLOCKS = D / 4;     // blocks of the reduce launch that sum dm and fold it: four features each

#define FOP_SITE_FILT(l) (1u + 2u * (uint32_t)(l))      // fmlp.hip's FS_FILT / FS_FFN
#define FOP_SITE_FFN(l) (2u + 2u * (uint32_t)(l))

struct Args {
    const float* x; dr4sr_fmlp_layer_weights w; const float* m;
    int64_t B; int L; float eps, p; uint64_t seed; uint32_t step; int layer;
    float* y; float* saved;
    const float* dy; float* dx; float* slots;
};

__host__ __device__ inline int64_t saved_stride(int L) { return (int64_t)L * (2 * D + F); }

// m[r][d] = (1 / L) sum_k c_k (Wre[k][d] cos(2 pi k r / L) - Wim[k][d] sin(2 pi k r / L)), c_0 = c_{L/2} = 1, else 2: one output per
// thread (k_fmlp_prep's coefficient blocks in fmlp.hip, for one layer)
__global__ __launch_bounds__(256) void k_fmlp_op_coef(const float* __restrict__ cw, float* __restrict__ m, int L) {
    __shared__ float ct[64], sn[64];
    if ((int)threadIdx.x < L) sincospif(2.0f * threadIdx.x / (float)L, &sn[threadIdx.x], &ct[threadIdx.x]);
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x, K = L / 2 + 1;
    if (i >= L * D) return;
    const int r = i / D, d = i % D;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
        const int j = (k * r) % L;
        const float cf = (k == 0 || 2 * k == L) ? 1.f : 2.f;
        acc += cf * (cw[(k * D + d) * 2] * ct[j] - cw[(k * D + d) * 2 + 1] * sn[j]);
    }
    m[i] = acc / (float)L;
}

// the FFN block's view of the layer: dense_1, dense_2, the intermediate LayerNorm; the filter LayerNorm made its input
__device__ __forceinline__ FfnWeights ffn_weights(const dr4sr_fmlp_layer_weights& w) {
    return {w.dense_1_weight, w.dense_1_bias, w.dense_2_weight, w.dense_2_bias, w.inter_ln_weight, w.inter_ln_bias, w.filter_ln_weight,
            w.filter_ln_bias};
}
// the sequence tile twice: x[(l - r) mod L] = X2[l - r + L]
__device__ __forceinline__ void load_twice(float* __restrict__ X2, const float* __restrict__ xb, int L) {
    for (int i = threadIdx.x; i < L * (D / 4); i += 256) {
        const float4 v = ld4(xb + 4 * i);
        st4(X2 + 4 * i, v);
        st4(X2 + L * D + 4 * i, v);
    }
}

// =================================================================================================================== forward
__global__ __launch_bounds__(256) void k_fmlp_layer_fwd(const Args a) {
    extern __shared__ __align__(16) float lds[];
    float* As = lds;                       // xf
    float* Bs = As + 64 * LDX;             // the FFN output
    float* R = Bs + 64 * LDX;              // X2, then the FFN hidden tile
    float* ML = R + R_FLOATS;
    float* X2 = R;
    const int tid = threadIdx.x, L = a.L, dq = tid & 15, rg = tid >> 4, c = 4 * dq, l0 = 4 * rg;
    const RngKey rk = make_rng(a.seed, a.step, a.p);
    const bool drop = a.p > 0.f;
    const uint32_t s_filt = FOP_SITE_FILT(a.layer), s_ffn = FOP_SITE_FFN(a.layer);
    const int64_t SS = saved_stride(L);
    const FfnWeights fw = ffn_weights(a.w);
    for (int i = tid; i < L * (D / 4); i += 256) st4(ML + 4 * i, ld4(a.m + 4 * i));

    for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
        const uint64_t t0 = (uint64_t)b * L;                   // the sequence's first token
        float* sv = a.saved ? a.saved + (size_t)b * SS : nullptr;
        float *sv_uf = sv, *sv_h = sv + (size_t)L * D, *sv_u2 = sv_h + (size_t)L * F;
        load_twice(X2, a.x + (size_t)b * L * D, L);
        __syncthreads();
        // ---- filter: f[l] = sum_r m[r] x[(l - r) mod L], rows l0 .. l0 + 3 of this thread
        float4 acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        conv4<true>(acc, L, [&](int k) { return ld4(X2 + min(max(l0 + 3 + L - k, 0), 2 * L - 1) * D + c); },
                    [&](int r) { return ld4(ML + min(r, L - 1) * D + c); });
        // ---- uf = drop(f) + x, xf = LN_f(uf) -> As (zero rows behind L): the 16 lanes of a row group hold one row
        {
            const float4 gm = ld4(a.w.filter_ln_weight + c), bt = ld4(a.w.filter_ln_bias + c);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int l = l0 + i;
                float4 xf = make_float4(0.f, 0.f, 0.f, 0.f);
                if (l < L) {
                    float4 f = acc[i];
                    if (drop) f = mul4(f, drop4(rk, s_filt, ((uint64_t)b * L + l) * D + c));
                    float4 u[1] = {add4(f, ld4(X2 + l * D + c))};
                    if (sv) st4(sv_uf + (size_t)l * D + c, u[0]);
                    float mean, rstd;
                    ln_stats16<1>(u, mean, rstd, a.eps);
                    xf = ln_apply(u[0], mean, rstd, gm, bt);
                }
                st4(As + l * LDX + c, xf);
            }
        }
        __syncthreads();                                       // every read of X2 is done: R is free
        // ---- FFN, y = LN_i(xf + drop(o))
        ffn_fwd<D, F, false>(As, Bs, LDX, R, LDF, fw, sv ? sv_h : nullptr, sv ? sv_u2 : nullptr, a.y + t0 * D, rk, drop, 0u, s_ffn, t0, L, a.eps);
        __syncthreads();
    }
}

// =================================================================================================================== backward
__global__ __launch_bounds__(256) void k_fmlp_layer_bwd(const Args a) {
    extern __shared__ __align__(16) float lds[];
    float* As = lds;                       // dy -> du2 -> d xf
    float* Bs = As + 64 * LDX;             // u2 -> d f2 -> xf -> uf
    float* R = Bs + 64 * LDX;              // the FFN hidden tile, then X2 | DY2
    float* ML = R + R_FLOATS;
    float* st1 = ML + M_FLOATS;            // (mean, rstd) of the filter LayerNorm's rows
    float* st2 = st1 + 128;                // ... of the intermediate LayerNorm's rows
    float* X2 = R;                         // [2 L][64]  x twice
    float* DY2 = R + 2 * 64 * D;           // [2 L][64]  d f twice: dy[(l + r) mod L] = DY2[l + r]
    const int tid = threadIdx.x, L = a.L, dq = tid & 15, rg = tid >> 4, c = 4 * dq, l0 = 4 * rg;
    const RngKey rk = make_rng(a.seed, a.step, a.p);
    const bool drop = a.p > 0.f;
    const uint32_t s_filt = FOP_SITE_FILT(a.layer), s_ffn = FOP_SITE_FFN(a.layer);
    const int64_t SS = saved_stride(L);
    float* ws = a.slots + (size_t)blockIdx.x * NW;
    const FfnWeights fw = ffn_weights(a.w);
    const FfnGrads fg = {ws + O_W1, ws + O_B1, ws + O_W2, ws + O_B2, ws + O_ILNW, ws + O_ILNB};
    for (int i = tid; i < L * (D / 4); i += 256) st4(ML + 4 * i, ld4(a.m + 4 * i));
    float4 dmacc[4];                       // this thread's taps r = l0 .. l0 + 3 of dm, summed over the workgroup's sequences in order
#pragma unroll
    for (int i = 0; i < 4; ++i) dmacc[i] = make_float4(0.f, 0.f, 0.f, 0.f);

    for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
        const bool first = b == (int64_t)blockIdx.x;
        const uint64_t t0 = (uint64_t)b * L;                   // the sequence's first token
        const float* sv = a.saved + (size_t)b * SS;
        const float *sv_uf = sv, *sv_h = sv + (size_t)L * D, *sv_u2 = sv_h + (size_t)L * F;
        // ---------------------------------------------------------------- A: the intermediate LayerNorm and the FFN
        ffn_ln_bwd<D, F, false>(As, Bs, LDX, R, LDF, st1, st2, fw, sv_uf, sv_h, sv_u2, a.dy + t0 * D, fg, rk, drop, 0u, s_ffn, t0, L, a.eps,
                                first);                // d xf -> As
        __syncthreads();                                       // every read of R is done: X2 | DY2 take it over
        // ---------------------------------------------------------------- B: the filter LayerNorm and the filter
        load_rows<D>(Bs, LDX, sv_uf, D, L);
        load_twice(X2, a.x + (size_t)b * L * D, L);
        __syncthreads();
        ln_affine_grads<D>(ws + O_FLNW, ws + O_FLNB, As, Bs, LDX, st1, L, first);
        // du = LN_f'(d xf) of this thread's rows (the 16 lanes of a row group hold one row), d f = du * mask -> DY2 twice
        float4 du[4];
        {
            const float4 gmv = ld4(a.w.filter_ln_weight + c);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int l = l0 + i;
                du[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (l < L) {
                    float4 dz[1] = {ld4(As + l * LDX + c)}, u[1] = {ld4(Bs + l * LDX + c)}, gm[1] = {gmv};
                    float4 dg[1] = {make_float4(0.f, 0.f, 0.f, 0.f)}, db[1] = {make_float4(0.f, 0.f, 0.f, 0.f)};
                    ln_bwd_row<1>(dz, u, st1[2 * l], st1[2 * l + 1], gm, dg, db);
                    du[i] = dz[0];
                    float4 df = dz[0];
                    if (drop) df = mul4(df, drop4(rk, s_filt, ((uint64_t)b * L + l) * D + c));
                    st4(DY2 + l * D + c, df);
                    st4(DY2 + (l + L) * D + c, df);
                }
            }
        }
        __syncthreads();
        // dx[l] = du[l] + sum_r m[r] d f[(l + r) mod L]
        {
            float4 acc[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = du[i];
            conv4<false>(acc, L, [&](int k) { return ld4(DY2 + min(l0 + k, 2 * L - 1) * D + c); },
                         [&](int r) { return ld4(ML + min(r, L - 1) * D + c); });
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (l0 + i < L) st4(a.dx + ((size_t)b * L + l0 + i) * D + c, acc[i]);
        }
        // dm[r] += sum_l d f[l] x[(l - r) mod L]   (this thread owns the taps r = l0 + i)
        conv4<true>(dmacc, L, [&](int k) { return ld4(X2 + min(max(k + L - l0 - 3, 0), 2 * L - 1) * D + c); },
                    [&](int l) { return ld4(DY2 + min(l, 2 * L - 1) * D + c); });
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (l0 + i < L) st4(ws + O_DM + (l0 + i) * D + c, dmacc[i]);
}

// Sums the workgroups' partial slots in index order and writes the 9 gradients.  The first FOLD_BLOCKS blocks take four features of dm
// each: thread (r, j) sums tap r of feature 4 blockIdx.x + j over the slots, then one (k, j) pair per thread folds the column back,
//     d Wre[k][d] = (c_k / L) sum_r cos(2 pi k r / L) dm[r][d],    d Wim[k][d] = -(c_k / L) sum_r sin(2 pi k r / L) dm[r][d]
// (fmlp_coef_bwd_job of linear.hip, stored instead of added).  The other blocks: one element of the eight remaining tensors (`rest`) per
// thread.
__global__ __launch_bounds__(256) void k_fmlp_layer_reduce(const float* __restrict__ slots, int n_slots, int L, float* __restrict__ dcw,
                                                           ReduceTable rest) {
    if ((int)blockIdx.x < FOLD_BLOCKS) {
        __shared__ float ct[64], sn[64], dm[64 * 4];
        const int r = threadIdx.x >> 2, j = threadIdx.x & 3, d0 = 4 * blockIdx.x;
        if ((int)threadIdx.x < L) sincospif(2.0f * threadIdx.x / (float)L, &sn[threadIdx.x], &ct[threadIdx.x]);
        dm[threadIdx.x] = r < L ? det_sum(slots + O_DM + r * D + d0 + j, n_slots, NW) : 0.f;
        __syncthreads();
        const int K = L / 2 + 1;
        for (int i = threadIdx.x; i < K * 4; i += 256) {
            const int k = i >> 2, jj = i & 3;
            float gr = 0.f, gi = 0.f;
            for (int rr = 0; rr < L; ++rr) {
                const int t = (k * rr) % L;
                const float v = dm[rr * 4 + jj];
                gr += ct[t] * v;
                gi -= sn[t] * v;
            }
            const float cf = ((k == 0 || 2 * k == L) ? 1.f : 2.f) / (float)L;
            dcw[(k * D + d0 + jj) * 2] = cf * gr;
            dcw[(k * D + d0 + jj) * 2 + 1] = cf * gi;
        }
        return;
    }
    reduce_store(slots, n_slots, NW, O_FLNW + ((int)blockIdx.x - FOLD_BLOCKS) * 256 + (int)threadIdx.x, rest);
}

// =================================================================================================================== LayerNorm op
// One wave per row, lane i takes the float4 chunks i, i + 64, ... of the row (D <= 1024: at most LN_CH chunks per lane); biased
// variance around the mean, as torch.nn.LayerNorm.
constexpr int LN_CH = 4, LN_MAX_D = 256 * LN_CH, LN_MAX_SLOTS = 256;

__device__ __forceinline__ void ln_row_stats(const float4 (&u)[LN_CH], int n4, int Dn, float eps, float& mean, float& rstd) {
    const int lane = threadIdx.x & 63;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < LN_CH; ++j)
        if (lane + 64 * j < n4) s += (u[j].x + u[j].y) + (u[j].z + u[j].w);
    mean = wave_sum(s) / (float)Dn;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < LN_CH; ++j)
        if (lane + 64 * j < n4) {
            const float x0 = u[j].x - mean, x1 = u[j].y - mean, x2 = u[j].z - mean, x3 = u[j].w - mean;
            q += (x0 * x0 + x1 * x1) + (x2 * x2 + x3 * x3);
        }
    rstd = 1.0f / sqrtf(wave_sum(q) / (float)Dn + eps);
}

__global__ __launch_bounds__(256) void k_ln_fwd(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bs,
                                                int64_t n_rows, int Dn, float eps, float* __restrict__ y) {
    const int lane = threadIdx.x & 63, n4 = Dn / 4;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n_rows; row += (int64_t)gridDim.x * 4) {
        float4 u[LN_CH];
#pragma unroll
        for (int j = 0; j < LN_CH; ++j) u[j] = lane + 64 * j < n4 ? ld4(x + row * Dn + 4 * (lane + 64 * j)) : make_float4(0.f, 0.f, 0.f, 0.f);
        float mean, rstd;
        ln_row_stats(u, n4, Dn, eps, mean, rstd);
#pragma unroll
        for (int j = 0; j < LN_CH; ++j)
            if (lane + 64 * j < n4) {
                const int cc = 4 * (lane + 64 * j);
                st4(y + row * Dn + cc, ln_apply(u[j], mean, rstd, ld4(w + cc), ld4(bs + cc)));
            }
    }
}

// dx is written per row; every wave keeps d weight | d bias of its rows (row = 4 blockIdx.x + wave, + 4 gridDim.x, ... in that order)
// in registers, the four waves of a workgroup meet in LDS in wave order, and the workgroup's sums go to its slot [2 D]
__global__ __launch_bounds__(256) void k_ln_bwd(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ dy,
                                                int64_t n_rows, int Dn, float eps, float* __restrict__ dx, float* __restrict__ slots) {
    extern __shared__ __align__(16) float lds[];              // [4][2 D]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, n4 = Dn / 4;
    float4 dgam[LN_CH], dbet[LN_CH], gm[LN_CH];
#pragma unroll
    for (int j = 0; j < LN_CH; ++j) {
        dgam[j] = dbet[j] = gm[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane + 64 * j < n4) gm[j] = ld4(w + 4 * (lane + 64 * j));
    }
    for (int64_t row = (int64_t)blockIdx.x * 4 + wv; row < n_rows; row += (int64_t)gridDim.x * 4) {
        float4 u[LN_CH], dz[LN_CH];
#pragma unroll
        for (int j = 0; j < LN_CH; ++j) {
            u[j] = dz[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (lane + 64 * j < n4) { u[j] = ld4(x + row * Dn + 4 * (lane + 64 * j)); dz[j] = ld4(dy + row * Dn + 4 * (lane + 64 * j)); }
        }
        float mean, rstd;
        ln_row_stats(u, n4, Dn, eps, mean, rstd);
        float4 xh[LN_CH], g[LN_CH];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < LN_CH; ++j) {
            xh[j] = g[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (lane + 64 * j < n4) {
                xh[j] = make_float4((u[j].x - mean) * rstd, (u[j].y - mean) * rstd, (u[j].z - mean) * rstd, (u[j].w - mean) * rstd);
                g[j] = mul4(dz[j], gm[j]);
                s1 += (g[j].x + g[j].y) + (g[j].z + g[j].w);
                s2 += (g[j].x * xh[j].x + g[j].y * xh[j].y) + (g[j].z * xh[j].z + g[j].w * xh[j].w);
                dgam[j] = add4(dgam[j], mul4(dz[j], xh[j]));
                dbet[j] = add4(dbet[j], dz[j]);
            }
        }
        s1 = wave_sum(s1) / (float)Dn;
        s2 = wave_sum(s2) / (float)Dn;
#pragma unroll
        for (int j = 0; j < LN_CH; ++j)
            if (lane + 64 * j < n4)
                st4(dx + row * Dn + 4 * (lane + 64 * j),
                    make_float4(rstd * (g[j].x - s1 - xh[j].x * s2), rstd * (g[j].y - s1 - xh[j].y * s2), rstd * (g[j].z - s1 - xh[j].z * s2),
                                rstd * (g[j].w - s1 - xh[j].w * s2)));
    }
#pragma unroll
    for (int j = 0; j < LN_CH; ++j)
        if (lane + 64 * j < n4) {
            st4(lds + wv * 2 * Dn + 4 * (lane + 64 * j), dgam[j]);
            st4(lds + wv * 2 * Dn + Dn + 4 * (lane + 64 * j), dbet[j]);
        }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * Dn; i += 256)
        slots[(size_t)blockIdx.x * 2 * Dn + i] = ((lds[i] + lds[2 * Dn + i]) + lds[4 * Dn + i]) + lds[6 * Dn + i];
}

// =================================================================================================================== host
static int shape_check(int64_t B, int L, int Dn, int Fn) {
    if (B < 0) return DR4SR_E_ARG;
    if (Dn != D || Fn != F || L < 2 || L > 64 || (L & 1)) return DR4SR_E_SHAPE;
    return 0;
}
static int64_t ws_bytes_of(int64_t B, int backward) {
    return ((int64_t)M_FLOATS + (backward ? (int64_t)n_slots(B) * NW : 0)) * (int64_t)sizeof(float);
}
static int launch_coef(const float* cw, float* m, int L, hipStream_t st) {
    hipLaunchKernelGGL(k_fmlp_op_coef, dim3((L * D + 255) / 256), dim3(256), 0, st, cw, m, L);
    return DR4SR_LAUNCH_CHECK();
}
static int ln_check(int64_t n_rows, int Dn) {
    if (n_rows < 0) return DR4SR_E_ARG;
    if (Dn < 4 || (Dn & 3) || Dn > LN_MAX_D) return DR4SR_E_SHAPE;
    return 0;
}
static int ln_slots(int64_t n_rows) {
    const int64_t g = (n_rows + 3) / 4;
    return g < LN_MAX_SLOTS ? (int)g : LN_MAX_SLOTS;
}

}  // namespace fop

extern "C" int64_t dr4sr_fmlp_layer_saved_floats(int64_t B, int32_t L, int32_t D, int32_t F) {
    const int rc = fop::shape_check(B, L, D, F);
    if (rc) return rc;
    return B * fop::saved_stride(L);
}

extern "C" int64_t dr4sr_fmlp_layer_workspace_bytes(int64_t B, int32_t L, int32_t D, int32_t F, int32_t backward) {
    const int rc = fop::shape_check(B, L, D, F);
    if (rc) return rc;
    return fop::ws_bytes_of(B, backward != 0);
}

extern "C" int dr4sr_fmlp_layer_fwd(const float* x, const dr4sr_fmlp_layer_weights* w, int64_t B, int32_t L, int32_t D, int32_t F, float eps,
                                    float p_drop, uint64_t seed, uint32_t step, int32_t layer, float* y, float* saved, void* ws,
                                    int64_t ws_bytes, void* stream) {
    if (!fop::all_set<9>(w) || !fop::layer_args_ok(layer, p_drop, eps)) return DR4SR_E_ARG;
    const int rc = fop::shape_check(B, L, D, F);
    if (rc) return rc;
    if (B == 0) return 0;                                      // (an empty tensor's pointer may be null)
    if (!x || !y) return DR4SR_E_ARG;
    if (!ws || ws_bytes < fop::ws_bytes_of(B, 0)) return DR4SR_E_WS;
    hipStream_t st = (hipStream_t)stream;
    const int e = fop::launch_coef(w->complex_weight, (float*)ws, L, st);
    if (e) return e;
    fop::Args a{};
    a.x = x; a.w = *w; a.m = (const float*)ws; a.B = B; a.L = L; a.eps = eps; a.p = p_drop; a.seed = seed; a.step = step; a.layer = layer;
    a.y = y; a.saved = saved;
    const size_t lds = fop::LDS_FLOATS * sizeof(float);
    big_lds(fop::k_fmlp_layer_fwd, lds);
    hipLaunchKernelGGL(fop::k_fmlp_layer_fwd, dim3((unsigned)(B < 65535 ? B : 65535)), dim3(256), lds, st, a);
    return DR4SR_LAUNCH_CHECK();
}

extern "C" int dr4sr_fmlp_layer_bwd(const float* x, const dr4sr_fmlp_layer_weights* w, int64_t B, int32_t L, int32_t D, int32_t F, float eps,
                                    float p_drop, uint64_t seed, uint32_t step, int32_t layer, const float* saved, const float* dy, float* dx,
                                    const dr4sr_fmlp_layer_grads* dw, void* ws, int64_t ws_bytes, void* stream) {
    if (!fop::all_set<9>(w) || !fop::all_set<9>(dw) || !fop::layer_args_ok(layer, p_drop, eps)) return DR4SR_E_ARG;
    const int rc = fop::shape_check(B, L, D, F);
    if (rc) return rc;
    if (B > 0 && (!x || !saved || !dy || !dx)) return DR4SR_E_ARG;
    if (B > 0 && (!ws || ws_bytes < fop::ws_bytes_of(B, 1))) return DR4SR_E_WS;
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {                                              // no sequence: the gradients of the weights are zeros
        const dr4sr_fmlp_layer_grads& g = *dw;
        const fop::ZeroSpan t[9] = {{g.complex_weight, (int64_t)(L / 2 + 1) * D * 2}, {g.filter_ln_weight, D}, {g.filter_ln_bias, D},
                                    {g.dense_1_weight, (int64_t)F * D}, {g.dense_1_bias, F}, {g.dense_2_weight, (int64_t)D * F},
                                    {g.dense_2_bias, D}, {g.inter_ln_weight, D}, {g.inter_ln_bias, D}};
        return fop::zero_fill(t, 9, st);
    }
    float* m = (float*)ws;
    int e = fop::launch_coef(w->complex_weight, m, L, st);
    if (e) return e;
    fop::Args a{};
    a.x = x; a.w = *w; a.m = m; a.B = B; a.L = L; a.eps = eps; a.p = p_drop; a.seed = seed; a.step = step; a.layer = layer;
    a.saved = const_cast<float*>(saved); a.dy = dy; a.dx = dx; a.slots = m + fop::M_FLOATS;
    const size_t lds = fop::LDS_FLOATS * sizeof(float);
    big_lds(fop::k_fmlp_layer_bwd, lds);
    const int ns = fop::n_slots(B);
    hipLaunchKernelGGL(fop::k_fmlp_layer_bwd, dim3(ns), dim3(256), lds, st, a);
    e = DR4SR_LAUNCH_CHECK();
    if (e) return e;
    using namespace fop;
    const int off[9] = {O_FLNW, O_FLNB, O_W1, O_B1, O_W2, O_B2, O_ILNW, O_ILNB, NW};
    float* dst[9];
    memcpy(dst, dw, sizeof dst);                               // complex_weight, then the eight gradients in the slot's order
    hipLaunchKernelGGL(k_fmlp_layer_reduce, dim3(FOLD_BLOCKS + (NW - O_FLNW + 255) / 256), dim3(256), 0, st, a.slots, ns, L, dst[0],
                       reduce_table(dst + 1, off, 8));
    return DR4SR_LAUNCH_CHECK();
}

extern "C" int64_t dr4sr_layer_norm_workspace_bytes(int64_t n_rows, int32_t D) {
    const int rc = fop::ln_check(n_rows, D);
    if (rc) return rc;
    return (int64_t)fop::ln_slots(n_rows) * 2 * D * (int64_t)sizeof(float);
}

extern "C" int dr4sr_layer_norm_fwd(const float* x, const float* weight, const float* bias, int64_t n_rows, int32_t D, float eps, float* y,
                                    void* stream) {
    if (!weight || !bias || !(eps >= 0.f)) return DR4SR_E_ARG;
    const int rc = fop::ln_check(n_rows, D);
    if (rc) return rc;
    if (n_rows == 0) return 0;
    if (!x || !y) return DR4SR_E_ARG;
    const int64_t g = (n_rows + 3) / 4;
    hipLaunchKernelGGL(fop::k_ln_fwd, dim3((unsigned)(g < 4096 ? g : 4096)), dim3(256), 0, (hipStream_t)stream, x, weight, bias, n_rows, D, eps, y);
    return DR4SR_LAUNCH_CHECK();
}

extern "C" int dr4sr_layer_norm_bwd(const float* x, const float* weight, int64_t n_rows, int32_t D, float eps, const float* dy, float* dx,
                                    float* dw, float* db, void* ws, int64_t ws_bytes, void* stream) {
    if (!weight || !dw || !db || !(eps >= 0.f)) return DR4SR_E_ARG;
    const int rc = fop::ln_check(n_rows, D);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (n_rows == 0) {
        const fop::ZeroSpan t[2] = {{dw, D}, {db, D}};
        return fop::zero_fill(t, 2, st);
    }
    if (!x || !dy || !dx) return DR4SR_E_ARG;
    const int ns = fop::ln_slots(n_rows);
    if (!ws || ws_bytes < (int64_t)ns * 2 * D * (int64_t)sizeof(float)) return DR4SR_E_WS;
    hipLaunchKernelGGL(fop::k_ln_bwd, dim3(ns), dim3(256), (size_t)8 * D * sizeof(float), st, x, weight, dy, n_rows, D, eps, dx, (float*)ws);
    int e = DR4SR_LAUNCH_CHECK();
    if (e) return e;
    float* dst[2] = {dw, db};
    const int off[3] = {0, D, 2 * D};
    hipLaunchKernelGGL(fop::k_slot_reduce, dim3((2 * D + 255) / 256), dim3(256), 0, st, (const float*)ws, ns, 2 * D, fop::reduce_table(dst, off, 2));
    return DR4SR_LAUNCH_CHECK();
}
