// layer_op.hip — the stateless encoder-layer op (dr4sr_sasrec_layer_fwd / _bwd) and sequence pooling (dr4sr_seq_pool_fwd / _bwd) on dense
// [B, L, D] tensors: what torch.ops.dr4sr_hip.sasrec_layer / seq_pool run.  One post-norm torch.nn.TransformerEncoderLayer as the
// reference configures it (model/sasrec.py:21-30), with a general mask (key padding and / or causal); no plan, no device state words.
//
// Work distribution: one 256-thread workgroup per sequence, every activation of the layer in LDS (L <= 64 rows, zero rows behind L), GEMMs
// on v_mfma_f32_32x32x2_f32 through common.h's 64-row tile helpers.  Attention runs per 64-column GROUP of the model width: at D = 64 a
// group is both heads (head_dim 32), at D = 128 one head (head_dim 64), so q / k / v of a group are three [64][64] tiles and a head's scores
// one [64][64] tile — the full [64][3 D] projection (96 KB at D = 128) is never resident.  LDS (floats):
//     A [64][D + 4] | B [64][D + 4] | R = max([64][F + 4],  (3 + 2 HG) tiles of [64][68])        HG = heads per group
// = 152 KB at D = 128 and 154 KB at D = 64 of the CU's 160 KB: one workgroup per CU.
//
// The backward recomputes nothing but the dropout masks (Philox is a pure function of (seed, step, site, element)) and the two LayerNorm
// statistics: the forward saves qkv, the attention context, both LayerNorm inputs, the FFN pre-activation and the attention
// probabilities (dr4sr_sasrec_layer_saved_floats).  Weight gradients: every workgroup writes ITS sum over the sequences it owns (b =
// blockIdx.x, + gridDim.x, ... in that order) into its own slot of the workspace, a second launch adds the slots in index order — no float
// atomics, the same bits on every call.
//
// This file holds the attention half of the layer and the out_proj / LayerNorm 1 step around it; the FFN + LayerNorm 2 half, forward and
// backward, the row passes and the slot reduction are op_tiles.h's (shared with fmlp_op.hip).
#include "common.h"
#include "op_tiles.h"
#include "layer_geo.h"

namespace lop {
using namespace optile;

__host__ __device__ inline int64_t saved_stride(int L, int D, int F) { return (((int64_t)L * (6 * D + F) + 2 * (int64_t)L * L) + 3) & ~(int64_t)3; }

struct Args {
    const float* x; const unsigned char* key_pad; int causal;
    dr4sr_layer_weights w;
    int64_t B; int L; float eps, p; uint64_t seed; uint32_t step; int layer;
    float* y; float* saved;
    const float* dy; float* dx; float* ws;
};

// the FFN block's view of the layer: linear1, linear2, norm2; norm1 made its input
__device__ __forceinline__ FfnWeights ffn_weights(const dr4sr_layer_weights& w) {
    return {w.linear1_weight, w.linear1_bias, w.linear2_weight, w.linear2_bias, w.norm2_weight, w.norm2_bias, w.norm1_weight, w.norm1_bias};
}
// does query i of this sequence admit key j?  kp = LDS flags (1: padded or behind L)
__device__ __forceinline__ bool admit(const float* kp, int causal, int i, int j) { return kp[j] == 0.f && (!causal || j <= i); }

// =================================================================================================================== forward
template <int D, int F>
__global__ __launch_bounds__(256) void k_layer_fwd(const Args a) {
    using G = Geo<D, F>;
    constexpr int LDX = G::LDX, LDF = G::LDF, DH = G::DH, HG = G::HG;
    extern __shared__ __align__(16) float lds[];
    float* As = lds;                       // x, then y1
    float* Bs = As + 64 * LDX;             // attention context, then the FFN output
    float* R = Bs + 64 * LDX;
    float* kp = R + G::R_FLOATS;
    float *Qs = R, *Ks = R + TILE, *Vs = R + 2 * TILE, *Ss = R + 3 * TILE;
    const int tid = threadIdx.x, L = a.L;
    const RngKey rk = make_rng(a.seed, a.step, a.p);
    const bool drop = a.p > 0.f;
    const uint32_t s_attn = DR4SR_SITE_ATTN + 4 * a.layer, s_proj = DR4SR_SITE_PROJ + 4 * a.layer, s_act = DR4SR_SITE_ACT + 4 * a.layer,
                   s_ffn = DR4SR_SITE_FFN + 4 * a.layer;
    const float scale = 1.0f / sqrtf((float)DH);
    const int64_t SS = saved_stride(L, D, F);
    const int wv = tid >> 6, cg = wv >> 1;
    const FfnWeights fw = ffn_weights(a.w);

    for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
        const uint64_t t0 = (uint64_t)b * L;                   // the sequence's first token
        float* sv = a.saved ? a.saved + (size_t)b * SS : nullptr;
        float* sv_qkv = sv, *sv_ctx = sv + (size_t)L * 3 * D, *sv_u1 = sv_ctx + (size_t)L * D, *sv_h = sv_u1 + (size_t)L * D,
              *sv_u2 = sv_h + (size_t)L * F, *sv_p = sv_u2 + (size_t)L * D;
        load_rows<D>(As, LDX, a.x + (size_t)b * L * D, D, L);
        if (tid < 64) kp[tid] = (tid >= L || (a.key_pad && a.key_pad[(size_t)b * L + tid])) ? 1.f : 0.f;
        __syncthreads();
        // ---- attention, one 64-column group at a time
        for (int g = 0; g < G::NG; ++g) {
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                f32x16 acc[1];
                acc_zero(acc);
                mma_64xN<D, 1>(As, LDX, a.w.in_proj_weight + (size_t)(m * D + g * 64) * D, acc);
                acc_to_lds<1>(acc, R + m * TILE, LDT, a.w.in_proj_bias + m * D + g * 64);
            }
            __syncthreads();
            if (sv)
                for (int m = 0; m < 3; ++m) store_rows<64>(sv_qkv + m * D + g * 64, 3 * D, R + m * TILE, LDT, L);
#pragma unroll
            for (int hh = 0; hh < HG; ++hh) {
                f32x16 acc[1];
                acc_zero(acc);
                mma_64xN_ld<DH, 1>(Qs + hh * DH, LDT, Ks + hh * DH, LDT, acc);
                acc_to_lds<1>(acc, Ss + hh * TILE, LDT, nullptr);
            }
            __syncthreads();
            // softmax + dropout: 4 lanes per query row, lane t takes keys t, t + 4, ...
            for (int hh = 0; hh < HG; ++hh) {
                const int i = tid >> 2, t = tid & 3, h = g * HG + hh;
                float* srow = Ss + hh * TILE + i * LDT;
                float v[16], mx = -INFINITY;
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const int j = t + 4 * c;
                    v[c] = admit(kp, a.causal, i, j) ? srow[j] * scale : -INFINITY;
                    mx = fmaxf(mx, v[c]);
                }
                mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
                mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
                float sum = 0.f;
#pragma unroll
                for (int c = 0; c < 16; ++c) { v[c] = (mx == -INFINITY) ? 0.f : expf(v[c] - mx); sum += v[c]; }
                sum += __shfl_xor(sum, 1, 64);
                sum += __shfl_xor(sum, 2, 64);
                const float inv = (mx == -INFINITY || i >= L) ? 0.f : 1.0f / sum;      // no admissible key: a zero context
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const int j = t + 4 * c;
                    float pv = v[c] * inv;
                    if (i < L && j < L) {
                        const size_t e = ((size_t)(b * 2 + h) * L + i) * L + j;
                        if (sv) sv_p[((size_t)h * L + i) * L + j] = pv;
                        if (drop) pv *= drop1(rk, s_attn, e);
                    }
                    srow[j] = pv;
                }
            }
            __syncthreads();
            {
                f32x16 acc[1];
                acc_zero(acc);
                mma_64xN_wT<64, 1>(Ss + ((cg * 32) / DH) * TILE, LDT, Vs, LDT, acc);
                acc_to_lds<1>(acc, Bs + g * 64, LDX, nullptr);
            }
            __syncthreads();
        }
        if (sv) store_rows<D>(sv_ctx, D, Bs, LDX, L);
        // ---- out_proj -> R [64][LDX]
        {
            f32x16 acc[D / 64];
            acc_zero(acc);
            mma_64xN<D, D / 64>(Bs, LDX, a.w.out_proj_weight, acc);
            acc_to_lds<D / 64>(acc, R, LDX, a.w.out_proj_bias);
        }
        __syncthreads();
        // ---- u1 = x + drop(o), y1 = LN1(u1) -> As : 16 lanes per row
        res_drop_ln_rows<D>(As, LDX, As, R, LDX, a.w.norm1_weight, a.w.norm1_bias, sv ? sv_u1 : nullptr, rk, drop, s_proj, t0, L, a.eps);
        __syncthreads();
        // ---- FFN, y = LN2(y1 + drop(f))
        ffn_fwd<D, F, true>(As, Bs, LDX, R, LDF, fw, sv ? sv_h : nullptr, sv ? sv_u2 : nullptr, a.y + t0 * D, rk, drop, s_act, s_ffn, t0, L, a.eps);
        __syncthreads();
    }
}

// =================================================================================================================== backward
template <int D, int F>
__global__ __launch_bounds__(256) void k_layer_bwd(const Args a) {
    using G = Geo<D, F>;
    constexpr int LDX = G::LDX, LDF = G::LDF, DH = G::DH, HG = G::HG;
    extern __shared__ __align__(16) float lds[];
    float* As = lds;                       // dy -> du2 -> dy1 -> du1 -> d ctx
    float* Bs = As + 64 * LDX;             // u2 -> d f2 -> y1 -> u1 -> d o -> x
    float* R = Bs + 64 * LDX;
    float* kp = R + G::R_FLOATS;
    float* st1 = kp + 64;
    float* st2 = st1 + 128;
    float *Qs = R, *Ks = R + TILE, *Vs = R + 2 * TILE, *Ss = R + 3 * TILE, *Ds = R + (3 + HG) * TILE;
    const int tid = threadIdx.x, L = a.L;
    const RngKey rk = make_rng(a.seed, a.step, a.p);
    const bool drop = a.p > 0.f;
    const uint32_t s_attn = DR4SR_SITE_ATTN + 4 * a.layer, s_proj = DR4SR_SITE_PROJ + 4 * a.layer, s_act = DR4SR_SITE_ACT + 4 * a.layer,
                   s_ffn = DR4SR_SITE_FFN + 4 * a.layer;
    const float scale = 1.0f / sqrtf((float)DH);
    const int64_t SS = saved_stride(L, D, F);
    const int lane = tid & 63, wv = tid >> 6, r32 = lane & 31, g32 = lane >> 5, rh = wv & 1, cg = wv >> 1;
    float* ws = a.ws + (size_t)blockIdx.x * G::NW;
    const FfnWeights fw = ffn_weights(a.w);
    const FfnGrads fg = {ws + G::O_W1, ws + G::O_B1, ws + G::O_W2, ws + G::O_B2, ws + G::O_N2W, ws + G::O_N2B};

    for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
        const bool first = b == (int64_t)blockIdx.x;
        const uint64_t t0 = (uint64_t)b * L;                   // the sequence's first token
        const float* sv = a.saved + (size_t)b * SS;
        const float *sv_qkv = sv, *sv_ctx = sv + (size_t)L * 3 * D, *sv_u1 = sv_ctx + (size_t)L * D, *sv_h = sv_u1 + (size_t)L * D,
                    *sv_u2 = sv_h + (size_t)L * F, *sv_p = sv_u2 + (size_t)L * D;
        float* dxb = a.dx + (size_t)b * L * D;
        // ---------------------------------------------------------------- A: LayerNorm 2 and the FFN
        if (tid < 64) kp[tid] = (tid >= L || (a.key_pad && a.key_pad[(size_t)b * L + tid])) ? 1.f : 0.f;
        ffn_ln_bwd<D, F, true>(As, Bs, LDX, R, LDF, st1, st2, fw, sv_u1, sv_h, sv_u2, a.dy + t0 * D, fg, rk, drop, s_act, s_ffn, t0, L, a.eps,
                               first);                 // dy1 -> As
        __syncthreads();
        // ---------------------------------------------------------------- B: LayerNorm 1 and out_proj
        load_rows<D>(Bs, LDX, sv_u1, D, L);
        __syncthreads();
        ln_affine_grads<D>(ws + G::O_N1W, ws + G::O_N1B, As, Bs, LDX, st1, L, first);
        __syncthreads();
        // du1 -> the residual branch of dx (the attention branch is added at the end), d o = du1 * mask -> Bs
        ln_bwd_rows<D>(As, Bs, LDX, st1, a.w.norm1_weight, dxb, rk, drop, s_proj, t0, L);
        load_rows<D>(R, LDX, sv_ctx, D, L);
        __syncthreads();
        wgrad_tn<D, D>(ws + G::O_OW, D, Bs, LDX, R, LDX, first);
        colsum(ws + G::O_OB, Bs, LDX, D, L, first);
        {
            f32x16 acc[D / 64];
            acc_zero(acc);
            mma_wT<D, D / 64>(Bs, LDX, a.w.out_proj_weight, D, acc);
            __syncthreads();
            acc_to_lds<D / 64>(acc, As, LDX, nullptr);        // d ctx
        }
        load_rows<D>(Bs, LDX, a.x + (size_t)b * L * D, D, L);
        // ---------------------------------------------------------------- C: attention, group by group
        f32x16 dxacc[D / 64];
        acc_zero(dxacc);
        for (int g = 0; g < G::NG; ++g) {
            __syncthreads();
            for (int m = 0; m < 3; ++m) load_rows<64>(R + m * TILE, LDT, sv_qkv + m * D + g * 64, 3 * D, L);
            for (int i = tid; i < HG * 64 * 64; i += 256) {
                const int hh = i >> 12, qi = (i >> 6) & 63, j = i & 63;
                Ss[hh * TILE + qi * LDT + j] = (qi < L && j < L) ? sv_p[((size_t)(g * HG + hh) * L + qi) * L + j] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int hh = 0; hh < HG; ++hh) {
                f32x16 acc[1];
                acc_zero(acc);
                mma_64xN_ld<DH, 1>(As + g * 64 + hh * DH, LDX, Vs + hh * DH, LDT, acc);
                acc_to_lds<1>(acc, Ds + hh * TILE, LDT, nullptr);
            }
            __syncthreads();
            // Ss := p * mask (what multiplied v), Ds := scale * p * (dp - <dp, p>)
            for (int hh = 0; hh < HG; ++hh) {
                const int i = tid >> 2, t = tid & 3, h = g * HG + hh;
                float* prow = Ss + hh * TILE + i * LDT;
                float* drow = Ds + hh * TILE + i * LDT;
                float pv[16], dp[16], dot = 0.f;
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const int j = t + 4 * c;
                    pv[c] = prow[j];
                    float m = 1.f;
                    if (drop && i < L && j < L) m = drop1(rk, s_attn, ((size_t)(b * 2 + h) * L + i) * L + j);
                    dp[c] = drow[j] * m;
                    dot += dp[c] * pv[c];
                    prow[j] = pv[c] * m;
                }
                dot += __shfl_xor(dot, 1, 64);
                dot += __shfl_xor(dot, 2, 64);
#pragma unroll
                for (int c = 0; c < 16; ++c) drow[t + 4 * c] = scale * pv[c] * (dp[c] - dot);
            }
            __syncthreads();
            {
                const int hd = (cg * 32) / DH;                 // head (inside the group) of this wave's 32 output columns
                const f32x16 dv = mma_tn(Ss + hd * TILE + rh * 32, LDT, As + g * 64 + cg * 32, LDX);
                const f32x16 dk = mma_tn(Ds + hd * TILE + rh * 32, LDT, Qs + cg * 32, LDT);
                f32x16 dq[1];
                acc_zero(dq);
                mma_64xN_wT<64, 1>(Ds + hd * TILE, LDT, Ks, LDT, dq);
                __syncthreads();
                f32x16 t1[1];
                acc_to_lds<1>(dq, Qs, LDT, nullptr);
                t1[0] = dk; acc_to_lds<1>(t1, Ks, LDT, nullptr);
                t1[0] = dv; acc_to_lds<1>(t1, Vs, LDT, nullptr);
            }
            __syncthreads();
            for (int m = 0; m < 3; ++m) {
                wgrad_tn<64, D>(ws + G::O_INW + (size_t)(m * D + g * 64) * D, D, R + m * TILE, LDT, Bs, LDX, first);
                colsum(ws + G::O_INB + m * D + g * 64, R + m * TILE, LDT, 64, L, first);
                mma_wT<64, D / 64>(R + m * TILE, LDT, a.w.in_proj_weight + (size_t)(m * D + g * 64) * D, D, dxacc);
            }
        }
        __syncthreads();                                       // makes this workgroup's residual-branch stores to dx visible to it
        // (not through acc_each: with it the d = 64 backward launches took 0.293 ms against 0.276, NOTEBOOK)
#pragma unroll
        for (int i = 0; i < D / 64; ++i)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int row = rh * 32 + (q & 3) + 8 * (q >> 2) + 4 * g32;
                if (row < L) dxb[(size_t)row * D + (cg + 2 * i) * 32 + r32] += dxacc[i][q];
            }
        __syncthreads();
    }
}

// =================================================================================================================== pooling
__device__ __forceinline__ int clamp_len(const int64_t* seqlen, int b, int L) {
    const int64_t n = seqlen[b];
    return n < 0 ? 0 : n > L ? L : (int)n;
}
// ORIGIN: one thread per element of [B, L, D]; LAST / MEAN: one thread per element of [B, D]
__global__ void k_pool_fwd(const float* __restrict__ x, const int64_t* __restrict__ seqlen, int pooling, int64_t B, int L, int D,
                           float* __restrict__ out) {
    const int64_t n = pooling == DR4SR_POOL_ORIGIN ? B * L * D : B * D;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        if (pooling == DR4SR_POOL_ORIGIN) {
            const int b = (int)(e / ((int64_t)L * D)), pos = (int)((e / D) % L);
            out[e] = pos < clamp_len(seqlen, b, L) ? x[e] : 0.f;
        } else {
            const int b = (int)(e / D), c = (int)(e % D), n_ = clamp_len(seqlen, b, L);
            const float* xb = x + (size_t)b * L * D + c;
            float v = 0.f;
            if (n_ > 0) {
                if (pooling == DR4SR_POOL_LAST) v = xb[(size_t)(n_ - 1) * D];
                else { for (int pos = 0; pos < n_; ++pos) v += xb[(size_t)pos * D]; v /= (float)n_; }
            }
            out[e] = v;
        }
    }
}
__global__ void k_pool_bwd(const float* __restrict__ dout, const int64_t* __restrict__ seqlen, int pooling, int64_t B, int L, int D,
                           float* __restrict__ dx) {
    const int64_t n = B * L * D;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(e / ((int64_t)L * D)), pos = (int)((e / D) % L), c = (int)(e % D), n_ = clamp_len(seqlen, b, L);
        float v = 0.f;
        if (pooling == DR4SR_POOL_ORIGIN) v = pos < n_ ? dout[e] : 0.f;
        else if (pooling == DR4SR_POOL_LAST) v = pos == n_ - 1 ? dout[(size_t)b * D + c] : 0.f;
        else v = pos < n_ ? dout[(size_t)b * D + c] / (float)n_ : 0.f;
        dx[e] = v;
    }
}

__global__ void k_dropout_apply(const float* __restrict__ x, int64_t n4, float p, uint64_t seed, uint32_t step, uint32_t site,
                                float* __restrict__ out) {
    const RngKey rk = make_rng(seed, step, p);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 v = ld4(x + i * 4);
        if (p > 0.f) v = mul4(v, drop4(rk, site, (uint64_t)i * 4));
        st4(out + i * 4, v);
    }
}

// backward of embed_gather_posadd: dE[idx[t]] += dx[t] (PAD id 0 and ids outside the table pass nothing), dP[pos] = sum_b dx[b, pos]
__global__ void k_embed_bwd_table(const float* __restrict__ dx, const int64_t* __restrict__ idx, int64_t T, int D, int N, float* __restrict__ dE) {
    const int C4 = D / 4;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < T * C4; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = e / C4, id = idx[t];
        if (id <= 0 || id >= N) continue;
        const int c = (int)(e % C4) * 4;
        const float4 v = ld4(dx + t * D + c);
        float* d = dE + id * D + c;
        atomicAdd(d, v.x); atomicAdd(d + 1, v.y); atomicAdd(d + 2, v.z); atomicAdd(d + 3, v.w);
    }
}
__global__ void k_embed_bwd_pos(const float* __restrict__ dx, int B, int LD, float* __restrict__ dP) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < LD) dP[e] = det_sum(dx + e, B, (size_t)LD);
}

// =================================================================================================================== host
template <int D, int F>
static int launch_fwd(const Args& a, hipStream_t st) {
    const size_t lds = Geo<D, F>::LDS_FLOATS * sizeof(float);
    big_lds(k_layer_fwd<D, F>, lds);
    hipLaunchKernelGGL((k_layer_fwd<D, F>), dim3((unsigned)(a.B < 65535 ? a.B : 65535)), dim3(256), lds, st, a);
    return DR4SR_LAUNCH_CHECK();
}
template <int D, int F>
static int launch_bwd(const Args& a, const dr4sr_layer_grads& dw, hipStream_t st) {
    using G = Geo<D, F>;
    static_assert(G::NW == 4 * D * D + 2 * D * F + 9 * D + F, "slot size");
    const int off[13] = {G::O_INW, G::O_INB, G::O_OW, G::O_OB, G::O_W1, G::O_B1, G::O_W2, G::O_B2, G::O_N1W, G::O_N1B, G::O_N2W, G::O_N2B, G::NW};
    float* dst[12];
    memcpy(dst, &dw, sizeof dst);                              // the 12 gradients in the slot's order
    const size_t lds = G::LDS_FLOATS * sizeof(float);
    big_lds(k_layer_bwd<D, F>, lds);
    const int ns = n_slots(a.B);
    hipLaunchKernelGGL((k_layer_bwd<D, F>), dim3(ns), dim3(256), lds, st, a);
    int rc = DR4SR_LAUNCH_CHECK();
    if (rc) return rc;
    hipLaunchKernelGGL(k_slot_reduce, dim3((G::NW + 255) / 256), dim3(256), 0, st, a.ws, ns, G::NW, reduce_table(dst, off, 12));
    return DR4SR_LAUNCH_CHECK();
}

}  // namespace lop

extern "C" int64_t dr4sr_sasrec_layer_saved_floats(int64_t B, int32_t L, int32_t D, int32_t H, int32_t F) {
    const int rc = lop::shape_check(B, L, D, H, F);
    if (rc) return rc;
    return B * lop::saved_stride(L, D, F);
}

extern "C" int64_t dr4sr_sasrec_layer_workspace_bytes(int64_t B, int32_t L, int32_t D, int32_t H, int32_t F) {
    const int rc = lop::shape_check(B, L, D, H, F);
    if (rc) return rc;
    return (int64_t)lop::n_slots(B) * lop::slot_floats(D, F) * (int64_t)sizeof(float);
}

extern "C" int dr4sr_sasrec_layer_fwd(const float* x, const uint8_t* key_pad, int32_t causal, const dr4sr_layer_weights* w, int64_t B, int32_t L,
                                      int32_t D, int32_t H, int32_t F, float eps, float p_drop, uint64_t seed, uint32_t step, int32_t layer,
                                      float* y, float* saved, void* stream) {
    if (!lop::all_set<12>(w) || !lop::layer_args_ok(layer, p_drop, eps)) return DR4SR_E_ARG;
    const int rc = lop::shape_check(B, L, D, H, F);
    if (rc) return rc;
    if (B == 0) return 0;                                      // (an empty tensor's pointer may be null)
    if (!x || !y) return DR4SR_E_ARG;
    lop::Args a{};
    a.x = x; a.key_pad = key_pad; a.causal = causal != 0; a.w = *w; a.B = B; a.L = L; a.eps = eps; a.p = p_drop; a.seed = seed; a.step = step;
    a.layer = layer; a.y = y; a.saved = saved;
    hipStream_t st = (hipStream_t)stream;
    if (D == 64 && F == 128) return lop::launch_fwd<64, 128>(a, st);
    if (D == 64) return lop::launch_fwd<64, 256>(a, st);
    return lop::launch_fwd<128, 128>(a, st);
}

extern "C" int dr4sr_sasrec_layer_bwd(const float* x, const uint8_t* key_pad, int32_t causal, const dr4sr_layer_weights* w, int64_t B, int32_t L,
                                      int32_t D, int32_t H, int32_t F, float eps, float p_drop, uint64_t seed, uint32_t step, int32_t layer,
                                      const float* saved, const float* dy, float* dx, const dr4sr_layer_grads* dw, void* ws, int64_t ws_bytes,
                                      void* stream) {
    if (!lop::all_set<12>(w) || !lop::all_set<12>(dw) || !lop::layer_args_ok(layer, p_drop, eps)) return DR4SR_E_ARG;
    const int rc = lop::shape_check(B, L, D, H, F);
    if (rc) return rc;
    if (B > 0 && (!x || !saved || !dy || !dx)) return DR4SR_E_ARG;
    if (B > 0 && (!ws || ws_bytes < (int64_t)lop::n_slots(B) * lop::slot_floats(D, F) * (int64_t)sizeof(float))) return DR4SR_E_WS;
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {                                              // no sequence: the gradients of the weights are zeros
        const dr4sr_layer_grads& g = *dw;
        const lop::ZeroSpan t[12] = {{g.in_proj_weight, 3LL * D * D}, {g.in_proj_bias, 3LL * D}, {g.out_proj_weight, (int64_t)D * D},
                                     {g.out_proj_bias, D}, {g.linear1_weight, (int64_t)F * D}, {g.linear1_bias, F},
                                     {g.linear2_weight, (int64_t)D * F}, {g.linear2_bias, D}, {g.norm1_weight, D}, {g.norm1_bias, D},
                                     {g.norm2_weight, D}, {g.norm2_bias, D}};
        return lop::zero_fill(t, 12, st);
    }
    lop::Args a{};
    a.x = x; a.key_pad = key_pad; a.causal = causal != 0; a.w = *w; a.B = B; a.L = L; a.eps = eps; a.p = p_drop; a.seed = seed; a.step = step;
    a.layer = layer; a.saved = const_cast<float*>(saved); a.dy = dy; a.dx = dx; a.ws = (float*)ws;
    if (D == 64 && F == 128) return lop::launch_bwd<64, 128>(a, *dw, st);
    if (D == 64) return lop::launch_bwd<64, 256>(a, *dw, st);
    return lop::launch_bwd<128, 128>(a, *dw, st);
}

static int pool_check(const void* a, const void* b, const void* c, int64_t B, int32_t L, int32_t D, int32_t pooling) {
    if (!a || !b || !c || B < 0 || L < 1 || D < 1) return DR4SR_E_ARG;
    if (pooling != DR4SR_POOL_ORIGIN && pooling != DR4SR_POOL_LAST && pooling != DR4SR_POOL_MEAN) return DR4SR_E_ARG;
    return 0;
}
static unsigned pool_blocks(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return (unsigned)(b > 4096 ? 4096 : b);
}

extern "C" int dr4sr_seq_pool_fwd(const float* x, const int64_t* seqlen, int32_t pooling, int64_t B, int32_t L, int32_t D, float* out, void* stream) {
    const int rc = pool_check(x, seqlen, out, B, L, D, pooling);
    if (rc) return rc;
    if (B == 0) return 0;
    const int64_t n = pooling == DR4SR_POOL_ORIGIN ? B * L * D : B * D;
    hipLaunchKernelGGL(lop::k_pool_fwd, dim3(pool_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, seqlen, pooling, B, L, D, out);
    return DR4SR_LAUNCH_CHECK();
}

extern "C" int dr4sr_dropout_apply(const float* x, int64_t n, float p_drop, uint64_t seed, uint32_t step, uint32_t site, float* out, void* stream) {
    if (!x || !out || n < 0 || (n & 3) || !(p_drop >= 0.f && p_drop < 1.f)) return DR4SR_E_ARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(lop::k_dropout_apply, dim3(pool_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, x, n / 4, p_drop, seed, step, site, out);
    return DR4SR_LAUNCH_CHECK();
}

extern "C" int dr4sr_embed_gather_posadd_bwd(const float* dx, const int64_t* idx, int64_t B, int32_t L, int32_t D, int32_t n_items, int32_t n_pos,
                                             float* dE, float* dP, void* stream) {
    if (!dx || !idx || !dE || !dP || B < 0 || L < 1 || n_items < 1 || n_pos < L || B > (1 << 24)) return DR4SR_E_ARG;
    if (D < 4 || (D & 3)) return DR4SR_E_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    int e = hip_ret(hipMemsetAsync(dE, 0, (size_t)n_items * D * sizeof(float), st));
    if (!e) e = hip_ret(hipMemsetAsync(dP, 0, (size_t)n_pos * D * sizeof(float), st));
    if (e || B == 0) return e;
    hipLaunchKernelGGL(lop::k_embed_bwd_table, dim3(pool_blocks(B * L * (D / 4))), dim3(256), 0, st, dx, idx, B * L, D, n_items, dE);
    hipLaunchKernelGGL(lop::k_embed_bwd_pos, dim3((L * D + 255) / 256), dim3(256), 0, st, dx, (int)B, L * D, dP);
    return DR4SR_LAUNCH_CHECK();
}

extern "C" int dr4sr_seq_pool_bwd(const float* dout, const int64_t* seqlen, int32_t pooling, int64_t B, int32_t L, int32_t D, float* dx, void* stream) {
    const int rc = pool_check(dout, seqlen, dx, B, L, D, pooling);
    if (rc) return rc;
    if (B == 0) return 0;
    hipLaunchKernelGGL(lop::k_pool_bwd, dim3(pool_blocks(B * L * D)), dim3(256), 0, (hipStream_t)stream, dout, seqlen, pooling, B, L, D, dx);
    return DR4SR_LAUNCH_CHECK();
}
