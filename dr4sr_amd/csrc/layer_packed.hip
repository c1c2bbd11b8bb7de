// layer_packed.hip — the encoder-layer op with sequence lengths (dr4sr_sasrec_layer_packed_fwd / _bwd): what
// torch.ops.dr4sr_hip.sasrec_layer_packed runs.  The layer, the tensors and the dropout elements are layer_op.hip's; here SEVERAL short
// sequences share one 64-row LDS tile, so the MFMA tiles, the workgroups and the weight-gradient partials go with the valid tokens and
// not with B * L.  Three things differ from the dense kernels:
//   * a device-side plan (k_plan_count, k_plan_fill) assigns the sequences to tiles, chunk by chunk, from seqlen: tile t is the
//     sequences [first[t], end[t]), whose valid rows lie one behind the other from row 0;
//   * a row table in LDS, tok[row] = b * L + pos and s0[row] = the first row of the row's sequence (-1 behind the tile's fill),
//     through which op_tiles.h's row-indirect passes address the global [B L][W] tensors and the dropout elements;
//   * admit(i, j) is block-diagonal: rows i and j belong to the same sequence (and j <= i when causal — rows of a sequence are in
//     position order, so row order is position order).
// LDS: layer_op.hip's tiles and statistics, the key flags replaced by the row table (+ 68 words): 154.5 KB at D = 64, 152.5 KB at D = 128.
//
// saved, by section over all B * L tokens: qkv [B L][3 D] | ctx [B L][D] | u1 [B L][D] | h [B L][F] | u2 [B L][D] | p [B][H][L][L]; only
// valid tokens (and key pairs of valid tokens of one sequence) are written and read.
//
// Grid: min(B, 256) workgroups stride over the tiles (a tile costs the same whatever its fill); the tile count is read from the plan.
// The backward's slot reduction reads it too and adds only the slots that were written.
#include "common.h"
#include "op_tiles.h"
#include "layer_geo.h"
#include "../../include/dr4sr_hip_probes.h"

namespace lpk {
using namespace optile;
using namespace lop;

constexpr int CHUNK = 128;             // consecutive sequences planned together (the probe dr4sr_sasrec_layer_packed_chunk)
constexpr int TABLE_WORDS = 64 + 64 + 4;       // tok | s0 | the tile's fill
static_assert(CHUNK <= 128 && CHUNK <= 256, "the lengths of a tile's sequences are staged in the 128 words of st1, one thread each");

template <int D, int F> struct PGeo {
    // layer_op's tail is key flags [64] | st1 [128] | st2 [128]; here: tok [64] | s0 [64] | fill [4] | st1 [128] | st2 [128]
    static constexpr int LDS_FLOATS = Geo<D, F>::LDS_FLOATS - 64 + TABLE_WORDS;
    static_assert(LDS_FLOATS * 4 <= 160 * 1024, "one workgroup's tiles and the row table fit the CU's LDS");
};

// ------------------------------------------------------------------------------------------------------------------------ the plan
// workspace, ints: [0] tile count | [4, 4 + chunks) tiles per chunk | first[B] | end[B]; the backward's slots follow (16-byte aligned)
static inline int64_t n_chunks(int64_t B) { return (B + CHUNK - 1) / CHUNK; }
static inline int64_t plan_ints(int64_t B) { return (4 + n_chunks(B) + 2 * B + 3) & ~(int64_t)3; }
struct Plan { int* n_tiles; int* cnt; int* first; int* end; };
static inline Plan plan_view(void* ws, int64_t B) {
    int* p = (int*)ws;
    return {p, p + 4, p + 4 + n_chunks(B), p + 4 + n_chunks(B) + B};
}

__device__ __forceinline__ int clamp_len(const int64_t* __restrict__ seqlen, int64_t b, int L) {
    const int64_t n = seqlen[b];
    return n < 0 ? 0 : n > L ? L : (int)n;
}
// the lengths of chunk ch -> LDS (0 behind B); every lane of the 64-thread block
__device__ __forceinline__ void chunk_lens(int* lens, const int64_t* __restrict__ seqlen, int64_t B, int L, int64_t ch) {
    for (int i = threadIdx.x; i < CHUNK; i += 64) {
        const int64_t b = ch * CHUNK + i;
        lens[i] = b < B ? clamp_len(seqlen, b, L) : 0;
    }
    __syncthreads();
}
// The walk over one chunk: emit(i, tile, row) for every sequence i of the chunk with rows, tile counted from 0 inside the chunk;
// returns the chunk's tile count.
template <class Emit>
__device__ __forceinline__ int chunk_walk(const int* lens, Emit emit) {
    int cur = -1, r = 0;
    for (int i = 0; i < CHUNK; ++i) {
        const int n = lens[i];
        if (n == 0) continue;
        if (cur < 0 || r + n > 64) { ++cur; r = 0; }
        emit(i, cur, r);
        r += n;
    }
    return cur + 1;
}
__global__ __launch_bounds__(64) void k_plan_count(const int64_t* __restrict__ seqlen, int64_t B, int L, Plan p) {
    __shared__ int lens[CHUNK];
    chunk_lens(lens, seqlen, B, L, blockIdx.x);
    if (threadIdx.x == 0) p.cnt[blockIdx.x] = chunk_walk(lens, [](int, int, int) {});
}
// tile_of / row_of: the probe's view of the plan (include/dr4sr_hip_probes.h), or null
__global__ __launch_bounds__(64) void k_plan_fill(const int64_t* __restrict__ seqlen, int64_t B, int L, Plan p, int* __restrict__ tile_of,
                                                  int* __restrict__ row_of) {
    __shared__ int lens[CHUNK], tl[CHUNK], rw[CHUNK];
    const int64_t ch = blockIdx.x;
    chunk_lens(lens, seqlen, B, L, ch);
    int base = 0;                                              // tiles of the chunks in front of this one
    for (int64_t c = threadIdx.x; c < ch; c += 64) base += p.cnt[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) base += __shfl_xor(base, o, 64);
    for (int i = threadIdx.x; i < CHUNK; i += 64) tl[i] = rw[i] = -1;
    __syncthreads();
    if (threadIdx.x == 0) {
        int* first = p.first + base;
        int* end = p.end + base;
        const int b0 = (int)(ch * CHUNK);
        const int n = chunk_walk(lens, [=](int i, int t, int r) {
            if (r == 0) first[t] = b0 + i;
            end[t] = b0 + i + 1;
            tl[i] = base + t;
            rw[i] = r;
        });
        if (ch == gridDim.x - 1) *p.n_tiles = base + n;
    }
    __syncthreads();
    if (tile_of)
        for (int i = threadIdx.x; i < CHUNK; i += 64) {
            const int64_t b = ch * CHUNK + i;
            if (b < B) { tile_of[b] = tl[i]; row_of[b] = rw[i]; }
        }
}
static int launch_plan(const int64_t* seqlen, int64_t B, int L, const Plan& p, int* tile_of, int* row_of, hipStream_t st) {
    const unsigned nch = (unsigned)n_chunks(B);
    hipLaunchKernelGGL(k_plan_count, dim3(nch), dim3(64), 0, st, seqlen, B, L, p);
    hipLaunchKernelGGL(k_plan_fill, dim3(nch), dim3(64), 0, st, seqlen, B, L, p, tile_of, row_of);
    return DR4SR_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------------------------------ the tile
struct Args {
    const float* x; const int64_t* seqlen; int causal;
    dr4sr_layer_weights w;
    int64_t B; int L; float eps, p; uint64_t seed; uint32_t step; int layer;
    float* y; float* saved;
    const float* dy; float* dx; float* ws;
    Plan plan;
};
// the sections of saved
struct Saved { float *qkv, *ctx, *u1, *h, *u2, *p; };
__host__ __device__ inline int64_t saved_floats(int64_t B, int L, int D, int F) { return B * ((int64_t)L * (6 * D + F) + 2 * (int64_t)L * L); }
__device__ __forceinline__ Saved saved_view(float* s, int64_t B, int L, int D, int F) {
    const size_t T = (size_t)B * L;
    Saved v;
    v.qkv = s; v.ctx = v.qkv + T * 3 * D; v.u1 = v.ctx + T * D; v.h = v.u1 + T * D; v.u2 = v.h + T * F; v.p = v.u2 + T * D;
    return v;
}

// Builds the row table of tile t (the caller's barrier of the tile before has passed); returns its fill.  lens: 128 words of scratch.
__device__ __forceinline__ int build_table(const Args& a, int t, int* tok, int* s0, int* fill, int* lens) {
    const int tid = threadIdx.x, first = a.plan.first[t], cnt = a.plan.end[t] - first;
    if (tid < 64) { tok[tid] = 0; s0[tid] = -1; }
    if (tid < cnt) lens[tid] = clamp_len(a.seqlen, first + tid, a.L);
    __syncthreads();
    if (tid < cnt) {
        const int n = lens[tid];
        int r0 = 0;
        for (int i = 0; i < tid; ++i) r0 += lens[i];
        for (int k = 0; k < n && r0 + k < 64; ++k) { tok[r0 + k] = (first + tid) * a.L + k; s0[r0 + k] = r0; }      // (the plan keeps r0 + n <= 64)
        if (tid == cnt - 1) *fill = r0 + n < 64 ? r0 + n : 64;
    }
    __syncthreads();
    return *fill;
}
// does query row i admit key row j?
__device__ __forceinline__ bool admit(const int* s0, int causal, int i, int j) { return s0[j] >= 0 && s0[i] == s0[j] && (!causal || j <= i); }
// the (query row i, head h) row of the attention tensor [B][2][L][L]: index of its key position 0.  Valid for s0[i] >= 0.
__device__ __forceinline__ size_t attn_row(const int* tok, const int* s0, int L, int i, int h) {
    return (size_t)(tok[i] + tok[s0[i]] + h * L) * L;          // ((b 2 + h) L + pos_i) L, with b L = the token of the sequence's first row
}

// =================================================================================================================== forward
template <int D, int F>
__global__ __launch_bounds__(256) void k_packed_fwd(const Args a) {
    using G = Geo<D, F>;
    constexpr int LDX = G::LDX, LDF = G::LDF, DH = G::DH, HG = G::HG;
    extern __shared__ __align__(16) float lds[];
    float* As = lds;                       // x, then y1
    float* Bs = As + 64 * LDX;             // attention context, then the FFN output
    float* R = Bs + 64 * LDX;
    int* tok = reinterpret_cast<int*>(R + G::R_FLOATS);
    int* s0 = tok + 64;
    int* fill = s0 + 64;
    int* lens = fill + 4;                  // (the statistics' place; the forward keeps none)
    float *Qs = R, *Ks = R + TILE, *Vs = R + 2 * TILE, *Ss = R + 3 * TILE;
    const int tid = threadIdx.x, L = a.L;
    const RngKey rk = make_rng(a.seed, a.step, a.p);
    const bool drop = a.p > 0.f;
    const uint32_t s_attn = DR4SR_SITE_ATTN + 4 * a.layer, s_proj = DR4SR_SITE_PROJ + 4 * a.layer, s_act = DR4SR_SITE_ACT + 4 * a.layer,
                   s_ffn = DR4SR_SITE_FFN + 4 * a.layer;
    const float scale = 1.0f / sqrtf((float)DH);
    const int wv = tid >> 6, cg = wv >> 1;
    const FfnWeights fw = {a.w.linear1_weight, a.w.linear1_bias, a.w.linear2_weight, a.w.linear2_bias, a.w.norm2_weight, a.w.norm2_bias,
                           a.w.norm1_weight, a.w.norm1_bias};
    const bool sv = a.saved != nullptr;
    const Saved s = saved_view(a.saved, a.B, L, D, F);
    const int n_tiles = *a.plan.n_tiles;

    for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int n = build_table(a, t, tok, s0, fill, lens);
        load_rows_ix<D>(As, LDX, a.x, D, tok, n);
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
                for (int m = 0; m < 3; ++m) store_rows_ix<64>(s.qkv + m * D + g * 64, 3 * D, R + m * TILE, LDT, tok, n);
#pragma unroll
            for (int hh = 0; hh < HG; ++hh) {
                f32x16 acc[1];
                acc_zero(acc);
                mma_64xN_ld<DH, 1>(Qs + hh * DH, LDT, Ks + hh * DH, LDT, acc);
                acc_to_lds<1>(acc, Ss + hh * TILE, LDT, nullptr);
            }
            __syncthreads();
            // softmax + dropout: 4 lanes per query row, lane t4 takes keys t4, t4 + 4, ...
            for (int hh = 0; hh < HG; ++hh) {
                const int i = tid >> 2, t4 = tid & 3, h = g * HG + hh;
                float* srow = Ss + hh * TILE + i * LDT;
                float v[16], mx = -INFINITY;
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const int j = t4 + 4 * c;
                    v[c] = admit(s0, a.causal, i, j) ? srow[j] * scale : -INFINITY;
                    mx = fmaxf(mx, v[c]);
                }
                mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
                mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
                float sum = 0.f;
#pragma unroll
                for (int c = 0; c < 16; ++c) { v[c] = (mx == -INFINITY) ? 0.f : expf(v[c] - mx); sum += v[c]; }
                sum += __shfl_xor(sum, 1, 64);
                sum += __shfl_xor(sum, 2, 64);
                const float inv = (mx == -INFINITY || i >= n) ? 0.f : 1.0f / sum;
                const int si = s0[i];
                const size_t e0 = si >= 0 ? attn_row(tok, s0, L, i, h) : 0;
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const int j = t4 + 4 * c;
                    float pv = v[c] * inv;
                    if (si >= 0 && s0[j] == si) {              // a key of the query's own sequence: the dense op's (i, j) < L
                        const size_t e = e0 + (j - si);
                        if (sv) s.p[e] = pv;
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
        if (sv) store_rows_ix<D>(s.ctx, D, Bs, LDX, tok, n);
        // ---- out_proj -> R [64][LDX]
        {
            f32x16 acc[D / 64];
            acc_zero(acc);
            mma_64xN<D, D / 64>(Bs, LDX, a.w.out_proj_weight, acc);
            acc_to_lds<D / 64>(acc, R, LDX, a.w.out_proj_bias);
        }
        __syncthreads();
        // ---- u1 = x + drop(o), y1 = LN1(u1) -> As
        res_drop_ln_rows_ix<D, false>(As, LDX, As, R, LDX, a.w.norm1_weight, a.w.norm1_bias, sv ? s.u1 : nullptr, rk, drop, s_proj, tok, n, a.eps);
        __syncthreads();
        // ---- FFN, y = LN2(y1 + drop(f))
        ffn_fwd_ix<D, F, true>(As, Bs, LDX, R, LDF, fw, sv ? s.h : nullptr, sv ? s.u2 : nullptr, a.y, rk, drop, s_act, s_ffn, tok, n, a.eps);
        __syncthreads();
    }
}

// =================================================================================================================== backward
template <int D, int F>
__global__ __launch_bounds__(256) void k_packed_bwd(const Args a) {
    using G = Geo<D, F>;
    constexpr int LDX = G::LDX, LDF = G::LDF, DH = G::DH, HG = G::HG;
    extern __shared__ __align__(16) float lds[];
    float* As = lds;                       // dy -> du2 -> dy1 -> du1 -> d ctx
    float* Bs = As + 64 * LDX;             // u2 -> d f2 -> y1 -> u1 -> d o -> x
    float* R = Bs + 64 * LDX;
    int* tok = reinterpret_cast<int*>(R + G::R_FLOATS);
    int* s0 = tok + 64;
    int* fill = s0 + 64;
    float* st1 = reinterpret_cast<float*>(fill + 4);
    float* st2 = st1 + 128;
    float *Qs = R, *Ks = R + TILE, *Vs = R + 2 * TILE, *Ss = R + 3 * TILE, *Ds = R + (3 + HG) * TILE;
    const int tid = threadIdx.x, L = a.L;
    const RngKey rk = make_rng(a.seed, a.step, a.p);
    const bool drop = a.p > 0.f;
    const uint32_t s_attn = DR4SR_SITE_ATTN + 4 * a.layer, s_proj = DR4SR_SITE_PROJ + 4 * a.layer, s_act = DR4SR_SITE_ACT + 4 * a.layer,
                   s_ffn = DR4SR_SITE_FFN + 4 * a.layer;
    const float scale = 1.0f / sqrtf((float)DH);
    const int lane = tid & 63, wv = tid >> 6, r32 = lane & 31, g32 = lane >> 5, rh = wv & 1, cg = wv >> 1;
    float* ws = a.ws + (size_t)blockIdx.x * G::NW;
    const FfnWeights fw = {a.w.linear1_weight, a.w.linear1_bias, a.w.linear2_weight, a.w.linear2_bias, a.w.norm2_weight, a.w.norm2_bias,
                           a.w.norm1_weight, a.w.norm1_bias};
    const FfnGrads fg = {ws + G::O_W1, ws + G::O_B1, ws + G::O_W2, ws + G::O_B2, ws + G::O_N2W, ws + G::O_N2B};
    const Saved s = saved_view(a.saved, a.B, L, D, F);
    const int n_tiles = *a.plan.n_tiles;

    for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const bool first = t == (int)blockIdx.x;
        const int n = build_table(a, t, tok, s0, fill, reinterpret_cast<int*>(st1));
        // ---------------------------------------------------------------- A: LayerNorm 2 and the FFN
        ffn_ln_bwd_ix<D, F, true>(As, Bs, LDX, R, LDF, st1, st2, fw, s.u1, s.h, s.u2, a.dy, fg, rk, drop, s_act, s_ffn, tok, n, a.eps,
                                  first);              // dy1 -> As
        __syncthreads();
        // ---------------------------------------------------------------- B: LayerNorm 1 and out_proj
        load_rows_ix<D>(Bs, LDX, s.u1, D, tok, n);
        __syncthreads();
        ln_affine_grads<D>(ws + G::O_N1W, ws + G::O_N1B, As, Bs, LDX, st1, n, first);
        __syncthreads();
        // du1 -> the residual branch of dx (the attention branch is added at the end), d o = du1 * mask -> Bs
        ln_bwd_rows_ix<D>(As, Bs, LDX, st1, a.w.norm1_weight, a.dx, rk, drop, s_proj, tok, n);
        load_rows_ix<D>(R, LDX, s.ctx, D, tok, n);
        __syncthreads();
        wgrad_tn<D, D>(ws + G::O_OW, D, Bs, LDX, R, LDX, first);
        colsum(ws + G::O_OB, Bs, LDX, D, n, first);
        {
            f32x16 acc[D / 64];
            acc_zero(acc);
            mma_wT<D, D / 64>(Bs, LDX, a.w.out_proj_weight, D, acc);
            __syncthreads();
            acc_to_lds<D / 64>(acc, As, LDX, nullptr);        // d ctx
        }
        load_rows_ix<D>(Bs, LDX, a.x, D, tok, n);
        // ---------------------------------------------------------------- C: attention, group by group
        f32x16 dxacc[D / 64];
        acc_zero(dxacc);
        for (int g = 0; g < G::NG; ++g) {
            __syncthreads();
            for (int m = 0; m < 3; ++m) load_rows_ix<64>(R + m * TILE, LDT, s.qkv + m * D + g * 64, 3 * D, tok, n);
            for (int i = tid; i < HG * 64 * 64; i += 256) {
                const int hh = i >> 12, qi = (i >> 6) & 63, j = i & 63, si = s0[qi];
                Ss[hh * TILE + qi * LDT + j] = (si >= 0 && s0[j] == si) ? s.p[attn_row(tok, s0, L, qi, g * HG + hh) + (j - si)] : 0.f;
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
                const int i = tid >> 2, t4 = tid & 3, h = g * HG + hh, si = s0[i];
                const size_t e0 = si >= 0 ? attn_row(tok, s0, L, i, h) : 0;
                float* prow = Ss + hh * TILE + i * LDT;
                float* drow = Ds + hh * TILE + i * LDT;
                float pv[16], dp[16], dot = 0.f;
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const int j = t4 + 4 * c;
                    pv[c] = prow[j];
                    float m = 1.f;
                    if (drop && si >= 0 && s0[j] == si) m = drop1(rk, s_attn, e0 + (j - si));
                    dp[c] = drow[j] * m;
                    dot += dp[c] * pv[c];
                    prow[j] = pv[c] * m;
                }
                dot += __shfl_xor(dot, 1, 64);
                dot += __shfl_xor(dot, 2, 64);
#pragma unroll
                for (int c = 0; c < 16; ++c) drow[t4 + 4 * c] = scale * pv[c] * (dp[c] - dot);
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
                colsum(ws + G::O_INB + m * D + g * 64, R + m * TILE, LDT, 64, n, first);
                mma_wT<64, D / 64>(R + m * TILE, LDT, a.w.in_proj_weight + (size_t)(m * D + g * 64) * D, D, dxacc);
            }
        }
        __syncthreads();                                       // makes this workgroup's residual-branch stores to dx visible to it
#pragma unroll
        for (int i = 0; i < D / 64; ++i)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int row = rh * 32 + (q & 3) + 8 * (q >> 2) + 4 * g32;
                if (row < n) a.dx[(size_t)tok[row] * D + (cg + 2 * i) * 32 + r32] += dxacc[i][q];
            }
        __syncthreads();
    }
}

// out [B L][D] := 0 at pos >= n_b (the tile kernels write the rows in front of the lengths; nothing else writes y or dx).  A kernel, not
// hipMemsetAsync: as nodes of a captured graph the memsets of this file stored other values than 0 from the second replay on
// (tests/test_gpu_layer_packed.py replays one graph on two length sets), and only the pads need the stores
__global__ void k_zero_pads(float* __restrict__ out, const int64_t* __restrict__ seqlen, int64_t B, int L, int D) {
    const int C4 = D / 4;
    const int64_t n = B * L * C4;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = e / C4;
        if ((int)(t % L) >= clamp_len(seqlen, t / L, L)) st4(out + e * 4, make_float4(0.f, 0.f, 0.f, 0.f));
    }
}
static int launch_zero_pads(float* out, const int64_t* seqlen, int64_t B, int L, int D, hipStream_t st) {
    const int64_t blocks = (B * L * (D / 4) + 255) / 256;
    hipLaunchKernelGGL(k_zero_pads, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, st, out, seqlen, B, L, D);
    return DR4SR_LAUNCH_CHECK();
}

// adds the slots that the backward wrote — min(tiles, max_slots), the tile count read here — in index order
__global__ void k_packed_reduce(const float* __restrict__ slots, const int* __restrict__ n_tiles, int max_slots, int stride, ReduceTable t) {
    const int nt = *n_tiles;
    reduce_store(slots, nt < max_slots ? nt : max_slots, (size_t)stride, t.begin + blockIdx.x * blockDim.x + threadIdx.x, t);
}

// =================================================================================================================== host
static int64_t ws_bytes_needed(int64_t B, int D, int F, int backward) {
    return (plan_ints(B) + (backward ? (int64_t)n_slots(B) * slot_floats(D, F) : 0)) * 4;
}

template <int D, int F>
static int launch_fwd(const Args& a, hipStream_t st) {
    const size_t lds = PGeo<D, F>::LDS_FLOATS * sizeof(float);
    big_lds(k_packed_fwd<D, F>, lds);
    hipLaunchKernelGGL((k_packed_fwd<D, F>), dim3(n_slots(a.B)), dim3(256), lds, st, a);
    return DR4SR_LAUNCH_CHECK();
}
template <int D, int F>
static int launch_bwd(const Args& a, const dr4sr_layer_grads& dw, hipStream_t st) {
    using G = Geo<D, F>;
    const int off[13] = {G::O_INW, G::O_INB, G::O_OW, G::O_OB, G::O_W1, G::O_B1, G::O_W2, G::O_B2, G::O_N1W, G::O_N1B, G::O_N2W, G::O_N2B, G::NW};
    float* dst[12];
    memcpy(dst, &dw, sizeof dst);                              // the 12 gradients in the slot's order
    const size_t lds = PGeo<D, F>::LDS_FLOATS * sizeof(float);
    big_lds(k_packed_bwd<D, F>, lds);
    const int ns = n_slots(a.B);
    hipLaunchKernelGGL((k_packed_bwd<D, F>), dim3(ns), dim3(256), lds, st, a);
    int rc = DR4SR_LAUNCH_CHECK();
    if (rc) return rc;
    hipLaunchKernelGGL(k_packed_reduce, dim3((G::NW + 255) / 256), dim3(256), 0, st, a.ws, a.plan.n_tiles, ns, G::NW, reduce_table(dst, off, 12));
    return DR4SR_LAUNCH_CHECK();
}

}  // namespace lpk

extern "C" int64_t dr4sr_sasrec_layer_packed_saved_floats(int64_t B, int32_t L, int32_t D, int32_t H, int32_t F) {
    const int rc = lop::shape_check(B, L, D, H, F);
    if (rc) return rc;
    return lpk::saved_floats(B, L, D, F);
}

extern "C" int64_t dr4sr_sasrec_layer_packed_workspace_bytes(int64_t B, int32_t L, int32_t D, int32_t H, int32_t F, int32_t backward) {
    const int rc = lop::shape_check(B, L, D, H, F);
    if (rc) return rc;
    return lpk::ws_bytes_needed(B, D, F, backward != 0);
}

extern "C" int dr4sr_sasrec_layer_packed_fwd(const float* x, const int64_t* seqlen, int32_t causal, const dr4sr_layer_weights* w, int64_t B,
                                             int32_t L, int32_t D, int32_t H, int32_t F, float eps, float p_drop, uint64_t seed, uint32_t step,
                                             int32_t layer, float* y, float* saved, void* ws, int64_t ws_bytes, void* stream) {
    if (!lpk::all_set<12>(w) || !lpk::layer_args_ok(layer, p_drop, eps)) return DR4SR_E_ARG;
    const int rc = lop::shape_check(B, L, D, H, F);
    if (rc) return rc;
    if (B == 0) return 0;                                      // (an empty tensor's pointer may be null)
    if (!x || !y || !seqlen) return DR4SR_E_ARG;
    if (!ws || ws_bytes < lpk::ws_bytes_needed(B, D, F, 0)) return DR4SR_E_WS;
    hipStream_t st = (hipStream_t)stream;
    lpk::Args a{};
    a.x = x; a.seqlen = seqlen; a.causal = causal != 0; a.w = *w; a.B = B; a.L = L; a.eps = eps; a.p = p_drop; a.seed = seed; a.step = step;
    a.layer = layer; a.y = y; a.saved = saved; a.plan = lpk::plan_view(ws, B);
    int e = lpk::launch_zero_pads(y, seqlen, B, L, D, st);
    if (!e) e = lpk::launch_plan(seqlen, B, L, a.plan, nullptr, nullptr, st);
    if (e) return e;
    if (D == 64 && F == 128) return lpk::launch_fwd<64, 128>(a, st);
    if (D == 64) return lpk::launch_fwd<64, 256>(a, st);
    return lpk::launch_fwd<128, 128>(a, st);
}

extern "C" int dr4sr_sasrec_layer_packed_bwd(const float* x, const int64_t* seqlen, int32_t causal, const dr4sr_layer_weights* w, int64_t B,
                                             int32_t L, int32_t D, int32_t H, int32_t F, float eps, float p_drop, uint64_t seed, uint32_t step,
                                             int32_t layer, const float* saved, const float* dy, float* dx, const dr4sr_layer_grads* dw, void* ws,
                                             int64_t ws_bytes, void* stream) {
    if (!lpk::all_set<12>(w) || !lpk::all_set<12>(dw) || !lpk::layer_args_ok(layer, p_drop, eps)) return DR4SR_E_ARG;
    const int rc = lop::shape_check(B, L, D, H, F);
    if (rc) return rc;
    if (B > 0 && (!x || !seqlen || !saved || !dy || !dx)) return DR4SR_E_ARG;
    if (B > 0 && (!ws || ws_bytes < lpk::ws_bytes_needed(B, D, F, 1))) return DR4SR_E_WS;
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {                                              // no sequence: the gradients of the weights are zeros
        const dr4sr_layer_grads& g = *dw;
        const lpk::ZeroSpan t[12] = {{g.in_proj_weight, 3LL * D * D}, {g.in_proj_bias, 3LL * D}, {g.out_proj_weight, (int64_t)D * D},
                                     {g.out_proj_bias, D}, {g.linear1_weight, (int64_t)F * D}, {g.linear1_bias, F},
                                     {g.linear2_weight, (int64_t)D * F}, {g.linear2_bias, D}, {g.norm1_weight, D}, {g.norm1_bias, D},
                                     {g.norm2_weight, D}, {g.norm2_bias, D}};
        return lpk::zero_fill(t, 12, st);
    }
    lpk::Args a{};
    a.x = x; a.seqlen = seqlen; a.causal = causal != 0; a.w = *w; a.B = B; a.L = L; a.eps = eps; a.p = p_drop; a.seed = seed; a.step = step;
    a.layer = layer; a.saved = const_cast<float*>(saved); a.dy = dy; a.dx = dx; a.plan = lpk::plan_view(ws, B);
    a.ws = (float*)ws + lpk::plan_ints(B);
    int e = lpk::launch_zero_pads(dx, seqlen, B, L, D, st);
    if (!e) e = lpk::launch_plan(seqlen, B, L, a.plan, nullptr, nullptr, st);
    if (e) return e;
    if (D == 64 && F == 128) return lpk::launch_bwd<64, 128>(a, *dw, st);
    if (D == 64) return lpk::launch_bwd<64, 256>(a, *dw, st);
    return lpk::launch_bwd<128, 128>(a, *dw, st);
}

extern "C" int32_t dr4sr_sasrec_layer_packed_chunk(void) { return lpk::CHUNK; }

extern "C" int dr4sr_sasrec_layer_packed_plan(const int64_t* seqlen, int64_t B, int32_t L, int32_t* tile_of, int32_t* row_of, int32_t* n_tiles,
                                              void* ws, int64_t ws_bytes, void* stream) {
    if (B < 0 || L < 1 || !n_tiles) return DR4SR_E_ARG;
    if (L > 64) return DR4SR_E_SHAPE;
    if (B * (int64_t)L * L >= ((int64_t)1 << 30)) return DR4SR_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) return hip_ret(hipMemsetAsync(n_tiles, 0, sizeof(int32_t), st));
    if (!seqlen || !tile_of || !row_of) return DR4SR_E_ARG;
    if (!ws || ws_bytes < lpk::plan_ints(B) * 4) return DR4SR_E_WS;
    const lpk::Plan p = lpk::plan_view(ws, B);
    const int e = lpk::launch_plan(seqlen, B, L, p, tile_of, row_of, st);
    if (e) return e;
    return hip_ret(hipMemcpyAsync(n_tiles, p.n_tiles, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
}
