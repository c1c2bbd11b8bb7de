// regen.hip — dataset regeneration (DR4SR stage 3, the reference's 3.Hybrid_inference.py): batched greedy decode of the pre-trained
// regenerator (nn.Transformer d 64, 2 heads, 2 + 2 post-norm layers, FFN 256, erf-GELU) under each of its K conditions.
//
// The reference decodes ONE sequence at a time and recomputes the whole prefix at every step, with a host sync per token
// (3.Hybrid_inference.py:185-208).  Here a decode row is one (source, condition) pair and every launch covers all rows:
//   k_regen_encode   one workgroup per source row: 2 bidirectional encoder layers (key padding beyond src_len), encoder.norm,
//                    condition_linear[0] + ReLU, then per condition its 64 rows of condition_linear[2] (the memory) and both decoder
//                    layers' cross-attention K | V (multihead_attn.in_proj rows 64:192) into the workspace.  Runs once per source, not
//                    once per (source, condition, step) as in the reference.
//   k_regen_step     16 rows per workgroup, one step of both decoder layers for the newest token only: QKV of the new token appended to
//                    a per-row K | V cache (causal self-attention + post-norm make the cached prefix exactly what a full recompute
//                    gives), cross-attention over the row's memory with key padding, FFN, decoder.norm -> h.  Steps 0 and 1 also pick
//                    the token here: only ids of the row's source may be chosen, so the <= 50 source ids are scored directly.
//   k_regen_logits   steps >= 2: h @ E^T on MFMA 32x32x2 (64 rows x 512 items per workgroup, the table streamed from L2) with the
//                    masked arg-max fused in; the [R, n_rows] logits never exist.  Each tile's scores go through LDS to threads that
//                    keep a running maximum over 16 columns of one row (a ys-membership test only when a score would beat it), one
//                    64-bit atomicMax per (row, workgroup) on (key(score) << 32 | ~id): ties go to the lowest id whatever the launch order.
//   k_regen_pick     appends the winner, marks rows that emitted EOS or reached max_len - 1 tokens.
// Every per-row arithmetic sequence is independent of the row's tile and of the batch: a row decodes bit-identically alone or batched.
// Tiles whose rows have all finished exit at once.
#include "common.h"
#include "kernels.h"

extern __shared__ __attribute__((aligned(16))) float smem[];

namespace {

constexpr int RD = 64, RH = 2, RDH = 32, RF = 256, RNL = 2;
constexpr int LMAX = 50;       // position table rows = longest source
constexpr int TMAX = 25;       // self-attention cache positions (max_len <= 25)
constexpr int TR = 16;         // decode rows per step workgroup
constexpr int LG_TILES = 8;    // 64-item tiles per logits workgroup
constexpr int NT = 256;

// offsets of the flat layout (include/dr4sr_hip.h, DR4SR_REGEN_TENSORS entries)
enum { T_E = 0, T_P = 1, T_ENC = 2, T_ENC_NORM = 26, T_DEC = 28, T_DEC_NORM = 64, T_CL0W = 66, T_CL0B = 67, T_CL2W = 68, T_CL2B = 69 };
enum { E_INW, E_INB, E_OUTW, E_OUTB, E_W1, E_B1, E_W2, E_B2, E_N1W, E_N1B, E_N2W, E_N2B };
enum { D_SAINW, D_SAINB, D_SAOUTW, D_SAOUTB, D_CAINW, D_CAINB, D_CAOUTW, D_CAOUTB, D_W1, D_B1, D_W2, D_B2,
       D_N1W, D_N1B, D_N2W, D_N2B, D_N3W, D_N3B };

struct RegenOff { int64_t o[DR4SR_REGEN_TENSORS]; };

int64_t regen_layout(int32_t n_rows, int32_t K, int64_t* off) {
    int64_t sz[DR4SR_REGEN_TENSORS];
    int i = 0;
    sz[i++] = (int64_t)n_rows * RD;
    sz[i++] = (int64_t)LMAX * RD;
    for (int l = 0; l < RNL; ++l) {
        const int64_t s[12] = {3 * RD * RD, 3 * RD, RD * RD, RD, RF * RD, RF, RD * RF, RD, RD, RD, RD, RD};
        for (int j = 0; j < 12; ++j) sz[i++] = s[j];
    }
    sz[i++] = RD; sz[i++] = RD;
    for (int l = 0; l < RNL; ++l) {
        const int64_t s[18] = {3 * RD * RD, 3 * RD, RD * RD, RD, 3 * RD * RD, 3 * RD, RD * RD, RD, RF * RD, RF, RD * RF, RD,
                               RD, RD, RD, RD, RD, RD};
        for (int j = 0; j < 18; ++j) sz[i++] = s[j];
    }
    sz[i++] = RD; sz[i++] = RD;
    sz[i++] = (int64_t)K * RD * RD; sz[i++] = (int64_t)K * RD; sz[i++] = (int64_t)K * RD * K * RD; sz[i++] = (int64_t)K * RD;
    int64_t pos = 0;
    for (int j = 0; j < DR4SR_REGEN_TENSORS; ++j) { if (off) off[j] = pos; pos += sz[j]; }     // every size is a multiple of 4 floats
    return pos;
}

struct Ws {                      // workspace carve-up for R decode rows
    float* ckv;                  // [R][RNL][LMAX][2*RD]  cross-attention K | V
    float* skv;                  // [R][RNL][TMAX][2*RD]  self-attention K | V cache
    float* h;                    // [R][RD]               decoder output of the newest position
    unsigned long long* best;    // [R]                   arg-max key of the current step
    int* done;                   // [R]
};
int64_t ws_bytes(int64_t R) {
    return R * ((int64_t)RNL * LMAX * 2 * RD + (int64_t)RNL * TMAX * 2 * RD + RD) * 4 + R * 8 + R * 4;
}
Ws ws_carve(void* w, int64_t R) {
    Ws s;
    s.ckv = static_cast<float*>(w);
    s.skv = s.ckv + R * RNL * LMAX * 2 * RD;
    s.h = s.skv + R * RNL * TMAX * 2 * RD;
    s.best = reinterpret_cast<unsigned long long*>(s.h + R * RD);
    s.done = reinterpret_cast<int*>(s.best + R);
    return s;
}

__device__ __forceinline__ unsigned rg_f2key(float v) { const unsigned u = __float_as_uint(v); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ unsigned long long umax64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned long long shfl_xor64(unsigned long long v, int o) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    return ((unsigned long long)hi << 32) | lo;
}

// Y[r][o] = act(b[o] + sum_c X[r][c] W[o][c]) for r < NR, o < out; each thread owns one column o for RPT consecutive rows, so the
// weight row is read once per RPT rows and a row's sum runs in the same order in every tile.
template <int NR, int RPT, int ACT>   // ACT: 0 none, 1 ReLU, 2 erf-GELU
__device__ __forceinline__ void lin(const float* X, int ldx, int in, const float* __restrict__ W, const float* __restrict__ b, int out,
                                    float* Y, int ldy) {
    constexpr int G = NR / RPT;
    for (int idx = threadIdx.x; idx < out * G; idx += NT) {
        const int o = idx % out, r0 = (idx / out) * RPT;
        float acc[RPT];
#pragma unroll
        for (int q = 0; q < RPT; ++q) acc[q] = 0.f;
        const float* w = W + (size_t)o * in;
        for (int c = 0; c < in; c += 4) {
            const float4 wv = ld4(w + c);
#pragma unroll
            for (int q = 0; q < RPT; ++q) {
                const float4 xv = ld4(X + (r0 + q) * ldx + c);
                acc[q] = fmaf(xv.x, wv.x, acc[q]); acc[q] = fmaf(xv.y, wv.y, acc[q]);
                acc[q] = fmaf(xv.z, wv.z, acc[q]); acc[q] = fmaf(xv.w, wv.w, acc[q]);
            }
        }
        const float bo = b[o];
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
            float v = acc[q] + bo;
            if (ACT == 1) v = fmaxf(v, 0.f);
            if (ACT == 2) v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
            Y[(r0 + q) * ldy + o] = v;
        }
    }
}

// X[r] = LayerNorm(X[r] + A[r]) (A may be null) for r < NR; one wave per row, lane = feature
template <int NR>
__device__ __forceinline__ void add_ln(float* X, int ldx, const float* A, int lda, const float* __restrict__ w, const float* __restrict__ b,
                                       float eps) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int r = wv; r < NR; r += NT / 64) {
        float v = X[r * ldx + lane];
        if (A) v += A[r * lda + lane];
        const float mean = wave_sum(v) * (1.0f / RD);
        const float d = v - mean;
        const float var = wave_sum(d * d) * (1.0f / RD);
        X[r * ldx + lane] = d * rsqrtf(var + eps) * w[lane] + b[lane];
    }
}

// softmax over j < n of S[j] in place (n >= 1)
__device__ __forceinline__ void softmax_row(float* S, int n) {
    float m = -INFINITY;
    for (int j = 0; j < n; ++j) m = fmaxf(m, S[j]);
    float s = 0.f;
    for (int j = 0; j < n; ++j) { const float e = __expf(S[j] - m); S[j] = e; s += e; }
    const float inv = 1.0f / s;
    for (int j = 0; j < n; ++j) S[j] *= inv;
}

// ------------------------------------------------------------------------------------------------------------------- encode
constexpr int ELD = RD + 4;                        // LDS row stride of the 64-wide buffers
constexpr int EBIG = LMAX * 5 * RD;                // 16 000 floats: qkv + scores, FFN hidden, or condition_linear[0]'s output
constexpr size_t ENC_LDS = sizeof(float) * (3 * LMAX * ELD + EBIG);

__global__ __launch_bounds__(NT) void k_regen_encode(const float* __restrict__ P, RegenOff off, float eps, int n_rows, int K,
                                                     const int64_t* __restrict__ src, const int64_t* __restrict__ src_len, int Lsrc,
                                                     int64_t n_seq, int cond0, int n_cond, float* __restrict__ ckv) {
    float* X = smem;                               // [LMAX][ELD]
    float* T = X + LMAX * ELD;                     // [LMAX][ELD]
    float* M = T + LMAX * ELD;                     // [LMAX][ELD] memory of one condition
    float* BIG = M + LMAX * ELD;
    const int64_t s = blockIdx.x;
    const int Ls = (int)min<int64_t>(max<int64_t>(src_len[s], 1), Lsrc);
    const float* E = P + off.o[T_E];
    const float* Pos = P + off.o[T_P];
    for (int e = threadIdx.x; e < LMAX * RD; e += NT) {
        const int j = e / RD, c = e % RD;
        float v = 0.f;
        if (j < Ls) {
            const int64_t id = min<int64_t>(max<int64_t>(src[s * Lsrc + j], 0), n_rows - 1);
            v = E[id * RD + c] + Pos[j * RD + c];
        }
        X[j * ELD + c] = v;
    }
    __syncthreads();
    const float scale = rsqrtf((float)RDH);
    for (int l = 0; l < RNL; ++l) {
        const int64_t* lo = off.o + T_ENC + 12 * l;
        float* QKV = BIG;                          // [LMAX][3*RD]
        float* S = BIG + LMAX * 3 * RD;            // [RH][LMAX][LMAX]
        lin<LMAX, 2, 0>(X, ELD, RD, P + lo[E_INW], P + lo[E_INB], 3 * RD, QKV, 3 * RD);
        __syncthreads();
        for (int e = threadIdx.x; e < RH * LMAX * LMAX; e += NT) {      // bidirectional, keys < Ls
            const int h = e / (LMAX * LMAX), i = (e / LMAX) % LMAX, j = e % LMAX;
            float v = -INFINITY;
            if (j < Ls) {
                const float* q = QKV + i * 3 * RD + h * RDH;
                const float* k = QKV + j * 3 * RD + RD + h * RDH;
                float a = 0.f;
                for (int d = 0; d < RDH; ++d) a = fmaf(q[d], k[d], a);
                v = a * scale;
            }
            S[e] = v;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < RH * LMAX; e += NT) softmax_row(S + e * LMAX, Ls);
        __syncthreads();
        for (int e = threadIdx.x; e < LMAX * RD; e += NT) {
            const int i = e / RD, c = e % RD, h = c / RDH;
            const float* p = S + (h * LMAX + i) * LMAX;
            float a = 0.f;
            for (int j = 0; j < Ls; ++j) a = fmaf(p[j], QKV[j * 3 * RD + 2 * RD + c], a);
            T[i * ELD + c] = a;
        }
        __syncthreads();
        lin<LMAX, 2, 0>(T, ELD, RD, P + lo[E_OUTW], P + lo[E_OUTB], RD, M, ELD);
        __syncthreads();
        add_ln<LMAX>(X, ELD, M, ELD, P + lo[E_N1W], P + lo[E_N1B], eps);
        __syncthreads();
        lin<LMAX, 2, 2>(X, ELD, RD, P + lo[E_W1], P + lo[E_B1], RF, BIG, RF);
        __syncthreads();
        lin<LMAX, 2, 0>(BIG, RF, RF, P + lo[E_W2], P + lo[E_B2], RD, T, ELD);
        __syncthreads();
        add_ln<LMAX>(X, ELD, T, ELD, P + lo[E_N2W], P + lo[E_N2B], eps);
        __syncthreads();
    }
    add_ln<LMAX>(X, ELD, nullptr, 0, P + off.o[T_ENC_NORM], P + off.o[T_ENC_NORM + 1], eps);
    __syncthreads();
    const int KD = K * RD;
    lin<LMAX, 2, 1>(X, ELD, RD, P + off.o[T_CL0W], P + off.o[T_CL0B], KD, BIG, KD);   // KD <= 5 * 64 (checked on the host)
    __syncthreads();
    for (int c = 0; c < n_cond; ++c) {
        const int k = cond0 + c;
        lin<LMAX, 2, 0>(BIG, KD, KD, P + off.o[T_CL2W] + (size_t)k * RD * KD, P + off.o[T_CL2B] + k * RD, RD, M, ELD);
        __syncthreads();
        const int64_t row = (int64_t)c * n_seq + s;
        for (int l = 0; l < RNL; ++l) {
            const int64_t* lo = off.o + T_DEC + 18 * l;
            float* dst = ckv + (row * RNL + l) * LMAX * 2 * RD;
            lin<LMAX, 2, 0>(M, ELD, RD, P + lo[D_CAINW] + RD * RD, P + lo[D_CAINB] + RD, 2 * RD, dst, 2 * RD);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------------- decode
__global__ void k_regen_init(int64_t R, int max_len, int64_t sos, int64_t* __restrict__ tokens, int* __restrict__ len, Ws w) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    for (int j = 0; j < max_len; ++j) tokens[r * max_len + j] = j == 0 ? sos : 0;
    len[r] = 1;
    w.done[r] = 0;
    w.best[r] = 0ull;
}

constexpr int SLD = RD + 4;
struct alignas(16) StepLds {
    float x[TR * SLD];
    float t[TR * SLD];
    float q[TR * 3 * RD];
    float big[TR * RF];            // FFN hidden / attention probabilities [TR][RH][LMAX]
    int ys[TR][TMAX];
    int act[TR];
    int any;
};

__global__ __launch_bounds__(NT) void k_regen_step(const float* __restrict__ P, RegenOff off, float eps, int n_rows, int t,
                                                   const int64_t* __restrict__ src, const int64_t* __restrict__ src_len, int Lsrc,
                                                   int64_t n_seq, int64_t R, int max_len, const int64_t* __restrict__ tokens, Ws w) {
    __shared__ StepLds S;
    const int64_t r0 = (int64_t)blockIdx.x * TR;
    if (threadIdx.x == 0) S.any = 0;
    __syncthreads();
    if (threadIdx.x < TR) {
        const int64_t r = r0 + threadIdx.x;
        const int a = r < R && !w.done[r];
        S.act[threadIdx.x] = a;
        if (a) atomicOr(&S.any, 1);
    }
    for (int e = threadIdx.x; e < TR * TMAX; e += NT) {
        const int i = e / TMAX, j = e % TMAX;
        const int64_t r = r0 + i;
        S.ys[i][j] = (r < R && j <= t) ? (int)tokens[r * max_len + j] : -1;
    }
    __syncthreads();
    if (!S.any) return;
    const float* E = P + off.o[T_E];
    const float* Pos = P + off.o[T_P];
    for (int e = threadIdx.x; e < TR * RD; e += NT) {
        const int i = e / RD, c = e % RD;
        const int64_t id = min(max(S.ys[i][t], 0), n_rows - 1);
        S.x[i * SLD + c] = E[id * RD + c] + Pos[t * RD + c];
    }
    __syncthreads();
    const float scale = rsqrtf((float)RDH);
    for (int l = 0; l < RNL; ++l) {
        const int64_t* lo = off.o + T_DEC + 18 * l;
        // ---- causal self-attention over the cached prefix + the new token
        lin<TR, 4, 0>(S.x, SLD, RD, P + lo[D_SAINW], P + lo[D_SAINB], 3 * RD, S.q, 3 * RD);
        __syncthreads();
        for (int e = threadIdx.x; e < TR * 2 * RD; e += NT) {
            const int i = e / (2 * RD), c = e % (2 * RD);
            const int64_t r = r0 + i;
            if (r < R && S.act[i]) w.skv[((r * RNL + l) * TMAX + t) * 2 * RD + c] = S.q[i * 3 * RD + RD + c];
        }
        float* pr = S.big;                          // [TR][RH][LMAX]
        for (int e = threadIdx.x; e < TR * RH * (t + 1); e += NT) {
            const int i = e / (RH * (t + 1)), h = (e / (t + 1)) % RH, j = e % (t + 1);
            const int64_t r = r0 + i;
            const float* q = S.q + i * 3 * RD + h * RDH;
            const float* k = (j == t || r >= R) ? S.q + i * 3 * RD + RD + h * RDH
                                                : w.skv + ((r * RNL + l) * TMAX + j) * 2 * RD + h * RDH;
            float a = 0.f;
            for (int d = 0; d < RDH; ++d) a = fmaf(q[d], k[d], a);
            pr[(i * RH + h) * LMAX + j] = a * scale;
        }
        __syncthreads();
        if (threadIdx.x < TR * RH) softmax_row(pr + threadIdx.x * LMAX, t + 1);
        __syncthreads();
        for (int e = threadIdx.x; e < TR * RD; e += NT) {
            const int i = e / RD, c = e % RD, h = c / RDH;
            const int64_t r = r0 + i;
            const float* p = pr + (i * RH + h) * LMAX;
            float a = 0.f;
            for (int j = 0; j < t; ++j) a = fmaf(p[j], r < R ? w.skv[((r * RNL + l) * TMAX + j) * 2 * RD + RD + c] : 0.f, a);
            a = fmaf(p[t], S.q[i * 3 * RD + 2 * RD + c], a);
            S.t[i * SLD + c] = a;
        }
        __syncthreads();
        lin<TR, 4, 0>(S.t, SLD, RD, P + lo[D_SAOUTW], P + lo[D_SAOUTB], RD, S.q, RD);
        __syncthreads();
        add_ln<TR>(S.x, SLD, S.q, RD, P + lo[D_N1W], P + lo[D_N1B], eps);
        __syncthreads();
        // ---- cross-attention over the row's memory (keys < Ls)
        lin<TR, 4, 0>(S.x, SLD, RD, P + lo[D_CAINW], P + lo[D_CAINB], RD, S.q, RD);
        __syncthreads();
        for (int e = threadIdx.x; e < TR * RH * LMAX; e += NT) {
            const int i = e / (RH * LMAX), h = (e / LMAX) % RH, j = e % LMAX;
            const int64_t r = r0 + i;
            float v = -INFINITY;
            if (r < R) {
                const int Ls = (int)min<int64_t>(max<int64_t>(src_len[r % n_seq], 1), Lsrc);
                if (j < Ls) {
                    const float* q = S.q + i * RD + h * RDH;
                    const float* k = w.ckv + ((r * RNL + l) * LMAX + j) * 2 * RD + h * RDH;
                    float a = 0.f;
                    for (int d = 0; d < RDH; ++d) a = fmaf(q[d], k[d], a);
                    v = a * scale;
                }
            } else if (j == 0) v = 0.f;
            pr[(i * RH + h) * LMAX + j] = v;
        }
        __syncthreads();
        if (threadIdx.x < TR * RH) {
            const int64_t r = r0 + threadIdx.x / RH;
            const int Ls = r < R ? (int)min<int64_t>(max<int64_t>(src_len[r % n_seq], 1), Lsrc) : 1;
            softmax_row(pr + threadIdx.x * LMAX, Ls);
        }
        __syncthreads();
        for (int e = threadIdx.x; e < TR * RD; e += NT) {
            const int i = e / RD, c = e % RD, h = c / RDH;
            const int64_t r = r0 + i;
            float a = 0.f;
            if (r < R) {
                const int Ls = (int)min<int64_t>(max<int64_t>(src_len[r % n_seq], 1), Lsrc);
                const float* p = pr + (i * RH + h) * LMAX;
                for (int j = 0; j < Ls; ++j) a = fmaf(p[j], w.ckv[((r * RNL + l) * LMAX + j) * 2 * RD + RD + c], a);
            }
            S.t[i * SLD + c] = a;
        }
        __syncthreads();
        lin<TR, 4, 0>(S.t, SLD, RD, P + lo[D_CAOUTW], P + lo[D_CAOUTB], RD, S.q, RD);
        __syncthreads();
        add_ln<TR>(S.x, SLD, S.q, RD, P + lo[D_N2W], P + lo[D_N2B], eps);
        __syncthreads();
        // ---- FFN
        lin<TR, 4, 2>(S.x, SLD, RD, P + lo[D_W1], P + lo[D_B1], RF, S.big, RF);
        __syncthreads();
        lin<TR, 4, 0>(S.big, RF, RF, P + lo[D_W2], P + lo[D_B2], RD, S.t, SLD);
        __syncthreads();
        add_ln<TR>(S.x, SLD, S.t, SLD, P + lo[D_N3W], P + lo[D_N3B], eps);
        __syncthreads();
    }
    add_ln<TR>(S.x, SLD, nullptr, 0, P + off.o[T_DEC_NORM], P + off.o[T_DEC_NORM + 1], eps);
    __syncthreads();
    if (t >= 2) {
        for (int e = threadIdx.x; e < TR * RD; e += NT) {
            const int i = e / RD, c = e % RD;
            const int64_t r = r0 + i;
            if (r < R) w.h[r * RD + c] = S.x[i * SLD + c];
        }
        return;
    }
    // ---- steps 0 and 1 (3.Hybrid_inference.py:172-177, :197): only ids of the source that are not in ys; a wave per row, lane = source slot
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int i = wv; i < TR; i += NT / 64) {
        const int64_t r = r0 + i;
        if (r >= R || !S.act[i]) continue;
        const int64_t sq = r % n_seq;
        const int Ls = (int)min<int64_t>(max<int64_t>(src_len[sq], 1), Lsrc);
        unsigned long long key = 0ull;
        if (lane < Ls) {
            const int id = (int)min<int64_t>(max<int64_t>(src[sq * Lsrc + lane], 0), n_rows - 1);
            bool ok = true;
            for (int j = 0; j <= t; ++j) ok = ok && S.ys[i][j] != id;
            if (ok) {
                const float* e = E + (size_t)id * RD;
                float a = 0.f;
                for (int c = 0; c < RD; c += 4) {
                    const float4 ev = ld4(e + c);
                    a = fmaf(S.x[i * SLD + c], ev.x, a); a = fmaf(S.x[i * SLD + c + 1], ev.y, a);
                    a = fmaf(S.x[i * SLD + c + 2], ev.z, a); a = fmaf(S.x[i * SLD + c + 3], ev.w, a);
                }
                key = ((unsigned long long)rg_f2key(a) << 32) | (unsigned)(~(unsigned)id);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) key = umax64(key, shfl_xor64(key, o));
        if (lane == 0) w.best[r] = key;
    }
}

// h @ E^T + masked arg-max over all n_rows ids except the row's ys (steps >= 2)
__global__ __launch_bounds__(NT) void k_regen_logits(const float* __restrict__ E, int n_rows, int t, int64_t R, int max_len,
                                                     const int64_t* __restrict__ tokens, Ws w) {
    constexpr int LD = RD + 1;
    float* Hs = smem;                               // [64][LD]
    float* Es = Hs + 64 * LD;                       // [64][LD]
    int* ys = reinterpret_cast<int*>(Es + 64 * LD); // [64][TMAX]
    int* act = ys + 64 * TMAX;                      // [64] + any
    float* Ss = reinterpret_cast<float*>(act + 68); // [64][LD] scores of the current tile
    const int64_t b0 = (int64_t)blockIdx.y * 64;
    if (threadIdx.x == 0) act[64] = 0;
    __syncthreads();
    if (threadIdx.x < 64) {
        const int64_t r = b0 + threadIdx.x;
        const int a = r < R && !w.done[r];
        act[threadIdx.x] = a;
        if (a) atomicOr(&act[64], 1);
    }
    __syncthreads();
    if (!act[64]) return;
    for (int e = threadIdx.x; e < 64 * TMAX; e += NT) {
        const int i = e / TMAX, j = e % TMAX;
        const int64_t r = b0 + i;
        ys[e] = (r < R && j <= t) ? (int)tokens[r * max_len + j] : -1;
    }
    for (int e = threadIdx.x; e < 64 * (RD / 4); e += NT) {
        const int rr = e / (RD / 4), c = (e % (RD / 4)) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (b0 + rr < R) v = ld4(w.h + (b0 + rr) * RD + c);
        float* d = Hs + rr * LD + c; d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, g = lane >> 5;
    const int rt = wv >> 1, ct = wv & 1;
    const int row = threadIdx.x >> 2, qc = (threadIdx.x & 3) * 16;     // arg-max: a thread scans 16 columns of one row per tile
    float bv = -INFINITY;
    int bi = -1;
    const int ntile = (n_rows + 63) / 64, tile0 = blockIdx.x * LG_TILES;
    for (int tile = tile0; tile < tile0 + LG_TILES && tile < ntile; ++tile) {
        const int n0 = tile * 64;
        __syncthreads();                            // the previous tile's scan is done (first pass: Hs / ys are written)
        for (int e = threadIdx.x; e < 64 * (RD / 4); e += NT) {
            const int rr = e / (RD / 4), c = (e % (RD / 4)) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n0 + rr < n_rows) v = ld4(E + (size_t)(n0 + rr) * RD + c);
            float* d = Es + rr * LD + c; d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        __syncthreads();
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        const float* ap = Hs + (rt * 32 + r) * LD + g;
        const float* bp = Es + (ct * 32 + r) * LD + g;
#pragma unroll 8
        for (int k = 0; k < RD / 2; ++k) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * k], bp[2 * k], acc, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 16; ++e) Ss[(rt * 32 + (e & 3) + 8 * (e >> 2) + 4 * g) * LD + ct * 32 + r] = acc[e];
        __syncthreads();
        const float* sr = Ss + row * LD + qc;
        for (int c = 0; c < 16; ++c) {              // ids grow along a thread's scan: strict > keeps the lowest id of a tie
            const int n = n0 + qc + c;
            const float v = sr[c];
            if (n < n_rows && v > bv) {
                bool ok = true;
                for (int j = 0; j <= t; ++j) ok = ok && ys[row * TMAX + j] != n;
                if (ok) { bv = v; bi = n; }
            }
        }
    }
    unsigned long long key = bi >= 0 ? (((unsigned long long)rg_f2key(bv) << 32) | (unsigned)(~(unsigned)bi)) : 0ull;
    key = umax64(key, shfl_xor64(key, 1));
    key = umax64(key, shfl_xor64(key, 2));
    if ((threadIdx.x & 3) == 0 && key && act[row]) atomicMax(w.best + b0 + row, key);
}

__global__ void k_regen_pick(int64_t R, int t, int max_len, int eos, int64_t* __restrict__ tokens, int* __restrict__ len, Ws w) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R || w.done[r]) return;
    const unsigned long long key = w.best[r];
    w.best[r] = 0ull;
    if (!key) { w.done[r] = 1; return; }            // no allowed id (cannot happen with the reference's masks)
    const int id = (int)(~(unsigned)key);
    tokens[r * max_len + t + 1] = id;
    len[r] = t + 2;
    if (id == eos || t + 2 == max_len) w.done[r] = 1;
}

int check_plan(const dr4sr_regen_plan* p) {
    if (!p || p->abi_version != DR4SR_ABI_VERSION || !p->params) return DR4SR_E_ARG;
    if (p->D != RD || p->H != RH || p->F != RF || p->n_layer != RNL || p->max_len < 2 || p->max_len > TMAX) return DR4SR_E_SHAPE;
    if (p->K < 1 || p->K > 5 || p->n_rows < 3) return p->K > 5 ? DR4SR_E_SHAPE : DR4SR_E_ARG;
    if (p->n_params != regen_layout(p->n_rows, p->K, nullptr)) return DR4SR_E_ARG;
    return 0;
}

int check_call(const dr4sr_regen_plan* p, const int64_t* src, const int64_t* src_len, int64_t n_seq, int32_t Lsrc, int32_t cond0,
               int32_t n_cond, void* workspace, int64_t workspace_bytes) {
    if (const int rc = check_plan(p)) return rc;
    if (Lsrc > LMAX) return DR4SR_E_SHAPE;
    if (!src || !src_len || n_seq < 0 || Lsrc < 1 || cond0 < 0 || n_cond < 1 || cond0 + n_cond > p->K) return DR4SR_E_ARG;
    if (n_seq * n_cond >= (1LL << 26)) return DR4SR_E_ARG;
    if (!workspace || workspace_bytes < ws_bytes(n_seq * n_cond)) return DR4SR_E_WS;
    return 0;
}

RegenOff offsets_of(const dr4sr_regen_plan* p) {
    RegenOff o;
    regen_layout(p->n_rows, p->K, o.o);
    return o;
}

}  // namespace

extern "C" int dr4sr_regen_plan_sizeof(void) { return (int)sizeof(dr4sr_regen_plan); }

extern "C" int64_t dr4sr_regen_param_layout(int32_t n_rows, int32_t K, int64_t* offsets) {
    if (n_rows < 3 || K < 1) return DR4SR_E_ARG;
    return regen_layout(n_rows, K, offsets);
}

extern "C" int64_t dr4sr_regen_workspace_bytes(const dr4sr_regen_plan* plan, int64_t n_seq, int32_t n_cond) {
    if (const int rc = check_plan(plan)) return rc;
    if (n_seq < 0 || n_cond < 1 || n_cond > plan->K || n_seq * n_cond >= (1LL << 26)) return DR4SR_E_ARG;
    return ws_bytes(n_seq * n_cond);
}

extern "C" int dr4sr_regen_encode(const dr4sr_regen_plan* plan, const int64_t* src, const int64_t* src_len, int64_t n_seq, int32_t Lsrc,
                                  int32_t cond0, int32_t n_cond, void* workspace, int64_t workspace_bytes, void* stream) {
    if (const int rc = check_call(plan, src, src_len, n_seq, Lsrc, cond0, n_cond, workspace, workspace_bytes)) return rc;
    if (n_seq == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const Ws w = ws_carve(workspace, n_seq * n_cond);
    big_lds(k_regen_encode, ENC_LDS);
    hipLaunchKernelGGL(k_regen_encode, dim3((unsigned)n_seq), dim3(NT), ENC_LDS, s, plan->params, offsets_of(plan), plan->ln_eps,
                       plan->n_rows, plan->K, src, src_len, Lsrc, n_seq, cond0, n_cond, w.ckv);
    return DR4SR_LAUNCH_CHECK();
}

extern "C" int dr4sr_regen_decode(const dr4sr_regen_plan* plan, const int64_t* src, const int64_t* src_len, int64_t n_seq, int32_t Lsrc,
                                  int32_t cond0, int32_t n_cond, void* workspace, int64_t workspace_bytes, int64_t* tokens, int32_t* len,
                                  void* stream) {
    if (const int rc = check_call(plan, src, src_len, n_seq, Lsrc, cond0, n_cond, workspace, workspace_bytes)) return rc;
    if (!tokens || !len) return DR4SR_E_ARG;
    if (n_seq == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int64_t R = n_seq * n_cond;
    const Ws w = ws_carve(workspace, R);
    const RegenOff off = offsets_of(plan);
    const int ml = plan->max_len, nr = plan->n_rows;
    const unsigned g1 = (unsigned)((R + 255) / 256);
    hipLaunchKernelGGL(k_regen_init, dim3(g1), dim3(256), 0, s, R, ml, (int64_t)(nr - 2), tokens, len, w);
    if (const int rc = DR4SR_LAUNCH_CHECK()) return rc;
    const size_t lg_lds = sizeof(float) * 3 * 64 * (RD + 1) + sizeof(int) * (64 * TMAX + 68);
    big_lds(k_regen_logits, lg_lds);
    const dim3 lg_grid((unsigned)(((nr + 63) / 64 + LG_TILES - 1) / LG_TILES), (unsigned)((R + 63) / 64));
    for (int t = 0; t + 1 < ml; ++t) {
        hipLaunchKernelGGL(k_regen_step, dim3((unsigned)((R + TR - 1) / TR)), dim3(NT), 0, s, plan->params, off, plan->ln_eps, nr, t,
                           src, src_len, Lsrc, n_seq, R, ml, (const int64_t*)tokens, w);
        if (const int rc = DR4SR_LAUNCH_CHECK()) return rc;
        if (t >= 2) {
            hipLaunchKernelGGL(k_regen_logits, lg_grid, dim3(NT), lg_lds, s, plan->params + off.o[T_E], nr, t, R, ml,
                               (const int64_t*)tokens, w);
            if (const int rc = DR4SR_LAUNCH_CHECK()) return rc;
        }
        hipLaunchKernelGGL(k_regen_pick, dim3(g1), dim3(256), 0, s, R, t, ml, nr - 1, tokens, len, w);
    }
    return DR4SR_LAUNCH_CHECK();
}
