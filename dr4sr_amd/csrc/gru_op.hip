// gru_op.hip — the stateless GRU layer op (dr4sr_gru_layer_fwd / _bwd) on dense tensors: what torch.ops.dr4sr_hip.gru_layer runs.  One layer
// of torch.nn.GRU(bias=False, batch_first=True) (module/layers.py:117-136) on x [B, L, I], h0 = 0, gates ordered r | z | n in the 3H rows:
//     gi = x_t W_ih^T ; gh = h_{t-1} W_hh^T
//     r = sigmoid(gi_r + gh_r) ; z = sigmoid(gi_z + gh_z) ; n = tanh(gi_n + r gh_n) ; h_t = (1 - z) n + z h_{t-1}
// no plan, no device state words, no communication between workgroups inside a launch.  Token (b, t) is row b L + t of every [B L][.]
// matrix (64-bit); a sequence has seqlen[b] (clamped to [0, L]) or L steps, the steps behind it are skipped: y and dx are zero there, dy
// and x there are never read.
//
// Forward, two launches:
//   k_gru_op_gi<I>     gi = x W_ih^T into the workspace: 64-token x 128-column tiles on v_mfma_f32_32x32x2_f32, token tiles without a
//                      valid token are skipped
//   k_gru_op_fwd<H>    the recurrence, the form of gru.hip's k_gru_fwd<H>: a group of GS sequences per 512-thread workgroup (GS = 16, 8 or
//                      4 rows of the 16-row v_mfma_f32_16x16x4_f32 tile, the others zero), h in LDS [2][16][H + 4], W_hh streamed from L2
//                      every step; wave w owns hidden units [w H / 8, (w + 1) H / 8) of all three gates, so the gate math is register-local
// Saved for the backward: r, z, n, gh_n per computed token, [B L][4][H]; h_{t-1} is y shifted by one step.
//
// Backward, five launches:
//   k_gru_op_bwd<H>    BPTT in the same tiling (k_gru_bwd<H>): carry' = dh z + dgh W_hh; dgi = (dr, dz, dn) [B L][3H] and dn r [B L][H] into
//                      the workspace (dgh = (dr, dz, dn r))
//   k_gru_op_dx<I/64>  dx = dgi W_ih, 64-token tiles, the 3H reduction in chunks of 128 through LDS
//   k_gru_op_wgrad     dW_ih = dgi^T x and dW_hh = dgh^T h_prev: one workgroup per (64 x 64 block of a weight, token split) sums its
//                      split's 64-token tiles in order into its own slot of the workspace — no float atomics
//   k_slot_reduce      (op_tiles.h) adds the slots in index order and writes dw_ih and dw_hh: the same bits on every call
#include "common.h"
#include "op_tiles.h"

namespace gop {
using namespace optile;

constexpr int MAX_SPLITS = 32;         // token splits (= partial slots) of the weight-gradient launch
constexpr int MIN_SPLIT_TILES = 2;     // ... of at least this many 64-token tiles each
constexpr int LDT = 64 + 4;            // row stride of the weight-gradient launch's two [64][64] LDS tiles

struct Args {
    const float* x; const float* w_ih; const float* w_hh; const int64_t* seqlen;
    int64_t B; int L, I, H, GS;
    float* gi;                                   // workspace [B L][3H]
    float* y; float* saved;
    const float* dy; float* dgi; float* dnr;     // workspace [B L][3H], [B L][H]
    float* dx; float* slots; int64_t tiles_per_split;
};

__device__ __forceinline__ int len_of(const int64_t* __restrict__ sl, int64_t b, int L) {
    if (!sl) return L;
    const int64_t v = sl[b];
    return (int)(v < 0 ? 0 : (v > L ? L : v));
}
// the step of token tok inside its sequence, or -1 for a token behind the tensor or behind its sequence's length
__device__ __forceinline__ int step_of(const Args& a, int64_t tok, int64_t T) {
    if (tok >= T) return -1;
    const int64_t b = tok / a.L;
    const int t = (int)(tok - b * a.L);
    return t < len_of(a.seqlen, b, a.L) ? t : -1;
}

// ================================================================================================================ gi = x W_ih^T
template <int I>
__global__ __launch_bounds__(256) void k_gru_op_gi(const Args a) {
    extern __shared__ __align__(16) float lds[];               // [64][I + 4]
    constexpr int LDA = I + 4, C4 = I / 4;
    const int64_t T = a.B * a.L, t0 = (int64_t)blockIdx.x * 64;
    const int n0 = blockIdx.y * 128, G3 = 3 * a.H;
    int any = 0;
    for (int i = threadIdx.x; i < 64 * C4; i += 256) {
        const int row = i / C4, c = (i % C4) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (step_of(a, t0 + row, T) >= 0) { v = ld4(a.x + (size_t)(t0 + row) * I + c); any = 1; }
        st4(lds + row * LDA + c, v);
    }
    if (!__syncthreads_or(any)) return;                        // no valid token in the tile: nobody reads its gi
    f32x16 acc[2];
    acc_zero(acc);
    mma_64xN<I, 2>(lds, LDA, a.w_ih + (size_t)n0 * I, acc);
    const int64_t left = T - t0;
    acc_to_global<2>(acc, a.gi + (size_t)t0 * G3 + n0, G3, nullptr, 0, left < 64 ? (int)left : 64);
}

// ================================================================================================================ recurrence, forward
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// rows [0, GS) of the 16-row tile hold sequences b0 .. b0 + GS - 1; meta[row] = the sequence's length, -1 for a row without a sequence
__device__ __forceinline__ void group_meta(const Args& a, int* meta, int64_t b0) {
    if (threadIdx.x < 16) {
        const int64_t b = b0 + threadIdx.x;
        meta[threadIdx.x] = ((int)threadIdx.x < a.GS && b < a.B) ? len_of(a.seqlen, b, a.L) : -1;
    }
}

template <int H>
__global__ __launch_bounds__(512) void k_gru_op_fwd(const Args a) {
    extern __shared__ __align__(16) float lds[];
    constexpr int UT = H / 128;                           // 16-unit tiles per wave
    constexpr int LDH = H + 4, KQ = H / 4, G3 = 3 * H;    // lane group g contracts k in [g KQ, (g + 1) KQ)
    float* hb = lds;                                      // [2][16][LDH]
    int* meta = reinterpret_cast<int*>(hb + 2 * 16 * LDH);
    const int64_t b0 = (int64_t)blockIdx.x * a.GS;
    group_meta(a, meta, b0);
    for (int i = threadIdx.x; i < 2 * 16 * LDH; i += 512) hb[i] = 0.f;
    lds_barrier();
    // y behind a sequence's length is one contiguous run of zeros
    for (int s = 0; s < a.GS; ++s) {
        const int n = meta[s];
        if (n < 0) continue;
        float* p = a.y + ((size_t)(b0 + s) * a.L + n) * H;
        for (int i = threadIdx.x; i < (a.L - n) * (H / 4); i += 512) st4(p + 4 * i, make_float4(0.f, 0.f, 0.f, 0.f));
    }
    int nmax = 0;
#pragma unroll
    for (int s = 0; s < 16; ++s) nmax = max(nmax, meta[s]);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l16 = lane & 15, g = lane >> 4;
    int64_t tq[4];
    int nq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        nq[q] = max(meta[4 * g + q], 0);
        tq[q] = nq[q] > 0 ? (b0 + 4 * g + q) * a.L : 0;
    }
    const bool keep = a.saved != nullptr;
    f32x4 hreg[UT];
#pragma unroll
    for (int u = 0; u < UT; ++u) hreg[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < nmax; ++t) {
        const float* hc = hb + (t & 1) * 16 * LDH + l16 * LDH + g * KQ;       // A operand rows: sequence l16
        float* hn = hb + ((t + 1) & 1) * 16 * LDH;
        // the input-projection terms do not depend on the recurrence: requested before the MFMA loops
        float gir[UT][4], giz[UT][4], gin[UT][4];
#pragma unroll
        for (int u = 0; u < UT; ++u)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool act = t < nq[q];
                const float* gip = a.gi + (size_t)(tq[q] + (act ? t : 0)) * G3 + w * (H / 8) + u * 16 + l16;
                gir[u][q] = act ? gip[0] : 0.f; giz[u][q] = act ? gip[H] : 0.f; gin[u][q] = act ? gip[2 * H] : 0.f;
            }
#pragma unroll
        for (int u = 0; u < UT; ++u) {
            const int unit = w * (H / 8) + u * 16 + l16;                     // B operand row / C column of this lane
            f32x4 acc[3];
#pragma unroll
            for (int q3 = 0; q3 < 3; ++q3) acc[q3] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const float* wr = a.w_hh + (size_t)unit * H + g * KQ;
#pragma unroll 8
            for (int c = 0; c < KQ; c += 4) {
                const float4 av = ld4(hc + c);
#pragma unroll
                for (int q3 = 0; q3 < 3; ++q3) {
                    const float4 bv = ld4(wr + (size_t)q3 * H * H + c);
                    acc[q3] = mfma16(av.x, bv.x, acc[q3]);
                    acc[q3] = mfma16(av.y, bv.y, acc[q3]);
                    acc[q3] = mfma16(av.z, bv.z, acc[q3]);
                    acc[q3] = mfma16(av.w, bv.w, acc[q3]);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float hnew = hreg[u][q];
                if (t < nq[q]) {
                    const size_t tok = (size_t)(tq[q] + t);
                    const float rr = sigm(gir[u][q] + acc[0][q]);
                    const float zz = sigm(giz[u][q] + acc[1][q]);
                    const float nn = tanh_f(gin[u][q] + rr * acc[2][q]);
                    hnew = (1.0f - zz) * nn + zz * hreg[u][q];
                    if (keep) {
                        float* sv = a.saved + tok * (4 * H) + unit;
                        sv[0] = rr; sv[H] = zz; sv[2 * H] = nn; sv[3 * H] = acc[2][q];
                    }
                    a.y[tok * H + unit] = hnew;
                }
                hreg[u][q] = hnew;
                hn[(4 * g + q) * LDH + unit] = hnew;
            }
        }
        lds_barrier();
    }
}

// ================================================================================================================ recurrence, backward
// Per step (t descending): dh = dy[t] + carry; the gate derivatives of the wave's own units (registers); dgh rows -> LDS;
// carry' = dh z + dgh W_hh (MFMA, W_hh read column-wise: B[k = j][n = unit] = W_hh[j][unit]).
template <int H>
__global__ __launch_bounds__(512) void k_gru_op_bwd(const Args a) {
    extern __shared__ __align__(16) float lds[];
    constexpr int UT = H / 128, G3 = 3 * H, LDG = G3 + 4, KQ = G3 / 4;
    float* db = lds;                                      // [16][LDG]  dgh rows of the current step
    int* meta = reinterpret_cast<int*>(db + 16 * LDG);
    const int64_t b0 = (int64_t)blockIdx.x * a.GS;
    group_meta(a, meta, b0);
    lds_barrier();
    int nmax = 0;
#pragma unroll
    for (int s = 0; s < 16; ++s) nmax = max(nmax, meta[s]);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l16 = lane & 15, g = lane >> 4;
    int64_t tq[4];
    int nq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        nq[q] = max(meta[4 * g + q], 0);
        tq[q] = nq[q] > 0 ? (b0 + 4 * g + q) * a.L : 0;
    }
    f32x4 carry[UT];
#pragma unroll
    for (int u = 0; u < UT; ++u) carry[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // what a step reads from memory does not depend on the carry: loaded one step AHEAD, behind the previous step's MFMA loop
    float sv[UT][4][6];
    auto load_saved = [&](int t) {
#pragma unroll
        for (int u = 0; u < UT; ++u)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool act = t >= 0 && t < nq[q];
                const size_t tok = (size_t)(tq[q] + (act ? t : 0));
                const int unit = w * (H / 8) + u * 16 + l16;
                const float* s = a.saved + tok * (4 * H) + unit;
                sv[u][q][0] = act ? a.dy[tok * H + unit] : 0.f;
                sv[u][q][1] = act ? s[0] : 0.f; sv[u][q][2] = act ? s[H] : 0.f; sv[u][q][3] = act ? s[2 * H] : 0.f;
                sv[u][q][4] = act ? s[3 * H] : 0.f;
                sv[u][q][5] = (act && t > 0) ? a.y[(tok - 1) * H + unit] : 0.f;          // h_{t-1}
            }
    };
    load_saved(nmax - 1);
    for (int t = nmax - 1; t >= 0; --t) {
        f32x4 dhz[UT];
#pragma unroll
        for (int u = 0; u < UT; ++u) {
            const int unit = w * (H / 8) + u * 16 + l16;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float dr = 0.f, dz = 0.f, dn = 0.f, dnr = 0.f, keep = 0.f;
                if (t < nq[q]) {
                    const size_t tok = (size_t)(tq[q] + t);
                    const float dh = sv[u][q][0] + carry[u][q];
                    const float rr = sv[u][q][1], zz = sv[u][q][2], nn = sv[u][q][3], gh = sv[u][q][4], hp = sv[u][q][5];
                    dn = dh * (1.0f - zz) * (1.0f - nn * nn);
                    dz = dh * (hp - nn) * zz * (1.0f - zz);
                    dr = dn * gh * rr * (1.0f - rr);
                    dnr = dn * rr;
                    keep = dh * zz;
                    float* gp = a.dgi + tok * G3 + unit;
                    gp[0] = dr; gp[H] = dz; gp[2 * H] = dn;
                    a.dnr[tok * H + unit] = dnr;
                }
                dhz[u][q] = keep;
                float* row = db + (4 * g + q) * LDG + unit;
                row[0] = dr; row[H] = dz; row[2 * H] = dnr;
            }
        }
        lds_barrier();
        load_saved(t - 1);
        const float* ar = db + l16 * LDG + g * KQ;                      // A operand: dgh row of sequence l16
#pragma unroll
        for (int u = 0; u < UT; ++u) {
            const int unit = w * (H / 8) + u * 16 + l16;                // output column (hidden unit) of this lane
            f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
            const float* wc = a.w_hh + (size_t)(g * KQ) * H + unit;
#pragma unroll 8
            for (int c = 0; c < KQ; c += 4) {
                const float4 av = ld4(ar + c);
                acc = mfma16(av.x, wc[(size_t)c * H], acc);
                acc = mfma16(av.y, wc[(size_t)(c + 1) * H], acc);
                acc = mfma16(av.z, wc[(size_t)(c + 2) * H], acc);
                acc = mfma16(av.w, wc[(size_t)(c + 3) * H], acc);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) carry[u][q] = dhz[u][q] + acc[q];
        }
        lds_barrier();
    }
}

// ================================================================================================================ dx = dgi W_ih
template <int NTW>
__global__ __launch_bounds__(256) void k_gru_op_dx(const Args a) {
    extern __shared__ __align__(16) float lds[];               // [64][KC + 4]
    constexpr int KC = 128, LDA = KC + 4, I = 64 * NTW;
    __shared__ int valid[64];
    const int64_t T = a.B * a.L, t0 = (int64_t)blockIdx.x * 64;
    const int G3 = 3 * a.H;
    int v = 0;
    if (threadIdx.x < 64) { v = step_of(a, t0 + threadIdx.x, T) >= 0; valid[threadIdx.x] = v; }
    const int any = __syncthreads_or(v);
    const int64_t left = T - t0;
    const int rows = left < 64 ? (int)left : 64;
    f32x16 acc[NTW];
    acc_zero(acc);
    if (any)
        for (int k0 = 0; k0 < G3; k0 += KC) {
            for (int i = threadIdx.x; i < 64 * (KC / 4); i += 256) {
                const int row = i / (KC / 4), c = (i % (KC / 4)) * 4;
                st4(lds + row * LDA + c, valid[row] ? ld4(a.dgi + (size_t)(t0 + row) * G3 + k0 + c) : make_float4(0.f, 0.f, 0.f, 0.f));
            }
            __syncthreads();
            mma_wT<KC, NTW>(lds, LDA, a.w_ih + (size_t)k0 * I, I, acc);
            __syncthreads();
        }
    acc_to_global<NTW>(acc, a.dx + (size_t)t0 * I, I, nullptr, 0, rows);            // zero rows behind the lengths
}

// ================================================================================================================ weight gradients
// blockIdx.x: the 64 x 64 block (rows j0, columns k0) of dW_ih [3H][I], then of dW_hh [3H][H]; blockIdx.y: the token split.  A slot is
// dW_ih | dW_hh, row-major.  Wave w takes the 32 x 32 quadrant (w & 1, w >> 1).
__global__ __launch_bounds__(256) void k_gru_op_wgrad(const Args a) {
    extern __shared__ __align__(16) float lds[];
    float* As = lds;                       // [64 tokens][64 rows of the block]      dgi / dgh
    float* Bs = As + 64 * LDT;             // [64 tokens][64 columns of the block]   x / h_prev
    const int H = a.H, I = a.I, G3 = 3 * H;
    const int n_ih = (G3 / 64) * (I / 64);
    int tile = blockIdx.x;
    const bool hh = tile >= n_ih;
    if (hh) tile -= n_ih;
    const int KW = hh ? H : I, nk = KW / 64, j0 = (tile / nk) * 64, k0 = (tile % nk) * 64;
    const bool from_dnr = hh && j0 >= 2 * H;                   // dgh's n rows are dn r
    const float* Ag = from_dnr ? a.dnr + (j0 - 2 * H) : a.dgi + j0;
    const int ldg = from_dnr ? H : G3;
    const int64_t T = a.B * a.L, n_tiles = (T + 63) / 64;
    const int64_t tt0 = (int64_t)blockIdx.y * a.tiles_per_split;
    const int64_t tt1 = tt0 + a.tiles_per_split < n_tiles ? tt0 + a.tiles_per_split : n_tiles;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, g = lane >> 5, jq = w & 1, kq = w >> 1;
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    for (int64_t tt = tt0; tt < tt1; ++tt) {
        int any = 0;
        for (int i = threadIdx.x; i < 64 * 16; i += 256) {
            const int row = i >> 4, c = (i & 15) * 4;
            const int64_t tok = tt * 64 + row;
            const int t = step_of(a, tok, T);
            float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
            if (t >= 0) {
                any = 1;
                va = ld4(Ag + (size_t)tok * ldg + c);
                if (!hh) vb = ld4(a.x + (size_t)tok * I + k0 + c);
                else if (t > 0) vb = ld4(a.y + (size_t)(tok - 1) * H + k0 + c);
            }
            st4(As + row * LDT + c, va);
            st4(Bs + row * LDT + c, vb);
        }
        if (!__syncthreads_or(any)) continue;                  // a tile without a valid token adds nothing
        const float* ap = As + (g * 32) * LDT + jq * 32 + r;
        const float* bp = Bs + (g * 32) * LDT + kq * 32 + r;
#pragma unroll 8
        for (int k = 0; k < 32; ++k) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k * LDT], bp[k * LDT], acc, 0, 0, 0);
        __syncthreads();
    }
    float* out = a.slots + (size_t)blockIdx.y * ((size_t)G3 * (I + H)) + (hh ? (size_t)G3 * I : 0);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int row = j0 + jq * 32 + (q & 3) + 8 * (q >> 2) + 4 * g;
        out[(size_t)row * KW + k0 + kq * 32 + r] = acc[q];
    }
}

// ================================================================================================================ host
static int shape_check(int64_t B, int L, int I, int H) {
    if (B < 0 || B > (1 << 24)) return DR4SR_E_ARG;
    if ((I != 64 && I != 128 && I != 256) || (H != 128 && H != 256) || L < 1 || L > 1024) return DR4SR_E_SHAPE;
    return 0;
}
static int64_t n_tiles_of(int64_t B, int L) { return (B * L + 63) / 64; }
static int64_t tiles_per_split_of(int64_t B, int L) {
    const int64_t nt = n_tiles_of(B, L);
    int64_t s = nt / MIN_SPLIT_TILES;
    s = s < 1 ? 1 : (s > MAX_SPLITS ? MAX_SPLITS : s);
    return nt > 0 ? (nt + s - 1) / s : 1;                       // (B = 0: no tile, no split)
}
static int n_splits_of(int64_t B, int L) {
    const int64_t tps = tiles_per_split_of(B, L);
    return (int)((n_tiles_of(B, L) + tps - 1) / tps);
}
static int64_t ws_floats_of(int64_t B, int L, int I, int H, int backward) {
    const int64_t T = B * L;
    if (!backward) return T * 3 * H;
    return T * 4 * H + (int64_t)n_splits_of(B, L) * 3 * H * (I + H);
}
// Sequences per workgroup of the two recurrence launches.  A workgroup's step costs the same whatever the group size (the MFMA tile has
// 16 rows, W_hh is streamed once per step), so the smallest group that still leaves no more workgroups than CUs wins (NOTEBOOK);
// DR4SR_GRU_OP_GROUP = 4 | 8 | 16 overrides (the tests hold the sizes against each other)
static int group_of(int64_t B) {
    if (const char* e = DR4SR_ENV("DR4SR_GRU_OP_GROUP")) {
        const int v = atoi(e);
        if (v == 4 || v == 8 || v == 16) return v;
    }
    return B <= 4 * 256 ? 4 : (B <= 8 * 256 ? 8 : 16);
}

template <int H>
static int launch_rec(const Args& a, bool bwd, hipStream_t st) {
    const dim3 grid((unsigned)((a.B + a.GS - 1) / a.GS)), blk(512);
    if (!bwd) {
        const size_t lds = sizeof(float) * 2 * 16 * (H + 4) + 16 * sizeof(int);
        big_lds(k_gru_op_fwd<H>, lds);
        hipLaunchKernelGGL(k_gru_op_fwd<H>, grid, blk, lds, st, a);
    } else {
        const size_t lds = sizeof(float) * 16 * (3 * H + 4) + 16 * sizeof(int);
        big_lds(k_gru_op_bwd<H>, lds);
        hipLaunchKernelGGL(k_gru_op_bwd<H>, grid, blk, lds, st, a);
    }
    return DR4SR_LAUNCH_CHECK();
}

}  // namespace gop

extern "C" int64_t dr4sr_gru_layer_saved_floats(int64_t B, int32_t L, int32_t I, int32_t H) {
    const int rc = gop::shape_check(B, L, I, H);
    if (rc) return rc;
    return B * L * 4 * H;
}

extern "C" int64_t dr4sr_gru_layer_workspace_bytes(int64_t B, int32_t L, int32_t I, int32_t H, int32_t backward) {
    const int rc = gop::shape_check(B, L, I, H);
    if (rc) return rc;
    return gop::ws_floats_of(B, L, I, H, backward != 0) * (int64_t)sizeof(float);
}

extern "C" int dr4sr_gru_layer_fwd(const float* x, const float* w_ih, const float* w_hh, const int64_t* seqlen, int64_t B, int32_t L, int32_t I,
                                   int32_t H, float* y, float* saved, void* ws, int64_t ws_bytes, void* stream) {
    using namespace gop;
    if (!w_ih || !w_hh) return DR4SR_E_ARG;
    const int rc = shape_check(B, L, I, H);
    if (rc) return rc;
    if (B == 0) return 0;                                      // (an empty tensor's pointer may be null)
    if (!x || !y) return DR4SR_E_ARG;
    if (!ws || ws_bytes < ws_floats_of(B, L, I, H, 0) * (int64_t)sizeof(float)) return DR4SR_E_WS;
    hipStream_t st = (hipStream_t)stream;
    Args a{};
    a.x = x; a.w_ih = w_ih; a.w_hh = w_hh; a.seqlen = seqlen; a.B = B; a.L = L; a.I = I; a.H = H; a.GS = group_of(B);
    a.gi = (float*)ws; a.y = y; a.saved = saved;
    const dim3 grid((unsigned)n_tiles_of(B, L), 3 * H / 128);
    const size_t lds = sizeof(float) * 64 * (I + 4);
    if (I == 64) hipLaunchKernelGGL(k_gru_op_gi<64>, grid, dim3(256), lds, st, a);
    else if (I == 128) hipLaunchKernelGGL(k_gru_op_gi<128>, grid, dim3(256), lds, st, a);
    else { big_lds(k_gru_op_gi<256>, lds); hipLaunchKernelGGL(k_gru_op_gi<256>, grid, dim3(256), lds, st, a); }
    const int e = DR4SR_LAUNCH_CHECK();
    if (e) return e;
    return H == 256 ? launch_rec<256>(a, false, st) : launch_rec<128>(a, false, st);
}

extern "C" int dr4sr_gru_layer_bwd(const float* x, const float* w_ih, const float* w_hh, const int64_t* seqlen, int64_t B, int32_t L, int32_t I,
                                   int32_t H, const float* y, const float* saved, const float* dy, float* dx, float* dw_ih, float* dw_hh,
                                   void* ws, int64_t ws_bytes, void* stream) {
    using namespace gop;
    if (!w_ih || !w_hh || !dw_ih || !dw_hh) return DR4SR_E_ARG;
    const int rc = shape_check(B, L, I, H);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {                                              // no sequence: the gradients of the weights are zeros
        const ZeroSpan t[2] = {{dw_ih, (int64_t)3 * H * I}, {dw_hh, (int64_t)3 * H * H}};
        return zero_fill(t, 2, st);
    }
    if (!x || !y || !saved || !dy || !dx) return DR4SR_E_ARG;
    if (!ws || ws_bytes < ws_floats_of(B, L, I, H, 1) * (int64_t)sizeof(float)) return DR4SR_E_WS;
    const int64_t T = B * L;
    Args a{};
    a.x = x; a.w_ih = w_ih; a.w_hh = w_hh; a.seqlen = seqlen; a.B = B; a.L = L; a.I = I; a.H = H; a.GS = group_of(B);
    a.y = const_cast<float*>(y); a.saved = const_cast<float*>(saved); a.dy = dy; a.dx = dx;
    a.dgi = (float*)ws; a.dnr = a.dgi + T * 3 * H; a.slots = a.dnr + T * H; a.tiles_per_split = tiles_per_split_of(B, L);
    int e = H == 256 ? launch_rec<256>(a, true, st) : launch_rec<128>(a, true, st);
    if (e) return e;
    {
        const dim3 grid((unsigned)n_tiles_of(B, L));
        const size_t lds = sizeof(float) * 64 * (128 + 4);
        if (I == 64) hipLaunchKernelGGL(k_gru_op_dx<1>, grid, dim3(256), lds, st, a);
        else if (I == 128) hipLaunchKernelGGL(k_gru_op_dx<2>, grid, dim3(256), lds, st, a);
        else hipLaunchKernelGGL(k_gru_op_dx<4>, grid, dim3(256), lds, st, a);
        e = DR4SR_LAUNCH_CHECK();
        if (e) return e;
    }
    const int ns = n_splits_of(B, L), n_w = 3 * H * (I + H);
    hipLaunchKernelGGL(k_gru_op_wgrad, dim3((3 * H / 64) * ((I + H) / 64), ns), dim3(256), sizeof(float) * 2 * 64 * LDT, st, a);
    e = DR4SR_LAUNCH_CHECK();
    if (e) return e;
    float* dst[2] = {dw_ih, dw_hh};
    const int off[3] = {0, 3 * H * I, n_w};
    hipLaunchKernelGGL(k_slot_reduce, dim3((n_w + 255) / 256), dim3(256), 0, st, (const float*)a.slots, ns, n_w, reduce_table(dst, off, 2));
    return DR4SR_LAUNCH_CHECK();
}
