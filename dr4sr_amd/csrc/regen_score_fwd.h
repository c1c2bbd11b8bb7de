// regen_score_fwd.h — the one forward of teacher-forced scoring.  regen_score.hip runs it and stores the NLL / the condition logits;
// regen_score_bwd.hip runs the same functions again, keeping what its backward chain reads.  The two differ only in the KEEP policy
// every piece is templated on:
//   KeepNone   keeps nothing (the scoring kernels).
//   KeepRec    writes the activations into the slot records of the workspace: `rec` is the tile's (or the pair's) first record, `tf`
//              the record stride in floats, `rows` the number of records that exist (64 for a tile, Ls for a source row).
// A piece takes the record fields it would fill as a small struct of offsets; with KeepNone they are ignored ({} at the call).
// Next to it the DROP policy of regen_score_common.h: DropNone (eval mode; every piece is then what it was before the policy existed)
// or DropPhilox (train mode: the keep factors of the reference's dropout sites, applied in LDS right behind the operation that the
// reference drops, so the records KeepRec writes hold the post-dropout GEMM inputs).  `rows(s, pair, pos)` names the global pair and
// the position of tile row s, false for a row that holds no token (no factor is generated for it).
// Every float operation and its order is the same under both KEEP policies, with two exceptions that are kept as they were and marked
// "KEPT DIFFERENCE" below; both leave the values bit-identical on every input the tests and tools/regen_bits.py know.
#pragma once
#include <type_traits>

#include "regen_score_common.h"

namespace {

struct KeepNone {
    static constexpr bool on = false;
    __device__ __forceinline__ void save(const float*, int, int, int) const {}
    __device__ __forceinline__ void put(int, int, float) const {}
};
struct KeepRec {
    static constexpr bool on = true;
    float* rec;
    int tf, rows;
    // record r, floats [field, field + ncol) = row r of L
    __device__ __forceinline__ void save(const float* L, int ld, int field, int ncol) const {
        for (int e = threadIdx.x; e < rows * ncol; e += NT) rec[(size_t)(e / ncol) * tf + field + e % ncol] = L[(e / ncol) * ld + e % ncol];
    }
    __device__ __forceinline__ void put(int r, int field, float v) const {
        if (r < rows) rec[(size_t)r * tf + field] = v;
    }
};
struct SelfRec { int x, qkv, o, v; };      // a self-attention block: its input, q | k | v, the attention output, the LayerNorm's input
struct CrossRec { int x, q, o, v; };       // the cross-attention block: its input, q, the attention output, the LayerNorm's input
struct FfnRec { int x, hp, hh, v; };       // the FFN block: its input, the hidden layer before and after GELU, the LayerNorm's input
struct TailRec { int vn, memn, c1; };      // the source tail: encoder.norm's input and output, condition_linear[0]'s output

// the rows of a packed tile and of a source tile
struct TileRows {
    const TileTab& tb;
    int64_t pair0;
    __device__ __forceinline__ bool operator()(int s, int64_t& pair, int& pos) const {
        const int r = tb.tok_row[s];
        if (r < 0) return false;
        pair = pair0 + tb.row_pair[r]; pos = tb.tok_pos[s];
        return true;
    }
};
struct SrcRows {
    int64_t pair_;
    int n;
    __device__ __forceinline__ bool operator()(int s, int64_t& pair, int& pos) const {
        if (s >= n) return false;
        pair = pair_; pos = s;
        return true;
    }
};

__device__ __forceinline__ void mul8(float4& a, float4& b, const float4& lo, const float4& hi) {
    a.x *= lo.x; a.y *= lo.y; a.z *= lo.z; a.w *= lo.w;
    b.x *= hi.x; b.y *= hi.y; b.z *= hi.z; b.w *= hi.w;
}

// L[64][NC] *= the keep factors of `site` on the live rows: 8 columns per Philox call (NC = 64: a hidden site, 256: the FFN's)
template <int NC, class Rows>
__device__ __forceinline__ void drop_tile(const DropPhilox& dp, uint32_t site, float* L, int ld, const Rows& rows) {
    constexpr int G = NC / 8;
    for (int u = threadIdx.x; u < TM * G; u += NT) {
        const int s = u / G, c0 = (u % G) * 8;
        int64_t pair = 0;
        int pos = 0;
        if (!rows(s, pair, pos)) continue;
        float4 lo, hi;
        drop8(dp.k, site, (uint64_t)((pair * 64 + pos) * NC + c0), lo, hi);
        float4* x = reinterpret_cast<float4*>(L + s * ld + c0);
        float4 a = x[0], b = x[1];
        mul8(a, b, lo, hi);
        x[0] = a; x[1] = b;
    }
}

__device__ __forceinline__ float gelu_exact(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

// Y[64][ldy] = act(A[64][K] W^T + bias) on the 32x32x2 MFMA tiles of common.h (W global [64 NTW][K]); Y must not alias A
template <int K, int NTW, int ACT>     // ACT: 0 none, 1 ReLU, 2 erf-GELU
__device__ __forceinline__ void gemm64(const float* A, int lda, const float* __restrict__ W, const float* __restrict__ bias, float* Y, int ldy) {
    f32x16 acc[NTW];
    acc_zero(acc);
    mma_64xN<K, NTW>(A, lda, W, acc);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, g = lane >> 5, rh = w & 1, cg = w >> 1;
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        const int col = (cg + 2 * i) * 32 + r;
        const float bv = bias ? bias[col] : 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int row = rh * 32 + (q & 3) + 8 * (q >> 2) + 4 * g;
            float v = acc[i][q] + bv;
            if (ACT == 1) v = fmaxf(v, 0.f);
            if (ACT == 2) v = gelu_exact(v);
            Y[row * ldy + col] = v;
        }
    }
}

// X[r] = LayerNorm(X[r] + A[r]) (A may be null) for the 64 rows; one wave per row, lane = feature.  Keeps the LayerNorm's input.
template <class Keep>
__device__ __forceinline__ void add_ln64(const Keep& keep, float* X, const float* A, int lda, const float* __restrict__ w,
                                         const float* __restrict__ b, float eps, int field) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int r = wv; r < TM; r += NT / 64) {
        float v = X[r * XLD + lane];
        if (A) v += A[r * lda + lane];
        else if (Keep::on) v += 0.f;       // KEPT DIFFERENCE: the keeping kernels add a zero for a null A, which turns a -0 input into +0
        keep.put(r, field + lane, v);
        const float mean = wave_sum(v) * (1.0f / RD);
        const float d = v - mean;
        const float var = wave_sum(d * d) * (1.0f / RD);
        X[r * XLD + lane] = d * rsqrtf(var + eps) * w[lane] + b[lane];
    }
}
__device__ __forceinline__ void add_ln64(float* X, const float* A, int lda, const float* __restrict__ w, const float* __restrict__ b, float eps) {
    add_ln64(KeepNone(), X, A, lda, w, b, eps, 0);
}

// ------------------------------------------------------------------------------------------------------------------- the tile table
// The packed tile of workgroup blockIdx.x: the score rows (pair-major, a pair's n_w weight vectors next to each other) whose first token
// lies in [blockIdx.x S, (blockIdx.x + 1) S), and their slots.  False when the tile is beyond the last token (nothing was written, no
// barrier was passed).  MODE 1 (decoder) also takes the row's source length and weights.  KEPT DIFFERENCE: FULL = false is the
// condition encoder's backward, which never filled tok_out and row_ls; the scoring kernel fills them in MODE 0 too (tok_out unread,
// row_ls = 0).
template <int MODE, bool FULL>
__device__ __forceinline__ bool build_tile_tab(TileTab& tb, int n_rows, int K, const int64_t* src_len, int Ls,
                                               const int64_t* tgt, int n_pair, int T, const float* wts, int n_w,
                                               const int* cum, int S) {
    const int64_t lo_g = (int64_t)blockIdx.x * S, hi_g = lo_g + S;
    if (lo_g >= (int64_t)n_w * cum[n_pair]) return false;
    if (threadIdx.x < TM) tb.tok_row[threadIdx.x] = -1;
    if (threadIdx.x == 0) {
        int a = 0, b = n_pair;                     // the last pair whose first row starts at or before lo_g
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            if ((int64_t)n_w * cum[mid] <= lo_g) a = mid; else b = mid;
        }
        int nr = 0;
        for (int p = a; p < n_pair; ++p) {
            const int64_t base = (int64_t)n_w * cum[p];
            if (base >= hi_g) break;
            const int np = cum[p + 1] - cum[p];
            for (int i = 0; i < n_w; ++i) {
                const int64_t st = base + (int64_t)i * np;
                if (st < lo_g) continue;
                if (st >= hi_g) break;
                tb.row_pair[nr] = p; tb.row_w[nr] = i; tb.row_base[nr] = (int)(st - lo_g); tb.row_n[nr] = np;
                ++nr;
            }
        }
        tb.n_row = nr;
    }
    __syncthreads();
    if (threadIdx.x < tb.n_row) {
        const int r = threadIdx.x, p = tb.row_pair[r], base = tb.row_base[r], n = tb.row_n[r];
        if (FULL) tb.row_ls[r] = MODE == 1 ? clampi(src_len[p], 1, Ls) : 0;
        if (FULL && MODE == 1)
            for (int k = 0; k < K; ++k) tb.row_wt[r][k] = wts[((int64_t)tb.row_w[r] * n_pair + p) * K + k];
        for (int t = 0; t < n; ++t) {
            tb.tok_row[base + t] = r;
            tb.tok_pos[base + t] = t;
            tb.tok_id[base + t] = clampi(tgt[(int64_t)p * (T + 1) + t], 0, n_rows - 1);
            if (FULL) tb.tok_out[base + t] = clampi(tgt[(int64_t)p * (T + 1) + t + 1], 0, n_rows - 1);
        }
    }
    __syncthreads();
    return true;
}

// X[s] = E[id] + Pos[pos] for the rows that slot(s, id, pos) calls live, zero for the others
template <class Slot>
__device__ __forceinline__ void embed_rows(const float* E, const float* Pos, float* X, Slot slot) {
    for (int e = threadIdx.x; e < TM * RD; e += NT) {
        const int s = e / RD, c = e % RD;
        int id = 0, pos = 0;
        X[s * XLD + c] = slot(s, id, pos) ? E[(size_t)id * RD + c] + Pos[pos * RD + c] : 0.f;
    }
}
__device__ __forceinline__ void embed_tile(const float* E, const float* Pos, float* X, const TileTab& tb) {
    embed_rows(E, Pos, X, [&](int s, int& id, int& pos) {
        if (tb.tok_row[s] < 0) return false;
        id = tb.tok_id[s]; pos = tb.tok_pos[s];
        return true;
    });
}

// ------------------------------------------------------------------------------------------------------------------- layer blocks
// `lo` points at the layer's first tensor offset; a block takes the indices of its weights (each bias and LayerNorm bias follows its
// weight), so an encoder layer (E_*) and a decoder layer (D_*) run the same body.  X [64][XLD] is the residual stream, T [64][XLD] and
// U are scratch.  Every block ends behind a barrier.

// self-attention: attend() turns q | k | v in U [64][QLD] into the attention output in T
// (train mode: attend() drops the probabilities of site0 itself; the block drops its output, site0 + 1)
template <class Keep, class Drop, class Rows, class Attend>
__device__ __forceinline__ void self_block_fwd(const Keep& keep, const Drop& dp, uint32_t site0, const Rows& rows, SelfRec f, const float* P,
                                               const int64_t* lo, int inw, int outw, int nw, float eps, float* X, float* T, float* U,
                                               Attend attend) {
    keep.save(X, XLD, f.x, RD);
    gemm64<RD, 3, 0>(X, XLD, P + lo[inw], P + lo[inw + 1], U, QLD);
    __syncthreads();
    keep.save(U, QLD, f.qkv, 3 * RD);
    attend();
    __syncthreads();
    keep.save(T, XLD, f.o, RD);
    gemm64<RD, 1, 0>(T, XLD, P + lo[outw], P + lo[outw + 1], U, XLD);
    __syncthreads();
    if constexpr (Drop::on) {
        drop_tile<RD>(dp, site0 + 1, U, XLD, rows);
        __syncthreads();
    }
    add_ln64(keep, X, U, XLD, P + lo[nw], P + lo[nw + 1], eps, f.v);
    __syncthreads();
}

// KEPT DIFFERENCE: the scoring kernels apply GELU in the first GEMM's epilogue; the keeping kernels store the GEMM, then read it back to
// keep the hidden layer before and after GELU.  The value is the same float expression on the same float either way.
// Train mode drops the hidden layer behind GELU (site0; the record's f.hh holds the dropped values, the second GEMM's input) and the
// block's output (site0 + 1).
template <class Keep, class Drop, class Rows>
__device__ __forceinline__ void ffn_block_fwd(const Keep& keep, const Drop& dp, uint32_t site0, const Rows& rows, FfnRec f, const float* P,
                                              const int64_t* lo, int w1, int w2, int nw, float eps, float* X, float* T, float* U) {
    keep.save(X, XLD, f.x, RD);
    gemm64<RD, 4, Keep::on ? 0 : 2>(X, XLD, P + lo[w1], P + lo[w1 + 1], U, FLD);
    __syncthreads();
    if constexpr (Keep::on && Drop::on) {
        for (int u = threadIdx.x; u < TM * (RF / 8); u += NT) {
            const int s = u / (RF / 8), c0 = (u % (RF / 8)) * 8;
            int64_t pair = 0;
            int pos = 0;
            float4 lo4 = make_float4(1.f, 1.f, 1.f, 1.f), hi4 = lo4;
            if (rows(s, pair, pos)) drop8(dp.k, site0, (uint64_t)((pair * 64 + pos) * RF + c0), lo4, hi4);
            const float m[8] = {lo4.x, lo4.y, lo4.z, lo4.w, hi4.x, hi4.y, hi4.z, hi4.w};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float v = U[s * FLD + c0 + i];
                const float g = gelu_exact(v) * m[i];
                keep.put(s, f.hp + c0 + i, v);
                keep.put(s, f.hh + c0 + i, g);
                U[s * FLD + c0 + i] = g;
            }
        }
        __syncthreads();
    } else if constexpr (Drop::on) {
        drop_tile<RF>(dp, site0, U, FLD, rows);
        __syncthreads();
    } else if constexpr (Keep::on) {
        for (int e = threadIdx.x; e < TM * RF; e += NT) {
            const int s = e / RF, c = e % RF;
            const float v = U[s * FLD + c];
            const float g = gelu_exact(v);
            keep.put(s, f.hp + c, v);
            keep.put(s, f.hh + c, g);
            U[s * FLD + c] = g;
        }
        __syncthreads();
    }
    gemm64<RF, 1, 0>(U, FLD, P + lo[w2], P + lo[w2 + 1], T, XLD);
    __syncthreads();
    if constexpr (Drop::on) {
        drop_tile<RD>(dp, site0 + 1, T, XLD, rows);
        __syncthreads();
    }
    add_ln64(keep, X, T, XLD, P + lo[nw], P + lo[nw + 1], eps, f.v);
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------------------------- cross-attention
__device__ __forceinline__ bool src_live(const int64_t* __restrict__ src, int64_t p, int Ls, int j, int n_rows) {
    return clampi(src[p * Ls + j], 0, n_rows - 1) != 0;
}

// head h's 32 features at column `col` (0: K, RD: V) of the row's mixed memory at source position j, bias included:
// sum_k w_k ckv_k + bias, mixed once per (row, head, key)
__device__ __forceinline__ void mix_kv(const TileTab& tb, int r, int K, int Ls, int l, int j, int col, const float* __restrict__ ckv,
                                       const float* __restrict__ cb, float (&kv)[RDH]) {
    const int64_t p = tb.row_pair[r];
#pragma unroll
    for (int d = 0; d < RDH; ++d) kv[d] = 0.f;
    for (int k = 0; k < K; ++k) {
        const float wk = tb.row_wt[r][k];
        const float* c = ckv + (((p * K + k) * RNL + l) * Ls + j) * (2 * RD) + col;
#pragma unroll
        for (int d = 0; d < RDH; d += 4) {
            const float4 v = ld4(c + d);
            kv[d] = fmaf(wk, v.x, kv[d]); kv[d + 1] = fmaf(wk, v.y, kv[d + 1]);
            kv[d + 2] = fmaf(wk, v.z, kv[d + 2]); kv[d + 3] = fmaf(wk, v.w, kv[d + 3]);
        }
    }
#pragma unroll
    for (int d = 0; d < RDH; ++d) kv[d] += cb[RD + col + d];
}

// cross-attention probabilities of every live slot over its row's source positions (keys with id 0 masked); Q [64][XLD].
// Train mode: with KM null the probabilities are dropped in place (the forward: P . V takes the dropped ones); otherwise PS keeps the
// softmax itself and KM[slot RH + h] takes the row's keep bits (the backward, whose softmax Jacobian needs the undropped ones).
template <class Drop>
__device__ __forceinline__ void cross_probs(const Drop& dp, uint32_t site, unsigned long long* KM, const TileTab& tb, int n_row, int K, int Ls,
                                            int n_rows, int l, const int64_t* __restrict__ src, const float* __restrict__ ckv,
                                            const float* __restrict__ cb, const float* Q, float* PS, float scale) {
    for (int e = threadIdx.x; e < n_row * RH * LMAX; e += NT) {
        const int r = e / (RH * LMAX), h = (e / LMAX) % RH, j = e % LMAX;
        const int base = tb.row_base[r], n = tb.row_n[r];
        if (j >= tb.row_ls[r]) continue;
        const bool live = src_live(src, tb.row_pair[r], Ls, j, n_rows);
        float kv[RDH];
        if (live) mix_kv(tb, r, K, Ls, l, j, h * RDH, ckv, cb, kv);
        for (int t = 0; t < n; ++t) {
            float v = -INFINITY;
            if (live) {
                const float* q = Q + (base + t) * XLD + h * RDH;
                float a = 0.f;
#pragma unroll
                for (int d = 0; d < RDH; ++d) a = fmaf(q[d], kv[d], a);
                v = a * scale;
            }
            PS[((base + t) * RH + h) * PLD + j] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x < TM * RH) {
        const int r = tb.tok_row[threadIdx.x >> 1];
        if (r >= 0) {
            softmax_masked(PS + threadIdx.x * PLD, tb.row_ls[r]);
            if constexpr (Drop::on) {
                const int ls = tb.row_ls[r];
                const uint64_t km = prob_keep_bits(dp, site, dp.pair0 + tb.row_pair[r], threadIdx.x & 1, tb.tok_pos[threadIdx.x >> 1], ls);
                if (KM) KM[threadIdx.x] = km;
                else
                    for (int j = 0; j < ls; ++j) PS[threadIdx.x * PLD + j] = ((km >> j) & 1) ? PS[threadIdx.x * PLD + j] * dp.k.scale : 0.f;
            }
        }
    }
    __syncthreads();
}

// O [64][XLD] = the probabilities times the row's mixed V (a thread per (row, feature), 8 slots at a time); empty slots get zero
__device__ __forceinline__ void cross_out(const TileTab& tb, int n_row, int K, int Ls, int l, const float* __restrict__ ckv,
                                          const float* __restrict__ cb, const float* PS, float* O) {
    for (int e = threadIdx.x; e < TM * RD; e += NT)
        if (tb.tok_row[e / RD] < 0) O[(e / RD) * XLD + e % RD] = 0.f;
    for (int e = threadIdx.x; e < n_row * RD; e += NT) {
        const int r = e / RD, c = e % RD, h = c / RDH;
        const int64_t p = tb.row_pair[r];
        const int base = tb.row_base[r], n = tb.row_n[r], ls = tb.row_ls[r];
        const float bv = cb[2 * RD + c];
        for (int t0 = 0; t0 < n; t0 += 8) {
            float acc[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u] = 0.f;
            for (int j = 0; j < ls; ++j) {
                float v = 0.f;
                for (int k = 0; k < K; ++k) v = fmaf(tb.row_wt[r][k], ckv[(((p * K + k) * RNL + l) * Ls + j) * (2 * RD) + RD + c], v);
                v += bv;
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (t0 + u < n) acc[u] = fmaf(PS[((base + t0 + u) * RH + h) * PLD + j], v, acc[u]);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (t0 + u < n) O[(base + t0 + u) * XLD + c] = acc[u];
        }
    }
}

// the decoder layer's cross-attention over the row's mixed memory, K | V = sum_k w_k ckv_k + bias; PS [64][RH][PLD]
template <class Keep, class Drop, class Rows>
__device__ __forceinline__ void cross_block_fwd(const Keep& keep, const Drop& dp, uint32_t site0, const Rows& rows, CrossRec f, const TileTab& tb,
                                                int n_row, int K, int Ls, int n_rows, int l, const int64_t* __restrict__ src,
                                                const float* __restrict__ ckv, const float* P, const int64_t* lo, float eps, float* X, float* T,
                                                float* U, float* PS, float scale) {
    keep.save(X, XLD, f.x, RD);
    gemm64<RD, 1, 0>(X, XLD, P + lo[D_CAINW], P + lo[D_CAINB], U, XLD);
    __syncthreads();
    keep.save(U, XLD, f.q, RD);
    const float* cb = P + lo[D_CAINB];
    cross_probs(dp, site0, nullptr, tb, n_row, K, Ls, n_rows, l, src, ckv, cb, U, PS, scale);
    cross_out(tb, n_row, K, Ls, l, ckv, cb, PS, T);
    __syncthreads();
    keep.save(T, XLD, f.o, RD);
    gemm64<RD, 1, 0>(T, XLD, P + lo[D_CAOUTW], P + lo[D_CAOUTB], U, XLD);
    __syncthreads();
    if constexpr (Drop::on) {
        drop_tile<RD>(dp, site0 + 1, U, XLD, rows);
        __syncthreads();
    }
    add_ln64(keep, X, U, XLD, P + lo[D_N2W], P + lo[D_N2B], eps, f.v);
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------------------------- source side
// the source encoder's attention probabilities S[h][i][j] of one pair's n live positions (causal as stage 2 trains or bidirectional as
// stage 3 decodes; keys with id 0 masked); QKV [64][QLD].  Train mode with `apply`: dropped in place with the masks of (site, pair).
template <class Drop>
__device__ __forceinline__ void src_probs(const Drop& dp, uint32_t site, int64_t pair, bool apply, const float* QKV, float* S, const int* ids,
                                          int n, int causal, float scale) {
    for (int e = threadIdx.x; e < RH * n * LMAX; e += NT) {
        const int h = e / (n * LMAX), i = (e / LMAX) % n, j = e % LMAX;
        float v = -INFINITY;
        if (j < n && ids[j] != 0 && (!causal || j <= i)) {
            const float* q = QKV + i * QLD + h * RDH;
            const float* k = QKV + j * QLD + RD + h * RDH;
            float a = 0.f;
            for (int d = 0; d < RDH; ++d) a = fmaf(q[d], k[d], a);
            v = a * scale;
        }
        S[(h * LMAX + i) * LMAX + j] = v;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < RH * n; e += NT) {
        float* row = S + ((e / n) * LMAX + e % n) * LMAX;
        softmax_masked(row, n);
        if constexpr (Drop::on) {
            if (apply) {
                const uint64_t km = prob_keep_bits(dp, site, pair, e / n, e % n, n);
                for (int j = 0; j < n; ++j) row[j] = ((km >> j) & 1) ? row[j] * dp.k.scale : 0.f;
            }
        }
    }
    __syncthreads();
}

// O [64][XLD] = the probabilities times V; rows beyond n get zero
__device__ __forceinline__ void src_context(const float* QKV, const float* S, int n, float* O) {
    for (int e = threadIdx.x; e < TM * RD; e += NT) {
        const int i = e / RD, c = e % RD, h = c / RDH;
        float a = 0.f;
        if (i < n) {
            const float* pr = S + (h * LMAX + i) * LMAX;
            for (int j = 0; j < n; ++j) a = fmaf(pr[j], QKV[j * QLD + 2 * RD + c], a);
        }
        O[i * XLD + c] = a;
    }
}

// encoder.norm, condition_linear[0] + ReLU into U [64][KC RD + 4], then per condition k its memory (64 rows of condition_linear[2])
// into T, handed to use_memory(k) between two barriers
template <int KC, class Keep, class UseMemory>
__device__ __forceinline__ void source_tail_fwd(const Keep& keep, TailRec f, const float* P, const ScoreOff& off, float eps, float* X,
                                                float* T, float* U, UseMemory use_memory) {
    constexpr int KD = KC * RD, CLD = KD + 4;
    add_ln64(keep, X, nullptr, 0, P + off.o[T_ENC_NORM], P + off.o[T_ENC_NORM + 1], eps, f.vn);
    __syncthreads();
    keep.save(X, XLD, f.memn, RD);
    gemm64<RD, KC, 1>(X, XLD, P + off.o[T_CL0W], P + off.o[T_CL0B], U, CLD);
    __syncthreads();
    keep.save(U, CLD, f.c1, KD);
    for (int k = 0; k < KC; ++k) {
        gemm64<KD, 1, 0>(U, CLD, P + off.o[T_CL2W] + (size_t)k * RD * KD, P + off.o[T_CL2B] + k * RD, T, XLD);
        __syncthreads();
        use_memory(k);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------------- the two heads
// condition_mask (2.Pretrain_regenerator.py:180-184): the softmax of one token's decoder.norm output x [RD] runs over the DISTINCT ids
// of the padded source row (PAD 0 included when the row is padded).  A wave per token, lane = source slot: `first` marks the first
// occurrence of the lane's id, a its logit against E, m the maximum, ex = exp(a - m) (0 off the first occurrences), sum their total,
// hit the lane that holds the target id (at most one), any whether a lane does.
struct RLogit { int id; bool first, hit, any; float a, m, ex, sum; };
__device__ __forceinline__ RLogit restricted_logit(const float* E, const int64_t* src, int64_t p, int Ls, int n_rows,
                                                   const float* x, int want) {
    const int lane = threadIdx.x & 63;
    RLogit o;
    o.id = lane < Ls ? clampi(src[p * Ls + lane], 0, n_rows - 1) : -1;
    o.first = lane < Ls;
    for (int j = 0; j < Ls; ++j) {
        const int other = __shfl(o.id, j, 64);
        if (j < lane && other == o.id) o.first = false;
    }
    o.a = 0.f;
    if (o.first) {
        const float* e = E + (size_t)o.id * RD;
        for (int c = 0; c < RD; c += 4) {
            const float4 ev = ld4(e + c);
            o.a = fmaf(x[c], ev.x, o.a); o.a = fmaf(x[c + 1], ev.y, o.a);
            o.a = fmaf(x[c + 2], ev.z, o.a); o.a = fmaf(x[c + 3], ev.w, o.a);
        }
    }
    o.m = o.first ? o.a : -INFINITY;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) o.m = fmaxf(o.m, __shfl_xor(o.m, s, 64));
    o.ex = o.first ? expf(o.a - o.m) : 0.f;
    o.sum = wave_sum(o.ex);
    o.hit = o.first && o.id == want;
    o.any = __ballot(o.hit) != 0ull;
    return o;
}

// SeqPoolingLayer('mean') into T (row r of the tile in row r): the sum of the row's min(tgt_len, T) outputs over tgt_len, then
// condition_layer[0] + ReLU into U [64][XLD]
__device__ __forceinline__ void pool_and_hidden(const TileTab& tb, int n_row, const int64_t* tgt_len, const float* P,
                                                const ScoreOff& off, const float* X, float* T, float* U) {
    for (int e = threadIdx.x; e < TM * RD; e += NT) {
        const int r = e / RD, c = e % RD;
        float a = 0.f;
        if (r < n_row) {
            const int base = tb.row_base[r], n = tb.row_n[r];
            for (int t = 0; t < n; ++t) a += X[(base + t) * XLD + c];
            a = a / (float)max<int64_t>(tgt_len[tb.row_pair[r]], 1);
        }
        T[r * XLD + c] = a;
    }
    __syncthreads();
    gemm64<RD, 1, 1>(T, XLD, P + off.o[T_CC0W], P + off.o[T_CC0B], U, XLD);
    __syncthreads();
}

// the KC template for a plan's K (check_plan has K in 1 .. KMAX): f(std::integral_constant<int, K>())
template <class F>
int with_kc(int K, F f) {
    switch (K) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
        case 4: return f(std::integral_constant<int, 4>());
        default: return f(std::integral_constant<int, 5>());
    }
}

}  // namespace
