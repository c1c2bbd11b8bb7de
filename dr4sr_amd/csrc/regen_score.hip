// regen_score.hip — teacher-forced scoring of the regenerator (the forward and loss of DR4SR stage 2, the reference's
// 2.Pretrain_regenerator.py Generator.forward + CrossEntropyLoss(ignore_index=0) in eval mode), batched, fp32.
//
// A score row is (pair, condition weight vector): the per-token NLL of the pair's pattern given its sequence, with the K condition
// memories mixed by the row's weights.
//   k_rs_source  one workgroup per PAIR, the 64-row MFMA tile holds the source (<= 50 ids): 2 encoder layers (causal as stage 2 trains,
//                or bidirectional as stage 3 decodes; keys with id 0 masked), encoder.norm, condition_linear[0] + ReLU, then per
//                condition k its memory (64 rows of condition_linear[2]) and both decoder layers' cross-attention K | V of that memory
//                WITHOUT the bias, into the workspace.  The projection is linear, so a score row's K | V is sum_k w_k (K | V)_k + bias:
//                the source side runs once per pair whatever the number of weight vectors scored.
//   k_rs_scan    exclusive scan of the live token counts per pair (one workgroup).
//   k_rs_tile    the target side on packed tiles: the LIVE tokens of consecutive score rows (pair-major, the pair's weight vectors next
//                to each other) fill a 64-row tile; pad positions are never computed.  Projections and FFN on v_mfma_f32_32x32x2f32,
//                attention per row on the VALU.  MODE 1: the 2 decoder layers over the len(t) + 1 positions whose target is not PAD,
//                decoder.norm, logits against the <= 50 DISTINCT ids of the padded source row only (condition_mask), NLL.
//                MODE 0: the condition_encoder over min(len(t) + 2, T) positions, mean pooling (divides by len(t) + 2 even when the
//                matrix width cut the EOS), the two linears -> condition logits.
// Packing: score row r starts at global token index g_r (from the scan); tile b takes the rows with g_r in [b S, (b + 1) S),
// S = 65 - T, so a row never straddles two tiles and its tokens sit at slots g_r - b S ... < 64.  A row's arithmetic never depends on
// its slot or on its neighbours (every MFMA output row is a function of its own A row; every reduction runs in a fixed order), so a
// pair scores bit-identically alone, in any batch and in any order.  No floating-point atomics.
#include "common.h"
#include "kernels.h"

#include "regen_score_common.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------- source side
template <int KC>
__global__ __launch_bounds__(NT) void k_rs_source(const float* __restrict__ P, ScoreOff off, float eps, int n_rows,
                                                  const int64_t* __restrict__ src, const int64_t* __restrict__ src_len, int Ls, int causal,
                                                  float* __restrict__ ckv) {
    constexpr int KD = KC * RD, CLD = KD + 4;
    constexpr int USZ = (TM * CLD > TM * QLD + RH * LMAX * LMAX) ? TM * CLD : TM * QLD + RH * LMAX * LMAX;
    float* X = smem;                               // [64][XLD]
    float* T = X + TM * XLD;                       // [64][XLD]
    float* U = T + TM * XLD;                       // qkv + scores | out-proj | FFN hidden | condition_linear[0]'s output
    int* ids = reinterpret_cast<int*>(U + (USZ > TM * FLD ? USZ : TM * FLD));      // [64]
    const int64_t p = blockIdx.x;
    const int n = clampi(src_len[p], 1, Ls);
    const float* E = P + off.o[T_E];
    const float* Pos = P + off.o[T_P];
    if (threadIdx.x < TM) ids[threadIdx.x] = threadIdx.x < n ? clampi(src[p * Ls + threadIdx.x], 0, n_rows - 1) : 0;
    __syncthreads();
    for (int e = threadIdx.x; e < TM * RD; e += NT) {
        const int j = e / RD, c = e % RD;
        X[j * XLD + c] = j < n ? E[(size_t)ids[j] * RD + c] + Pos[j * RD + c] : 0.f;
    }
    __syncthreads();
    const float scale = rsqrtf((float)RDH);
    for (int l = 0; l < RNL; ++l) {
        const int64_t* lo = off.o + T_ENC + 12 * l;
        float* QKV = U;                            // [64][QLD]
        float* S = U + TM * QLD;                   // [RH][LMAX][LMAX]
        gemm64<RD, 3, 0>(X, XLD, P + lo[E_INW], P + lo[E_INB], QKV, QLD);
        __syncthreads();
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
        for (int e = threadIdx.x; e < RH * n; e += NT) softmax_masked(S + ((e / n) * LMAX + e % n) * LMAX, n);
        __syncthreads();
        for (int e = threadIdx.x; e < TM * RD; e += NT) {
            const int i = e / RD, c = e % RD, h = c / RDH;
            float a = 0.f;
            if (i < n) {
                const float* pr = S + (h * LMAX + i) * LMAX;
                for (int j = 0; j < n; ++j) a = fmaf(pr[j], QKV[j * QLD + 2 * RD + c], a);
            }
            T[i * XLD + c] = a;
        }
        __syncthreads();
        gemm64<RD, 1, 0>(T, XLD, P + lo[E_OUTW], P + lo[E_OUTB], U, XLD);
        __syncthreads();
        add_ln64(X, U, XLD, P + lo[E_N1W], P + lo[E_N1B], eps);
        __syncthreads();
        gemm64<RD, 4, 2>(X, XLD, P + lo[E_W1], P + lo[E_B1], U, FLD);
        __syncthreads();
        gemm64<RF, 1, 0>(U, FLD, P + lo[E_W2], P + lo[E_B2], T, XLD);
        __syncthreads();
        add_ln64(X, T, XLD, P + lo[E_N2W], P + lo[E_N2B], eps);
        __syncthreads();
    }
    add_ln64(X, nullptr, 0, P + off.o[T_ENC_NORM], P + off.o[T_ENC_NORM + 1], eps);
    __syncthreads();
    gemm64<RD, KC, 1>(X, XLD, P + off.o[T_CL0W], P + off.o[T_CL0B], U, CLD);
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, g = lane >> 5, rh = w & 1, cg = w >> 1;
    for (int k = 0; k < KC; ++k) {
        gemm64<KD, 1, 0>(U, CLD, P + off.o[T_CL2W] + (size_t)k * RD * KD, P + off.o[T_CL2B] + k * RD, T, XLD);     // memory of condition k
        __syncthreads();
        for (int l = 0; l < RNL; ++l) {
            const int64_t* lo = off.o + T_DEC + 18 * l;
            f32x16 acc[2];
            acc_zero(acc);
            mma_64xN<RD, 2>(T, XLD, P + lo[D_CAINW] + RD * RD, acc);          // in_proj rows 64:192 = K | V; the bias is added after the mix
            float* dst = ckv + (((p * KC + k) * RNL + l) * Ls) * (2 * RD);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int row = rh * 32 + (q & 3) + 8 * (q >> 2) + 4 * g;
                    if (row < Ls) dst[(size_t)row * (2 * RD) + (cg + 2 * i) * 32 + r] = acc[i][q];
                }
        }
        __syncthreads();
    }
}
template <int KC> constexpr size_t source_lds() {
    constexpr int CLD = KC * RD + 4;
    constexpr int a = TM * CLD, b = TM * QLD + RH * LMAX * LMAX, c = TM * FLD;
    constexpr int u = a > b ? (a > c ? a : c) : (b > c ? b : c);
    return sizeof(float) * (2 * TM * XLD + u) + sizeof(int) * TM;
}

template <int MODE>      // 0: condition encoder -> condition logits, 1: decoder -> per-token NLL
__global__ __launch_bounds__(NT) void k_rs_tile(const float* __restrict__ P, ScoreOff off, float eps, int n_rows, int K,
                                                const int64_t* __restrict__ src, const int64_t* __restrict__ src_len, int Ls,
                                                const int64_t* __restrict__ tgt, const int64_t* __restrict__ tgt_len, int n_pair, int T,
                                                const float* __restrict__ wts, int n_w, const int* __restrict__ cum, int S,
                                                const float* __restrict__ ckv, float* __restrict__ out) {
    __shared__ TileTab tb;
    float* X = smem;                               // [64][XLD]
    float* Tt = X + TM * XLD;                      // [64][XLD]
    float* U = Tt + TM * XLD;                      // [64][FLD]: qkv | cross-attention q | out-proj | FFN hidden
    float* PS = U + TM * FLD;                      // [64][RH][PLD] attention probabilities
    const int64_t lo_g = (int64_t)blockIdx.x * S, hi_g = lo_g + S;
    if (lo_g >= (int64_t)n_w * cum[n_pair]) return;
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
    const int n_row = tb.n_row;
    if (threadIdx.x < n_row) {
        const int r = threadIdx.x, p = tb.row_pair[r], base = tb.row_base[r], n = tb.row_n[r];
        tb.row_ls[r] = MODE == 1 ? clampi(src_len[p], 1, Ls) : 0;
        if (MODE == 1)
            for (int k = 0; k < K; ++k) tb.row_wt[r][k] = wts[((int64_t)tb.row_w[r] * n_pair + p) * K + k];
        for (int t = 0; t < n; ++t) {
            tb.tok_row[base + t] = r;
            tb.tok_pos[base + t] = t;
            tb.tok_id[base + t] = clampi(tgt[(int64_t)p * (T + 1) + t], 0, n_rows - 1);
            tb.tok_out[base + t] = clampi(tgt[(int64_t)p * (T + 1) + t + 1], 0, n_rows - 1);
        }
    }
    __syncthreads();
    const float* E = P + off.o[T_E];
    const float* Pos = P + off.o[T_P];
    for (int e = threadIdx.x; e < TM * RD; e += NT) {
        const int s = e / RD, c = e % RD;
        X[s * XLD + c] = tb.tok_row[s] >= 0 ? E[(size_t)tb.tok_id[s] * RD + c] + Pos[tb.tok_pos[s] * RD + c] : 0.f;
    }
    __syncthreads();
    const float scale = rsqrtf((float)RDH);
    for (int l = 0; l < RNL; ++l) {
        const int64_t* lo = off.o + (MODE == 1 ? T_DEC + 18 * l : T_CENC + 12 * l);
        // ---- causal self-attention (the first four tensors of an encoder and of a decoder layer are the same ones)
        gemm64<RD, 3, 0>(X, XLD, P + lo[E_INW], P + lo[E_INB], U, QLD);
        __syncthreads();
        self_attention(tb, U, PS, Tt, scale);
        __syncthreads();
        gemm64<RD, 1, 0>(Tt, XLD, P + lo[E_OUTW], P + lo[E_OUTB], U, XLD);
        __syncthreads();
        add_ln64(X, U, XLD, P + lo[MODE == 1 ? (int)D_N1W : (int)E_N1W], P + lo[MODE == 1 ? (int)D_N1B : (int)E_N1B], eps);
        __syncthreads();
        if (MODE == 1) {
            // ---- cross-attention over the row's mixed memory: K | V = sum_k w_k ckv_k + bias, mixed once per (row, head, key)
            gemm64<RD, 1, 0>(X, XLD, P + lo[D_CAINW], P + lo[D_CAINB], U, XLD);
            __syncthreads();
            const float* cb = P + lo[D_CAINB];
            for (int e = threadIdx.x; e < n_row * RH * LMAX; e += NT) {
                const int r = e / (RH * LMAX), h = (e / LMAX) % RH, j = e % LMAX;
                const int p = tb.row_pair[r], base = tb.row_base[r], n = tb.row_n[r];
                if (j >= tb.row_ls[r]) continue;
                const bool live = clampi(src[(int64_t)p * Ls + j], 0, n_rows - 1) != 0;
                float kv[RDH];
                if (live) {
#pragma unroll
                    for (int d = 0; d < RDH; ++d) kv[d] = 0.f;
                    for (int k = 0; k < K; ++k) {
                        const float wk = tb.row_wt[r][k];
                        const float* c = ckv + ((((int64_t)p * K + k) * RNL + l) * Ls + j) * (2 * RD) + h * RDH;
#pragma unroll
                        for (int d = 0; d < RDH; d += 4) {
                            const float4 v = ld4(c + d);
                            kv[d] = fmaf(wk, v.x, kv[d]); kv[d + 1] = fmaf(wk, v.y, kv[d + 1]);
                            kv[d + 2] = fmaf(wk, v.z, kv[d + 2]); kv[d + 3] = fmaf(wk, v.w, kv[d + 3]);
                        }
                    }
#pragma unroll
                    for (int d = 0; d < RDH; ++d) kv[d] += cb[RD + h * RDH + d];
                }
                for (int t = 0; t < n; ++t) {
                    float v = -INFINITY;
                    if (live) {
                        const float* q = U + (base + t) * XLD + h * RDH;
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
                const int s = threadIdx.x >> 1, r = tb.tok_row[s];
                if (r >= 0) softmax_masked(PS + threadIdx.x * PLD, tb.row_ls[r]);
            }
            __syncthreads();
            for (int e = threadIdx.x; e < TM * RD; e += NT) {
                if (tb.tok_row[e / RD] < 0) Tt[(e / RD) * XLD + e % RD] = 0.f;
            }
            for (int e = threadIdx.x; e < n_row * RD; e += NT) {
                const int r = e / RD, c = e % RD, h = c / RDH;
                const int p = tb.row_pair[r], base = tb.row_base[r], n = tb.row_n[r], ls = tb.row_ls[r];
                const float bv = cb[2 * RD + c];
                for (int t0 = 0; t0 < n; t0 += 8) {
                    float acc[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) acc[u] = 0.f;
                    for (int j = 0; j < ls; ++j) {
                        float v = 0.f;
                        for (int k = 0; k < K; ++k)
                            v = fmaf(tb.row_wt[r][k], ckv[((((int64_t)p * K + k) * RNL + l) * Ls + j) * (2 * RD) + RD + c], v);
                        v += bv;
#pragma unroll
                        for (int u = 0; u < 8; ++u)
                            if (t0 + u < n) acc[u] = fmaf(PS[((base + t0 + u) * RH + h) * PLD + j], v, acc[u]);
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (t0 + u < n) Tt[(base + t0 + u) * XLD + c] = acc[u];
                }
            }
            __syncthreads();
            gemm64<RD, 1, 0>(Tt, XLD, P + lo[D_CAOUTW], P + lo[D_CAOUTB], U, XLD);
            __syncthreads();
            add_ln64(X, U, XLD, P + lo[D_N2W], P + lo[D_N2B], eps);
            __syncthreads();
        }
        // ---- FFN
        gemm64<RD, 4, 2>(X, XLD, P + lo[MODE == 1 ? (int)D_W1 : (int)E_W1], P + lo[MODE == 1 ? (int)D_B1 : (int)E_B1], U, FLD);
        __syncthreads();
        gemm64<RF, 1, 0>(U, FLD, P + lo[MODE == 1 ? (int)D_W2 : (int)E_W2], P + lo[MODE == 1 ? (int)D_B2 : (int)E_B2], Tt, XLD);
        __syncthreads();
        add_ln64(X, Tt, XLD, P + lo[MODE == 1 ? (int)D_N3W : (int)E_N2W], P + lo[MODE == 1 ? (int)D_N3B : (int)E_N2B], eps);
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (MODE == 1) {
        add_ln64(X, nullptr, 0, P + off.o[T_DEC_NORM], P + off.o[T_DEC_NORM + 1], eps);
        __syncthreads();
        // ---- condition_mask + cross entropy (2.Pretrain_regenerator.py:180-184, :283): the softmax runs over the distinct ids of the
        // padded source row (PAD 0 included when the row is padded); a wave per token, lane = source slot
        for (int e = threadIdx.x; e < n_row * T; e += NT) {                  // the PAD columns of the tile's rows: every entry of nll is written
            const int r = e / T, t = e % T;
            if (t >= tb.row_n[r]) out[((int64_t)tb.row_w[r] * n_pair + tb.row_pair[r]) * T + t] = 0.f;
        }
        for (int s = wv; s < TM; s += NT / 64) {
            const int r = tb.tok_row[s];
            if (r < 0) continue;
            const int p = tb.row_pair[r], want = tb.tok_out[s];
            const int id = lane < Ls ? clampi(src[(int64_t)p * Ls + lane], 0, n_rows - 1) : -1;
            bool first = lane < Ls;
            for (int j = 0; j < Ls; ++j) {
                const int other = __shfl(id, j, 64);
                if (j < lane && other == id) first = false;
            }
            float a = 0.f;
            if (first) {
                const float* e = E + (size_t)id * RD;
                for (int c = 0; c < RD; c += 4) {
                    const float4 ev = ld4(e + c);
                    a = fmaf(X[s * XLD + c], ev.x, a); a = fmaf(X[s * XLD + c + 1], ev.y, a);
                    a = fmaf(X[s * XLD + c + 2], ev.z, a); a = fmaf(X[s * XLD + c + 3], ev.w, a);
                }
            }
            float m = first ? a : -INFINITY;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
            const float sum = wave_sum(first ? expf(a - m) : 0.f);
            const bool hit = first && id == want;
            const float tl = wave_sum(hit ? a : 0.f);                        // at most one lane holds the target id
            const bool any = __ballot(hit) != 0ull;
            if (lane == 0) {
                float v = 0.f;
                if (want != 0) v = any ? logf(sum) - (tl - m) : INFINITY;
                out[((int64_t)tb.row_w[r] * n_pair + p) * T + tb.tok_pos[s]] = v;
            }
        }
    } else {
        // ---- SeqPoolingLayer('mean'): the sum of the row's min(tgt_len, T) outputs over tgt_len, then condition_layer
        for (int e = threadIdx.x; e < TM * RD; e += NT) {
            const int r = e / RD, c = e % RD;
            float a = 0.f;
            if (r < n_row) {
                const int base = tb.row_base[r], n = tb.row_n[r];
                for (int t = 0; t < n; ++t) a += X[(base + t) * XLD + c];
                a = a / (float)max<int64_t>(tgt_len[tb.row_pair[r]], 1);
            }
            Tt[r * XLD + c] = a;
        }
        __syncthreads();
        gemm64<RD, 1, 1>(Tt, XLD, P + off.o[T_CC0W], P + off.o[T_CC0B], U, XLD);
        __syncthreads();
        for (int e = threadIdx.x; e < n_row * K; e += NT) {
            const int r = e / K, k = e % K;
            const float* wr = P + off.o[T_CC2W] + k * RD;
            float a = 0.f;
            for (int c = 0; c < RD; ++c) a = fmaf(U[r * XLD + c], wr[c], a);
            out[(int64_t)tb.row_pair[r] * K + k] = a + P[off.o[T_CC2B] + k];
        }
    }
}
constexpr size_t TILE_LDS = sizeof(float) * (2 * TM * XLD + TM * FLD + TM * RH * PLD);

// ------------------------------------------------------------------------------------------------------------------- host
template <int KC>
int launch_source(const dr4sr_regen_plan* plan, const int64_t* src, const int64_t* src_len, int64_t n_pair, int Ls, int causal, float* ckv,
                  hipStream_t s) {
    big_lds(k_rs_source<KC>, source_lds<KC>());
    hipLaunchKernelGGL(k_rs_source<KC>, dim3((unsigned)n_pair), dim3(NT), source_lds<KC>(), s, plan->params, offsets_of(plan), plan->ln_eps,
                       plan->n_rows, src, src_len, Ls, causal, ckv);
    return DR4SR_LAUNCH_CHECK();
}

}  // namespace

extern "C" int64_t dr4sr_regen_score_param_layout(int32_t n_rows, int32_t K, int64_t* offsets) {
    if (n_rows < 3 || K < 1) return DR4SR_E_ARG;
    return score_layout(n_rows, K, offsets);
}

extern "C" int64_t dr4sr_regen_score_workspace_bytes(const dr4sr_regen_plan* plan, int64_t n_pair, int32_t Ls, int32_t T, int32_t n_w) {
    if (const int rc = check_sizes(plan, n_pair, Ls, T, n_w)) return rc;
    return ws_bytes(n_pair, plan->K, Ls);
}

extern "C" int dr4sr_regen_score_condition(const dr4sr_regen_plan* plan, const int64_t* tgt, const int64_t* tgt_len, int64_t n_pair, int32_t T,
                                           void* workspace, int64_t workspace_bytes, float* cond_logits, void* stream) {
    if (const int rc = check_sizes(plan, n_pair, 1, T, 1)) return rc;
    if (!tgt || !tgt_len || !cond_logits) return DR4SR_E_ARG;
    if (!workspace || workspace_bytes < cum_bytes(n_pair)) return DR4SR_E_WS;
    if (n_pair == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    int* cum = static_cast<int*>(workspace);
    hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(1024), 0, s, tgt_len, (int)n_pair, T, 0, cum);
    if (const int rc = DR4SR_LAUNCH_CHECK()) return rc;
    const int S = TM + 1 - T;
    big_lds(k_rs_tile<0>, TILE_LDS);
    hipLaunchKernelGGL(k_rs_tile<0>, dim3((unsigned)((n_pair * T + S - 1) / S)), dim3(NT), TILE_LDS, s, plan->params, offsets_of(plan),
                       plan->ln_eps, plan->n_rows, plan->K, (const int64_t*)nullptr, (const int64_t*)nullptr, 1, tgt, tgt_len, (int)n_pair, T,
                       (const float*)nullptr, 1, (const int*)cum, S, (const float*)nullptr, cond_logits);
    return DR4SR_LAUNCH_CHECK();
}

extern "C" int dr4sr_regen_score(const dr4sr_regen_plan* plan, const int64_t* src, const int64_t* src_len, const int64_t* tgt,
                                 const int64_t* tgt_len, int64_t n_pair, int32_t Ls, int32_t T, const float* w, int32_t n_w,
                                 int32_t causal_source, void* workspace, int64_t workspace_bytes, float* nll, void* stream) {
    if (const int rc = check_sizes(plan, n_pair, Ls, T, n_w)) return rc;
    if (!src || !src_len || !tgt || !tgt_len || !w || !nll) return DR4SR_E_ARG;
    if (!workspace || workspace_bytes < ws_bytes(n_pair, plan->K, Ls)) return DR4SR_E_WS;
    if (n_pair == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    int* cum = static_cast<int*>(workspace);
    float* ckv = reinterpret_cast<float*>(static_cast<char*>(workspace) + cum_bytes(n_pair));
    hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(1024), 0, s, tgt_len, (int)n_pair, T, 1, cum);
    if (const int rc = DR4SR_LAUNCH_CHECK()) return rc;
    int rc = 0;
    switch (plan->K) {
        case 1: rc = launch_source<1>(plan, src, src_len, n_pair, Ls, causal_source != 0, ckv, s); break;
        case 2: rc = launch_source<2>(plan, src, src_len, n_pair, Ls, causal_source != 0, ckv, s); break;
        case 3: rc = launch_source<3>(plan, src, src_len, n_pair, Ls, causal_source != 0, ckv, s); break;
        case 4: rc = launch_source<4>(plan, src, src_len, n_pair, Ls, causal_source != 0, ckv, s); break;
        default: rc = launch_source<5>(plan, src, src_len, n_pair, Ls, causal_source != 0, ckv, s); break;
    }
    if (rc) return rc;
    const int S = TM + 1 - T;
    big_lds(k_rs_tile<1>, TILE_LDS);
    hipLaunchKernelGGL(k_rs_tile<1>, dim3((unsigned)((n_pair * n_w * T + S - 1) / S)), dim3(NT), TILE_LDS, s, plan->params, offsets_of(plan),
                       plan->ln_eps, plan->n_rows, plan->K, src, src_len, Ls, tgt, tgt_len, (int)n_pair, T, w, n_w, (const int*)cum, S,
                       (const float*)ckv, nll);
    return DR4SR_LAUNCH_CHECK();
}
