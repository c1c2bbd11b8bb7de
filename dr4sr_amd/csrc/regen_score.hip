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
// The forward itself is regen_score_fwd.h, shared with the backward (regen_score_bwd.hip): each kernel here is its set-up, the shared
// pieces with the KeepNone policy, and its own tail (the K | V projection of a condition's memory, the NLL or the logits store).
// Train mode (the *_train entry points): the same kernels instantiated with the DropPhilox policy, which they take as one more
// argument; the eval instantiations take none and are what they were.
#include "regen_score_fwd.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------- source side
template <int KC, class... D>          // D: nothing (eval mode) or DropPhilox
__global__ __launch_bounds__(NT) void k_rs_source(const float* __restrict__ P, ScoreOff off, float eps, int n_rows,
                                                  const int64_t* __restrict__ src, const int64_t* __restrict__ src_len, int Ls, int causal,
                                                  float* __restrict__ ckv, D... dpa) {
    const auto dp = pick_drop(dpa...);
    using Drop = std::remove_const_t<decltype(dp)>;
    constexpr int CLD = KC * RD + 4;
    constexpr int USZ = (TM * CLD > TM * QLD + RH * LMAX * LMAX) ? TM * CLD : TM * QLD + RH * LMAX * LMAX;
    float* X = smem;                               // [64][XLD]
    float* T = X + TM * XLD;                       // [64][XLD]
    float* U = T + TM * XLD;                       // qkv + scores | out-proj | FFN hidden | condition_linear[0]'s output
    int* ids = reinterpret_cast<int*>(U + (USZ > TM * FLD ? USZ : TM * FLD));      // [64]
    const int64_t p = blockIdx.x;
    const int n = clampi(src_len[p], 1, Ls);
    if (threadIdx.x < TM) ids[threadIdx.x] = threadIdx.x < n ? clampi(src[p * Ls + threadIdx.x], 0, n_rows - 1) : 0;
    __syncthreads();
    embed_rows(P + off.o[T_E], P + off.o[T_P], X, [&](int j, int& id, int& pos) { id = ids[j]; pos = j; return j < n; });
    __syncthreads();
    const SrcRows rows{dp.pair0 + p, n};
    if constexpr (Drop::on) {
        drop_tile<RD>(dp, DR4SR_REGEN_SITE_SRC_EMB, X, XLD, rows);
        __syncthreads();
    }
    const float scale = rsqrtf((float)RDH);
    const KeepNone keep;
    for (int l = 0; l < RNL; ++l) {
        const int64_t* lo = off.o + T_ENC + 12 * l;
        float* S = U + TM * QLD;                   // [RH][LMAX][LMAX] behind q | k | v [64][QLD]
        self_block_fwd(keep, dp, rs_site(ST_SRC, l, 0), rows, {}, P, lo, E_INW, E_OUTW, E_N1W, eps, X, T, U, [&] {
            src_probs(dp, rs_site(ST_SRC, l, 0), rows.pair_, true, U, S, ids, n, causal, scale);
            src_context(U, S, n, T);
        });
        ffn_block_fwd(keep, dp, rs_site(ST_SRC, l, 2), rows, {}, P, lo, E_W1, E_W2, E_N2W, eps, X, T, U);
    }
    source_tail_fwd<KC>(keep, {}, P, off, eps, X, T, U, [&](int k) {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, g = lane >> 5, rh = w & 1, cg = w >> 1;
        for (int l = 0; l < RNL; ++l) {            // both decoder layers' cross-attention K | V of the memory of condition k
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
    });
}
template <int KC> constexpr size_t source_lds() {
    constexpr int CLD = KC * RD + 4;
    constexpr int a = TM * CLD, b = TM * QLD + RH * LMAX * LMAX, c = TM * FLD;
    constexpr int u = a > b ? (a > c ? a : c) : (b > c ? b : c);
    return sizeof(float) * (2 * TM * XLD + u) + sizeof(int) * TM;
}

template <int MODE, class... D>      // 0: condition encoder -> condition logits, 1: decoder -> per-token NLL; D: nothing or DropPhilox
__global__ __launch_bounds__(NT) void k_rs_tile(const float* __restrict__ P, ScoreOff off, float eps, int n_rows, int K,
                                                const int64_t* __restrict__ src, const int64_t* __restrict__ src_len, int Ls,
                                                const int64_t* __restrict__ tgt, const int64_t* __restrict__ tgt_len, int n_pair, int T,
                                                const float* __restrict__ wts, int n_w, const int* __restrict__ cum, int S,
                                                const float* __restrict__ ckv, float* __restrict__ out, D... dpa) {
    const auto dp = pick_drop(dpa...);
    using Drop = std::remove_const_t<decltype(dp)>;
    __shared__ TileTab tb;
    float* X = smem;                               // [64][XLD]
    float* Tt = X + TM * XLD;                      // [64][XLD]
    float* U = Tt + TM * XLD;                      // [64][FLD]: qkv | cross-attention q | out-proj | FFN hidden
    float* PS = U + TM * FLD;                      // [64][RH][PLD] attention probabilities
    if (!build_tile_tab<MODE, true>(tb, n_rows, K, src_len, Ls, tgt, n_pair, T, wts, n_w, cum, S)) return;
    const int n_row = tb.n_row;
    const float* E = P + off.o[T_E];
    embed_tile(E, P + off.o[T_P], X, tb);
    __syncthreads();
    const TileRows rows{tb, dp.pair0};
    if constexpr (Drop::on) {          // the condition encoder and the decoder drop tgt_emb with ONE mask, as the reference drops it once
        drop_tile<RD>(dp, DR4SR_REGEN_SITE_TGT_EMB, X, XLD, rows);
        __syncthreads();
    }
    const float scale = rsqrtf((float)RDH);
    const KeepNone keep;
    constexpr int ST = MODE == 1 ? (int)ST_DEC : (int)ST_COND;
    // the first four tensors of an encoder and of a decoder layer are the same ones; the FFN and the norms sit elsewhere
    constexpr int N1 = MODE == 1 ? (int)D_N1W : (int)E_N1W, W1 = MODE == 1 ? (int)D_W1 : (int)E_W1, W2 = MODE == 1 ? (int)D_W2 : (int)E_W2,
                  NF = MODE == 1 ? (int)D_N3W : (int)E_N2W;
    for (int l = 0; l < RNL; ++l) {
        const int64_t* lo = off.o + (MODE == 1 ? T_DEC + 18 * l : T_CENC + 12 * l);
        self_block_fwd(keep, dp, rs_site(ST, l, 0), rows, {}, P, lo, E_INW, E_OUTW, N1, eps, X, Tt, U,
                       [&] { self_attention(dp, rs_site(ST, l, 0), tb, U, PS, Tt, scale); });
        if (MODE == 1) cross_block_fwd(keep, dp, rs_site(ST_DEC, l, 2), rows, {}, tb, n_row, K, Ls, n_rows, l, src, ckv, P, lo, eps, X, Tt, U, PS, scale);
        ffn_block_fwd(keep, dp, rs_site(ST, l, MODE == 1 ? 4 : 2), rows, {}, P, lo, W1, W2, NF, eps, X, Tt, U);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (MODE == 1) {
        add_ln64(X, nullptr, 0, P + off.o[T_DEC_NORM], P + off.o[T_DEC_NORM + 1], eps);
        __syncthreads();
        // ---- cross entropy over the restricted softmax (2.Pretrain_regenerator.py:283); a wave per token
        for (int e = threadIdx.x; e < n_row * T; e += NT) {                  // the PAD columns of the tile's rows: every entry of nll is written
            const int r = e / T, t = e % T;
            if (t >= tb.row_n[r]) out[((int64_t)tb.row_w[r] * n_pair + tb.row_pair[r]) * T + t] = 0.f;
        }
        for (int s = wv; s < TM; s += NT / 64) {
            const int r = tb.tok_row[s];
            if (r < 0) continue;
            const int p = tb.row_pair[r], want = tb.tok_out[s];
            const RLogit g = restricted_logit(E, src, p, Ls, n_rows, X + s * XLD, want);
            const float tl = wave_sum(g.hit ? g.a : 0.f);                    // at most one lane holds the target id
            if (lane == 0) {
                float v = 0.f;
                if (want != 0) v = g.any ? logf(g.sum) - (tl - g.m) : INFINITY;
                out[((int64_t)tb.row_w[r] * n_pair + p) * T + tb.tok_pos[s]] = v;
            }
        }
    } else {
        pool_and_hidden(tb, n_row, tgt_len, P, off, X, Tt, U);
        for (int e = threadIdx.x; e < n_row * K; e += NT) {                  // condition_layer[2]
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
template <int KC, class... D>
int launch_source(const dr4sr_regen_plan* plan, const int64_t* src, const int64_t* src_len, int64_t n_pair, int Ls, int causal, float* ckv,
                  hipStream_t s, D... dp) {
    big_lds(k_rs_source<KC, D...>, source_lds<KC>());
    hipLaunchKernelGGL((k_rs_source<KC, D...>), dim3((unsigned)n_pair), dim3(NT), source_lds<KC>(), s, plan->params, offsets_of(plan),
                       plan->ln_eps, plan->n_rows, src, src_len, Ls, causal, ckv, dp...);
    return DR4SR_LAUNCH_CHECK();
}

// the two entry points with the dropout policy as a trailing argument pack: nothing (eval mode) or one DropPhilox
template <class... D>
int score_condition(const dr4sr_regen_plan* plan, const int64_t* tgt, const int64_t* tgt_len, int64_t n_pair, int32_t T, void* workspace,
                    int64_t workspace_bytes, float* cond_logits, void* stream, D... dp) {
    if (const int rc = check_sizes(plan, n_pair, 1, T, 1)) return rc;
    if (!tgt || !tgt_len || !cond_logits) return DR4SR_E_ARG;
    if (!workspace || workspace_bytes < cum_bytes(n_pair)) return DR4SR_E_WS;
    if (n_pair == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    int* cum = static_cast<int*>(workspace);
    hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(1024), 0, s, tgt_len, (int)n_pair, T, 0, cum);
    if (const int rc = DR4SR_LAUNCH_CHECK()) return rc;
    const int S = TM + 1 - T;
    big_lds(k_rs_tile<0, D...>, TILE_LDS);
    hipLaunchKernelGGL((k_rs_tile<0, D...>), dim3((unsigned)((n_pair * T + S - 1) / S)), dim3(NT), TILE_LDS, s, plan->params, offsets_of(plan),
                       plan->ln_eps, plan->n_rows, plan->K, (const int64_t*)nullptr, (const int64_t*)nullptr, 1, tgt, tgt_len, (int)n_pair, T,
                       (const float*)nullptr, 1, (const int*)cum, S, (const float*)nullptr, cond_logits, dp...);
    return DR4SR_LAUNCH_CHECK();
}

template <class... D>
int score_rows(const dr4sr_regen_plan* plan, const int64_t* src, const int64_t* src_len, const int64_t* tgt, const int64_t* tgt_len,
               int64_t n_pair, int32_t Ls, int32_t T, const float* w, int32_t n_w, int32_t causal_source, void* workspace,
               int64_t workspace_bytes, float* nll, void* stream, D... dp) {
    if (const int rc = check_sizes(plan, n_pair, Ls, T, n_w)) return rc;
    if (!src || !src_len || !tgt || !tgt_len || !w || !nll) return DR4SR_E_ARG;
    if (!workspace || workspace_bytes < ws_bytes(n_pair, plan->K, Ls)) return DR4SR_E_WS;
    if (n_pair == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    int* cum = static_cast<int*>(workspace);
    float* ckv = reinterpret_cast<float*>(static_cast<char*>(workspace) + cum_bytes(n_pair));
    hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(1024), 0, s, tgt_len, (int)n_pair, T, 1, cum);
    if (const int rc = DR4SR_LAUNCH_CHECK()) return rc;
    if (const int rc = with_kc(plan->K, [&](auto kc) {
            return launch_source<decltype(kc)::value, D...>(plan, src, src_len, n_pair, Ls, causal_source != 0, ckv, s, dp...);
        })) return rc;
    const int S = TM + 1 - T;
    big_lds(k_rs_tile<1, D...>, TILE_LDS);
    hipLaunchKernelGGL((k_rs_tile<1, D...>), dim3((unsigned)((n_pair * n_w * T + S - 1) / S)), dim3(NT), TILE_LDS, s, plan->params,
                       offsets_of(plan), plan->ln_eps, plan->n_rows, plan->K, src, src_len, Ls, tgt, tgt_len, (int)n_pair, T, w, n_w,
                       (const int*)cum, S, (const float*)ckv, nll, dp...);
    return DR4SR_LAUNCH_CHECK();
}

// p = 0 is eval mode; a train-mode call needs 0 <= p < 1 and a pair0 whose element indices stay inside 64 bits
int check_drop(float p, int64_t pair0) { return (p >= 0.f && p < 1.f && pair0 >= 0 && pair0 < (1LL << 40)) ? 0 : DR4SR_E_ARG; }

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
    return score_condition(plan, tgt, tgt_len, n_pair, T, workspace, workspace_bytes, cond_logits, stream);
}

extern "C" int dr4sr_regen_score(const dr4sr_regen_plan* plan, const int64_t* src, const int64_t* src_len, const int64_t* tgt,
                                 const int64_t* tgt_len, int64_t n_pair, int32_t Ls, int32_t T, const float* w, int32_t n_w,
                                 int32_t causal_source, void* workspace, int64_t workspace_bytes, float* nll, void* stream) {
    return score_rows(plan, src, src_len, tgt, tgt_len, n_pair, Ls, T, w, n_w, causal_source, workspace, workspace_bytes, nll, stream);
}

extern "C" int dr4sr_regen_score_condition_train(const dr4sr_regen_plan* plan, const int64_t* tgt, const int64_t* tgt_len, int64_t n_pair,
                                                 int32_t T, void* workspace, int64_t workspace_bytes, float* cond_logits, float p, uint64_t seed,
                                                 uint32_t step, int64_t pair0, void* stream) {
    if (const int rc = check_drop(p, pair0)) return rc;
    if (p == 0.f) return score_condition(plan, tgt, tgt_len, n_pair, T, workspace, workspace_bytes, cond_logits, stream);
    return score_condition(plan, tgt, tgt_len, n_pair, T, workspace, workspace_bytes, cond_logits, stream, host_drop(p, seed, step, pair0));
}

extern "C" int dr4sr_regen_score_train(const dr4sr_regen_plan* plan, const int64_t* src, const int64_t* src_len, const int64_t* tgt,
                                       const int64_t* tgt_len, int64_t n_pair, int32_t Ls, int32_t T, const float* w, int32_t n_w,
                                       int32_t causal_source, void* workspace, int64_t workspace_bytes, float* nll, float p, uint64_t seed,
                                       uint32_t step, int64_t pair0, void* stream) {
    if (const int rc = check_drop(p, pair0)) return rc;
    if (p == 0.f)
        return score_rows(plan, src, src_len, tgt, tgt_len, n_pair, Ls, T, w, n_w, causal_source, workspace, workspace_bytes, nll, stream);
    return score_rows(plan, src, src_len, tgt, tgt_len, n_pair, Ls, T, w, n_w, causal_source, workspace, workspace_bytes, nll, stream,
                      host_drop(p, seed, step, pair0));
}
