// regen_score_bwd.hip — gradients of teacher-forced scoring, fp32: the vector-Jacobian product of everything dr4sr_regen_score and
// dr4sr_regen_score_condition compute (regen_score.hip), exact against float64 autograd.  Nothing stochastic, nothing stateful.
//
//   k_rsb_dec_tile   the target side (backward of k_rs_tile<1>), one workgroup per packed tile: same scan, same S = 65 - T windows, same
//                    slots.  It runs the tile's forward again and then its backward, both on the 32x32x2 MFMA tiles; data gradients use
//                    the forward weights as they lie (mma_64xN_wT).  Chain: dnll -> restricted softmax (p_j - 1[target slot] on the
//                    first-occurrence slots) -> decoder.norm -> 2 decoder layers (LayerNorm x3, erf-GELU FFN, cross-attention, causal
//                    self-attention) -> the input rows.  The cross-attention leaves d(K | V) of the row's MIXED memory in dkv.
//   k_rsb_dw         dw[row][k] = <d(K | V), (K | V)_k>, a wave per score row.
//   k_rsb_source     the source side (backward of k_rs_source), one workgroup per pair: d(K | V)_k = sum over the pair's weight vectors of
//                    w_k d(K | V), back through the K | V rows of both decoder in_proj, condition_linear[2], ReLU, condition_linear[0],
//                    encoder.norm and the two encoder layers (causal or bidirectional).
//   k_rsb_cond_tile  the condition encoder (backward of k_rs_tile<0>): dlogits -> the two linears -> mean pooling (over len(t) + 2, as
//                    the forward) -> 2 encoder layers -> the input rows.
// Activations: every tile kernel runs its forward again, through the same functions as the scoring kernels (regen_score_fwd.h) with
// the KeepRec policy, which writes what a weight gradient needs into the tile's slot RECORDS in the workspace; the backward chain adds
// every per-token output gradient (empty slots hold zero gradients and finite activations); the LDS holds one operation's
// working set (the forward's layout + one score-gradient buffer).  The chain of a layer is the forward's blocks in reverse, one text
// for the three kernels as in regen_score_fwd.h: ffn_block_bwd, self_block_bwd (with self_attention_bwd or src_attention_bwd as its
// attention) and the decoder's cross_block_bwd, so a kernel's backward layer loop is two or three calls under the two or three forward
// calls it differentiates.  What differs between the kernels is an argument or is marked "KEPT DIFFERENCE".
//   k_rsb_wgrad      every weight, bias and LayerNorm gradient as one job list: dW[n][k] = sum over records of dY[n] X[k] (a bias is the
//                    job with X = 1).  The records are cut into NSPLIT contiguous ranges, each summed in record order into its own
//                    partial slab.
//   k_rsb_reduce     grad += the NSPLIT partial slabs, added in slab order.
//   k_rsb_embed      store-then-sum per destination: one workgroup per table row scans the record keys in order and adds the matching
//                    records' rows (target lookups, source lookups, the logit term; positions likewise).
// Train mode (the *_train entry points, DropPhilox policy): the forward drops at the reference's sites, so the records hold the post-dropout
// GEMM inputs; the chain multiplies the gradient by the same regenerated factor at each site (drop_grad64 behind an output site, inside
// the GELU loop for the hidden layer, on the input rows' gradient before the table sums); an attention block forms dP = (dO V^T) keep,
// applies the softmax Jacobian to the UNDROPPED probabilities, and takes dV from the dropped ones.
// No floating-point atomics; every sum has a fixed order, so a call gives the same bits every time.  Kernels write their own zeros
// (k_rsb_zero), nothing is memset.
#include "regen_score_fwd.h"

namespace {

// ---- the slot record (floats).  Per layer l at l * LF: what the forward saved, then what the backward produced.
constexpr int LF = 1856;
enum { F_X = 0, F_QKV = 64, F_O = 256, F_V1 = 320, F_X1 = 384, F_HP = 448, F_HH = 704, F_V2 = 960,
       F_DQKV = 1024, F_DV1 = 1216, F_DHP = 1280, F_DV2 = 1536, F_G1 = 1600, F_Y1 = 1664, F_G2 = 1728, F_Y2 = 1792 };
constexpr int F_DX0 = RNL * LF, F_POOL = F_DX0 + 64, F_HID = F_POOL + 64, F_DHID = F_HID + 64, F_DLOG = F_DHID + 64;
constexpr int TOKF = F_DLOG + 8;
static_assert(F_V2 + 64 == F_DQKV && F_Y2 + 64 == LF && TOKF % 4 == 0, "slot record layout");
constexpr int NSPLIT = 32;
constexpr int MAXJ = 40;

// dW[n][k] = sum over records m and sub-rows q < rep of rec[m][yoff + q ystep + n] * rec[m][xoff + q xstep + k]; xoff < 0: x = 1 (a bias)
struct WJob { int yoff, xoff, N, K, nkt, blk0, rep, ystep, xstep, pad; int64_t out; };
struct WJobs { int n, nblk; WJob j[MAXJ]; };

// `tf` is the record stride in floats, `rows` the number of records (rows of the tile) that exist
__device__ __forceinline__ void load64(float* L, int ld, const float* rec, int field, int ncol, int tf = TOKF, int rows = TM) {
    for (int e = threadIdx.x; e < TM * ncol; e += NT)
        L[(e / ncol) * ld + e % ncol] = e / ncol < rows ? rec[(size_t)(e / ncol) * tf + field + e % ncol] : 0.f;
}

// Y[64][ldy] = A[64][KR] W, W global [KR][64 NTW] as the forward stores it
template <int KR, int NTW>
__device__ __forceinline__ void gemm_dx(const float* A, int lda, const float* __restrict__ W, float* Y, int ldy, int ldw = 64 * NTW) {
    f32x16 acc[NTW];
    acc_zero(acc);
    mma_64xN_wT<KR, NTW>(A, lda, W, ldw, acc);
    acc_to_lds<NTW>(acc, Y, ldy, nullptr);
}

// LayerNorm backward of the 64 rows: X holds dL/dy and leaves dL/d(input); the records take dy * xhat, dy and the input gradient
__device__ __forceinline__ void ln_bwd64(float* X, float* rec, int f_in, const float* __restrict__ w, float eps, int f_g, int f_y, int f_dv,
                                         int tf = TOKF, int rows = TM) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int r = wv; r < TM; r += NT / 64) {
        if (r >= rows) { X[r * XLD + lane] = 0.f; continue; }
        float* rr = rec + (size_t)r * tf;
        const float v = rr[f_in + lane];
        const float mean = wave_sum(v) * (1.0f / RD);
        const float d = v - mean;
        const float var = wave_sum(d * d) * (1.0f / RD);
        const float rstd = rsqrtf(var + eps);
        const float xh = d * rstd;
        const float dy = X[r * XLD + lane];
        rr[f_g + lane] = dy * xh;
        rr[f_y + lane] = dy;
        const float dxh = dy * w[lane];
        const float m1 = wave_sum(dxh) * (1.0f / RD);
        const float m2 = wave_sum(dxh * xh) * (1.0f / RD);
        const float dv = rstd * (dxh - m1 - xh * m2);
        X[r * XLD + lane] = dv;
        rr[f_dv + lane] = dv;
    }
}

__device__ __forceinline__ float gelu_grad_exact(float x) {
    const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
    return fmaf(x * 0.39894228040143267794f, expf(-0.5f * x * x), cdf);
}

// the gradient behind an output dropout site: Y[64][XLD] = X keep on the live rows (the others are copied), and the record field that
// held X (the linear's dY of the weight-gradient jobs) takes Y
template <class Rows>
__device__ __forceinline__ void drop_grad64(const DropPhilox& dp, uint32_t site, const Rows& rows, const float* X, float* Y, float* rec, int tf,
                                            int field, int nrec) {
    for (int u = threadIdx.x; u < TM * (RD / 8); u += NT) {
        const int s = u / (RD / 8), c0 = (u % (RD / 8)) * 8;
        const float4* x = reinterpret_cast<const float4*>(X + s * XLD + c0);
        float4 a = x[0], b = x[1];
        int64_t pair = 0;
        int pos = 0;
        if (rows(s, pair, pos)) {
            float4 lo, hi;
            drop8(dp.k, site, (uint64_t)((pair * 64 + pos) * RD + c0), lo, hi);
            mul8(a, b, lo, hi);
            if (s < nrec) {
                float* rr = rec + (size_t)s * tf + field + c0;
                st4(rr, a); st4(rr + 4, b);
            }
        }
        float4* y = reinterpret_cast<float4*>(Y + s * XLD + c0);
        y[0] = a; y[1] = b;
    }
}

// U[64][FLD] = U keep gelu'(hp) over the first `nrec` rows, into the record's dhp too: the gradient behind the FFN's hidden site
// (eval mode: no factor, and an element per thread rather than the 8 of a Philox call)
template <class Drop, class Rows>
__device__ __forceinline__ void gelu_bwd64(const Drop& dp, uint32_t site, const Rows& rows, float* U, float* rec, int tf, int f_hp, int f_dhp,
                                           int nrec) {
    if constexpr (!Drop::on) {
        for (int e = threadIdx.x; e < nrec * RF; e += NT) {
            const int s = e / RF, c = e % RF;
            const float d = U[s * FLD + c] * gelu_grad_exact(rec[(size_t)s * tf + f_hp + c]);
            U[s * FLD + c] = d;
            rec[(size_t)s * tf + f_dhp + c] = d;
        }
    } else {
        for (int u = threadIdx.x; u < nrec * (RF / 8); u += NT) {
            const int s = u / (RF / 8), c0 = (u % (RF / 8)) * 8;
            int64_t pair = 0;
            int pos = 0;
            float4 lo = make_float4(1.f, 1.f, 1.f, 1.f), hi = lo;
            if (rows(s, pair, pos)) drop8(dp.k, site, (uint64_t)((pair * 64 + pos) * RF + c0), lo, hi);
            const float m[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float d = U[s * FLD + c0 + i] * m[i] * gelu_grad_exact(rec[(size_t)s * tf + f_hp + c0 + i]);
                U[s * FLD + c0 + i] = d;
                rec[(size_t)s * tf + f_dhp + c0 + i] = d;
            }
        }
    }
}

// backward of self_attention: QKV [64][QLD] and dO [64][XLD] in LDS -> dQKV into the slot records (gout = record base + field).
// Pass A, a thread per (query slot, head): the probabilities again (PS), dS = p (dP - sum p dP) scale (DS), dQ.
// Pass B, a thread per (key slot, head): dK and dV over the row's later queries, in query order.
// Train mode: dP = (dO . V) keep, the Jacobian on the undropped p; pass A then leaves the DROPPED probabilities in PS for pass B's dV.
template <class Drop>
__device__ __forceinline__ void self_attention_bwd(const Drop& dp, uint32_t site, const TileTab& tb, const float* QKV, const float* dO, float* PS,
                                                   float* DS, float* gout, float scale, int tf = TOKF) {
    const int s = threadIdx.x >> 1, h = threadIdx.x & 1;
    if (threadIdx.x < TM * RH) {
        const int r = tb.tok_row[s];
        float dq[RDH];
#pragma unroll
        for (int d = 0; d < RDH; ++d) dq[d] = 0.f;
        if (r >= 0) {
            const int base = tb.row_base[r], nk = tb.tok_pos[s] + 1;
            float* pr = PS + (s * RH + h) * PLD;
            float* ds = DS + (s * RH + h) * PLD;
            const float* q = QKV + s * QLD + h * RDH;
            const float* go = dO + s * XLD + h * RDH;
            for (int j = 0; j < nk; ++j) {
                float v = -INFINITY;
                if (tb.tok_id[base + j] != 0) {
                    const float* k = QKV + (base + j) * QLD + RD + h * RDH;
                    float a = 0.f;
                    for (int d = 0; d < RDH; ++d) a = fmaf(q[d], k[d], a);
                    v = a * scale;
                }
                pr[j] = v;
            }
            softmax_masked(pr, nk);
            uint64_t km = 0;
            if constexpr (Drop::on) km = prob_keep_bits(dp, site, dp.pair0 + tb.row_pair[r], h, tb.tok_pos[s], nk);
            float dsum = 0.f;
            for (int j = 0; j < nk; ++j) {
                const float* v = QKV + (base + j) * QLD + 2 * RD + h * RDH;
                float a = 0.f;
                for (int d = 0; d < RDH; ++d) a = fmaf(go[d], v[d], a);
                if constexpr (Drop::on) a = ((km >> j) & 1) ? a * dp.k.scale : 0.f;
                ds[j] = a;
                dsum = fmaf(pr[j], a, dsum);
            }
            for (int j = 0; j < nk; ++j) {
                const float g = pr[j] * (ds[j] - dsum) * scale;
                ds[j] = g;
                if constexpr (Drop::on) pr[j] = ((km >> j) & 1) ? pr[j] * dp.k.scale : 0.f;
                const float* k = QKV + (base + j) * QLD + RD + h * RDH;
#pragma unroll
                for (int d = 0; d < RDH; ++d) dq[d] = fmaf(g, k[d], dq[d]);
            }
        }
#pragma unroll
        for (int d = 0; d < RDH; ++d) gout[(size_t)s * tf + h * RDH + d] = dq[d];
    }
    __syncthreads();
    if (threadIdx.x < TM * RH) {
        const int r = tb.tok_row[s];
        float dk[RDH], dv[RDH];
#pragma unroll
        for (int d = 0; d < RDH; ++d) { dk[d] = 0.f; dv[d] = 0.f; }
        if (r >= 0 && tb.tok_id[s] != 0) {
            const int base = tb.row_base[r], n = tb.row_n[r], pj = tb.tok_pos[s];
            for (int i = pj; i < n; ++i) {
                const int si = base + i;
                const float p = PS[(si * RH + h) * PLD + pj], g = DS[(si * RH + h) * PLD + pj];
                const float* q = QKV + si * QLD + h * RDH;
                const float* go = dO + si * XLD + h * RDH;
#pragma unroll
                for (int d = 0; d < RDH; ++d) { dk[d] = fmaf(g, q[d], dk[d]); dv[d] = fmaf(p, go[d], dv[d]); }
            }
        }
#pragma unroll
        for (int d = 0; d < RDH; ++d) {
            gout[(size_t)s * tf + RD + h * RDH + d] = dk[d];
            gout[(size_t)s * tf + 2 * RD + h * RDH + d] = dv[d];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- layer blocks
// The backward of the layer blocks of regen_score_fwd.h, with the same arguments: `lo` and the indices of the block's weights, the
// site numbering of the forward block, X [64][XLD] the residual stream (in: the gradient of the block's output, out: of its input),
// T and U scratch.  `rec, tf, nrec`: the first record, the record stride in floats and the number of records that exist.
// KEPT DIFFERENCE: the tile kernels have nrec = 64 records, a source row has Ls, which bounds every record access and the GELU loop.
// KEPT DIFFERENCE: G, a free [64][XLD] buffer for the gradient behind an output dropout site (train mode only), is the caller's: the
// tile kernels have DS, idle between two attention blocks; the source kernel has no such buffer and lends T or S (see there).
struct LnBwdRec { int v, g, y, dv; };              // a LayerNorm: its input; what ln_bwd64 leaves: dy * xhat, dy, the input's gradient
struct FfnBwdRec { LnBwdRec n; int hp, dhp; };     // the FFN block: the hidden layer before GELU and its gradient
struct SelfBwdRec { LnBwdRec n; int qkv, dqkv; };  // a self-attention block: q | k | v and their gradient
struct CrossBwdRec { LnBwdRec n; int q, dq; };     // the cross-attention block: q and its gradient

__device__ __forceinline__ void add64(float* X, const float* A) {
    for (int e = threadIdx.x; e < TM * RD; e += NT) X[(e / RD) * XLD + e % RD] += A[(e / RD) * XLD + e % RD];
}

// X += A[64][KR] W through T: a linear's input gradient joins the residual stream.  Starts behind a barrier, ends behind one.
template <int KR>
__device__ __forceinline__ void add_dx(const float* A, int lda, const float* __restrict__ W, float* X, float* T) {
    gemm_dx<KR, 1>(A, lda, W, T, XLD);
    __syncthreads();
    add64(X, T);
    __syncthreads();
}

// the block's LayerNorm and output projection: T = (dL/d(LayerNorm input), dropped at `site` in train mode) Wo.  No barrier at the end.
template <class Drop, class Rows>
__device__ __forceinline__ void out_proj_bwd(const Drop& dp, uint32_t site, const Rows& rows, LnBwdRec f, const float* P, const int64_t* lo, int outw,
                                             int nw, float eps, float* X, float* T, float* G, float* rec, int tf, int nrec) {
    ln_bwd64(X, rec, f.v, P + lo[nw], eps, f.g, f.y, f.dv, tf, nrec);
    __syncthreads();
    if constexpr (Drop::on) {              // the dropped gradient is the linear's dY
        drop_grad64(dp, site, rows, X, G, rec, tf, f.dv, nrec);
        __syncthreads();
        gemm_dx<RD, 1>(G, XLD, P + lo[outw], T, XLD);
    } else {
        gemm_dx<RD, 1>(X, XLD, P + lo[outw], T, XLD);
    }
}

// FFN: sites site0 (hidden) and site0 + 1 (output), as ffn_block_fwd numbers them
template <class Drop, class Rows>
__device__ __forceinline__ void ffn_block_bwd(const Drop& dp, uint32_t site0, const Rows& rows, FfnBwdRec f, const float* P, const int64_t* lo, int w1,
                                              int w2, int nw, float eps, float* X, float* T, float* U, float* G, float* rec, int tf, int nrec) {
    ln_bwd64(X, rec, f.n.v, P + lo[nw], eps, f.n.g, f.n.y, f.n.dv, tf, nrec);
    __syncthreads();
    if constexpr (Drop::on) {
        drop_grad64(dp, site0 + 1, rows, X, G, rec, tf, f.n.dv, nrec);
        __syncthreads();
        gemm_dx<RD, 4>(G, XLD, P + lo[w2], U, FLD);
    } else {
        gemm_dx<RD, 4>(X, XLD, P + lo[w2], U, FLD);
    }
    __syncthreads();
    gelu_bwd64(dp, site0, rows, U, rec, tf, f.hp, f.dhp, nrec);
    __syncthreads();
    add_dx<RF>(U, FLD, P + lo[w1], X, T);
}

// self-attention: attend() turns q | k | v in U [64][QLD] and dO in T into the record's dQKV (site0: its probabilities; site0 + 1: the
// block's output, as self_block_fwd numbers them)
template <class Drop, class Rows, class Attend>
__device__ __forceinline__ void self_block_bwd(const Drop& dp, uint32_t site0, const Rows& rows, SelfBwdRec f, const float* P, const int64_t* lo,
                                               int inw, int outw, int nw, float eps, float* X, float* T, float* U, float* G, float* rec, int tf,
                                               int nrec, Attend attend) {
    out_proj_bwd(dp, site0 + 1, rows, f.n, P, lo, outw, nw, eps, X, T, G, rec, tf, nrec);
    load64(U, QLD, rec, f.qkv, 3 * RD, tf, nrec);
    __syncthreads();
    attend();
    __syncthreads();
    load64(U, QLD, rec, f.dqkv, 3 * RD, tf, nrec);
    __syncthreads();
    add_dx<3 * RD>(U, QLD, P + lo[inw], X, T);
}

// the input rows of a tile kernel: both embedding terms went through the tgt_emb mask, so does their gradient; dead slots store zeros
template <class Drop>
__device__ __forceinline__ void tile_input_bwd(const Drop& dp, const TileRows& rows, float* X, float* rec, int tf, int f_dx0) {
    if constexpr (Drop::on) {
        drop_tile<RD>(dp, DR4SR_REGEN_SITE_TGT_EMB, X, XLD, rows);
        __syncthreads();
    }
    for (int e = threadIdx.x; e < TM * RD; e += NT) {
        const int s = e / RD, c = e % RD;
        rec[(size_t)s * tf + f_dx0 + c] = rows.tb.tok_row[s] >= 0 ? X[s * XLD + c] : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------------------------- the tile
template <class... D>      // D: nothing (eval mode) or DropPhilox
__global__ __launch_bounds__(NT) void k_rsb_cond_tile(const float* __restrict__ P, ScoreOff off, float eps, int n_rows, int K,
                                                      const int64_t* __restrict__ tgt, const int64_t* __restrict__ tgt_len, int n_pair, int T,
                                                      const int* __restrict__ cum, int S, const float* __restrict__ dlogits,
                                                      float* __restrict__ slab, int* __restrict__ slot_id, int* __restrict__ slot_pos, D... dpa) {
    const auto dp = pick_drop(dpa...);
    using Drop = std::remove_const_t<decltype(dp)>;
    __shared__ TileTab tb;
    float* X = smem;                               // [64][XLD]
    float* Tt = X + TM * XLD;                      // [64][XLD]
    float* U = Tt + TM * XLD;                      // [64][FLD]
    float* PS = U + TM * FLD;                      // [64][RH][PLD] attention probabilities
    float* DS = PS + TM * RH * PLD;                // [64][RH][PLD] score gradients
    if (!build_tile_tab<0, false>(tb, n_rows, K, nullptr, 1, tgt, n_pair, T, nullptr, 1, cum, S)) return;
    const int n_row = tb.n_row;
    float* rec = slab + (size_t)blockIdx.x * TM * TOKF;
    if (threadIdx.x < TM) {
        const int s = threadIdx.x, live = tb.tok_row[s] >= 0;
        slot_id[(size_t)blockIdx.x * TM + s] = live ? tb.tok_id[s] : -1;
        slot_pos[(size_t)blockIdx.x * TM + s] = live ? tb.tok_pos[s] : -1;
    }
    embed_tile(P + off.o[T_E], P + off.o[T_P], X, tb);
    __syncthreads();
    const TileRows rows{tb, dp.pair0};
    if constexpr (Drop::on) {
        drop_tile<RD>(dp, DR4SR_REGEN_SITE_TGT_EMB, X, XLD, rows);
        __syncthreads();
    }
    const float scale = rsqrtf((float)RDH);
    // ---- the forward of k_rs_tile<0>, keeping what the backward reads (row r of the tile's pooling sits in record r)
    const KeepRec keep{rec, TOKF, TM};
    for (int l = 0; l < RNL; ++l) {
        const int64_t* lo = off.o + T_CENC + 12 * l;
        const int f = l * LF;
        self_block_fwd(keep, dp, rs_site(ST_COND, l, 0), rows, {f + F_X, f + F_QKV, f + F_O, f + F_V1}, P, lo, E_INW, E_OUTW, E_N1W, eps, X, Tt, U,
                       [&] { self_attention(dp, rs_site(ST_COND, l, 0), tb, U, PS, Tt, scale); });
        ffn_block_fwd(keep, dp, rs_site(ST_COND, l, 2), rows, {f + F_X1, f + F_HP, f + F_HH, f + F_V2}, P, lo, E_W1, E_W2, E_N2W, eps, X, Tt, U);
    }
    pool_and_hidden(tb, n_row, tgt_len, P, off, X, Tt, U);
    keep.save(Tt, XLD, F_POOL, RD);
    keep.save(U, XLD, F_HID, RD);
    // ---- backward of the two linears and of the pooling
    const float* W2c = P + off.o[T_CC2W];
    for (int e = threadIdx.x; e < TM * RD; e += NT) {
        const int r = e / RD, c = e % RD;
        float v = 0.f;
        if (r < n_row && U[r * XLD + c] > 0.f) {
            const float* dl = dlogits + (int64_t)tb.row_pair[r] * K;
            for (int k = 0; k < K; ++k) v = fmaf(dl[k], W2c[k * RD + c], v);
        }
        X[r * XLD + c] = v;
        rec[(size_t)r * TOKF + F_DHID + c] = v;
    }
    for (int e = threadIdx.x; e < TM * 8; e += NT) {
        const int r = e / 8, k = e % 8;
        rec[(size_t)r * TOKF + F_DLOG + k] = (r < n_row && k < K) ? dlogits[(int64_t)tb.row_pair[r] * K + k] : 0.f;
    }
    __syncthreads();
    gemm_dx<RD, 1>(X, XLD, P + off.o[T_CC0W], Tt, XLD);
    __syncthreads();
    for (int e = threadIdx.x; e < TM * RD; e += NT) {
        const int s = e / RD, c = e % RD, r = tb.tok_row[s];
        X[s * XLD + c] = r >= 0 ? Tt[r * XLD + c] / (float)max<int64_t>(tgt_len[tb.row_pair[r]], 1) : 0.f;
    }
    __syncthreads();
    // ---- backward of the two encoder layers; X carries the gradient of the layer's output
    for (int l = RNL - 1; l >= 0; --l) {
        const int64_t* lo = off.o + T_CENC + 12 * l;
        const int f = l * LF;
        ffn_block_bwd(dp, rs_site(ST_COND, l, 2), rows, {{f + F_V2, f + F_G2, f + F_Y2, f + F_DV2}, f + F_HP, f + F_DHP}, P, lo, E_W1, E_W2, E_N2W,
                      eps, X, Tt, U, DS, rec, TOKF, TM);
        self_block_bwd(dp, rs_site(ST_COND, l, 0), rows, {{f + F_V1, f + F_G1, f + F_Y1, f + F_DV1}, f + F_QKV, f + F_DQKV}, P, lo, E_INW, E_OUTW,
                       E_N1W, eps, X, Tt, U, DS, rec, TOKF, TM,
                       [&] { self_attention_bwd(dp, rs_site(ST_COND, l, 0), tb, U, Tt, PS, DS, rec + f + F_DQKV, scale); });
    }
    tile_input_bwd(dp, rows, X, rec, TOKF, F_DX0);
}
constexpr size_t BWD_TILE_LDS = sizeof(float) * (2 * TM * XLD + TM * FLD + 2 * TM * RH * PLD);

// ------------------------------------------------------------------------------------------------------------------- decoder tile
// the decoder slot record: per layer l at l * LFD what the forward saved and what the backward produced, then decoder.norm
constexpr int LFD = 2368;
enum { R_X = 0, R_QKV = 64, R_O = 256, R_V1 = 320, R_X1 = 384, R_QC = 448, R_OC = 512, R_V2 = 576, R_X2 = 640, R_HP = 704, R_HH = 960, R_V3 = 1216,
       R_DQKV = 1280, R_DV1 = 1472, R_DQC = 1536, R_DV2 = 1600, R_DHP = 1664, R_DV3 = 1920,
       R_G1 = 1984, R_Y1 = 2048, R_G2 = 2112, R_Y2 = 2176, R_G3 = 2240, R_Y3 = 2304 };
constexpr int R_VN = RNL * LFD, R_GN = R_VN + 64, R_YN = R_GN + 64, R_DX0 = R_YN + 64, TOKD = R_DX0 + 64;
static_assert(R_Y3 + 64 == LFD && TOKD % 4 == 0, "decoder slot record layout");
constexpr int KVW = RNL * 2 * RD;      // floats per (row, source position) of the mixed-memory gradient: [layer][K | V]

// backward of the cross-attention: Q and dO [64][XLD] in LDS, PS holds the probabilities -> dQ [64][XLD] in LDS and the gradient of
// the row's mixed K | V into dkv[row][j][layer][K | V] (zero where the key is masked or beyond the source).  Train mode: KM holds the keep
// bits of every (slot, head) row (cross_probs): dV takes the dropped probabilities, DS = (dO . V) keep before the Jacobian on PS.
template <class Drop>
__device__ __forceinline__ void cross_bwd(const Drop& dp, const unsigned long long* KM, const TileTab& tb, int n_row, int K, int Ls, int n_rows, int n_pair, int l, const int64_t* __restrict__ src,
                                          const float* __restrict__ ckv, const float* __restrict__ cb, const float* Q, const float* dO,
                                          const float* PS, float* DS, float* DQ, float* __restrict__ dkv, float scale) {
    for (int e = threadIdx.x; e < n_row * RH * LMAX; e += NT) {
        const int r = e / (RH * LMAX), h = (e / LMAX) % RH, j = e % LMAX;
        if (j >= Ls) continue;
        const int base = tb.row_base[r], n = tb.row_n[r];
        float* gk = dkv + (((int64_t)tb.row_w[r] * n_pair + tb.row_pair[r]) * Ls + j) * KVW + l * 2 * RD + h * RDH;
        const bool inside = j < tb.row_ls[r];
        if (!inside || !src_live(src, tb.row_pair[r], Ls, j, n_rows)) {
#pragma unroll
            for (int d = 0; d < RDH; ++d) { gk[d] = 0.f; gk[RD + d] = 0.f; }
            if (inside)
                for (int t = 0; t < n; ++t) DS[((base + t) * RH + h) * PLD + j] = 0.f;
            continue;
        }
        float v[RDH], dv[RDH];
        mix_kv(tb, r, K, Ls, l, j, RD + h * RDH, ckv, cb, v);
#pragma unroll
        for (int d = 0; d < RDH; ++d) dv[d] = 0.f;
        for (int t = 0; t < n; ++t) {
            const float* go = dO + (base + t) * XLD + h * RDH;
            float pj = PS[((base + t) * RH + h) * PLD + j];
            bool kept = true;
            if constexpr (Drop::on) {
                kept = (KM[(base + t) * RH + h] >> j) & 1;
                pj = kept ? pj * dp.k.scale : 0.f;
            }
            float a = 0.f;
#pragma unroll
            for (int d = 0; d < RDH; ++d) { a = fmaf(go[d], v[d], a); dv[d] = fmaf(pj, go[d], dv[d]); }
            if constexpr (Drop::on) a = kept ? a * dp.k.scale : 0.f;
            DS[((base + t) * RH + h) * PLD + j] = a;
        }
#pragma unroll
        for (int d = 0; d < RDH; ++d) gk[RD + d] = dv[d];
    }
    __syncthreads();
    if (threadIdx.x < TM * RH) {
        const int r = tb.tok_row[threadIdx.x >> 1];
        if (r >= 0) {
            const int ls = tb.row_ls[r];
            const float* pr = PS + threadIdx.x * PLD;
            float* ds = DS + threadIdx.x * PLD;
            float dsum = 0.f;
            for (int j = 0; j < ls; ++j) dsum = fmaf(pr[j], ds[j], dsum);
            for (int j = 0; j < ls; ++j) ds[j] = pr[j] * (ds[j] - dsum) * scale;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n_row * RH * LMAX; e += NT) {
        const int r = e / (RH * LMAX), h = (e / LMAX) % RH, j = e % LMAX;
        if (j >= tb.row_ls[r] || !src_live(src, tb.row_pair[r], Ls, j, n_rows)) continue;
        const int base = tb.row_base[r], n = tb.row_n[r];
        float dk[RDH];
#pragma unroll
        for (int d = 0; d < RDH; ++d) dk[d] = 0.f;
        for (int t = 0; t < n; ++t) {
            const float g = DS[((base + t) * RH + h) * PLD + j];
            const float* q = Q + (base + t) * XLD + h * RDH;
#pragma unroll
            for (int d = 0; d < RDH; ++d) dk[d] = fmaf(g, q[d], dk[d]);
        }
        float* gk = dkv + (((int64_t)tb.row_w[r] * n_pair + tb.row_pair[r]) * Ls + j) * KVW + l * 2 * RD + h * RDH;
#pragma unroll
        for (int d = 0; d < RDH; ++d) gk[d] = dk[d];
    }
    if (threadIdx.x < TM * RH) {
        const int s = threadIdx.x >> 1, h = threadIdx.x & 1, r = tb.tok_row[s];
        float dq[RDH];
#pragma unroll
        for (int d = 0; d < RDH; ++d) dq[d] = 0.f;
        if (r >= 0) {
            const int ls = tb.row_ls[r];
            for (int j = 0; j < ls; ++j) {
                if (!src_live(src, tb.row_pair[r], Ls, j, n_rows)) continue;
                const float g = DS[threadIdx.x * PLD + j];
                float k[RDH];
                mix_kv(tb, r, K, Ls, l, j, h * RDH, ckv, cb, k);
#pragma unroll
                for (int d = 0; d < RDH; ++d) dq[d] = fmaf(g, k[d], dq[d]);
            }
        }
#pragma unroll
        for (int d = 0; d < RDH; ++d) DQ[s * XLD + h * RDH + d] = dq[d];
    }
}

// cross-attention (site0: its probabilities; site0 + 1: the block's output, as cross_block_fwd numbers them): dO = dV2 Wo, the
// probabilities again from the saved q (U: q [64][XLD], then dq [64][XLD] behind it), d(K | V) of the mixed memory into dkv
template <class Drop, class Rows>
__device__ __forceinline__ void cross_block_bwd(const Drop& dp, uint32_t site0, const Rows& rows, CrossBwdRec f, const TileTab& tb, int n_row, int K,
                                                int Ls, int n_rows, int n_pair, int l, const int64_t* __restrict__ src,
                                                const float* __restrict__ ckv, const float* P, const int64_t* lo, float eps, float* X, float* T,
                                                float* U, float* PS, float* DS, unsigned long long* KM, float* __restrict__ dkv, float scale,
                                                float* rec, int tf, int nrec) {
    out_proj_bwd(dp, site0 + 1, rows, f.n, P, lo, D_CAOUTW, D_N2W, eps, X, T, DS, rec, tf, nrec);
    load64(U, XLD, rec, f.q, RD, tf, nrec);
    __syncthreads();
    const float* cb = P + lo[D_CAINB];
    cross_probs(dp, site0, KM, tb, n_row, K, Ls, n_rows, l, src, ckv, cb, U, PS, scale);
    float* DQ = U + TM * XLD;
    cross_bwd(dp, KM, tb, n_row, K, Ls, n_rows, n_pair, l, src, ckv, cb, U, T, PS, DS, DQ, dkv, scale);
    __syncthreads();
    KeepRec{rec, tf, nrec}.save(DQ, XLD, f.dq, RD);
    add_dx<RD>(DQ, XLD, P + lo[D_CAINW], X, T);
}

template <class... D>      // D: nothing (eval mode) or DropPhilox
__global__ __launch_bounds__(NT) void k_rsb_dec_tile(const float* __restrict__ P, ScoreOff off, float eps, int n_rows, int K,
                                                     const int64_t* __restrict__ src, const int64_t* __restrict__ src_len, int Ls,
                                                     const int64_t* __restrict__ tgt, const int64_t* __restrict__ tgt_len, int n_pair, int T,
                                                     const float* __restrict__ wts, int n_w, const int* __restrict__ cum, int S,
                                                     const float* __restrict__ ckv, const float* __restrict__ dnll, float* __restrict__ slab,
                                                     int* __restrict__ slot_id, int* __restrict__ slot_pos, float* __restrict__ dkv,
                                                     float* __restrict__ delog, int* __restrict__ lkey, D... dpa) {
    const auto dp = pick_drop(dpa...);
    using Drop = std::remove_const_t<decltype(dp)>;
    __shared__ TileTab tb;
    float* X = smem;
    float* Tt = X + TM * XLD;
    float* U = Tt + TM * XLD;                      // [64][FLD]; in the cross-attention backward: q [64][XLD] then dq [64][XLD]
    float* PS = U + TM * FLD;
    float* DS = PS + TM * RH * PLD;
    unsigned long long* KM = reinterpret_cast<unsigned long long*>(DS + TM * RH * PLD);     // [64][RH] keep bits; train mode only (DROP_KM_LDS)
    if (!build_tile_tab<1, true>(tb, n_rows, K, src_len, Ls, tgt, n_pair, T, wts, n_w, cum, S)) return;
    const int n_row = tb.n_row;
    float* rec = slab + (size_t)blockIdx.x * TM * TOKD;
    if (threadIdx.x < TM) {
        const int s = threadIdx.x, live = tb.tok_row[s] >= 0;
        slot_id[(size_t)blockIdx.x * TM + s] = live ? tb.tok_id[s] : -1;
        slot_pos[(size_t)blockIdx.x * TM + s] = live ? tb.tok_pos[s] : -1;
    }
    const float* E = P + off.o[T_E];
    embed_tile(E, P + off.o[T_P], X, tb);
    __syncthreads();
    const TileRows rows{tb, dp.pair0};
    if constexpr (Drop::on) {
        drop_tile<RD>(dp, DR4SR_REGEN_SITE_TGT_EMB, X, XLD, rows);
        __syncthreads();
    }
    const float scale = rsqrtf((float)RDH);
    // ---- the forward of k_rs_tile<1>, keeping what the backward reads
    const KeepRec keep{rec, TOKD, TM};
    for (int l = 0; l < RNL; ++l) {
        const int64_t* lo = off.o + T_DEC + 18 * l;
        const int f = l * LFD;
        self_block_fwd(keep, dp, rs_site(ST_DEC, l, 0), rows, {f + R_X, f + R_QKV, f + R_O, f + R_V1}, P, lo, D_SAINW, D_SAOUTW, D_N1W, eps, X, Tt,
                       U, [&] { self_attention(dp, rs_site(ST_DEC, l, 0), tb, U, PS, Tt, scale); });
        cross_block_fwd(keep, dp, rs_site(ST_DEC, l, 2), rows, {f + R_X1, f + R_QC, f + R_OC, f + R_V2}, tb, n_row, K, Ls, n_rows, l, src, ckv, P,
                        lo, eps, X, Tt, U, PS, scale);
        ffn_block_fwd(keep, dp, rs_site(ST_DEC, l, 4), rows, {f + R_X2, f + R_HP, f + R_HH, f + R_V3}, P, lo, D_W1, D_W2, D_N3W, eps, X, Tt, U);
    }
    keep.save(X, XLD, R_VN, RD);
    __syncthreads();
    add_ln64(X, nullptr, 0, P + off.o[T_DEC_NORM], P + off.o[T_DEC_NORM + 1], eps);
    __syncthreads();
    // ---- the restricted softmax and its gradient: a wave per token, lane = source slot; DL[s][j] = dnll (p_j - 1[j is the target's slot])
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float* DL = PS;                                 // [64][RH * PLD], 64 used
    for (int s = wv; s < TM; s += NT / 64) {
        const int r = tb.tok_row[s];
        if (r < 0) { DL[s * RH * PLD + lane] = 0.f; continue; }
        const int p = tb.row_pair[r], want = tb.tok_out[s];
        const RLogit o = restricted_logit(E, src, p, Ls, n_rows, X + s * XLD, want);
        const int64_t ri = (int64_t)tb.row_w[r] * n_pair + p;
        const float g = (want != 0 && o.any) ? dnll[ri * T + tb.tok_pos[s]] : 0.f;   // a target outside its source contributes nothing
        DL[s * RH * PLD + lane] = o.first ? g * (o.ex / o.sum - (o.hit ? 1.f : 0.f)) : 0.f;
        if (tb.tok_pos[s] == 0 && lane < Ls) lkey[ri * Ls + lane] = o.first ? o.id : -1;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < TM * RD; e += NT) {                                // d(decoder.norm output)
        const int s = e / RD, c = e % RD, r = tb.tok_row[s];
        float a = 0.f;
        if (r >= 0) {
            const int64_t p = tb.row_pair[r];
            for (int j = 0; j < Ls; ++j) {
                const float g = DL[s * RH * PLD + j];
                if (g != 0.f) a = fmaf(g, E[(size_t)clampi(src[p * Ls + j], 0, n_rows - 1) * RD + c], a);
            }
        }
        Tt[s * XLD + c] = a;
    }
    for (int e = threadIdx.x; e < n_row * Ls * RD; e += NT) {                        // the logit term of the table gradient, per row
        const int r = e / (Ls * RD), j = (e / RD) % Ls, c = e % RD;
        const int base = tb.row_base[r], n = tb.row_n[r];
        float a = 0.f;
        for (int t = 0; t < n; ++t) a = fmaf(DL[(base + t) * RH * PLD + j], X[(base + t) * XLD + c], a);
        delog[(((int64_t)tb.row_w[r] * n_pair + tb.row_pair[r]) * Ls + j) * RD + c] = a;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < TM * RD; e += NT) X[(e / RD) * XLD + e % RD] = Tt[(e / RD) * XLD + e % RD];
    __syncthreads();
    ln_bwd64(X, rec, R_VN, P + off.o[T_DEC_NORM], eps, R_GN, R_YN, R_DX0, TOKD);
    __syncthreads();
    // ---- backward of the two decoder layers; X carries the gradient of the layer's output
    for (int l = RNL - 1; l >= 0; --l) {
        const int64_t* lo = off.o + T_DEC + 18 * l;
        const int f = l * LFD;
        ffn_block_bwd(dp, rs_site(ST_DEC, l, 4), rows, {{f + R_V3, f + R_G3, f + R_Y3, f + R_DV3}, f + R_HP, f + R_DHP}, P, lo, D_W1, D_W2, D_N3W,
                      eps, X, Tt, U, DS, rec, TOKD, TM);
        cross_block_bwd(dp, rs_site(ST_DEC, l, 2), rows, {{f + R_V2, f + R_G2, f + R_Y2, f + R_DV2}, f + R_QC, f + R_DQC}, tb, n_row, K, Ls, n_rows,
                        n_pair, l, src, ckv, P, lo, eps, X, Tt, U, PS, DS, KM, dkv, scale, rec, TOKD, TM);
        self_block_bwd(dp, rs_site(ST_DEC, l, 0), rows, {{f + R_V1, f + R_G1, f + R_Y1, f + R_DV1}, f + R_QKV, f + R_DQKV}, P, lo, D_SAINW, D_SAOUTW,
                       D_N1W, eps, X, Tt, U, DS, rec, TOKD, TM,
                       [&] { self_attention_bwd(dp, rs_site(ST_DEC, l, 0), tb, U, Tt, PS, DS, rec + f + R_DQKV, scale, TOKD); });
    }
    tile_input_bwd(dp, rows, X, rec, TOKD, R_DX0);
}
constexpr size_t DROP_KM_LDS = sizeof(unsigned long long) * TM * RH;      // the decoder tile's keep bits, behind DS (train mode only)

// dw[row][k] = <d(K | V) of the row's mixed memory, (K | V)_k of its pair>: a wave per row, lane = feature, fixed order
__global__ __launch_bounds__(256) void k_rsb_dw(const float* __restrict__ dkv, const float* __restrict__ ckv, int K, int n_pair, int n_w, int Ls,
                                                float* __restrict__ dw) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)n_w * n_pair) return;
    const int64_t p = row % n_pair;
    for (int k = 0; k < K; ++k) {
        float a = 0.f;
        for (int l = 0; l < RNL; ++l)
            for (int j = 0; j < Ls; ++j) {
                const float* g = dkv + (row * Ls + j) * KVW + l * 2 * RD;
                const float* c = ckv + (((p * K + k) * RNL + l) * Ls + j) * (2 * RD);
                a = fmaf(g[lane], c[lane], a);
                a = fmaf(g[RD + lane], c[RD + lane], a);
            }
        a = wave_sum(a);
        if (lane == 0) dw[row * K + k] = a;
    }
}

// ------------------------------------------------------------------------------------------------------------------- source side
// the source record (one per pair and source position < Ls): the two encoder layers as the condition encoder's, then
constexpr int S_VN = RNL * LF, S_GN = S_VN + 64, S_YN = S_GN + 64, S_MEMN = S_YN + 64, S_C1 = S_MEMN + 64, S_DC1 = S_C1 + KMAX * RD,
              S_MEM = S_DC1 + KMAX * RD, S_DMEM = S_MEM + KMAX * RD, S_DCKV = S_DMEM + KMAX * RD, S_DX0 = S_DCKV + RNL * KMAX * 2 * RD,
              TOKS = S_DX0 + 64;
static_assert(TOKS % 4 == 0, "source record layout");
constexpr int ALD = 2 * RD + 4;

// backward of the source side's self-attention (src_probs + src_context): q | k | v [64][QLD] and dO [64][XLD] in LDS -> dQKV of the
// `nrec` records (gout = record base + field).  S takes the undropped probabilities again, DSb the score gradients.
template <class Drop>
__device__ __forceinline__ void src_attention_bwd(const Drop& dp, uint32_t site, int64_t pair, const float* QKV, const float* dO, float* S, float* DSb,
                                                  const int* ids, int n, int causal, float* gout, float scale, int tf, int nrec) {
    src_probs(dp, site, pair, false, QKV, S, ids, n, causal, scale);
    for (int e = threadIdx.x; e < RH * n * n; e += NT) {
        const int h = e / (n * n), i = (e / n) % n, j = e % n;
        const float* go = dO + i * XLD + h * RDH;
        const float* v = QKV + j * QLD + 2 * RD + h * RDH;
        float a = 0.f;
        for (int d = 0; d < RDH; ++d) a = fmaf(go[d], v[d], a);
        DSb[(h * LMAX + i) * LMAX + j] = a;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < RH * n; e += NT) {
        const float* pr = S + ((e / n) * LMAX + e % n) * LMAX;
        float* ds = DSb + ((e / n) * LMAX + e % n) * LMAX;
        float dsum = 0.f;
        if constexpr (Drop::on) {          // dP = (dO . V) keep; the Jacobian on the undropped p; S then takes the dropped p for dV
            float* pw = S + ((e / n) * LMAX + e % n) * LMAX;
            const uint64_t km = prob_keep_bits(dp, site, pair, e / n, e % n, n);
            for (int j = 0; j < n; ++j) {
                ds[j] = ((km >> j) & 1) ? ds[j] * dp.k.scale : 0.f;
                dsum = fmaf(pr[j], ds[j], dsum);
            }
            for (int j = 0; j < n; ++j) {
                ds[j] = pr[j] * (ds[j] - dsum) * scale;
                pw[j] = ((km >> j) & 1) ? pr[j] * dp.k.scale : 0.f;
            }
        } else {
            for (int j = 0; j < n; ++j) dsum = fmaf(pr[j], ds[j], dsum);
            for (int j = 0; j < n; ++j) ds[j] = pr[j] * (ds[j] - dsum) * scale;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nrec * RD; e += NT) {
        const int i = e / RD, c = e % RD, h = c / RDH;
        float dq = 0.f, dk = 0.f, dv = 0.f;
        if (i < n) {
            for (int j = 0; j < n; ++j) {
                dq = fmaf(DSb[(h * LMAX + i) * LMAX + j], QKV[j * QLD + RD + c], dq);
                dk = fmaf(DSb[(h * LMAX + j) * LMAX + i], QKV[j * QLD + c], dk);
                dv = fmaf(S[(h * LMAX + j) * LMAX + i], dO[j * XLD + c], dv);
            }
        }
        float* rr = gout + (size_t)i * tf;
        rr[c] = dq; rr[RD + c] = dk; rr[2 * RD + c] = dv;
    }
}

template <int KC, class... D>      // D: nothing (eval mode) or DropPhilox
__global__ __launch_bounds__(NT) void k_rsb_source(const float* __restrict__ P, ScoreOff off, float eps, int n_rows,
                                                   const int64_t* __restrict__ src, const int64_t* __restrict__ src_len, int Ls, int causal,
                                                   const float* __restrict__ wts, int n_w, int n_pair, const float* __restrict__ dkv,
                                                   float* __restrict__ slab, int* __restrict__ key_id, int* __restrict__ key_pos, D... dpa) {
    const auto dp = pick_drop(dpa...);
    using Drop = std::remove_const_t<decltype(dp)>;
    constexpr int KD = KC * RD, CLD = KD + 4;
    float* X = smem;                               // [64][XLD]
    float* T = X + TM * XLD;                       // [64][XLD]
    float* U = T + TM * XLD;                       // qkv + probabilities + their gradients | FFN hidden | [64][CLD] + [64][ALD]
    constexpr int USZ0 = TM * CLD + TM * ALD, USZ1 = TM * QLD + 2 * RH * LMAX * LMAX, USZ2 = TM * FLD;
    constexpr int USZ = USZ0 > USZ1 ? (USZ0 > USZ2 ? USZ0 : USZ2) : (USZ1 > USZ2 ? USZ1 : USZ2);
    int* ids = reinterpret_cast<int*>(U + USZ);
    const int64_t p = blockIdx.x;
    const int n = clampi(src_len[p], 1, Ls);
    float* rec = slab + (size_t)p * Ls * TOKS;
    if (threadIdx.x < TM) ids[threadIdx.x] = threadIdx.x < n ? clampi(src[p * Ls + threadIdx.x], 0, n_rows - 1) : 0;
    __syncthreads();
    if (threadIdx.x < Ls) {
        key_id[p * Ls + threadIdx.x] = threadIdx.x < n ? ids[threadIdx.x] : -1;
        key_pos[p * Ls + threadIdx.x] = threadIdx.x < n ? (int)threadIdx.x : -1;
    }
    embed_rows(P + off.o[T_E], P + off.o[T_P], X, [&](int j, int& id, int& pos) { id = ids[j]; pos = j; return j < n; });
    __syncthreads();
    const int64_t gpair = dp.pair0 + p;
    const SrcRows rows{gpair, n};
    if constexpr (Drop::on) {
        drop_tile<RD>(dp, DR4SR_REGEN_SITE_SRC_EMB, X, XLD, rows);
        __syncthreads();
    }
    const float scale = rsqrtf((float)RDH);
    float* QKV = U;                                // [64][QLD]
    float* S = U + TM * QLD;                       // [RH][LMAX][LMAX]
    float* DSb = S + RH * LMAX * LMAX;             // [RH][LMAX][LMAX]
    // ---- the forward of k_rs_source, keeping what the backward reads: only the Ls records of the pair exist
    const KeepRec keep{rec, TOKS, Ls};
    for (int l = 0; l < RNL; ++l) {
        const int64_t* lo = off.o + T_ENC + 12 * l;
        const int f = l * LF;
        self_block_fwd(keep, dp, rs_site(ST_SRC, l, 0), rows, {f + F_X, f + F_QKV, f + F_O, f + F_V1}, P, lo, E_INW, E_OUTW, E_N1W, eps, X, T, U, [&] {
            src_probs(dp, rs_site(ST_SRC, l, 0), gpair, true, QKV, S, ids, n, causal, scale);
            src_context(QKV, S, n, T);
        });
        ffn_block_fwd(keep, dp, rs_site(ST_SRC, l, 2), rows, {f + F_X1, f + F_HP, f + F_HH, f + F_V2}, P, lo, E_W1, E_W2, E_N2W, eps, X, T, U);
    }
    source_tail_fwd<KC>(keep, {S_VN, S_MEMN, S_C1}, P, off, eps, X, T, U, [&](int k) { keep.save(T, XLD, S_MEM + k * RD, RD); });
    // ---- backward.  d(K | V)_k of condition k = sum over the pair's weight vectors of w_k d(K | V), in vector order
    float* DM = U;                                 // [64][CLD]: d(memory), condition k at columns 64 k
    float* A = U + TM * CLD;                       // [64][ALD]
    for (int k = 0; k < KC; ++k) {
        for (int l = 0; l < RNL; ++l) {
            for (int e = threadIdx.x; e < TM * 2 * RD; e += NT) {
                const int j = e / (2 * RD), c = e % (2 * RD);
                float v = 0.f;
                if (j < Ls) {
                    for (int i = 0; i < n_w; ++i)
                        v = fmaf(wts[((int64_t)i * n_pair + p) * KC + k], dkv[(((int64_t)i * n_pair + p) * Ls + j) * KVW + l * 2 * RD + c], v);
                    rec[(size_t)j * TOKS + S_DCKV + (l * KC + k) * 2 * RD + c] = v;
                }
                A[j * ALD + c] = v;
            }
            __syncthreads();
            gemm_dx<2 * RD, 1>(A, ALD, P + off.o[T_DEC + 18 * l + D_CAINW] + RD * RD, T, XLD);
            __syncthreads();
            for (int e = threadIdx.x; e < TM * RD; e += NT) {
                const int j = e / RD, c = e % RD;
                DM[j * CLD + k * RD + c] = (l ? DM[j * CLD + k * RD + c] : 0.f) + T[j * XLD + c];
            }
            __syncthreads();
        }
    }
    keep.save(DM, CLD, S_DMEM, KD);
    for (int cbk = 0; cbk < KC; ++cbk) {               // d(condition_linear[0]'s output), 64 columns at a time
        gemm_dx<KD, 1>(DM, CLD, P + off.o[T_CL2W] + cbk * RD, T, XLD, KD);
        __syncthreads();
        for (int e = threadIdx.x; e < Ls * RD; e += NT) {
            const int j = e / RD, c = e % RD;
            float* rr = rec + (size_t)j * TOKS;
            rr[S_DC1 + cbk * RD + c] = rr[S_C1 + cbk * RD + c] > 0.f ? T[j * XLD + c] : 0.f;
        }
        __syncthreads();
    }
    load64(U, CLD, rec, S_DC1, KD, TOKS, Ls);
    __syncthreads();
    gemm_dx<KD, 1>(U, CLD, P + off.o[T_CL0W], T, XLD);
    __syncthreads();
    for (int e = threadIdx.x; e < TM * RD; e += NT) X[(e / RD) * XLD + e % RD] = T[(e / RD) * XLD + e % RD];
    __syncthreads();
    ln_bwd64(X, rec, S_VN, P + off.o[T_ENC_NORM], eps, S_GN, S_YN, S_DX0, TOKS, Ls);
    __syncthreads();
    for (int l = RNL - 1; l >= 0; --l) {
        const int64_t* lo = off.o + T_ENC + 12 * l;
        const int f = l * LF;
        // KEPT DIFFERENCE: no idle buffer for the dropped gradient here.  The FFN lends T, free until the GEMM through W1 fills it; the
        // self-attention lends S (behind q | k | v), free until src_probs fills it, because T is the out-projection's output
        ffn_block_bwd(dp, rs_site(ST_SRC, l, 2), rows, {{f + F_V2, f + F_G2, f + F_Y2, f + F_DV2}, f + F_HP, f + F_DHP}, P, lo, E_W1, E_W2, E_N2W,
                      eps, X, T, U, T, rec, TOKS, Ls);
        self_block_bwd(dp, rs_site(ST_SRC, l, 0), rows, {{f + F_V1, f + F_G1, f + F_Y1, f + F_DV1}, f + F_QKV, f + F_DQKV}, P, lo, E_INW, E_OUTW,
                       E_N1W, eps, X, T, U, S, rec, TOKS, Ls, [&] {
                           src_attention_bwd(dp, rs_site(ST_SRC, l, 0), gpair, QKV, T, S, DSb, ids, n, causal, rec + f + F_DQKV, scale, TOKS, Ls);
                       });
    }
    if constexpr (Drop::on) {              // both embedding terms went through the src_emb mask: so does their gradient
        drop_tile<RD>(dp, DR4SR_REGEN_SITE_SRC_EMB, X, XLD, rows);
        __syncthreads();
    }
    keep.save(X, XLD, S_DX0, RD);           // KEPT DIFFERENCE: the Ls records of the pair only (tile_input_bwd writes all 64 slots)
}
template <int KC> constexpr size_t bwd_source_lds() {
    constexpr int CLD = KC * RD + 4;
    constexpr int a = TM * CLD + TM * ALD, b = TM * QLD + 2 * RH * LMAX * LMAX, c = TM * FLD;
    constexpr int u = a > b ? (a > c ? a : c) : (b > c ? b : c);
    return sizeof(float) * (2 * TM * XLD + u) + sizeof(int) * TM;
}

// ------------------------------------------------------------------------------------------------------------------- reductions
__device__ __forceinline__ int used_tiles(const int* __restrict__ cum, int n_pair, int n_w, int S) {
    return (int)(((int64_t)n_w * cum[n_pair] + S - 1) / S);
}

// grid (jobs.nblk, NSPLIT): a 64 x 64 block of one job's dW over one contiguous range of records, 4 x 4 outputs per thread.
// The records are `stride` floats apart; there are fixed_m of them, or 64 per used tile when fixed_m < 0.
__global__ __launch_bounds__(256) void k_rsb_wgrad(WJobs jobs, const float* __restrict__ slab, int stride, const int* __restrict__ cum, int n_pair,
                                                   int n_w, int S, int64_t fixed_m, float* __restrict__ part, int64_t part_stride) {
    const int64_t M = fixed_m >= 0 ? fixed_m : (int64_t)used_tiles(cum, n_pair, n_w, S) * TM;
    const int64_t units = (M + TM - 1) / TM, per = (units + NSPLIT - 1) / NSPLIT;
    const int64_t m0 = min<int64_t>(M, blockIdx.y * per * TM), m1 = min<int64_t>(M, m0 + per * TM);
    int ji = 0;
    while (ji + 1 < jobs.n && jobs.j[ji + 1].blk0 <= (int)blockIdx.x) ++ji;
    const int yoff = jobs.j[ji].yoff, xoff = jobs.j[ji].xoff, N = jobs.j[ji].N, Kd = jobs.j[ji].K, nkt = jobs.j[ji].nkt;
    const int rep = jobs.j[ji].rep, ystep = jobs.j[ji].ystep, xstep = jobs.j[ji].xstep;
    const int lb = blockIdx.x - jobs.j[ji].blk0;
    const int n0 = (lb / nkt) * 64 + (threadIdx.x >> 4) * 4, k0 = (lb % nkt) * 64 + (threadIdx.x & 15) * 4;
    int yi[4], xi[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { yi[i] = yoff + min(n0 + i, N - 1); xi[i] = xoff + min(k0 + i, Kd - 1); }
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int64_t m = m0; m < m1; ++m) {
        const float* row = slab + m * stride;
        for (int q = 0; q < rep; ++q) {
            float y[4], x[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { y[i] = row[yi[i] + q * ystep]; x[i] = xoff < 0 ? 1.f : row[xi[i] + q * xstep]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(y[i], x[j], acc[i][j]);
        }
    }
    float* dst = part + (int64_t)blockIdx.y * part_stride + jobs.j[ji].out;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (n0 + i < N && k0 + j < Kd) dst[(int64_t)(n0 + i) * Kd + k0 + j] = acc[i][j];
}

__global__ __launch_bounds__(256) void k_rsb_reduce(const float* __restrict__ part, int64_t part_stride, int64_t n, float* __restrict__ grad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int sp = 0; sp < NSPLIT; ++sp) s += part[sp * part_stride + i];
    grad[i] += s;
}

__global__ __launch_bounds__(256) void k_rsb_zero(float* __restrict__ g, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) g[i] = 0.f;
}

// store-then-sum per destination: workgroup blockIdx.x owns row blockIdx.x of dst and adds rows[m][field ..] of every record m whose
// key is that row.  Each wave scans a quarter of the records in order (lane = feature); the four sums are added in wave order.
__global__ __launch_bounds__(256) void k_rsb_embed(const float* __restrict__ rows, int stride, int field, const int* __restrict__ keys,
                                                   const int* __restrict__ cum, int n_pair, int n_w, int S, int64_t fixed_m,
                                                   float* __restrict__ dst) {
    __shared__ float part[4][RD];
    const int key = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t M = fixed_m >= 0 ? fixed_m : (int64_t)used_tiles(cum, n_pair, n_w, S) * TM;
    const int64_t per = ((M + TM - 1) / TM + 3) / 4 * TM, m_lo = min<int64_t>(M, wv * per), m_hi = min<int64_t>(M, m_lo + per);
    float a = 0.f;
    for (int64_t m0 = m_lo; m0 < m_hi; m0 += 64) {
        unsigned long long mask = __ballot(m0 + lane < m_hi && keys[m0 + lane] == key);
        while (mask) {
            const int j = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            a += rows[(m0 + j) * stride + field + lane];
        }
    }
    part[wv][lane] = a;
    __syncthreads();
    if (wv == 0) dst[(int64_t)key * RD + lane] += ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}

// ------------------------------------------------------------------------------------------------------------------- host
int64_t al256(int64_t b) { return (b + 255) / 256 * 256; }
int64_t cond_tiles(int64_t n_pair, int T) { const int S = TM + 1 - T; return (n_pair * T + S - 1) / S; }

struct CondWs { int64_t cum, ids, pos, part, slab, total, part_n; };
CondWs cond_ws(const dr4sr_regen_plan* plan, const ScoreOff& off, int64_t n_pair, int T) {
    CondWs w;
    const int64_t slots = cond_tiles(n_pair, T) * TM;
    w.part_n = plan->n_params - off.o[T_CENC];
    w.cum = 0;
    w.ids = cum_bytes(n_pair);
    w.pos = w.ids + al256(slots * 4);
    w.part = w.pos + al256(slots * 4);
    w.slab = w.part + al256(NSPLIT * w.part_n * 4);
    w.total = w.slab + al256(slots * TOKF * 4);
    return w;
}

struct ScoreWs { int64_t nll, ids, pos, sid, spos, lkey, dkv, delog, part, slab_d, slab_s, total, part_n, tiles; };
ScoreWs score_ws(const dr4sr_regen_plan* plan, const ScoreOff& off, int64_t n_pair, int Ls, int T, int n_w) {
    ScoreWs w;
    const int S = TM + 1 - T;
    w.tiles = (n_pair * n_w * T + S - 1) / S;
    w.part_n = off.o[T_CENC] - off.o[T_ENC];
    w.nll = al256(ws_bytes(n_pair, plan->K, Ls));                     // the forward's own workspace comes first: cum | ckv
    w.ids = w.nll + al256(n_pair * n_w * T * 4);
    w.pos = w.ids + al256(w.tiles * TM * 4);
    w.sid = w.pos + al256(w.tiles * TM * 4);
    w.spos = w.sid + al256(n_pair * Ls * 4);
    w.lkey = w.spos + al256(n_pair * Ls * 4);
    w.dkv = w.lkey + al256(n_pair * n_w * Ls * 4);
    w.delog = w.dkv + al256(n_pair * n_w * Ls * KVW * 4);
    w.part = w.delog + al256(n_pair * n_w * Ls * RD * 4);
    w.slab_d = w.part + al256(NSPLIT * w.part_n * 4);
    w.slab_s = w.slab_d + al256(w.tiles * TM * TOKD * 4);
    w.total = w.slab_s + al256(n_pair * Ls * TOKS * 4);
    return w;
}

void add_job(WJobs& js, int64_t out, int yoff, int N, int xoff, int Kd, int rep = 1, int ystep = 0, int xstep = 0) {
    WJob& j = js.j[js.n++];
    j.yoff = yoff; j.xoff = xoff; j.N = N; j.K = Kd; j.rep = rep; j.ystep = ystep; j.xstep = xstep; j.pad = 0;
    j.nkt = (Kd + 63) / 64;
    j.blk0 = js.nblk;
    j.out = out;
    js.nblk += ((N + 63) / 64) * j.nkt;
}
void add_linear(WJobs& js, const ScoreOff& off, int64_t base, int tensor_w, int yoff, int N, int xoff, int Kd) {     // weight, then its bias
    add_job(js, off.o[tensor_w] - base, yoff, N, xoff, Kd);
    add_job(js, off.o[tensor_w + 1] - base, yoff, N, -1, 1);
}
// the 12 tensors of an encoder layer whose records start at field f (the F_* layout)
void add_encoder_layer(WJobs& js, const ScoreOff& off, int64_t base, int t, int f) {
    add_linear(js, off, base, t + E_INW, f + F_DQKV, 3 * RD, f + F_X, RD);
    add_linear(js, off, base, t + E_OUTW, f + F_DV1, RD, f + F_O, RD);
    add_linear(js, off, base, t + E_W1, f + F_DHP, RF, f + F_X1, RD);
    add_linear(js, off, base, t + E_W2, f + F_DV2, RD, f + F_HH, RF);
    add_job(js, off.o[t + E_N1W] - base, f + F_G1, RD, -1, 1);
    add_job(js, off.o[t + E_N1B] - base, f + F_Y1, RD, -1, 1);
    add_job(js, off.o[t + E_N2W] - base, f + F_G2, RD, -1, 1);
    add_job(js, off.o[t + E_N2B] - base, f + F_Y2, RD, -1, 1);
}

int launch_wgrad(const WJobs& js, const float* slab, int stride, const int* cum, int64_t n_pair, int n_w, int S, int64_t fixed_m, float* part,
                 int64_t part_n, hipStream_t s) {
    hipLaunchKernelGGL(k_rsb_wgrad, dim3((unsigned)js.nblk, NSPLIT), dim3(256), 0, s, js, slab, stride, cum, (int)n_pair, n_w, S, fixed_m, part,
                       part_n);
    return DR4SR_LAUNCH_CHECK();
}
int launch_embed(int n_dst, const float* rows, int stride, int field, const int* keys, const int* cum, int64_t n_pair, int n_w, int S,
                 int64_t fixed_m, float* dst, hipStream_t s) {
    hipLaunchKernelGGL(k_rsb_embed, dim3((unsigned)n_dst), dim3(256), 0, s, rows, stride, field, keys, cum, (int)n_pair, n_w, S, fixed_m, dst);
    return DR4SR_LAUNCH_CHECK();
}
int zero_grad(const dr4sr_regen_plan* plan, float* grad, hipStream_t s) {
    hipLaunchKernelGGL(k_rsb_zero, dim3((unsigned)std::min<int64_t>((plan->n_params + 255) / 256, 4096)), dim3(256), 0, s, grad, plan->n_params);
    return DR4SR_LAUNCH_CHECK();
}

template <int KC, class... D>
int launch_bwd_source(const dr4sr_regen_plan* plan, const ScoreOff& off, const int64_t* src, const int64_t* src_len, int64_t n_pair, int Ls,
                      int causal, const float* w, int n_w, const float* dkv, float* slab, int* sid, int* spos, hipStream_t s, D... dp) {
    big_lds(k_rsb_source<KC, D...>, bwd_source_lds<KC>());
    hipLaunchKernelGGL((k_rsb_source<KC, D...>), dim3((unsigned)n_pair), dim3(NT), bwd_source_lds<KC>(), s, plan->params, off, plan->ln_eps,
                       plan->n_rows, src, src_len, Ls, causal, w, n_w, (int)n_pair, dkv, slab, sid, spos, dp...);
    return DR4SR_LAUNCH_CHECK();
}

// the raw dropout arguments of a *_train entry point; the eval entry points pass none
struct DropArgs { float p; uint64_t seed; uint32_t step; int64_t pair0; };
int check_drop(float p, int64_t pair0) { return (p >= 0.f && p < 1.f && pair0 >= 0 && pair0 < (1LL << 40)) ? 0 : DR4SR_E_ARG; }

}  // namespace

extern "C" int64_t dr4sr_regen_score_condition_bwd_workspace_bytes(const dr4sr_regen_plan* plan, int64_t n_pair, int32_t T) {
    if (const int rc = check_sizes(plan, n_pair, 1, T, 1)) return rc;
    return cond_ws(plan, offsets_of(plan), n_pair, T).total;
}

namespace {
template <class... D>
int condition_bwd(const dr4sr_regen_plan* plan, const int64_t* tgt, const int64_t* tgt_len, int64_t n_pair, int32_t T, const float* dlogits,
                  void* workspace, int64_t workspace_bytes, float* grad, int32_t accumulate, void* stream, D... dp) {
    if (const int rc = check_sizes(plan, n_pair, 1, T, 1)) return rc;
    if (!tgt || !tgt_len || !dlogits || !grad) return DR4SR_E_ARG;
    const ScoreOff off = offsets_of(plan);
    const CondWs w = cond_ws(plan, off, n_pair, T);
    if (!workspace || workspace_bytes < w.total) return DR4SR_E_WS;
    hipStream_t s = (hipStream_t)stream;
    if (!accumulate)
        if (const int rc = zero_grad(plan, grad, s)) return rc;
    if (n_pair == 0) return 0;
    char* base = static_cast<char*>(workspace);
    int* cum = reinterpret_cast<int*>(base + w.cum);
    int* ids = reinterpret_cast<int*>(base + w.ids);
    int* pos = reinterpret_cast<int*>(base + w.pos);
    float* part = reinterpret_cast<float*>(base + w.part);
    float* slab = reinterpret_cast<float*>(base + w.slab);
    const int S = TM + 1 - T, K = plan->K;
    hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(1024), 0, s, tgt_len, (int)n_pair, T, 0, cum);
    if (const int rc = DR4SR_LAUNCH_CHECK()) return rc;
    big_lds(k_rsb_cond_tile<D...>, BWD_TILE_LDS);
    hipLaunchKernelGGL((k_rsb_cond_tile<D...>), dim3((unsigned)cond_tiles(n_pair, T)), dim3(NT), BWD_TILE_LDS, s, plan->params, off, plan->ln_eps,
                       plan->n_rows, K, tgt, tgt_len, (int)n_pair, T, (const int*)cum, S, dlogits, slab, ids, pos, dp...);
    if (const int rc = DR4SR_LAUNCH_CHECK()) return rc;
    WJobs js;
    js.n = 0; js.nblk = 0;
    const int64_t pb = off.o[T_CENC];
    for (int l = 0; l < RNL; ++l) add_encoder_layer(js, off, pb, T_CENC + 12 * l, l * LF);
    add_linear(js, off, pb, T_CC0W, F_DHID, RD, F_POOL, RD);
    add_linear(js, off, pb, T_CC2W, F_DLOG, K, F_HID, RD);
    if (const int rc = launch_wgrad(js, slab, TOKF, cum, n_pair, 1, S, -1, part, w.part_n, s)) return rc;
    hipLaunchKernelGGL(k_rsb_reduce, dim3((unsigned)((w.part_n + 255) / 256)), dim3(256), 0, s, (const float*)part, w.part_n, w.part_n,
                       grad + off.o[T_CENC]);
    if (const int rc = DR4SR_LAUNCH_CHECK()) return rc;
    if (const int rc = launch_embed(plan->n_rows, slab, TOKF, F_DX0, ids, cum, n_pair, 1, S, -1, grad + off.o[T_E], s)) return rc;
    return launch_embed(LMAX, slab, TOKF, F_DX0, pos, cum, n_pair, 1, S, -1, grad + off.o[T_P], s);
}
}  // namespace

extern "C" int dr4sr_regen_score_condition_bwd(const dr4sr_regen_plan* plan, const int64_t* tgt, const int64_t* tgt_len, int64_t n_pair, int32_t T,
                                               const float* dlogits, void* workspace, int64_t workspace_bytes, float* grad, int32_t accumulate,
                                               void* stream) {
    return condition_bwd(plan, tgt, tgt_len, n_pair, T, dlogits, workspace, workspace_bytes, grad, accumulate, stream);
}

extern "C" int dr4sr_regen_score_condition_bwd_train(const dr4sr_regen_plan* plan, const int64_t* tgt, const int64_t* tgt_len, int64_t n_pair,
                                                     int32_t T, const float* dlogits, void* workspace, int64_t workspace_bytes, float* grad,
                                                     int32_t accumulate, float p, uint64_t seed, uint32_t step, int64_t pair0, void* stream) {
    if (const int rc = check_drop(p, pair0)) return rc;
    if (p == 0.f) return condition_bwd(plan, tgt, tgt_len, n_pair, T, dlogits, workspace, workspace_bytes, grad, accumulate, stream);
    return condition_bwd(plan, tgt, tgt_len, n_pair, T, dlogits, workspace, workspace_bytes, grad, accumulate, stream,
                         host_drop(p, seed, step, pair0));
}

extern "C" int64_t dr4sr_regen_score_bwd_workspace_bytes(const dr4sr_regen_plan* plan, int64_t n_pair, int32_t Ls, int32_t T, int32_t n_w) {
    if (const int rc = check_sizes(plan, n_pair, Ls, T, n_w)) return rc;
    return score_ws(plan, offsets_of(plan), n_pair, Ls, T, n_w).total;
}

namespace {
// `da` (the raw arguments, for the forward's own entry point) and `dp` (the policy the kernels take) come together or not at all
template <class... D>
int score_bwd(const dr4sr_regen_plan* plan, const int64_t* src, const int64_t* src_len, const int64_t* tgt, const int64_t* tgt_len,
              int64_t n_pair, int32_t Ls, int32_t T, const float* w, int32_t n_w, int32_t causal_source, const float* dnll, void* workspace,
              int64_t workspace_bytes, float* grad, float* dw, float* nll_or_null, int32_t accumulate, void* stream, const DropArgs* da, D... dp) {
    if (const int rc = check_sizes(plan, n_pair, Ls, T, n_w)) return rc;
    if (!src || !src_len || !tgt || !tgt_len || !w || !dnll || !grad || !dw) return DR4SR_E_ARG;
    const ScoreOff off = offsets_of(plan);
    const ScoreWs ws = score_ws(plan, off, n_pair, Ls, T, n_w);
    if (!workspace || workspace_bytes < ws.total) return DR4SR_E_WS;
    hipStream_t s = (hipStream_t)stream;
    if (!accumulate)
        if (const int rc = zero_grad(plan, grad, s)) return rc;
    if (n_pair == 0) return 0;
    char* base = static_cast<char*>(workspace);
    int* cum = reinterpret_cast<int*>(base);
    float* ckv = reinterpret_cast<float*>(base + cum_bytes(n_pair));
    float* nll = nll_or_null ? nll_or_null : reinterpret_cast<float*>(base + ws.nll);
    int* ids = reinterpret_cast<int*>(base + ws.ids);
    int* pos = reinterpret_cast<int*>(base + ws.pos);
    int* sid = reinterpret_cast<int*>(base + ws.sid);
    int* spos = reinterpret_cast<int*>(base + ws.spos);
    int* lkey = reinterpret_cast<int*>(base + ws.lkey);
    float* dkv = reinterpret_cast<float*>(base + ws.dkv);
    float* delog = reinterpret_cast<float*>(base + ws.delog);
    float* part = reinterpret_cast<float*>(base + ws.part);
    float* slab_d = reinterpret_cast<float*>(base + ws.slab_d);
    float* slab_s = reinterpret_cast<float*>(base + ws.slab_s);
    const int S = TM + 1 - T, K = plan->K;
    // the forward itself: the scan, every pair's K | V per condition and the NLLs stay in the first part of the workspace
    if (const int rc = da ? dr4sr_regen_score_train(plan, src, src_len, tgt, tgt_len, n_pair, Ls, T, w, n_w, causal_source, workspace,
                                                    ws_bytes(n_pair, K, Ls), nll, da->p, da->seed, da->step, da->pair0, stream)
                          : dr4sr_regen_score(plan, src, src_len, tgt, tgt_len, n_pair, Ls, T, w, n_w, causal_source, workspace,
                                              ws_bytes(n_pair, K, Ls), nll, stream)) return rc;
    constexpr size_t dec_lds = BWD_TILE_LDS + (sizeof...(D) ? DROP_KM_LDS : 0);
    big_lds(k_rsb_dec_tile<D...>, dec_lds);
    hipLaunchKernelGGL((k_rsb_dec_tile<D...>), dim3((unsigned)ws.tiles), dim3(NT), dec_lds, s, plan->params, off, plan->ln_eps, plan->n_rows, K,
                       src, src_len, Ls, tgt, tgt_len, (int)n_pair, T, w, n_w, (const int*)cum, S, (const float*)ckv, dnll, slab_d, ids, pos, dkv,
                       delog, lkey, dp...);
    if (const int rc = DR4SR_LAUNCH_CHECK()) return rc;
    hipLaunchKernelGGL(k_rsb_dw, dim3((unsigned)((n_pair * n_w + 3) / 4)), dim3(256), 0, s, (const float*)dkv, (const float*)ckv, K, (int)n_pair,
                       n_w, Ls, dw);
    if (const int rc = DR4SR_LAUNCH_CHECK()) return rc;
    int rc = with_kc(K, [&](auto kc) {
        return launch_bwd_source<decltype(kc)::value, D...>(plan, off, src, src_len, n_pair, Ls, causal_source != 0, w, n_w, dkv, slab_s, sid, spos,
                                                            s, dp...);
    });
    if (rc) return rc;
    const int64_t pb = off.o[T_ENC];
    WJobs jd;                                       // the decoder's slot records
    jd.n = 0; jd.nblk = 0;
    for (int l = 0; l < RNL; ++l) {
        const int f = l * LFD, t = T_DEC + 18 * l;
        add_linear(jd, off, pb, t + D_SAINW, f + R_DQKV, 3 * RD, f + R_X, RD);
        add_linear(jd, off, pb, t + D_SAOUTW, f + R_DV1, RD, f + R_O, RD);
        add_linear(jd, off, pb, t + D_CAINW, f + R_DQC, RD, f + R_X1, RD);          // the Q rows and the Q bias
        add_linear(jd, off, pb, t + D_CAOUTW, f + R_DV2, RD, f + R_OC, RD);
        add_linear(jd, off, pb, t + D_W1, f + R_DHP, RF, f + R_X2, RD);
        add_linear(jd, off, pb, t + D_W2, f + R_DV3, RD, f + R_HH, RF);
        add_job(jd, off.o[t + D_N1W] - pb, f + R_G1, RD, -1, 1);
        add_job(jd, off.o[t + D_N1B] - pb, f + R_Y1, RD, -1, 1);
        add_job(jd, off.o[t + D_N2W] - pb, f + R_G2, RD, -1, 1);
        add_job(jd, off.o[t + D_N2B] - pb, f + R_Y2, RD, -1, 1);
        add_job(jd, off.o[t + D_N3W] - pb, f + R_G3, RD, -1, 1);
        add_job(jd, off.o[t + D_N3B] - pb, f + R_Y3, RD, -1, 1);
    }
    add_job(jd, off.o[T_DEC_NORM] - pb, R_GN, RD, -1, 1);
    add_job(jd, off.o[T_DEC_NORM + 1] - pb, R_YN, RD, -1, 1);
    if ((rc = launch_wgrad(jd, slab_d, TOKD, cum, n_pair, n_w, S, -1, part, ws.part_n, s))) return rc;
    WJobs jsrc;                                     // the source records
    jsrc.n = 0; jsrc.nblk = 0;
    const int KD = K * RD;
    for (int l = 0; l < RNL; ++l) add_encoder_layer(jsrc, off, pb, T_ENC + 12 * l, l * LF);
    add_job(jsrc, off.o[T_ENC_NORM] - pb, S_GN, RD, -1, 1);
    add_job(jsrc, off.o[T_ENC_NORM + 1] - pb, S_YN, RD, -1, 1);
    add_linear(jsrc, off, pb, T_CL0W, S_DC1, KD, S_MEMN, RD);
    add_linear(jsrc, off, pb, T_CL2W, S_DMEM, KD, S_C1, KD);
    for (int l = 0; l < RNL; ++l)                   // the K | V rows of the decoder's cross-attention in_proj: summed over the conditions
        add_job(jsrc, off.o[T_DEC + 18 * l + D_CAINW] + RD * RD - pb, S_DCKV + l * K * 2 * RD, 2 * RD, S_MEM, RD, K, 2 * RD, RD);
    if ((rc = launch_wgrad(jsrc, slab_s, TOKS, cum, n_pair, n_w, S, n_pair * Ls, part, ws.part_n, s))) return rc;
    WJobs jb;                                       // the K | V bias: the mixed-memory gradient summed over rows and source positions
    jb.n = 0; jb.nblk = 0;
    for (int l = 0; l < RNL; ++l) add_job(jb, off.o[T_DEC + 18 * l + D_CAINB] + RD - pb, l * 2 * RD, 2 * RD, -1, 1);
    if ((rc = launch_wgrad(jb, dkv, KVW, cum, n_pair, n_w, S, n_pair * n_w * Ls, part, ws.part_n, s))) return rc;
    hipLaunchKernelGGL(k_rsb_reduce, dim3((unsigned)((ws.part_n + 255) / 256)), dim3(256), 0, s, (const float*)part, ws.part_n, ws.part_n,
                       grad + pb);
    if ((rc = DR4SR_LAUNCH_CHECK())) return rc;
    float* gE = grad + off.o[T_E];
    float* gP = grad + off.o[T_P];
    if ((rc = launch_embed(plan->n_rows, slab_d, TOKD, R_DX0, ids, cum, n_pair, n_w, S, -1, gE, s))) return rc;
    if ((rc = launch_embed(plan->n_rows, slab_s, TOKS, S_DX0, sid, cum, n_pair, n_w, S, n_pair * Ls, gE, s))) return rc;
    if ((rc = launch_embed(plan->n_rows, delog, RD, 0, lkey, cum, n_pair, n_w, S, n_pair * n_w * Ls, gE, s))) return rc;
    if ((rc = launch_embed(LMAX, slab_d, TOKD, R_DX0, pos, cum, n_pair, n_w, S, -1, gP, s))) return rc;
    return launch_embed(LMAX, slab_s, TOKS, S_DX0, spos, cum, n_pair, n_w, S, n_pair * Ls, gP, s);
}
}  // namespace

extern "C" int dr4sr_regen_score_bwd(const dr4sr_regen_plan* plan, const int64_t* src, const int64_t* src_len, const int64_t* tgt,
                                     const int64_t* tgt_len, int64_t n_pair, int32_t Ls, int32_t T, const float* w, int32_t n_w,
                                     int32_t causal_source, const float* dnll, void* workspace, int64_t workspace_bytes, float* grad, float* dw,
                                     float* nll_or_null, int32_t accumulate, void* stream) {
    return score_bwd(plan, src, src_len, tgt, tgt_len, n_pair, Ls, T, w, n_w, causal_source, dnll, workspace, workspace_bytes, grad, dw,
                     nll_or_null, accumulate, stream, nullptr);
}

extern "C" int dr4sr_regen_score_bwd_train(const dr4sr_regen_plan* plan, const int64_t* src, const int64_t* src_len, const int64_t* tgt,
                                           const int64_t* tgt_len, int64_t n_pair, int32_t Ls, int32_t T, const float* w, int32_t n_w,
                                           int32_t causal_source, const float* dnll, void* workspace, int64_t workspace_bytes, float* grad,
                                           float* dw, float* nll_or_null, int32_t accumulate, float p, uint64_t seed, uint32_t step, int64_t pair0,
                                           void* stream) {
    if (const int rc = check_drop(p, pair0)) return rc;
    if (p == 0.f)
        return score_bwd(plan, src, src_len, tgt, tgt_len, n_pair, Ls, T, w, n_w, causal_source, dnll, workspace, workspace_bytes, grad, dw,
                         nll_or_null, accumulate, stream, nullptr);
    const DropArgs da{p, seed, step, pair0};
    return score_bwd(plan, src, src_len, tgt, tgt_len, n_pair, Ls, T, w, n_w, causal_source, dnll, workspace, workspace_bytes, grad, dw,
                     nll_or_null, accumulate, stream, &da, host_drop(p, seed, step, pair0));
}
