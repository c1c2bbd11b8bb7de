// regen_head.hip — the condition head of the regenerator's pre-training step (DR4SR stage 2, 2.Pretrain_regenerator.py:270-292): the few
// [n_pair, K] operations between the condition encoder's logits and the decoder's condition weights, and back.
//   forward : w = softmax((cond_logits + g) / tau)  (F.gumbel_softmax's soft sample), the per-pair entropy terms -(w log(w + 1e-12)).sum(-1),
//             and dnll [1, n_pair, T] filled with 1 / n_tok (the loss's gradient with respect to every token NLL)
//   backward: dlogits = d(CE + entropy_weight * mean_over_batch(entropy)) / d cond_logits from dw (what dr4sr_regen_score_bwd returns), and
//             the step's two log entries (sum of the token NLLs / n_tok, sum of the entropy terms / n_batch), added to a slot
// One thread per pair, K <= 8 values in registers, plain fp32 (the two logs of the Gumbel transform run in double: near u = 1 / e the
// sample is near 0 and an fp32 -log(u) cannot carry it to fp32 ulps).  No atomics: a pair's values depend on its GLOBAL index pair0 + i
// alone, the log sums are added in a fixed order by one wave.  Both entry points only enqueue on the caller's stream.
#include "common.h"

#define HEAD_KMAX 8

// the Gumbel(0, 1) sample of one Philox word: u = ((r >> 8) + 0.5) 2^-24 in fp32 (csrc/linear.hip's u).  In fp32 the + 0.5 of the
// largest 24-bit value rounds up to 2^24, so u is held below 1: the largest fp32 under 1 (dr4sr_amd/regen_dropout.py gumbel_u is the mirror)
__device__ __forceinline__ float gumbel_of(const uint32_t r) {
    const float u = fminf(((float)(r >> 8) + 0.5f) * (1.0f / 16777216.0f), 0x1.fffffep-1f);
    return (float)(-log(-log((double)u)));
}

__global__ __launch_bounds__(64) void k_regen_head_fwd(const float* __restrict__ logits, const float* __restrict__ noise, const int n,
                                                       const int K, const int T, const float tau, const float inv_ntok, const uint32_t seed_lo,
                                                       const uint32_t seed_hi, const uint32_t step, const int64_t pair0, float* __restrict__ w,
                                                       float* __restrict__ ent, float* __restrict__ dnll, float* __restrict__ noise_out) {
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i < n) {
        float g[HEAD_KMAX];
        if (noise) {
#pragma unroll
            for (int k = 0; k < HEAD_KMAX; ++k) g[k] = k < K ? noise[(size_t)i * K + k] : 0.f;
        } else {                                          // element e = pair * 8 + k: word e & 3 of call e >> 2
            const uint64_t call = (uint64_t)(pair0 + i) * 2;
            const uint2 key = make_uint2(seed_lo, seed_hi);
            const uint4 r0 = philox4x32_10(make_uint4((uint32_t)call, (uint32_t)(call >> 32), DR4SR_REGEN_SITE_GUMBEL, step), key);
            g[0] = gumbel_of(r0.x); g[1] = gumbel_of(r0.y); g[2] = gumbel_of(r0.z); g[3] = gumbel_of(r0.w);
            g[4] = g[5] = g[6] = g[7] = 0.f;
            if (K > 4) {
                const uint64_t c1 = call + 1;
                const uint4 r1 = philox4x32_10(make_uint4((uint32_t)c1, (uint32_t)(c1 >> 32), DR4SR_REGEN_SITE_GUMBEL, step), key);
                g[4] = gumbel_of(r1.x); g[5] = gumbel_of(r1.y); g[6] = gumbel_of(r1.z); g[7] = gumbel_of(r1.w);
            }
        }
        float z[HEAD_KMAX], mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < HEAD_KMAX; ++k)
            if (k < K) { z[k] = (logits[(size_t)i * K + k] + g[k]) / tau; mx = fmaxf(mx, z[k]); }
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < HEAD_KMAX; ++k)
            if (k < K) { z[k] = expf(z[k] - mx); s += z[k]; }
        float h = 0.f;
#pragma unroll
        for (int k = 0; k < HEAD_KMAX; ++k)
            if (k < K) {
                const float wk = z[k] / s;
                w[(size_t)i * K + k] = wk;
                h += wk * logf(wk + 1e-12f);
                if (noise_out) noise_out[(size_t)i * K + k] = g[k];
            }
        ent[i] = -h;
    }
    const int64_t total = (int64_t)n * T, stride = (int64_t)gridDim.x * 64;
    for (int64_t j = i; j < total; j += stride) dnll[j] = inv_ntok;
}

// blocks 0 .. gridDim.x - 2: one thread per pair; the LAST block (when loss_log or ent_log is given) is the log's: one wave sums nll and
// ent, each lane its strided share in index order, then the butterfly (a fixed order: the same inputs give the same bits)
__global__ __launch_bounds__(64) void k_regen_head_bwd(const float* __restrict__ dw, const float* __restrict__ w, const float* __restrict__ ent,
                                                       const float* __restrict__ nll, const int n, const int K, const int T, const float tau,
                                                       const float ent_scale, const float n_tok, const float n_batch, const int pair_blocks,
                                                       float* __restrict__ dlogits, float* __restrict__ loss_log, float* __restrict__ ent_log,
                                                       const int64_t slot) {
    if ((int)blockIdx.x >= pair_blocks) {
        const int lane = (int)threadIdx.x;
        if (loss_log) {
            float a = 0.f;
            for (int64_t j = lane; j < (int64_t)n * T; j += 64) a += nll[j];
            a = wave_sum(a);
            if (lane == 0) loss_log[slot] += a / n_tok;
        }
        if (ent_log) {
            float b = 0.f;
            for (int j = lane; j < n; j += 64) b += ent[j];
            b = wave_sum(b);
            if (lane == 0) ent_log[slot] += b / n_batch;
        }
        return;
    }
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= n) return;
    float wv[HEAD_KMAX], u[HEAD_KMAX], s = 0.f;
#pragma unroll
    for (int k = 0; k < HEAD_KMAX; ++k)
        if (k < K) {
            wv[k] = w[(size_t)i * K + k];
            const float we = wv[k] + 1e-12f;
            u[k] = dw[(size_t)i * K + k] + ent_scale * (-logf(we) - wv[k] / we);
            s += wv[k] * u[k];
        }
#pragma unroll
    for (int k = 0; k < HEAD_KMAX; ++k)
        if (k < K) dlogits[(size_t)i * K + k] = wv[k] * (u[k] - s) / tau;
}

static int head_args_ok(const int64_t n_pair, const int32_t K, const int32_t T, const float tau) {
    return n_pair >= 1 && n_pair < (1 << 24) && K >= 1 && K <= HEAD_KMAX && T >= 1 && T <= 50 && tau > 0.f;
}

extern "C" int dr4sr_regen_head_fwd(const float* cond_logits, const float* noise_or_null, int64_t n_pair, int32_t K, int32_t T, float tau,
                                    int64_t n_tok, uint64_t seed, uint32_t step, int64_t pair0, float* w, float* ent, float* dnll,
                                    float* noise_out_or_null, void* stream) {
    if (!cond_logits || !w || !ent || !dnll || !head_args_ok(n_pair, K, T, tau) || n_tok < 1 || pair0 < 0 || pair0 >= ((int64_t)1 << 40))
        return DR4SR_E_ARG;
    const float inv_ntok = (float)(1.0 / (double)n_tok);
    const int blocks = (int)((n_pair + 63) / 64);
    hipLaunchKernelGGL(k_regen_head_fwd, dim3(blocks), dim3(64), 0, (hipStream_t)stream, cond_logits, noise_or_null, (int)n_pair, K, T, tau,
                       inv_ntok, (uint32_t)seed, (uint32_t)(seed >> 32), step, pair0, w, ent, dnll, noise_out_or_null);
    return DR4SR_LAUNCH_CHECK();
}

extern "C" int dr4sr_regen_head_bwd(const float* dw, const float* w, const float* ent, const float* nll, int64_t n_pair, int32_t K, int32_t T,
                                    float tau, float entropy_weight, int64_t n_batch, int64_t n_tok, float* dlogits, float* loss_log_or_null,
                                    float* ent_log_or_null, int64_t slot, void* stream) {
    if (!dw || !w || !ent || !dlogits || !head_args_ok(n_pair, K, T, tau) || n_batch < n_pair || n_tok < 1 || slot < 0) return DR4SR_E_ARG;
    if (loss_log_or_null && !nll) return DR4SR_E_ARG;
    const int pair_blocks = (int)((n_pair + 63) / 64);
    const int log_block = (loss_log_or_null || ent_log_or_null) ? 1 : 0;
    hipLaunchKernelGGL(k_regen_head_bwd, dim3(pair_blocks + log_block), dim3(64), 0, (hipStream_t)stream, dw, w, ent, nll, (int)n_pair, K, T, tau,
                       entropy_weight / (float)n_batch, (float)n_tok, (float)n_batch, pair_blocks, dlogits, loss_log_or_null, ent_log_or_null, slot);
    return DR4SR_LAUNCH_CHECK();
}
