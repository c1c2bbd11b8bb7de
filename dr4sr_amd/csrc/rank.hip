// rank.hip — evaluation by TARGET RANK: every rank metric of a row with one target is a function of one integer,
//
//     rank(b) = #{ valid items j : s(b, j) > s(b, t_b), or s(b, j) == s(b, t_b) and j < t_b }
//
// with the validity rules of dr4sr_full_score_topk_masked_ws (topk.hip): 1 <= j < n_items, not blocked, not in the row's history.
// That is the GEMM of the top-k with a compare-and-count epilogue: no [B, N] score matrix, no selection, no sort, no candidates.
//
// dr4sr_target_rank, two launches:
//   k_rank_target: one workgroup per 64 rows stages E[target[b]] as the ITEM tile of the MFMA loop of k_score_gemm and keeps the
//                  diagonal: s_t[b] goes through the same instructions in the same k order as column t_b of the score matrix, so it is
//                  bit-identical to it (an output element's accumulation order depends on k alone) and "rank < k" means "the top-k call
//                  returns the target at position rank" for arbitrary floats.  The launch also resolves the target's validity (range,
//                  blocked, the row's Lh history words) and initialises rank_out[b] to 0, or to DR4SR_RANK_NONE for an invalid target.
//   k_rank_count : k_score_emit's structure — 64 rows x a chunk of 8 item tiles per workgroup, Q tile in LDS once — with a 64 x 512-bit
//                  LDS mask of the chunk's history hits (LDS atomicOr: duplicates and foreign words fall out) and a compare per
//                  accumulator element.  The compare is a wave ballot: the 32 lanes of a half-wave hold 32 items of ONE row, so the
//                  popcount of each half of the ballot is that row's count for the tile, kept in scalar registers.  Counts meet in LDS
//                  integer atomics and leave with one global integer atomicAdd per (row, workgroup).  Integer adds only: two calls on
//                  the same inputs are bitwise equal.
//
// dr4sr_rank_metrics_accumulate: one launch of one workgroup ADDS the row count and, per cutoff, the seven metric sums of a batch to
// a device accumulator in fp64, in a fixed order (a thread's rows ascending, xor butterfly over the wave, waves 0..3).
#include "common.h"
#include "kernels.h"

extern __shared__ __attribute__((aligned(16))) float smem[];

constexpr int RANK_TILES = 8;                              // 512 items per workgroup of k_rank_count

// workspace: [B] fp32 s_t (+inf for an invalid target) | [B] int32 target id (-1 for an invalid target)
template <int D>
__global__ __launch_bounds__(256) void k_rank_target(const float* __restrict__ Q, const float* __restrict__ E,
                                                     const int64_t* __restrict__ target, const int64_t* __restrict__ hist,
                                                     const uint8_t* __restrict__ blocked, float* __restrict__ s_out,
                                                     int* __restrict__ t_out, int* __restrict__ rank_out, int B, int n_items, int Lh) {
    constexpr int LD = D + 1;                              // odd stride, as in k_score_gemm
    float* Qs = smem;                                      // [64][LD]
    float* Es = smem + 64 * LD;                            // [64][LD]
    int* bad = reinterpret_cast<int*>(Es + 64 * LD);       // [64] 1 = the target is in the row's history
    const int b0 = blockIdx.x * 64;
    if (threadIdx.x < 64) bad[threadIdx.x] = 0;
    for (int e = threadIdx.x; e < 64 * (D / 4); e += 256) {
        const int r = e / (D / 4), c = (e % (D / 4)) * 4;
        float4 qv = make_float4(0.f, 0.f, 0.f, 0.f), ev = qv;
        if (b0 + r < B) {
            qv = ld4(Q + (size_t)(b0 + r) * D + c);
            const int64_t t = target[b0 + r];
            if (t >= 0 && t < n_items) ev = ld4(E + (size_t)t * D + c);
        }
        float* qd = Qs + r * LD + c; qd[0] = qv.x; qd[1] = qv.y; qd[2] = qv.z; qd[3] = qv.w;
        float* ed = Es + r * LD + c; ed[0] = ev.x; ed[1] = ev.y; ed[2] = ev.z; ed[3] = ev.w;
    }
    __syncthreads();
    {   // four threads per row scan the row's history for the target (an int64 compare: a foreign word equals no valid target)
        const int rl = threadIdx.x >> 2, b = b0 + rl;
        if (b < B) {
            const int64_t t = target[b];
            bool hit = false;
            for (int j = threadIdx.x & 3; j < Lh; j += 4) hit |= hist[(size_t)b * Lh + j] == t;
            if (hit) atomicOr(&bad[rl], 1);
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, g = lane >> 5;
    const int rt = w >> 1, ct = w & 1;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    const float* ap = Qs + (rt * 32 + r) * LD + g;
    const float* bp = Es + (ct * 32 + r) * LD + g;
#pragma unroll 8
    for (int sidx = 0; sidx < D / 2; ++sidx) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * sidx], bp[2 * sidx], acc, 0, 0, 0);
    __syncthreads();                                       // bad[] is complete
    if (rt != ct) return;                                  // the diagonal lives in the two diagonal quadrants
    float s = 0.f;
    bool mine = false;
#pragma unroll
    for (int e = 0; e < 16; ++e)
        if ((e & 3) + 8 * (e >> 2) + 4 * g == r) { s = acc[e]; mine = true; }
    const int rl = rt * 32 + r, b = b0 + rl;
    if (!mine || b >= B) return;
    const int64_t t = target[b];
    const bool valid = t >= 1 && t < n_items && !(blocked && blocked[t]) && !bad[rl];
    s_out[b] = valid ? s : INFINITY;
    t_out[b] = valid ? (int)t : -1;
    rank_out[b] = valid ? 0 : DR4SR_RANK_NONE;
}

template <int D>
__global__ __launch_bounds__(256) void k_rank_count(const float* __restrict__ Q, const float* __restrict__ E,
                                                    const int64_t* __restrict__ hist, const uint8_t* __restrict__ blocked,
                                                    const float* __restrict__ s_t, const int* __restrict__ t_id,
                                                    int* __restrict__ rank_out, int B, int n_items, int Lh) {
    constexpr int LD = D + 1;
    float* Qs = smem;                                      // [64][LD]
    float* Es = smem + 64 * LD;                            // [64][LD]
    unsigned* mask = reinterpret_cast<unsigned*>(Es + 64 * LD);      // [64][16]: bit i of row rl = item chunk0 + i is in the row's history
    int* cnt = reinterpret_cast<int*>(mask + 64 * 16);     // [64]
    const int b0 = blockIdx.y * 64, tile0 = blockIdx.x * RANK_TILES, ntile = (n_items + 63) / 64;
    for (int e = threadIdx.x; e < 64 * (D / 4); e += 256) {
        const int r = e / (D / 4), c = (e % (D / 4)) * 4;
        float4 qv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (b0 + r < B) qv = ld4(Q + (size_t)(b0 + r) * D + c);
        float* qd = Qs + r * LD + c; qd[0] = qv.x; qd[1] = qv.y; qd[2] = qv.z; qd[3] = qv.w;
    }
    for (int i = threadIdx.x; i < 64 * 16; i += 256) mask[i] = 0u;
    if (threadIdx.x < 64) cnt[threadIdx.x] = 0;
    __syncthreads();
    {
        const int64_t lo = (int64_t)tile0 * 64;
        const int64_t hi = lo + RANK_TILES * 64 < n_items ? lo + RANK_TILES * 64 : (int64_t)n_items;
        for (int i = threadIdx.x; i < 64 * Lh; i += 256) {
            const int rl = i / Lh, j = i - rl * Lh;
            if (b0 + rl >= B) break;                       // rl ascends with i
            const int64_t h = hist[(size_t)(b0 + rl) * Lh + j];
            if (h >= lo && h < hi) { const int bit = (int)(h - lo); atomicOr(&mask[rl * 16 + (bit >> 5)], 1u << (bit & 31)); }
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, g = lane >> 5;
    const int rt = w >> 1, ct = w & 1;
    // the lane's 16 rows never change: their target score and id stay in registers (+inf / -1: nothing counts)
    float st[16];
    int tg[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int b = b0 + rt * 32 + (e & 3) + 8 * (e >> 2) + 4 * g;
        st[e] = b < B ? s_t[b] : INFINITY;
        tg[e] = b < B ? t_id[b] : -1;
    }
    int c0[16], c1[16];                                    // wave-uniform: the counts of the rows of half-wave 0 / 1
#pragma unroll
    for (int e = 0; e < 16; ++e) { c0[e] = 0; c1[e] = 0; }
    for (int tile = tile0; tile < tile0 + RANK_TILES && tile < ntile; ++tile) {
        const int n0 = tile * 64;
        __syncthreads();                                   // the previous tile's MFMAs have read Es (first pass: the mask is complete)
        for (int e = threadIdx.x; e < 64 * (D / 4); e += 256) {
            const int rr = e / (D / 4), c = (e % (D / 4)) * 4;
            float4 ev = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n0 + rr < n_items) ev = ld4(E + (size_t)(n0 + rr) * D + c);
            float* ed = Es + rr * LD + c; ed[0] = ev.x; ed[1] = ev.y; ed[2] = ev.z; ed[3] = ev.w;
        }
        __syncthreads();
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        const float* ap = Qs + (rt * 32 + r) * LD + g;
        const float* bp = Es + (ct * 32 + r) * LD + g;
#pragma unroll 8
        for (int sidx = 0; sidx < D / 2; ++sidx) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * sidx], bp[2 * sidx], acc, 0, 0, 0);
        const int n = n0 + ct * 32 + r;
        const bool off = n == 0 || n >= n_items || (blocked && blocked[n]);
        const int mw = (tile - tile0) * 2 + ct;            // the mask word of this wave's 32 items; the lane's item is bit r
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int rl = rt * 32 + (e & 3) + 8 * (e >> 2) + 4 * g;
            const bool hbit = (mask[rl * 16 + mw] >> r) & 1u;
            const bool before = !off && !hbit && (acc[e] > st[e] || (acc[e] == st[e] && n < tg[e]));
            const unsigned long long bal = __ballot(before);
            c0[e] += __builtin_popcount((unsigned)bal);
            c1[e] += __builtin_popcount((unsigned)(bal >> 32));
        }
    }
    if (r == 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int c = g ? c1[e] : c0[e];
            if (c) atomicAdd(&cnt[rt * 32 + (e & 3) + 8 * (e >> 2) + 4 * g], c);
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int b = b0 + threadIdx.x, c = cnt[threadIdx.x];
        if (b < B && c > 0 && t_id[b] >= 0) atomicAdd(rank_out + b, c);
    }
}

extern "C" int64_t dr4sr_target_rank_workspace_bytes(int64_t B) {
    if (B < 0) return DR4SR_E_ARG;
    return B * 8 + 256;
}

extern "C" int dr4sr_target_rank(const float* q, const float* E, const int64_t* target, const int64_t* hist, const uint8_t* item_blocked,
                                 int32_t* rank_out, int64_t B, int32_t D, int32_t n_items, int32_t Lh, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
    if (B < 0 || B > 65535ll * 64 || n_items < 2 || Lh < 0 || Lh > (1 << 20)) return DR4SR_E_ARG;
    if (D != 64 && D != 128) return DR4SR_E_SHAPE;
    if (B == 0) return 0;
    if (!q || !E || !target || !rank_out || (Lh > 0 && !hist)) return DR4SR_E_ARG;
    if (!workspace || workspace_bytes < B * 8) return DR4SR_E_WS;
    hipStream_t s = (hipStream_t)stream;
    float* s_t = reinterpret_cast<float*>(workspace);
    int* t_id = reinterpret_cast<int*>(s_t + B);
    const int ntile = (n_items + 63) / 64;
    const dim3 gt((unsigned)((B + 63) / 64)), gc((unsigned)((ntile + RANK_TILES - 1) / RANK_TILES), (unsigned)((B + 63) / 64));
    const size_t lds_t = sizeof(float) * 2 * 64 * (D + 1) + sizeof(int) * 64;
    const size_t lds_c = sizeof(float) * 2 * 64 * (D + 1) + sizeof(unsigned) * 64 * 16 + sizeof(int) * 64;
    if (D == 64) {
        hipLaunchKernelGGL(k_rank_target<64>, gt, dim3(256), lds_t, s, q, E, target, hist, item_blocked, s_t, t_id, rank_out, (int)B, n_items, Lh);
        hipLaunchKernelGGL(k_rank_count<64>, gc, dim3(256), lds_c, s, q, E, hist, item_blocked, s_t, t_id, rank_out, (int)B, n_items, Lh);
    } else {
        big_lds(k_rank_target<128>, lds_t);
        big_lds(k_rank_count<128>, lds_c);
        hipLaunchKernelGGL(k_rank_target<128>, gt, dim3(256), lds_t, s, q, E, target, hist, item_blocked, s_t, t_id, rank_out, (int)B, n_items, Lh);
        hipLaunchKernelGGL(k_rank_count<128>, gc, dim3(256), lds_c, s, q, E, hist, item_blocked, s_t, t_id, rank_out, (int)B, n_items, Lh);
    }
    return DR4SR_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------ metric sums on the device
// per-row values of the reference's evaluation/__init__.py for ONE target per row, in fp64: h = [rank < c], count = [label > 0]
//   ndcg = label <= eps ? 0 : h / log2(rank + 2)     recall = h / count     precision = h / c     map = h (1 / (rank + 1)) / min(count, c)
//   mrr = h ? 1 / (rank + 1) : 0                     hit = h                f1 = 2 h / (count + c)
struct RankCuts { int c[8]; };

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_rank_metrics(const int* __restrict__ rank, const float* __restrict__ label, long long B,
                                                      const RankCuts cuts, int n_cut, double* __restrict__ acc) {
    __shared__ double part[4][7];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const double eps = 2.220446049250313e-16;              // sys.float_info.epsilon
    for (int ci = 0; ci < n_cut; ++ci) {
        const int c = cuts.c[ci];
        double s_ndcg = 0., s_rec = 0., s_prec = 0., s_map = 0., s_mrr = 0., s_hit = 0., s_f1 = 0.;
        for (long long i = tid; i < B; i += 256) {
            const int rk = rank[i];
            const double lab = (double)label[i];
            const bool hb = rk < c;
            const double h = hb ? 1. : 0., count = lab > 0. ? 1. : 0.;
            const double inv = 1. / ((double)rk + 1.);
            s_ndcg += lab <= eps ? 0. : (hb ? h / log2((double)rk + 2.) : 0.);
            s_rec += h / count;
            s_prec += h / (double)c;
            s_map += h * inv / fmin(count, (double)c);
            s_mrr += hb ? inv : 0.;
            s_hit += h;
            s_f1 += 2. * h / (count + (double)c);
        }
        s_ndcg = wave_sum_d(s_ndcg); s_rec = wave_sum_d(s_rec); s_prec = wave_sum_d(s_prec); s_map = wave_sum_d(s_map);
        s_mrr = wave_sum_d(s_mrr); s_hit = wave_sum_d(s_hit); s_f1 = wave_sum_d(s_f1);
        __syncthreads();                                   // the previous cutoff's part[] has been read
        if (lane == 0) {
            part[w][0] = s_ndcg; part[w][1] = s_rec; part[w][2] = s_prec; part[w][3] = s_map;
            part[w][4] = s_mrr; part[w][5] = s_hit; part[w][6] = s_f1;
        }
        __syncthreads();
        if (tid < 7) acc[1 + 7 * ci + tid] += ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    }
    if (tid == 0) acc[0] += (double)B;
}

extern "C" int dr4sr_rank_metrics_accumulate(const int32_t* rank, const float* label, int64_t B, const int32_t* cutoffs, int32_t n_cut,
                                             int32_t topk, double* acc, void* stream) {
    if (B < 0 || !cutoffs || n_cut < 1 || n_cut > 8 || topk < 1 || !acc) return DR4SR_E_ARG;
    RankCuts cuts{};
    for (int i = 0; i < n_cut; ++i) {
        if (cutoffs[i] < 1 || cutoffs[i] > topk) return DR4SR_E_ARG;        // the reference's map breaks for a cutoff above topk
        cuts.c[i] = cutoffs[i];
    }
    if (B == 0) return 0;
    if (!rank || !label) return DR4SR_E_ARG;
    hipLaunchKernelGGL(k_rank_metrics, dim3(1), dim3(256), 0, (hipStream_t)stream, rank, label, (long long)B, cuts, n_cut, acc);
    return DR4SR_LAUNCH_CHECK();
}
