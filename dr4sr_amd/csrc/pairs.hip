// pairs.hip — the regenerator's pre-training pairs (DR4SR stage 1, the reference's 1.Build_pretraining_dataset.py:70-93): for every
// training sequence, which mined patterns are subsequences of it, and a uniformly random min(10, m) of those m in uniformly random order.
//
// The reference shuffles the WHOLE pattern list once per sequence and walks it with a pure-Python subsequence test until ten patterns
// matched.  Here every (sequence i, pattern j) pair is tested once, and the random order comes from a counter-based key:
//
//   key(i, j) = philox4x32_10(counter = (i, j, 0x50414952 "PAIR", 0), key = (seed & 0xffffffff, seed >> 32)).x
//
// with i the sequence's index in the file (seq_index0 + its row in this call) and j the pattern's index in the list (pat_index0 + its
// row in this call), both as uint32.  The chosen patterns of sequence i are the min(10, m_i) matching ones with the smallest
// (key, j), in ascending (key, j) order — the order of the 64-bit word key << 32 | j.  That is a pure function of (seed, i, j): it does
// not depend on the tile, on the launch geometry, on how sequences or patterns are chunked, or on what else is in the batch.
//
//   k_pairs_sig      per pattern: a 128-bit signature (bit (id * 0x9E3779B1 mod 2^32) >> 25 set for each of its ids), its offset and
//                    its length.  Offsets that are not monotonic inside [0, n_ids], empty patterns and patterns of more than 64 ids get
//                    length 0 = "never matches", so nothing is ever read out of bounds.
//   k_pairs_match    a workgroup owns a tile of 32 sequences (ids, lengths and signatures in LDS) and one chunk of the pattern list;
//                    each of its 4 waves streams 64 patterns at a time, one per lane.  Per sequence of the tile (uniform loop, LDS
//                    broadcast reads): reject unless plen <= slen and psig & ~ssig == 0 (almost every pair stops here), survivors run
//                    the greedy left-most scan of is_sublist against the LDS copy.  Matches of a wave are counted with one ballot and
//                    inserted one by one into the wave's own sorted top-10 of that sequence (lane l owns slot l, so a wave never
//                    shares a slot with another); a match whose word is not below the current tenth is only counted.  The 4 waves'
//                    lists are merged at the end and written as the (tile, chunk) partial result.
//   k_pairs_merge    one thread per sequence: the 10 smallest words over the chunks' ascending partial lists, the sum of their counts.
// The top-10 of a union is the top-10 of the union of the parts' top-10s, so the result is the same for any number of chunks.
#include "common.h"

namespace {

constexpr int PT_TS = 32;      // sequences per tile
constexpr int PT_L = 64;       // longest sequence (Lmax <= 64)
constexpr int PT_NT = 256;
constexpr int PT_NW = PT_NT / DR4SR_WAVE;
constexpr int PT_K = 10;       // patterns kept per sequence (1.Build_pretraining_dataset.py:88)
constexpr int PT_MAX_CHUNKS = 64;
constexpr uint32_t PT_SITE = 0x50414952u;
constexpr unsigned long long PT_EMPTY = ~0ull;

__device__ __forceinline__ void sig_add(uint4& s, const int32_t id) {
    const uint32_t bit = ((uint32_t)id * 0x9E3779B1u) >> 25, m = 1u << (bit & 31u), q = bit >> 5;
    s.x |= q == 0 ? m : 0u;
    s.y |= q == 1 ? m : 0u;
    s.z |= q == 2 ? m : 0u;
    s.w |= q == 3 ? m : 0u;
}

__global__ void k_pairs_sig(const int32_t* __restrict__ pat_ids, const int64_t* __restrict__ pat_off, const int64_t n_ids, const int64_t P,
                            uint4* __restrict__ sig, int2* __restrict__ meta) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= P) return;
    const int64_t a = pat_off[j], b = pat_off[j + 1];
    const bool ok = a >= 0 && b > a && b <= n_ids && b - a <= PT_L;
    uint4 s = make_uint4(0u, 0u, 0u, 0u);
    if (ok)
        for (int64_t k = a; k < b; ++k) sig_add(s, pat_ids[k]);
    sig[j] = s;
    meta[j] = make_int2(ok ? (int)a : 0, ok ? (int)(b - a) : 0);
}

// the PT_K smallest words of n sorted-or-not candidates read through `at`, ascending, PT_EMPTY padded (words of real matches are distinct)
template <typename At, typename Put>
__device__ __forceinline__ void smallest_k(const int n, At at, Put put) {
    unsigned long long last = 0;
    bool first = true;
    for (int o = 0; o < PT_K; ++o) {
        unsigned long long best = PT_EMPTY;
        if (first || last != PT_EMPTY)
            for (int e = 0; e < n; ++e) {
                const unsigned long long v = at(e);
                if ((first || v > last) && v < best) best = v;
            }
        put(o, best);
        last = best;
        first = false;
    }
}

__global__ __launch_bounds__(PT_NT) void k_pairs_match(const int32_t* __restrict__ seqs, const int32_t* __restrict__ seq_len, const int64_t S,
                                                       const int Lmax, const int32_t* __restrict__ pat_ids, const uint4* __restrict__ sig,
                                                       const int2* __restrict__ meta, const int64_t P, const int64_t pat_per_chunk,
                                                       const int n_chunks, const uint32_t seed_lo, const uint32_t seed_hi,
                                                       const uint32_t seq_index0, const uint32_t pat_index0,
                                                       unsigned long long* __restrict__ part_list, int32_t* __restrict__ part_cnt) {
    __shared__ int32_t s_seq[PT_TS][PT_L];
    __shared__ uint4 s_sig[PT_TS];
    __shared__ int s_len[PT_TS];
    __shared__ unsigned long long s_list[PT_NW][PT_TS][PT_K];
    __shared__ int s_cnt[PT_NW][PT_TS];
    const int tid = threadIdx.x, lane = tid & (DR4SR_WAVE - 1), w = tid / DR4SR_WAVE;
    const int64_t s0 = (int64_t)blockIdx.x * PT_TS;

    if (tid < PT_TS) {
        const int64_t gi = s0 + tid;
        int n = gi < S ? seq_len[gi] : 0;
        n = n < 0 ? 0 : (n > Lmax ? Lmax : n);
        uint4 sg = make_uint4(0u, 0u, 0u, 0u);
        for (int c = 0; c < n; ++c) sig_add(sg, seqs[gi * Lmax + c]);
        s_len[tid] = n;
        s_sig[tid] = sg;
    }
    for (int e = tid; e < PT_TS * PT_L; e += PT_NT) {
        const int r = e / PT_L, c = e % PT_L;
        const int64_t gi = s0 + r;
        s_seq[r][c] = (gi < S && c < Lmax) ? seqs[gi * Lmax + c] : -1;      // entries at or past the row's length are never compared
    }
    for (int e = tid; e < PT_NW * PT_TS * PT_K; e += PT_NT) (&s_list[0][0][0])[e] = PT_EMPTY;
    if (tid < PT_NW * PT_TS) (&s_cnt[0][0])[tid] = 0;
    __syncthreads();

    const int chunk = blockIdx.y;
    const int64_t p_begin = (int64_t)chunk * pat_per_chunk;
    const int64_t p_end = p_begin + pat_per_chunk < P ? p_begin + pat_per_chunk : P;
    for (int64_t base = p_begin + (int64_t)w * DR4SR_WAVE; base < p_end; base += PT_NT) {
        const int64_t j = base + lane;
        const bool live = j < p_end;
        const uint4 ps = live ? sig[j] : make_uint4(0u, 0u, 0u, 0u);
        const int2 pm = live ? meta[j] : make_int2(0, 0);
        const int plen = pm.y;
        const uint32_t jj = pat_index0 + (uint32_t)j;
        for (int s = 0; s < PT_TS; ++s) {
            const int slen = s_len[s];
            if (slen == 0) continue;                                       // uniform: an empty row (or one past S) matches nothing
            const uint4 ss = s_sig[s];
            bool match = false;
            if (plen >= 1 && plen <= slen && ((ps.x & ~ss.x) | (ps.y & ~ss.y) | (ps.z & ~ss.z) | (ps.w & ~ss.w)) == 0u) {
                int k = 0;
                int32_t want = pat_ids[pm.x];
                for (int t = 0; t < slen; ++t) {
                    if (s_seq[s][t] == want) {
                        if (++k == plen) { match = true; break; }
                        want = pat_ids[pm.x + k];
                    }
                    if (slen - t - 1 < plen - k) break;                   // not enough ids left
                }
            }
            unsigned long long mask = __ballot(match);
            if (mask == 0ull) continue;
            if (lane == 0) s_cnt[w][s] += __popcll(mask);
            unsigned long long word = PT_EMPTY;
            if (match) {
                const uint32_t key = philox4x32_10(make_uint4(seq_index0 + (uint32_t)(s0 + s), jj, PT_SITE, 0u), make_uint2(seed_lo, seed_hi)).x;
                word = ((unsigned long long)key << 32) | jj;
            }
            unsigned long long cur = lane < PT_K ? s_list[w][s][lane] : PT_EMPTY;      // lane l owns slot l of its wave's list
            while (mask) {
                const int src = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const unsigned long long v = ((unsigned long long)(uint32_t)__shfl((int)(word >> 32), src) << 32)
                                             | (uint32_t)__shfl((int)(word & 0xffffffffull), src);
                const int pos = __popcll(__ballot(lane < PT_K && cur < v));
                if (pos >= PT_K) continue;                                 // not below the current tenth: counted only
                const unsigned long long prev = ((unsigned long long)(uint32_t)__shfl_up((int)(cur >> 32), 1) << 32)
                                                | (uint32_t)__shfl_up((int)(cur & 0xffffffffull), 1);
                if (lane == pos) cur = v;
                else if (lane > pos) cur = prev;
            }
            if (lane < PT_K) s_list[w][s][lane] = cur;
        }
    }
    __syncthreads();

    if (tid < PT_TS && s0 + tid < S) {
        const int64_t o = (s0 + tid) * n_chunks + chunk;
        int n = 0;
        for (int q = 0; q < PT_NW; ++q) n += s_cnt[q][tid];
        part_cnt[o] = n;
        smallest_k(PT_NW * PT_K, [&](int e) { return s_list[e / PT_K][tid][e % PT_K]; },
                   [&](int slot, unsigned long long v) { part_list[o * PT_K + slot] = v; });
    }
}

// every chunk's list is ascending, so its candidate in a round is its first word above the last one taken: a round reads about one word
// per chunk (the heads have moved by at most PT_K in total), not all 10 (the plain 10-rounds-over-everything form took 0.54 ms at 27 chunks)
__global__ void k_pairs_merge(const unsigned long long* __restrict__ part_list, const int32_t* __restrict__ part_cnt, const int64_t S,
                              const int n_chunks, int32_t* __restrict__ n_match, int32_t* __restrict__ chosen) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    int n = 0;
    for (int c = 0; c < n_chunks; ++c) n += part_cnt[i * n_chunks + c];
    n_match[i] = n;
    const unsigned long long* mine = part_list + i * n_chunks * PT_K;
    unsigned long long last = 0;
    for (int o = 0; o < PT_K; ++o) {
        unsigned long long best = PT_EMPTY;
        if (o == 0 || last != PT_EMPTY)
            for (int c = 0; c < n_chunks; ++c)
                for (int e = 0; e < PT_K; ++e) {
                    const unsigned long long v = mine[c * PT_K + e];
                    if (o > 0 && v <= last) continue;
                    best = v < best ? v : best;
                    break;
                }
        chosen[i * PT_K + o] = best == PT_EMPTY ? -1 : (int32_t)(uint32_t)(best & 0xffffffffull);
        last = best;
    }
}

// chunks of the pattern list: the caller's value, or about 16 K workgroups (eight rounds of the 8 resident workgroups per CU: tiles with
// long rows scan far more than the others, and small workgroups even that out) of at least 1 536 patterns each (six 256-pattern passes
// per load of the tile).  Measured, 19 412 x 250 000: 1 chunk 29.7 ms, 2 17.9, 8 9.8, 16 8.5, 32 8.2, 64 8.3; x 25 000: 8 1.10, 16 1.09,
// 32 1.22, 64 1.66 (NOTEBOOK)
int resolve_chunks(const int64_t S, const int64_t P, const int32_t n_chunks) {
    if (P == 0) return 0;
    int64_t c = n_chunks;
    if (c == 0) {
        const int64_t tiles = (S + PT_TS - 1) / PT_TS;
        c = (16384 + tiles - 1) / (tiles > 0 ? tiles : 1);
        const int64_t most = (P + 1535) / 1536;
        c = c > most ? most : c;
    }
    c = c > PT_MAX_CHUNKS ? PT_MAX_CHUNKS : c;
    c = c > P ? P : c;
    return (int)(c < 1 ? 1 : c);
}

constexpr int64_t al16(const int64_t n) { return (n + 15) / 16 * 16; }

struct PairsWs {
    uint4* sig;
    int2* meta;
    unsigned long long* part_list;
    int32_t* part_cnt;
    int64_t bytes;
};

PairsWs carve(void* base, const int64_t S, const int64_t P, const int C) {
    PairsWs w;
    char* p = (char*)base;
    int64_t o = 0;
    w.sig = (uint4*)(p + o);                    o += al16(P * (int64_t)sizeof(uint4));
    w.meta = (int2*)(p + o);                    o += al16(P * (int64_t)sizeof(int2));
    w.part_list = (unsigned long long*)(p + o); o += al16(S * C * PT_K * (int64_t)sizeof(unsigned long long));
    w.part_cnt = (int32_t*)(p + o);             o += al16(S * C * (int64_t)sizeof(int32_t));
    w.bytes = o > 16 ? o : 16;
    return w;
}

int check_sizes(const int64_t S, const int64_t P, const int32_t n_chunks) {
    if (S < 0 || P < 0 || S >= (1LL << 31) || P >= (1LL << 31) || n_chunks < 0 || n_chunks > PT_MAX_CHUNKS) return DR4SR_E_ARG;
    return 0;
}

}  // namespace

extern "C" int64_t dr4sr_pairs_workspace_bytes(int64_t n_seq, int64_t n_pat, int32_t n_chunks) {
    if (const int rc = check_sizes(n_seq, n_pat, n_chunks)) return rc;
    return carve(nullptr, n_seq, n_pat, resolve_chunks(n_seq, n_pat, n_chunks)).bytes;
}

extern "C" int dr4sr_pairs_match(const int32_t* seqs, const int32_t* seq_len, int64_t n_seq, int32_t Lmax, const int32_t* pat_ids,
                                 const int64_t* pat_off, int64_t n_pat, int64_t n_ids, uint64_t seed, int64_t seq_index0,
                                 int64_t pat_index0, int32_t n_chunks, void* workspace, int64_t workspace_bytes, int32_t* n_match,
                                 int32_t* chosen, void* stream) {
    if (const int rc = check_sizes(n_seq, n_pat, n_chunks)) return rc;
    if (Lmax > PT_L) return DR4SR_E_SHAPE;
    if (!seqs || !seq_len || !n_match || !chosen || Lmax < 1 || n_ids < 0 || n_ids >= (1LL << 31)) return DR4SR_E_ARG;
    if (n_pat > 0 && (!pat_off || (n_ids > 0 && !pat_ids))) return DR4SR_E_ARG;
    if (seq_index0 < 0 || pat_index0 < 0 || seq_index0 + n_seq > (1LL << 31) || pat_index0 + n_pat > (1LL << 31)) return DR4SR_E_ARG;
    const int C = resolve_chunks(n_seq, n_pat, n_chunks);
    const PairsWs w = carve(workspace, n_seq, n_pat, C);
    if (!workspace || workspace_bytes < w.bytes) return DR4SR_E_WS;
    if (n_seq == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (n_pat > 0) {
        hipLaunchKernelGGL(k_pairs_sig, dim3((unsigned)((n_pat + 255) / 256)), dim3(256), 0, s, pat_ids, pat_off, n_ids, n_pat, w.sig, w.meta);
        if (const int rc = DR4SR_LAUNCH_CHECK()) return rc;
        const int64_t per = (n_pat + C - 1) / C;
        hipLaunchKernelGGL(k_pairs_match, dim3((unsigned)((n_seq + PT_TS - 1) / PT_TS), (unsigned)C), dim3(PT_NT), 0, s, seqs, seq_len, n_seq,
                           (int)Lmax, pat_ids, (const uint4*)w.sig, (const int2*)w.meta, n_pat, per, C, (uint32_t)seed, (uint32_t)(seed >> 32),
                           (uint32_t)seq_index0, (uint32_t)pat_index0, w.part_list, w.part_cnt);
        if (const int rc = DR4SR_LAUNCH_CHECK()) return rc;
    }
    hipLaunchKernelGGL(k_pairs_merge, dim3((unsigned)((n_seq + 255) / 256)), dim3(256), 0, s, (const unsigned long long*)w.part_list,
                       (const int32_t*)w.part_cnt, n_seq, C, n_match, chosen);
    return DR4SR_LAUNCH_CHECK();
}
