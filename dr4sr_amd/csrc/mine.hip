// mine.hip — the regenerator's pattern mining (DR4SR stage 1, the reference's 1.Build_pretraining_dataset.py:24-27:
// Seq2Pat(sequences, max_span = alpha).get_patterns(min_frequency = beta)), by the rule of DESIGN §4h:
//
//   a pattern is a tuple of k ids, 2 <= k <= alpha; it occurs in a sequence s if there are positions p_0 < ... < p_{k-1} with
//   s[p_i] = t_i and p_{k-1} - p_0 <= mine_reach(alpha) (all of its items inside a window of alpha consecutive positions); its frequency
//   is the number of sequences with at least one occurrence; the result is every pattern with frequency >= beta.
//
// A candidate is a pair (global position g of the packed id array, non-empty mask m over the offsets 1..reach, bit j = offset j + 1)
// whose highest offset still lies inside g's sequence: the tuple ids[g], ids[g + o] for every offset o of m.  Several candidates of one
// sequence can give the same tuple; exactly one of them CONTRIBUTES, the one for which
//   (a) m is the greedy left-most embedding of its tuple starting exactly at g (the numerically smallest mask that yields it), and
//   (b) from no earlier start p' < g of the sequence with ids[p'] = t_0 does the greedy embedding of the tuple fit inside the window
// so a sequence is counted once per tuple with no sort, no per-sequence set and no ordering between waves.
//
//   k_mine_clear    owner words to EMPTY, counts, the output counter and the status words to 0.
//   k_mine_count    one thread per candidate.  A contributing one inserts its tuple into an open-addressing table: a slot is a 64-bit
//                   owner word — the candidate (g << reach | m) that claimed it with ONE compare-and-swap from EMPTY — and a 32-bit
//                   count.  The key is never stored: a thread that finds a slot taken re-derives the owner's tuple from the immutable
//                   input arrays and compares; equal: integer atomicAdd on the count, different: linear probe.  Nobody ever waits for
//                   another thread's store, and integer counts do not depend on arrival order.  Probing is bounded by the table size; a
//                   full table sets status[0] and the thread returns (threads that start after that return at once).
//   k_mine_extract  one thread per slot: a taken slot with count >= beta is appended to out_ids / out_freq through one integer counter
//                   (rows past cap are counted, not written); status[1] / status[2]: taken slots and the sum of their displacements from
//                   their home slot (load factor and mean probe length of the finished table).
// The ORDER of the appended rows depends on the schedule; their SET does not.  The caller orders them (dr4sr_amd/mine.py).
#include "common.h"

namespace {

// THE span rule of this backend: the last item of an occurrence lies at most this many positions after its first.  seq2pat documents
// its built-in index-span constraint as span <= max_span - 1; if a run of the real library ever shows the bound to be off by one, this
// constant changes and nothing else (dr4sr_amd/mine.py `reach` is the same place of the numpy backend).
constexpr int mine_reach(const int alpha) { return alpha - 1; }

constexpr int MN_NT = 256;
constexpr int MN_ALPHA_MIN = 2, MN_ALPHA_MAX = 10;
constexpr unsigned long long MN_EMPTY = ~0ull;
constexpr int64_t MN_MAX_SLOTS = 1LL << 30;      // counts of slots fit the int32 output counter
constexpr int64_t MN_MAX_THREADS = 1LL << 38;    // n_ids << reach: one thread per (position, mask), 2^30 workgroups at most

template <int W>
struct Tup {
    int32_t v[W];      // the tuple's ids, zero padded (ids are >= 1)
};

// the tuple of candidate (g, m); reads ids[g] and ids[g + o] for the offsets o of m only
template <int R>
__device__ __forceinline__ Tup<R + 1> tuple_of(const int32_t* __restrict__ ids, const int64_t g, const uint32_t m) {
    Tup<R + 1> t;
#pragma unroll
    for (int i = 0; i <= R; ++i) t.v[i] = 0;
    t.v[0] = ids[g];
    int k = 1;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const bool on = (m >> j) & 1u;
        const int32_t x = on ? ids[g + j + 1] : 0;
#pragma unroll
        for (int i = 1; i <= j + 1; ++i)
            if (on && i == k) t.v[i] = x;
        k += on ? 1 : 0;
    }
    return t;
}

template <int W>
__device__ __forceinline__ int32_t pick(const Tup<W>& t, const int i) {
    int32_t x = 0;
#pragma unroll
    for (int e = 0; e < W; ++e) x = e == i ? t.v[e] : x;
    return x;
}

template <int W>
__device__ __forceinline__ bool same(const Tup<W>& a, const Tup<W>& b) {
    bool eq = true;
#pragma unroll
    for (int e = 0; e < W; ++e) eq = eq && a.v[e] == b.v[e];
    return eq;
}

template <int W>
__device__ __forceinline__ uint32_t hash_of(const Tup<W>& t) {
    uint32_t h = 0x811C9DC5u;
#pragma unroll
    for (int e = 0; e < W; ++e) {
        h = (h ^ (uint32_t)t.v[e]) * 0x01000193u;
        h ^= h >> 15;
    }
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// the greedy left-most embedding of the k-id tuple t with t_0 at position p, inside the window p .. p + R and before `end`: the mask of the
// offsets it takes; fits = all k ids found
template <int R>
__device__ __forceinline__ uint32_t greedy_mask(const int32_t* __restrict__ ids, const int64_t p, const int64_t end, const Tup<R + 1>& t,
                                                const int k, bool& fits) {
    int i = 1;
    uint32_t gm = 0;
#pragma unroll
    for (int q = 1; q <= R; ++q) {
        const bool in = p + q < end;
        const int32_t x = in ? ids[p + q] : 0;
        const bool hit = in && i < k && x == pick(t, i);
        gm |= hit ? 1u << (q - 1) : 0u;
        i += hit ? 1 : 0;
    }
    fits = i == k;
    return gm;
}

__global__ void k_mine_clear(unsigned long long* __restrict__ owner, int32_t* __restrict__ count, const int64_t n_slots,
                             int32_t* __restrict__ n_out, unsigned long long* __restrict__ status) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n_slots) {
        owner[s] = MN_EMPTY;
        count[s] = 0;
    }
    if (s == 0) n_out[0] = 0;
    if (s < 4) status[s] = 0ull;
}

template <int A>
__global__ __launch_bounds__(MN_NT) void k_mine_count(const int32_t* __restrict__ ids, const int64_t* __restrict__ seq_off,
                                                      const int64_t n_ids, const int64_t n_seq, unsigned long long* __restrict__ owner,
                                                      int32_t* __restrict__ count, const int64_t slot_mask,
                                                      unsigned long long* __restrict__ status) {
    constexpr int R = mine_reach(A);
    static_assert(R >= 1 && R + 1 <= A && R <= 16, "an output row holds alpha ids");
    const int64_t c = (int64_t)blockIdx.x * MN_NT + threadIdx.x;
    const int64_t g = c >> R;
    const uint32_t m = (uint32_t)c & ((1u << R) - 1u);
    if (g >= n_ids || m == 0u) return;
    // g's sequence: the last s with seq_off[s] <= g.  Offsets are not trusted: whatever the search ends on is checked below
    int64_t lo = 0, hi = n_seq;
    for (int it = 0; it < 32 && hi - lo > 1; ++it) {
        const int64_t mid = (lo + hi) >> 1;
        if (seq_off[mid] <= g) lo = mid;
        else hi = mid;
    }
    const int64_t begin = seq_off[lo], end = seq_off[lo + 1];
    if (begin < 0 || begin > g || end <= g || end > n_ids) return;
    const int top = 32 - __clz((int)m);                                       // the mask's highest offset
    if (g + top >= end) return;                                                // not a candidate: it leaves the sequence
    const int k = 1 + __popc(m);
    const Tup<R + 1> t = tuple_of<R>(ids, g, m);
    bool fits;
    if (greedy_mask<R>(ids, g, end, t, k, fits) != m) return;                  // (a)
    for (int64_t p = begin; p < g; ++p) {                                      // (b)
        if (ids[p] != t.v[0]) continue;
        greedy_mask<R>(ids, p, end, t, k, fits);
        if (fits) return;
    }
    if (__hip_atomic_load(&status[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull) return;      // the table has overflowed already
    const unsigned long long me = (unsigned long long)c;
    const uint32_t h = hash_of(t);
    for (int64_t probe = 0; probe <= slot_mask; ++probe) {
        const int64_t s = ((int64_t)h + probe) & slot_mask;
        unsigned long long o = __hip_atomic_load(&owner[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (o == MN_EMPTY) {
            o = atomicCAS(&owner[s], MN_EMPTY, me);
            if (o == MN_EMPTY) o = me;
        }
        // an owner word was written by a thread that passed every check above, so its tuple is read inside [0, n_ids)
        if (o == me || same(tuple_of<R>(ids, (int64_t)(o >> R), (uint32_t)o & ((1u << R) - 1u)), t)) {
            atomicAdd(&count[s], 1);
            return;
        }
    }
    atomicOr(&status[0], 1ull);
}

template <int A>
__global__ __launch_bounds__(MN_NT) void k_mine_extract(const int32_t* __restrict__ ids, const unsigned long long* __restrict__ owner,
                                                        const int32_t* __restrict__ count, const int64_t n_slots, const int32_t beta,
                                                        int32_t* __restrict__ out_ids, int32_t* __restrict__ out_freq, const int64_t cap,
                                                        int32_t* __restrict__ n_out, unsigned long long* __restrict__ status) {
    constexpr int R = mine_reach(A);
    __shared__ unsigned int s_taken;
    __shared__ unsigned long long s_disp;
    if (threadIdx.x == 0) {
        s_taken = 0u;
        s_disp = 0ull;
    }
    __syncthreads();
    const int64_t s = (int64_t)blockIdx.x * MN_NT + threadIdx.x;
    const unsigned long long o = s < n_slots ? owner[s] : MN_EMPTY;
    if (o != MN_EMPTY) {
        const Tup<R + 1> t = tuple_of<R>(ids, (int64_t)(o >> R), (uint32_t)o & ((1u << R) - 1u));
        atomicAdd(&s_taken, 1u);
        atomicAdd(&s_disp, (unsigned long long)((s - (int64_t)hash_of(t)) & (n_slots - 1)));
        const int32_t f = count[s];
        if (f >= beta) {
            const int64_t row = atomicAdd(n_out, 1);
            if (row < cap) {
#pragma unroll
                for (int i = 0; i < A; ++i) out_ids[row * A + i] = i <= R ? t.v[i <= R ? i : R] : 0;
                out_freq[row] = f;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_taken) {
        atomicAdd(&status[1], (unsigned long long)s_taken);
        atomicAdd(&status[2], s_disp);
    }
}

constexpr int64_t al16(const int64_t n) { return (n + 15) / 16 * 16; }

bool alpha_ok(const int32_t alpha) { return alpha >= MN_ALPHA_MIN && alpha <= MN_ALPHA_MAX; }

// slots of the table: the caller's power of two, or (0) the first power of two at or above twice n_ids * (2^reach - 1), the number of
// (position, mask) pairs — at least the number of candidates of any split into sequences, so that table cannot fill up.  < 0: DR4SR_E_ARG
int64_t resolve_slots(const int64_t n_ids, const int32_t alpha, const int64_t table_slots) {
    if (table_slots < 0 || table_slots > MN_MAX_SLOTS || (table_slots & (table_slots - 1)) != 0) return DR4SR_E_ARG;
    if (table_slots > 0) return table_slots;
    const int64_t bound = n_ids * ((1LL << mine_reach(alpha)) - 1);
    if (bound > MN_MAX_SLOTS) return DR4SR_E_ARG;
    int64_t s = 256;
    while (s < 2 * bound && s < MN_MAX_SLOTS) s <<= 1;
    return s;
}

int check_sizes(const int64_t n_ids, const int64_t n_seq, const int32_t alpha) {
    if (n_ids < 0 || n_seq < 0 || n_ids >= (1LL << 31) || n_seq >= (1LL << 31)) return DR4SR_E_ARG;
    if (!alpha_ok(alpha)) return DR4SR_E_SHAPE;
    if ((n_ids << mine_reach(alpha)) > MN_MAX_THREADS) return DR4SR_E_ARG;
    return 0;
}

template <int A>
int launch(const int32_t* ids, const int64_t* seq_off, const int64_t n_ids, const int64_t n_seq, const int32_t beta, const int64_t slots,
           unsigned long long* owner, int32_t* count, int32_t* out_ids, int32_t* out_freq, const int64_t cap, int32_t* n_out,
           unsigned long long* status, hipStream_t s) {
    const unsigned slot_blocks = (unsigned)((slots + MN_NT - 1) / MN_NT);
    hipLaunchKernelGGL(k_mine_clear, dim3(slot_blocks), dim3(MN_NT), 0, s, owner, count, slots, n_out, status);
    if (const int rc = DR4SR_LAUNCH_CHECK()) return rc;
    if (n_ids > 0 && n_seq > 0) {
        const int64_t threads = n_ids << mine_reach(A);
        hipLaunchKernelGGL(k_mine_count<A>, dim3((unsigned)((threads + MN_NT - 1) / MN_NT)), dim3(MN_NT), 0, s, ids, seq_off, n_ids, n_seq,
                           owner, count, slots - 1, status);
        if (const int rc = DR4SR_LAUNCH_CHECK()) return rc;
    }
    hipLaunchKernelGGL(k_mine_extract<A>, dim3(slot_blocks), dim3(MN_NT), 0, s, ids, (const unsigned long long*)owner, (const int32_t*)count,
                       slots, beta, out_ids, out_freq, cap, n_out, status);
    return DR4SR_LAUNCH_CHECK();
}

}  // namespace

extern "C" int64_t dr4sr_mine_workspace_bytes(int64_t n_ids, int64_t n_seq, int32_t alpha, int64_t table_slots) {
    if (const int rc = check_sizes(n_ids, n_seq, alpha)) return rc;
    const int64_t slots = resolve_slots(n_ids, alpha, table_slots);
    if (slots < 0) return slots;
    return al16(slots * (int64_t)sizeof(unsigned long long)) + al16(slots * (int64_t)sizeof(int32_t));
}

extern "C" int dr4sr_mine_patterns(const int32_t* ids, const int64_t* seq_off, int64_t n_ids, int64_t n_seq, int32_t alpha, int32_t beta,
                                   int64_t table_slots, void* workspace, int64_t workspace_bytes, int32_t* out_ids, int32_t* out_freq,
                                   int64_t cap, int32_t* n_out, int64_t* status, void* stream) {
    if (const int rc = check_sizes(n_ids, n_seq, alpha)) return rc;
    if (!n_out || !status || beta < 1 || cap < 0 || (cap > 0 && (!out_ids || !out_freq))) return DR4SR_E_ARG;
    if ((n_ids > 0 && !ids) || (n_seq > 0 && !seq_off)) return DR4SR_E_ARG;
    const int64_t slots = resolve_slots(n_ids, alpha, table_slots);
    if (slots < 0) return (int)slots;
    const int64_t owner_bytes = al16(slots * (int64_t)sizeof(unsigned long long));
    if (!workspace || workspace_bytes < owner_bytes + al16(slots * (int64_t)sizeof(int32_t))) return DR4SR_E_WS;
    unsigned long long* owner = (unsigned long long*)workspace;
    int32_t* count = (int32_t*)((char*)workspace + owner_bytes);
    hipStream_t s = (hipStream_t)stream;
#define DR4SR_MINE_CASE(A) \
    case A: return launch<A>(ids, seq_off, n_ids, n_seq, beta, slots, owner, count, out_ids, out_freq, cap, n_out, (unsigned long long*)status, s)
    switch (alpha) {
        DR4SR_MINE_CASE(2);
        DR4SR_MINE_CASE(3);
        DR4SR_MINE_CASE(4);
        DR4SR_MINE_CASE(5);
        DR4SR_MINE_CASE(6);
        DR4SR_MINE_CASE(7);
        DR4SR_MINE_CASE(8);
        DR4SR_MINE_CASE(9);
        DR4SR_MINE_CASE(10);
    }
#undef DR4SR_MINE_CASE
    return DR4SR_E_SHAPE;
}
