// gnn.hip — graph propagation of the item table for the GNN target model (the reference's model/gnn.py:43-50, get_gnn_embeddings):
//   out (+)= (in + A in + A^2 in + ... + A^n_hop in) / (n_hop + 1)        A: [N, N] CSR, fp32, each row sorted by column
// A is symmetric (dr4sr_amd/model/gnn.py build_graph asserts it), so the SAME call is the operator's adjoint: forward in = E, out = G;
// backward in = dG, out = dE with accumulate = 1.
//
// Form: one gather launch per hop, on the caller's stream, nothing but kernel launches (capturable).  A hop is a gather-SpMM,
// one wave64 per destination row: the row's (col, val) pairs are loaded 64 at a time, one per lane, and handed round with v_readlane, so an
// edge is ONE coalesced row read from a scalar base (D = 64: lane = column, 256 B; D = 128: float2 per lane, 512 B); four source rows are
// in flight per wave, in four independent accumulators: edge e of the row goes to accumulator e & 3, and they are combined as
// (a0 + a1) + (a2 + a3).  The same kernel adds the hop's result into the running sum (workspace table S; the first hop starts it from
// `in`), and the LAST hop writes out (+)= S / (n_hop + 1) instead: there is no mean pass.  The two ping-pong tables of A^k in live in the
// workspace too.
// Degree skew (a hub item has thousands of neighbours against a median of tens): a row longer than GNN_SPLIT edges is cut into chunks of
// GNN_CHUNK edges; each chunk is summed by a wave of its own (waves N .. N + n_chunks of the same launch) into a workspace partial, and
// the chunk wave that arrives LAST at the row's ticket (an integer counter) adds the row's partials IN CHUNK ORDER and finishes the row.
// Which wave arrives last changes nothing in the sum, so the result does not depend on timing.  The hand-off is the partial-slab
// reducer: plain stores -> vmcnt(0) -> agent-scope release fence -> vmcnt(0) -> relaxed agent-scope ticket; the last arriver: agent-scope
// acquire fence -> vmcnt(0) -> plain loads.  Nobody waits for anybody (no spin, no grid barrier, no cooperative launch).
// The chunk list is derived ON THE DEVICE from row_ptr by k_gnn_plan, once per call (one workgroup, a scan over the rows): the caller
// prepares nothing and the workspace carries nothing from call to call.  The capacity of the chunk list follows from workspace_bytes; a
// row whose chunks do not fit (a workspace sized for a smaller nnz than row_ptr describes) is summed whole by its row wave: slower, same
// contract.
// NO float atomics in this file and every sum in a fixed order: two calls on the same inputs give the same bits.
#include "common.h"

#define GNN_SPLIT 256            // rows with more edges than this are split (dr4sr_gnn_split_rows)
#define GNN_CHUNK 256            // edges per chunk
#define GNN_HEAD_BYTES 256       // workspace header: int32 n_chunks
#define GNN_MAX_HOP 64
#define GNN_MAX_CHUNKS (1 << 20)
#define RC(x) do { int _rc = (x); if (_rc) return _rc; } while (0)

struct GnnWs {
    int* head;                   // [0] = number of chunks of this call
    int* row_first;              // [N]: first chunk of a split row, -1 for a row summed by its own wave
    float *t0, *t1, *S;          // ping, pong, running sum: [N, D] each
    float* partial;              // [cap, D]
    int* chunk_row;              // [cap]
    int* ticket;                 // [cap], indexed by a split row's first chunk
    int64_t cap;
};

static int64_t gnn_align(int64_t b) { return (b + 255) / 256 * 256; }
static int64_t gnn_fixed_bytes(int32_t N, int32_t D) { return GNN_HEAD_BYTES + gnn_align((int64_t)N * 4) + 3 * gnn_align((int64_t)N * D * 4); }
static int64_t gnn_chunk_bytes(int32_t D) { return (int64_t)D * 4 + 8; }

extern "C" int32_t dr4sr_gnn_split_rows(void) { return GNN_SPLIT; }

extern "C" int64_t dr4sr_gnn_workspace_bytes(int32_t n_items, int32_t D, int64_t nnz) {
    if (n_items < 1 || nnz < 0) return DR4SR_E_ARG;
    if (D != 64 && D != 128) return DR4SR_E_SHAPE;
    // sum over rows with deg > SPLIT of ceil(deg / CHUNK) <= nnz / CHUNK + (number of such rows) <= nnz / CHUNK + nnz / SPLIT
    const int64_t cap = nnz / GNN_CHUNK + nnz / GNN_SPLIT + 1;
    return gnn_fixed_bytes(n_items, D) + cap * gnn_chunk_bytes(D);
}

static int gnn_carve(void* workspace, int64_t bytes, int32_t N, int32_t D, GnnWs* w) {
    const int64_t fixed = gnn_fixed_bytes(N, D);
    if (!workspace || bytes < fixed) return DR4SR_E_WS;
    char* p = (char*)workspace;
    w->head = (int*)p; p += GNN_HEAD_BYTES;
    w->row_first = (int*)p; p += gnn_align((int64_t)N * 4);
    const int64_t tb = gnn_align((int64_t)N * D * 4);
    w->t0 = (float*)p; p += tb;
    w->t1 = (float*)p; p += tb;
    w->S = (float*)p; p += tb;
    int64_t cap = (bytes - fixed) / gnn_chunk_bytes(D);
    if (cap > GNN_MAX_CHUNKS) cap = GNN_MAX_CHUNKS;
    w->cap = cap;
    w->partial = (float*)p; p += cap * D * 4;
    w->chunk_row = (int*)p; p += cap * 4;
    w->ticket = (int*)p;
    return 0;
}

// one workgroup: the chunk list of this call (rows in index order, a row's chunks consecutive), the tickets zeroed
__global__ __launch_bounds__(1024) void k_gnn_plan(const int64_t* __restrict__ row_ptr, const int N, const int cap, int* __restrict__ head,
                                                   int* __restrict__ row_first, int* __restrict__ chunk_row, int* __restrict__ ticket) {
    __shared__ int sc[1024];
    __shared__ int running, fitted;
    const int tid = (int)threadIdx.x;
    if (tid == 0) { running = 0; fitted = 0; }
    for (int c = tid; c < cap; c += 1024) ticket[c] = 0;
    __syncthreads();
    for (int base = 0; base < N; base += 1024) {
        const int r = base + tid;
        int nc = 0;
        if (r < N) {
            const int64_t deg = row_ptr[r + 1] - row_ptr[r];
            if (deg > GNN_SPLIT) nc = (int)((deg + GNN_CHUNK - 1) / GNN_CHUNK);
        }
        sc[tid] = nc;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {               // inclusive scan
            const int v = tid >= o ? sc[tid - o] : 0;
            __syncthreads();
            sc[tid] += v;
            __syncthreads();
        }
        const int first = running + sc[tid] - nc;
        if (r < N) {
            const bool fits = nc > 0 && first + nc <= cap;      // (a row that does not fit is summed whole by its row wave)
            row_first[r] = fits ? first : -1;
            if (fits) {
                for (int k = 0; k < nc; ++k) chunk_row[first + k] = r;
                atomicMax(&fitted, first + nc);                 // (`first` grows with the row: the rows that fit are a prefix of the list)
            }
        }
        __syncthreads();
        if (tid == 1023) running += sc[1023];
        __syncthreads();
    }
    if (tid == 0) head[0] = fitted;
}

template <int VPL> struct GnnVec;
template <> struct GnnVec<1> { typedef float T; };
template <> struct GnnVec<2> { typedef float2 T; };
__device__ __forceinline__ float gnn_zero(float) { return 0.f; }
__device__ __forceinline__ float2 gnn_zero(float2) { return make_float2(0.f, 0.f); }
__device__ __forceinline__ float gnn_fma(float v, float x, float a) { return fmaf(v, x, a); }
__device__ __forceinline__ float2 gnn_fma(float v, float2 x, float2 a) { return make_float2(fmaf(v, x.x, a.x), fmaf(v, x.y, a.y)); }
// (explicitly rounded: no contraction of the mean's scale into the accumulate's add, so accumulate = 1 adds exactly what accumulate = 0 writes)
__device__ __forceinline__ float gnn_add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float2 gnn_add(float2 a, float2 b) { return make_float2(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y)); }
__device__ __forceinline__ float gnn_scale(float a, float s) { return __fmul_rn(a, s); }
__device__ __forceinline__ float2 gnn_scale(float2 a, float s) { return make_float2(__fmul_rn(a.x, s), __fmul_rn(a.y, s)); }

// sum over edges [e0, e1) of val[e] * src[col[e]] for this lane's column(s); edge e0 + i goes to accumulator i & 3
template <typename V>
__device__ __forceinline__ V gnn_gather(const int32_t* __restrict__ col, const float* __restrict__ val, const V* __restrict__ src,
                                        const int64_t e0, const int64_t e1, const int N, const int lane) {
    V a0 = gnn_zero(V()), a1 = a0, a2 = a0, a3 = a0;
    for (int64_t base = e0; base < e1; base += 64) {
        const int nb = (int)(e1 - base < 64 ? e1 - base : 64);
        int my_c = 0;
        float my_v = 0.f;
        if (lane < nb) {
            my_c = col[base + lane];
            my_c = my_c < 0 ? 0 : (my_c >= N ? N - 1 : my_c);             // a launch cannot raise: ids are clamped (as csrc/embed.hip)
            my_v = val[base + lane];
        }
        int j = 0;
        for (; j + 4 <= nb; j += 4) {                                       // four source rows in flight
            const int c0 = __builtin_amdgcn_readlane(my_c, j), c1 = __builtin_amdgcn_readlane(my_c, j + 1);
            const int c2 = __builtin_amdgcn_readlane(my_c, j + 2), c3 = __builtin_amdgcn_readlane(my_c, j + 3);
            const V x0 = src[(size_t)c0 * 64 + lane], x1 = src[(size_t)c1 * 64 + lane];
            const V x2 = src[(size_t)c2 * 64 + lane], x3 = src[(size_t)c3 * 64 + lane];
            const float v0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_v), j));
            const float v1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_v), j + 1));
            const float v2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_v), j + 2));
            const float v3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_v), j + 3));
            a0 = gnn_fma(v0, x0, a0); a1 = gnn_fma(v1, x1, a1); a2 = gnn_fma(v2, x2, a2); a3 = gnn_fma(v3, x3, a3);
        }
        if (j < nb) {                                                       // the batch's last 1..3 edges (64-edge batches have none)
            const int c0 = __builtin_amdgcn_readlane(my_c, j);
            const float v0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_v), j));
            const V x0 = src[(size_t)c0 * 64 + lane];
            if (j + 1 < nb) {
                const int c1 = __builtin_amdgcn_readlane(my_c, j + 1);
                const float v1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_v), j + 1));
                const V x1 = src[(size_t)c1 * 64 + lane];
                if (j + 2 < nb) {
                    const int c2 = __builtin_amdgcn_readlane(my_c, j + 2);
                    const float v2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_v), j + 2));
                    a2 = gnn_fma(v2, src[(size_t)c2 * 64 + lane], a2);
                }
                a1 = gnn_fma(v1, x1, a1);
            }
            a0 = gnn_fma(v0, x0, a0);
        }
    }
    return gnn_add(gnn_add(a0, a1), gnn_add(a2, a3));
}

// the end of a row: g = (A src)[row].  Not the last hop: cur[row] = g, S[row] = (first hop ? in : S)[row] + g.
// The last hop: out[row] = (accumulate ? out[row] : 0) + ((first hop ? in : S)[row] + g) * scale.
template <typename V>
__device__ __forceinline__ void gnn_finish(const V g, const size_t at, const V* sum_in, V* __restrict__ cur, V* S,
                                           V* out, const int last, const int accumulate, const float scale) {
    const V s = gnn_add(sum_in[at], g);
    if (!last) {
        cur[at] = g;
        S[at] = s;
    } else {
        const V o = gnn_scale(s, scale);
        out[at] = accumulate ? gnn_add(out[at], o) : o;
    }
}

// waves 0 .. N - 1: one destination row each; waves N .. : one chunk of a split row each.  sum_in: `in` on the first hop, else S.
template <int VPL>
__global__ __launch_bounds__(256) void k_gnn_hop(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                 const float* __restrict__ val, const int N, const float* __restrict__ src_,
                                                 const float* sum_in_, float* __restrict__ cur_, float* S_,
                                                 float* __restrict__ out_, const int last, const int accumulate, const float scale,
                                                 const int* __restrict__ head, const int* __restrict__ row_first,
                                                 const int* __restrict__ chunk_row, int* __restrict__ ticket, float* __restrict__ partial_) {
    typedef typename GnnVec<VPL>::T V;
    const V* src = (const V*)src_;
    const V* sum_in = (const V*)sum_in_;
    V *cur = (V*)cur_, *S = (V*)S_, *out = (V*)out_, *partial = (V*)partial_;
    const int lane = (int)threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (w < N) {
        const int r = (int)w;
        if (row_first[r] >= 0) return;                                      // a split row: its chunk waves finish it
        const V g = gnn_gather<V>(col, val, src, row_ptr[r], row_ptr[r + 1], N, lane);
        gnn_finish<V>(g, (size_t)r * 64 + lane, sum_in, cur, S, out, last, accumulate, scale);
        return;
    }
    const int64_t c64 = w - N;
    if (c64 >= head[0]) return;
    const int c = (int)c64;
    const int r = chunk_row[c], first = row_first[r];
    const int64_t rs = row_ptr[r], re = row_ptr[r + 1];
    const int nc = (int)((re - rs + GNN_CHUNK - 1) / GNN_CHUNK);
    const int64_t e0 = rs + (int64_t)(c - first) * GNN_CHUNK;
    const int64_t e1 = e0 + GNN_CHUNK < re ? e0 + GNN_CHUNK : re;
    const V g = gnn_gather<V>(col, val, src, e0, e1, N, lane);
    partial[(size_t)c * 64 + lane] = g;
    // publish the partial, then draw the row's ticket (see the head of this file)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int t = 0;
    if (lane == 0) t = __hip_atomic_fetch_add(&ticket[first], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    t = __builtin_amdgcn_readfirstlane(t);
    if (t != nc - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    V s = partial[(size_t)first * 64 + lane];
    for (int k = 1; k < nc; ++k) s = gnn_add(s, partial[(size_t)(first + k) * 64 + lane]);      // chunk order
    gnn_finish<V>(s, (size_t)r * 64 + lane, sum_in, cur, S, out, last, accumulate, scale);
    if (lane == 0) ticket[first] = 0;                                       // for the next hop (the kernel boundary publishes it)
}

// n_hop = 0: out (+)= in, bit-exact
__global__ __launch_bounds__(256) void k_gnn_copy(const float4* __restrict__ in, float4* __restrict__ out, const int64_t n4, const int accumulate) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 v = in[i];
        if (accumulate) { const float4 o = out[i]; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
        out[i] = v;
    }
}

extern "C" int dr4sr_gnn_propagate(const int64_t* row_ptr, const int32_t* col, const float* val, int32_t n_items, int32_t D, int32_t n_hop,
                                   const float* in, float* out, int32_t accumulate, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!row_ptr || !col || !val || !in || !out || in == out || n_items < 1 || n_hop < 0 || n_hop > GNN_MAX_HOP ||
        (accumulate != 0 && accumulate != 1))
        return DR4SR_E_ARG;
    if (D != 64 && D != 128) return DR4SR_E_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    const int N = n_items;
    if (n_hop == 0) {
        const int64_t n4 = (int64_t)N * D / 4;
        int64_t gb = (n4 + 255) / 256;
        if (gb > 2048) gb = 2048;
        hipLaunchKernelGGL(k_gnn_copy, dim3((unsigned)gb), dim3(256), 0, s, (const float4*)in, (float4*)out, n4, accumulate);
        return DR4SR_LAUNCH_CHECK();
    }
    GnnWs w;
    RC(gnn_carve(workspace, workspace_bytes, N, D, &w));
    hipLaunchKernelGGL(k_gnn_plan, dim3(1), dim3(1024), 0, s, row_ptr, N, (int)w.cap, w.head, w.row_first, w.chunk_row, w.ticket);
    const int64_t waves = (int64_t)N + w.cap;
    const dim3 grid((unsigned)((waves + 3) / 4));
    const float scale = (float)(1.0 / (double)(n_hop + 1));
    for (int h = 1; h <= n_hop; ++h) {
        const float* src = h == 1 ? in : ((h & 1) ? w.t1 : w.t0);           // hop h reads A^(h-1) in and writes A^h in: t0, t1, t0, ...
        float* cur = (h & 1) ? w.t0 : w.t1;
        const float* sum_in = h == 1 ? in : w.S;
        const int last = h == n_hop;
        if (D == 64)
            hipLaunchKernelGGL(k_gnn_hop<1>, grid, dim3(256), 0, s, row_ptr, col, val, N, src, sum_in, cur, w.S, out, last, accumulate, scale,
                               w.head, w.row_first, w.chunk_row, w.ticket, w.partial);
        else
            hipLaunchKernelGGL(k_gnn_hop<2>, grid, dim3(256), 0, s, row_ptr, col, val, N, src, sum_in, cur, w.S, out, last, accumulate, scale,
                               w.head, w.row_first, w.chunk_row, w.ticket, w.partial);
    }
    return DR4SR_LAUNCH_CHECK();
}
