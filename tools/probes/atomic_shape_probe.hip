// atomic_shape_probe.hip — what does the SHAPE of one fp32 atomic-add wave-instruction cost at the latency step's grid?
// The same 64 dwords per instruction, laid out as
//   1  one contiguous 256-byte row
//   2  4 rows x one dense 64-byte segment                          (a 16x16 accumulator stored key-major)
//   3  16 rows x one 64-byte segment, 4 live dwords at 16-B stride  (attn_tile.h bwd(): dK | dV as it stands)
//   4  4 rows x 4 segments, 4 live dwords in each                  (TableAdds::issue / the dE adds: one component of a float4 per instruction)
//   5  64 rows, one dword each                                      (the known-slow anchor)
// "2c" / "3c" are 2 and 3 with the rows of one instruction adjacent (16 consecutive tokens of a tile) instead of pseudo-random.
// Targets: the item table (11 925 x 64 floats) and a dqkv-shaped buffer ([2 240][192] floats, the K | V columns).
// Reported: microseconds per launch minus an empty launch of the same grid (HIP events over LAUNCHES launches), and the sum check.
// build: hipcc --offload-arch=gfx950 -O3 -munsafe-fp-atomics -o atomic_shape_probe atomic_shape_probe.hip ; run on the GPU box.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)

__device__ __forceinline__ unsigned mix(unsigned x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }

enum { S_ROW = 1, S_DENSE4, S_STRIDE16, S_FLOAT4, S_SCATTER, S_DENSE4_ADJ, S_STRIDE16_ADJ };

// width: floats per row; coff: first of the 64 columns written (0 in the table, 64 = the K block in dqkv); n_rows % 16 == 0 is not required
template <int SHAPE>
__global__ __launch_bounds__(256) void k_add(float* __restrict__ buf, unsigned n_rows, unsigned width, unsigned coff, int n, unsigned salt) {
    const unsigned gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63, l16 = lane & 15, g = lane >> 4;
    for (int k = 0; k < n; ++k) {
        const unsigned h = (gw * 977u + (unsigned)k) * 64u + salt;          // one hash stream per (wave, instruction); + small index per row
        const unsigned fb = mix(h + 63u) & 3u, e = (unsigned)k & 3u;
        const unsigned base16 = (mix(h) % (n_rows / 16u)) * 16u;            // an aligned run of 16 rows, all < n_rows
        unsigned row, col;
        if (SHAPE == S_ROW)               { row = mix(h) % n_rows;        col = lane; }
        else if (SHAPE == S_DENSE4)       { row = mix(h + g) % n_rows;    col = fb * 16u + l16; }
        else if (SHAPE == S_STRIDE16)     { row = mix(h + l16) % n_rows;  col = fb * 16u + 4u * g + e; }
        else if (SHAPE == S_FLOAT4)       { row = mix(h + g) % n_rows;    col = 4u * l16 + e; }
        else if (SHAPE == S_SCATTER)      { row = mix(h + lane) % n_rows; col = (unsigned)k & 63u; }
        else if (SHAPE == S_DENSE4_ADJ)   { row = base16 + 4u * g + e;    col = fb * 16u + l16; }
        else                              { row = base16 + l16;           col = fb * 16u + 4u * g + e; }
        unsafeAtomicAdd(&buf[(size_t)row * width + coff + col], 1.0f);      // row < n_rows, coff + col < width by construction
    }
}

struct Target { const char* name; unsigned n_rows, width, coff; };

int main() {
    const int LAUNCHES = 300, threads = 256;
    const Target targets[2] = {{"table 11925x64", 11925u, 64u, 0u}, {"dqkv [2240][192]", 2240u, 192u, 64u}};
    const int grids[2] = {140, 256}, counts[2] = {32, 128};
    const size_t max_floats = (size_t)11925 * 64;                           // > 2240 * 192
    float* d; CK(hipMalloc(&d, max_floats * sizeof(float)));
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    std::vector<float> host(max_floats);

    using Kern = void (*)(float*, unsigned, unsigned, unsigned, int, unsigned);
    struct Shape { const char* name; Kern k; bool dqkv_only; };
    const Shape shapes[7] = {
        {"1  1 row x 256 B", k_add<S_ROW>, false},
        {"2  4 rows x 64 B dense", k_add<S_DENSE4>, false},
        {"3  16 rows x 64 B seg, 4 live", k_add<S_STRIDE16>, false},
        {"4  4 rows x 4 segs, 4 live each", k_add<S_FLOAT4>, false},
        {"5  64 rows x 1 dword", k_add<S_SCATTER>, false},
        {"2c 4 adjacent rows x 64 B dense", k_add<S_DENSE4_ADJ>, true},
        {"3c 16 adjacent rows, 4 live", k_add<S_STRIDE16_ADJ>, true},
    };

    auto time_us = [&](Kern k, const Target& t, int grid, int n) {
        for (int i = 0; i < 20; ++i) k<<<grid, threads>>>(d, t.n_rows, t.width, t.coff, n, (unsigned)i);
        CK(hipDeviceSynchronize());
        CK(hipEventRecord(a));
        for (int i = 0; i < LAUNCHES; ++i) k<<<grid, threads>>>(d, t.n_rows, t.width, t.coff, n, (unsigned)i * 4096u);
        CK(hipEventRecord(b)); CK(hipEventSynchronize(b)); CK(hipGetLastError());
        float ms; CK(hipEventElapsedTime(&ms, a, b));
        return (double)ms * 1e3 / LAUNCHES;
    };
    auto check = [&](Kern k, const Target& t, int grid, int n) {            // one launch into a zeroed buffer: every add must arrive
        const size_t fl = (size_t)t.n_rows * t.width;
        CK(hipMemset(d, 0, fl * sizeof(float)));
        k<<<grid, threads>>>(d, t.n_rows, t.width, t.coff, n, 7u);
        CK(hipMemcpy(host.data(), d, fl * sizeof(float), hipMemcpyDeviceToHost));
        double sum = 0; for (size_t i = 0; i < fl; ++i) sum += host[i];
        return sum == (double)grid * threads * n;
    };

    printf("fp32 no-return atomic adds, 64 dwords per wave-instruction, %d threads per workgroup, %d launches per figure\n", threads, LAUNCHES);
    printf("us per launch MINUS the empty launch of the same grid (n = 0); 'wave-instr' = n per wave\n\n");
    for (const Target& t : targets)
        for (int grid : grids) {
            const double empty = time_us(k_add<S_ROW>, t, grid, 0);
            printf("== %s, %d workgroups (empty launch %.2f us)\n", t.name, grid, empty);
            printf("%-36s %12s %12s   %s\n", "shape", "n=32 us", "n=128 us", "sums");
            for (const Shape& s : shapes) {
                if (s.dqkv_only && t.width != 192u) continue;
                double us[2]; bool ok = true;
                for (int c = 0; c < 2; ++c) { us[c] = time_us(s.k, t, grid, counts[c]) - empty; ok = ok && check(s.k, t, grid, counts[c]); }
                printf("%-36s %12.2f %12.2f   %s\n", s.name, us[0], us[1], ok ? "exact" : "LOST UPDATES");
            }
            printf("\n");
        }
    CK(hipFree(d));
    return 0;
}
