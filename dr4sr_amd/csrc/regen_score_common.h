// regen_score_common.h — the ground under teacher-forced scoring (regen_score.hip) and its gradients (regen_score_bwd.hip): the
// parameter layout, the masked softmax, the live-token scan, the tile table with its causal self-attention, and the argument checks.
// The forward that both files run is regen_score_fwd.h.
#pragma once
#include "common.h"
#include "kernels.h"

extern __shared__ __attribute__((aligned(16))) float smem[];

namespace {

constexpr int RD = 64, RH = 2, RDH = 32, RF = 256, RNL = 2;
constexpr int LMAX = 50;       // position table rows: longest source row and widest target matrix
constexpr int KMAX = 5;
constexpr int TM = 64;         // token slots per tile
constexpr int NT = 256;
constexpr int XLD = RD + 4, QLD = 3 * RD + 4, FLD = RF + 4, PLD = 52;

enum { T_E = 0, T_P = 1, T_ENC = 2, T_ENC_NORM = 26, T_DEC = 28, T_DEC_NORM = 64, T_CL0W = 66, T_CL0B = 67, T_CL2W = 68, T_CL2B = 69,
       T_CENC = 70, T_CC0W = 94, T_CC0B = 95, T_CC2W = 96, T_CC2B = 97 };
enum { E_INW, E_INB, E_OUTW, E_OUTB, E_W1, E_B1, E_W2, E_B2, E_N1W, E_N1B, E_N2W, E_N2B };
enum { D_SAINW, D_SAINB, D_SAOUTW, D_SAOUTB, D_CAINW, D_CAINB, D_CAOUTW, D_CAOUTB, D_W1, D_B1, D_W2, D_B2,
       D_N1W, D_N1B, D_N2W, D_N2B, D_N3W, D_N3B };

struct ScoreOff { int64_t o[DR4SR_REGEN_SCORE_TENSORS]; };

// ------------------------------------------------------------------------------------------------------------------- dropout
// The DROP policy every piece of the forward and of the backward is templated on:
//   DropNone    eval mode: no site exists, nothing is generated (the kernels take no dropout argument at all).
//   DropPhilox  train mode: the keep factor (0 or 1 / (1 - p)) of nn.Transformer's 30 sites, regenerated wherever it is consumed from
//               (seed, step, site, element index) with common.h's 16-bit decisions (8 per Philox call).
// Sites: rs_site(stack, layer, kind) and the two embedding sites (DR4SR_REGEN_SITE_* in include/dr4sr_hip.h; DESIGN.md has the table).
// Element index (64-bit; fixed strides that depend on neither Ls, T, the tile nor the chunk), pair = pair0 + the call's pair:
//   hidden sites  (pair 64 + position) 64 + column        FFN hidden  (pair 64 + position) 256 + column
//   probabilities ((pair 2 + head) 64 + query position) 64 + key position
// Host mirror, bit for bit: dr4sr_amd/regen_dropout.py.
struct DropNone { static constexpr bool on = false; static constexpr int64_t pair0 = 0; };
struct DropPhilox { static constexpr bool on = true; RngKey k; int64_t pair0; };
__device__ __forceinline__ DropNone pick_drop() { return DropNone(); }
__device__ __forceinline__ DropPhilox pick_drop(const DropPhilox& d) { return d; }

enum { ST_SRC = 0, ST_COND = 1, ST_DEC = 2 };
constexpr uint32_t rs_site(int stack, int layer, int kind) { return DR4SR_REGEN_SITE_BASE + stack * 32 + layer * 8 + kind; }

DropPhilox host_drop(float p, uint64_t seed, uint32_t step, int64_t pair0) {      // make_rng of common.h on the host
    DropPhilox d;
    d.k.seed_lo = (uint32_t)seed; d.k.seed_hi = (uint32_t)(seed >> 32); d.k.step = step; d.k.p = p;
    d.k.scale = 1.0f / (1.0f - p);
    const float t = p * 65536.0f + 0.5f;
    d.k.thresh = t >= 65535.0f ? 65535u : (uint32_t)t;
    d.pair0 = pair0;
    return d;
}

// the keep decisions of key positions 0 .. n - 1 (n <= 56) of the probability row (pair, head h, query position i): bit j = key j is kept
__device__ __forceinline__ uint64_t prob_keep_bits(const DropPhilox& dp, uint32_t site, int64_t pair, int h, int i, int n) {
    const uint64_t e0 = (uint64_t)(((pair * 2 + h) * 64 + i) * 64);
    uint64_t m = 0;
    for (int j = 0; j < n; j += 8) m |= (uint64_t)drop_bits8(dp.k, site, e0 + j) << j;
    return m;
}

int64_t score_layout(int32_t n_rows, int32_t K, int64_t* off) {
    int64_t pos = dr4sr_regen_param_layout(n_rows, K, off);
    int i = DR4SR_REGEN_TENSORS;
    const int64_t enc[12] = {3 * RD * RD, 3 * RD, RD * RD, RD, RF * RD, RF, RD * RF, RD, RD, RD, RD, RD};
    for (int l = 0; l < RNL; ++l)
        for (int j = 0; j < 12; ++j) { if (off) off[i] = pos; ++i; pos += enc[j]; }
    const int64_t tail[4] = {RD * RD, RD, (int64_t)K * RD, (int64_t)K};
    for (int j = 0; j < 4; ++j) { if (off) off[i] = pos; ++i; pos += tail[j]; }
    return pos;
}

// softmax over j < n of S[j] in place; masked entries are -inf; a row with no live entry becomes all zero
__device__ __forceinline__ void softmax_masked(float* S, int n) {
    float m = -INFINITY;
    for (int j = 0; j < n; ++j) m = fmaxf(m, S[j]);
    if (m == -INFINITY) { for (int j = 0; j < n; ++j) S[j] = 0.f; return; }
    float s = 0.f;
    for (int j = 0; j < n; ++j) { const float e = __expf(S[j] - m); S[j] = e; s += e; }
    const float inv = 1.0f / s;
    for (int j = 0; j < n; ++j) S[j] *= inv;
}

__device__ __forceinline__ int clampi(int64_t v, int lo, int hi) { return (int)min<int64_t>(max<int64_t>(v, lo), hi); }

// ------------------------------------------------------------------------------------------------------------------- scan
// cum[p] = sum over p' < p of live(p'), cum[n_pair] = total.  live = the decoder's positions with a non-PAD target (mode 1:
// min(tgt_len - 1, T)) or the condition encoder's positions (mode 0: min(tgt_len, T)); tgt_len counts SOS and EOS.
__global__ __launch_bounds__(1024) void k_rs_scan(const int64_t* __restrict__ tgt_len, int n_pair, int T, int mode, int* __restrict__ cum) {
    __shared__ int part[1024];
    const int per = (n_pair + 1023) / 1024, a = threadIdx.x * per, b = min(n_pair, a + per);
    int s = 0;
    for (int p = a; p < b; ++p) s += clampi(tgt_len[p] - mode, 1, T);
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int i = 0; i < 1024; ++i) { const int v = part[i]; part[i] = run; run += v; }
        cum[n_pair] = run;
    }
    __syncthreads();
    s = part[threadIdx.x];
    for (int p = a; p < b; ++p) { cum[p] = s; s += clampi(tgt_len[p] - mode, 1, T); }
}

// ------------------------------------------------------------------------------------------------------------------- target side
struct TileTab {
    int tok_row[TM], tok_pos[TM], tok_id[TM], tok_out[TM];     // per slot: row of the table (-1: empty), position, tgt_in id, tgt_out id
    int row_pair[TM], row_w[TM], row_base[TM], row_n[TM], row_ls[TM];
    float row_wt[TM][KMAX + 3];
    int n_row;
};

// causal self-attention of every live slot over its own row's earlier slots (keys with id 0 masked); QKV [64][QLD] -> O [64][XLD]
// (train mode: P . V takes the dropped probabilities of `site`)
template <class Drop>
__device__ __forceinline__ void self_attention(const Drop& dp, uint32_t site, const TileTab& tb, const float* QKV, float* PS, float* O, float scale) {
    if (threadIdx.x < TM * RH) {
        const int s = threadIdx.x >> 1, h = threadIdx.x & 1, r = tb.tok_row[s];
        float acc[RDH];
#pragma unroll
        for (int d = 0; d < RDH; ++d) acc[d] = 0.f;
        if (r >= 0) {
            const int base = tb.row_base[r], nk = tb.tok_pos[s] + 1;
            float* pr = PS + (s * RH + h) * PLD;
            const float* q = QKV + s * QLD + h * RDH;
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
            for (int j = 0; j < nk; ++j) {
                float pj = pr[j];
                if constexpr (Drop::on) pj = ((km >> j) & 1) ? pj * dp.k.scale : 0.f;
                const float* v = QKV + (base + j) * QLD + 2 * RD + h * RDH;
#pragma unroll
                for (int d = 0; d < RDH; ++d) acc[d] = fmaf(pj, v[d], acc[d]);
            }
        }
#pragma unroll
        for (int d = 0; d < RDH; ++d) O[s * XLD + h * RDH + d] = acc[d];
    }
}

int64_t cum_bytes(int64_t n_pair) { return ((n_pair + 1) * 4 + 255) / 256 * 256; }
int64_t ws_bytes(int64_t n_pair, int K, int Ls) { return cum_bytes(n_pair) + n_pair * K * RNL * Ls * 2 * RD * 4; }

int check_plan(const dr4sr_regen_plan* p) {
    if (!p || p->abi_version != DR4SR_ABI_VERSION || !p->params) return DR4SR_E_ARG;
    if (p->D != RD || p->H != RH || p->F != RF || p->n_layer != RNL) return DR4SR_E_SHAPE;
    if (p->K < 1 || p->K > KMAX || p->n_rows < 3) return p->K > KMAX ? DR4SR_E_SHAPE : DR4SR_E_ARG;
    if (p->n_params != score_layout(p->n_rows, p->K, nullptr)) return DR4SR_E_ARG;       // a 70-tensor decode buffer is refused here
    return 0;
}

int check_sizes(const dr4sr_regen_plan* p, int64_t n_pair, int32_t Ls, int32_t T, int32_t n_w) {
    if (const int rc = check_plan(p)) return rc;
    if (Ls > LMAX || T > LMAX) return DR4SR_E_SHAPE;
    if (n_pair < 0 || Ls < 1 || T < 1 || n_w < 1) return DR4SR_E_ARG;
    if (n_pair >= (1LL << 24) || n_pair * n_w * T >= (1LL << 30)) return DR4SR_E_ARG;
    return 0;
}

ScoreOff offsets_of(const dr4sr_regen_plan* p) {
    ScoreOff o;
    score_layout(p->n_rows, p->K, o.o);
    return o;
}

}  // namespace
