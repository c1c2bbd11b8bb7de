/* dr4sr_hip_probes.h — PROBE entry points of libdr4sr_hip.so: device primitives run on their own, for tests/ only.
 *
 * Additive to the ABI and apart from both the product surface (include/dr4sr_hip.h) and the test / measurement hooks
 * (include/dr4sr_hip_hooks.h): dr4sr_amd/_lib.py binds them on first use (lane_probe()), not in load(), so that a library built
 * before they existed still loads (A/B runs through DR4SR_LIB_PATH).
 */
#ifndef DR4SR_HIP_PROBES_H
#define DR4SR_HIP_PROBES_H
#include "dr4sr_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The cross-lane primitives of csrc/common.h (DPP / permlane forms: the d = 64 latency kernels) beside the shuffle forms, on the same inputs.
 * One kernel, 256-thread blocks, thread i of n (a multiple of 256): in[i] (fp32) goes straight into every float reduction — no arithmetic
 * in front of it — and in_u[i] into the lane exchange.  out is [DR4SR_LANE_PROBE_N][2][n] words: out[(2 q + f) n + i] is primitive q's
 * result in thread i, f = 0 the DPP / permlane form, f = 1 the shuffle form. */
#define DR4SR_LP_GROUP16_SUM 0   /* group16_sum_dpp == lane_group_sum<16>: lanes 16 k .. 16 k + 15 */
#define DR4SR_LP_GROUP8_SUM  1   /* group8_sum: the `rd` head sum at n_head = 2, d = 64 */
#define DR4SR_LP_WAVE_SUM    2   /* wave_sum_dpp */
#define DR4SR_LP_XG_MAX      3   /* tattn::xg_max<true>: max over lanes l, l ^ 16, l ^ 32, l ^ 48 */
#define DR4SR_LP_XG_SUM      4   /* tattn::xg_sum<true> */
#define DR4SR_LP_FOLD        5   /* flush_affine's fold (xrow_sum) */
#define DR4SR_LP_XOR1        6   /* row_keep_word's exchange: in_u[i ^ 1] */
#define DR4SR_LANE_PROBE_N   7
int dr4sr_lane_probe(const float* in, const uint32_t* in_u, uint32_t* out, int64_t n, void* stream);

/* The tile plan of dr4sr_sasrec_layer_packed_fwd / _bwd (csrc/layer_packed.hip) on its own.  _chunk: the number C of consecutive
 * sequences that are planned together.  _plan: runs the plan launches for seqlen [B] (int64, device) on `stream` and writes, for every
 * sequence, tile_of[b] (int32 [B], device; -1: n_b = 0, the sequence has no rows) and row_of[b] (int32 [B]: its first row in that tile,
 * -1 beside tile_of = -1), and the tile count to n_tiles (int32 [1]).  ws as for the forward (backward = 0).  Refusals as the forward's. */
int32_t dr4sr_sasrec_layer_packed_chunk(void);
int dr4sr_sasrec_layer_packed_plan(const int64_t* seqlen, int64_t B, int32_t L, int32_t* tile_of, int32_t* row_of, int32_t* n_tiles, void* ws,
                                   int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DR4SR_HIP_PROBES_H */
