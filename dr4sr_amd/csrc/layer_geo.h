// layer_geo.h — what the two encoder-layer ops (layer_op.hip: one sequence per tile; layer_packed.hip: several) agree on: the LDS
// geometry of a (D, F) instantiation, the layout of a weight-gradient slot, and the supported shapes.
#pragma once
#include "common.h"

namespace lop {

constexpr int LDT = 68;                // row stride of the [64][64] attention tiles
constexpr int TILE = 64 * LDT;

template <int D, int F> struct Geo {
    static constexpr int LDX = D + 4, LDF = F + 4, DH = D / 2, HG = 64 / DH, NG = D / 64;
    static constexpr int R_FLOATS = (64 * LDF > (3 + 2 * HG) * TILE) ? 64 * LDF : (3 + 2 * HG) * TILE;
    static constexpr int LDS_FLOATS = 2 * 64 * LDX + R_FLOATS + 64 + 4 * 64;
    // one slot of weight-gradient partials: the 12 tensors in the flat layout's order
    static constexpr int O_INW = 0, O_INB = O_INW + 3 * D * D, O_OW = O_INB + 3 * D, O_OB = O_OW + D * D, O_W1 = O_OB + D, O_B1 = O_W1 + F * D,
                         O_W2 = O_B1 + F, O_B2 = O_W2 + D * F, O_N1W = O_B2 + D, O_N1B = O_N1W + D, O_N2W = O_N1B + D, O_N2B = O_N2W + D,
                         NW = O_N2B + D;
};

static int shape_check(int64_t B, int L, int D, int H, int F) {
    if (B < 0 || L < 1 || D < 1 || H < 1 || F < 1) return DR4SR_E_ARG;
    if (L > 64 || D % H) return DR4SR_E_SHAPE;
    const int dh = D / H;
    if (!((D == 64 && (F == 128 || F == 256) && dh == 32) || (D == 128 && F == 128 && dh == 64))) return DR4SR_E_SHAPE;
    if (B * (int64_t)L * L >= ((int64_t)1 << 30)) return DR4SR_E_ARG;      // 32-bit sequence x head index of the attention dropout stream
    return 0;
}
static int64_t slot_floats(int D, int F) { return 4 * (int64_t)D * D + 2 * (int64_t)D * F + 9 * (int64_t)D + F; }

}  // namespace lop
