// kkt_fused_ny34.hip -- the fused fp64 kernels (kkt_fused.hip) instantiated with THREE and FOUR y tiles: 32 <= k <= 47 and 48 <= k <= 63 equality
// constraints on the 32- and 64-variable tile grids (the reference puts no limit on the number of equality rows, qp.cc:36-48; beyond these
// shapes the generic kernel takes over).  Every y tile but the last is a full 16-pivot tile of the Schur complement; the last holds the
// remaining rows and the right-hand side in index 15.  (NT + NY)(NT + NY + 1) / 2 live tiles: 15 / 21 on the 32 grid (three / two waves per
// SIMD), 28 / 36 on the 64 grid (one wave per SIMD), 45 / 55 on the 96 grid, 66 on the 128 grid with three (round 4: k <= 63 up to n = 96, k <= 47 up to n = 128).  Packed even-n J or (G, c) input with m <= 256 (two constraint slots per lane, four beyond 128: round 4); any other layout of J through the gather
// stream with m <= 64 (round 4).
#define MO_FUSED_IMPL_ONLY
#include "kkt_fused.hip"

namespace mo {
namespace {
constexpr int kUnit = UNIT_NY34;
// (G, c) or packed J with two or four constraint slots, every other layout of J on the gather stream with one
const FusedRow kRows[] = {
    MO_FUSED_ROW(FUSED_STEP, 2, 3, false, 1, JMODE_GATHER, 3, true),
    MO_FUSED_ROW(FUSED_STEP, 2, 3, false, 2, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_STEP, 2, 3, true, 2, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_STEP, 2, 3, false, 4, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_STEP, 2, 3, true, 4, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_STEP, 4, 1, false, 1, JMODE_GATHER, 3, true),
    MO_FUSED_ROW(FUSED_STEP, 4, 1, false, 2, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_STEP, 4, 1, true, 2, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_STEP, 4, 1, false, 4, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_STEP, 4, 1, true, 4, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_STEP, 6, 1, false, 1, JMODE_GATHER, 3, true),
    MO_FUSED_ROW(FUSED_STEP, 6, 1, false, 2, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_STEP, 6, 1, true, 2, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_STEP, 6, 1, false, 4, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_STEP, 6, 1, true, 4, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_STEP, 8, 1, false, 1, JMODE_GATHER, 3, true),
    MO_FUSED_ROW(FUSED_STEP, 8, 1, false, 2, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_STEP, 8, 1, true, 2, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_STEP, 8, 1, false, 4, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_STEP, 8, 1, true, 4, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_STEP, 2, 2, false, 1, JMODE_GATHER, 4, true),
    MO_FUSED_ROW(FUSED_STEP, 2, 2, false, 2, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_STEP, 2, 2, true, 2, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_STEP, 2, 2, false, 4, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_STEP, 2, 2, true, 4, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_STEP, 4, 1, false, 1, JMODE_GATHER, 4, true),
    MO_FUSED_ROW(FUSED_STEP, 4, 1, false, 2, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_STEP, 4, 1, true, 2, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_STEP, 4, 1, false, 4, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_STEP, 4, 1, true, 4, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_STEP, 6, 1, false, 1, JMODE_GATHER, 4, true),
    MO_FUSED_ROW(FUSED_STEP, 6, 1, false, 2, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_STEP, 6, 1, true, 2, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_STEP, 6, 1, false, 4, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_STEP, 6, 1, true, 4, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_SOLVE, 2, 2, false, 1, JMODE_GATHER, 3, true),
    MO_FUSED_ROW(FUSED_SOLVE, 2, 2, false, 2, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_SOLVE, 2, 2, true, 2, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_SOLVE, 2, 2, false, 4, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_SOLVE, 2, 2, true, 4, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 1, false, 1, JMODE_GATHER, 3, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 1, false, 2, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 1, true, 2, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 1, false, 4, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 1, true, 4, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, false, 1, JMODE_GATHER, 3, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, false, 2, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, true, 2, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, false, 4, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, true, 4, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_SOLVE, 8, 1, false, 1, JMODE_GATHER, 3, true),
    MO_FUSED_ROW(FUSED_SOLVE, 8, 1, false, 2, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_SOLVE, 8, 1, true, 2, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_SOLVE, 8, 1, false, 4, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_SOLVE, 8, 1, true, 4, JMODE_VECTOR, 3, true),
    MO_FUSED_ROW(FUSED_SOLVE, 2, 2, false, 1, JMODE_GATHER, 4, true),
    MO_FUSED_ROW(FUSED_SOLVE, 2, 2, false, 2, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_SOLVE, 2, 2, true, 2, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_SOLVE, 2, 2, false, 4, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_SOLVE, 2, 2, true, 4, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 1, false, 1, JMODE_GATHER, 4, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 1, false, 2, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 1, true, 2, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 1, false, 4, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 1, true, 4, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, false, 1, JMODE_GATHER, 4, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, false, 2, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, true, 2, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, false, 4, JMODE_VECTOR, 4, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, true, 4, JMODE_VECTOR, 4, true),
};
}  // namespace
FusedTable fused_table_ny34() { return {kRows, MO_FUSED_TABLE_SIZE(kRows)}; }

}  // namespace mo
