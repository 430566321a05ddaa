// kkt_fused_ny2.hip -- the fused fp64 kernels (kkt_fused.hip) instantiated with TWO y tiles (NY = 2): 16 <= k <= 31 equality constraints.
// The first y tile is a full 16-pivot tile of the Schur complement, the second holds the remaining k - 16 rows and, as in the one-tile
// kernels, carries the right-hand side in index 15.  A translation unit of its own so that the instantiations compile beside the others.
// Waves per SIMD follow the register budget of the (NT + 2)(NT + 3) / 2 live tiles: 3 on the 32 grid, 2 on the 64 grid, 1 beyond.
#define MO_FUSED_IMPL_ONLY
#include "kkt_fused.hip"

namespace mo {
namespace {
constexpr int kUnit = UNIT_NY2;
// (G, c) or packed J with two or four constraint slots (the Solve kernel on the 64 grid and beyond: one where m <= 64), every other
// layout of J on the gather stream with one; the Solve kernel on the 32 / 64 grids with and without the corrector's code (PCK)
const FusedRow kRows[] = {
    MO_FUSED_ROW(FUSED_STEP, 2, 3, false, 1, JMODE_GATHER, 2, true),
    MO_FUSED_ROW(FUSED_STEP, 2, 3, false, 2, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_STEP, 2, 3, true, 2, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_STEP, 2, 3, false, 4, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_STEP, 2, 3, true, 4, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_STEP, 4, 2, false, 1, JMODE_GATHER, 2, true),
    MO_FUSED_ROW(FUSED_STEP, 4, 2, false, 2, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_STEP, 4, 2, true, 2, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_STEP, 4, 2, false, 4, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_STEP, 4, 2, true, 4, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_STEP, 6, 1, false, 1, JMODE_GATHER, 2, true),
    MO_FUSED_ROW(FUSED_STEP, 6, 1, false, 2, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_STEP, 6, 1, true, 2, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_STEP, 6, 1, false, 4, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_STEP, 6, 1, true, 4, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_STEP, 8, 1, false, 1, JMODE_GATHER, 2, true),
    MO_FUSED_ROW(FUSED_STEP, 8, 1, false, 2, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_STEP, 8, 1, true, 2, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_STEP, 8, 1, false, 4, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_STEP, 8, 1, true, 4, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 2, 3, false, 1, JMODE_GATHER, 2, false),
    MO_FUSED_ROW(FUSED_SOLVE, 2, 3, false, 1, JMODE_GATHER, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 2, 3, false, 2, JMODE_VECTOR, 2, false),
    MO_FUSED_ROW(FUSED_SOLVE, 2, 3, false, 2, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 2, 3, true, 2, JMODE_VECTOR, 2, false),
    MO_FUSED_ROW(FUSED_SOLVE, 2, 3, true, 2, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 2, 3, false, 4, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 2, 3, true, 4, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 2, false, 1, JMODE_VECTOR, 2, false),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 2, false, 1, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 2, true, 1, JMODE_VECTOR, 2, false),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 2, true, 1, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 2, false, 1, JMODE_GATHER, 2, false),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 2, false, 1, JMODE_GATHER, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 2, false, 2, JMODE_VECTOR, 2, false),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 2, false, 2, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 2, true, 2, JMODE_VECTOR, 2, false),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 2, true, 2, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 2, false, 4, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 2, true, 4, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, false, 1, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, true, 1, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, false, 1, JMODE_GATHER, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, false, 2, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, true, 2, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, false, 4, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, true, 4, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 8, 1, false, 1, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 8, 1, true, 1, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 8, 1, false, 1, JMODE_GATHER, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 8, 1, false, 2, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 8, 1, true, 2, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 8, 1, false, 4, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 8, 1, true, 4, JMODE_VECTOR, 2, true),
#ifdef MO_TUNING   // MO_NY2_SOLVE_WPS=1: Solve on the 64 grid with one wave per SIMD (no spill)
    MO_FUSED_ROW(FUSED_SOLVE, 4, 1, false, 1, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 1, true, 1, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 1, false, 1, JMODE_GATHER, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 1, false, 2, JMODE_VECTOR, 2, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 1, true, 2, JMODE_VECTOR, 2, true),
#endif
};
}  // namespace
FusedTable fused_table_ny2() { return {kRows, MO_FUSED_TABLE_SIZE(kRows)}; }

}  // namespace mo
