// kkt_fused_mc4.hip -- the fused fp64 kernels (kkt_fused.hip) with FOUR constraint slots per lane: 128 < m <= 256 inequality entries, e.g. a
// two-sided box on every one of 128 variables -- and Solve / Iterate / the KKT residual on the 96 / 128 tile grids with m > 64 (two or four
// slots), which the one-slot instantiations of kkt_fused.hip do not take.  k <= 15, packed (J, r, lambda) or (G, c).  The constraint state
// (s, z, a, b, variable, residual parts) lives in registers, so the larger grids spill: correctness-first instantiations, one or two waves per
// SIMD.  A translation unit of its own so that the instantiations compile beside the others.
#define MO_FUSED_IMPL_ONLY
#include "kkt_fused.hip"

namespace mo {
namespace {
constexpr int kUnit = UNIT_MC4;
// four slots on every grid; the Solve kernel with two on the 96 / 128 grids
const FusedRow kRows[] = {
    MO_FUSED_ROW(FUSED_STEP, 2, 3, false, 4, JMODE_VECTOR, 1, true),
    MO_FUSED_ROW(FUSED_STEP, 2, 3, true, 4, JMODE_VECTOR, 1, true),
    MO_FUSED_ROW(FUSED_STEP, 4, 2, false, 4, JMODE_VECTOR, 1, true),
    MO_FUSED_ROW(FUSED_STEP, 4, 2, true, 4, JMODE_VECTOR, 1, true),
    MO_FUSED_ROW(FUSED_STEP, 6, 1, false, 4, JMODE_VECTOR, 1, true),
    MO_FUSED_ROW(FUSED_STEP, 6, 1, true, 4, JMODE_VECTOR, 1, true),
    MO_FUSED_ROW(FUSED_STEP, 8, 1, false, 4, JMODE_VECTOR, 1, true),
    MO_FUSED_ROW(FUSED_STEP, 8, 1, true, 4, JMODE_VECTOR, 1, true),
    MO_FUSED_ROW(FUSED_SOLVE, 2, 3, false, 4, JMODE_VECTOR, 1, true),
    MO_FUSED_ROW(FUSED_SOLVE, 2, 3, true, 4, JMODE_VECTOR, 1, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 2, false, 4, JMODE_VECTOR, 1, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 2, true, 4, JMODE_VECTOR, 1, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, false, 2, JMODE_VECTOR, 1, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, true, 2, JMODE_VECTOR, 1, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, false, 4, JMODE_VECTOR, 1, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, true, 4, JMODE_VECTOR, 1, true),
    MO_FUSED_ROW(FUSED_SOLVE, 8, 1, false, 2, JMODE_VECTOR, 1, true),
    MO_FUSED_ROW(FUSED_SOLVE, 8, 1, true, 2, JMODE_VECTOR, 1, true),
    MO_FUSED_ROW(FUSED_SOLVE, 8, 1, false, 4, JMODE_VECTOR, 1, true),
    MO_FUSED_ROW(FUSED_SOLVE, 8, 1, true, 4, JMODE_VECTOR, 1, true),
};
}  // namespace
FusedTable fused_table_mc4() { return {kRows, MO_FUSED_TABLE_SIZE(kRows)}; }

}  // namespace mo
