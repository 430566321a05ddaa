// kkt_fused_gather.hip -- the fused fp64 kernels (kkt_fused.hip) instantiated with the per-lane gather stream (JMODE_GATHER): J in any
// layout the C ABI accepts -- column-major, a leading dimension beyond n, rows that are only 8-byte aligned, odd n up to 128.  A
// translation unit of its own so that the instantiations compile beside the fast-path ones.
#define MO_FUSED_IMPL_ONLY
#include "kkt_fused.hip"

namespace mo {
namespace {
constexpr int kUnit = UNIT_GATHER;
// waves per SIMD: the register budgets of the fast-path instantiations (fused_wps); one constraint slot per lane
const FusedRow kRows[] = {
    MO_FUSED_ROW(FUSED_LINEARIZE, 2, 3, false, 1, JMODE_GATHER, 1, true),
    MO_FUSED_ROW(FUSED_LINEARIZE, 4, 3, false, 1, JMODE_GATHER, 1, true),
    MO_FUSED_ROW(FUSED_LINEARIZE, 6, 2, false, 1, JMODE_GATHER, 1, true),
    MO_FUSED_ROW(FUSED_LINEARIZE, 8, 1, false, 1, JMODE_GATHER, 1, true),
    MO_FUSED_ROW(FUSED_STEP, 2, 4, false, 1, JMODE_GATHER, 1, true),
    MO_FUSED_ROW(FUSED_STEP, 4, 3, false, 1, JMODE_GATHER, 1, true),
    MO_FUSED_ROW(FUSED_STEP, 6, 2, false, 1, JMODE_GATHER, 1, true),
    MO_FUSED_ROW(FUSED_STEP, 8, 1, false, 1, JMODE_GATHER, 1, true),
    MO_FUSED_ROW(FUSED_SOLVE, 2, 3, false, 1, JMODE_GATHER, 1, true),
    MO_FUSED_ROW(FUSED_SOLVE, 4, 2, false, 1, JMODE_GATHER, 1, true),
    MO_FUSED_ROW(FUSED_SOLVE, 6, 1, false, 1, JMODE_GATHER, 1, true),
    MO_FUSED_ROW(FUSED_SOLVE, 8, 1, false, 1, JMODE_GATHER, 1, true),
};
}  // namespace
FusedTable fused_table_gather() { return {kRows, MO_FUSED_TABLE_SIZE(kRows)}; }

}  // namespace mo
