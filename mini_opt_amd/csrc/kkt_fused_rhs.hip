// kkt_fused_rhs.hip -- the fused fp64 step kernel (kkt_fused.hip) instantiated in its right-hand-side mode (RHS = true): mo_kkt_solve on the
// matrix cores.  Same J stream, assembly, block LDL^T, substitution and scheduling as the step; only the right-hand side (the caller's rho,
// or the transformed g of MO_KKT_TRANSPOSE) and the epilogue (no residual, no alpha) differ.  A translation unit of its own: the mode is a
// template argument, so no instantiation of the other units carries a register or an instruction of it.
// Coverage (fused_rhs_supported, mo_fused_select.h): one or two y tiles, one or two constraint slots, (G, c) or the 16-byte vector stream.
#define MO_FUSED_IMPL_ONLY
#include "kkt_fused.hip"

namespace mo {
namespace {
// The twin of the step kernel with these template arguments, filed under the STEP kernel's key.
template <int NT, int WPS, bool QPL, int MC, int NY> FusedRow rhs_row() {
  return FusedRow{FusedKey{FUSED_STEP, NT, WPS, QPL, MC, JMODE_VECTOR, NY, 1}, kkt_fused_f64_kernel<NT, WPS, QPL, MC, JMODE_VECTOR, NY, true>};
}
#define MO_RHS_ROWS(NT, WPS, MC, NY) rhs_row<NT, WPS, false, MC, NY>(), rhs_row<NT, WPS, true, MC, NY>()
// (NT, WPS, MC, NY), J-level and (G, c) each; WPS as fused_wps() gives it to the step sibling
const FusedRow kRows[] = {
    MO_RHS_ROWS(2, 4, 1, 1), MO_RHS_ROWS(2, 3, 2, 1), MO_RHS_ROWS(2, 3, 2, 2),
    MO_RHS_ROWS(4, 3, 1, 1), MO_RHS_ROWS(4, 2, 2, 1), MO_RHS_ROWS(4, 2, 2, 2),
    MO_RHS_ROWS(6, 2, 1, 1), MO_RHS_ROWS(6, 2, 2, 1), MO_RHS_ROWS(6, 1, 2, 2),
    MO_RHS_ROWS(8, 1, 1, 1), MO_RHS_ROWS(8, 1, 2, 1), MO_RHS_ROWS(8, 1, 2, 2),
#ifdef MO_TUNING   // MO_FUSED_WPS: the twins of the plain step kernel with one wave per SIMD less
    MO_RHS_ROWS(2, 3, 1, 1), MO_RHS_ROWS(4, 2, 1, 1),
#endif
};
#undef MO_RHS_ROWS
}  // namespace
FusedTable fused_rhs_table() { return {kRows, MO_FUSED_TABLE_SIZE(kRows)}; }

hipError_t launch_fused_rhs(const KernelArgs& a, int, int num_cus, hipStream_t stream) {
  return fused_launch(fused_rhs_table(), fused_rhs_select(a, num_cus), a, stream);   // a supported key without a row is an error, never another kernel
}

}  // namespace mo
