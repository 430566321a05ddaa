// fused_rhs_dispatch_driver.cpp OUT_DIR -- walks a shape lattice of mo_kkt_solve arguments (MODE_RHS) through mo::decide_kernel (the
// decision mo_api.hip takes: fused_rhs_supported / fused_rhs_select / fused_rhs_name behind it) and the table of kkt_fused_rhs.hip (host objects only: nothing is launched) and writes, for
// tests/test_fused_rhs_dispatch_cpu.py:
//   OUT_DIR/shapes.txt    one line per (n, k, m, kind, m_r, flags, no_tiny): supported, the key, the name, rows of the table with that key
//   OUT_DIR/counters.txt  name <tab> count: points walked and every violation the walk counts itself
//   OUT_DIR/table.txt     every row of the RHS table: the key, how many lattice points selected it
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../mini_opt_amd/csrc/mo_fused_select.h"
#include "fused_dispatch_lattice.h"

static const int kN[] = {1, 2, 7, 8, 15, 16, 20, 31, 32, 33, 63, 64, 65, 90, 95, 96, 97, 127, 128, 129};
static const int kK[] = {0, 1, 4, 7, 8, 13, 15, 16, 31, 32, 47};
static const int kM[] = {0, 1, 64, 65, 128, 129, 130, 256};
static const int kMr[] = {8, 64, 65, 130};
static const unsigned kFlags[] = {0u, MO_STEP_NO_INEQUALITIES, MO_KKT_TRANSPOSE, MO_STEP_NO_INEQUALITIES | MO_KKT_TRANSPOSE};
static const long long kBatch[] = {1, 3, 4096, 65536, 1ll << 20};
static const int kStaticRounds[] = {-1, 0, 1 << 30};

static std::string launch_text(const mo::FusedLaunch& L) {
  char buf[256];
  const mo::FusedKey& k = L.key;
  snprintf(buf, sizeof buf, "%d %d %d %d %d %d %d %d | %d %u %u %d %d %d %d", k.family, k.nt, k.wps, k.qpl, k.mc, k.jmode, k.ny, k.pck,
           L.problems_per_wg, L.grid, L.block, (int)L.zero_ticket, L.stagger, L.chain_prio, L.static_rounds);
  return buf;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string out = argv[1];
  const mo::FusedTable table = mo::fused_rhs_table();
  std::vector<long long> hits(table.count, 0);
  long long points = 0, supported = 0, supported_without_step = 0, launch_differs = 0, rows_not_one = 0, f32_supported = 0, not_rhs_mode_supported = 0,
            null_rhs_supported = 0, varies_with_batch = 0, decision_differs = 0;
  FILE* f = fopen((out + "/shapes.txt").c_str(), "w");
  if (!f) return 4;
  for (int n : kN) for (int k : kK) for (int m : kM) for (int kind = 0; kind < lattice::kInputKinds; ++kind)
    for (int mr_i = 0; mr_i < (kind == 0 ? 1 : 4); ++mr_i) for (unsigned flags : kFlags) for (int no_tiny = 0; no_tiny < 2; ++no_tiny) {
      int shape_supported = -1, found = 0;
      mo::FusedKey key{};
      const char* name = "generic";
      for (long long batch : kBatch) for (int sr : kStaticRounds) {
        mo::KernelArgs a = lattice::make_args(n, k, m, mo::MODE_RHS, flags, kind, kMr[mr_i], false, no_tiny, batch, sr);
        a.alpha = nullptr; a.mu = nullptr;
        a.rhs = (const void*)(uintptr_t)0x20008; a.rhs_stride = a.vars_stride;   // 8-byte aligned only
        ++points;
        if (mo::fused_rhs_supported(a, MO_F32) || mo::decide_kernel(a, MO_F32, false, lattice::kNumCus).kind != mo::KERNEL_GENERIC) ++f32_supported;
        mo::KernelArgs b = a; b.mode = mo::MODE_STEP; b.flags = flags & ~(unsigned)MO_KKT_TRANSPOSE;
        if (mo::fused_rhs_supported(b, MO_F64)) ++not_rhs_mode_supported;
        b = a; b.rhs = nullptr;
        if (mo::fused_rhs_supported(b, MO_F64)) ++null_rhs_supported;
        const mo::KernelDecision d = mo::decide_kernel(a, MO_F64, false, lattice::kNumCus);
        const bool sup = d.kind == mo::KERNEL_FUSED_RHS;
        if (sup != mo::fused_rhs_supported(a, MO_F64) || (!sup && d.kind != mo::KERNEL_GENERIC) ||
            mo::decide_kernel(a, MO_F64, true, lattice::kNumCus).kind != mo::KERNEL_GENERIC) ++decision_differs;
        if (shape_supported >= 0 && shape_supported != (int)sup) ++varies_with_batch;
        shape_supported = sup;
        if (!sup) continue;
        ++supported;
        // the step the same arguments would launch
        mo::KernelArgs s = a; s.mode = mo::MODE_STEP; s.flags = flags & ~(unsigned)MO_KKT_TRANSPOSE; s.rhs = nullptr;
        if (!mo::fused_supported(s, MO_F64)) { ++supported_without_step; continue; }
        const mo::FusedLaunch Ls = mo::fused_select(s, lattice::kNumCus), Lr = d.launch;
        if (launch_text(Ls) != launch_text(Lr)) ++launch_differs;
        found = 0;
        for (int i = 0; i < table.count; ++i)
          if (table.rows[i].key == Lr.key && table.rows[i].kernel) { ++hits[i]; ++found; }
        if (found != 1) ++rows_not_one;
        key = Lr.key; name = d.name;
      }
      fprintf(f, "%d\t%d\t%d\t%d\t%d\t%u\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%d\n", n, k, m, kind, kind == 0 ? 0 : kMr[mr_i], flags, no_tiny, shape_supported,
              key.nt, key.wps, key.qpl, key.mc, key.jmode, key.ny, name, found);
    }
  fclose(f);
  f = fopen((out + "/counters.txt").c_str(), "w");
  if (!f) return 4;
  fprintf(f, "points\t%lld\nsupported\t%lld\nsupported_without_step\t%lld\nlaunch_differs\t%lld\nrows_not_one\t%lld\nf32_supported\t%lld\n"
             "not_rhs_mode_supported\t%lld\nnull_rhs_supported\t%lld\nvaries_with_batch\t%lld\ndecision_differs\t%lld\n",
          points, supported, supported_without_step, launch_differs, rows_not_one, f32_supported, not_rhs_mode_supported, null_rhs_supported, varies_with_batch,
          decision_differs);
  fclose(f);
  f = fopen((out + "/table.txt").c_str(), "w");
  if (!f) return 4;
  for (int i = 0; i < table.count; ++i) {
    const mo::FusedKey& k = table.rows[i].key;
    fprintf(f, "%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%lld\n", k.family, k.nt, k.wps, k.qpl, k.mc, k.jmode, k.ny, k.pck, hits[i]);
  }
  fclose(f);
  return 0;
}
