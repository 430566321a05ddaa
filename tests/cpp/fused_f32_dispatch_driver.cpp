// fused_f32_dispatch_driver.cpp OUT_DIR -- walks a shape lattice through mo::decide_kernel (the decision mo_api.hip takes) with an fp32 plan
// and the table of kkt_fused_f32.hip (host objects only: nothing is launched) and writes, for tests/test_fused_f32_dispatch_cpu.py:
//   OUT_DIR/points.txt    one line per (n, k, m, mode, flags, kind, m_r, batch, static_rounds): the decision's kind, the launch description,
//                         the name, rows of the table with that key
//   OUT_DIR/counters.txt  name <tab> count: points walked and every violation the walk counts itself
//   OUT_DIR/table.txt     every row of the fp32 table: the key, how many lattice points selected it
#include <cstdio>
#include <string>
#include <vector>

#include "../../mini_opt_amd/csrc/mo_fused_select.h"
#include "fused_dispatch_lattice.h"

static const int kN[] = {4, 8, 60, 63, 64, 68, 100, 124, 128, 132};
static const int kK[] = {0, 16, 17};
static const int kM[] = {0, 64, 65};
static const int kMr[] = {6, 8, 64};
static const int kMode[] = {mo::MODE_LINEARIZE, mo::MODE_RESIDUAL, mo::MODE_STEP, mo::MODE_ITERATE, mo::MODE_SOLVE, mo::MODE_RHS};
static const unsigned kFlags[] = {0u, MO_STEP_NO_INEQUALITIES};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string out = argv[1];
  const mo::FusedTable table = mo::fused_f32_table();
  std::vector<long long> hits(table.count, 0);
  long long points = 0, fused_f32 = 0, kind_is_not_the_predicate = 0, other_fused_kind = 0, forced_not_generic = 0, f64_plan_f32_kernel = 0,
            f64_plan_f32_predicate = 0, denormalised_key = 0;
  FILE* f = fopen((out + "/points.txt").c_str(), "w");
  if (!f) return 4;
  for (int n : kN) for (int k : kK) for (int m : kM) for (int mode : kMode) for (unsigned flags : kFlags)
    for (int kind = 0; kind < lattice::kInputKinds; ++kind) for (int mr_i = 0; mr_i < (kind == 0 ? 1 : 3); ++mr_i)
      for (long long batch : lattice::kBatch) for (int sr : lattice::kStaticRounds) {
        const mo::KernelArgs a = lattice::make_args(n, k, m, mode, flags, kind, kMr[mr_i], false, 0, batch, sr);
        ++points;
        // an fp64 plan never reaches an fp32 kernel, and a forced plan none at all
        if (mo::fused_f32_supported(a, MO_F64)) ++f64_plan_f32_predicate;
        if (mo::decide_kernel(a, MO_F64, false, lattice::kNumCus).kind == mo::KERNEL_FUSED_F32) ++f64_plan_f32_kernel;
        const mo::KernelDecision forced = mo::decide_kernel(a, MO_F32, true, lattice::kNumCus);
        if (forced.kind != mo::KERNEL_GENERIC || std::string(forced.name) != "generic") ++forced_not_generic;
        const mo::KernelDecision d = mo::decide_kernel(a, MO_F32, false, lattice::kNumCus);
        if ((d.kind == mo::KERNEL_FUSED_F32) != mo::fused_f32_supported(a, MO_F32)) ++kind_is_not_the_predicate;
        if (d.kind != mo::KERNEL_FUSED_F32 && d.kind != mo::KERNEL_GENERIC) ++other_fused_kind;
        const mo::FusedLaunch& L = d.launch;
        const mo::FusedKey& key = L.key;
        int found = 0;
        if (d.kind == mo::KERNEL_FUSED_F32) {
          ++fused_f32;
          for (int i = 0; i < table.count; ++i)
            if (table.rows[i].key == key && table.rows[i].kernel) { ++hits[i]; ++found; }
          if (!key.f32 || key.qpl != 0 || key.mc != 1 || key.jmode != mo::JMODE_VECTOR || key.ny != 1 || key.pck != 1 ||
              mo::fused_unit(key) != mo::UNIT_F32 || L.problems_per_wg != 4) ++denormalised_key;
        }
        fprintf(f, "%d\t%d\t%d\t%d\t%u\t%d\t%d\t%lld\t%d\t%d\t%d\t%d\t%d\t%d\t%u\t%u\t%d\t%d\t%d\t%d\t%s\t%d\n", n, k, m, mode, flags, kind,
                kind == 0 ? 0 : kMr[mr_i], batch, sr, d.kind == mo::KERNEL_FUSED_F32, key.family, key.nt, key.wps, key.pad, L.grid, L.block,
                (int)L.zero_ticket, L.static_rounds, L.stagger, L.chain_prio, d.name, found);
      }
  fclose(f);
  f = fopen((out + "/counters.txt").c_str(), "w");
  if (!f) return 4;
  fprintf(f, "points\t%lld\nfused_f32\t%lld\nkind_is_not_the_predicate\t%lld\nother_fused_kind\t%lld\nforced_not_generic\t%lld\n"
             "f64_plan_f32_kernel\t%lld\nf64_plan_f32_predicate\t%lld\ndenormalised_key\t%lld\n",
          points, fused_f32, kind_is_not_the_predicate, other_fused_kind, forced_not_generic, f64_plan_f32_kernel, f64_plan_f32_predicate,
          denormalised_key);
  fclose(f);
  f = fopen((out + "/table.txt").c_str(), "w");
  if (!f) return 4;
  for (int i = 0; i < table.count; ++i) {
    const mo::FusedKey& k = table.rows[i].key;
    fprintf(f, "%d\t%d\t%d\t%d\t%lld\n", k.family, k.nt, k.wps, k.pad, hits[i]);
  }
  fclose(f);
  return 0;
}
