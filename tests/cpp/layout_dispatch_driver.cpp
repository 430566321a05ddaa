// layout_dispatch_driver.cpp CASES_FILE -- runs mo::decide_kernel (the decision mo_api.hip takes) on every line of CASES_FILE, written by
// tests/test_layout_dispatch_cpu.py from tests/layout_cases.py: one call of one case in one memory layout, as name=value tokens -- the
// shape, the plan's dtype and flags, the mode, and the strides, leading dimensions and (synthetic) base addresses of the layout.  Linked with
// the host-only objects of the fused units and of the generic kernel (their tables and size rules; nothing is launched).  Prints per line:
//   label <tab> kind <tab> family nt wps qpl mc jmode ny pck f32 pad (tabs) <tab> rows of the unit's table with that key <tab> unit <tab>
//   generic_needs_large <tab> name
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>

#include "../../mini_opt_amd/csrc/mo_fused_select.h"

static long long num(const std::map<std::string, std::string>& kv, const char* name) {
  auto it = kv.find(name);
  if (it == kv.end()) { fprintf(stderr, "missing token %s\n", name); exit(3); }
  return strtoll(it->second.c_str(), nullptr, 0);
}
static void* ptr(const std::map<std::string, std::string>& kv, const char* name) { return (void*)(uintptr_t)num(kv, name); }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 4;
  char line[4096];
  while (fgets(line, sizeof(line), f)) {
    std::map<std::string, std::string> kv;
    std::istringstream in(line);
    std::string tok;
    while (in >> tok) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) { fprintf(stderr, "bad token %s\n", tok.c_str()); return 3; }
      kv[tok.substr(0, eq)] = tok.substr(eq + 1);
    }
    if (kv.empty()) continue;
    mo::KernelArgs a;
    memset(&a, 0, sizeof(a));
    a.n = (int)num(kv, "n"); a.k = (int)num(kv, "k"); a.m = (int)num(kv, "m"); a.m_r = (int)num(kv, "m_r");
    a.mode = (int)num(kv, "mode"); a.flags = (unsigned)num(kv, "flags"); a.batch = num(kv, "batch");
    a.J = ptr(kv, "J"); a.J_stride = num(kv, "J_stride"); a.J_ld = (int)num(kv, "J_ld"); a.J_row_major = 1;
    a.r = ptr(kv, "r"); a.r_stride = num(kv, "r_stride");
    a.lambda = 1e-3; a.lambda_vec = ptr(kv, "lam"); a.lambda_vec_stride = num(kv, "lam_stride");
    a.G = ptr(kv, "G"); a.G_stride = num(kv, "G_stride"); a.G_ld = (int)num(kv, "G_ld");
    a.c = ptr(kv, "c"); a.c_stride = num(kv, "c_stride");
    a.A = ptr(kv, "A"); a.A_stride = num(kv, "A_stride"); a.A_ld = (int)num(kv, "A_ld");
    a.b = ptr(kv, "b"); a.b_stride = num(kv, "b_stride");
    a.cons_var = (const int*)ptr(kv, "cons_var"); a.cons_a = ptr(kv, "cons_a"); a.cons_b = ptr(kv, "cons_b"); a.cons_stride = num(kv, "cons_stride");
    a.vars = ptr(kv, "vars"); a.vars_stride = num(kv, "vars_stride");
    a.mu = ptr(kv, "mu"); a.mu_stride = num(kv, "mu_stride"); a.tau = 0.995;
    a.barrier_strategy = (int)num(kv, "strategy");
    a.sp.barrier_strategy = (int)num(kv, "strategy");
    a.delta = ptr(kv, "delta"); a.delta_stride = num(kv, "delta_stride");
    a.r_out = ptr(kv, "r_out"); a.r_out_stride = num(kv, "r_out_stride");
    a.G_out = ptr(kv, "G_out"); a.G_out_stride = num(kv, "G_out_stride"); a.G_out_ld = (int)num(kv, "G_out_ld");
    a.c_out = ptr(kv, "c_out"); a.c_out_stride = num(kv, "c_out_stride");
    a.ticket = (unsigned long long*)(uintptr_t)0x10000;
    a.static_rounds = -1;
    a.no_tiny = (int)num(kv, "no_tiny");
    const int dtype = (int)num(kv, "dtype");
    const mo::KernelDecision d = mo::decide_kernel(a, dtype, num(kv, "force_generic") != 0, 256);
    const mo::FusedKey& key = d.launch.key;
    int found = 0;
    const char* unit = "generic";
    if (d.kind == mo::KERNEL_FUSED_F64 || d.kind == mo::KERNEL_FUSED_F32) {
      static const char* const units[] = {"main", "gather", "ny2", "ny34", "mc4", "tiny", "f32"};
      const int u = mo::fused_unit(key);
      unit = units[u];
      const mo::FusedTable table = u == mo::UNIT_F32 ? mo::fused_f32_table() : mo::fused_table(u);
      for (int i = 0; i < table.count; ++i)
        if (table.rows[i].key == key && table.rows[i].kernel) ++found;
    }
    const int elem = dtype == MO_F64 ? 8 : 4;
    printf("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%d\t%s\n", kv["label"].c_str(), d.kind, key.family, key.nt, key.wps, key.qpl,
           key.mc, key.jmode, key.ny, key.pck, key.f32, key.pad, found, unit, d.kind == mo::KERNEL_GENERIC ? (int)mo::generic_needs_large(a, elem) : 0,
           d.name);
  }
  fclose(f);
  return 0;
}
