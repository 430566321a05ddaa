// fused_dispatch_driver.cpp OUT_DIR -- walks the lattice of fused_dispatch_lattice.h through mo::decide_kernel (the decision mo_api.hip
// takes: fused_supported / fused_select / fused_name behind it) with an fp64 plan and the units' kernel tables (host objects only: nothing
// is launched) and writes, for tests/test_fused_dispatch_cpu.py:
//   OUT_DIR/records.txt   distinct launch descriptions, one per line, tab-separated in the field order of the golden; line 0: unsupported
//   OUT_DIR/index.u16     one record index per lattice point, in enumeration order
//   OUT_DIR/tables.txt    every table row: unit, the key, how many lattice points selected it
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../mini_opt_amd/csrc/mo_fused_select.h"
#include "fused_dispatch_lattice.h"

static const char* const kFamily[] = {"step", "solve", "linearize", "tiny"};

static std::string key_text(const mo::FusedKey& k) {
  char buf[128];
  snprintf(buf, sizeof buf, "%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d", kFamily[k.family], k.nt, k.wps, k.qpl, k.mc, k.jmode, k.ny, k.pck);
  return buf;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string out = argv[1];
  std::map<std::string, int> ids;
  std::vector<std::string> recs;
  std::vector<unsigned short> idx;
  auto intern = [&](const std::string& s) {
    auto it = ids.find(s);
    if (it != ids.end()) return it->second;
    const int i = (int)recs.size();
    ids[s] = i;
    recs.push_back(s);
    return i;
  };
  intern("unsupported");
  std::vector<std::vector<long long>> hits(mo::FUSED_UNITS);
  for (int u = 0; u < mo::FUSED_UNITS; ++u) hits[u].assign(mo::fused_table(u).count, 0);
  long long forced_not_generic = 0, other_fused_kind = 0;

  lattice::for_each_point([&](const mo::KernelArgs& a) {
    const mo::KernelDecision d = mo::decide_kernel(a, MO_F64, false, lattice::kNumCus);
    if (mo::decide_kernel(a, MO_F64, true, lattice::kNumCus).kind != mo::KERNEL_GENERIC) ++forced_not_generic;
    if (d.kind != mo::KERNEL_FUSED_F64) {   // an fp64 plan outside MODE_RHS: the fused fp64 kernels or the generic one, nothing else
      if (d.kind != mo::KERNEL_GENERIC) ++other_fused_kind;
      idx.push_back(0);
      return;
    }
    const mo::FusedLaunch& L = d.launch;
    const int unit = mo::fused_unit(L.key);
    const mo::FusedTable t = mo::fused_table(unit);
    int found = 0;
    for (int i = 0; i < t.count; ++i)
      if (t.rows[i].key == L.key && t.rows[i].kernel) { ++hits[unit][i]; ++found; }
    char buf[256];
    snprintf(buf, sizeof buf, "\t%u\t%u\t%d\t%d\t%d\t%d\t%s\t%d", L.grid, L.block, (int)L.zero_ticket, L.stagger, L.chain_prio, L.static_rounds,
             d.name, found);
    idx.push_back((unsigned short)intern(key_text(L.key) + buf));
  });
  if (recs.size() > 65535) return 3;
  if (forced_not_generic || other_fused_kind) return 5;

  FILE* f = fopen((out + "/records.txt").c_str(), "w");
  if (!f) return 4;
  for (const auto& r : recs) fprintf(f, "%s\n", r.c_str());
  fclose(f);
  f = fopen((out + "/index.u16").c_str(), "wb");
  if (!f) return 4;
  fwrite(idx.data(), sizeof(unsigned short), idx.size(), f);
  fclose(f);
  f = fopen((out + "/tables.txt").c_str(), "w");
  if (!f) return 4;
  for (int u = 0; u < mo::FUSED_UNITS; ++u) {
    const mo::FusedTable t = mo::fused_table(u);
    for (int i = 0; i < t.count; ++i) fprintf(f, "%d\t%s\t%lld\n", u, key_text(t.rows[i].key).c_str(), hits[u][i]);
  }
  fclose(f);
  return 0;
}
