// fused_dispatch_lattice.h -- the shape lattice of tests/test_fused_dispatch_cpu.py.  The ORDER of the enumeration is the contract between
// tests/golden/fused_dispatch/index.u16.xz (one record index per point) and the test's driver: change neither without the other.
// Pointers are placeholders with the alignment the dispatch looks at; nothing is ever launched on them.
#pragma once
#include <cstring>

#include "../../mini_opt_amd/csrc/mo_kernels.h"

namespace lattice {

constexpr int kN[] = {2, 7, 15, 16, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128};
constexpr int kK[] = {0, 1, 8, 15, 16, 31, 32, 47, 48, 63};
constexpr int kM[] = {0, 1, 64, 65, 128, 129, 256};
constexpr int kMr[] = {8, 64, 65, 130};
constexpr int kMode[] = {mo::MODE_LINEARIZE, mo::MODE_RESIDUAL, mo::MODE_STEP, mo::MODE_ITERATE, mo::MODE_SOLVE};
constexpr long long kBatch[] = {1, 3, 4096, 65536, 1ll << 20};
constexpr int kStaticRounds[] = {-1, 0, 1 << 30};
constexpr int kNumCus = 256;
// input kinds: 0 (G, c); then J-level: 1 packed 16-byte-aligned row-major, 2 column-major, 3 row-major with J_ld > n, 4 a pointer that is
// only 8-byte aligned, 5 an odd J_stride.  Kind 0 is enumerated once, kinds 1 .. 5 once per m_r.
constexpr int kInputKinds = 6;

inline mo::KernelArgs make_args(int n, int k, int m, int mode, unsigned flags, int kind, int m_r, bool pc, int no_tiny, long long batch,
                                int static_rounds) {
  mo::KernelArgs a;
  memset(&a, 0, sizeof(a));
  void* const p = (void*)(uintptr_t)0x10000;   // 16-byte aligned
  a.n = n; a.k = k; a.m = m; a.mode = mode; a.flags = flags; a.batch = batch;
  if (kind == 0) {
    a.G = p; a.G_ld = n; a.G_stride = (long long)n * n; a.c = p; a.c_stride = n;
  } else {
    const long long packed = (long long)m_r * n;
    a.m_r = m_r; a.r = p; a.r_stride = m_r;
    a.J = kind == 4 ? (void*)(uintptr_t)0x10008 : p;
    a.J_row_major = kind != 2;
    a.J_ld = kind == 2 ? m_r : (kind == 3 ? n + 2 : n);
    a.J_stride = kind == 3 ? (long long)m_r * (n + 2) : (kind == 5 ? packed + ((packed & 1) ? 2 : 1) : packed);
  }
  a.A = p; a.A_ld = k; a.A_stride = (long long)k * n; a.b = p; a.b_stride = k;
  a.cons_var = (const int*)p; a.cons_a = p; a.cons_b = p; a.cons_stride = m;
  a.vars = p; a.vars_stride = n + 2 * m + k; a.mu = p; a.mu_stride = 1; a.tau = 0.995;
  a.barrier_strategy = pc ? MO_PREDICTOR_CORRECTOR : MO_COMPLEMENTARITY;
  a.sp.barrier_strategy = (mo_barrier_strategy)a.barrier_strategy;
  a.delta = p; a.delta_stride = a.vars_stride; a.alpha = p; a.status = (int*)p; a.ip_out = p;
  a.r_out = p; a.r_out_stride = a.vars_stride; a.kkt_out = p;
  a.G_out = p; a.G_out_ld = n; a.G_out_stride = (long long)n * n; a.c_out = p; a.c_out_stride = n;
  a.ticket = (unsigned long long*)p;
  a.static_rounds = static_rounds;
  a.no_tiny = no_tiny;
  return a;
}

// f(const mo::KernelArgs&) for every point, outermost loop first: n, k, m, mode, MO_STEP_NO_INEQUALITIES (STEP / RESIDUAL only), input
// (kind 0, then kinds 1 .. 5 x m_r), predictor-corrector, no_tiny, batch, static_rounds.
template <class F>
void for_each_point(F&& f) {
  for (int n : kN) for (int k : kK) for (int m : kM) for (int mode : kMode) {
    const int nflags = (mode == mo::MODE_STEP || mode == mo::MODE_RESIDUAL) ? 2 : 1;
    for (int fl = 0; fl < nflags; ++fl)
      for (int kind = 0; kind < kInputKinds; ++kind)
        for (int mr_i = 0; mr_i < (kind == 0 ? 1 : (int)(sizeof(kMr) / sizeof(int))); ++mr_i)
          for (int pc = 0; pc < 2; ++pc) for (int no_tiny = 0; no_tiny < 2; ++no_tiny)
            for (long long batch : kBatch) for (int sr : kStaticRounds)
              f(make_args(n, k, m, mode, fl ? MO_STEP_NO_INEQUALITIES : 0u, kind, kMr[mr_i], pc != 0, no_tiny, batch, sr));
  }
}

}  // namespace lattice
