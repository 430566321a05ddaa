// mo_fused_select.h -- which kernel serves a call, as data.  Host code only: the key that names one template instantiation of a fused
// kernel (fp64, its right-hand-side twins, fp32), the launch description (key + geometry + the values written into the argument block), the
// functions that derive it from the arguments (fused_select, fused_rhs_select, fused_f32_select) with the public predicates beside them, so
// that every rule is written once; decide_kernel, the one decision of mo_api.hip between the fused families and the generic kernel; and
// fused_launch, the one launch tail.  The instantiations themselves are rows {key, kernel} of one table per translation unit
// (kkt_fused*.hip); the launchers there select, then fused_launch finds the row and launches it.
#pragma once
#include <stdlib.h>

#include "mo_kernels.h"

// The diagnostic builds of tools/phase_timer*.hip compile kkt_fused.hip alone: only its own table exists there, and shapes the one-tile
// kernel would take stay on the 32 grid.
#if defined(MO_FUSED_STAMPS) || defined(MO_GENERIC_STAMPS)
#define MO_FUSED_SINGLE_UNIT 1
#endif

namespace mo {

enum FusedFamily : int {
  FUSED_STEP = 0,       // kkt_fused_f64_kernel: the step, and EvaluateKKTConditions on the way (STEP)
  FUSED_SOLVE = 1,      // kkt_fused_solve_kernel: SOLVE, ITERATE, RESIDUAL
  FUSED_LINEARIZE = 2,  // kkt_fused_linearize_kernel: LINEARIZE
  FUSED_TINY = 3,       // kkt_tiny_kernel: the whole KKT system in one tile, every mode but LINEARIZE
};
constexpr int JMODE_VECTOR = 0, JMODE_FLAT = 1, JMODE_GATHER = 2;   // how J reaches the matrix cores (kkt_fused.hip "J stream")

// One template instantiation.  Every field is always set: a parameter the family's kernel does not have holds the value below.
struct FusedKey {
  int family;
  int nt = 1;               // tile grid: 16 nt variables (2 / 4 / 6 / 8)
  int wps = 3;              // waves per SIMD the kernel is register-budgeted for; the workgroup has 4 wps waves
  int qpl = 0;              // QP-level input (G, c) instead of (J, r, lambda)
  int mc = 1;               // constraint slots per lane: m <= 64 mc
  int jmode = JMODE_VECTOR;
  int ny = 1;               // y tiles: k <= 16 ny - 1
  int pck = 1;              // Solve kernel: carries the code of the predictor-corrector's second solve
  int f32 = 0;              // an fp32 kernel (kkt_fused_f32.hip): named by family, nt (4 / 8), wps and pad; every other field at its default
  int pad = 0;              // fp32 step / Solve: n below the tile grid, masked inside the kernel
};
constexpr bool operator==(const FusedKey& a, const FusedKey& b) {
  return a.family == b.family && a.nt == b.nt && a.wps == b.wps && a.qpl == b.qpl && a.mc == b.mc && a.jmode == b.jmode && a.ny == b.ny &&
         a.pck == b.pck && a.f32 == b.f32 && a.pad == b.pad;
}

struct FusedLaunch {
  FusedKey key;
  int problems_per_wg;  // divisor of the grid formula: 4 (one problem per SIMD), 4 wps for the one-tile kernel
  unsigned grid, block;
  bool zero_ticket;     // the work counter is zeroed on the stream in front of the kernel
  int stagger, chain_prio, static_rounds;  // written to the argument block (mo_kernels.h)
};

// The translation unit whose table holds a key.  A function of the key alone: the routing conditions live in fused_select only, and a row
// written into the wrong unit's table does not compile (MO_FUSED_ROW).
// (FUSED_UNITS: the fp64 units fused_table() serves; the fp32 unit's table is fused_f32_table())
enum FusedUnit : int { UNIT_MAIN = 0, UNIT_GATHER, UNIT_NY2, UNIT_NY34, UNIT_MC4, UNIT_TINY, FUSED_UNITS, UNIT_F32 = FUSED_UNITS };
constexpr int fused_unit(const FusedKey& k) {
  if (k.f32) return UNIT_F32;
  if (k.family == FUSED_TINY) return UNIT_TINY;
  if (k.ny >= 3) return UNIT_NY34;
  if (k.ny == 2) return UNIT_NY2;
  if (k.jmode == JMODE_GATHER) return UNIT_GATHER;
  if (k.mc == 4 || (k.mc == 2 && k.family == FUSED_SOLVE && k.nt >= 6)) return UNIT_MC4;
  return UNIT_MAIN;
}

typedef void (*FusedKernel)(const KernelArgs);
struct FusedRow { FusedKey key; FusedKernel kernel; };
struct FusedTable { const FusedRow* rows; int count; };
FusedTable fused_table_main(), fused_table_gather(), fused_table_ny2(), fused_table_ny34(), fused_table_mc4(), fused_table_tiny();   // one per unit
FusedTable fused_table(int unit);   // kkt_fused.hip
#define MO_FUSED_TABLE_SIZE(rows) (int)(sizeof(rows) / sizeof(rows[0]))

// The one launch tail: the row of L.key in `table`, the scheduling values of L into the argument block, the ticket zeroed on the stream
// if L asks for it, the launch.  A key without a row is an internal error: there is no fallback kernel.
inline hipError_t fused_launch(FusedTable table, const FusedLaunch& L, const KernelArgs& a_in, hipStream_t stream) {
  FusedKernel kernel = nullptr;
  for (int i = 0; i < table.count && !kernel; ++i)
    if (table.rows[i].key == L.key) kernel = table.rows[i].kernel;
  if (!kernel) return hipErrorInvalidDeviceFunction;
  KernelArgs a = a_in;
  a.stagger = L.stagger; a.chain_prio = L.chain_prio; a.static_rounds = L.static_rounds;
  if (L.zero_ticket) {
    hipError_t e = hipMemsetAsync(a.ticket, 0, sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kernel, dim3(L.grid), dim3(L.block), 0, stream, a);
  return hipGetLastError();
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// J-level input whose layout the 16-byte / flat streams cannot take: column-major, a leading dimension beyond n, rows that are not 16-byte
// aligned (even n), odd n beyond the flat stream's 64 -- served by the per-lane gather stream (JMODE_GATHER, kkt_fused_gather.hip).
inline bool fused_needs_gather(const KernelArgs& a) {
  if (!a.J) return false;
  if (!a.J_row_major || a.J_ld != a.n) return true;
  if (a.n & 1) return a.n > 64 || a.m > 64;
  return !aligned16(a.J) || (a.J_stride & 1);
}

// Fused single-wave MFMA kernels for fixed tile grids.  False if (shape, layout) is unsupported.
inline bool fused_supported(const KernelArgs& a, int dtype) {
  if (dtype != MO_F64) return false;
  if (a.flags & ~MO_STEP_NO_INEQUALITIES) return false;
  if (a.flags && a.mode != MODE_STEP && a.mode != MODE_RESIDUAL) return false;
  if (a.mode == MODE_LINEARIZE) {  // standalone J^T J: J-level fp64; packed J on the 16-byte stream, every other layout (odd n included) on the gather stream
    return a.J && a.ticket && a.G_out && a.c_out && a.n >= 2 && a.n <= 128 && a.m_r > 0 && a.J_ld >= (a.J_row_major ? a.n : a.m_r) && a.G_out_ld >= a.n;
  }
  if (a.mode != MODE_SOLVE && a.mode != MODE_ITERATE && a.mode != MODE_STEP && a.mode != MODE_RESIDUAL) return false;
  if (a.mode == MODE_RESIDUAL && !a.r_out) return false;
  if (a.n < 2 || a.n > 128) return false;  // padded to 32 / 64 / 96 / 128 variables inside the kernel
  if (a.m < 0) return false;
  if (a.k > 31) {  // one y tile up to k = 15, two (kkt_fused_ny2.hip) up to 31, three / four (kkt_fused_ny34.hip) up to 47 / 63 on the 32 / 64 grids,
                   // and since round 4 three / four on the 96 grid (45 / 55 live tiles) and three on the 128 grid (66: it spills, and is still 2 x the generic kernel)
    if (a.k > 63) return false;                  // (m <= 256 as everywhere since round 4: four constraint slots per lane beyond 128)
    if (a.n > 96 && a.k > 47) return false;      // (the 128 grid with four y tiles would be 78 live tiles)
  }
  // up to four constraint slots per lane: m <= 256 (beyond 128, and beyond 64 for Solve / Iterate on the 96 / 128 grids: kkt_fused_mc4.hip)
  if (a.m > 256) return false;
  // (round 4: the two-y-tile kernels carry up to four slots on every grid, Solve / Iterate included -- a box on each of 128 variables
  // beside 16 .. 31 equalities used to fall to the generic kernel)
  if (!a.ticket || !a.vars) return false;
  if (a.mode == MODE_STEP && !a.delta) return false;
  if (a.J) {  // J-level: 16-byte pieces of a packed row-major J (even n), the flat-group stream (odd n <= 64), or the gather stream
    if (a.m_r <= 0) return false;  // m_r % 4 rows are handled after the ring stream
    if (a.J_ld < (a.J_row_major ? a.n : a.m_r)) return false;
    // the gather and flat instantiations carry one constraint slot per lane (odd n with m > 64 is a gather shape: fused_needs_gather)
    if (fused_needs_gather(a) && a.m > 64) return false;
  } else {    // QP-level: G, c given; no alignment requirements
    if (!a.G || !a.c || a.G_ld < a.n) return false;
  }
  return true;
}

// kkt_fused_tiny.hip: n + k <= 15, m <= 64 (a subset of fused_supported: the caller has run fused_supported() on the same arguments)
inline bool fused_tiny_supported(const KernelArgs& a) {
  if (a.mode == MODE_LINEARIZE || a.no_tiny) return false;
  if (a.n + a.k > 15 || a.m > 64) return false;
  if (a.J && a.m_r > 64) return false;  // larger stacks: the 32-variable grid streams J through the matrix cores
  return true;
}

// Waves per SIMD an instantiation is register-budgeted for; index: the tile grid nt / 2 - 1.
inline int fused_wps(const FusedKey& k) {
  static const int by_grid[5][4] = {
      {3, 2, 1, 1},   // [0] the Solve kernel with one y tile (2 waves at n = 64, 3 at n = 32), every kernel with two y tiles ((NT + 2)(NT + 3) / 2
                      //     live tiles), and the step kernel with four constraint slots; the 96 / 128 grids are correctness-first (the 128 one spills)
      {4, 3, 2, 1},   // [1] the step kernel, one slot.  64 grid: 3 (A/B in DESIGN.md).  32 grid: FOUR since round 4 (the kernel needs 100 VGPRs,
                      //     its gather sibling 105).  Round 3 had measured a fourth wave 10 % slower at BASELINE configs[1] (0.136 vs 0.123 ms) -- when
                      //     launches still took a ticket per problem; with static rounds it is faster at every batch size: configs[1] 86.4 / 87.1 ->
                      //     94.9 / 96.4 M steps/s (4 096 problems are ONE round of 4 096 waves), batch 65 536: 140.6 -> 152.9 M.
      {3, 2, 2, 1},   // [2] the step kernel, two slots (a box on every one of 64 variables is m = 128)
      {3, 3, 2, 1},   // [3] the linearize kernel
      {3, 3, 0, 0}};  // [4] the step kernel on the flat stream (odd n <= 64)
  const int g = k.nt / 2 - 1;
  if (k.family == FUSED_LINEARIZE) return by_grid[3][g];
  // three / four y tiles: 15 / 21 live tiles on the 32 grid (three / two waves per SIMD; the Solve kernel two), 28 and more beyond: one wave
  if (k.ny >= 3) return k.nt > 2 ? 1 : (k.ny == 4 || k.family == FUSED_SOLVE ? 2 : 3);
  if (k.ny == 2 || k.family == FUSED_SOLVE || k.mc == 4) return by_grid[0][g];
  if (k.mc == 2) return by_grid[2][g];
  return k.jmode == JMODE_FLAT ? by_grid[4][g] : by_grid[1][g];
}

#ifdef MO_TUNING   // (A/B builds only: the product library reads no environment variable)
inline int fused_env_int(const char* name, int otherwise) { const char* e = getenv(name); return e ? atoi(e) : otherwise; }
#endif

// The tile grid a problem of n variables is padded to (16 nt variables), and the tile park of the fused fp64 Solve kernels beyond the 32
// grid: the elements of one wave slot -- the nt (nt + 1) / 2 tiles of G and nt vectors a wave cannot keep in LDS between the passes.  The
// plan allocates fused_tile_park_slots slots of it (one workgroup per CU, at most twelve waves each) and hands the kernel the slot size.
constexpr int fused_nt(int n) { return n > 96 ? 8 : n > 64 ? 6 : n > 32 ? 4 : 2; }
constexpr size_t fused_tile_park_slot_elems(int n) { return (size_t)(fused_nt(n) * (fused_nt(n) + 1) / 2) * 256 + (size_t)fused_nt(n) * 64; }
constexpr size_t fused_tile_park_slots(int num_cus) { return (size_t)num_cus * 12; }

// Static rounds up to this many problems per wave (mo_kernels.h; measured): the caller's value, else equal-cost work
// (step, Iterate, residual, linearisation) splits statically further than a Solve, whose problems need different numbers of passes.
inline int fused_static_rounds(const KernelArgs& a) {
  return a.static_rounds >= 0 ? a.static_rounds : a.mode == MODE_SOLVE ? (a.n > 32 ? 2 : 6) : (a.n > 32 ? 8 : 32);
}
// The work counter is zeroed on the stream in front of the kernel -- unless the launch is certain to run in static rounds, which never
// touch it: every kernel has at least 4 waves per workgroup and min(CUs, ceil(batch / 4)) workgroups, so batch <= rounds x 4 x workgroups
// is static whatever the instantiation (the kernels test batch <= rounds x waves).  One enqueued operation less per small launch.
inline bool fused_zero_ticket(int static_rounds, long long batch, int num_cus) {
  return !(static_rounds > 0 && batch <= (long long)static_rounds * 4 * fused_grid(batch, num_cus));
}

// Everything launch_fused needs to know about a launch of supported arguments (fused_supported(a, MO_F64) holds).
// (static: an A/B library links objects built with and without -DMO_TUNING, tools/ab_build.sh, and each must keep its own copy)
static inline FusedLaunch fused_select(const KernelArgs& a, int num_cus) {
  FusedLaunch L{};
  const bool solve = a.mode == MODE_SOLVE || a.mode == MODE_ITERATE || a.mode == MODE_RESIDUAL;
  L.static_rounds = fused_static_rounds(a);
  // start stagger and chain priority: the 64-variable grid of the step kernel with J-level input (the BASELINE configs[2] / [4] shape);
  // measured neutral elsewhere
  const bool headline_shape = a.mode == MODE_STEP && a.J && a.n > 32 && a.n <= 64;
  L.stagger = headline_shape ? 4 : 0;
  L.chain_prio = headline_shape ? 1 : 0;
#ifdef MO_TUNING
  static const int env_stagger = fused_env_int("MO_FUSED_STAGGER", -1);   // units + 256 * priority
  if (env_stagger >= 0) { L.stagger = env_stagger & 0xff; L.chain_prio = (env_stagger >> 8) & 1; }
#endif

  FusedKey& key = L.key;
#ifdef MO_FUSED_SINGLE_UNIT
  const bool tiny = false;
#else
  const bool tiny = fused_tiny_supported(a);
#endif
  if (tiny) {  // the whole KKT system in one tile: 145 VGPRs, three waves per SIMD (four would spill)
    key.family = FUSED_TINY;
    L.problems_per_wg = 4 * key.wps;
    L.zero_ticket = true;         // the one-tile kernel hands out tickets of up to 64 problems whatever the size
  } else {
    key.family = a.mode == MODE_LINEARIZE ? FUSED_LINEARIZE : solve ? FUSED_SOLVE : FUSED_STEP;
    key.nt = fused_nt(a.n);
    const bool qp = key.family != FUSED_LINEARIZE;
    key.qpl = !a.J;
    // one y tile up to k = 15, two up to 31, three / four up to 47 / 63; every y tile but the last is a full 16-pivot tile
    key.ny = !qp ? 1 : a.k > 47 ? 4 : a.k > 31 ? 3 : a.k > 15 ? 2 : 1;
    // J-level input: 16-byte pieces of a packed row-major J (even n); odd n <= 64 on the flat-group stream, which only the one-y-tile
    // step / Solve kernels have; the per-lane gather stream for every other layout
    const bool odd = a.J && (a.n & 1);
    key.jmode = !a.J ? JMODE_VECTOR : (fused_needs_gather(a) || (odd && (!qp || key.ny > 1))) ? JMODE_GATHER : odd ? JMODE_FLAT : JMODE_VECTOR;
    // Constraint slots per lane.  The gather and flat instantiations carry one (fused_supported keeps them at m <= 64); four beyond m = 128;
    // three / four y tiles: two; two y tiles: two, but one where it is enough for the Solve kernel on the 64 grid and beyond (fewer live
    // registers); one y tile: what m needs.
    if (!qp || key.jmode != JMODE_VECTOR) key.mc = 1;
    else if (a.m > 128) key.mc = 4;
    else if (key.ny >= 3) key.mc = 2;
    else if (key.ny == 2) key.mc = (solve && key.nt >= 4 && a.m <= 64) ? 1 : 2;
    else key.mc = a.m > 64 ? 2 : 1;
    key.wps = fused_wps(key);
    // The corrector's second solve keeps all 21 factor tiles of the 64 grid alive behind the back-substitution: with it the two-y-tile Solve
    // kernel needs more than the 256 registers of two waves per SIMD (84 B of scratch per lane), without it none; the one-y-tile, two-slot,
    // J-level one on the 64 grid needs 20 B with it, none without.  Hence two instantiations there, picked by barrier strategy: PCK = false
    // for COMPLEMENTARITY / FIXED_DECREASE (and the KKT residual), PCK = true for PREDICTOR_CORRECTOR.
    const bool pc = (a.mode == MODE_SOLVE ? a.sp.barrier_strategy : a.barrier_strategy) == MO_PREDICTOR_CORRECTOR && a.mode != MODE_RESIDUAL;
    const bool has_lean = key.family == FUSED_SOLVE && key.mc <= 2 &&
                          ((key.ny == 2 && key.nt <= 4) || (key.ny == 1 && key.mc == 2 && key.nt == 4 && !key.qpl));
    key.pck = !(has_lean && !pc);
#ifdef MO_TUNING
    // waves per SIMD of the plain step kernel (one y tile, one slot, vector stream): 2 instead of 3 on the 64 grid, 3 instead of 4 on the 32 grid
    static const int env_wps = fused_env_int("MO_FUSED_WPS", 0);
    if (key.family == FUSED_STEP && key.ny == 1 && key.mc == 1 && key.jmode == JMODE_VECTOR && ((key.nt == 4 && env_wps == 2) || (key.nt == 2 && env_wps == 3)))
      key.wps = env_wps;
    // Solve with two y tiles on the 64 grid: 21 live tiles + the loop state do not fit the 256 registers of two waves per SIMD (408 B of spill
    // per lane, which showed up as 30 GB of HBM traffic per launch in profiles/r03_solve_k24_*).  MO_NY2_SOLVE_WPS=1: one wave per SIMD, no spill.
    static const int env_ny2_solve_wps = fused_env_int("MO_NY2_SOLVE_WPS", 0);
    if (key.family == FUSED_SOLVE && key.ny == 2 && key.nt == 4 && key.mc <= 2 && env_ny2_solve_wps == 1) { key.wps = 1; key.pck = 1; }
#endif
    L.problems_per_wg = 4;
    L.zero_ticket = fused_zero_ticket(L.static_rounds, a.batch, num_cus);
  }
  L.grid = fused_grid(a.batch, num_cus, L.problems_per_wg);   // one workgroup of 4 wps waves per CU; problems are pulled from the ticket counter
  L.block = 256u * key.wps;
  return L;
}

// The kernel name the plan reports (mo_plan_step_kernel): family, input level and tile grid of the key.
inline const char* fused_name(const FusedKey& k) {
  static const char* const names[2][2][4] = {
      {{"fused_mfma_f64_n32", "fused_mfma_f64_n64", "fused_mfma_f64_n96", "fused_mfma_f64_n128"},
       {"fused_qp_f64_n32", "fused_qp_f64_n64", "fused_qp_f64_n96", "fused_qp_f64_n128"}},
      {{"fused_solve_mfma_f64_n32", "fused_solve_mfma_f64_n64", "fused_solve_mfma_f64_n96", "fused_solve_mfma_f64_n128"},
       {"fused_solve_qp_f64_n32", "fused_solve_qp_f64_n64", "fused_solve_qp_f64_n96", "fused_solve_qp_f64_n128"}}};
  return names[k.family == FUSED_SOLVE][k.qpl][k.nt / 2 - 1];
}
inline const char* fused_name(const KernelArgs& a, const FusedKey& key) {
  if (key.family == FUSED_TINY) {  // one instantiation for every mode and input level: the name tells what it was asked for
    const bool solve = a.mode == MODE_SOLVE || a.mode == MODE_ITERATE || a.mode == MODE_RESIDUAL;
    if (!a.J) return solve ? "fused_solve_qp_tiny_f64" : "fused_qp_tiny_f64";
    return solve ? "fused_solve_tiny_f64" : "fused_tiny_f64";
  }
  return fused_name(key);
}
static inline const char* fused_name(const KernelArgs& a, int) { return fused_name(a, fused_select(a, 1).key); }

hipError_t launch_fused(const KernelArgs& a, int dtype, int num_cus, hipStream_t stream);   // kkt_fused.hip

// ---- the right-hand-side mode of the step kernel (mo_kkt_solve, MODE_RHS; kkt_fused_rhs.hip) ------------------------------------------
// The RHS kernel of a shape is the twin of that shape's step kernel -- kkt_fused_f64_kernel<..., RHS = true> with the step's template
// arguments, grid, block and scheduling values -- so everything here derives from fused_select of the same arguments in MODE_STEP.
// The arguments a MODE_RHS call would hand to the step (MO_KKT_TRANSPOSE is the RHS kernel's own flag).
inline KernelArgs fused_rhs_as_step(const KernelArgs& a) {
  KernelArgs s = a;
  s.mode = MODE_STEP;
  s.flags = a.flags & ~(unsigned)MO_KKT_TRANSPOSE;
  return s;
}
// Coverage: fp64 shapes whose step runs kkt_fused_f64_kernel (not the one-tile kernel) with one or two y tiles (k <= 31), one or two
// constraint slots (m <= 128) and (G, c) or the 16-byte vector stream (packed row-major J, even n, 16-byte aligned, even stride).
// Everything else -- flat and gather streams, k > 31, m > 128, one-tile shapes, fp32 -- stays on the generic kernel.
inline bool fused_rhs_supported(const KernelArgs& a, int dtype) {
  if (a.mode != MODE_RHS || !a.rhs) return false;
  if (a.flags & ~(unsigned)(MO_STEP_NO_INEQUALITIES | MO_KKT_TRANSPOSE)) return false;
  const KernelArgs s = fused_rhs_as_step(a);
  if (!fused_supported(s, dtype)) return false;
  if (a.k > 31 || a.m > 128) return false;
  const FusedKey key = fused_select(s, 1).key;
  return key.family == FUSED_STEP && key.jmode == JMODE_VECTOR && key.ny <= 2 && key.mc <= 2;
}
// The launch of supported arguments: the step's launch description, field for field.
static inline FusedLaunch fused_rhs_select(const KernelArgs& a, int num_cus) { return fused_select(fused_rhs_as_step(a), num_cus); }
// The kernel name the plan reports (mo_plan_kkt_solve_kernel).
inline const char* fused_rhs_name(const FusedKey& k) {
  static const char* const names[2][4] = {{"fused_rhs_mfma_f64_n32", "fused_rhs_mfma_f64_n64", "fused_rhs_mfma_f64_n96", "fused_rhs_mfma_f64_n128"},
                                          {"fused_rhs_qp_f64_n32", "fused_rhs_qp_f64_n64", "fused_rhs_qp_f64_n96", "fused_rhs_qp_f64_n128"}};
  return names[k.qpl][k.nt / 2 - 1];
}
// Rows {the STEP kernel's key, kkt_fused_f64_kernel<..., RHS = true>}.  Not one of the FUSED_UNITS tables: it is reached through this
// function only, and a supported key without a row is an error (launch_fused_rhs), never another kernel.
FusedTable fused_rhs_table();                                                                    // kkt_fused_rhs.hip
hipError_t launch_fused_rhs(const KernelArgs& a, int dtype, int num_cus, hipStream_t stream);   // kkt_fused_rhs.hip

// ---- the fused fp32 kernels (kkt_fused_f32.hip): step, Solve / Iterate / residual and linearisation on the 64 / 128 grids -------------
inline bool fused_f32_supported(const KernelArgs& a, int dtype) {
  if (dtype != MO_F32) return false;
  if (a.mode == MODE_LINEARIZE && a.n != 128 && a.n != 64) return false;
  if (a.n < 4 || a.n > 128 || (a.n & 3)) return false;   // step / Solve / Iterate / residual: any multiple of 4, padded inside the kernels to the 64 / 128 grid
  if (a.mode == MODE_LINEARIZE) {  // kkt_fused_f32_linearize_kernel: packed row-major J, rows in whole 4-row groups
    return a.J && a.ticket && a.G_out && a.c_out && a.J_row_major && a.J_ld == a.n && a.m_r > 0 && !(a.m_r & 3) && aligned16(a.J) &&
           !(a.J_stride & 3) && aligned16(a.r) && !(a.r_stride & 3) && a.G_out_ld >= a.n;
  }
  if (a.k > 16 || a.m > 64 || a.m < 0) return false;
  if (!a.ticket || !a.vars) return false;
  if (a.mode == MODE_SOLVE || a.mode == MODE_ITERATE || a.mode == MODE_RESIDUAL) {  // kkt_fused_f32_solve_kernel
    if (a.mode == MODE_RESIDUAL ? ((a.flags & ~MO_STEP_NO_INEQUALITIES) != 0 || !a.r_out) : a.flags != 0) return false;
    if (a.J) {
      if (!a.J_row_major || a.J_ld != a.n || a.m_r <= 0) return false;
      if (!aligned16(a.J) || (a.J_stride & 3)) return false;
    } else if (!a.G || !a.c || a.G_ld < a.n) {
      return false;
    }
    return true;
  }
  if ((a.flags & ~MO_STEP_NO_INEQUALITIES) != 0 || a.mode != MODE_STEP) return false;
  if (!a.delta || !a.J) return false;
  if (!a.J_row_major || a.J_ld != a.n || a.m_r <= 0) return false;
  if (!aligned16(a.J) || (a.J_stride & 3)) return false;
  return true;
}

inline const char* fused_f32_name(const KernelArgs& a) {
  if (a.mode == MODE_LINEARIZE) return a.n > 64 ? "fused_linearize_f32_n128" : "fused_linearize_f32_n64";
  if (a.mode == MODE_STEP) return a.n > 64 ? "fused_mfma_f32_n128" : "fused_mfma_f32_n64";
  if (!a.J) return a.n > 64 ? "fused_solve_qp_f32_n128" : "fused_solve_qp_f32_n64";
  return a.n > 64 ? "fused_solve_mfma_f32_n128" : "fused_solve_mfma_f32_n64";
}

// The launch of supported arguments (fused_f32_supported(a, MO_F32) holds).  Waves per SIMD: the 128 grid runs the step and the
// linearisation at two (the step: 255 VGPRs, no scratch -- the 216 accumulator registers + operands just fit) and Solve / Iterate / residual
// at one (216 tile registers + the state); the 64 grid runs everything at three.  PAD: n below the grid.
static inline FusedLaunch fused_f32_select(const KernelArgs& a, int num_cus) {
  FusedLaunch L{};
  L.static_rounds = fused_static_rounds(a);
  L.chain_prio = a.chain_prio;   // (as handed in: the fp32 kernels have no chain priority of their own)
  FusedKey& key = L.key;
  const bool big = a.n > 64;
  key.family = a.mode == MODE_LINEARIZE ? FUSED_LINEARIZE : a.mode == MODE_STEP ? FUSED_STEP : FUSED_SOLVE;
  key.f32 = 1;
  key.nt = big ? 8 : 4;
  key.wps = !big ? 3 : key.family == FUSED_SOLVE ? 1 : 2;
  key.pad = key.family != FUSED_LINEARIZE && a.n != 16 * key.nt;
#ifdef MO_TUNING
  static const int env_stagger = fused_env_int("MO_FUSED_F32_STAGGER", -1);
  if (env_stagger >= 0) L.stagger = env_stagger;
  static const int env_wps = fused_env_int("MO_FUSED_F32_WPS", 0);   // the step on the 128 grid at one wave per SIMD
  if (key.family == FUSED_STEP && big && env_wps == 1) key.wps = 1;
#endif
  L.problems_per_wg = 4;
  L.zero_ticket = fused_zero_ticket(L.static_rounds, a.batch, num_cus);
  L.grid = fused_grid(a.batch, num_cus);
  L.block = 256u * key.wps;
  return L;
}
FusedTable fused_f32_table();                                                       // kkt_fused_f32.hip
hipError_t launch_fused_f32(const KernelArgs& a, int num_cus, hipStream_t stream);   // kkt_fused_f32.hip

// ---- which kernel serves a call ------------------------------------------------------------------------------------------------------
// The ONE decision of mo_api.hip, from the arguments, the plan's dtype and its force-generic flag: MODE_RHS (mo_kkt_solve) runs the step
// kernel's right-hand-side twin where one exists and the generic kernel everywhere else; every other mode the fused fp64 kernels, then the
// fused fp32 kernels, then the generic kernel.  `launch` is set for the fused kinds; `name` is what the plan's kernel queries report.
enum KernelKind : int { KERNEL_GENERIC = 0, KERNEL_FUSED_F64, KERNEL_FUSED_F32, KERNEL_FUSED_RHS };
struct KernelDecision { int kind; FusedLaunch launch; const char* name; };
static inline KernelDecision decide_kernel(const KernelArgs& a, int dtype, bool force_generic, int num_cus) {
  KernelDecision d{KERNEL_GENERIC, FusedLaunch{}, "generic"};
  if (force_generic) return d;
  if (a.mode == MODE_RHS) {
    if (fused_rhs_supported(a, dtype)) { d.kind = KERNEL_FUSED_RHS; d.launch = fused_rhs_select(a, num_cus); d.name = fused_rhs_name(d.launch.key); }
  } else if (fused_supported(a, dtype)) {
    d.kind = KERNEL_FUSED_F64; d.launch = fused_select(a, num_cus); d.name = fused_name(a, d.launch.key);
  } else if (fused_f32_supported(a, dtype)) {
    d.kind = KERNEL_FUSED_F32; d.launch = fused_f32_select(a, num_cus); d.name = fused_f32_name(a);
  }
  return d;
}

}  // namespace mo
