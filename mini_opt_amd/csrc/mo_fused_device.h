// mo_fused_device.h -- what the fused single-wavefront kernels of both precisions share on the device (kkt_fused.hip and the units built on it,
// kkt_fused_f32.hip): the wave primitives, and the one statement of which problem a wave of the persistent grid works on next.
// Device code only; every translation unit gets its own copy (anonymous namespace).
#pragma once

#include "mo_kernels.h"

namespace mo {
namespace {

// Phase stamps exist only in the diagnostic builds of tools/phase_timer.hip (MO_FUSED_STAMPS) and tools/phase_timer_f32.hip (MO_F32_STAMPS);
// the product kernels execute none.
#if defined(MO_FUSED_STAMPS) || defined(MO_F32_STAMPS)
#define MO_STAMP(i)                                                                                   \
  do {                                                                                                \
    __builtin_amdgcn_sched_barrier(0);                                                                \
    unsigned long long t__;                                                                           \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t__)::"memory");                       \
    stamp_acc[i] += t__ - stamp_prev;                                                                 \
    stamp_prev = t__;                                                                                 \
    __builtin_amdgcn_sched_barrier(0);                                                                \
  } while (0)
#else
#define MO_STAMP(i) do { } while (0)
#endif

// Lane index recomputed on the spot (two VALU ops).  The asm is volatile on purpose: nothing derived from it can be hoisted
// out of a loop and kept live in VGPRs the tiles need.
__device__ inline int lane_id() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

// The kernel's argument block as the hardware sees it (kernarg segment, constant address space), behind a pointer the
// compiler cannot see through: loads through it stay where they are written instead of being hoisted to the kernel entry.
typedef const KernelArgs __attribute__((address_space(4)))* KArgs;
__device__ inline KArgs fresh_args() {
  KArgs p = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}

// A 64-bit value that is wave-uniform by construction, said so to hipcc where its divergence analysis gives up (values carried around a
// loop with data-dependent exits; lane 0's ticket): two readfirstlanes, which fold away when the value already sits in SGPRs.
__device__ inline long long uniform64(unsigned long long v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// LDS-DMA: every lane's 16 bytes at `gsrc` land at LDS byte address lds_dst + 16 * lane (no VGPR destination).
// hipcc does not count this load: its completion is waited for by hand with wait_vmcnt<N>() (loads retire in order).
__device__ inline void dma16(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_dst)
      : "memory");
}
// Same with 4 bytes per lane: LDS byte address lds_dst + 4 * lane.
__device__ inline void dma4(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_dst)
      : "memory");
}
template <int N> __device__ inline void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory"); }
__device__ inline void lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }  // single-wave workgroup

// One ticket of `chunk` problems from the device-wide counter (zeroed on the stream before the launch).  Lane 0 asks; the answer is made
// uniform (uniform64) only where it is used, so the atomic's latency hides under whatever lies between.
__device__ inline unsigned long long take_counter_ticket(unsigned long long* counter, int chunk) {
  unsigned long long t = 0;
  if (lane_id() == 0) t = atomicAdd(counter, (unsigned long long)chunk);
  return t;
}

// ---- problem hand-out of the persistent grid (WAVES = 4 WPS waves per workgroup, one workgroup per CU) ---------------------------------
// The policy of the six fused kernels of kkt_fused.hip and kkt_fused_f32.hip (kkt_fused_tiny.hip keeps one of its own -- tickets of up to 64
// problems, a floor chunk and a skip scan -- and shares only uniform64 and take_counter_ticket).
// Problems are handed out from the device-wide ticket counter: the SIMD arbitrates oldest-wave-first and CUs do not run at identical speed,
// so a static split leaves 12-30 % of the waves idle at the end (measured with tools/phase_timer).  Tickets are taken in guided chunks (up to
// 8 problems while the queue is long, single problems at the end) because one counter word sustains only ~88 M atomics/s, and the next
// chunk is requested at the START of the current chunk's last problem, so the atomic's latency hides under the J stream.
// The FIRST chunk of every wave is static (wave w of the persistent grid takes problems [w c0, (w + 1) c0)); tickets from the counter start
// behind that part (ticket_base).  All waves asking one counter word for their first ticket at kernel start costs 3 072 / 88 M atomics/s =
// 35 us: most of a small launch (BASELINE configs[1]: 4 096 problems) and 2 % of the headline one.
// Small launches -- at most a.static_rounds problems per wave -- are split STATICALLY, round by round, in slot-major wave order (first one
// wave on every SIMD of every CU, then the second wave of every SIMD, ...): no ticket at all.  A wave must otherwise wait for a ticket just
// to learn that nothing is left, and 3 072 waves asking one counter word is again 35 us -- as long as the whole first round of BASELINE
// configs[1].  A partial round then also lands one wave per SIMD instead of three per SIMD on a third of the CUs.
//
// How a kernel uses it.  The state stays in the kernel's own locals, and four pieces stay written out in each kernel -- the static-rounds
// predicate, the chunk size (a lambda), the first problem of a wave and the branch at the loop end: as shared functions (or inside an
// object that owns p) they compile to other control flow and scalar code, and the spill figures or wait operands of the kernels that
// already spill move with it
// (profiles/refactor_fused_device_isa.txt).  They must stay equal in the six kernels: tests/test_fused_handout_text_cpu.py compares the texts.
//   const int chunk_shift = queue_chunk_shift<WAVES>();
//   const long long waves_all = (long long)gridDim.x * WAVES;
//   const bool st_rounds = a.static_rounds > 0 && a.batch <= (long long)a.static_rounds * waves_all;   // wave-uniform
//   queue_stagger(a, st_rounds, wave);                                   // step kernels only
//   auto chunk_for = [&](long long observed) -> int { if (st_rounds) return 1; c = (a.batch - observed) >> chunk_shift; return clamp(c, 1, 8); };
//   int chunk = chunk_for(0);
//   const long long ticket_base = (long long)gridDim.x * WAVES * chunk;
//   long long p = st_rounds ? <slot-major rank of the wave> : ((long long)blockIdx.x * WAVES + wave) * chunk;   // static first chunk
//   long long chunk_end = p + chunk;
//   while (p < a.batch) {
//     const bool last_of_chunk = p + 1 >= chunk_end;                     // wave-uniform
//     int next_chunk = 0;
//     unsigned long long next_ticket = 0;
//     if (last_of_chunk) { next_chunk = chunk_for(p); next_ticket = queue_take_ticket(a, st_rounds, next_chunk, p); }
//     ... problem p ...
//     if (last_of_chunk) { p = queue_ticket_problem(next_ticket, ticket_base); chunk_end = p + next_chunk; } else { ++p; }
//   }
template <int WAVES> __device__ inline int queue_chunk_shift() {   // guided chunk ~ remaining / (4 waves' worth)
  return 63 - __builtin_clzll((unsigned long long)gridDim.x * WAVES * 4);
}
__device__ inline unsigned long long queue_take_ticket(const KernelArgs& a, bool st_rounds, int chunk, long long p_now) {
  if (st_rounds) return (unsigned long long)p_now;   // static rounds: the next problem of this wave is p_now + all waves (= "ticket" p_now + ticket_base)
  return take_counter_ticket(a.ticket, chunk);
}
__device__ inline long long queue_ticket_problem(unsigned long long ticket, long long ticket_base) { return uniform64(ticket) + ticket_base; }
// Start stagger (step kernels).  Every problem costs the same, so the waves that share a SIMD (waves w, w + 4, w + 8 of the workgroup) would
// march through the phases in lockstep for the whole launch -- three J streams together, then three dependent pivot chains together.
// Delaying the second and third wave of each SIMD once, by about a third of a problem each (a.stagger units of 127 x 64 cycles), keeps one
// wave in the matrix-bound phase while another is in the sweeps: +1.4 % at cfg 3 (A/B on one box), nothing at cfg 2.
__device__ inline void queue_stagger(const KernelArgs& a, bool st_rounds, int wave) {
  if (a.stagger > 0 && !st_rounds) {
    const int slot = wave >> 2;
    for (int i = 0; i < slot * a.stagger; ++i) __builtin_amdgcn_s_sleep(127);
  }
}

}  // namespace
}  // namespace mo
