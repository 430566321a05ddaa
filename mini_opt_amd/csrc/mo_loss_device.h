// mo_loss_device.h -- the robust loss of one residual block, shared by the stand-alone kernel (residual_loss.hip)
// and the fused robust linearise (residual_blocks.hip, kL): both call the SAME three functions, so the weights and 0.5 sum rho of the fused
// call are the bits of mo_residual_loss_eval by construction.
//   s_b   = sum of r^2 over the block's rows IN ORDER, every square rounded before it is added (fp contract off: no FMA either side)
//   w_b   = rho'(s_b), rho_b = rho(s_b) in the forms below (no cancellation at s << a^2, none at s = a^2)
//   sum   a lane adds the rho_b of its blocks tid, tid + kThreads, ... in that order, then loss_rho_sum: the wave's butterfly, one value per
//         wave through LDS, thread 0 adds the waves in order -- the block_sum pattern of blocks_linearize_kernel's half_sq
#pragma once
#include "mo_sens_device.h"

namespace mo {

// s_b: the rows of one block in order
template <typename T> __device__ __forceinline__ T loss_block_sq(const T* r, int R) {
#pragma clang fp contract(off)
  T s = 0;
  for (int q = 0; q < R; ++q) {
    const T sq = r[q] * r[q];
    s += sq;
  }
  return s;
}

// (w, rho) at s for scale a.  Every comparison is written so that a NaN s takes the branch that computes with it (w and rho NaN).
//   HUBER    s <= a^2: (1, s), the quotient a / sqrt(s) is formed only beyond a^2 (never a / sqrt(0))
//   SOFT_L1  q = sqrt(1 + t): w = 1 / q, rho = 2 s / (q + 1)                        (= 2 a^2 (q - 1) without its cancellation at small t)
//   CAUCHY   w = 1 / (1 + t), rho = a^2 log1p(t)
//   TUKEY    s > a^2: (0, a^2 / 3) -- w EXACTLY 0; else u = (a^2 - s) / a^2 (the difference is exact near the cutoff): w = u^2,
//            rho = s (1 - t (1 - t / 3))                                            (= (a^2 / 3)(1 - u^3) without its cancellation at small t)
// with t = s / a^2.
template <typename T> __device__ __forceinline__ void loss_point(int kind, T a, T s, T* w_out, T* rho_out) {
#pragma clang fp contract(off)
  const T a2 = a * a;
  T w = (T)1, rho = s;
  if (kind == MO_LOSS_HUBER) {
    if (!(s <= a2)) {
      const T q = sqrt(s);
      w = a / q;
      const T two_q = q + q;
      const T d = two_q - a;
      rho = a * d;
    }
  } else if (kind == MO_LOSS_SOFT_L1) {
    const T t = s / a2;
    const T q = sqrt((T)1 + t);
    w = (T)1 / q;
    const T two_s = s + s;
    rho = two_s / (q + (T)1);
  } else if (kind == MO_LOSS_CAUCHY) {
    const T t = s / a2;
    w = (T)1 / ((T)1 + t);
    rho = a2 * log1p(t);
  } else if (kind == MO_LOSS_TUKEY) {
    if (s > a2) {
      w = (T)0;
      rho = a2 / (T)3;
    } else {
      const T t = s / a2;
      const T u = (a2 - s) / a2;
      w = u * u;
      const T t3 = t / (T)3;
      const T inner = (T)1 - t3;
      const T ti = t * inner;
      const T f = (T)1 - ti;
      rho = s * f;
    }
  }
  *w_out = w;
  *rho_out = rho;
}

// the workgroup's sum of the lanes' partial rho sums, valid in thread 0; `red` holds one value per wave
template <typename T> __device__ __forceinline__ T loss_rho_sum(T v, T* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  T s = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kThreads / 64; ++w) s += red[w];
  return s;
}

// One lane's blocks of one problem: the weight of every row of block b to w_rows (and to w_copy when given), the lane's partial rho sum returned.
template <typename T>
__device__ __forceinline__ T loss_blocks(const int4* blk, const T* scale, int num_blocks, const T* r, T* w_rows, T* w_copy, int tid) {
  T part = 0;
  for (int b = tid; b < num_blocks; b += kThreads) {
    const int4 bi = blk[b];  // {first stacked row, R_b, kind, 0}
    const T s = loss_block_sq(r + bi.x, bi.y);
    T w, rho;
    loss_point(bi.z, scale[b], s, &w, &rho);
    for (int q = 0; q < bi.y; ++q) {
      if (w_rows) w_rows[bi.x + q] = w;
      if (w_copy) w_copy[bi.x + q] = w;
    }
    part += rho;
  }
  return part;
}

}  // namespace mo
