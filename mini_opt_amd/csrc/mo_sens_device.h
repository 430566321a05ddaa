// mo_sens_device.h -- what the sensitivity kernels share (qp_grad.hip, qp_tangent.hip, qp_tangent_blocks.hip, residual_blocks.hip; DESIGN.md
// section 4.8): the workgroup size, the 16-byte vector types and their launch-side checks, the grid of the persistent workgroups, and the
// constraint-row part of rho that the dense and the block tangent kernel compute alike.
#pragma once
#include "mo_kernels.h"

namespace mo {

constexpr int kThreads = 256;

template <typename T> struct Vec;
template <> struct Vec<double> { using type = double2; static constexpr int N = 2; };
template <> struct Vec<float> { using type = float4; static constexpr int N = 4; };

// sum over aligned groups of `width` lanes (a power of two <= 64): the same tree on every launch
template <typename T> __device__ __forceinline__ T group_sum(T v, int width) {
  for (int off = width >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// v rounded up to whole 16-byte pieces of VN = Vec<T>::N elements: every LDS vector of the dense kernels starts on a 16-byte boundary
template <int VN, typename I> __host__ __device__ constexpr I pad16(I v) { return (v + VN - 1) / VN * VN; }

// 16-byte accesses to a per-problem matrix: base, leading dimension and problem stride all multiples of 16 bytes
inline bool vec_ok(const void* base, long long stride, int ld, int elem) {
  const int vn = 16 / elem;
  return base && ((uintptr_t)base & 15) == 0 && stride % vn == 0 && ld % vn == 0;
}

// a workgroup per problem in turn: as many resident workgroups as the LDS allows, at most eight per CU (eight waves per SIMD keep enough
// loads in flight).  lds_bytes = 0: eight per CU whatever the kernel uses (the dense gradient and tangent kernels)
inline unsigned grid_for(long long batch, int num_cus, size_t lds_bytes) {
  long long per_cu = 8;
  if (lds_bytes > 0) {
    const long long fit = (long long)((160 * 1024) / (lds_bytes + 64));
    per_cu = fit < per_cu ? (fit < 1 ? 1 : fit) : per_cu;
  }
  long long g = (long long)num_cus * per_cu;
  if (g > batch) g = batch;
  return (unsigned)(g < 1 ? 1 : g);
}

// ---- the constraint rows of rho (forward mode): rho_d -= sum_i dcons_a[i] z_i e_{var_i}, rho_comp = 0, rho_pi[i] = dcons_a[i] x[var_i] + dcons_b[i]

// phase 1: cv[i] = cons_var[i], an index outside [0, n) as -1 (F_ASSERT qp.cc:70-72: never an index); az[i] = dcons_a[i] z_i, z = vars + z0
template <typename T>
__device__ __forceinline__ void cons_rows_load(int* cv, T* az, const int* cons_var, const T* dcons_a, const T* vars, int z0, int n, int m,
                                               int tid) {
  for (int i = tid; i < m; i += kThreads) {
    int v = cons_var ? cons_var[i] : 0;
    if (v < 0 || v >= n) v = -1;
    cv[i] = v;
    az[i] = dcons_a ? dcons_a[i] * vars[z0 + i] : (T)0;
  }
}

// rho_d[var_i] -= az[i]: the owner of variable j walks the rows in their order, however many name j
template <typename T> __device__ __forceinline__ void cons_rows_scatter(T* rho_d, const int* cv, const T* az, int n, int m, int tid) {
  for (int j = tid; j < n; j += kThreads) {
    T s = rho_d[j];
    for (int i = 0; i < m; ++i)
      if (cv[i] == j) s -= az[i];
    rho_d[j] = s;
  }
}

// a b + c as the caller's kernel rounds it: one FMA (the units compile with -ffp-contract=fast), or the product rounded before the sum (the
// block kernels, which run under fp contract(off): the pragma is lexical and would not reach a helper out here)
template <bool kContract, typename T> __device__ __forceinline__ T mul_add(T a, T b, T c) {
  if (kContract) return a * b + c;
  {
#pragma clang fp contract(off)
    const T p = a * b;
    return p + c;
  }
}

// rho_comp[i] = rho[comp0 + i] = 0 and rho_pi[i] = rho[pi0 + i] = dcons_a[i] x[var_i] + dcons_b[i], NaN for a row whose index is none
template <typename T, bool kContract>
__device__ __forceinline__ void cons_rows_write(T* rho, int comp0, int pi0, const int* cv, const T* dcons_a, const T* dcons_b, const T* x,
                                                int m, int tid) {
  for (int i = tid; i < m; i += kThreads) {
    rho[comp0 + i] = (T)0;
    const int v = cv[i];
    const T b = dcons_b ? dcons_b[i] : (T)0;
    T out = b;
    if (dcons_a) out = mul_add<kContract>(dcons_a[i], x[v < 0 ? 0 : v], b);
    rho[pi0 + i] = v < 0 ? (T)__builtin_nan("") : out;
  }
}

}  // namespace mo
