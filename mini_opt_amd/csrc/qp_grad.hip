// qp_grad.hip -- mo_qp_gradients: the gradients of a loss through the solution of a QP, from the state v = [x | s | y | z] and the adjoint
// u = K^-T g = [u_x | u_s | u_y | u_z] that mo_kkt_solve(MO_KKT_TRANSPOSE) returns.
//   dc = -u_x      dG = -1/2 (u_x x^T + x u_x^T)      dA_eq = y u_x^T - u_y x^T      db_eq = -u_y
//   dcons_a[i] = z_i u_x[var_i] - u_z[i] x[var_i]      dcons_b[i] = -u_z[i]
//   J-level:  t = J u_x,  w = J x + r:   dJ = -t x^T - w u_x^T      dr = -t      dlambda = -u_x . x
// Pure data movement.  One workgroup takes one problem at a time: the vectors go to LDS, the two products with J read J ONCE, in its stored
// layout, 16 bytes per lane, and every matrix output is a rank-2 update written 16 bytes per lane along its contiguous dimension, a whole
// line per group of lanes.  Every output element has one owner and a fixed order of operations: no atomics, the same bits on every launch.
// kThreads, Vec<T>, group_sum, pad16, vec_ok and grid_for are those of every sensitivity kernel: mo_sens_device.h.
#include "mo_sens_device.h"

namespace mo {
namespace {

// out[c * ld + r] = s1 a1[r] b1[c] + s2 a2[r] b2[c] for r < R (the contiguous dimension), c < C.  The two products are rounded before they
// are added (no contraction): with a1 = b2, a2 = b1 and s1 = s2 the element (r, c) and the element (c, r) are the same sum of the same two
// numbers, so dG is symmetric to the bit.  `vec`: base, ld and stride allow 16-byte stores.
template <typename T>
__device__ __forceinline__ void rank2_store(T* out, int ld, int R, int C, const T* a1, const T* b1, T s1, const T* a2, const T* b2, T s2,
                                            bool vec, int tid) {
#pragma clang fp contract(off)
  constexpr int VN = Vec<T>::N;
  if (vec) {
    const int rv = (R + VN - 1) / VN;  // 16-byte pieces per column (the last one may be partial)
    for (int e = tid; e < rv * C; e += kThreads) {
      const int c = e / rv, r0 = (e - c * rv) * VN;
      const T p1 = s1 * b1[c], p2 = s2 * b2[c];
      T* dst = out + (size_t)c * ld + r0;
      if (r0 + VN <= R) {
        typename Vec<T>::type v;
        T* ve = reinterpret_cast<T*>(&v);
#pragma unroll
        for (int q = 0; q < VN; ++q) {
          const T t1 = a1[r0 + q] * p1, t2 = a2[r0 + q] * p2;
          ve[q] = t1 + t2;
        }
        *reinterpret_cast<typename Vec<T>::type*>(dst) = v;
      } else {
        for (int q = 0; r0 + q < R; ++q) {
          const T t1 = a1[r0 + q] * p1, t2 = a2[r0 + q] * p2;
          dst[q] = t1 + t2;
        }
      }
    }
  } else {
    for (int e = tid; e < R * C; e += kThreads) {
      const int c = e / R, r = e - c * R;
      const T t1 = a1[r] * (s1 * b1[c]), t2 = a2[r] * (s2 * b2[c]);
      out[(size_t)c * ld + r] = t1 + t2;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void qp_grad_kernel(const GradArgs a, const int vec_J, const int vec_dJ, const int vec_dG,
                                                           const int vec_dA) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int VN = Vec<T>::N;
  using V = typename Vec<T>::type;
  const int n = a.n, k = a.k, m = a.m, m_r = a.J ? a.m_r : 0;
  // every vector starts on a 16-byte boundary
  const int n_p = pad16<VN>(n), k_p = pad16<VN>(k), m_p = pad16<VN>(m), r_p = pad16<VN>(m_r);
  T* x = reinterpret_cast<T*>(smem);
  T* ux = x + n_p;
  T* y = ux + n_p;
  T* uy = y + k_p;
  T* z = uy + k_p;
  T* uz = z + m_p;
  T* t = uz + m_p;   // J u_x
  T* w = t + r_p;    // J x + r
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const mo_qp_grads& o = a.out;

  for (long long p = blockIdx.x; p < a.batch; p += gridDim.x) {
    const T* vp = (const T*)a.vars + p * a.vars_stride;
    const T* up = (const T*)a.u + p * a.u_stride;
    __syncthreads();  // the previous problem's readers are done with the LDS
    for (int i = tid; i < n; i += kThreads) { x[i] = vp[i]; ux[i] = up[i]; }
    for (int i = tid; i < k; i += kThreads) { y[i] = vp[n + m + i]; uy[i] = up[n + m + i]; }
    for (int i = tid; i < m; i += kThreads) { z[i] = vp[n + m + k + i]; uz[i] = up[n + m + k + i]; }
    __syncthreads();

    if (m_r > 0) {
      const T* J = (const T*)a.J + p * a.J_stride;
      const T* rp = a.r ? (const T*)a.r + p * a.r_stride : nullptr;
      if (a.J_row_major) {
        // a row is shared by a group of G lanes (16 bytes each per pass), 64 / G rows per wave and pass; the group sums with shuffles
        const int nv = (n + VN - 1) / VN;
        int G = 1;
        while (G < nv && G < 64) G <<= 1;
        const int sub = lane / G, l = lane - sub * G, rows_per_pass = (kThreads / 64) * (64 / G);
        for (int q0 = 0; q0 < m_r; q0 += rows_per_pass) {   // (uniform bounds: every lane takes part in the shuffles)
          const int q = q0 + wave * (64 / G) + sub;
          T at = 0, aw = 0;
          if (q < m_r) {
            const T* row = J + (size_t)q * a.J_ld;
            for (int jv = l; jv < nv; jv += G) {
              const int j = jv * VN;
              if (vec_J && j + VN <= n) {
                const V v = *reinterpret_cast<const V*>(row + j);
                const T* ve = reinterpret_cast<const T*>(&v);
#pragma unroll
                for (int e = 0; e < VN; ++e) { at += ve[e] * ux[j + e]; aw += ve[e] * x[j + e]; }
              } else {
                for (int e = 0; e < VN && j + e < n; ++e) { const T v = row[j + e]; at += v * ux[j + e]; aw += v * x[j + e]; }
              }
            }
          }
          at = group_sum(at, G); aw = group_sum(aw, G);
          if (l == 0 && q < m_r) { t[q] = at; w[q] = aw + (rp ? rp[q] : (T)0); }
        }
      } else {
        // column-major: a lane owns VN consecutive rows and walks the columns; consecutive lanes read consecutive 16-byte pieces of a column
        const int rv = (m_r + VN - 1) / VN;
        for (int qv = tid; qv < rv; qv += kThreads) {
          const int q = qv * VN;
          T at[VN], aw[VN];
#pragma unroll
          for (int e = 0; e < VN; ++e) { at[e] = 0; aw[e] = 0; }
          if (vec_J && q + VN <= m_r) {
#pragma unroll 4
            for (int j = 0; j < n; ++j) {
              const V v = *reinterpret_cast<const V*>(J + (size_t)j * a.J_ld + q);
              const T* ve = reinterpret_cast<const T*>(&v);
              const T uj = ux[j], xj = x[j];
#pragma unroll
              for (int e = 0; e < VN; ++e) { at[e] += ve[e] * uj; aw[e] += ve[e] * xj; }
            }
          } else {
            for (int j = 0; j < n; ++j) {
              const T uj = ux[j], xj = x[j];
#pragma unroll
              for (int e = 0; e < VN; ++e)
                if (q + e < m_r) { const T v = J[(size_t)j * a.J_ld + q + e]; at[e] += v * uj; aw[e] += v * xj; }
            }
          }
#pragma unroll
          for (int e = 0; e < VN; ++e)
            if (q + e < m_r) { t[q + e] = at[e]; w[q + e] = aw[e] + (rp ? rp[q + e] : (T)0); }
        }
      }
      __syncthreads();
      if (o.dr) {
        T* d = (T*)o.dr + p * o.dr_stride;
        for (int i = tid; i < m_r; i += kThreads) d[i] = -t[i];
      }
      if (o.dJ) {
        T* d = (T*)o.dJ + p * o.dJ_stride;
        if (o.dJ_layout == MO_ROW_MAJOR) rank2_store<T>(d, o.dJ_ld, n, m_r, x, t, (T)-1, ux, w, (T)-1, vec_dJ != 0, tid);
        else rank2_store<T>(d, o.dJ_ld, m_r, n, t, x, (T)-1, w, ux, (T)-1, vec_dJ != 0, tid);
      }
    }
    if (o.dlambda && wave == 0) {
      T s = 0;
      for (int i = lane; i < n; i += 64) s += ux[i] * x[i];
      s = group_sum(s, 64);
      if (lane == 0) ((T*)o.dlambda)[p * o.dlambda_stride] = -s;
    }
    if (o.dc) {
      T* d = (T*)o.dc + p * o.dc_stride;
      for (int i = tid; i < n; i += kThreads) d[i] = -ux[i];
    }
    if (o.dG) rank2_store<T>((T*)o.dG + p * o.dG_stride, o.dG_ld, n, n, ux, x, (T)-0.5, x, ux, (T)-0.5, vec_dG != 0, tid);
    if (o.dA_eq && k > 0) rank2_store<T>((T*)o.dA_eq + p * o.dA_stride, o.dA_ld, k, n, y, ux, (T)1, uy, x, (T)-1, vec_dA != 0, tid);
    if (o.db_eq) {
      T* d = (T*)o.db_eq + p * o.db_stride;
      for (int i = tid; i < k; i += kThreads) d[i] = -uy[i];
    }
    if (o.dcons_a) {
      const int* cv = a.cons_var + p * a.cons_stride;
      T* d = (T*)o.dcons_a + p * o.dcons_stride;
      for (int i = tid; i < m; i += kThreads) {
        const int v = cv[i];
        d[i] = (v >= 0 && v < n) ? z[i] * ux[v] - uz[i] * x[v] : (T)__builtin_nan("");   // F_ASSERT qp.cc:70-72
      }
    }
    if (o.dcons_b) {
      T* d = (T*)o.dcons_b + p * o.dcons_stride;
      for (int i = tid; i < m; i += kThreads) d[i] = -uz[i];
    }
  }
}

template <typename T> size_t lds_bytes(const GradArgs& a) {
  auto pad = [](int v) { return pad16<Vec<T>::N>((size_t)v); };
  return (2 * pad(a.n) + 2 * pad(a.k) + 2 * pad(a.m) + 2 * pad(a.J ? a.m_r : 0)) * sizeof(T);
}

}  // namespace

size_t qp_grad_lds_bytes(const GradArgs& a, int elem_size) { return elem_size == 8 ? lds_bytes<double>(a) : lds_bytes<float>(a); }

hipError_t launch_qp_gradients(const GradArgs& a, int dtype, int num_cus, hipStream_t stream) {
  if (a.batch <= 0) return hipSuccess;
  const int elem = dtype == MO_F64 ? 8 : 4;
  const size_t lds = qp_grad_lds_bytes(a, elem);
  if (lds > 64 * 1024) return hipErrorInvalidValue;   // (mo_qp_gradients refuses such shapes with its own message)
  const unsigned grid = grid_for(a.batch, num_cus, 0);   // eight resident workgroups per CU, whatever the LDS
  const int vJ = vec_ok(a.J, a.J_stride, a.J_ld, elem), vdJ = vec_ok(a.out.dJ, a.out.dJ_stride, a.out.dJ_ld, elem);
  const int vdG = vec_ok(a.out.dG, a.out.dG_stride, a.out.dG_ld, elem), vdA = vec_ok(a.out.dA_eq, a.out.dA_stride, a.out.dA_ld, elem);
  if (dtype == MO_F64) hipLaunchKernelGGL(qp_grad_kernel<double>, dim3(grid), dim3(kThreads), lds, stream, a, vJ, vdJ, vdG, vdA);
  else hipLaunchKernelGGL(qp_grad_kernel<float>, dim3(grid), dim3(kThreads), lds, stream, a, vJ, vdJ, vdG, vdA);
  return hipGetLastError();
}

}  // namespace mo
