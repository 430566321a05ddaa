// qp_tangent.hip -- mo_qp_tangent_rhs: the right-hand side rho = F_theta thetadot of the forward-mode system K vdot = -rho, from the state
// v = [x | s | y | z] and the tangents of the problem's data ("Forward mode").  The transpose of qp_grad.hip:
//   (G, c):   rho_d = sym(dG) x + dc - dA_eq^T y - sum_i dcons_a[i] z_i e_{var_i}
//   J-level:  rho_d = dJ^T w + J^T tdot + dlambda x - dA_eq^T y - sum_i dcons_a[i] z_i e_{var_i},   w = J x + r,  tdot = dJ x + dr
//   rho_comp = 0      rho_pe = dA_eq x + db_eq      rho_pi[i] = dcons_a[i] x[var_i] + dcons_b[i]
// Pure data movement.  One workgroup takes one problem at a time: x, y, z go to LDS, every matrix is read in its stored layout, 16 bytes per
// lane where base, leading dimension and stride allow it, and rho is assembled in LDS and written once as V contiguous values.  Two
// products cover every matrix: along the contiguous dimension (a group of lanes per vector, summed with shuffles) and across it (a lane owns
// 16 bytes of the contiguous dimension, row groups leave partial sums in LDS that ONE lane adds in a fixed order).  J and dJ are read twice
// per problem, first for the row products (w, tdot), then for the column products; the second pass finds them in the cache hierarchy.
// Every element of rho has one owner and a fixed order of operations: no atomics, the same bits on every launch.
// kThreads, Vec<T>, group_sum, pad16, vec_ok, grid_for and the constraint rows of rho (cons_rows_load / _scatter / _write, shared with
// qp_tangent_blocks.hip; here with the unit's contraction: one FMA per row of rho_pi) are in mo_sens_device.h.
#include "mo_sens_device.h"

namespace mo {
namespace {

// Which elements (l, c) of a column-major matrix (l: the contiguous index, c: the vector) take part: all of it, the lower triangle with its
// diagonal, or the strict lower triangle.  An element that takes no part is never multiplied: it may be NaN.
enum Tri : int { TRI_ALL = 0, TRI_LOWER = 1, TRI_STRICT = 2 };
template <int TRI> __device__ __forceinline__ bool tri_keep(int l, int c) { return TRI == TRI_ALL || (TRI == TRI_LOWER ? l >= c : l > c); }

// out[c] += sign * (sum_l M1[c * ld1 + l] a1[l] + M2[c * ld2 + l] a2[l])   for c < C, l < L (the contiguous dimension); M2 may be NULL.
// A vector is shared by a group of G lanes (16 bytes each per pass), 64 / G vectors per wave and pass; the group sums with shuffles and its
// first lane owns out[c].
template <typename T, int TRI>
__device__ __forceinline__ void dot_along(T* out, T sign, int L, int C, const T* M1, int ld1, bool vec1, const T* a1, const T* M2, int ld2,
                                          bool vec2, const T* a2, int tid) {
  constexpr int VN = Vec<T>::N;
  using V = typename Vec<T>::type;
  const int lane = tid & 63, wave = tid >> 6;
  const int nv = (L + VN - 1) / VN;
  int G = 1;
  while (G < nv && G < 64) G <<= 1;
  const int sub = lane / G, l = lane - sub * G, per_pass = (kThreads / 64) * (64 / G);
  for (int c0 = 0; c0 < C; c0 += per_pass) {   // (uniform bounds: every lane takes part in the shuffles)
    const int c = c0 + wave * (64 / G) + sub;
    T acc = 0;
    if (c < C) {
      const T* v1 = M1 + (size_t)c * ld1;
      const T* v2 = M2 ? M2 + (size_t)c * ld2 : nullptr;
      for (int jv = l; jv < nv; jv += G) {
        const int j = jv * VN;
        if (TRI != TRI_ALL && !tri_keep<TRI>(j + VN - 1, c)) continue;   // the whole piece lies in the excluded triangle
        if (vec1 && j + VN <= L) {
          const V v = *reinterpret_cast<const V*>(v1 + j);
          const T* ve = reinterpret_cast<const T*>(&v);
#pragma unroll
          for (int e = 0; e < VN; ++e) acc += tri_keep<TRI>(j + e, c) ? ve[e] * a1[j + e] : (T)0;
        } else {
          for (int e = 0; e < VN && j + e < L; ++e)
            if (tri_keep<TRI>(j + e, c)) acc += v1[j + e] * a1[j + e];
        }
        if (v2) {
          if (vec2 && j + VN <= L) {
            const V v = *reinterpret_cast<const V*>(v2 + j);
            const T* ve = reinterpret_cast<const T*>(&v);
#pragma unroll
            for (int e = 0; e < VN; ++e) acc += ve[e] * a2[j + e];
          } else {
            for (int e = 0; e < VN && j + e < L; ++e) acc += v2[j + e] * a2[j + e];
          }
        }
      }
    }
    acc = group_sum(acc, G);
    if (l == 0 && c < C) out[c] += sign * acc;
  }
}

// out[l] += sign * sum_c (M1[c * ld1 + l] b1[c] + M2[c * ld2 + l] b2[c])   for l < L (the contiguous dimension), c < C; M2 may be NULL.
// A lane owns VN consecutive l (16 bytes) and walks the vectors c; consecutive lanes read consecutive pieces of one vector.  With fewer than
// kThreads pieces the vectors are dealt round-robin to kThreads / pieces groups of lanes, each group leaves its partial sums in `part`
// (kThreads * VN values) and the owner of out[l] adds them in the order of the groups.  Ends with a barrier: `part` and `out` are settled.
template <typename T, int TRI>
__device__ __forceinline__ void dot_across(T* out, T sign, int L, int C, const T* M1, int ld1, bool vec1, const T* b1, const T* M2, int ld2,
                                           bool vec2, const T* b2, T* part, int tid) {
  constexpr int VN = Vec<T>::N;
  using V = typename Vec<T>::type;
  const int P = (L + VN - 1) / VN;
  int Gr = P >= kThreads ? 1 : kThreads / P;
  if (Gr > C) Gr = C > 0 ? C : 1;
  for (int it = tid; it < P * Gr; it += kThreads) {
    const int g = it / P, l0 = (it - g * P) * VN;
    T acc[VN];
#pragma unroll
    for (int e = 0; e < VN; ++e) acc[e] = 0;
    const bool full = l0 + VN <= L;
#pragma unroll 4
    for (int c = g; c < C; c += Gr) {
      if (TRI != TRI_ALL && !tri_keep<TRI>(l0 + VN - 1, c)) continue;   // the whole piece lies in the excluded triangle
      const T bc = b1[c];
      if (vec1 && full) {
        const V v = *reinterpret_cast<const V*>(M1 + (size_t)c * ld1 + l0);
        const T* ve = reinterpret_cast<const T*>(&v);
#pragma unroll
        for (int e = 0; e < VN; ++e) acc[e] += tri_keep<TRI>(l0 + e, c) ? ve[e] * bc : (T)0;
      } else {
#pragma unroll
        for (int e = 0; e < VN; ++e)
          if (l0 + e < L && tri_keep<TRI>(l0 + e, c)) acc[e] += M1[(size_t)c * ld1 + l0 + e] * bc;
      }
      if (M2) {
        const T b2c = b2[c];
        if (vec2 && full) {
          const V v = *reinterpret_cast<const V*>(M2 + (size_t)c * ld2 + l0);
          const T* ve = reinterpret_cast<const T*>(&v);
#pragma unroll
          for (int e = 0; e < VN; ++e) acc[e] += ve[e] * b2c;
        } else {
#pragma unroll
          for (int e = 0; e < VN; ++e)
            if (l0 + e < L) acc[e] += M2[(size_t)c * ld2 + l0 + e] * b2c;
        }
      }
    }
    if (Gr == 1) {
#pragma unroll
      for (int e = 0; e < VN; ++e)
        if (l0 + e < L) out[l0 + e] += sign * acc[e];
    } else {   // (P * Gr <= kThreads: one item per lane, part holds Gr rows of P * VN values)
#pragma unroll
      for (int e = 0; e < VN; ++e) part[(size_t)g * P * VN + l0 + e] = acc[e];
    }
  }
  __syncthreads();
  if (Gr > 1) {
    for (int l = tid; l < L; l += kThreads) {
      T s = 0;
      for (int g = 0; g < Gr; ++g) s += part[(size_t)g * P * VN + l];
      out[l] += sign * s;
    }
    __syncthreads();
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void qp_tangent_kernel(const TangentArgs a, const int vec_J, const int vec_dJ, const int vec_dG,
                                                              const int vec_dA) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int VN = Vec<T>::N;
  const int n = a.n, k = a.k, m = a.m, m_r = a.J ? a.m_r : 0;
  // every vector starts on a 16-byte boundary
  const int n_p = pad16<VN>(n), k_p = pad16<VN>(k), m_p = pad16<VN>(m), r_p = pad16<VN>(m_r);
  T* x = reinterpret_cast<T*>(smem);
  T* y = x + n_p;
  T* az = y + k_p;     // dcons_a[i] z_i
  T* w = az + m_p;     // J x + r
  T* td = w + r_p;     // dJ x + dr
  T* rd = td + r_p;    // rho_d
  T* pe = rd + n_p;    // rho_pe
  T* part = pe + k_p;  // partial sums of dot_across
  int* cv = reinterpret_cast<int*>(part + kThreads * VN);   // cons_var, -1 for an index outside [0, n)
  const int tid = threadIdx.x;
  const mo_qp_tangents& t = a.t;
  const bool cons = m > 0 && t.dcons_a != nullptr;

  for (long long p = blockIdx.x; p < a.batch; p += gridDim.x) {
    const T* vp = (const T*)a.vars + p * a.vars_stride;
    T* rho = (T*)a.rho + p * a.rho_stride;
    const T* dc = t.dc ? (const T*)t.dc + p * t.dc_stride : nullptr;
    const T dlam = t.dlambda ? ((const T*)t.dlambda)[p * t.dlambda_stride] : (T)0;
    const int* cvp = a.cons_var ? a.cons_var + p * a.cons_stride : nullptr;
    const T* dca = cons ? (const T*)t.dcons_a + p * t.dcons_stride : nullptr;
    const T* dcb = (m > 0 && t.dcons_b) ? (const T*)t.dcons_b + p * t.dcons_stride : nullptr;
    __syncthreads();  // the previous problem's readers are done with the LDS
    for (int i = tid; i < n; i += kThreads) {
      const T xi = vp[i];
      x[i] = xi;
      rd[i] = (dc ? dc[i] : (T)0) + dlam * xi;
    }
    if (k > 0) {
      const T* db = t.db_eq ? (const T*)t.db_eq + p * t.db_stride : nullptr;
      for (int i = tid; i < k; i += kThreads) { y[i] = vp[n + m + i]; pe[i] = db ? db[i] : (T)0; }
    }
    cons_rows_load(cv, az, cvp, dca, vp, n + m + k, n, m, tid);
    if (m_r > 0) {
      const T* rp = a.r ? (const T*)a.r + p * a.r_stride : nullptr;
      const T* dr = t.dr ? (const T*)t.dr + p * t.dr_stride : nullptr;
      for (int i = tid; i < m_r; i += kThreads) { w[i] = rp ? rp[i] : (T)0; td[i] = dr ? dr[i] : (T)0; }
    }
    __syncthreads();

    if (m_r > 0) {
      const T* J = (const T*)a.J + p * a.J_stride;
      const T* dJ = t.dJ ? (const T*)t.dJ + p * t.dJ_stride : nullptr;
      if (a.J_row_major) {
        // rows are contiguous: w, tdot along them, then the column products across them
        if (dJ) {
          dot_along<T, TRI_ALL>(w, (T)1, n, m_r, J, a.J_ld, vec_J != 0, x, nullptr, 0, false, nullptr, tid);
          dot_along<T, TRI_ALL>(td, (T)1, n, m_r, dJ, t.dJ_ld, vec_dJ != 0, x, nullptr, 0, false, nullptr, tid);
          __syncthreads();
          dot_across<T, TRI_ALL>(rd, (T)1, n, m_r, dJ, t.dJ_ld, vec_dJ != 0, w, J, a.J_ld, vec_J != 0, td, part, tid);
        } else {
          dot_across<T, TRI_ALL>(rd, (T)1, n, m_r, J, a.J_ld, vec_J != 0, td, nullptr, 0, false, nullptr, part, tid);
        }
      } else {
        // columns are contiguous: w, tdot across them, then the column products along them
        if (dJ) {
          dot_across<T, TRI_ALL>(w, (T)1, m_r, n, J, a.J_ld, vec_J != 0, x, nullptr, 0, false, nullptr, part, tid);
          dot_across<T, TRI_ALL>(td, (T)1, m_r, n, dJ, t.dJ_ld, vec_dJ != 0, x, nullptr, 0, false, nullptr, part, tid);
          dot_along<T, TRI_ALL>(rd, (T)1, m_r, n, dJ, t.dJ_ld, vec_dJ != 0, w, J, a.J_ld, vec_J != 0, td, tid);
        } else {
          dot_along<T, TRI_ALL>(rd, (T)1, m_r, n, J, a.J_ld, vec_J != 0, td, nullptr, 0, false, nullptr, tid);
        }
        __syncthreads();
      }
    }
    if (t.dG) {
      // sym(dG) x from the lower triangle alone: column j gives dG[i, j] x_j to row i >= j (across) and dG[i, j] x_i to row j < i (along)
      const T* dG = (const T*)t.dG + p * t.dG_stride;
      dot_across<T, TRI_LOWER>(rd, (T)1, n, n, dG, t.dG_ld, vec_dG != 0, x, nullptr, 0, false, nullptr, part, tid);
      dot_along<T, TRI_STRICT>(rd, (T)1, n, n, dG, t.dG_ld, vec_dG != 0, x, nullptr, 0, false, nullptr, tid);
      __syncthreads();
    }
    if (k > 0 && t.dA_eq) {
      const T* dA = (const T*)t.dA_eq + p * t.dA_stride;
      dot_along<T, TRI_ALL>(rd, (T)-1, k, n, dA, t.dA_ld, vec_dA != 0, y, nullptr, 0, false, nullptr, tid);   // -dA_eq^T y
      dot_across<T, TRI_ALL>(pe, (T)1, k, n, dA, t.dA_ld, vec_dA != 0, x, nullptr, 0, false, nullptr, part, tid);   // dA_eq x (ends with a barrier)
    }
    // rho_d[var_i] -= dcons_a[i] z_i: the owner of variable j walks the rows in their order, however many name j
    if (cons) {
      cons_rows_scatter(rd, cv, az, n, m, tid);
      __syncthreads();
    }
    for (int i = tid; i < n; i += kThreads) rho[i] = rd[i];
    cons_rows_write<T, true>(rho, n, n + m + k, cv, dca, dcb, x, m, tid);   // (one FMA per row: the unit's contraction)
    for (int i = tid; i < k; i += kThreads) rho[n + m + i] = pe[i];
  }
}

template <typename T> size_t lds_bytes(const TangentArgs& a) {
  auto pad = [](int v) { return pad16<Vec<T>::N>((size_t)v); };
  return (2 * pad(a.n) + 2 * pad(a.k) + pad(a.m) + 2 * pad(a.J ? a.m_r : 0) + kThreads * Vec<T>::N) * sizeof(T) + (size_t)a.m * sizeof(int);
}

}  // namespace

size_t qp_tangent_lds_bytes(const TangentArgs& a, int elem_size) { return elem_size == 8 ? lds_bytes<double>(a) : lds_bytes<float>(a); }

hipError_t launch_qp_tangent(const TangentArgs& a, int dtype, int num_cus, hipStream_t stream) {
  if (a.batch <= 0) return hipSuccess;
  const int elem = dtype == MO_F64 ? 8 : 4;
  const size_t lds = qp_tangent_lds_bytes(a, elem);
  if (lds > 64 * 1024) return hipErrorInvalidValue;   // (mo_qp_tangent_rhs refuses such shapes with its own message)
  const unsigned grid = grid_for(a.batch, num_cus, 0);   // eight resident workgroups per CU, as the gradient kernel
  const int vJ = vec_ok(a.J, a.J_stride, a.J_ld, elem), vdJ = vec_ok(a.t.dJ, a.t.dJ_stride, a.t.dJ_ld, elem);
  const int vdG = vec_ok(a.t.dG, a.t.dG_stride, a.t.dG_ld, elem), vdA = vec_ok(a.t.dA_eq, a.t.dA_stride, a.t.dA_ld, elem);
  if (dtype == MO_F64) hipLaunchKernelGGL(qp_tangent_kernel<double>, dim3(grid), dim3(kThreads), lds, stream, a, vJ, vdJ, vdG, vdA);
  else hipLaunchKernelGGL(qp_tangent_kernel<float>, dim3(grid), dim3(kThreads), lds, stream, a, vJ, vdJ, vdG, vdA);
  return hipGetLastError();
}

}  // namespace mo
