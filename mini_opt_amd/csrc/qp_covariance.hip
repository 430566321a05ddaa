// qp_covariance.hip -- mo_qp_covariance: the parameter covariance of an (equality-constrained) least-squares fit,
//   C = scale Z (Z^T S Z)^-1 Z^T,   S = sym(G) from the lower triangle, Z an orthonormal basis of null(A_eq)      (k = 0: C = scale S^-1),
// the top-left n x n block of the inverse of [[S, A^T], [A, 0]].  It is the factorisation of nullspace_kernel (kkt_generic.hip) carried one
// step further and transformed back; the QR and the reflector code are COPIES of that kernel's (its generated code is not touched), with
// its two accuracy rules: the Householder tail is summed directly (never big - c0^2), and a reflector beyond the rank transforms every row
// of the reduced block.
//
// One workgroup per problem in turn (persistent grid, static stride), everything in LDS, every step in place in the G array:
//   1. G's lower triangle -> LDS, mirrored on the way; M = A_eq^T.  A non-finite entry among those read -> MO_STATUS_NONFINITE.
//   2. pivoted Householder QR of M; rank r by Eigen's threshold |R_jj| > |R|_max eps min(n, k)
//   3. G <- Q^T G Q, reflector by reflector (two-sided rank-2 updates)
//   4. LLT of the trailing (n - r) block R = G[r.., r..]; a pivot <= 0 -> MO_STATUS_NOT_POSITIVE_DEFINITE
//   5. X = L^-1: four lanes of one wave solve L x = e_j by forward substitution (each sums every fourth term of a row's dot product, two
//      butterfly steps add them) and keep x TRANSPOSED in the strict upper triangle of R (row j), its diagonal 1 / L_jj in a vector -- no
//      wave reads what another writes, so the phase needs no barrier.  Then R.lower <- X^T X, entry
//      (i, l) = sum_{t >= i} X(t, i) X(t, l) read from the upper triangle alone (L is dead by then), one fixed summation order per entry.
//   6. mirror the lower triangle up; zero the leading r rows and columns
//   7. G <- Q G Q^T: the reflectors two-sidedly in reverse order.  The rank-2 update is written so that entry (i, l) and entry (l, i) get
//      the same two products and one sum (no contraction), which keeps the LDS matrix symmetric TO THE BIT.
//   8. out = scale * G[sel, sel], whole columns per wave; var_out reads the same LDS words as cov_out's diagonal.
// With k = 0 steps 2, 3, 6 (the zeroing) and 7 vanish.  With only var_out wanted and r = 0 step 5 forms the diagonal of X^T X alone (the
// same sums in the same order, so the same bits) and step 6 is skipped; with r > 0 the back-transform needs the whole matrix.
// Scaling: no absolute threshold touches G (the only one, the smallest normal number in makeHouseholder, is A_eq's): 4 G scales every
// square root by exactly 2 and every other quantity by a power of two, so C / 4 comes out bit for bit.
//
// LDS: G (n x n, leading dimension n | 1) | M (n x k, same leading dimension) | pv, wv (n each) | tau, nrm (k each) | sel (q ints) |
// 8 flags:   ((n | 1) (n + k) + 2 n + 2 k) sizeof(T) + 4 (q + 8) bytes <= 160 KiB.
// fp64, q = n: n = 128, k = 16 needs 151 456 B and fits (mo_nullspace_solve's own limit); every n + k <= 112 needs at most 103 520 B (n = 112, k = 0).
// The symmetric product and the back-transform run on the vector ALUs: neither is on the matrix cores yet.
#include "mo_kernels.h"

namespace mo {
namespace {

constexpr int kMaxThreads = 256;
#define kThreads ((int)blockDim.x)
#define kWaves ((int)(blockDim.x >> 6))

__host__ __device__ inline int odd_ld(int P) { return P | 1; }
__host__ __device__ inline size_t cov_elems(int n, int k) { return (size_t)odd_ld(n) * (n + k) + 2 * (size_t)n + 2 * (size_t)k; }

__device__ inline double absT(double v) { return fabs(v); }
__device__ inline float absT(float v) { return fabsf(v); }
__device__ inline double sqrtT(double v) { return sqrt(v); }
__device__ inline float sqrtT(float v) { return sqrtf(v); }
__device__ inline double fmaT(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ inline float fmaT(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
template <typename T> __device__ inline T nanT() { return (T)__builtin_nan(""); }
template <typename T> __device__ inline bool finiteT(T v) { return __builtin_isfinite(v); }
// Orders one wave's own LDS traffic: values another lane of the SAME wave stored are visible to the loads that follow.
__device__ inline void wave_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
template <typename T> __device__ inline T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// a b + c d with both products and the sum rounded on their own: sym2(a, b, c, d) == sym2(d, c, b, a) to the bit
template <typename T> __device__ inline T sym2(T a, T b, T c, T d) {
#pragma clang fp contract(off)
  const T x = a * b, y = c * d;
  return x + y;
}

template <typename T>
__global__ __launch_bounds__(kMaxThreads) void qp_covariance_kernel(const CovArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int n = a.n, k = a.k, q = a.q, ld = odd_ld(n);
  const int kq = k < n ? k : n;
  T* lp = reinterpret_cast<T*>(smem);
  T* const Gs = lp; lp += (size_t)ld * n;
  T* const Mb = lp; lp += (size_t)ld * k;
  T* const pv = lp; lp += n;    // scratch of the two-sided update; 1 / L_jj during the inversion
  T* const wv = lp; lp += n;
  T* const tau = lp; lp += k;   // Householder coefficients
  T* const nrm = lp; lp += k;   // column norms
  int* const sel = reinterpret_cast<int*>(lp);
  int* const iflag = sel + q;   // [0] non-finite input, [1] non-finite result, [4] bad index (set once)
  const auto G = [&](int i, int l) -> T& { return Gs[i + (size_t)l * ld]; };
  const auto M = [&](int i, int c) -> T& { return Mb[i + (size_t)c * ld]; };
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const T eps = sizeof(T) == 8 ? (T)2.220446049250313e-16 : (T)1.1920929e-7f;
  const T tiny = sizeof(T) == 8 ? (T)__DBL_MIN__ : (T)__FLT_MIN__;   // the smallest normal number (makeHouseholder's tol)

  if (tid < 8) iflag[tid] = 0;
  __syncthreads();
  for (int i = tid; i < q; i += kThreads) {
    const int s = a.sel ? a.sel[i] : i;
    sel[i] = s;
    if (s < 0 || s >= n) iflag[4] = 1;
  }
  __syncthreads();
  const bool bad_sel = iflag[4] != 0;
  const bool diag_only = a.cov == nullptr;

  for (long long p = blockIdx.x; p < a.batch; p += gridDim.x) {
    __syncthreads();
    if (tid < 4) iflag[tid] = 0;
    __syncthreads();
    T* const co = a.cov ? (T*)a.cov + p * a.cov_stride : nullptr;
    T* const vo = a.var ? (T*)a.var + p * a.var_stride : nullptr;
    int st = bad_sel ? MO_STATUS_BAD_INDEX : MO_STATUS_OK;
    const T sc = a.scale ? ((const T*)a.scale)[p * a.scale_stride] : (T)1;
    int rank = 0;

    if (st == MO_STATUS_OK) {
      // ---- 1. load: the lower triangle of G (mirrored), M = A_eq^T
      const T* Gp = (const T*)a.G + p * a.G_stride;
      bool bad = !finiteT(sc);
      for (int l = wave; l < n; l += kWaves)
        for (int i = l + lane; i < n; i += 64) {
          const T v = Gp[i + (size_t)l * a.G_ld];
          bad |= !finiteT(v);
          G(i, l) = v;
          G(l, i) = v;
        }
      if (k > 0) {
        const T* Ap = (const T*)a.A + p * a.A_stride;
        for (int idx = tid; idx < n * k; idx += kThreads) {
          const int i = idx / k, c = idx - i * k;
          const T v = Ap[c + (size_t)i * a.A_ld];
          bad |= !finiteT(v);
          M(i, c) = v;
        }
        for (int c = tid; c < k; c += kThreads) tau[c] = (T)0;
      }
      if (bad) iflag[0] = 1;
      __syncthreads();
      if (iflag[0]) st = MO_STATUS_NONFINITE;   // uniform
    }

    if (st == MO_STATUS_OK && k > 0) {
      // ---- 2. Householder QR of M = A_eq^T with column pivoting (the loop of nullspace_kernel; the permutation itself is not needed)
      T maxpivot = (T)0;
      for (int j = 0; j < kq; ++j) {
        for (int c = j + wave; c < k; c += kWaves) {
          T s = (T)0;
          for (int i = j + lane; i < n; i += 64) { const T v = M(i, c); s += v * v; }
          s = wave_sum(s);
          if (lane == 0) nrm[c] = s;
        }
        __syncthreads();
        int piv = j;
        T big = nrm[j];
        for (int c = j + 1; c < k; ++c) if (nrm[c] > big) { big = nrm[c]; piv = c; }   // uniform: every thread reads the same LDS values
        if (big == (T)0) break;                     // the remaining columns are exactly zero: no further reflectors
        __syncthreads();
        if (piv != j)
          for (int i = tid; i < n; i += kThreads) { const T t = M(i, j); M(i, j) = M(i, piv); M(i, piv) = t; }
        __syncthreads();
        // makeHouseholder on x = M(j.., j): beta = -sign(x0) |x|, tau = (beta - x0) / beta, essential = tail / (x0 - beta).  The tail's
        // squared norm is summed directly (big - c0^2 is 0 for a tail below sqrt(eps) |c0|, an ordinary row [1, 1e-9, ...])
        const T c0 = M(j, j);
        T beta = c0, tj = (T)0;
        T tsum = (T)0;
        for (int i = j + 1 + lane; i < n; i += 64) { const T v = M(i, j); tsum += v * v; }
        tsum = wave_sum(tsum);
        if (tsum > tiny) {
          beta = sqrtT(c0 * c0 + tsum);
          if (c0 >= (T)0) beta = -beta;
          tj = (beta - c0) / beta;
        }
        __syncthreads();
        if (tj != (T)0) {
          const T inv = (T)1 / (c0 - beta);
          for (int i = j + 1 + tid; i < n; i += kThreads) M(i, j) *= inv;
        } else {
          for (int i = j + 1 + tid; i < n; i += kThreads) M(i, j) = (T)0;
        }
        if (tid == 0) { M(j, j) = beta; tau[j] = tj; }
        __syncthreads();
        if (tj != (T)0) {
          for (int c = j + 1 + wave; c < k; c += kWaves) {   // remaining columns <- H_j columns
            T s = (T)0;
            for (int i = j + lane; i < n; i += 64) s += (i == j ? (T)1 : M(i, j)) * M(i, c);
            s = wave_sum(s) * tj;
            for (int i = j + lane; i < n; i += 64) M(i, c) -= s * (i == j ? (T)1 : M(i, j));
          }
        }
        maxpivot = absT(beta) > maxpivot ? absT(beta) : maxpivot;
        __syncthreads();
      }
      {
        const T thr = maxpivot * eps * (T)kq;
        for (int j = 0; j < kq; ++j) rank += (absT(M(j, j)) > thr) ? 1 : 0;
      }
    }

    // the two-sided application of reflector j to G on the indices >= lo: G <- H_j G H_j
    const auto two_sided = [&](int j, int lo) {
      const T tj = tau[j];
      const auto v = [&](int i) { return i < j ? (T)0 : i == j ? (T)1 : M(i, j); };
      for (int i = lo + tid; i < n; i += kThreads) {                           // p = tau G v
        T acc = (T)0;
        for (int l = j; l < n; ++l) acc += G(i, l) * v(l);
        pv[i] = acc * tj;
      }
      __syncthreads();
      if (wave == 0) {
        T s = (T)0;
        for (int i = j + lane; i < n; i += 64) s += v(i) * pv[i];
        s = wave_sum(s) * (T)0.5 * tj;                                         // alpha = tau (v^T p) / 2
        for (int i = lo + lane; i < n; i += 64) wv[i] = pv[i] - s * v(i);
      }
      __syncthreads();
      for (int l = lo + wave; l < n; l += kWaves) {                            // G -= v w^T + w v^T, symmetric to the bit
        const T vl = v(l), wl = wv[l];
        for (int i = lo + lane; i < n; i += 64) G(i, l) -= sym2(v(i), wl, vl, wv[i]);
      }
      __syncthreads();
    };

    const int q0 = rank, qn = n - rank;
    const auto R = [&](int i, int l) -> T& { return Gs[(q0 + i) + (size_t)(q0 + l) * ld]; };
    if (st == MO_STATUS_OK) {
      // ---- 3. G <- Q^T G Q on the block that still matters: indices >= j while j < rank, indices >= rank beyond
      for (int j = 0; j < kq; ++j)
        if (tau[j] != (T)0) two_sided(j, j < rank ? j : rank);                 // uniform

      // ---- 4. LLT of R = G[rank.., rank..], right-looking, lower triangle
      for (int kk = 0; kk < qn; ++kk) {
        const T d = R(kk, kk);
        if (!(d > (T)0)) { st = d == d ? MO_STATUS_NOT_POSITIVE_DEFINITE : MO_STATUS_NONFINITE; break; }   // uniform
        const T l = sqrtT(d), inv = (T)1 / l;
        __syncthreads();
        for (int i = kk + tid; i < qn; i += kThreads) R(i, kk) = i == kk ? l : R(i, kk) * inv;
        __syncthreads();
        for (int jj = kk + 1 + wave; jj < qn; jj += kWaves) {
          const T wj = R(jj, kk);
          for (int i = jj + lane; i < qn; i += 64) R(i, jj) -= R(i, kk) * wj;
        }
        __syncthreads();
      }
      __syncthreads();
    }

    const bool diag_path = diag_only && rank == 0;   // only the diagonal of X^T X is needed, and nothing transforms it afterwards
    if (st == MO_STATUS_OK) {
      // ---- 5. X = L^-1, column j by thread j, kept transposed in the strict upper triangle; then R.lower <- X^T X
      T* const dinv = pv + q0;
      for (int i = tid; i < qn; i += kThreads) dinv[i] = (T)1 / R(i, i);
      __syncthreads();
      for (int j0 = 0; j0 < qn; j0 += kThreads / 4) {                            // four lanes per column: each sums every fourth term
        const int j = j0 + (tid >> 2), r = tid & 3;
        const bool act = j < qn;
        const T xj = act ? dinv[j] : (T)0;
        for (int i = j0 + (wave << 4) + 1; i < qn; ++i) {                        // (wave-uniform bounds: the wave's first column + 1)
          T acc = (T)0;
          const bool row = act && i > j;
          if (row)
            for (int t = j + r; t < i; t += 4) acc = fmaT(R(i, t), t == j ? xj : R(j, t), acc);
          acc += __shfl_xor(acc, 1, 64);
          acc += __shfl_xor(acc, 2, 64);
          if (row && r == 0) R(j, i) = -acc / R(i, i);
          wave_lds_fence();                                                      // the next row reads x_i from the lane that stored it
        }
      }
      __syncthreads();
      if (diag_path) {
        for (int i = tid; i < qn; i += kThreads) {
          const T ui = dinv[i];
          T acc = ui * ui;
          for (int t = i + 1; t < qn; ++t) acc = fmaT(R(i, t), R(i, t), acc);
          R(i, i) = acc;
        }
      } else {
        for (int l = wave; l < qn; l += kWaves)
          for (int i = l + lane; i < qn; i += 64) {
            const T ui = dinv[i];
            T acc = ui * (i == l ? ui : R(l, i));
            for (int t = i + 1; t < qn; ++t) acc = fmaT(R(i, t), R(l, t), acc);
            R(i, l) = acc;
          }
      }
      __syncthreads();
      if (!diag_path) {
        // ---- 6. mirror the lower triangle up; zero the leading rank rows and columns
        for (int l = wave; l < n; l += kWaves)
          for (int i = lane; i <= l; i += 64) {
            if (i < q0) { G(i, l) = (T)0; G(l, i) = (T)0; }
            else G(i, l) = G(l, i);
          }
        __syncthreads();
        // ---- 7. G <- Q G Q^T: the reflectors in reverse order (rows and columns below min(j, rank) are zero and stay zero)
        if (qn > 0)
          for (int j = kq - 1; j >= 0; --j)
            if (tau[j] != (T)0) two_sided(j, j < rank ? j : rank);             // uniform
      }
      // a result that is not finite
      bool bad = false;
      if (diag_path) {
        for (int i = tid; i < n; i += kThreads) bad |= !finiteT(G(i, i) * sc);
      } else {
        for (int l = wave; l < n; l += kWaves)
          for (int i = l + lane; i < n; i += 64) bad |= !finiteT(G(i, l) * sc);
      }
      if (bad) iflag[1] = 1;
      __syncthreads();
      if (iflag[1]) st = MO_STATUS_NONFINITE;
    }

    // ---- 8. scale, gather by sel, write whole columns
    const bool ok = st == MO_STATUS_OK;
    const bool zero = qn == 0;     // rank n: C = 0 exactly, every entry +0
    if (co)
      for (int j = wave; j < q; j += kWaves) {
        const int sj = ok ? sel[j] : 0;
        for (int i = lane; i < q; i += 64) co[i + (size_t)j * a.cov_ld] = !ok ? nanT<T>() : zero ? (T)0 : sc * G(ok ? sel[i] : 0, sj);
      }
    if (vo)
      for (int i = tid; i < q; i += kThreads) {
        const int s = ok ? sel[i] : 0;
        vo[i] = !ok ? nanT<T>() : zero ? (T)0 : sc * G(s, s);
      }
    if (a.status && tid == 0) a.status[p] = st;
  }
}

}  // namespace

size_t qp_covariance_lds_bytes(int n, int k, int q, int elem_size) {
  const size_t bytes = cov_elems(n, k) * (size_t)elem_size + ((size_t)q + 8) * sizeof(int);
  return (bytes + 15) & ~(size_t)15;
}

static int cov_threads(int n, int k) { return (n + k <= 48) ? 64 : kMaxThreads; }

int qp_covariance_grid(int n, int k, int q, int elem_size, int num_cus) {
  const size_t lds = qp_covariance_lds_bytes(n, k, q, elem_size);
  const int max_per_cu = 32 / (cov_threads(n, k) / 64);
  int per_cu = (int)(kLdsBytes / (lds ? lds : 1));
  if (per_cu < 1) per_cu = 1;
  if (per_cu > max_per_cu) per_cu = max_per_cu;
  return num_cus * per_cu;
}

hipError_t launch_qp_covariance(const CovArgs& a, int dtype, int num_cus, hipStream_t stream) {
  const int elem = dtype == MO_F64 ? 8 : 4;
  const size_t lds = qp_covariance_lds_bytes(a.n, a.k, a.q, elem);
  if (lds > kLdsBytes) return hipErrorInvalidValue;
  long long grid = qp_covariance_grid(a.n, a.k, a.q, elem, num_cus);
  if (grid > a.batch) grid = a.batch;
  if (grid < 1) grid = 1;
  const int threads = cov_threads(a.n, a.k);
  hipError_t e;
  if (dtype == MO_F64) {
    e = hipFuncSetAttribute((const void*)qp_covariance_kernel<double>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((qp_covariance_kernel<double>), dim3((unsigned)grid), dim3(threads), lds, stream, a);
  } else {
    e = hipFuncSetAttribute((const void*)qp_covariance_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((qp_covariance_kernel<float>), dim3((unsigned)grid), dim3(threads), lds, stream, a);
  }
  return hipGetLastError();
}

}  // namespace mo
