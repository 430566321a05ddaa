// residual_blocks.hip -- the cost and equality halves of LinearizeAndFillQP (nonlinear.cc:182-206) for residual-BLOCK input: every
// residual is an R_b x P_b column-major local Jacobian over an index list of P_b of the n variables (Residual::Model, residual.hpp:60-143).
//   blocks_linearize_kernel   sum_b UpdateHessian (residual.hpp:186-226) + lambda I: G (lower, strict upper 0), c, 0.5 |r|^2
//   blocks_jacobian_kernel    UpdateJacobian stacked (residual.hpp:230-250): the dense (sum R_b) x n matrix, |r|_1
//   blocks_grad_kernel        the transpose of the first gather applied to (x, u_x): dJ_blocks, dr, dlambda (mo_qp_gradients_blocks)
//   blocks_eq_grad_kernel     the transpose of the second: dJ_eq_blocks, dr_eq (mo_qp_gradients_eq_blocks)
// Gather formulation: mo_residual_layout_create lists, for every cell of G and every entry of c, its contributions
// in the reference's order (blocks in order, then row_local / col_local).  A lane owns one cell at a time and sums its list in that order,
// so there are no atomics, no G accumulator and the result is the same on every launch.  The schedule is shared by the batch: it stays in
// L2 while the workgroups stream their problems' packed J and r (through LDS when they fit) and write whole lines of G.
// kThreads and grid_for (the grid of the persistent workgroups) are those of every sensitivity kernel: mo_sens_device.h.
#include "mo_loss_device.h"

namespace mo {
namespace {

constexpr size_t kStageBudget = 48 * 1024;  // per workgroup: above it the packed values are read straight from global memory
constexpr size_t kGradLds = 63 * 1024;      // blocks_grad_kernel: the vectors it always keeps in LDS (x, u_x, t, w) and, staged, the values on top

template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// sum over the workgroup, valid in thread 0; `red` holds one value per wave
template <typename T> __device__ __forceinline__ T block_sum(T v, T* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  T s = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kThreads / 64; ++w) s += red[w];
  return s;
}

// kW (mo_linearize_blocks_weighted): row rho of a block counts with its weight, G += w J_a J_b, c += w J_a r, half_sq += w r^2, each as
// (w J_a) * (.) in the order of the unweighted sums -- with w = 1 the same operations, with w a power of four the bits of the call on
// (sqrt(w) J, sqrt(w) r).  A row whose weight is exactly 0 is skipped: its J values and r are never multiplied (they may be NaN).
// kL (mo_linearize_blocks_robust; staged and kW only): no weights are read.  Once r is staged a lane per block forms s_b, w_b = rho'(s_b) and
// rho_b (mo_loss_device.h, the code of mo_residual_loss_eval), writes w_b over the block's rows of sW (and of weights_out when given) and the
// kernel goes on as kW; half_sq_out receives 0.5 sum rho in the order of the stand-alone kernel.
template <typename T, bool kStaged, bool kW = false, bool kL = false>
__global__ __launch_bounds__(kThreads) void blocks_linearize_kernel(const BlocksArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ T red[kThreads / 64];
  T* sJ = reinterpret_cast<T*>(smem);
  T* sR = sJ + a.values;
  T* sW = sR + a.rows;   // kW, staged: the weights
  const int tid = threadIdx.x;
  const int n = a.n, nn = n * n;
  for (long long p = blockIdx.x; p < a.batch; p += gridDim.x) {
    const T* gJ = (const T*)a.J + p * a.J_stride;
    const T* gR = (const T*)a.r + p * a.r_stride;
    const T* Jv = gJ;
    const T* rv = gR;
    const T* wv = (kW && !kL) ? (const T*)a.weights + p * a.weights_stride : nullptr;
    T rho_part = 0;
    if (kStaged) {
      for (long long i = tid; i < a.values; i += kThreads) sJ[i] = gJ[i];
      for (int i = tid; i < a.rows; i += kThreads) sR[i] = gR[i];
      if (kL) {
        __syncthreads();  // r is staged
        rho_part = loss_blocks<T>(a.loss_blk, (const T*)a.loss_scale, a.loss_blocks, sR, sW,
                                  a.weights_out ? (T*)a.weights_out + p * a.weights_out_stride : nullptr, tid);
        wv = sW;
      } else if (kW) {
        for (int i = tid; i < a.rows; i += kThreads) sW[i] = wv[i];
        wv = sW;
      }
      __syncthreads();
      Jv = sJ;
      rv = sR;
    }
    const T lam = a.lambda_vec ? ((const T*)a.lambda_vec)[p * a.lambda_vec_stride] : (T)a.lambda;
    T* G = (T*)a.G_out + p * a.G_out_stride;
    // consecutive lanes own consecutive cells of G's column-major order: whole-line stores when G_ld == n.  (G_out NULL: c and half_sq only)
    for (int cell = tid; a.G_out && cell < nn; cell += kThreads) {
      const int col = cell / n, row = cell - col * n;
      const int e1 = a.g_ptr[cell + 1];
      T s = 0;
      for (int e = a.g_ptr[cell]; e < e1; ++e) {
        const int4 c = a.g_ent[e];
        T d = 0;
        if (kW) {
          for (int q = 0; q < c.z; ++q) {
            const T w = wv[c.w + q];
            if (w != (T)0) {
              const T wa = w * Jv[c.x + q];
              d += wa * Jv[c.y + q];
            }
          }
        } else {
          for (int q = 0; q < c.z; ++q) d += Jv[c.x + q] * Jv[c.y + q];
        }
        s += d;
      }
      if (row == col && lam > (T)0) s += lam;  // nonlinear.cc:187-189, after the sum
      G[(size_t)col * a.G_out_ld + row] = s;
    }
    T* cv = (T*)a.c_out + p * a.c_out_stride;
    for (int i = tid; i < n; i += kThreads) {
      const int e1 = a.c_ptr[i + 1];
      T s = 0;
      for (int e = a.c_ptr[i]; e < e1; ++e) {
        const int4 c = a.c_ent[e];
        T d = 0;
        if (kW) {
          for (int q = 0; q < c.z; ++q) {
            const T w = wv[c.y + q];
            if (w != (T)0) {
              const T wa = w * Jv[c.x + q];
              d += wa * rv[c.y + q];
            }
          }
        } else {
          for (int q = 0; q < c.z; ++q) d += Jv[c.x + q] * rv[c.y + q];
        }
        s += d;
      }
      cv[i] = s;
    }
    if (a.half_sq_out) {
      T sq = 0;
      if (kL) {
        sq = loss_rho_sum(rho_part, red);
        if (tid == 0) ((T*)a.half_sq_out)[p * a.half_sq_stride] = (T)0.5 * sq;
      } else if (kW) {
        for (int i = tid; i < a.rows; i += kThreads) {
          const T w = wv[i];
          if (w != (T)0) {
            const T wr = w * rv[i];
            sq += wr * rv[i];
          }
        }
      } else {
        for (int i = tid; i < a.rows; i += kThreads) sq += rv[i] * rv[i];
      }
      if (!kL) {
        sq = block_sum(sq, red);
        if (tid == 0) ((T*)a.half_sq_out)[p] = (T)0.5 * sq;
      }
    }
    __syncthreads();  // the next problem overwrites the staged values and the reduction slots
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void blocks_jacobian_kernel(const BlocksArgs a) {
  __shared__ T red[kThreads / 64];
  const int tid = threadIdx.x;
  const int n = a.n, rows = a.rows, total = rows * n;
  for (long long p = blockIdx.x; p < a.batch; p += gridDim.x) {
    const T* J = (const T*)a.J + p * a.J_stride;
    T* out = (T*)a.J_out + p * a.J_out_stride;
    // consecutive lanes own consecutive elements of the output's own order (down a column, or along a row)
    for (int e = tid; e < total; e += kThreads) {
      int row, col;
      if (a.J_out_row_major) { row = e / n; col = e - row * n; }
      else { col = e / rows; row = e - col * rows; }
      const int2 ri = a.row_info[row];
      const int w = a.win[ri.x + col];
      const T v = w >= 0 ? J[w + ri.y] : (T)0;
      if (a.J_out_row_major) out[(size_t)row * a.J_out_ld + col] = v;
      else out[(size_t)col * a.J_out_ld + row] = v;
    }
    if (a.abs_sum_out) {  // Errors::equality, nonlinear.cc:204
      const T* r = (const T*)a.r + p * a.r_stride;
      T s = 0;
      for (int i = tid; i < rows; i += kThreads) s += fabs(r[i]);
      s = block_sum(s, red);
      if (tid == 0) ((T*)a.abs_sum_out)[p] = s;
      __syncthreads();
    }
  }
}

// mo_qp_gradients_blocks (the formulas: include/mini_opt_hip.h).  The same hand-out as blocks_linearize_kernel.  Phase 1: a lane owns a stacked
// residual row (b, q) and walks the block's P_b columns in order: t = J_b x_loc + r_b, w = J_b u_loc, into LDS; dr = -w.  Phase 2: consecutive
// lanes own consecutive packed values (column-major inside a block: whole-line stores), dJ = -u_p t[q] - x_p w[q] plus (u_p x_p) J_b[q, q'] for
// every other local column q' on the same variable.  Every product is rounded before it is added.
// kW (mo_qp_gradients_blocks_weighted): the weights go to LDS beside t and w; dJ = weight x (the value above), dr = -weight x w, both exactly 0
// at a row whose weight is exactly 0, whatever its data hold; dweights[row] = -w[row] t[row] + sum over the pairs {p, p'} of local columns of
// the row's block on one variable i of (u_i x_i) J[row, p] J[row, p'] (d_pair / d_plist of the layout; no list for almost every block).
template <typename T, bool kStaged, bool kW = false>
__global__ __launch_bounds__(kThreads) void blocks_grad_kernel(const BlockGradArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ T red[kThreads / 64];
  T* sx = reinterpret_cast<T*>(smem);
  T* su = sx + a.n;
  T* st = su + a.n;
  T* sw = st + a.rows;
  T* sg = sw + a.rows;   // kW: the weights
  T* sJ = sg + (kW ? a.rows : 0);
  T* sR = sJ + a.values;
  const int tid = threadIdx.x;
  const int n = a.n, rows = a.rows;
  const bool need_rows = a.dJ || a.dr || (kW && a.dw);
  for (long long p = blockIdx.x; p < a.batch; p += gridDim.x) {
    const T* vp = (const T*)a.vars + p * a.vars_stride;
    const T* up = (const T*)a.u + p * a.u_stride;
    const T* Jv = (const T*)a.J + p * a.J_stride;
    const T* rv = (const T*)a.r + p * a.r_stride;
    for (int i = tid; i < n; i += kThreads) { sx[i] = vp[i]; su[i] = up[i]; }
    if (kStaged && need_rows) {
      for (long long i = tid; i < a.values; i += kThreads) sJ[i] = Jv[i];
      for (int i = tid; i < rows; i += kThreads) sR[i] = rv[i];
      Jv = sJ;
      rv = sR;
    }
    __syncthreads();
    if (need_rows) {
      T* dr = a.dr ? (T*)a.dr + p * a.dr_stride : nullptr;
      const T* wv = kW ? (const T*)a.weights + p * a.weights_stride : nullptr;
      T* dw = (kW && a.dw) ? (T*)a.dw + p * a.dw_stride : nullptr;
      for (int row = tid; row < rows; row += kThreads) {
        const int4 ri = a.d_row[row];
        T t = 0, w = 0;
        for (int c = 0; c < ri.z; ++c) {
          const int g = a.d_idx[ri.w + c];
          const T v = Jv[ri.x + c * ri.y];
          const T tx = v * sx[g], tu = v * su[g];
          t += tx;
          w += tu;
        }
        st[row] = t + rv[row];
        sw[row] = w;
        if (kW) {
          const T g = wv[row];
          sg[row] = g;
          if (dr) {
            const T gw = g * w;
            dr[row] = g == (T)0 ? (T)0 : -gw;
          }
          if (dw) {
            const T wt = w * st[row];
            T s = -wt;
            const int pl = a.d_pair[row];
            if (pl >= 0) {  // a repeated variable inside the block: the derivative of the pair that landed once
              const int cnt = a.d_plist[pl];
              for (int d = 0; d < cnt; ++d) {
                const int ca = a.d_plist[pl + 1 + 3 * d], cb = a.d_plist[pl + 2 + 3 * d], gi = a.d_plist[pl + 3 + 3 * d];
                const T ux = su[gi] * sx[gi];
                const T jj = Jv[ri.x + ca] * Jv[ri.x + cb];
                const T pd = ux * jj;
                s += pd;
              }
            }
            dw[row] = s;
          }
        } else if (dr) dr[row] = -w;
      }
      __syncthreads();
      if (a.dJ) {
        T* dJ = (T*)a.dJ + p * a.dJ_stride;
        for (long long e = tid; e < a.values; e += kThreads) {
          const int4 vi = a.d_val[e];
          const T ug = su[vi.y], xg = sx[vi.y];
          const T p1 = ug * st[vi.x], p2 = xg * sw[vi.x];
          T s = -p1 - p2;
          if (vi.w >= 0) {  // a repeated variable inside the block: the pair landed once, on the diagonal
            const T ux = ug * xg;
            const int cnt = a.d_dup[vi.w];
            for (int d = 1; d <= cnt; ++d) {
              const T pd = ux * Jv[a.d_dup[vi.w + d] + vi.z];
              s += pd;
            }
          }
          if (kW) {
            const T g = sg[vi.x];
            const T gs = g * s;
            s = g == (T)0 ? (T)0 : gs;
          }
          dJ[e] = s;
        }
      }
    }
    if (a.dlambda) {
      T s = 0;
      for (int i = tid; i < n; i += kThreads) {
        const T pr = su[i] * sx[i];
        s += pr;
      }
      s = block_sum(s, red);
      if (tid == 0) ((T*)a.dlambda)[p * a.dlambda_stride] = -s;
    }
    __syncthreads();  // the next problem overwrites the staged values, the vectors and the reduction slots
  }
}

// mo_qp_gradients_eq_blocks: consecutive lanes own consecutive packed equality values; a column that lost its global column gets exactly 0
template <typename T>
__global__ __launch_bounds__(kThreads) void blocks_eq_grad_kernel(const BlockGradArgs a) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const int yo = a.n + a.m;  // v = [x | s | y | z]
  for (long long p = blockIdx.x; p < a.batch; p += gridDim.x) {
    const T* vp = (const T*)a.vars + p * a.vars_stride;
    const T* up = (const T*)a.u + p * a.u_stride;
    if (a.dJ) {
      T* dJ = (T*)a.dJ + p * a.dJ_stride;
      for (long long e = tid; e < a.values; e += kThreads) {
        const int2 vi = a.e_val[e];
        T s = 0;
        if (vi.y >= 0) {
          const T p1 = vp[yo + vi.x] * up[vi.y], p2 = up[yo + vi.x] * vp[vi.y];
          s = p1 - p2;
        }
        dJ[e] = s;
      }
    }
    if (a.dr) {
      T* dr = (T*)a.dr + p * a.dr_stride;
      for (int i = tid; i < a.rows; i += kThreads) dr[i] = -up[yo + i];
    }
  }
}

template <typename T> hipError_t launch_linearize_t(const BlocksArgs& a, int num_cus, hipStream_t stream) {
  if (a.loss_blk) {  // the weights are formed in LDS: staged layouts only (mo_linearize_blocks_robust takes the two-launch route otherwise)
    const size_t stage = (size_t)(a.values + 2 * (long long)a.rows) * sizeof(T);
    if (stage > kStageBudget) return hipErrorInvalidValue;
    hipLaunchKernelGGL((blocks_linearize_kernel<T, true, true, true>), dim3(grid_for(a.batch, num_cus, stage)), dim3(kThreads), stage, stream, a);
    return hipGetLastError();
  }
  if (a.weights) {  // the weights are staged with the values: rows more elements
    const size_t stage = (size_t)(a.values + 2 * (long long)a.rows) * sizeof(T);
    if (stage <= kStageBudget) {
      hipLaunchKernelGGL((blocks_linearize_kernel<T, true, true>), dim3(grid_for(a.batch, num_cus, stage)), dim3(kThreads), stage, stream, a);
    } else {
      hipLaunchKernelGGL((blocks_linearize_kernel<T, false, true>), dim3(grid_for(a.batch, num_cus, 0)), dim3(kThreads), 0, stream, a);
    }
    return hipGetLastError();
  }
  const size_t stage = (size_t)(a.values + a.rows) * sizeof(T);
  if (stage <= kStageBudget) {
    hipLaunchKernelGGL((blocks_linearize_kernel<T, true>), dim3(grid_for(a.batch, num_cus, stage)), dim3(kThreads), stage, stream, a);
  } else {
    hipLaunchKernelGGL((blocks_linearize_kernel<T, false>), dim3(grid_for(a.batch, num_cus, 0)), dim3(kThreads), 0, stream, a);
  }
  return hipGetLastError();
}

template <typename T> hipError_t launch_grad_t(const BlockGradArgs& a, int num_cus, hipStream_t stream) {
  if (a.weights) {
    const size_t vectors = (size_t)(2 * a.n + 3 * a.rows) * sizeof(T);
    const size_t stage = (size_t)(a.values + a.rows) * sizeof(T);
    if (stage <= kStageBudget && vectors + stage <= kGradLds) {
      hipLaunchKernelGGL((blocks_grad_kernel<T, true, true>), dim3(grid_for(a.batch, num_cus, vectors + stage)), dim3(kThreads), vectors + stage, stream, a);
    } else {
      hipLaunchKernelGGL((blocks_grad_kernel<T, false, true>), dim3(grid_for(a.batch, num_cus, vectors)), dim3(kThreads), vectors, stream, a);
    }
    return hipGetLastError();
  }
  const size_t vectors = (size_t)(2 * a.n + 2 * a.rows) * sizeof(T);
  const size_t stage = (size_t)(a.values + a.rows) * sizeof(T);
  if (stage <= kStageBudget && vectors + stage <= kGradLds) {
    hipLaunchKernelGGL((blocks_grad_kernel<T, true>), dim3(grid_for(a.batch, num_cus, vectors + stage)), dim3(kThreads), vectors + stage, stream, a);
  } else {
    hipLaunchKernelGGL((blocks_grad_kernel<T, false>), dim3(grid_for(a.batch, num_cus, vectors)), dim3(kThreads), vectors, stream, a);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_blocks_linearize(const BlocksArgs& a, int dtype, int num_cus, hipStream_t stream) {
  if (a.batch <= 0) return hipSuccess;
  return dtype == MO_F64 ? launch_linearize_t<double>(a, num_cus, stream) : launch_linearize_t<float>(a, num_cus, stream);
}

hipError_t launch_blocks_jacobian(const BlocksArgs& a, int dtype, int num_cus, hipStream_t stream) {
  if (a.batch <= 0) return hipSuccess;
  const dim3 g(grid_for(a.batch, num_cus, 0)), b(kThreads);
  if (dtype == MO_F64) hipLaunchKernelGGL(blocks_jacobian_kernel<double>, g, b, 0, stream, a);
  else hipLaunchKernelGGL(blocks_jacobian_kernel<float>, g, b, 0, stream, a);
  return hipGetLastError();
}

bool blocks_weighted_stages(long long values, int rows, int elem_size) {
  return (size_t)(values + 2 * (long long)rows) * elem_size <= kStageBudget;
}

bool blocks_grad_fits(int n, int rows, int elem_size, bool weighted) {
  return (size_t)(2 * (long long)n + (weighted ? 3 : 2) * (long long)rows) * elem_size <= kGradLds;
}

hipError_t launch_blocks_grad(const BlockGradArgs& a, int dtype, int num_cus, hipStream_t stream) {
  if (a.batch <= 0) return hipSuccess;
  if (!blocks_grad_fits(a.n, a.rows, dtype == MO_F64 ? 8 : 4, a.weights != nullptr)) return hipErrorInvalidValue;  // (mo_qp_gradients_blocks refuses with its own message)
  return dtype == MO_F64 ? launch_grad_t<double>(a, num_cus, stream) : launch_grad_t<float>(a, num_cus, stream);
}

hipError_t launch_blocks_eq_grad(const BlockGradArgs& a, int dtype, int num_cus, hipStream_t stream) {
  if (a.batch <= 0) return hipSuccess;
  const dim3 g(grid_for(a.batch, num_cus, 0)), b(kThreads);
  if (dtype == MO_F64) hipLaunchKernelGGL(blocks_eq_grad_kernel<double>, g, b, 0, stream, a);
  else hipLaunchKernelGGL(blocks_eq_grad_kernel<float>, g, b, 0, stream, a);
  return hipGetLastError();
}

}  // namespace mo
