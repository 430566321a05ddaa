// qp_tangent_blocks.hip -- mo_qp_tangent_rhs_blocks: the right-hand side rho = F_theta thetadot of the forward-mode system K vdot = -rho for
// RESIDUAL-BLOCK input, from the state v = [x | s | y | z] and the PACKED tangents of the blocks (the formulas: include/mini_opt_hip.h;
// DESIGN.md section 4.8, "Forward mode, block input").  The transpose of blocks_grad_kernel / blocks_eq_grad_kernel (residual_blocks.hip):
//   rho_d[i]    = dlambda x_i + sum over the local columns p on i of (dJ_b[:, p] . t_b + J_b[:, p] . tdot_b - x_i sum_q' dJ_b[:, p] . J_b[:, q'])
//                 - sum over the WINNING equality columns on i of dJeq_b[:, a] . y_b - sum_i' dcons_a[i'] z_i' [var_i' = i]
//   rho_pe[row] = dr_eq[row] + sum over the winning columns a of the row's block of dJeq_b[q, a] x[idx_b[a]]
//   rho_comp = 0      rho_pi[i] = dcons_a[i] x[var_i] + dcons_b[i]
// with t_b = J_b x_loc + r_b, tdot_b = dJ_b x_loc + dr_b and q' the OTHER local columns of block b on p's variable.  No n x n and no rows x n
// matrix is formed.  One workgroup takes one problem at a time.  Phase 1: x, y, dcons_a z to LDS, rho_d = dlambda x, rho_pe = dr_eq.  Phase 2:
// a lane owns a stacked cost row and walks its block's columns (phase 1 of blocks_grad_kernel): t, tdot to LDS.  Phase 3: a group of kW
// lanes owns variable i and walks its contribution list in the layout's order (c_ptr / c_ent of the cost layout, the winners' list of the
// equality layout), lane l taking the entries l, l + kW, ...; the partial sums are added in a shuffle tree of fixed shape.  Phase 4: the owner
// of rho_pe[row] walks the winners among its block's columns.  Phase 5: the owner of variable j walks the constraint rows in order.  Phase 6:
// rho is written once, V contiguous values.  Every element has one owner and a fixed order of operations, every product is rounded before
// it is added: no atomics, the same bits on every launch.  Phases 1, 5 and 6 share their constraint rows with qp_tangent.hip (cons_rows_load /
// _scatter / _write of mo_sens_device.h, here with kContract = false); kThreads, group_sum and grid_for come from there as well.
#include <stdlib.h>

#include "mo_sens_device.h"

namespace mo {
namespace {

constexpr size_t kStageBudget = 48 * 1024;  // per workgroup: above it the packed values and tangents are read straight from global memory
constexpr size_t kTangentLds = 64 * 1024;   // the vectors the kernel always keeps in LDS and, staged, the values on top

// kW (mo_qp_tangent_rhs_blocks_weighted): Gdot = sum_b (dJ^T W J + J^T W dJ + J^T Wdot J), cdot = sum_b (dJ^T W r + J^T Wdot r + J^T W dr).
// Phase 2 keeps the weights in LDS and stores  t := w t  and  tdot := w tdot + wdot t  per stacked row, so that phase 3 is the unweighted walk;
// a row whose two values are exactly 0 (weight 0, no direction in it) is skipped there, whatever its J and dJ hold.  The repeated-variable
// correction carries the row's weight, and for the pair's derivative along wdot each pair is taken once (the partner behind the column).
template <typename T, bool kStaged, bool kW = false>
__global__ __launch_bounds__(kThreads) void blocks_tangent_kernel(const BlockTangentArgs a, const int width) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char smem[];
  const int n = a.n, k = a.k, m = a.m, rows = a.rows;
  T* sx = reinterpret_cast<T*>(smem);
  T* sy = sx + n;
  T* saz = sy + k;      // dcons_a[i] z_i
  T* st = saz + m;      // t = J x_loc + r
  T* std_ = st + rows;  // tdot = dJ x_loc + dr
  T* srd = std_ + rows; // rho_d
  T* spe = srd + n;     // rho_pe
  T* sg = spe + k;      // kW: the weights
  T* sJ = sg + (kW ? rows : 0);   // staged: J_blocks, dJ_blocks, r, dr
  T* sdJ = sJ + (kStaged ? a.values : 0);
  T* sR = sdJ + (kStaged ? a.values : 0);
  T* sdR = sR + (kStaged ? rows : 0);
  int* scv = reinterpret_cast<int*>(sdR + (kStaged ? rows : 0));   // cons_var, -1 for an index outside [0, n)
  const int tid = threadIdx.x;
  const mo_block_tangents& t = a.t;
  const bool has_dJ = t.dJ_blocks != nullptr, has_dr = t.dr != nullptr;
  const bool has_dw = kW && a.dw != nullptr;
  const bool need_r = has_dJ || has_dw;               // r is read only against dJ_blocks (and the tangent of the weights)
  const bool cost = has_dJ || has_dr || has_dw;       // the only tangents that read J_blocks
  const bool eq = k > 0 && t.dJ_eq_blocks != nullptr;
  const bool cons = m > 0 && t.dcons_a != nullptr;
  const int sub = tid / width, l = tid - sub * width, per_pass = kThreads / width;
  // the schedule is the same for every problem: what a lane needs for its first stacked row and its first variable is read once
  const int4 row0 = (cost && tid < rows) ? a.d_row[tid] : make_int4(0, 0, 0, 0);
  int ce0 = 0, ce1 = 0, we0 = 0, we1 = 0;
  int4 cent0 = make_int4(0, 0, 0, -1);
  if (sub < n) {
    if (cost) {
      ce0 = a.c_ptr[sub] + l; ce1 = a.c_ptr[sub + 1];
      if (ce0 < ce1) cent0 = a.c_ent[ce0];
    }
    if (eq) { we0 = a.w_ptr[sub] + l; we1 = a.w_ptr[sub + 1]; }
  }

  for (long long p = blockIdx.x; p < a.batch; p += gridDim.x) {
    const T* vp = (const T*)a.vars + p * a.vars_stride;
    T* rho = (T*)a.rho + p * a.rho_stride;
    const T* Jv = cost ? (const T*)a.J + p * a.J_stride : nullptr;
    const T* rv = need_r ? (const T*)a.r + p * a.r_stride : nullptr;
    const T* wv = kW ? (const T*)a.weights + p * a.weights_stride : nullptr;
    const T* dwv = has_dw ? (const T*)a.dw + p * a.dw_stride : nullptr;
    const T* dJv = has_dJ ? (const T*)t.dJ_blocks + p * t.dJ_stride : nullptr;
    const T* drv = has_dr ? (const T*)t.dr + p * t.dr_stride : nullptr;
    const T* dJe = eq ? (const T*)t.dJ_eq_blocks + p * t.dJ_eq_stride : nullptr;
    const T dlam = t.dlambda ? ((const T*)t.dlambda)[p * t.dlambda_stride] : (T)0;
    const int* cvp = a.cons_var ? a.cons_var + p * a.cons_stride : nullptr;
    const T* dca = cons ? (const T*)t.dcons_a + p * t.dcons_stride : nullptr;
    const T* dcb = (m > 0 && t.dcons_b) ? (const T*)t.dcons_b + p * t.dcons_stride : nullptr;
    __syncthreads();  // the previous problem's readers are done with the LDS
    // phase 1
    for (int i = tid; i < n; i += kThreads) {
      const T xi = vp[i];
      sx[i] = xi;
      srd[i] = dlam * xi;
    }
    if (k > 0) {
      const T* dre = t.dr_eq ? (const T*)t.dr_eq + p * t.dr_eq_stride : nullptr;
      for (int i = tid; i < k; i += kThreads) { sy[i] = vp[n + m + i]; spe[i] = dre ? dre[i] : (T)0; }
    }
    cons_rows_load(scv, saz, cvp, dca, vp, n + m + k, n, m, tid);
    if (kStaged && cost) {
      for (long long i = tid; i < a.values; i += kThreads) sJ[i] = Jv[i];
      Jv = sJ;
      if (has_dJ) {
        for (long long i = tid; i < a.values; i += kThreads) sdJ[i] = dJv[i];
        dJv = sdJ;
      }
      if (need_r) {
        for (int i = tid; i < rows; i += kThreads) sR[i] = rv[i];
        rv = sR;
      }
      if (has_dr) {
        for (int i = tid; i < rows; i += kThreads) sdR[i] = drv[i];
        drv = sdR;
      }
    }
    __syncthreads();
    // phase 2: t, tdot per stacked cost row
    if (cost) {
      for (int row = tid; row < rows; row += kThreads) {
        const int4 ri = row == tid ? row0 : a.d_row[row];
        T tt = 0, td = 0;
        if (has_dJ) {
          for (int c = 0; c < ri.z; ++c) {
            const T xg = sx[a.d_idx[ri.w + c]];
            const T p1 = Jv[ri.x + c * ri.y] * xg, p2 = dJv[ri.x + c * ri.y] * xg;
            tt += p1;
            td += p2;
          }
          tt += rv[row];
        } else if (has_dw) {
          for (int c = 0; c < ri.z; ++c) {
            const T p1 = Jv[ri.x + c * ri.y] * sx[a.d_idx[ri.w + c]];
            tt += p1;
          }
          tt += rv[row];
        }
        if (has_dr) td += drv[row];
        if (kW) {
          const T g = wv[row];
          sg[row] = g;
          const T gt = g * tt, gd = g * td;
          T tw = g == (T)0 ? (T)0 : gt, tdw = g == (T)0 ? (T)0 : gd;
          if (has_dw) {
            const T gdot = dwv[row];
            if (gdot != (T)0) {
              const T pw = gdot * tt;
              tdw += pw;
            }
          }
          tt = tw;
          td = tdw;
        }
        st[row] = tt;
        std_[row] = td;
      }
      __syncthreads();
    }
    // phase 3: rho_d[i], a group of `width` lanes per variable (uniform bounds: every lane takes part in the shuffles)
    if (cost || eq) {
      for (int i0 = 0; i0 < n; i0 += per_pass) {
        const int i = i0 + sub;
        T acc = 0;
        if (i < n) {
          if (cost) {
            const T xi = sx[i];
            const int e0 = i0 == 0 ? ce0 : a.c_ptr[i] + l, e1 = i0 == 0 ? ce1 : a.c_ptr[i + 1];
            for (int e = e0; e < e1; e += width) {
              const int4 c = (i0 == 0 && e == e0) ? cent0 : a.c_ent[e];
              T d = 0;
              if (has_dJ) {
                for (int q = 0; q < c.z; ++q) {
                  if (kW && st[c.y + q] == (T)0 && std_[c.y + q] == (T)0) continue;
                  const T p1 = dJv[c.x + q] * st[c.y + q], p2 = Jv[c.x + q] * std_[c.y + q];
                  d += p1;
                  d += p2;
                }
              } else {
                for (int q = 0; q < c.z; ++q) {
                  if (kW && std_[c.y + q] == (T)0) continue;
                  const T p2 = Jv[c.x + q] * std_[c.y + q];
                  d += p2;
                }
              }
              const int dup = c.w;
              if (dup >= 0 && (has_dJ || has_dw)) {  // a repeated variable inside the block: the pair landed once, on the diagonal
                const int cnt = a.d_dup[dup];
                for (int j = 1; j <= cnt; ++j) {
                  const int o = a.d_dup[dup + j];
                  T dd = 0;
                  if (kW) {
                    for (int q = 0; q < c.z; ++q) {
                      const T g = sg[c.y + q];
                      if (has_dJ && g != (T)0) {
                        const T gj = g * dJv[c.x + q];
                        const T pd = gj * Jv[o + q];
                        dd += pd;
                      }
                      if (has_dw && o > c.x) {
                        const T gdot = dwv[c.y + q];
                        if (gdot != (T)0) {
                          const T gj = gdot * Jv[c.x + q];
                          const T pd = gj * Jv[o + q];
                          dd += pd;
                        }
                      }
                    }
                  } else {
                    for (int q = 0; q < c.z; ++q) {
                      const T pd = dJv[c.x + q] * Jv[o + q];
                      dd += pd;
                    }
                  }
                  const T px = xi * dd;
                  d -= px;
                }
              }
              acc += d;
            }
          }
          if (eq) {
            const int e0 = i0 == 0 ? we0 : a.w_ptr[i] + l, e1 = i0 == 0 ? we1 : a.w_ptr[i + 1];
            for (int e = e0; e < e1; e += width) {
              const int4 c = a.w_ent[e];
              T d = 0;
              for (int q = 0; q < c.z; ++q) {
                const T p1 = dJe[c.x + q] * sy[c.y + q];
                d += p1;
              }
              acc -= d;
            }
          }
        }
        acc = group_sum(acc, width);
        if (l == 0 && i < n) srd[i] += acc;
      }
    }
    // phase 4: rho_pe[row], the winners among the columns of the row's equality block
    if (eq) {
      for (int row = tid; row < k; row += kThreads) {
        const int4 ri = a.e_row[row];
        T s = 0;
        for (int c = 0; c < ri.z; ++c) {
          const int e = ri.x + c * ri.y;
          const int g = a.e_val[e].y;
          if (g >= 0) {
            const T p1 = dJe[e] * sx[g];
            s += p1;
          }
        }
        spe[row] += s;
      }
    }
    __syncthreads();
    // phase 5: rho_d[var_i] -= dcons_a[i] z_i: the owner of variable j walks the rows in their order, however many name j
    if (cons) {
      cons_rows_scatter(srd, scv, saz, n, m, tid);
      __syncthreads();
    }
    // phase 6
    for (int i = tid; i < n; i += kThreads) rho[i] = srd[i];
    cons_rows_write<T, false>(rho, n, n + m + k, scv, dca, dcb, sx, m, tid);   // (the product rounded before the sum, as everywhere here)
    for (int i = tid; i < k; i += kThreads) rho[n + m + i] = spe[i];
  }
}

// lanes per variable in phase 3: the largest power of two that keeps the whole workgroup busy in one pass, at most 16 (the lists are short)
int width_for(int n) {
#ifdef MO_TUNING   // MO_BLOCKS_TANGENT_WIDTH=1: one lane per variable (A/B builds only: the product library reads no environment variable)
  if (const char* e = getenv("MO_BLOCKS_TANGENT_WIDTH")) {
    const int w = atoi(e);
    if (w >= 1 && w <= 64 && (w & (w - 1)) == 0) return w;
  }
#endif
  int w = 1;
  while (w < 16 && (long long)n * (w * 2) <= kThreads) w *= 2;
  return w;
}

template <typename T> hipError_t launch_t(const BlockTangentArgs& a, int num_cus, hipStream_t stream) {
  const bool weighted = a.weights != nullptr;
  const size_t vectors = blocks_tangent_lds_bytes(a.n, a.k, a.m, a.rows, sizeof(T), weighted);
  const bool cost = a.t.dJ_blocks || a.t.dr || (weighted && a.dw);
  const size_t stage = cost ? (size_t)(2 * (a.values + a.rows)) * sizeof(T) : 0;
  const int width = width_for(a.n);
  if (weighted) {
    if (cost && stage <= kStageBudget && vectors + stage <= kTangentLds) {
      hipLaunchKernelGGL((blocks_tangent_kernel<T, true, true>), dim3(grid_for(a.batch, num_cus, vectors + stage)), dim3(kThreads), vectors + stage, stream, a, width);
    } else {
      hipLaunchKernelGGL((blocks_tangent_kernel<T, false, true>), dim3(grid_for(a.batch, num_cus, vectors)), dim3(kThreads), vectors, stream, a, width);
    }
    return hipGetLastError();
  }
  if (cost && stage <= kStageBudget && vectors + stage <= kTangentLds) {
    hipLaunchKernelGGL((blocks_tangent_kernel<T, true>), dim3(grid_for(a.batch, num_cus, vectors + stage)), dim3(kThreads), vectors + stage, stream, a, width);
  } else {
    hipLaunchKernelGGL((blocks_tangent_kernel<T, false>), dim3(grid_for(a.batch, num_cus, vectors)), dim3(kThreads), vectors, stream, a, width);
  }
  return hipGetLastError();
}

}  // namespace

size_t blocks_tangent_lds_bytes(int n, int k, int m, int rows, int elem_size, bool weighted) {
  return (size_t)(2 * (long long)n + 2 * (long long)k + (long long)m + (weighted ? 3 : 2) * (long long)rows) * elem_size + (size_t)m * sizeof(int);
}

bool blocks_tangent_fits(int n, int k, int m, int rows, int elem_size, bool weighted) {
  return blocks_tangent_lds_bytes(n, k, m, rows, elem_size, weighted) <= kTangentLds;
}

hipError_t launch_blocks_tangent(const BlockTangentArgs& a, int dtype, int num_cus, hipStream_t stream) {
  if (a.batch <= 0) return hipSuccess;
  const int elem = dtype == MO_F64 ? 8 : 4;
  if (!blocks_tangent_fits(a.n, a.k, a.m, a.rows, elem, a.weights != nullptr)) return hipErrorInvalidValue;  // (mo_qp_tangent_rhs_blocks refuses with its own message)
  return dtype == MO_F64 ? launch_t<double>(a, num_cus, stream) : launch_t<float>(a, num_cus, stream);
}

}  // namespace mo
