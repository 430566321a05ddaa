// qp_grad_blocks_wshared.hip -- mo_qp_gradients_blocks_weighted_shared: the gradients of mo_qp_gradients_blocks_weighted SUMMED over the
// batch, for ONE instance of the packed blocks under weights and residuals per problem (the formulas:
// include/mini_opt_hip.h).  With a weight per row and per problem the sums do not factor through the moments of (x, u_x), so nothing of
// qp_grad_shared.hip is used: every problem's t = J x_loc + r and s = J u_loc are formed on chip from the one J and consumed at once, at the
// packed positions only.
// blocks_ws_kernel: the chunks of the other batch-reduced launches; a workgroup owns one chunk and kQPerGroup packed values, stages the
// [x | u_x | r | w] rows of `stage` problems at a time in LDS.  Phase A: a thread per (staged problem, stacked row) walks the row's columns
// against J (read in place through the vector cache: one instance, `values` elements, the same addresses for every problem and every
// workgroup of the launch; in LDS it would cost stage depth and cap `values`) and overwrites the row's r, w slots with a = w t, c = w s --
// both exactly 0, without a multiplication, where w == 0.  Phase B: every thread adds u[i] a + x[i] c for its values over the problems that
// count, in problem order, each product rounded before it is added; with partner lists in the layout also w u_i x_i, into a second
// accumulator.  The value-group 0 of a chunk owns the row sums (sum c, sum s t) and the n sums (sum u_i x_i), formed only when a member
// needs them.  A masked problem is skipped whole.  One owner per partial: no atomics, no memset.
// blocks_ws_finish_kernel: pass 0 sums the chunk partials of every element in chunk order, in double; pass 1 forms the outputs from those
// totals in double through d_val / d_dup / d_pair / d_plist and rounds once, in the packing of J_blocks.
#include <string.h>

#include "mo_sens_device.h"

namespace mo {
namespace {

constexpr int kQPerThread = 8;                       // packed values a thread owns
constexpr int kQPerGroup = kThreads * kQPerThread;   // ... and a workgroup; more values = more workgroups per chunk (grid y)
constexpr int kQStage = 16;                          // problems staged at a time, at most
constexpr int kLoads = 8;                            // staging loads in flight per lane
constexpr size_t kStageBudget = 48 * 1024;           // what more than one staged problem may use
constexpr size_t kLdsLimit = 64 * 1024;              // one staged problem and the flags

struct BlockWSharedPlan {
  BlockWSharedArgs b;
  int need_v, need_c, need_st, need_ux;   // partials: packed values (dJ_blocks), sum c (dr), sum s t (dweights), sum u_i x_i (dlambda; dweights' pairs)
  int dup;                     // the layout has partner lists: the second accumulator per packed value
  int stage, wl;               // problems staged at a time; values of one staged problem
  long long chunk_len, chunks;
  long long off_v2, off_c, off_st, off_ux, chunk_elems;   // a chunk's partials: [values | values (dup) | rows (c) | rows (s t) | n (u x)]
  void* partials;              // [chunks][chunk_elems]
  double* totals;              // [chunk_elems]
  size_t workspace_bytes;
};

template <typename T, bool kDup>
__global__ __launch_bounds__(kThreads) void blocks_ws_kernel(const BlockWSharedPlan a) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char smem[];
  const BlockWSharedArgs& s = a.b;
  __shared__ int counts[kQStage];         // problem pl of the stage counts
  T* rows = reinterpret_cast<T*>(smem);   // problem pl of a stage: [x (n) | u_x (n) | r -> a (rows) | w -> c (rows) | s t (rows, only with dweights)]
  const int tid = threadIdx.x, n = s.n, R = s.rows, W = 2 * s.n + 2 * s.rows, WL = a.wl;
  const int xo = 0, uo = n, ao = 2 * n, co = 2 * n + R, so = 2 * n + 2 * R;
  const long long chunk = blockIdx.x;
  const long long e0 = (long long)blockIdx.y * kQPerGroup;
  const bool owner = blockIdx.y == 0;     // of the row sums and the n sums
  const bool phase_a = a.need_v || (owner && (a.need_c || a.need_st));
  const bool want_st = owner && a.need_st;
  const long long p_begin = chunk * a.chunk_len;
  const long long p_end = p_begin + a.chunk_len < s.batch ? p_begin + a.chunk_len : s.batch;
  const int step_pl = kThreads / W, step_e = kThreads - step_pl * W;   // element at + kThreads of a stage: problem + step_pl, offset + step_e
  const int pl_first = tid / W, e_first = tid - pl_first * W;
  const int step_apl = kThreads / R, step_ar = kThreads - step_apl * R;   // the same for phase A's (problem, row)
  const int apl_first = tid / R, ar_first = tid - apl_first * R;
  const T* Jv = (const T*)s.J;
  T* part = (T*)a.partials + chunk * a.chunk_elems;
  int ro[kQPerThread], io[kQPerThread];
  bool dp[kQPerThread];
  T acc[kQPerThread], acc2[kQPerThread];
#pragma unroll
  for (int j = 0; j < kQPerThread; ++j) {
    const long long e = e0 + j * kThreads + tid;
    const int4 vi = s.d_val[e < s.values ? e : 0];   // (in bounds whatever e; such a slot is never written)
    ro[j] = vi.x;
    io[j] = vi.y;
    dp[j] = kDup && vi.w >= 0;
    acc[j] = (T)0;
    acc2[j] = (T)0;
  }
  bool first = true;   // the owner's sums have nothing in the partials yet
  for (long long p0 = p_begin; p0 < p_end; p0 += a.stage) {
    const int live = p_end - p0 < a.stage ? (int)(p_end - p0) : a.stage;
    const int total = live * W;
    __syncthreads();   // the previous stage's readers are done with the rows and the flags
    if (tid < live) {
      bool ok = true;
      if (s.status_fwd) ok = ok && s.status_fwd[p0 + tid] == MO_STATUS_OK;
      if (s.status_adj) ok = ok && s.status_adj[p0 + tid] == MO_STATUS_OK;
      counts[tid] = ok;
    }
    // the rows as they are, kLoads loads in flight per lane before the first LDS write; a masked problem's row is never read back
    int pl = pl_first, e = e_first;   // the lane's elements lie kThreads apart: {problem, offset} is stepped, never divided per load
    for (int base = tid; base < total; base += kLoads * kThreads) {
      T v[kLoads];
      int at_lds[kLoads];
#pragma unroll
      for (int i = 0; i < kLoads; ++i) {
        const bool in = base + i * kThreads < total;   // (past the stage: element 0 of its first problem, in bounds whatever i)
        const long long p = p0 + (in ? pl : 0);
        const int at = in ? e : 0;
        const T* src = at < uo ? (const T*)s.vars + p * s.vars_stride + at
                     : at < ao ? (const T*)s.u + p * s.u_stride + (at - uo)
                     : at < co ? (const T*)s.r + p * s.r_stride + (at - ao)
                               : (const T*)s.weights + p * s.weights_stride + (at - co);
        v[i] = *src;
        at_lds[i] = in ? pl * WL + e : -1;
        pl += step_pl;
        e += step_e;
        if (e >= W) { e -= W; ++pl; }
      }
#pragma unroll
      for (int i = 0; i < kLoads; ++i)
        if (at_lds[i] >= 0) rows[at_lds[i]] = v[i];
    }
    __syncthreads();
    if (phase_a) {   // (problem, row): t = J x_loc + r, s = J u_loc; the r, w slots become a = w t, c = w s
      int apl = apl_first, ar = ar_first;
      for (int item = tid; item < live * R; item += kThreads) {
        if (counts[apl]) {   // (a masked problem's rows may be NaN and are never multiplied)
          T* row = rows + (size_t)apl * WL;
          const int4 ri = s.d_row[ar];        // {offset of J_b[q, 0], R_b, P_b, start of idx_b}
          T t = 0, sv = 0;
          for (int c = 0; c < ri.z; ++c) {
            const int g = s.d_idx[ri.w + c];
            const T v = Jv[ri.x + c * ri.y];
            const T tx = v * row[xo + g], tu = v * row[uo + g];
            t += tx;
            sv += tu;
          }
          t += row[ao + ar];
          const T w = row[co + ar];
          const T wt = w * t, ws = w * sv;
          row[ao + ar] = w == (T)0 ? (T)0 : wt;
          row[co + ar] = w == (T)0 ? (T)0 : ws;
          if (want_st) row[so + ar] = sv * t;
        }
        apl += step_apl;
        ar += step_ar;
        if (ar >= R) { ar -= R; ++apl; }
      }
      __syncthreads();
    }
    if (a.need_v)
      for (int pl = 0; pl < live; ++pl) {
        if (!counts[pl]) continue;   // (uniform)
        const T* row = rows + (size_t)pl * WL;
#pragma unroll
        for (int j = 0; j < kQPerThread; ++j) {
          const T ui = row[uo + io[j]], xi = row[xo + io[j]];
          const T p1 = ui * row[ao + ro[j]], p2 = xi * row[co + ro[j]];
          const T sum = p1 + p2;
          acc[j] += sum;
          if (kDup && dp[j]) {   // a repeated variable inside the block: w u_i x_i (the w slot holds c by now: the weight from memory)
            const T w = ((const T*)s.weights)[(p0 + pl) * s.weights_stride + ro[j]];
            const T ux = ui * xi;
            const T wux = w * ux;
            acc2[j] += w == (T)0 ? (T)0 : wux;
          }
        }
      }
    if (owner) {   // the sums that are no packed value: their owner threads keep them in the partials from stage to stage
      if (a.need_c)
        for (int r = tid; r < R; r += kThreads) {
          T sum = first ? (T)0 : part[a.off_c + r];
          for (int pl = 0; pl < live; ++pl)
            if (counts[pl]) sum += rows[(size_t)pl * WL + co + r];
          part[a.off_c + r] = sum;
        }
      if (a.need_st)
        for (int r = tid; r < R; r += kThreads) {
          T sum = first ? (T)0 : part[a.off_st + r];
          for (int pl = 0; pl < live; ++pl)
            if (counts[pl]) sum += rows[(size_t)pl * WL + so + r];
          part[a.off_st + r] = sum;
        }
      if (a.need_ux)
        for (int i = tid; i < n; i += kThreads) {
          T sum = first ? (T)0 : part[a.off_ux + i];
          for (int pl = 0; pl < live; ++pl)
            if (counts[pl]) {
              const T pr = rows[(size_t)pl * WL + uo + i] * rows[(size_t)pl * WL + xo + i];
              sum += pr;
            }
          part[a.off_ux + i] = sum;
        }
      first = false;
    }
  }
  if (a.need_v) {
#pragma unroll
    for (int j = 0; j < kQPerThread; ++j) {
      const long long e = e0 + j * kThreads + tid;
      if (e < s.values) {
        part[e] = acc[j];
        if (kDup) part[a.off_v2 + e] = acc2[j];
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void blocks_ws_finish_kernel(const BlockWSharedPlan a, const int pass) {
  const BlockWSharedArgs& s = a.b;
  const mo_block_weighted_shared_grads& o = s.out;
  const long long gtid = (long long)blockIdx.x * kThreads + threadIdx.x, gsize = (long long)gridDim.x * kThreads;
  double* tot = a.totals;
  if (pass == 0) {   // every element of a chunk's partials summed over the chunks in their order
    const T* part = (const T*)a.partials;
    for (long long e = gtid; e < a.chunk_elems; e += gsize) {
      double sum = 0.0;
      for (long long c = 0; c < a.chunks; ++c) sum += (double)part[c * a.chunk_elems + e];
      tot[e] = sum;
    }
    return;
  }
  const T* J = (const T*)s.J;
  if (o.dJ_blocks)
    for (long long e = gtid; e < s.values; e += gsize) {
      double out = 0.0 - tot[e];
      if (a.dup) {
        const int4 vi = s.d_val[e];           // {stacked row, global index, row within the block, partner list}
        if (vi.w >= 0) {   // a repeated variable inside the block: the pair landed once, on the diagonal
          const int cnt = s.d_dup[vi.w];
          double d = 0.0;
          for (int q = 1; q <= cnt; ++q) d += (double)J[s.d_dup[vi.w + q] + vi.z];
          out += d * tot[a.off_v2 + e];
        }
      }
      ((T*)o.dJ_blocks)[e] = (T)out;
    }
  if (o.dr)
    for (long long row = gtid; row < s.rows; row += gsize) ((T*)o.dr)[row] = (T)(0.0 - tot[a.off_c + row]);
  if (o.dweights)
    for (long long row = gtid; row < s.rows; row += gsize) {
      double out = 0.0 - tot[a.off_st + row];
      const int pl = a.dup ? s.d_pair[row] : -1;
      if (pl >= 0) {   // the derivative of the pairs that landed once
        const int4 ri = s.d_row[row];
        const int cnt = s.d_plist[pl];
        for (int d = 0; d < cnt; ++d) {
          const int ca = s.d_plist[pl + 1 + 3 * d], cb = s.d_plist[pl + 2 + 3 * d], gi = s.d_plist[pl + 3 + 3 * d];
          out += (double)J[ri.x + ca] * (double)J[ri.x + cb] * tot[a.off_ux + gi];
        }
      }
      ((T*)o.dweights)[row] = (T)out;
    }
  if (o.dlambda && gtid == 0) {
    double tr = 0.0;
    for (int i = 0; i < s.n; ++i) tr += tot[a.off_ux + i];
    *(T*)o.dlambda = (T)(0.0 - tr);
  }
}

size_t pad16b(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

BlockWSharedPlan plan_of(const BlockWSharedArgs& b, int elem, int num_cus) {
  BlockWSharedPlan a;
  memset(&a, 0, sizeof(a));
  a.b = b;
  const mo_block_weighted_shared_grads& o = b.out;
  a.dup = b.has_dup != 0;
  a.need_v = o.dJ_blocks != nullptr;
  a.need_c = o.dr != nullptr;
  a.need_st = o.dweights != nullptr;
  a.need_ux = o.dlambda != nullptr || (o.dweights && a.dup);
  a.chunk_len = shared_grad_chunk_len(b.batch, num_cus);
  a.chunks = shared_grad_chunks(b.batch, num_cus);
  a.wl = 2 * b.n + 2 * b.rows + (a.need_st ? b.rows : 0);
  const size_t row_bytes = (size_t)a.wl * elem;
  a.stage = 1;
  for (int ps = kQStage; ps > 1; ps >>= 1)
    if (ps * row_bytes <= kStageBudget) { a.stage = ps; break; }
  long long at = a.need_v ? b.values : 0;
  a.off_v2 = at; at += a.need_v && a.dup ? b.values : 0;
  a.off_c = at;  at += a.need_c ? b.rows : 0;
  a.off_st = at; at += a.need_st ? b.rows : 0;
  a.off_ux = at; at += a.need_ux ? b.n : 0;
  a.chunk_elems = at;
  // [chunk partials | totals]: both 16-byte aligned
  const size_t off_tot = pad16b((size_t)a.chunks * a.chunk_elems * elem);
  a.workspace_bytes = off_tot + pad16b((size_t)a.chunk_elems * sizeof(double));
  if (b.workspace) {
    a.partials = b.workspace;
    a.totals = (double*)((char*)b.workspace + off_tot);
  }
  return a;
}

template <typename T>
void launch_partial(const BlockWSharedPlan& a, dim3 grid, size_t lds, hipStream_t stream) {
  if (a.dup) hipLaunchKernelGGL((blocks_ws_kernel<T, true>), grid, dim3(kThreads), lds, stream, a);
  else hipLaunchKernelGGL((blocks_ws_kernel<T, false>), grid, dim3(kThreads), lds, stream, a);
}

}  // namespace

size_t blocks_wshared_workspace_bytes(const BlockWSharedArgs& b, int elem_size, int num_cus) {
  return plan_of(b, elem_size, num_cus).workspace_bytes;
}

// one staged problem -- 2 n + 2 rows values, rows more with dweights -- beside the kQStage flags within 64 KiB
bool blocks_wshared_fits(const BlockWSharedArgs& b, int elem_size) {
  const size_t wl = 2 * (size_t)b.n + 2 * (size_t)b.rows + (b.out.dweights ? (size_t)b.rows : 0);
  return wl * elem_size + kQStage * sizeof(int) <= kLdsLimit;
}

hipError_t launch_blocks_wshared_grad(const BlockWSharedArgs& b, int dtype, int num_cus, hipStream_t stream) {
  const int elem = dtype == MO_F64 ? 8 : 4;
  if (!blocks_wshared_fits(b, elem)) return hipErrorInvalidValue;   // (mo_qp_gradients_blocks_weighted_shared refuses such shapes with its own message)
  const BlockWSharedPlan a = plan_of(b, elem, num_cus);
  if (a.chunk_elems == 0) return hipSuccess;
  if (a.chunks > 0) {
    const dim3 grid((unsigned)a.chunks, a.need_v ? (unsigned)((b.values + kQPerGroup - 1) / kQPerGroup) : 1u);
    const size_t lds = (size_t)a.stage * a.wl * elem;
    if (dtype == MO_F64) launch_partial<double>(a, grid, lds, stream);
    else launch_partial<float>(a, grid, lds, stream);
    if (hipError_t e = hipGetLastError()) return e;
  }
  // pass 0: one thread per element of a chunk's partials; pass 1: one thread per element of the largest output
  const long long work0 = (a.chunk_elems + kThreads - 1) / kThreads;
  long long largest = b.out.dJ_blocks ? b.values : 1;
  if ((b.out.dr || b.out.dweights) && b.rows > largest) largest = b.rows;
  const long long work1 = (largest + kThreads - 1) / kThreads;
  const long long cap = (long long)num_cus * 8;
  for (int pass = 0; pass < 2; ++pass) {
    long long blocks = pass == 0 ? work0 : work1;
    blocks = blocks > cap ? cap : (blocks < 1 ? 1 : blocks);
    if (dtype == MO_F64) hipLaunchKernelGGL(blocks_ws_finish_kernel<double>, dim3((unsigned)blocks), dim3(kThreads), 0, stream, a, pass);
    else hipLaunchKernelGGL(blocks_ws_finish_kernel<float>, dim3((unsigned)blocks), dim3(kThreads), 0, stream, a, pass);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}

}  // namespace mo
