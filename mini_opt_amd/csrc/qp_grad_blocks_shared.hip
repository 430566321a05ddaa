// qp_grad_blocks_shared.hip -- mo_qp_gradients_blocks_shared: the gradients of mo_qp_gradients_blocks / mo_qp_gradients_eq_blocks SUMMED over
// the batch, for packed blocks the whole batch shares (the formulas: include/mini_opt_hip.h).
// Stage 1 is qp_moment_kernel of qp_grad_shared.hip (launch_qp_moments): M = sum u_x x^T, A1 = sum y u_x^T, A2 = sum u_y x^T and the column
// sums per chunk of problems, on the matrix cores.
// blocks_q_kernel, only with an r per problem: the same chunks; a workgroup owns one chunk and kQPerGroup packed values, stages the r and u_x
// rows of `stage` problems at a time in LDS and every thread sums its values' products r[row] u_x[index] over the problems that count, in
// problem order, each product rounded before it is added (a masked problem's rows are skipped whole: never multiplied).  One owner per partial: no atomics, no memset.
// blocks_shared_finish_kernel: pass 0 sums the chunk partials of every element in chunk order, in double; pass 1 forms the outputs from those
// totals in double by gathering through the layouts' backward schedules (d_row / d_idx / d_val / d_dup, the eq layout's e_val) and rounds
// once, in the packing of J_blocks.
#include <string.h>

#include "mo_sens_device.h"

namespace mo {
namespace {

constexpr int kQPerThread = 8;                       // packed values a thread owns: 8 accumulators
constexpr int kQPerGroup = kThreads * kQPerThread;   // ... and a workgroup; more values = more workgroups per chunk (grid y)
constexpr int kQStage = 16;                          // problems staged at a time, at most
constexpr int kLoads = 8;                            // staging loads in flight per lane

struct BlockSharedPlan {
  BlockSharedArgs b;
  MomentLayout ml;
  int has_q;                   // Q partials exist (dJ_blocks with an r per problem)
  int stage;                   // problems blocks_q_kernel stages at a time
  long long chunk_len;
  const void* partials;        // [chunks][ml.chunk_elems], written by qp_moment_kernel
  void* q_partials;            // [chunks][values]
  double* totals;              // [ml.chunk_elems]
  double* q_totals;            // [values]
  size_t workspace_bytes;
};

template <typename T>
__global__ __launch_bounds__(kThreads) void blocks_q_kernel(const BlockSharedPlan a) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char smem[];
  const BlockSharedArgs& s = a.b;
  __shared__ int counts[kQStage];         // problem pl of the stage counts
  T* rows = reinterpret_cast<T*>(smem);   // problem pl of a stage: [r (rows) | u_x (n)] at rows + pl * W
  const int tid = threadIdx.x, R = s.rows, W = s.rows + s.n;
  const long long chunk = blockIdx.x;
  const long long e0 = (long long)blockIdx.y * kQPerGroup;
  const long long p_begin = chunk * a.chunk_len;
  const long long p_end = p_begin + a.chunk_len < s.batch ? p_begin + a.chunk_len : s.batch;
  const int step_pl = kThreads / W, step_e = kThreads - step_pl * W;   // element at + kThreads of a stage: problem + step_pl, offset + step_e
  const int pl_first = tid / W, e_first = tid - pl_first * W;
  int ro[kQPerThread], uo[kQPerThread];
  T acc[kQPerThread];
#pragma unroll
  for (int j = 0; j < kQPerThread; ++j) {
    const long long e = e0 + j * kThreads + tid;
    const int4 vi = s.d_val[e < s.values ? e : 0];   // (in bounds whatever e; such a slot is never written)
    ro[j] = vi.x;
    uo[j] = R + vi.y;
    acc[j] = (T)0;
  }
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
#pragma unroll
      for (int i = 0; i < kLoads; ++i) {
        const bool in = base + i * kThreads < total;   // (past the stage: element 0 of its first problem, in bounds whatever i)
        const long long p = p0 + (in ? pl : 0);
        const int at = in ? e : 0;
        v[i] = at < R ? ((const T*)s.r)[p * s.r_stride + at] : ((const T*)s.u)[p * s.u_stride + (at - R)];
        pl += step_pl;
        e += step_e;
        if (e >= W) { e -= W; ++pl; }
      }
#pragma unroll
      for (int i = 0; i < kLoads; ++i)
        if (base + i * kThreads < total) rows[base + i * kThreads] = v[i];
    }
    __syncthreads();
    for (int pl = 0; pl < live; ++pl) {
      if (!counts[pl]) continue;   // (uniform: a masked problem's rows may be NaN and are never multiplied)
      const T* row = rows + (size_t)pl * W;
#pragma unroll
      for (int j = 0; j < kQPerThread; ++j) {
        const T pr = row[ro[j]] * row[uo[j]];
        acc[j] += pr;
      }
    }
  }
  T* part = (T*)a.q_partials + chunk * s.values;
#pragma unroll
  for (int j = 0; j < kQPerThread; ++j) {
    const long long e = e0 + j * kThreads + tid;
    if (e < s.values) part[e] = acc[j];
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void blocks_shared_finish_kernel(const BlockSharedPlan a, const int pass) {
  const BlockSharedArgs& s = a.b;
  const mo_block_shared_grads& o = s.out;
  const MomentLayout& ml = a.ml;
  const long long gtid = (long long)blockIdx.x * kThreads + threadIdx.x, gsize = (long long)gridDim.x * kThreads;
  double* tot = a.totals;
  if (pass == 0) {   // every element of a chunk's block, and every packed Q value, summed over the chunks in their order
    const T* part = (const T*)a.partials;
    for (long long e = gtid; e < ml.chunk_elems; e += gsize) {
      double sum = 0.0;
      for (long long c = 0; c < ml.chunks; ++c) sum += (double)part[c * ml.chunk_elems + e];
      tot[e] = sum;
    }
    if (a.has_q) {
      const T* qp = (const T*)a.q_partials;
      for (long long e = gtid; e < s.values; e += gsize) {
        double sum = 0.0;
        for (long long c = 0; c < ml.chunks; ++c) sum += (double)qp[c * s.values + e];
        a.q_totals[e] = sum;
      }
    }
    return;
  }
  const int n = s.n, ntn = ml.ntn;
  auto tile_at = [=](int first, int i, int j) { return tot[(size_t)(first + (i >> 4) * ntn + (j >> 4)) * 256 + (i & 15) * 16 + (j & 15)]; };
  auto M = [=](int i, int j) { return tile_at(0, i, j); };
  const double* sv = tot + (size_t)ml.tiles * 256;   // [s_u | s_uy | ...]
  const T* J = (const T*)s.J;
  if (o.dJ_blocks) {
    const T* r = (const T*)s.r;
    for (long long e = gtid; e < s.values; e += gsize) {
      const int4 vi = s.d_val[e];           // {stacked row, global index, row within the block, partner list}
      const int4 ri = s.d_row[vi.x];        // {offset of J_b[q, 0], R_b, P_b, start of idx_b}
      const int i = vi.y;
      double t = 0.0;
      for (int c = 0; c < ri.z; ++c) {
        const int j = s.d_idx[ri.w + c];
        t += (double)J[ri.x + c * ri.y] * (M(i, j) + M(j, i));
      }
      double out = -t - (a.has_q ? a.q_totals[e] : (double)r[vi.x] * sv[i]);
      if (vi.w >= 0) {   // a repeated variable inside the block: the pair landed once, on the diagonal
        const int cnt = s.d_dup[vi.w];
        double d = 0.0;
        for (int q = 1; q <= cnt; ++q) d += (double)J[s.d_dup[vi.w + q] + vi.z];
        out += M(i, i) * d;
      }
      ((T*)o.dJ_blocks)[e] = (T)out;
    }
  }
  if (o.dr)
    for (long long row = gtid; row < s.rows; row += gsize) {
      const int4 ri = s.d_row[row];
      double t = 0.0;
      for (int c = 0; c < ri.z; ++c) t += (double)J[ri.x + c * ri.y] * sv[s.d_idx[ri.w + c]];
      ((T*)o.dr)[row] = (T)-t;
    }
  if (o.dlambda && gtid == 0) {
    double tr = 0.0;
    for (int i = 0; i < n; ++i) tr += M(i, i);
    *(T*)o.dlambda = (T)-tr;
  }
  if (o.dJ_eq_blocks) {
    const int first = ml.m_tiles, second = ml.m_tiles + ml.a_tiles;
    for (long long e = gtid; e < s.eq_values; e += gsize) {
      const int2 vi = s.e_val[e];           // {stacked row, global index or -1 for a column that loses its global column}
      ((T*)o.dJ_eq_blocks)[e] = vi.y >= 0 ? (T)(tile_at(first, vi.x, vi.y) - tile_at(second, vi.x, vi.y)) : (T)0;
    }
  }
  if (o.dr_eq)
    for (long long i = gtid; i < s.k; i += gsize) ((T*)o.dr_eq)[i] = (T)-sv[n + i];
}

MomentNeeds needs_of(const BlockSharedArgs& b) {
  const mo_block_shared_grads& o = b.out;
  MomentNeeds nd;
  nd.M = o.dJ_blocks || o.dlambda;
  nd.A = o.dJ_eq_blocks != nullptr;
  nd.Q = 0;   // (the dense form's rows x n tiles: the block form keeps Q packed)
  nd.y = o.dJ_eq_blocks || o.dr_eq;
  nd.z = 0;
  return nd;
}

// what qp_moment_kernel reads of the call
SharedGradArgs moment_args(const BlockSharedArgs& b) {
  SharedGradArgs g;
  memset(&g, 0, sizeof(g));
  g.n = b.n; g.k = b.k; g.m = b.m; g.batch = b.batch;
  g.vars = b.vars; g.vars_stride = b.vars_stride;
  g.u = b.u; g.u_stride = b.u_stride;
  g.status_fwd = b.status_fwd; g.status_adj = b.status_adj;
  g.workspace = b.workspace;
  return g;
}

size_t pad16b(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

BlockSharedPlan plan_of(const BlockSharedArgs& b, int elem, int num_cus) {
  BlockSharedPlan a;
  memset(&a, 0, sizeof(a));
  a.b = b;
  a.ml = shared_moment_layout(moment_args(b), needs_of(b), elem, num_cus);
  a.has_q = b.out.dJ_blocks && b.r_stride != 0;
  a.chunk_len = shared_grad_chunk_len(b.batch, num_cus);
  const size_t row_bytes = (size_t)(b.rows + b.n) * elem;
  a.stage = 1;
  for (int ps = kQStage; ps >= 1; ps >>= 1)
    if (ps * row_bytes <= 48 * 1024) { a.stage = ps; break; }
  // [moment partials | Q partials | totals | Q totals]: every piece 16-byte aligned
  const size_t off_q = pad16b((size_t)a.ml.chunks * a.ml.chunk_elems * elem);
  const size_t off_tot = off_q + (a.has_q ? pad16b((size_t)a.ml.chunks * b.values * elem) : 0);
  const size_t off_qtot = off_tot + pad16b((size_t)a.ml.chunk_elems * sizeof(double));
  a.workspace_bytes = off_qtot + (a.has_q ? pad16b((size_t)b.values * sizeof(double)) : 0);
  if (b.workspace) {
    char* base = (char*)b.workspace;
    a.partials = base; a.q_partials = base + off_q; a.totals = (double*)(base + off_tot); a.q_totals = (double*)(base + off_qtot);
  }
  return a;
}

}  // namespace

size_t blocks_shared_workspace_bytes(const BlockSharedArgs& b, int elem_size, int num_cus) {
  return plan_of(b, elem_size, num_cus).workspace_bytes;
}

bool blocks_shared_fits(const BlockSharedArgs& b, int elem_size) {
  if (shared_moment_lds_bytes(moment_args(b), needs_of(b), elem_size) > 64 * 1024) return false;
  // blocks_q_kernel: one problem's [r | u_x] beside its kQStage flags
  return !(b.out.dJ_blocks && b.r_stride != 0) || (size_t)(b.rows + b.n) * elem_size + kQStage * sizeof(int) <= 64 * 1024;
}

hipError_t launch_blocks_shared_grad(const BlockSharedArgs& b, int dtype, int num_cus, hipStream_t stream) {
  const int elem = dtype == MO_F64 ? 8 : 4;
  if (!blocks_shared_fits(b, elem)) return hipErrorInvalidValue;   // (mo_qp_gradients_blocks_shared refuses such shapes with its own message)
  const BlockSharedPlan a = plan_of(b, elem, num_cus);
  if (hipError_t e = launch_qp_moments(moment_args(b), needs_of(b), dtype, num_cus, stream)) return e;
  if (a.has_q && a.ml.chunks > 0) {
    const dim3 grid((unsigned)a.ml.chunks, (unsigned)((b.values + kQPerGroup - 1) / kQPerGroup));
    const size_t lds = (size_t)a.stage * (b.rows + b.n) * elem;
    if (dtype == MO_F64) hipLaunchKernelGGL(blocks_q_kernel<double>, grid, dim3(kThreads), lds, stream, a);
    else hipLaunchKernelGGL(blocks_q_kernel<float>, grid, dim3(kThreads), lds, stream, a);
    if (hipError_t e = hipGetLastError()) return e;
  }
  // pass 0: one thread per element of a chunk's block and per packed Q value; pass 1: one thread per element of the largest output
  const long long work0 = (a.ml.chunk_elems + (a.has_q ? b.values : 0) + kThreads - 1) / kThreads;
  long long largest = b.out.dJ_blocks ? b.values : 1;
  if (b.out.dJ_eq_blocks && b.eq_values > largest) largest = b.eq_values;
  if (b.out.dr && b.rows > largest) largest = b.rows;
  if (b.out.dr_eq && b.k > largest) largest = b.k;
  const long long work1 = (largest + kThreads - 1) / kThreads;
  const long long cap = (long long)num_cus * 8;
  for (int pass = 0; pass < 2; ++pass) {
    long long blocks = pass == 0 ? work0 : work1;
    blocks = blocks > cap ? cap : (blocks < 1 ? 1 : blocks);
    if (dtype == MO_F64) hipLaunchKernelGGL(blocks_shared_finish_kernel<double>, dim3((unsigned)blocks), dim3(kThreads), 0, stream, a, pass);
    else hipLaunchKernelGGL(blocks_shared_finish_kernel<float>, dim3((unsigned)blocks), dim3(kThreads), 0, stream, a, pass);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}

}  // namespace mo
