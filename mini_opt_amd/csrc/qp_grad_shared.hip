// qp_grad_shared.hip -- mo_qp_gradients_shared: the gradients of mo_qp_gradients SUMMED over the batch, for data the whole batch shares
// (DESIGN.md section 4.8.7).  With ok_p = "problem p counts" and v_p = [x | s | y | z], u_p = [u_x | u_s | u_y | u_z]:
//   M = sum ok_p u_x,p x_p^T (n x n)     s_u = sum ok_p u_x,p     s_uy = sum ok_p u_y,p     s_uz = sum ok_p u_z,p
//   dG = -1/2 (M + M^T)     dc = -s_u     dlambda = -trace(M)     dA_eq = A1 - A2 = sum ok_p y_p u_x,p^T - sum ok_p u_y,p x_p^T     db_eq = -s_uy
// (A1 and A2 are tiles of their own: every accumulator is then the sum of ONE product over the problems in their order, so a problem that
// does not count leaves every bit of it as if the problem were not in the batch)
//   dcons_a[i] = sum ok_p (z_p,i u_x,p[var_i] - u_z,p,i x_p[var_i])     dcons_b = -s_uz
//   dJ = -J (M + M^T) - Q,  Q = sum ok_p r_p u_x,p^T (= r s_u^T for a shared r)     dr = -J s_u
// Stage 1, qp_moment_kernel: the batch is cut into chunks of consecutive problems (shared_grad_chunk_len: a function of batch and CU count
// alone); a workgroup owns one chunk and one group of 16 x 16 output tiles, stages the rows of 16, 8 or 4 problems at a time in LDS -- a masked
// problem and everything beyond n, k, m_r or the chunk SELECTED to zero (a masked adjoint is NaN: never multiplied) -- and accumulates its
// tiles on the matrix cores, four problems per MFMA.  The column sums and dcons_a are VALU sums in problem order.  Every workgroup writes its
// partial tiles once: one owner per workspace element, no atomics, no memset.
// Stage 2, qp_moment_finish_kernel: pass 0 sums the chunk partials of every element in chunk order, in double; pass 1 forms the outputs from
// those totals in double (the products with J on the VALU, ascending index) and rounds once.
// Stage 1 alone is also what mo_qp_gradients_blocks_shared starts with (launch_qp_moments; its finish is in qp_grad_blocks_shared.hip).
#include <string.h>

#include "mo_sens_device.h"

namespace mo {
namespace {

// v_mfma_{f64,f32}_16x16x4: operand lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15]; the C/D row maps differ (restated from
// kkt_generic.hip, which keeps its own copy: no existing unit includes anything new)
typedef double v4f64 __attribute__((ext_vector_type(4)));
typedef float v4f32 __attribute__((ext_vector_type(4)));
template <typename T> struct Mfma16;
template <> struct Mfma16<double> {
  typedef v4f64 Acc;
  __device__ static inline Acc mac(double a, double b, Acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  __device__ static inline int row(int g, int t) { return g + 4 * t; }   // lane (g = lane >> 4, l = lane & 15), register t <-> (row g + 4 t, col l)
};
template <> struct Mfma16<float> {
  typedef v4f32 Acc;
  __device__ static inline Acc mac(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
  __device__ static inline int row(int g, int t) { return 4 * g + t; }   // (row 4 g + t, col l)
};

constexpr int kWaves = kThreads / 64;
constexpr int kTilesPerWave = 8;                       // 8 accumulators of 4 values: 64 VGPRs in fp64, no scratch
constexpr int kTilesPerGroup = kWaves * kTilesPerWave;  // the tiles of one workgroup; more tiles = more workgroups per chunk (grid y)

// the launch plan: which tile sets exist, where a problem's vectors lie in its LDS row, how the workspace is cut
struct MomentArgs {
  SharedGradArgs g;
  int ntn;                               // 16-wide tiles across n
  int m_tiles, a_tiles, q_tiles, tiles;  // M (n x n), A1 and A2 (k x n each: a_tiles apiece), Q (m_r x n): tile counts, row-major over
                                         // (tile row, tile column); tiles = m_tiles + 2 a_tiles + q_tiles
  int vec, vec_pad;                      // [s_u n | s_uy k | s_uz m | dcons_a m], padded to 16
  long long chunk_len, chunks, chunk_elems;   // problems per chunk, chunks, workspace elements per chunk = 256 tiles + vec_pad
  int off_x, off_ux, off_y, off_uy, off_z, off_uz, off_r;   // LDS row: segments of whole tiles, zero beyond the vector
  int S, stage;                          // row stride (elements) and rows staged at a time (a multiple of 4)
  int has_y, has_z, has_r;
  int vec_dG, vec_dA, vec_dJ;
  void* partials; double* totals;
};

// NP problems' worth of one segment pair (the same `count` elements at `src_off` of a problem's vars row and of its u row) to the LDS
// rows: every load of a pass is issued before the first LDS write, 2 NP loads in flight per lane.  With u = nullptr: the vars-side only (r).
template <typename T, int NP>
__device__ __forceinline__ void stage_pair(T* const (&row)[NP], int off_v, int off_u, const T* const (&vp)[NP], const T* const (&up)[NP],
                                           bool has_u, int count, int count16, const bool (&ok)[NP], int lane) {
  for (int e = lane; e < count16; e += 64) {
    const int ec = e < count ? e : 0;   // (in bounds whatever e; selected to zero below)
    T a[NP], b[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      a[q] = vp[q][ec];
      b[q] = has_u ? up[q][ec] : (T)0;
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const bool keep = ok[q] && e < count;
      row[q][off_v + e] = keep ? a[q] : (T)0;
      if (has_u) row[q][off_u + e] = keep ? b[q] : (T)0;
    }
  }
}

// the rows pl = first, first + kWaves, ... (NP of them) of a stage: a wave stages whole problems, so their status words are uniform
template <typename T, int NP>
__device__ __forceinline__ void stage_rows(const MomentArgs& a, T* rows, int first, int live, long long p0, long long p_end, int lane) {
  const SharedGradArgs& s = a.g;
  const int n = s.n, k = s.k, m = s.m;
  T* row[NP];
  const T* vp[NP];
  const T* up[NP];
  const T* rp[NP];
  bool ok[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    const int pl = first + q * kWaves;
    const bool in = pl < live;
    const long long pc = in ? p0 + pl : p_end - 1;      // (clamped in bounds)
    ok[q] = in;
    if (s.status_fwd) ok[q] = ok[q] && s.status_fwd[pc] == MO_STATUS_OK;
    if (s.status_adj) ok[q] = ok[q] && s.status_adj[pc] == MO_STATUS_OK;
    vp[q] = (const T*)s.vars + pc * s.vars_stride;
    up[q] = (const T*)s.u + pc * s.u_stride;
    rp[q] = a.has_r ? (const T*)s.r + pc * s.r_stride : vp[q];
    row[q] = rows + (size_t)pl * a.S;
  }
  const T* yv[NP];
  const T* yu[NP];
  const T* zv[NP];
  const T* zu[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) { yv[q] = vp[q] + n + m; yu[q] = up[q] + n + m; zv[q] = vp[q] + n + m + k; zu[q] = up[q] + n + m + k; }
  stage_pair<T, NP>(row, a.off_x, a.off_ux, vp, up, true, n, 16 * a.ntn, ok, lane);
  if (a.has_y) stage_pair<T, NP>(row, a.off_y, a.off_uy, yv, yu, true, k, (k + 15) & ~15, ok, lane);
  if (a.has_z) stage_pair<T, NP>(row, a.off_z, a.off_uz, zv, zu, true, m, (m + 15) & ~15, ok, lane);
  if (a.has_r) stage_pair<T, NP>(row, a.off_r, 0, rp, rp, false, s.m_r, (s.m_r + 15) & ~15, ok, lane);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void qp_moment_kernel(const MomentArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef Mfma16<T> MF;
  typedef typename MF::Acc Acc;
  const SharedGradArgs& s = a.g;
  const int n = s.n, k = s.k, m = s.m, S = a.S;
  T* rows = reinterpret_cast<T*>(smem);
  T* vsum = rows + (size_t)a.stage * S;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, l = lane & 15;
  const long long chunk = blockIdx.x;
  const int group = blockIdx.y;
  const long long p_begin = chunk * a.chunk_len;
  const long long p_end = p_begin + a.chunk_len < s.batch ? p_begin + a.chunk_len : s.batch;   // (> p_begin: the last chunk is not empty)

  // this wave's tiles: tile group * kTilesPerGroup + i * kWaves + wave.  acc = sum A[.][p] B[p][.]
  int a1[kTilesPerWave], b1[kTilesPerWave];
  bool have[kTilesPerWave];
  Acc acc[kTilesPerWave];
#pragma unroll
  for (int i = 0; i < kTilesPerWave; ++i) {
    int t = group * kTilesPerGroup + i * kWaves + wave;
    have[i] = t < a.tiles;
    a1[i] = b1[i] = 0;
    if (t < a.m_tiles) {                       // M = u_x x^T
      a1[i] = a.off_ux + 16 * (t / a.ntn); b1[i] = a.off_x + 16 * (t % a.ntn);
    } else if (t < a.m_tiles + a.a_tiles) {    // A1 = y u_x^T
      t -= a.m_tiles;
      a1[i] = a.off_y + 16 * (t / a.ntn); b1[i] = a.off_ux + 16 * (t % a.ntn);
    } else if (t < a.m_tiles + 2 * a.a_tiles) {   // A2 = u_y x^T
      t -= a.m_tiles + a.a_tiles;
      a1[i] = a.off_uy + 16 * (t / a.ntn); b1[i] = a.off_x + 16 * (t % a.ntn);
    } else if (have[i]) {                      // Q = r u_x^T
      t -= a.m_tiles + 2 * a.a_tiles;
      a1[i] = a.off_r + 16 * (t / a.ntn); b1[i] = a.off_ux + 16 * (t % a.ntn);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[i][q] = (T)0;
  }
  if (group == 0)
    for (int e = tid; e < a.vec_pad; e += kThreads) vsum[e] = (T)0;   // (each element has one owner thread throughout)

  for (long long p0 = p_begin; p0 < p_end; p0 += a.stage) {
    const int live = p_end - p0 < a.stage ? (int)(p_end - p0) : a.stage;
    const int steps = (live + 3) >> 2;
    __syncthreads();   // the previous stage's readers are done with the rows
    {   // rows wave, wave + kWaves, ...: `steps` of them per wave (at most stage / 4 = 4), four, two or one at a time
      int j = 0;
      for (; j + 4 <= steps; j += 4) stage_rows<T, 4>(a, rows, wave + j * kWaves, live, p0, p_end, lane);
      for (; j + 2 <= steps; j += 2) stage_rows<T, 2>(a, rows, wave + j * kWaves, live, p0, p_end, lane);
      for (; j < steps; ++j) stage_rows<T, 1>(a, rows, wave + j * kWaves, live, p0, p_end, lane);
    }
    __syncthreads();
    for (int st = 0; st < steps; ++st) {
      const T* base = rows + (size_t)(4 * st + g) * S + l;   // operand lane (l, g): element l of the tile's 16, problem 4 st + g
#pragma unroll
      for (int i = 0; i < kTilesPerWave; ++i) {
        if (have[i]) acc[i] = MF::mac(base[a1[i]], base[b1[i]], acc[i]);
      }
    }
    if (group == 0) {   // the column sums and dcons_a: the owner of element e walks the staged problems in their order (masked rows are zero)
      for (int e = tid; e < a.vec; e += kThreads) {
        T sum = vsum[e];
        int off = -1;
        if (e < n) off = a.off_ux + e;
        else if (e < n + k) off = a.has_y ? a.off_uy + (e - n) : -1;
        else if (e < n + k + m) off = a.has_z ? a.off_uz + (e - n - k) : -1;
        else if (a.has_z && s.cons_var) {
          const int i = e - n - k - m, v = s.cons_var[i];
          if (v >= 0 && v < n)
            for (int pl = 0; pl < live; ++pl) {
              const T* row = rows + (size_t)pl * S;
              sum += row[a.off_z + i] * row[a.off_ux + v] - row[a.off_uz + i] * row[a.off_x + v];
            }
        }
        if (off >= 0)
          for (int pl = 0; pl < live; ++pl) sum += rows[(size_t)pl * S + off];
        vsum[e] = sum;
      }
    }
  }

  // tile t of chunk c: 256 values, row-major, at partials[c * chunk_elems + 256 t]; the vector sums behind the tiles
  T* part = (T*)a.partials + chunk * a.chunk_elems;
#pragma unroll
  for (int i = 0; i < kTilesPerWave; ++i) {
    if (have[i]) {
      T* tile = part + (size_t)(group * kTilesPerGroup + i * kWaves + wave) * 256;
#pragma unroll
      for (int q = 0; q < 4; ++q) tile[MF::row(g, q) * 16 + l] = acc[i][q];
    }
  }
  if (group == 0) {
    T* pv = part + (size_t)a.tiles * 256;
    for (int e = tid; e < a.vec_pad; e += kThreads) pv[e] = vsum[e];
  }
}

// out[c * ld + r] = (T)f(r, c) for r < R (the contiguous dimension), c < C, by the threads gtid of gsize: 16 bytes per lane where `vec` allows
template <typename T, typename F>
__device__ __forceinline__ void store_matrix(T* out, int ld, int R, int C, bool vec, long long gtid, long long gsize, F f) {
  constexpr int VN = Vec<T>::N;
  if (vec) {
    const int rv = (R + VN - 1) / VN;   // 16-byte pieces per column (the last one may be partial)
    for (long long e = gtid; e < (long long)rv * C; e += gsize) {
      const int c = (int)(e / rv), r0 = (int)(e - (long long)c * rv) * VN;
      T* dst = out + (size_t)c * ld + r0;
      if (r0 + VN <= R) {
        typename Vec<T>::type v;
        T* ve = reinterpret_cast<T*>(&v);
#pragma unroll
        for (int q = 0; q < VN; ++q) ve[q] = (T)f(r0 + q, c);
        *reinterpret_cast<typename Vec<T>::type*>(dst) = v;
      } else {
        for (int q = 0; r0 + q < R; ++q) dst[q] = (T)f(r0 + q, c);
      }
    }
  } else {
    for (long long e = gtid; e < (long long)R * C; e += gsize) {
      const int c = (int)(e / R), r = (int)(e - (long long)c * R);
      out[(size_t)c * ld + r] = (T)f(r, c);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void qp_moment_finish_kernel(const MomentArgs a, const int pass) {
  const SharedGradArgs& s = a.g;
  const mo_qp_grads& o = s.out;
  const long long gtid = (long long)blockIdx.x * kThreads + threadIdx.x, gsize = (long long)gridDim.x * kThreads;
  double* tot = a.totals;
  if (pass == 0) {   // every element of a chunk's block, summed over the chunks in their order
    const T* part = (const T*)a.partials;
    for (long long e = gtid; e < a.chunk_elems; e += gsize) {
      double sum = 0.0;
      for (long long c = 0; c < a.chunks; ++c) sum += (double)part[c * a.chunk_elems + e];
      tot[e] = sum;
    }
    return;
  }
  const int n = s.n, k = s.k, m = s.m, m_r = s.m_r, ntn = a.ntn;
  auto tile_at = [=](int first, int i, int j) { return tot[(size_t)(first + (i >> 4) * ntn + (j >> 4)) * 256 + (i & 15) * 16 + (j & 15)]; };
  auto M = [=](int i, int j) { return tile_at(0, i, j); };
  const double* sv = tot + (size_t)a.tiles * 256;   // [s_u | s_uy | s_uz | dcons_a]
  if (o.dG)   // (i, j) and (j, i) add the same two totals: symmetric to the bit
    store_matrix<T>((T*)o.dG, o.dG_ld, n, n, a.vec_dG != 0, gtid, gsize, [=](int i, int j) { return -0.5 * (M(i, j) + M(j, i)); });
  if (o.dA_eq && k > 0) {
    const int first = a.m_tiles, second = a.m_tiles + a.a_tiles;
    store_matrix<T>((T*)o.dA_eq, o.dA_ld, k, n, a.vec_dA != 0, gtid, gsize, [=](int i, int j) { return tile_at(first, i, j) - tile_at(second, i, j); });
  }
  if (o.dc)
    for (long long i = gtid; i < n; i += gsize) ((T*)o.dc)[i] = (T)-sv[i];
  if (o.db_eq)
    for (long long i = gtid; i < k; i += gsize) ((T*)o.db_eq)[i] = (T)-sv[n + i];
  if (o.dcons_b)
    for (long long i = gtid; i < m; i += gsize) ((T*)o.dcons_b)[i] = (T)-sv[n + k + i];
  if (o.dcons_a)
    for (long long i = gtid; i < m; i += gsize) {
      const int v = s.cons_var[i];
      ((T*)o.dcons_a)[i] = (v >= 0 && v < n) ? (T)sv[n + k + m + i] : (T)__builtin_nan("");   // F_ASSERT qp.cc:70-72, as mo_qp_gradients
    }
  if (o.dlambda && gtid == 0) {
    double tr = 0.0;
    for (int i = 0; i < n; ++i) tr += M(i, i);
    *(T*)o.dlambda = (T)-tr;
  }
  if (m_r > 0 && (o.dJ || o.dr)) {
    const T* J = (const T*)s.J;
    const int ld = s.J_ld, row_major = s.J_row_major;
    auto Jat = [=](int q, int i) { return (double)(row_major ? J[(size_t)q * ld + i] : J[(size_t)i * ld + q]); };
    if (o.dr)
      for (long long q = gtid; q < m_r; q += gsize) {
        double t = 0.0;
        for (int j = 0; j < n; ++j) t += Jat((int)q, j) * sv[j];
        ((T*)o.dr)[q] = (T)-t;
      }
    if (o.dJ) {
      const T* r = (const T*)s.r;
      const int qfirst = a.m_tiles + 2 * a.a_tiles, has_q = a.q_tiles > 0;
      auto dJ = [=](int q, int j) {   // -(J (M + M^T))[q][j] - Q[q][j]
        double t = 0.0;
        for (int i = 0; i < n; ++i) t += Jat(q, i) * (M(i, j) + M(j, i));
        return -t - (has_q ? tile_at(qfirst, q, j) : (double)r[q] * sv[j]);
      };
      if (o.dJ_layout == MO_ROW_MAJOR) store_matrix<T>((T*)o.dJ, o.dJ_ld, n, m_r, a.vec_dJ != 0, gtid, gsize, [=](int j, int q) { return dJ(q, j); });
      else store_matrix<T>((T*)o.dJ, o.dJ_ld, m_r, n, a.vec_dJ != 0, gtid, gsize, [=](int q, int j) { return dJ(q, j); });
    }
  }
}

// the LDS row stride: whole tiles, and 16 (fp32) or 32 (fp64) dwords modulo 64, so that the four problems of an operand read fall on
// different banks
int row_stride(int width, int elem) {
  const int want = elem == 8 ? 32 : 16;
  int S = width < 16 ? 16 : width;
  while ((S * (elem / 4)) % 64 != want) S += 16;
  return S;
}

// the moments the members of mo_qp_gradients_shared ask for
MomentNeeds needs_of(const SharedGradArgs& g) {
  const mo_qp_grads& o = g.out;
  MomentNeeds nd;
  nd.M = o.dG || o.dJ || o.dlambda;
  nd.A = o.dA_eq && g.k > 0;
  nd.Q = o.dJ && g.r_stride != 0;   // a shared r: Q = r s_u^T, formed by the finish kernel
  nd.y = g.k > 0 && (o.dA_eq || o.db_eq);
  nd.z = g.m > 0 && (o.dcons_a || o.dcons_b);
  return nd;
}

MomentArgs plan_of(const SharedGradArgs& g, const MomentNeeds& nd, int elem, int num_cus) {
  MomentArgs a;
  memset(&a, 0, sizeof(a));
  a.g = g;
  const mo_qp_grads& o = g.out;
  const int n = g.n, k = g.k, m = g.m, m_r = g.m_r;
  a.ntn = (n + 15) / 16;
  a.m_tiles = nd.M ? a.ntn * a.ntn : 0;
  a.a_tiles = nd.A ? ((k + 15) / 16) * a.ntn : 0;
  a.has_r = nd.Q;
  a.q_tiles = a.has_r ? ((m_r + 15) / 16) * a.ntn : 0;
  a.tiles = a.m_tiles + 2 * a.a_tiles + a.q_tiles;
  a.vec = n + k + 2 * m;
  a.vec_pad = (a.vec + 15) & ~15;
  a.chunk_len = shared_grad_chunk_len(g.batch, num_cus);
  a.chunks = shared_grad_chunks(g.batch, num_cus);
  a.chunk_elems = (long long)a.tiles * 256 + a.vec_pad;
  a.has_y = nd.y;
  a.has_z = nd.z;
  int w = 0;
  auto seg = [&w](int len, bool present) { const int at = w; if (present) w += (len + 15) & ~15; return at; };
  a.off_x = seg(n, true); a.off_ux = seg(n, true);
  a.off_y = seg(k, a.has_y); a.off_uy = seg(k, a.has_y);
  a.off_z = seg(m, a.has_z); a.off_uz = seg(m, a.has_z);
  a.off_r = seg(m_r, a.has_r);
  a.S = row_stride(w, elem);
  a.stage = 4;
  for (int ps = 16; ps >= 4; ps >>= 1)
    if (((size_t)ps * a.S + a.vec_pad) * elem <= 48 * 1024) { a.stage = ps; break; }
  a.vec_dG = vec_ok(o.dG, 0, o.dG_ld, elem);
  a.vec_dA = vec_ok(o.dA_eq, 0, o.dA_ld, elem);
  a.vec_dJ = vec_ok(o.dJ, 0, o.dJ_ld, elem);
  const size_t part_bytes = ((size_t)a.chunks * a.chunk_elems * elem + 15) & ~(size_t)15;
  a.partials = g.workspace;
  a.totals = reinterpret_cast<double*>((char*)g.workspace + part_bytes);
  return a;
}

MomentArgs plan_of(const SharedGradArgs& g, int elem, int num_cus) { return plan_of(g, needs_of(g), elem, num_cus); }

size_t lds_of(const MomentArgs& a, int elem) { return ((size_t)a.stage * a.S + a.vec_pad) * elem; }

}  // namespace

size_t shared_grad_workspace_bytes(const SharedGradArgs& g, int elem_size, int num_cus) {
  const MomentArgs a = plan_of(g, elem_size, num_cus);
  return (((size_t)a.chunks * a.chunk_elems * elem_size + 15) & ~(size_t)15) + (size_t)a.chunk_elems * sizeof(double);
}

size_t shared_grad_lds_bytes(const SharedGradArgs& g, int elem_size) { return lds_of(plan_of(g, elem_size, 1), elem_size); }

// stage 1: a workgroup per (chunk, group of tiles); none for an empty batch
static hipError_t launch_moments(const MomentArgs& a, int dtype, size_t lds, hipStream_t stream) {
  if (a.chunks <= 0) return hipSuccess;
  const int groups = (a.tiles + kTilesPerGroup - 1) / kTilesPerGroup;   // (none: group 0 still owns the column sums)
  const dim3 grid((unsigned)a.chunks, (unsigned)(groups > 0 ? groups : 1));
  if (dtype == MO_F64) hipLaunchKernelGGL(qp_moment_kernel<double>, grid, dim3(kThreads), lds, stream, a);
  else hipLaunchKernelGGL(qp_moment_kernel<float>, grid, dim3(kThreads), lds, stream, a);
  return hipGetLastError();
}

MomentLayout shared_moment_layout(const SharedGradArgs& g, const MomentNeeds& needs, int elem_size, int num_cus) {
  const MomentArgs a = plan_of(g, needs, elem_size, num_cus);
  MomentLayout l;
  l.ntn = a.ntn; l.m_tiles = a.m_tiles; l.a_tiles = a.a_tiles; l.tiles = a.tiles; l.vec_pad = a.vec_pad;
  l.chunks = a.chunks; l.chunk_elems = a.chunk_elems;
  return l;
}

size_t shared_moment_lds_bytes(const SharedGradArgs& g, const MomentNeeds& needs, int elem_size) {
  return lds_of(plan_of(g, needs, elem_size, 1), elem_size);
}

hipError_t launch_qp_moments(const SharedGradArgs& g, const MomentNeeds& needs, int dtype, int num_cus, hipStream_t stream) {
  const int elem = dtype == MO_F64 ? 8 : 4;
  const MomentArgs a = plan_of(g, needs, elem, num_cus);
  const size_t lds = lds_of(a, elem);
  if (lds > 64 * 1024) return hipErrorInvalidValue;   // (mo_qp_gradients_blocks_shared refuses such shapes with its own message)
  return launch_moments(a, dtype, lds, stream);
}

hipError_t launch_qp_gradients_shared(const SharedGradArgs& g, int dtype, int num_cus, hipStream_t stream) {
  const int elem = dtype == MO_F64 ? 8 : 4;
  const MomentArgs a = plan_of(g, elem, num_cus);
  const size_t lds = lds_of(a, elem);
  if (lds > 64 * 1024) return hipErrorInvalidValue;   // (mo_qp_gradients_shared refuses such shapes with its own message)
  if (hipError_t e = launch_moments(a, dtype, lds, stream)) return e;
  // pass 0: one thread per workspace element of a chunk; pass 1: one thread per 16-byte piece (or element) of the largest output
  long long work0 = (a.chunk_elems + kThreads - 1) / kThreads;
  long long largest = (long long)g.n * g.n;
  if (g.out.dJ && (long long)g.m_r * g.n > largest) largest = (long long)g.m_r * g.n;
  long long work1 = (largest + kThreads - 1) / kThreads;
  const long long cap = (long long)num_cus * 8;
  for (int pass = 0; pass < 2; ++pass) {
    long long blocks = pass == 0 ? work0 : work1;
    blocks = blocks > cap ? cap : (blocks < 1 ? 1 : blocks);
    if (dtype == MO_F64) hipLaunchKernelGGL(qp_moment_finish_kernel<double>, dim3((unsigned)blocks), dim3(kThreads), 0, stream, a, pass);
    else hipLaunchKernelGGL(qp_moment_finish_kernel<float>, dim3((unsigned)blocks), dim3(kThreads), 0, stream, a, pass);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}

}  // namespace mo
