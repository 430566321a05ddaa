// mo_kernels.h -- internal launch interface between the C ABI (mo_api.hip) and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mini_opt_hip.h"

namespace mo {

enum Mode : int {
  MODE_LINEARIZE = 0,  // nonlinear.cc:182-189 (J^T J, J^T r)
  MODE_RESIDUAL = 1,   // qp.cc:391-437
  MODE_STEP = 2,       // qp.cc:391-420, 275-364, 485-507 on the caller's state
  MODE_ITERATE = 3,    // qp.cc:153-201
  MODE_SOLVE = 4,      // qp.cc:100-151
  MODE_RHS = 5,        // qp.cc:275-364 on the caller's state for the CALLER's right-hand side (mo_kkt_solve): no residual, no alpha
};

// Everything a kernel needs, passed by value (kernarg segment).
struct KernelArgs {
  int n, k, m, m_r;
  int mode;
  unsigned flags;  // MO_STEP_*
  long long batch;
  // problem
  const void* J; long long J_stride; int J_ld; int J_row_major;
  const void* r; long long r_stride;
  double lambda;
  const void* lambda_vec; long long lambda_vec_stride;  // per-problem damping, overrides lambda when non-NULL
  const void* G; long long G_stride; int G_ld;
  const void* c; long long c_stride;
  const void* A; long long A_stride; int A_ld;
  const void* b; long long b_stride;
  const int* cons_var; const void* cons_a; const void* cons_b; long long cons_stride;
  // state
  void* vars; long long vars_stride;
  const void* mu; long long mu_stride;
  double tau;
  int barrier_strategy;
  // outputs
  void* delta; long long delta_stride;
  void* alpha;     // [batch][2]
  int* status;     // [batch]
  void* ip_out;    // [batch][6]
  void* r_out; long long r_out_stride;  // MODE_RESIDUAL
  void* kkt_out;   // [batch][4]
  void* G_out; long long G_out_stride; int G_out_ld;  // MODE_LINEARIZE (also SOLVE scratch for J-level input)
  void* c_out; long long c_out_stride;
  void* half_sq_out; long long half_sq_stride;  // stride in elements (0 means 1)
  // MODE_SOLVE
  mo_solve_params sp;
  int* termination; int* num_iterations; void* iterations; void* lagrange;
  // MODE_SOLVE inside mo_nls_solve: problems whose word skip[p * skip_stride] is >= 0 have terminated and are left untouched
  const int* skip; long long skip_stride;
  long long skip_active;  // how many of them are still active (host-side count from the previous outer iteration; -1: unknown)
  // fused kernel: device work counter (plan-owned, zeroed on the launch stream before every launch)
  unsigned long long* ticket;
  int stagger;     // fused step kernel: start offset between the waves that share a SIMD, in units of 127 x 64 cycles (set by fused_launch from the selected FusedLaunch)
  int chain_prio;  // fused step kernel: s_setprio 1 while a wave is in the elimination / substitution chains
  int static_rounds;  // fused kernels: launches of at most this many problems per wave are split statically, round by round, with no ticket
                      // (mo_api.hip hands over -1 = "the launcher decides" or MO_FUSED_STATIC_ROUNDS; 0 = tickets always).  The grids are
                      // min(CUs, ceil(batch / 4)) workgroups, so that a small batch spreads one wave per SIMD over the CUs before any SIMD
                      // gets a second wave.  Measured: the 32-variable grid wins with static rounds at every batch up to
                      // 65 536 (21 rounds), the 64 grid and the fp32 128 grid up to ~8 rounds; beyond, tickets in guided chunks balance better.
  int no_tiny;     // MO_PLAN_NO_TINY: keep n + k <= 15 on the 32-variable tile grid (set by mo_api.hip from the plan flags)
  // generic kernel beyond its LDS-resident range: P x ldh workspace of H per workgroup of the persistent grid (plan-owned)
  void* H_work; long long H_work_stride;
  long long H_work_slots;   // workgroup slots behind H_work: the launch clamps its grid to it
  // diagnostics only (tools/phase_timer.hip builds kkt_fused.hip with MO_FUSED_STAMPS); NULL in the product
  unsigned long long* debug;
  // MODE_RHS (generic kernel only): the caller's right-hand side [batch][V]; the result goes to delta.  Appended behind every older field,
  // so the kernarg offsets the other modes read are what they were.
  const void* rhs; long long rhs_stride;
};

constexpr size_t kLdsBytes = 160 * 1024;   // the LDS of a gfx950 CU: what one workgroup of the LDS-resident kernels may use

// shape-generic LDS kernel (any n,k,m,m_r that fits LDS), kkt_generic.hip
size_t generic_lds_bytes(const KernelArgs& a, int elem_size);
hipError_t launch_generic(const KernelArgs& a, int dtype, int num_cus, hipStream_t stream);
// beyond n + k = 192 or the 160 KiB of LDS the generic kernel keeps H in a global workspace (blocked LDL^T, kkt_generic.hip "LARGE")
bool generic_needs_large(const KernelArgs& a, int elem_size);
size_t generic_large_lds_bytes(const KernelArgs& a, int elem_size);   // > 160 KiB: not even the vectors fit
size_t generic_large_workspace_elems(const KernelArgs& a);            // per workgroup
int generic_large_grid(const KernelArgs& a, int elem_size, int num_cus);
// QPNullSpaceSolver::Solve (qp.cc:679-729): pivoted Householder QR of A_eq^T, reduced Hessian, LLT; x -> a.delta, status -> a.status
hipError_t launch_nullspace(const KernelArgs& a, int dtype, int num_cus, hipStream_t stream);
size_t nullspace_lds_bytes(int n, int k, int m_r, int elem_size);

// mo_qp_covariance, qp_covariance.hip: C = scale Z (Z^T sym(G) Z)^-1 Z^T per problem, gathered by `sel`.  The same factorisation as the
// null-space solver carried one step further (triangular inverse, symmetric product, back-transform), in place in the LDS copy of G.
struct CovArgs {
  int n, k, q;
  long long batch;
  const void* G; long long G_stride; int G_ld;
  const void* A; long long A_stride; int A_ld;
  const int* sel;                                  // [q] shared by the batch, NULL: the identity (q = n)
  const void* scale; long long scale_stride;       // NULL: 1
  void* cov; long long cov_stride; int cov_ld;     // NULL: not written
  void* var; long long var_stride;                 // NULL: not written
  int* status;                                     // NULL: not written
};
size_t qp_covariance_lds_bytes(int n, int k, int q, int elem_size);
int qp_covariance_grid(int n, int k, int q, int elem_size, int num_cus);   // workgroups of the persistent grid before the clamp to the batch
hipError_t launch_qp_covariance(const CovArgs& a, int dtype, int num_cus, hipStream_t stream);

// QP::ComputeEigenvalueStats (qp.cc:12-16): {min, max, min |.|} of the eigenvalues of sym(G) per problem, eig_kernels.hip.  `work`: the plan's
// global workspace (one slot of work_slot_bytes per workgroup) for matrices beyond the LDS; out [batch][3] in the plan's dtype.
bool eig_needs_global(int n);
size_t eig_workspace_bytes(int n);
size_t eig_lds_bytes(int n, bool matrix_in_lds);
int eig_grid(int n, int num_cus);
hipError_t launch_qp_eig(const KernelArgs& a, int dtype, int num_cus, void* out, long long out_stride, void* work, size_t work_slot_bytes,
                         long long work_slots, hipStream_t stream);

// min(CUs, ceil(batch / problems_per_wg)) workgroups of a persistent grid, so that a small batch spreads one wave per SIMD over the CUs
// before any SIMD gets a second wave (static_rounds above).  The one formula of every fused launcher, fp32 included.
inline unsigned fused_grid(long long batch, int num_cus, int problems_per_wg = 4) {
  long long grid = num_cus;
  const long long need = (batch + problems_per_wg - 1) / problems_per_wg;
  if (grid > need) grid = need;
  if (grid < 1) grid = 1;
  return (unsigned)grid;
}

// fused single-wave MFMA kernels for fixed tile grids (fp64, its right-hand-side twins, fp32): mo_fused_select.h

// small per-problem kernels around the QP (LinearizeAndFillQP tail, EvaluateNonlinearErrors, ComputeQPCostDerivative), nls_kernels.hip
struct AuxArgs {
  int n, k, m, m_r;
  long long batch;
  const void* x; long long x_stride;                  // linearisation point / direction dx
  const void* J; long long J_stride; int J_ld; int J_row_major;
  const void* r; long long r_stride;
  const void* G; long long G_stride; int G_ld;
  const void* c; long long c_stride;
  const void* A; long long A_stride; int A_ld;
  const void* b; long long b_stride;                  // b_eq or r_eq
  const int* cons_var; const void* cons_a; const void* cons_b; long long cons_stride;
  double lambda; const void* lambda_vec; long long lambda_vec_stride;
  void* cons_b_out; long long cons_b_out_stride;
  int* cons_var_out; void* cons_a_out;                // optional per-problem copies of (variable, a), same stride as cons_b_out
  void* out2;                                         // [batch][2]
  void* quad_out;                                     // [batch]
  int* status;
};
hipError_t launch_shift_constraints(const AuxArgs& a, int dtype, hipStream_t stream);
hipError_t launch_nonlinear_errors(const AuxArgs& a, int dtype, hipStream_t stream);
hipError_t launch_cost_derivative(const AuxArgs& a, int dtype, hipStream_t stream);
hipError_t launch_nullspace_termination(const AuxArgs& a, hipStream_t stream);  // status[p] = status[p] != 0

// per-problem state machine of the batched SQP loop (mo_nls_solve), nls_kernels.hip; fp64 only
enum { NLS_SD_LAMBDA = 0, NLS_SD_PENALTY, NLS_SD_ALPHA, NLS_SD_DIRECTIONAL, NLS_SD_A2, NLS_SD_T2, NLS_SD_A1, NLS_SD_T1, NLS_SD = 8 };
enum { NLS_SI_TERM = 0, NLS_SI_STATE, NLS_SI_LS_RESULT, NLS_SI_NSTEPS, NLS_SI_NITER, NLS_SI = 8 };
struct NlsArgs {
  int n, k, m;
  long long batch;
  mo_nls_params prm;
  int iter, ls;                                    // outer / line-search iteration this launch belongs to
  double* vars; long long vars_stride;
  double* cand; long long cand_stride;
  const double* qp_vars; long long qp_vars_stride;  // [x | s | y | z] of the QP; dx = its x block
  const double* errors_pre;                         // [batch][2]
  const double* errors_step;                        // [batch][2]
  const double* deriv;                              // [batch][2]
  const double* quad;                               // [batch]
  const double* lagrange;                           // [batch][2]
  const int* qp_status; const int* qp_term; const int* qp_nit;
  double* sd; int* si;                              // [batch][NLS_SD], [batch][NLS_SI]
  double* iterations; int rec;                      // [batch][max_iterations][rec] or NULL
  int* termination; int* num_iterations; int* status;
  int* counters;                                    // [0] problems still in the line search, [1] problems still active
  double* step; long long step_stride; double* step_alpha;  // MO_RETRACT_CALLBACK: dx and alpha handed to the caller's retraction
  const int* user_exit;                             // SetUserExitCallback flags (NULL: none)
};
// device residual families (nls_kernels.hip); rows = -1 if (family, n, rows_hint) is not a valid combination
int residual_family_rows(int family, int n, int rows_hint);
hipError_t launch_residual_family(int family, int n, int rows, long long batch, int dtype, const void* prm, const void* x,
                                  long long x_stride, void* r, long long r_stride, void* J, long long J_stride, int J_ld,
                                  int row_major, hipStream_t stream);
hipError_t launch_nls_init(const NlsArgs& a, hipStream_t stream);
hipError_t launch_nls_begin_search(const NlsArgs& a, hipStream_t stream);
hipError_t launch_nls_search_step(const NlsArgs& a, hipStream_t stream);
hipError_t launch_nls_update(const NlsArgs& a, hipStream_t stream);
hipError_t launch_nls_user_exit(const NlsArgs& a, hipStream_t stream);

// residual-block input (mo_linearize_blocks / mo_jacobian_blocks), residual_blocks.hip.  The schedule is built on the host by
// mo_residual_layout_create and shared by every problem of the batch; all offsets index one problem's packed values / residual rows.
struct BlocksArgs {
  int n, rows;                // plan n, sum R_b
  long long values;           // sum R_b P_b: packed Jacobian length per problem
  long long batch;
  const int* g_ptr;           // [n * n + 1] CSR over the cells of G in column-major order (strict upper cells: empty lists)
  const int4* g_ent;          // {offset of J col a, offset of J col b, R_b, first stacked row of block b}: G(i, j) += J_a . J_b, in the reference's order
  const int* c_ptr;           // [n + 1]
  const int4* c_ent;          // {offset of J col a, offset of block b's rows in r, R_b, a's partner list in d_dup or -1}: c(i) += J_a . r_b
  const int2* row_info;       // [rows] {b * n, row within block b}
  const int* win;             // [num_blocks * n] offset of the column block b assigns to global column j (last wins), -1: none
  const void* J; long long J_stride;
  const void* r; long long r_stride;
  double lambda; const void* lambda_vec; long long lambda_vec_stride;
  void* G_out; long long G_out_stride; int G_out_ld;
  void* c_out; long long c_out_stride;
  void* half_sq_out;          // [batch] or NULL
  void* J_out; long long J_out_stride; int J_out_ld; int J_out_row_major;
  void* abs_sum_out;          // [batch] or NULL
  // mo_linearize_blocks_weighted (behind every older field): one weight per stacked row, NULL = unweighted; g_ent's fourth component is the
  // first stacked row of the entry's block (c_ent.y has it already)
  const void* weights; long long weights_stride;
  // mo_linearize_blocks_robust (behind every older field): the loss table in the plan's dtype, NULL = none.  The kernel forms the weights
  // itself (mo_loss_device.h), copies them to weights_out when given and writes 0.5 sum rho to half_sq_out[p * half_sq_stride]
  const int4* loss_blk;       // [loss_blocks] {first stacked row, R_b, kind, 0}
  const void* loss_scale;     // [loss_blocks]
  int loss_blocks;
  void* weights_out; long long weights_out_stride;
  long long half_sq_stride;   // read by the loss instantiations only
};
// whether the weighted / robust linearise of this layout goes through LDS: (values + 2 rows) elements within the stage budget
bool blocks_weighted_stages(long long values, int rows, int elem_size);

// mo_residual_loss_eval, residual_loss.hip: per block s_b, w_b = rho'(s_b) over the block's rows, 0.5 sum rho per problem
struct LossArgs {
  int num_blocks, rows;
  long long batch;
  const int4* blk;            // [num_blocks] {first stacked row, R_b, kind, 0}
  const void* scale;          // [num_blocks], the plan's dtype
  const void* r; long long r_stride;
  void* weights_out; long long weights_stride;   // NULL: not written
  void* rho_out; long long rho_stride;           // NULL: not written
};
hipError_t launch_residual_loss(const LossArgs& a, int dtype, int num_cus, hipStream_t stream);
hipError_t launch_blocks_linearize(const BlocksArgs& a, int dtype, int num_cus, hipStream_t stream);
hipError_t launch_blocks_jacobian(const BlocksArgs& a, int dtype, int num_cus, hipStream_t stream);

// gradients with respect to the packed block values (mo_qp_gradients_blocks / mo_qp_gradients_eq_blocks), residual_blocks.hip: the transpose
// of the gathers above applied to (x, u_x).  The schedule is built by mo_residual_layout_create beside the forward one.
struct BlockGradArgs {
  int n, k, m, rows;          // plan n, k, m; sum R_b of the layout
  long long values;
  long long batch;
  const int4* d_row;          // [rows] {offset of J_b[q, 0], R_b (the column stride), P_b, start of idx_b in d_idx}
  const int* d_idx;           // the concatenated index lists
  const int4* d_val;          // [values] {stacked row, global index, row within the block, start of the partner list in d_dup or -1}
  const int* d_dup;           // partner lists: {count, count x offset of J_b[0, q']}: the other local columns q' on the same variable
  const int2* e_val;          // [values] equality blocks: {stacked row, global index or -1 for a column that loses its global column}
  const void* J; long long J_stride;
  const void* r; long long r_stride;
  const void* vars; long long vars_stride;
  const void* u; long long u_stride;
  void* dJ; long long dJ_stride;
  void* dr; long long dr_stride;
  void* dlambda; long long dlambda_stride;
  // mo_qp_gradients_blocks_weighted (behind every older field): NULL weights = unweighted
  const void* weights; long long weights_stride;
  void* dw; long long dw_stride;
  const int* d_pair;          // [rows] start of the row's block's pair list in d_plist, -1: the block repeats no variable
  const int* d_plist;         // pair lists: {count, count x {p R_b, p' R_b, variable}}: the pairs p' < p of local columns on one variable
};
bool blocks_grad_fits(int n, int rows, int elem_size, bool weighted = false);   // the vectors the kernel keeps in LDS (x, u_x, t, w; the weights) within 63 KiB
hipError_t launch_blocks_grad(const BlockGradArgs& a, int dtype, int num_cus, hipStream_t stream);
hipError_t launch_blocks_eq_grad(const BlockGradArgs& a, int dtype, int num_cus, hipStream_t stream);

// what the two dense sensitivity kernels read of the plan and the problem (filled by sens_args of mo_api.hip).  Inputs that are not needed
// may be NULL: J only for the dJ / dr members (m_r = 0 otherwise), r as each kernel says, cons_var only for the dcons_a member.
struct SensArgs {
  int n, k, m, m_r;
  long long batch;
  const void* vars; long long vars_stride;   // [batch][V]
  const void* J; long long J_stride; int J_ld; int J_row_major;
  const void* r; long long r_stride;
  const int* cons_var; long long cons_stride;
};

// gradients of a loss through the solution of a QP (mo_qp_gradients), qp_grad.hip: rank-2 updates of the state v = [x | s | y | z] and the
// adjoint u = K^-T g.  r comes with J.
struct GradArgs : SensArgs {
  mo_qp_grads out;                           // NULL members are neither computed nor written
  const void* u; long long u_stride;         // [batch][V]  (behind `out`: the kernel's scalar loads stay closest to the ones it had)
};
size_t qp_grad_lds_bytes(const GradArgs& a, int elem_size);
hipError_t launch_qp_gradients(const GradArgs& a, int dtype, int num_cus, hipStream_t stream);

// the same gradients SUMMED over the batch, for data the whole batch shares (mo_qp_gradients_shared), qp_grad_shared.hip: moments of
// (x, u_x), (y, u_x), (u_y, x), (r, u_x) per chunk of problems on the matrix cores, then one pass over the chunk partials.  `out` is one
// instance per member (its strides are not read).  J only for dJ / dr (stride 0), r only for dJ, cons_var only for dcons_a (stride 0).
struct SharedGradArgs : GradArgs {
  const int* status_fwd; const int* status_adj;   // either may be NULL; a problem counts iff every given word is MO_STATUS_OK
  void* workspace;                                // shared_grad_workspace_bytes, 16-byte aligned
};
// chunks of consecutive problems, each summed by its own workgroups: a function of (batch, CU count) alone, so that the order of every sum --
// and with it every bit of the result -- is the same on every launch of one device
inline long long shared_grad_chunk_len(long long batch, int num_cus) {   // problems per chunk (the last chunk may be shorter)
  long long c = (batch + 31) / 32;                  // at least 32 problems a chunk, at most one chunk per CU
  if (c > num_cus) c = num_cus;
  if (c < 1) c = 1;
  const long long len = (batch + c - 1) / c;
  return len < 1 ? 1 : len;
}
inline long long shared_grad_chunks(long long batch, int num_cus) {
  const long long len = shared_grad_chunk_len(batch, num_cus);
  return (batch + len - 1) / len;                   // 0 for an empty batch
}
size_t shared_grad_workspace_bytes(const SharedGradArgs& a, int elem_size, int num_cus);
size_t shared_grad_lds_bytes(const SharedGradArgs& a, int elem_size);
hipError_t launch_qp_gradients_shared(const SharedGradArgs& a, int dtype, int num_cus, hipStream_t stream);

// stage 1 alone -- qp_moment_kernel -- for a caller with a finish of its own (the block form below).  MomentNeeds names the tile families and
// vector sums to accumulate instead of deriving them from `out`; Q (with r, r_stride and m_r of the args) is the dense form's.
struct MomentNeeds { int M, A, Q, y, z; };   // M = u_x x^T; A1 = y u_x^T and A2 = u_y x^T; Q = r u_x^T; s_uy; s_uz and dcons_a
// how the chunk partials lie at `workspace`: chunk c's block of chunk_elems values = `tiles` row-major 16 x 16 tiles -- M (ntn x ntn of them,
// row-major over (tile row, tile column)), then A1, then A2 (a_tiles each) -- and the vector sums [s_u n | s_uy k | s_uz m | dcons_a m]
struct MomentLayout {
  int ntn, m_tiles, a_tiles, tiles, vec_pad;
  long long chunks, chunk_elems;
};
MomentLayout shared_moment_layout(const SharedGradArgs& a, const MomentNeeds& needs, int elem_size, int num_cus);
size_t shared_moment_lds_bytes(const SharedGradArgs& a, const MomentNeeds& needs, int elem_size);
hipError_t launch_qp_moments(const SharedGradArgs& a, const MomentNeeds& needs, int dtype, int num_cus, hipStream_t stream);

// the gradients of the packed blocks SUMMED over the batch, for blocks the whole batch shares (mo_qp_gradients_blocks_shared),
// qp_grad_blocks_shared.hip: the moments above, the packed Q = sum r_p[row] u_x,p[index] per chunk, and a finish that gathers through the
// layouts' backward schedules.  J is ONE instance; r is per problem (r_stride != 0: read by the Q kernel) or one instance too.
struct BlockSharedArgs {
  int n, k, m, rows;          // plan n, k, m; sum R_b of the cost layout
  long long values, eq_values;
  long long batch;
  const int4* d_row; const int* d_idx; const int4* d_val; const int* d_dup;   // cost layout (BlockGradArgs)
  const int2* e_val;          // equality layout: {stacked row, global index or -1}
  const void* J;
  const void* r; long long r_stride;
  const void* vars; long long vars_stride;
  const void* u; long long u_stride;
  const int* status_fwd; const int* status_adj;
  mo_block_shared_grads out;  // NULL members are neither computed nor written
  void* workspace;            // blocks_shared_workspace_bytes, 16-byte aligned
};
size_t blocks_shared_workspace_bytes(const BlockSharedArgs& a, int elem_size, int num_cus);
bool blocks_shared_fits(const BlockSharedArgs& a, int elem_size);   // the LDS rule of mo_qp_gradients_blocks_shared
hipError_t launch_blocks_shared_grad(const BlockSharedArgs& a, int dtype, int num_cus, hipStream_t stream);

// forward-mode right-hand side rho = F_theta thetadot of a QP (mo_qp_tangent_rhs), qp_tangent.hip: the transpose of the gradient kernel
// above.  r is read only against the dJ tangent, cons_var whenever the problem has one.
struct TangentArgs : SensArgs {
  mo_qp_tangents t;                          // NULL members are zero tangents
  void* rho; long long rho_stride;           // [batch][V]
};
size_t qp_tangent_lds_bytes(const TangentArgs& a, int elem_size);
hipError_t launch_qp_tangent(const TangentArgs& a, int dtype, int num_cus, hipStream_t stream);

// the same right-hand side for residual-block input (mo_qp_tangent_rhs_blocks), qp_tangent_blocks.hip: the transpose of blocks_grad_kernel
// and blocks_eq_grad_kernel, from the packed tangents alone.  The schedules are those of the two layouts (mo_residual_layout_create).
struct BlockTangentArgs {
  int n, k, m, rows;          // plan n, k, m; sum R_b of the cost layout
  long long values;           // packed cost values per problem
  long long batch;
  const int4* d_row;          // cost layout: [rows] {offset of J_b[q, 0], R_b, P_b, start of idx_b in d_idx}
  const int* d_idx;
  const int* d_dup;           // partner lists: {count, count x offset of J_b[0, q']}
  const int* c_ptr;           // [n + 1] per variable i, in the layout's order:
  const int4* c_ent;          // {offset of J_b[0, p], first stacked row of block b, R_b, start of p's partner list in d_dup or -1} per local column p on i
  const int4* e_row;          // equality layout (NULL without one): its d_row, [k]
  const int2* e_val;          // its e_val: {stacked row, global index or -1 for a column that loses its global column}
  const int* w_ptr;           // [n + 1] its c_ptr / c_ent filtered by winners: the columns that reach A_eq
  const int4* w_ent;
  const void* J; long long J_stride;   // read only with dJ_blocks or dr
  const void* r; long long r_stride;   // read only with dJ_blocks
  const void* vars; long long vars_stride;
  const int* cons_var; long long cons_stride;
  mo_block_tangents t;        // NULL members are zero tangents
  void* rho; long long rho_stride;
  // mo_qp_tangent_rhs_blocks_weighted (behind every older field): NULL weights = unweighted; dw the tangent of the weights (NULL: zero)
  const void* weights; long long weights_stride;
  const void* dw; long long dw_stride;
};
size_t blocks_tangent_lds_bytes(int n, int k, int m, int rows, int elem_size, bool weighted = false);   // the vectors the kernel always keeps in LDS
bool blocks_tangent_fits(int n, int k, int m, int rows, int elem_size, bool weighted = false);          // ... within 64 KiB
hipError_t launch_blocks_tangent(const BlockTangentArgs& a, int dtype, int num_cus, hipStream_t stream);

// the gradients of the weighted block cost SUMMED over the batch, for ONE instance of the packed blocks under weights and residuals per
// problem (mo_qp_gradients_blocks_weighted_shared), qp_grad_blocks_wshared.hip: t = J x_loc + r and s = J u_loc per problem on chip, the
// packed sums per chunk, and a finish through the layout's backward schedules.  No moments: the weights keep the sums from factoring.
struct BlockWSharedArgs {
  int n, k, m, rows;          // plan n, k, m; sum R_b of the cost layout
  long long values;
  long long batch;
  const int4* d_row; const int* d_idx; const int4* d_val; const int* d_dup; const int* d_pair; const int* d_plist;   // cost layout (BlockGradArgs)
  int has_dup;                // the layout's partner / pair lists are non-empty
  const void* J;              // ONE instance
  const void* r; long long r_stride;
  const void* weights; long long weights_stride;
  const void* vars; long long vars_stride;
  const void* u; long long u_stride;
  const int* status_fwd; const int* status_adj;
  mo_block_weighted_shared_grads out;   // NULL members are neither computed nor written
  void* workspace;            // blocks_wshared_workspace_bytes, 16-byte aligned
};
size_t blocks_wshared_workspace_bytes(const BlockWSharedArgs& a, int elem_size, int num_cus);
bool blocks_wshared_fits(const BlockWSharedArgs& a, int elem_size);   // the LDS rule of mo_qp_gradients_blocks_weighted_shared
hipError_t launch_blocks_wshared_grad(const BlockWSharedArgs& a, int dtype, int num_cus, hipStream_t stream);

}  // namespace mo
