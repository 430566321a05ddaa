/*
 * mini_opt_hip.h -- C ABI of the MI355X-native batched interior-point Newton-step solver.
 *
 * This is the drop-in boundary for mini_opt's dense KKT hot path (source/qp.cc).  The reference has no FFI:
 * its boundary is the C++ class API (include/mini_opt/qp.hpp:132-205, residual.hpp:28-117,
 * nonlinear.hpp:33-52,127-157).  Each entry point below names the reference member function(s) it replaces;
 * INTEGRATION.md shows the binding a mini_opt maintainer would add inside QPInteriorPointSolver /
 * ConstrainedNonlinearLeastSquares, and mini_opt_amd/cpp/ holds the C++ facade that mirrors those classes.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no exceptions across the boundary.  Every call returns an int:
 *    MO_OK (0) or a negative MO_ERR_* (the reference's F_ASSERT / assert::default_error cases,
 *    assertions.hpp:68-73).  Per-problem numeric failures never abort the batch: they are written to the
 *    caller's `status[batch]` array (MO_STATUS_*), mirroring the reference's two exceptions.
 *  - All data pointers are DEVICE pointers on the plan's GPU (caller-owned).  The plan owns only scratch.
 *  - A "batch" is `batch` independent QPs of identical dimensions (n, k, m, m_r).  Problem p of tensor X lives at
 *    X + p * X_stride (strides in ELEMENTS; stride 0 = one instance shared by the whole batch).
 *  - Matrices G (n x n, only the lower triangle is read -- qp.cc:289, :404) and A_eq (k x n) are COLUMN-MAJOR
 *    with a leading dimension, exactly Eigen's default, so `MatrixXd::data()` can be passed unchanged.
 *    The stacked Jacobian J (m_r x n; the reference never materialises it -- residual.hpp:198-224 accumulates
 *    J^T J residual by residual) is ROW-MAJOR by default (each residual appends its rows); column-major is
 *    accepted via J_layout.
 *  - State / residual / delta vectors use the reference block order [x(n) | s(m) | y(k) | z(m)]
 *    (qp.cc:36-42, 548-582); V = n + 2m + k.
 *  - dtype MO_F64 is the reference's arithmetic (qp.hpp:15: double only); MO_F32 is the BASELINE.json cfg-4
 *    extension: every floating-point tensor (incl. mu, alpha, ip records) is then float.
 *  - Thread-safety: a plan may be used from one host thread -- and one stream -- at a time (it owns the device work counter
 *    of the fused kernels and the scratch of mo_qp_solve); distinct plans are independent.
 *    Multi-GPU = one plan (and one process or thread) per device; there is no cross-device traffic.
 */
#ifndef MINI_OPT_HIP_H_
#define MINI_OPT_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MO_VERSION_MAJOR 0
#define MO_VERSION_MINOR 5

/* return codes */
#define MO_OK 0
#define MO_ERR_INVALID_ARGUMENT (-1) /* null pointer, bad enum, bad params (CheckParams qp.cc:76-82) */
#define MO_ERR_DIMENSION (-2)        /* dimension mismatch (Setup asserts, qp.cc:24-34) */
#define MO_ERR_UNSUPPORTED (-3)      /* unknown dtype; state / residual vectors of one problem beyond the 160 KiB of LDS (n in the thousands) ... */
#define MO_ERR_HIP (-4)              /* a HIP runtime call failed; see mo_last_error() */
#define MO_ERR_NO_DEVICE (-5)        /* no usable gfx950 device: the HIP path never falls back to the CPU */

/* per-problem status words */
#define MO_STATUS_OK 0
#define MO_STATUS_NONPOSITIVE_SLACK 1    /* some s <= 0 at factorisation time (F_ASSERT qp.cc:285) */
#define MO_STATUS_FACTORIZATION_FAILED 2 /* FailedFactorization (qp.cc:303-307, qp.hpp:331-333) */
#define MO_STATUS_NONFINITE 3            /* the computed direction contains NaN/Inf */
#define MO_STATUS_BAD_INDEX 4            /* constraint variable index outside [0,n) (F_ASSERT qp.cc:70-72) */
#define MO_STATUS_NOT_POSITIVE_DEFINITE 5 /* mo_nullspace_solve: QPNullSpaceTerminationState::NOT_POSITIVE_DEFINITE (qp.cc:711-713) */

typedef enum { MO_F64 = 0, MO_F32 = 1 } mo_dtype;
typedef enum { MO_COL_MAJOR = 0, MO_ROW_MAJOR = 1 } mo_layout;

/* BarrierStrategy (structs.hpp:24-31), InitialGuessMethod (structs.hpp:34-41), termination (structs.hpp:97-102) */
typedef enum { MO_COMPLEMENTARITY = 0, MO_FIXED_DECREASE = 1, MO_PREDICTOR_CORRECTOR = 2 } mo_barrier_strategy;
typedef enum { MO_GUESS_NAIVE = 0, MO_GUESS_SOLVE_EQUALITY_CONSTRAINED = 1, MO_GUESS_USER_PROVIDED = 2 } mo_initial_guess;
typedef enum { MO_SATISFIED_KKT_TOL = 0, MO_MAX_ITERATIONS = 1 } mo_termination;

/* plan flags */
#define MO_PLAN_FORCE_GENERIC 1u /* always use the shape-generic LDS kernel (testing / A-B measurements) */
#define MO_PLAN_NO_TINY 2u       /* do not use the one-tile kernels for n + k <= 15 (testing / A-B: the 32-variable tile grid instead) */
/* How the fused kernels hand out problems to the waves of their persistent grid.  Default: launches of a few problems per wave are split
 * statically, larger ones take tickets from a device counter in guided chunks.  The two flags pin one scheme for every launch of the plan
 * (testing: the suite's small batches would otherwise never take a ticket). */
#define MO_PLAN_TICKETS_ALWAYS 4u
#define MO_PLAN_STATIC_ROUNDS_ALWAYS 8u

typedef struct {
  int32_t n;   /* variables (QPInteriorPointSolver::dims_.N, qp.cc:37) */
  int32_t k;   /* equality rows (dims_.K) */
  int32_t m;   /* LinearInequalityConstraint entries (dims_.M); a two-sided box is two entries */
  int32_t m_r; /* stacked residual rows for J-level input; 0 if only QP-level (G, c) input is used */
  int32_t dtype;  /* mo_dtype */
  int32_t device; /* HIP device ordinal */
  uint32_t flags; /* MO_PLAN_* */
  int32_t reserved;
  int64_t max_batch; /* sizes plan-owned scratch: the (G, c) of mo_qp_solve with J-level input on the generic kernel; beyond the
                        LDS-resident range of the generic kernel (n + k >= 72 since round 4) also the number of H workspaces
                        mo_plan_create allocates (0: one per workgroup of the full persistent grid) */
} mo_plan_desc;

typedef struct mo_plan mo_plan; /* opaque; replaces the solver-owned scratch of qp.hpp:221-231 */

/* One batch of QPs (mini_opt::QP, qp.hpp:104-124) or of linearised least-squares problems
 * (ConstrainedNonlinearLeastSquares::LinearizeAndFillQP, nonlinear.cc:170-214).
 * Cost: give EITHER (J, r, lambda) -- then G = J^T J + lambda I (lower) and c = J^T r are formed on device
 * (residual.hpp:206-224 summed, nonlinear.cc:187-189) -- OR (G, c).  J == NULL selects (G, c). */
typedef struct {
  const void* J;      int64_t J_stride; int32_t J_ld; int32_t J_layout; /* m_r x n */
  const void* r;      int64_t r_stride;                                /* m_r */
  double lambda;                                                      /* Levenberg-Marquardt damping, added iff > 0 */
  const void* G;      int64_t G_stride; int32_t G_ld; int32_t reserved0; /* n x n col-major, lower read */
  const void* c;      int64_t c_stride;                                /* n */
  const void* A_eq;   int64_t A_stride; int32_t A_ld; int32_t reserved1; /* k x n col-major (NULL iff k == 0) */
  const void* b_eq;   int64_t b_stride;                                /* k */
  const int32_t* cons_var; const void* cons_a; const void* cons_b; int64_t cons_stride; /* m each: a*x[var]+b >= 0 */
  const void* lambda_vec; int64_t lambda_stride; /* optional per-problem damping (the lambda state of nonlinear.cc:92-96);
                                                    overrides `lambda` when non-NULL */
} mo_problem;

/* QPInteriorPointSolver::Params (qp.hpp:134-164); mo_default_solve_params fills the reference defaults. */
typedef struct {
  double initial_mu;
  double sigma;
  double termination_kkt_tol;
  double termination_complementarity_tol;
  int32_t max_iterations;
  int32_t barrier_strategy;                 /* mo_barrier_strategy */
  int32_t decrease_mu_only_on_small_error;
  int32_t initial_guess_method;             /* mo_initial_guess */
  int32_t initialize_mu_with_complementarity;
  int32_t reserved;
} mo_solve_params;

/* Records are arrays of the plan's scalar type, laid out as:
 *   KKTError (structs.hpp:68-78)            kkt[4]  = {r_dual, r_comp, r_primal_eq, r_primal_ineq}
 *   IPIterationOutputs (structs.hpp:53-64)  ip[6]   = {mu, alpha.primal, alpha.dual, alpha_probe.primal,
 *                                                      alpha_probe.dual, mu_affine}   (NaN where the reference has NaN)
 *   QPInteriorPointIteration (:81-94)       iter[14] = {kkt_initial[4], kkt_final[4], ip[6]}
 */
#define MO_KKT_RECORD 4
#define MO_IP_RECORD 6
#define MO_ITER_RECORD 14

/* step flags */
#define MO_STEP_NO_INEQUALITIES 1u    /* EvaluateKKTConditions(false) + ComputeLDLT(false) + SolveForUpdateNoInequalities
                                         (qp.cc:366-386, used by the initial guess :455-460): only dx, dy are written,
                                         ds = dz = 0, alpha = 1 */
#define MO_STEP_PREDICTOR_CORRECTOR 2u /* mo_iterate only: the Mehrotra double solve of qp.cc:170-187 */
#define MO_KKT_TRANSPOSE 4u            /* mo_kkt_solve only: solve K^T u = rhs instead of K delta = -rhs */

const char* mo_version_string(void);
const char* mo_status_string(int32_t status);
/* Message of the last failing call on this host thread ("" if none). */
const char* mo_last_error(void);

void mo_default_solve_params(mo_solve_params* params);

/* Replaces QPInteriorPointSolver::Setup (qp.cc:20-73): validates dimensions, selects kernels, allocates scratch. */
int mo_plan_create(const mo_plan_desc* desc, mo_plan** plan);
int mo_plan_destroy(mo_plan* plan);
/* Name of the kernel variant mo_newton_step will launch for this plan and problem layout ("generic", "fused_n64", ...). */
const char* mo_plan_step_kernel(const mo_plan* plan, const mo_problem* prob);
/* The same for mo_qp_solve / mo_iterate / mo_kkt_residual ("generic", "fused_solve_mfma_f64_n64", "fused_solve_mfma_f32_n128", ...). */
const char* mo_plan_solve_kernel(const mo_plan* plan, const mo_problem* prob);
/* The same for mo_kkt_solve: "generic", or the right-hand-side twin of the fused fp64 step kernel, "fused_rhs_mfma_f64_n32|64|96|128" for
 * J-level and "fused_rhs_qp_f64_n32|64|96|128" for (G, c) input (the coverage rule stands above mo_kkt_solve). */
const char* mo_plan_kkt_solve_kernel(const mo_plan* plan, const mo_problem* prob);

/* Replaces LinearizeAndFillQP's cost part (nonlinear.cc:182-189; Residual::Model::UpdateHessian, residual.hpp:186-226):
 * G_out (n x n col-major, leading dim G_ld; lower triangle written, strict upper written as 0) = J^T J + lambda I,
 * c_out = J^T r, half_sq_out[p] = 0.5 |r|^2 (may be NULL). */
int mo_linearize(mo_plan* plan, const mo_problem* prob, int64_t batch, void* G_out, int64_t G_stride, int32_t G_ld,
                 void* c_out, int64_t c_stride, void* half_sq_out, void* stream);

/* QP::ComputeEigenvalueStats (qp.hpp:122-123, qp.cc:12-16): out[p] = {min, max, min |.|} of the eigenvalues of the QP Hessian of problem p
 * (QPEigenvalues, structs.hpp:267-275) -- of sym(G) from the lower triangle of (G, c) input, as Eigen's SelfAdjointEigenSolver reads it, or of
 * G = J^T J + lambda I for (J, r, lambda) input (what LinearizeAndFillQP hands the reference's QP, nonlinear.cc:182-189).  Any n the plan
 * accepts; computed in fp64 (Householder tridiagonalisation + Sturm-count multisection), written in the plan's dtype.  out: [batch][3].
 * Non-finite input: a NaN or +-inf among the entries read -- the lower triangle of G (the strict upper triangle is never read), any entry of
 * J, or a J^T J that overflows -- makes the three outputs of THAT problem NaN, as SelfAdjointEigenSolver propagates it; the other problems of
 * the batch are not affected.  A NaN (or negative) lambda acts as 0, like the reference's `if (lambda > 0)`.
 * Scaling: the matrix is scaled by the exact power of two that brings its largest |entry| into [1, 2) and the results are scaled back, so
 * 2^s G gives 2^s times the results of G, bit for bit, as long as the results neither overflow nor become subnormal in the plan's dtype. */
int mo_qp_eigenvalue_stats(mo_plan* plan, const mo_problem* prob, int64_t batch, void* out, void* stream);

/* Replaces the whole of LinearizeAndFillQP (nonlinear.cc:170-214) for dense residual stacks.  The caller hands over the cost
 * stack (J, r, lambda[_vec]) and -- as prob->A_eq / prob->b_eq -- the equality residuals' Jacobian and values at the
 * linearisation point x (UpdateJacobian, residual.hpp:230-250, is a plain copy for a dense stack), plus the problem's
 * UNSHIFTED inequality constraints.  Written: G_out / c_out as mo_linearize; cons_b_out[m] = a * x[var] + b
 * (LinearInequalityConstraint::ShiftTo, qp.hpp:57-65); errors_out[p] = {f = 0.5 |r|^2, equality = |b_eq|_1}
 * (Errors, structs.hpp:169-186); status[p] = MO_STATUS_BAD_INDEX for a constraint variable outside [0, n). */
int mo_fill_qp(mo_plan* plan, const mo_problem* prob, int64_t batch, const void* x, int64_t x_stride, void* G_out,
               int64_t G_stride, int32_t G_ld, void* c_out, int64_t c_stride, void* cons_b_out, int64_t cons_b_stride,
               void* errors_out, int32_t* status, void* stream);

/* Replaces EvaluateNonlinearErrors (nonlinear.cc:279-293) for dense residual stacks evaluated by the caller:
 * errors_out[p] = {0.5 |r|^2, |r_eq|_1}.  r: m_r values per problem, r_eq: k values per problem (NULL iff k == 0). */
int mo_nonlinear_errors(mo_plan* plan, const void* r, int64_t r_stride, const void* r_eq, int64_t r_eq_stride,
                        int64_t batch, void* errors_out, void* stream);

/* Replaces ComputeQPCostDerivative (nonlinear.cc:452-483): deriv_out[p] = {d_f = c^T dx, d_equality = sum_i sign(b_eq_i)
 * (A_eq dx)_i} (DirectionalDerivatives, structs.hpp:189-203).  With J-level input c^T dx is evaluated as r^T (J dx).
 * quad_out[p] (may be NULL) = dx^T G dx, the curvature term SelectPenalty needs (nonlinear.cc:496-498). */
int mo_qp_cost_derivative(mo_plan* plan, const mo_problem* prob, int64_t batch, const void* dx, int64_t dx_stride,
                          void* deriv_out, void* quad_out, void* stream);

/* Replaces EvaluateKKTConditions (qp.cc:391-420) + ComputeErrors (qp.cc:423-437):
 * r_out [V] = [r_d | r_comp | r_pe | r_pi] (mu NOT applied, as in the reference), kkt_out [4] (may be NULL) with mu[p]. */
int mo_kkt_residual(mo_plan* plan, const mo_problem* prob, int64_t batch, const void* vars, int64_t vars_stride,
                    const void* mu, int64_t mu_stride, uint32_t flags, void* r_out, int64_t r_stride, void* kkt_out,
                    void* stream);

/* THE HOT PATH.  One dense KKT Newton step per problem on the caller's state; replaces the sequence
 *   EvaluateKKTConditions (qp.cc:391-420) -> ComputeLDLT (qp.cc:275-316) -> SolveForUpdate(mu) (qp.cc:318-364)
 *   -> ComputeAlpha(tau) (qp.cc:485-507)
 * (what qp_test.cc:132-134 calls through `friend`), including the J^T J assembly when J-level input is given.
 * The direction is obtained by a direct LDL^T solve; the reference's explicit inverse (qp.cc:310-311) is not formed.
 *   vars  [batch][V]  in   strictly interior state (s > 0)
 *   mu    per-problem barrier parameter (mu_stride 0: one shared value); ignored (0) if m == 0 (qp.cc:165-167)
 *   delta [batch][V]  out  [dx | ds | dy | dz]   (NaN-filled for problems whose status != 0)
 *   alpha [batch][2]  out  {primal, dual} step lengths (may be NULL)
 *   status[batch]     out  MO_STATUS_* (may be NULL) */
int mo_newton_step(mo_plan* plan, const mo_problem* prob, int64_t batch, const void* vars, int64_t vars_stride,
                   const void* mu, int64_t mu_stride, double tau, uint32_t flags, void* delta, int64_t delta_stride,
                   void* alpha, int32_t* status, void* stream);

/* Replaces QPInteriorPointSolver::Iterate (qp.cc:153-201): Newton step (optionally predictor-corrector,
 * qp.cc:170-187 with ComputePredictorCorrectorMuAffine :519-537), ComputeAlpha(0.995), and the state update
 * x,s += alpha_p (dx,ds); y,z += alpha_d (dy,dz) IN PLACE in vars.  ip_out [batch][6] (may be NULL),
 * delta (may be NULL). */
int mo_iterate(mo_plan* plan, const mo_problem* prob, int64_t batch, void* vars, int64_t vars_stride, const void* mu,
               int64_t mu_stride, int32_t barrier_strategy, void* delta, int64_t delta_stride, void* ip_out,
               int32_t* status, void* stream);

/* Replaces QPInteriorPointSolver::Solve (qp.cc:100-151) incl. ComputeInitialGuess (qp.cc:439-482): the whole
 * interior-point loop runs on device, one problem per workgroup, with per-problem early termination.
 *   vars            [batch][V] in/out (input only read for MO_GUESS_USER_PROVIDED)
 *   termination     [batch] out mo_termination
 *   num_iterations  [batch] out
 *   iterations      [batch][max_iterations][14] out (may be NULL)
 *   lagrange        [batch][2] out {min(y), |y|_inf} (may be NULL; qp.cc:539-546) */
int mo_qp_solve(mo_plan* plan, const mo_problem* prob, int64_t batch, const mo_solve_params* params, void* vars,
                int64_t vars_stride, int32_t* termination, int32_t* num_iterations, void* iterations, void* lagrange,
                int32_t* status, void* stream);

/* Replaces QPNullSpaceSolver::Solve (qp.cc:679-729): minimise 1/2 x^T G x + c^T x subject to A_eq x + b_eq = 0 (k >= 1, no
 * inequalities; the plan's m is ignored).  x_out [batch][n] = QPNullSpaceSolver::variables(); termination [batch] =
 * QPNullSpaceTerminationState (structs.hpp:137-142): 0 SUCCESS, 1 NOT_POSITIVE_DEFINITE (x_out is NaN then).
 * Same algorithm as the reference, one workgroup per problem with G and A_eq^T resident in LDS: Householder QR of A_eq^T with column
 * pivoting (qp.cc:687; rank = Eigen's default threshold |R_jj| > |R|_max eps min(n, k), :697), u = Q1 R1^-T P^T (-b_eq) (:703-704),
 * G_reduced = Q2^T G Q2 by two-sided application of the reflectors (:708), LLT that fails iff a pivot is <= 0 (:711-714 ->
 * NOT_POSITIVE_DEFINITE), y from -(Q2^T (c + G u)) (:718-721), x = u + Q2 y (:725).  What decides SUCCESS is the reduced Hessian
 * alone: a singular or indefinite G is fine when it is positive definite on null(A_eq).  k <= n is required; for a rank-deficient
 * A_eq (rank r < k) the solve uses R's leading r x r block (the reference's k x k solve against Q1's r columns is a size mismatch
 * there).  Limits: LDS-resident, (n | 1) (n + k) + 5 n + 4 k scalars <= 160 KiB (n = 128, k = 16 fits in fp64). */
typedef enum { MO_NULLSPACE_SUCCESS = 0, MO_NULLSPACE_NOT_POSITIVE_DEFINITE = 1 } mo_nullspace_termination;
int mo_nullspace_solve(mo_plan* plan, const mo_problem* prob, int64_t batch, void* x_out, int64_t x_stride,
                       int32_t* termination, void* stream);

/* Parameter covariance of an (equality-constrained) least-squares fit.  With S = sym(G) read from the LOWER triangle only (the strict upper
 * triangle is never read), A = A_eq (k x n, k <= n; k = 0: absent) and Z an orthonormal basis of null(A):
 *   C = scale_p Z (Z^T S Z)^-1 Z^T          (k = 0: C = scale_p S^-1)
 * the top-left n x n block of the inverse of [[S, A^T], [A, 0]]: the covariance of the equality-constrained least-squares estimator with
 * G = sum w J^T J.  C depends on S and null(A) alone; what decides success is the reduced Hessian: a singular or indefinite G that is positive
 * definite on null(A) succeeds.  The rank of A follows mo_nullspace_solve (Eigen's threshold on the pivoted QR): a duplicated or zero row
 * lowers the rank and does not fail the problem; rank n gives C = 0 exactly (every entry +0) with MO_STATUS_OK.  Inequality constraints are
 * not part of this (the plan's m is ignored, as in mo_nullspace_solve): a caller who wants an active bound pinned passes it as an equality row.
 * Input: (G, A_eq) only -- prob->J != NULL is MO_ERR_INVALID_ARGUMENT (linearise first); c, b_eq, cons_* and lambda* are ignored; G_stride = 0
 * / A_stride = 0 share one instance among the batch.
 *   sel      device, [q], shared by the batch: the variables wanted, unsorted and repeated indices allowed; NULL = all n (q must be n).  An
 *            index outside [0, n) gives MO_STATUS_BAD_INDEX for EVERY problem and NaN outputs.
 *   scale    per-problem factor in the plan's dtype, NULL = 1; scale_stride 0 = one value for the batch
 *   cov_out  [batch] q x q column-major, leading dimension cov_ld >= q, BOTH triangles written, symmetric to the bit; may be NULL
 *   var_out  [batch][q] the diagonal (the bits of cov_out's diagonal); may be NULL (not both)
 *   status   [batch] MO_STATUS_OK; MO_STATUS_NOT_POSITIVE_DEFINITE iff a pivot of the reduced LLT is <= 0; MO_STATUS_NONFINITE iff an entry
 *            that is read or a result is not finite.  Every output of a failed problem is NaN; no other problem is affected.  May be NULL.
 * Padding (cov_ld > q, strides beyond the payload) is never written.  No absolute thresholds: 4 G gives C / 4 and a power-of-two scale scales
 * the result, bit for bit (short of over- / underflow).  Two launches give the same bits.  No allocation, no host synchronisation.
 * Limits: one workgroup per problem with G and A_eq^T in LDS, ((n | 1) (n + k) + 2 n + 2 k) scalars + 4 (q + 8) bytes <= 160 KiB
 * (fp64: n = 128, k = 16, q = n fits; n + k <= 112 always does); beyond: MO_ERR_UNSUPPORTED before any launch. */
int mo_qp_covariance(mo_plan* plan, const mo_problem* prob, int64_t batch, const int32_t* sel, int32_t q, const void* scale,
                     int64_t scale_stride, void* cov_out, int64_t cov_stride, int32_t cov_ld, void* var_out, int64_t var_stride,
                     int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Batched constrained nonlinear least squares: ConstrainedNonlinearLeastSquares::Solve (nonlinear.cc:75-158) for a batch of
 * independent problems of one shape, every problem with its own lambda / penalty / optimizer state, in lock step.
 * The residual functions stay with the caller (the reference's Residual objects are host functors, residual.hpp:28-143):
 * `eval` is called on the host and must ENQUEUE, on `stream`, device work that fills the buffers named in mo_nls_problem:
 *   MO_NLS_EVAL_LINEARIZE : J, r (cost stack) and J_eq, r_eq (equality stack) at `vars`        (LinearizeAndFillQP)
 *   MO_NLS_EVAL_ERRORS    : r_cand, r_eq_cand at `candidate`                                   (EvaluateNonlinearErrors)
 * for ALL problems of the batch (finished problems are ignored afterwards).  Everything else -- the errors, the shifted
 * constraints, the interior-point QP (mo_qp_solve), directional derivatives, penalty selection, the line search with
 * quadratic / cubic interpolation, the lambda state machine and the exit tests -- runs on the device.
 * fp64 plans only.  A problem whose QP fails (status != MO_STATUS_OK; the reference throws there) ends with
 * MO_NLS_QP_FAILURE and its QP status in status[p].  With equality constraints and no inequalities the reference switches
 * to QPNullSpaceSolver (nonlinear.cc:83-86, 249-258) and so does this call (the null-space kernel behind mo_nullspace_solve: a
 * singular G = J^T J is fine as long as the reduced Hessian is positive definite); the penalty then follows the no-multiplier
 * branch of SelectPenalty (nonlinear.cc:491-499), and NOT_POSITIVE_DEFINITE ends the problem with MO_NLS_QP_INDEFINITE
 * (nonlinear.cc:103-105). */
typedef enum { MO_NLS_MAX_ITERATIONS = 0, MO_NLS_SATISFIED_ABSOLUTE_TOL = 1, MO_NLS_SATISFIED_RELATIVE_TOL = 2,
               MO_NLS_SATISFIED_FIRST_ORDER_TOL = 3, MO_NLS_MAX_LAMBDA = 4, MO_NLS_QP_INDEFINITE = 5,
               MO_NLS_USER_CALLBACK = 6, MO_NLS_QP_FAILURE = 7 } mo_nls_termination;   /* NLSTerminationState, structs.hpp:233-248 */
typedef enum { MO_LS_SUCCESS = 0, MO_LS_MAX_ITERATIONS = 1, MO_LS_FIRST_ORDER_SATISFIED = 2, MO_LS_POSITIVE_DERIVATIVE = 3,
               MO_LS_FAILURE_NON_FINITE_COST = 4, MO_LS_FAILURE_INVALID_ALPHA = 5 } mo_step_result; /* StepSizeSelectionResult, structs.hpp:215-228 */
typedef enum { MO_ARMIJO_BACKTRACK = 0, MO_POLYNOMIAL_APPROXIMATION = 1 } mo_line_search;      /* structs.hpp:148-153 */
typedef enum { MO_NLS_EVAL_LINEARIZE = 0, MO_NLS_EVAL_ERRORS = 1, MO_NLS_EVAL_RETRACT = 2, MO_NLS_EVAL_ITERATION_DONE = 3 } mo_nls_eval;
/* Retraction (nonlinear.hpp:127, RetractCandidateVars nonlinear.cc:160-168): how a trial point is formed from vars, the step dx and
 * the step length alpha.  EUCLIDEAN = the reference's default x + alpha dx; WRAP_PI = every variable wrapped into [-pi, pi) afterwards
 * (math::ModPi: the custom Retraction of the reference's robot tests, nonlinear_test.cc:874-880, 1077-1084); CALLBACK = the caller's
 * own: before each evaluation the library writes dx to mo_nls_problem.step and alpha to mo_nls_problem.step_alpha and calls
 * eval(user, MO_NLS_EVAL_RETRACT, stream), which must enqueue work that fills `candidate` for all problems. */
typedef enum { MO_RETRACT_EUCLIDEAN = 0, MO_RETRACT_WRAP_PI = 1, MO_RETRACT_CALLBACK = 2 } mo_retraction;

/* ConstrainedNonlinearLeastSquares::Params (nonlinear.hpp:64-124); mo_default_nls_params fills the reference defaults. */
typedef struct {
  int32_t max_iterations;
  int32_t max_qp_iterations;
  double termination_kkt_tolerance;
  double absolute_exit_tol;
  double relative_exit_tol;
  double absolute_first_derivative_tol;
  int32_t max_line_search_iterations;
  int32_t line_search_strategy;        /* mo_line_search */
  double armijo_search_tau;
  double equality_penalty_initial;
  double equality_penalty_scale_factor;
  double equality_penalty_rho;
  double lambda_initial;
  double lambda_failure_init;
  double lambda_decrease_on_success;
  double lambda_decrease_on_restore;
  double max_lambda;
  double min_lambda;
  int32_t retraction;                  /* mo_retraction */
  int32_t log_qp_eigenvalues;          /* Params::log_qp_eigenvalues (nonlinear.hpp:122-123): non-zero = every outer iteration records the
                                          QPEigenvalues of its QP Hessian into mo_nls_problem.qp_eigenvalues (nonlinear.cc:138) */
} mo_nls_params;

/* Device buffers of one batch (all owned by the caller; shapes per problem, strides in elements, plan dims n, k, m, m_r). */
typedef struct {
  void* vars;      int64_t vars_stride;      /* n : in = initial guess, out = solution (Solve(params, variables), variables()) */
  void* candidate; int64_t candidate_stride; /* n : the line search's trial point (RetractCandidateVars, nonlinear.cc:160-168) */
  void* J;     int64_t J_stride; int32_t J_ld; int32_t J_layout;   /* m_r x n, filled by eval(LINEARIZE) */
  void* r;     int64_t r_stride;                                  /* m_r */
  void* J_eq;  int64_t J_eq_stride; int32_t J_eq_ld; int32_t reserved0; /* k x n column-major (= QP::A_eq), eval(LINEARIZE) */
  void* r_eq;  int64_t r_eq_stride;                                /* k (= QP::b_eq) */
  void* r_cand;    int64_t r_cand_stride;    /* m_r, filled by eval(ERRORS) */
  void* r_eq_cand; int64_t r_eq_cand_stride; /* k */
  const int32_t* cons_var; const void* cons_a; const void* cons_b; int64_t cons_stride; /* m: Problem::inequality_constraints */
  void* step; int64_t step_stride;   /* n : dx of the current outer iteration (written only with MO_RETRACT_CALLBACK) */
  void* step_alpha;                  /* 1 per problem: the alpha of the trial point to form (MO_RETRACT_CALLBACK) */
  int32_t* user_exit;                /* NULL, or [batch] flags for SetUserExitCallback (nonlinear.hpp:157, nonlinear.cc:142-149): after every
                                        outer iteration eval(user, MO_NLS_EVAL_ITERATION_DONE, stream) is called (the iteration's record is in
                                        `iterations`, the state in `vars`); a problem whose flag it sets non-zero ends with
                                        MO_NLS_USER_CALLBACK unless that iteration terminated it anyway.  Zeroed by mo_nls_solve on entry. */
  void* qp_iterations;               /* NULL, or [max_iterations][batch][max_qp_iterations][MO_ITER_RECORD]: the QPInteriorPointIteration records
                                        of every outer iteration's QP (NLSIteration::qp_outputs, structs.hpp:288); the caller pre-fills NaN */
  void* qp_lagrange;                 /* NULL, or [max_iterations][batch][2]: QPLagrangeMultipliers {min, l_infinity} of each QP (k > 0) */
  void* qp_eigenvalues;              /* required with params.log_qp_eigenvalues: [max_iterations][batch][3] = NLSIteration::qp_eigenvalues
                                        {min, max, abs_min} of G = J^T J + lambda I of each outer iteration (structs.hpp:267-310); the caller
                                        pre-fills NaN (iterations a problem never ran keep it) */
} mo_nls_problem;

typedef int (*mo_nls_eval_fn)(void* user, int32_t what, void* stream);  /* non-zero return aborts mo_nls_solve with MO_ERR_CALLBACK */
#define MO_ERR_CALLBACK (-6)

/* NLSIteration (structs.hpp:277-330) as doubles: {optimizer_state, lambda, errors_initial.f, errors_initial.equality, d_f,
 * d_equality, penalty, step_result, n_line_search_steps, qp_termination, qp_num_iterations, qp_status} followed by
 * (max_line_search_iterations + 1) x {alpha, f, equality} (LineSearchStep, structs.hpp:206-213; NaN when not taken). */
#define MO_NLS_ITER_HEADER 12
#define MO_NLS_ITER_RECORD(max_line_search_iterations) (MO_NLS_ITER_HEADER + 3 * ((max_line_search_iterations) + 1))

void mo_default_nls_params(mo_nls_params* params);
/* 1 when mo_nls_solve takes QPNullSpaceSolver's path for this plan's shape (equalities, no inequalities: nonlinear.cc:83-86 -- and the
 * shape fits the null-space kernel), 0 when its QPs go through the interior-point Solve: tells which record layout `iterations` carries
 * (NLSIteration::qp_outputs / qp_term_state, structs.hpp:277-326). */
int mo_plan_nls_uses_nullspace(const mo_plan* plan);
/* termination [batch] (mo_nls_termination), num_iterations [batch], iterations [batch][max_iterations][MO_NLS_ITER_RECORD]
 * (may be NULL), status [batch] (may be NULL).  Synchronises `stream` (one small read-back per outer iteration and per
 * line-search step to learn whether any problem is still active). */
int mo_nls_solve(mo_plan* plan, const mo_nls_problem* prob, int64_t batch, const mo_nls_params* params, mo_nls_eval_fn eval,
                 void* user, int32_t* termination, int32_t* num_iterations, void* iterations, int32_t* status, void* stream);

/* Device residual families: the residual functions of the reference's own NLS tests as kernels (its Residual functors are host
 * lambdas, residual.hpp:28-143), so that an mo_nls_solve callback can be two launches instead of a PCIe round trip.
 *   ROSENBROCK     n >= 2, rows = 2 (n - 1): r_2i = 1 - x_i, r_2i+1 = 10 (x_i+1 - x_i^2)     (nonlinear_test.cc:375-386, 502-521)
 *   HIMMELBLAU     n = 2, rows = 2: x^2 + y - 11, x + y^2 - 7                                  (nonlinear_test.cc:578-593)
 *   SPHERE         rows = n: r = x                                                             (nonlinear_test.cc:722-730)
 *   PRODUCT_PAIRS  rows <= n / 2: r_q = x_2q x_2q+1 - params[q]  (params: `rows` device scalars) (nonlinear_test.cc:737-743)
 *   ACTUATOR_CHAIN the kinematic chains of the reference's robot tests (test/transform_chains.cc:23-82 ComputeChain, :125-158
 *                  ActuatorLink::Compute, :165-244 ActuatorChain::Update; used at nonlinear_test.cc:828-1136): every row is affine in
 *                  the effector translations of up to 4 chains and in x,  r_q = const_q + sum_i lin_qi x_i + sum_c w_qc . t_c(x),
 *                  with the Jacobian through translation_D_params.  params (device scalars of the plan's dtype, integers stored as
 *                  scalars):  [C,  then per chain: L, then per link 12 values: euler-xyz rotation (R = Rx Ry Rz), translation, and for
 *                  each of the 6 degrees of freedom (rx, ry, rz, tx, ty, tz) the index in x of the parameter that replaces it or -1;
 *                  then per row: const, n_lin, n_lin x (index, coefficient), n_terms, n_terms x (chain, wx, wy, wz)].  L <= 8.
 * r [batch][rows]; J (NULL = values only) dense rows x n per problem, row-major (cost stacks) or column-major (equality stacks,
 * = QP::A_eq), zeros written. */
typedef enum { MO_RESIDUAL_ROSENBROCK = 0, MO_RESIDUAL_HIMMELBLAU = 1, MO_RESIDUAL_SPHERE = 2, MO_RESIDUAL_PRODUCT_PAIRS = 3,
               MO_RESIDUAL_ACTUATOR_CHAIN = 4 } mo_residual_family;
int mo_residual_eval(mo_plan* plan, int32_t family, int32_t rows, const void* params, const void* x, int64_t x_stride,
                     int64_t batch, void* r, int64_t r_stride, void* J, int64_t J_stride, int32_t J_ld, int32_t J_layout,
                     void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Residual-block input: the reference's own model of a cost (mini_opt::Problem::costs, nonlinear.hpp:33-52).  Each residual b is an
 * R_b x P_b local Jacobian over an index list of P_b of the n variables (Residual::Model, residual.hpp:60-143).  A residual LAYOUT
 * describes the block structure once and is shared by the whole batch, like Problem::costs.
 * Packed values of one problem: block b's local Jacobian is R_b x P_b COLUMN-major (Eigen's JacobianType, what the functor fills) and
 * starts at offset sum_{b' < b} R_b' P_b'; r is the stacked residual values in block order (the dense stack's r).  Strides in elements,
 * stride 0 = one instance shared by the batch. */
typedef struct mo_residual_layout mo_residual_layout;
/* rows[b] = R_b >= 1, params[b] = P_b >= 1, index = the concatenated index lists (sum P_b entries), all HOST arrays.
 * 0 <= index < plan n, else MO_ERR_DIMENSION (F_ASSERT_LT of GatherValues / UpdateHessian, residual.hpp:160-162, :209).
 * Builds the gather schedule on the host and uploads it to the plan's device: all allocation happens here, none in a launch.
 * The layout may be used with any plan of the same n on the same device. */
int mo_residual_layout_create(const mo_plan* plan, int32_t num_blocks, const int32_t* rows, const int32_t* params,
                              const int32_t* index, mo_residual_layout** out);
int mo_residual_layout_destroy(mo_residual_layout* layout);
int64_t mo_residual_layout_values(const mo_residual_layout* layout);   /* sum R_b P_b: packed Jacobian length per problem (-1: NULL) */
int32_t mo_residual_layout_rows(const mo_residual_layout* layout);     /* sum R_b (-1: NULL) */

/* The cost half of LinearizeAndFillQP (nonlinear.cc:182-189) for block input: G_out (n x n col-major, lower written, strict upper written
 * as 0) = sum_b UpdateHessian (residual.hpp:186-226, the reference's summation order) + lambda I after the sum (lambda[_vec] added iff
 * > 0; lambda_vec NULL = the scalar), c_out = sum_b J_b^T r_b, half_sq_out[p] (may be NULL) = sum_b 0.5 |r_b|^2.  Requires sum R_b ==
 * plan m_r.  Deterministic: every cell is summed by one lane in a fixed order.  G_out == NULL: only c_out and half_sq_out are formed (G_stride
 * and G_ld are ignored), in the same order, so the bits of c are those of the full call -- for a caller whose G comes from elsewhere (one
 * G for the whole batch, formed by a batch-1 call). */
int mo_linearize_blocks(mo_plan* plan, const mo_residual_layout* layout, const void* J_blocks, int64_t J_stride, const void* r,
                        int64_t r_stride, double lambda, const void* lambda_vec, int64_t lambda_stride, int64_t batch, void* G_out,
                        int64_t G_stride, int32_t G_ld, void* c_out, int64_t c_stride, void* half_sq_out, void* stream);
/* UpdateJacobian stacked (nonlinear.cc:191-206, residual.hpp:230-250): J_out = the dense (sum R_b) x n matrix, zeros, then every block's
 * columns ASSIGNED in local order (a duplicate index keeps the last column); J_out_layout MO_COL_MAJOR gives QP::A_eq.
 * abs_sum_out[p] (may be NULL) = |r|_1, Errors::equality (nonlinear.cc:204). */
int mo_jacobian_blocks(mo_plan* plan, const mo_residual_layout* layout, const void* J_blocks, int64_t J_stride, const void* r,
                       int64_t r_stride, int64_t batch, void* J_out, int64_t J_out_stride, int32_t J_out_ld, int32_t J_out_layout,
                       void* abs_sum_out, void* stream);
/* mo_nls_solve with block input: eval(MO_NLS_EVAL_LINEARIZE) fills np->J / np->J_eq with PACKED block Jacobians of cost_layout /
 * eq_layout (J_ld, J_layout and J_eq_ld are ignored; J_stride / J_eq_stride are per-problem strides of the packed values).  Every outer
 * iteration forms G, c (with the problem's lambda) and A_eq with the two calls above into per-call scratch and hands the QP over as
 * (G, c) input.  fp64 only; eq_layout is NULL iff k == 0; sum R_b of cost_layout == m_r and of eq_layout == k. */
int mo_nls_solve_blocks(mo_plan* plan, const mo_nls_problem* np, const mo_residual_layout* cost_layout,
                        const mo_residual_layout* eq_layout, int64_t batch, const mo_nls_params* params, mo_nls_eval_fn eval, void* user,
                        int32_t* termination, int32_t* num_iterations, void* iterations, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Differentiating through a solve: the KKT system of a state for a CALLER's right-hand side, and the gradients of a loss.
 * With the reference's residual (qp.cc:391-420) F(v; theta) = [r_d | r_comp - mu | r_pe | r_pi], v = [x | s | y | z], C the m x n matrix
 * with C[i, var_i] = a_i, S = diag(s), Z = diag(z):
 *   r_d = G x + c - A_eq^T y - C^T z     r_comp = s o z     r_pe = A_eq x + b_eq     r_pi = C x + b - s
 *           | G     0   -A_eq^T  -C^T |
 *   K(v) =  | 0     Z     0       S   |     the matrix of BuildFullSystem; SolveForUpdate solves K delta = -r through the reduced system
 *           | A_eq  0     0       0   |     H = G + C^T S^-1 Z C (qp.cc:275-364)
 *           | C    -I     0       0   |
 *
 * The call below factorises at `vars` exactly as the Newton step does (ComputeLDLT, qp.cc:275-316: s > 0 required; status[p] =
 * NONPOSITIVE_SLACK / FACTORIZATION_FAILED / NONFINITE / BAD_INDEX as there, `out` NaN-filled for such problems) and then runs
 * SolveForUpdate (qp.cc:318-364) with r_ := rhs, mu = 0, delta_affine_ = 0:
 *   flags = 0                 out = delta with K delta = -rhs.  With rhs = the r_out of the residual call above, mu subtracted from its r_comp
 *                             block, this is the Newton direction of the hot path, bit for bit on the generic kernel.
 *   MO_KKT_TRANSPOSE          out = u with K^T u = rhs: the kernel solves K delta = -[-g_x | -s o g_s | g_y | g_z] and returns
 *                             [delta_x | delta_s / s | -delta_y | -delta_z], so the adjoint shares the factorisation code of the step.
 *   MO_STEP_NO_INEQUALITIES   as in the Newton step: the system of [x | y] alone; the s and z blocks of rhs are ignored and written as 0.
 * rhs, out: [batch][V], 8-byte aligned; rhs may alias neither vars nor out.  J-level and (G, c) input are both accepted.
 * Which kernel runs (mo_plan_kkt_solve_kernel tells): the right-hand-side twin of the fused fp64 step kernel -- the step's template
 * instantiated with a compile-time right-hand-side mode, in a translation unit of its own, so that no step or Solve instantiation pays a
 * register for it -- where ALL of these hold: fp64; 2 <= n <= 128; k <= 31; m <= 128; input (G, c), or a J the 16-byte vector stream
 * takes (packed row-major with J_ld = n, even n, 16-byte aligned, even stride); not a shape whose step runs the one-tile kernel (n + k <= 15,
 * m <= 64, J-level: m_r <= 64; none with MO_PLAN_NO_TINY); no MO_PLAN_FORCE_GENERIC.  Every other call runs the shape-generic kernel.  The two kernels agree to
 * rounding (same reduced system, different elimination order); only on the generic kernel is the flags = 0 result bit for bit the Newton
 * direction of that kernel's step.  No allocation and no synchronisation on the launch path: at most an 8-byte memset and one kernel. */
int mo_kkt_solve(mo_plan* plan, const mo_problem* prob, int64_t batch, const void* vars, int64_t vars_stride, const void* rhs,
                 int64_t rhs_stride, uint32_t flags, void* out, int64_t out_stride, int32_t* status, void* stream);

/* Gradients of a loss l through v*(theta), the root of F(v; theta) = 0, from g = dl/dv and u = K^-T g (MO_KKT_TRANSPOSE above):
 *   dc = -u_x                 dG = -1/2 (u_x x^T + x u_x^T)         dA_eq = y u_x^T - u_y x^T         db_eq = -u_y
 *   dcons_a[i] = z_i u_x[var_i] - u_z[i] x[var_i]                   dcons_b[i] = -u_z[i]   (NaN for a var_i outside [0, n))
 * and for J-level input (G = J^T J + lambda I, c = J^T r), without forming an n x n matrix:
 *   dJ = -(J u_x) x^T - (J x + r) u_x^T        dr = -J u_x        dlambda = -u_x . x
 * dG is the gradient with respect to a SYMMETRIC G, returned full and exactly symmetric; the library reads only the lower triangle of G
 * (qp.cc:289), so a caller who owns just the lower entries adds dG[i][j] + dG[j][i] for i > j.
 * Every output is optional: a NULL member is neither computed nor written.  Layouts as the inputs: dG n x n and dA_eq k x n column-major
 * with a leading dimension, dJ m_r x n in dJ_layout (mo_layout) with dJ_ld; strides per problem, in elements.  dG with J-level input, and
 * dJ / dr / dlambda with (G, c) input, are MO_ERR_INVALID_ARGUMENT.  Only prob->J / r (for dJ, dr) and prob->cons_var (for dcons_a) are
 * read.  Pure data movement: one workgroup per problem in turn, every output element has one owner (no atomics), so two launches give the
 * same bits.  No allocation and no synchronisation on the launch path. */
typedef struct {
  void* dG;      int64_t dG_stride; int32_t dG_ld; int32_t reserved0;   /* n x n */
  void* dc;      int64_t dc_stride;                                   /* n */
  void* dA_eq;   int64_t dA_stride; int32_t dA_ld; int32_t reserved1;   /* k x n */
  void* db_eq;   int64_t db_stride;                                   /* k */
  void* dcons_a; void* dcons_b; int64_t dcons_stride;                 /* m each */
  void* dJ;      int64_t dJ_stride; int32_t dJ_ld; int32_t dJ_layout;   /* m_r x n */
  void* dr;      int64_t dr_stride;                                   /* m_r */
  void* dlambda; int64_t dlambda_stride;                              /* 1 */
} mo_qp_grads;
int mo_qp_gradients(mo_plan* plan, const mo_problem* prob, int64_t batch, const void* vars, int64_t vars_stride, const void* u,
                    int64_t u_stride, const mo_qp_grads* out, void* stream);

/* The same gradients SUMMED over the batch, for data the whole batch shares (a learned layer: one G, A_eq, constraint set or J for every
 * sample).  With ok_p = "problem p counts" and M = sum ok_p u_x,p x_p^T, s_u = sum ok_p u_x,p, s_uy = sum ok_p u_y,p, s_uz = sum ok_p u_z,p:
 *   dG = -1/2 (M + M^T)       dc = -s_u       dA_eq = sum ok_p (y_p u_x,p^T - u_y,p x_p^T)       db_eq = -s_uy
 *   dcons_a[i] = sum ok_p (z_p,i u_x,p[var_i] - u_z,p,i x_p[var_i])       dcons_b = -s_uz
 *   dJ = -J (M + M^T) - Q,  Q = sum ok_p r_p u_x,p^T (r s_u^T when r_stride is 0 too)       dr = -J s_u       dlambda = -trace(M)
 * No per-problem matrix is written or read: the inputs are the two [batch][V] arrays.  `out` is the struct of mo_qp_gradients holding ONE
 * instance per member: the *_stride fields are ignored, the leading dimensions honoured, a NULL member neither computed nor written.
 * status_fwd / status_adj ([batch] MO_STATUS_* words, either may be NULL): problem p counts iff every given word is MO_STATUS_OK; a problem
 * that does not count contributes exactly nothing, whatever its rows of vars / u hold (mo_kkt_solve leaves NaN there).
 * MO_ERR_INVALID_ARGUMENT, with nothing written: dJ or dr unless prob->J_stride == 0; dcons_a / dcons_b unless prob->cons_stride == 0; dG
 * with J-level input, dJ / dr / dlambda with (G, c) input (mo_qp_gradients' rules); a workspace smaller than
 * mo_qp_gradients_shared_workspace reports for the same (plan, prob, batch, out), or not 16-byte aligned.  MO_ERR_DIMENSION as
 * mo_qp_gradients.  Shapes, dtypes and J layouts: those of mo_qp_gradients; any vars_stride, u_stride >= V.  batch == 0 writes zeros.
 * The batch is cut into chunks of consecutive problems, their number a function of (batch, CU count) alone; the moments of a chunk are
 * accumulated on the matrix cores (v_mfma_*_16x16x4, four problems per instruction), the chunk partials are summed in chunk order in
 * double, the outputs are formed in double and rounded once.  Every workspace and output element has one owner: no atomics, no memset, the
 * same bits on every launch of one device; dG is symmetric to the bit.  No allocation and no synchronisation on the launch path: three
 * kernels on `stream`.  The workspace's contents are scratch. */
int mo_qp_gradients_shared_workspace(const mo_plan* plan, const mo_problem* prob, int64_t batch, const mo_qp_grads* out, int64_t* bytes);
int mo_qp_gradients_shared(mo_plan* plan, const mo_problem* prob, int64_t batch, const void* vars, int64_t vars_stride, const void* u,
                           int64_t u_stride, const int32_t* status_fwd, const int32_t* status_adj, const mo_qp_grads* out, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* The same gradients for RESIDUAL-BLOCK input (the packed local Jacobians of a mo_residual_layout), without forming an n x n or an
 * m_r x n matrix: the transpose of the gather mo_linearize_blocks / mo_jacobian_blocks perform, applied to the pair (x, u_x).
 * mo_linearize_blocks forms, per block b and local pair q <= p, G_low[max(i, j), min(i, j)] += J_b[:, p] . J_b[:, q] with i = idx_b[p],
 * j = idx_b[q] (residual.hpp:206-224), c[idx_b[p]] += J_b[:, p] . r_b, and lambda on the diagonal after the sum.  With the loss gradient
 * of the LOWER entries, W[i][j] = -(u_i x_j + x_i u_j) for i > j and W[i][i] = -u_i x_i (u = u_x), transposing the pair map gives
 *   dJ_b[:, p] = sum_q w_b(p, q) J_b[:, q] - u[idx_b[p]] r_b
 *       w_b(p, p) = -2 u_i x_i                    (i = idx_b[p])
 *       w_b(p, q) = -u_i x_i                      q != p on the SAME variable i (a repeated index: the pair lands once, on the diagonal)
 *       w_b(p, q) = -(u_i x_j + x_i u_j)          otherwise (j = idx_b[q])
 *   dr_b = -sum_p u[idx_b[p]] J_b[:, p]           dlambda = -u_x . x   (lambda counts only where it was added: lambda > 0)
 * The kernel evaluates it as  dJ_b[q, p] = -u_p t_b[q] - x_p w_b[q] + sum over the OTHER local columns q' on p's variable of
 * (u_p x_p) J_b[q, q']  with t_b = J_b x_loc + r_b, w_b = J_b u_loc (x_loc[p] = x[idx_b[p]]); dr_b = -w_b.  Without repeated indices
 * the last sum is empty (the partner lists are built by mo_residual_layout_create and are empty for almost every layout).
 * The plan is that of the (G, c) solve: it supplies n, k, m, dtype and device (vars, u: [batch][V]); no m_r requirement.  The layout's n
 * must equal the plan's.  J_stride / r_stride 0 = one instance shared by the batch; outputs are always per problem, dJ_blocks in the order
 * and packing of J_blocks.  A NULL member of mo_block_grads is neither computed nor written; J_blocks and r are read only for dJ_blocks /
 * dr.  Arguments are judged before the plan is looked at.  Every output element has one owner and a fixed order of operations, products
 * are rounded before they are added: no atomics, two launches give the same bits.  No allocation and no synchronisation on the launch
 * path: the backward schedule is part of the layout.  MO_ERR_UNSUPPORTED if 2 (n + sum R_b) values exceed 63 KiB (the vectors the kernel
 * keeps in LDS). */
typedef struct {
  void* dJ_blocks; int64_t dJ_stride;     /* sum R_b P_b per problem, the order and packing of J_blocks */
  void* dr;        int64_t dr_stride;     /* sum R_b */
  void* dlambda;   int64_t dlambda_stride;
} mo_block_grads;
int mo_qp_gradients_blocks(mo_plan* plan, const mo_residual_layout* cost_layout, const void* J_blocks, int64_t J_stride, const void* r,
                           int64_t r_stride, int64_t batch, const void* vars, int64_t vars_stride, const void* u, int64_t u_stride,
                           const mo_block_grads* out, void* stream);
/* Equality blocks (mo_jacobian_blocks: columns ASSIGNED, a duplicate index keeps the last local column; A_eq = the stack, b_eq = r_eq).
 * With dA_eq = y u_x^T - u_y x^T and row = the block's first row + q:
 *   dJeq_b[q, a] = y[row] u_x[idx_b[a]] - u_y[row] x[idx_b[a]]   if local column a is the one that wins its global column, else exactly 0
 *   dr_eq[row]   = -u_y[row]
 * The layout's rows must equal the plan's k.  dJ_eq_blocks and dr_eq may each be NULL.  Reads no block values. */
int mo_qp_gradients_eq_blocks(mo_plan* plan, const mo_residual_layout* eq_layout, int64_t batch, const void* vars, int64_t vars_stride,
                              const void* u, int64_t u_stride, void* dJ_eq_blocks, int64_t dJ_eq_stride, void* dr_eq,
                              int64_t dr_eq_stride, void* stream);

/* The block gradients SUMMED over the batch, for blocks the whole batch shares (a learned structured cost: the factor structure is fixed,
 * the local Jacobians are the parameters of every sample, the residual values differ per sample).  J_blocks is ONE instance; r is per
 * problem (r_stride != 0) or one instance too (r_stride == 0).  With the moments of mo_qp_gradients_shared, all sums over the problems
 * that count -- M = sum u_x x^T, s_u = sum u_x, A1 = sum y u_x^T, A2 = sum u_y x^T, s_uy = sum u_y -- and i_p = idx_b[p]:
 *   dJ_b[q, p] = -sum_p' J_b[q, p'] (M[i_p][i_p'] + M[i_p'][i_p]) - Q_b[q, p] + M[i_p][i_p] sum over the OTHER local columns q' on p's variable of J_b[q, q']
 *   Q_b[q, p]  = sum over the problems of r[row_b + q] u_x[i_p]       (r[row_b + q] s_u[i_p] when r is shared too)
 *   dr_b       = -sum_p' s_u[i_p'] J_b[:, p']       (only with r_stride == 0)       dlambda = -trace(M)   (ONE value: the caller masks it where lambda <= 0)
 *   dJeq_b[q, a] = A1[row, i_a] - A2[row, i_a] if local column a wins its global column, else exactly 0       dr_eq = -s_uy
 * that is mo_qp_gradients_blocks' and mo_qp_gradients_eq_blocks' outputs summed over the problems that count.  No per-problem matrix or
 * packed gradient is written or read: the inputs are the two [batch][V] arrays, one instance of the blocks, and r.  Q is formed only at
 * the packed positions, never as a rows x n matrix.
 * The plan is that of the (G, c) solve (n, k, m, dtype, device), as for mo_qp_gradients_blocks; status_fwd / status_adj as for
 * mo_qp_gradients_shared: a problem that does not count contributes exactly nothing, whatever its rows of vars / u / r hold.
 * Arguments are judged before the plan is looked at.  MO_ERR_INVALID_ARGUMENT, with nothing written: NULL cost_layout / out; dr with
 * r_stride != 0; dJ_blocks or dr without J_blocks and r; dJ_eq_blocks or dr_eq without eq_layout; a workspace smaller than the workspace
 * query reports for the same arguments, or not 16-byte aligned.  MO_ERR_DIMENSION: a layout's n differs from the plan's, eq_layout's rows
 * from the plan's k, vars_stride / u_stride < V.  With k = 0 the equality members are ignored.  MO_ERR_UNSUPPORTED: four problems' moment rows (x, u_x and,
 * with an equality member, y, u_y; every vector padded to 16 values) exceed 64 KiB of LDS, or -- dJ_blocks with r_stride != 0 -- the
 * (n + sum R_b) values of one problem (r and u_x, staged for the packed Q) exceed 64 KiB less the 64 bytes of that kernel's flags.  batch == 0 writes zeros.
 * Stage 1 is mo_qp_gradients_shared's: the same chunks (a function of batch and CU count alone), the moments on the matrix cores, masked
 * problems selected to zero.  The packed Q partials use the same chunks: one owner per packed value, r and u_x rows staged through LDS,
 * summed in problem order, products rounded before they are added.  The finish sums the chunk partials in chunk order in double, forms
 * every output from the totals in double through the layouts' schedules and rounds once.  Every workspace and output element has one
 * owner: no atomics, no memset, the same bits on every launch of one device, and each member alone gets the bits it gets beside the
 * others.  No allocation and no synchronisation on the launch path: at most four kernels on `stream`.  The workspace's contents are scratch. */
typedef struct {            /* ONE instance per member; NULL = neither computed nor written */
  void* dJ_blocks;          /* cost_layout values, the packing of J_blocks */
  void* dr;                 /* cost_layout rows; only with r_stride == 0 */
  void* dlambda;            /* 1 */
  void* dJ_eq_blocks;       /* eq_layout values */
  void* dr_eq;              /* k */
} mo_block_shared_grads;
int mo_qp_gradients_blocks_shared_workspace(const mo_plan* plan, const mo_residual_layout* cost_layout, const mo_residual_layout* eq_layout,
                                            int64_t r_stride, int64_t batch, const mo_block_shared_grads* out, int64_t* bytes);
int mo_qp_gradients_blocks_shared(mo_plan* plan, const mo_residual_layout* cost_layout, const void* J_blocks /* one instance */, const void* r,
                                  int64_t r_stride, const mo_residual_layout* eq_layout, int64_t batch, const void* vars, int64_t vars_stride,
                                  const void* u, int64_t u_stride, const int32_t* status_fwd, const int32_t* status_adj,
                                  const mo_block_shared_grads* out, void* workspace, int64_t workspace_bytes, void* stream);

/* Forward mode: the directional derivative vdot = (dv* / dtheta) thetadot of the root of F(v; theta) = 0 along a direction thetadot in the
 * problem's data.  From F(v*(theta); theta) = 0 follows K vdot = -rho with rho = F_theta thetadot; the call below forms rho at the state
 * `vars` from the tangents (a NULL member is a zero tangent):
 *   (G, c) input:   rho_d = sym(dG) x + dc - dA_eq^T y - sum_i dcons_a[i] z_i e_{var_i}
 *   (J, r, lambda): rho_d = dJ^T w + J^T tdot + dlambda x - dA_eq^T y - sum_i dcons_a[i] z_i e_{var_i},   w = J x + r,  tdot = dJ x + dr
 *   rho_comp = 0       rho_pe = dA_eq x + db_eq       rho_pi[i] = dcons_a[i] x[var_i] + dcons_b[i]   (NaN for a var_i outside [0, n))
 * sym(dG) is the symmetric matrix whose lower triangle is that of dG: dG is read as G is read, lower triangle only; its strict upper
 * triangle and the padding beyond any matrix (ld > rows) are never read into the result and may hold anything.  dlambda counts
 * unconditionally, as the dlambda of mo_qp_gradients does.
 * The two-call recipe:   mo_qp_tangent_rhs(..., t, rho, ...);   mo_kkt_solve(..., rhs = rho, flags = 0, out = vdot, ...).
 * The map thetadot -> rho is the exact transpose of mo_qp_gradients' map u -> gradients (up to the sign of K delta = -rhs): for every g,
 *   g . vdot = sum over the members of < gradient of the member from u = K^-T g,  tangent of the member >,
 * with dG's tangent taken symmetric (a caller with an arbitrary Gdot passes 1/2 (Gdot + Gdot^T)).
 * Layouts as the inputs: dG n x n and dA_eq k x n column-major with a leading dimension; dJ m_r x n in prob->J_layout with its OWN leading
 * dimension and stride; strides per problem, in elements, 0 = one direction shared by the batch.  Only prob->J / r (for dJ, dr) and
 * prob->cons_var are read from the problem; with k = 0 the equality members and with m = 0 the inequality members are ignored.
 * rho: [batch][V], all V values written (rho_comp as zeros), nothing beyond V.
 * MO_ERR_INVALID_ARGUMENT (judged before the plan is looked at): NULL prob / t / vars / rho; dG with J-level input; dJ / dr / dlambda
 * with (G, c) input; dJ without prob->r; dcons_a without prob->cons_var.  MO_ERR_DIMENSION: dG_ld < n, dA_ld < k, dJ_ld below the layout's
 * minimum.  MO_ERR_UNSUPPORTED if the vectors the kernel keeps in LDS -- (2 n + 2 k + m + 2 m_r) values, each block padded to 16 bytes,
 * m 32-bit indices and 4 KiB of partial sums; m_r counts only with dJ or dr -- exceed 64 KiB.
 * Pure data movement: one workgroup per problem in turn, every element of rho has one owner and a fixed order of operations (no atomics,
 * also where several rows name one variable), so two launches give the same bits.  No allocation and no synchronisation on the launch
 * path: one kernel. */
typedef struct {                                   /* every member optional: NULL = zero tangent.  Strides per problem, in elements; 0 = one direction shared by the batch */
  const void* dG;    int64_t dG_stride; int32_t dG_ld; int32_t reserved0;   /* n x n column-major, LOWER triangle read as a symmetric matrix */
  const void* dc;    int64_t dc_stride;
  const void* dA_eq; int64_t dA_stride; int32_t dA_ld; int32_t reserved1;   /* k x n column-major */
  const void* db_eq; int64_t db_stride;
  const void* dcons_a; const void* dcons_b; int64_t dcons_stride;
  const void* dJ;    int64_t dJ_stride; int32_t dJ_ld; int32_t reserved2;   /* m_r x n in prob->J_layout */
  const void* dr;    int64_t dr_stride;
  const void* dlambda; int64_t dlambda_stride;
} mo_qp_tangents;
int mo_qp_tangent_rhs(mo_plan* plan, const mo_problem* prob, int64_t batch, const void* vars, int64_t vars_stride,
                      const mo_qp_tangents* t, void* rho, int64_t rho_stride, void* stream);

/* Forward mode for RESIDUAL-BLOCK input: the same rho from the PACKED tangents of the blocks, without forming an n x n or a rows x n
 * matrix.  The (G, c) problem is the one mo_linearize_blocks / mo_jacobian_blocks produce, so rho is by definition what
 * mo_qp_tangent_rhs gives for (G, c) input with dG, dc the directional derivatives of mo_linearize_blocks along (dJ_blocks, dr, dlambda)
 * and dA_eq, db_eq those of mo_jacobian_blocks and r_eq along (dJ_eq_blocks, dr_eq).
 * Cost blocks, with x_loc[p] = x[idx_b[p]], t_b = J_b x_loc + r_b and tdot_b = dJ_b x_loc + dr_b:
 *   rho_d[i] += dJ_b[:, p] . t_b + J_b[:, p] . tdot_b                      for every local column p with idx_b[p] = i
 *   rho_d[i] -= x_i (dJ_b[:, p] . J_b[:, q'])                              for every OTHER local column q' of block b on p's variable i
 *   rho_d    += dlambda x
 * The second line is the repeated-index rule of mo_qp_gradients_blocks seen from the other side: the pair (p, q') of one variable lands
 * once, on the diagonal (w_b(p, q) = -u_i x_i above), so sym(G) lacks one J_p . J_q' against the dense J^T J of the gathered columns and the
 * tangent lacks its derivative.  The partner lists are those of the backward and are empty for almost every layout.  dlambda counts
 * unconditionally, as the dlambda of mo_qp_gradients_blocks does (a caller masks it where lambda <= 0).
 * Equality blocks (mo_jacobian_blocks is linear in the packed values: no J_eq_blocks values are read), for a packed value e with stacked
 * row `row` and global column g whose local column WINS g:
 *   rho_pe[row] += dJeq[e] x[g]         rho_d[g] -= dJeq[e] y[row]         rho_pe += dr_eq
 * A column that loses its global column contributes exactly nothing: its dJ_eq_blocks entries are never read into rho and may be NaN.
 * Constraint rows as in mo_qp_tangent_rhs: rho_d[var_i] -= dcons_a[i] z_i, rho_pi[i] = dcons_a[i] x[var_i] + dcons_b[i] (NaN for a var_i
 * outside [0, n)), rho_comp = 0.
 * The transpose identity that ties the call to the merged backward: for every u and the same `vars`,
 *   u . rho = - sum over the members of < gradient of the member from u,  tangent of the member >,
 * the gradients being those of mo_qp_gradients_blocks (dJ_blocks, dr, dlambda), mo_qp_gradients_eq_blocks (dJ_eq_blocks, dr_eq) and
 * mo_qp_gradients (dcons_a, dcons_b).  The two-call recipe:  mo_qp_tangent_rhs_blocks(..., t, rho, ...);  mo_kkt_solve on the (G, c)
 * problem with rhs = rho, flags = 0, out = vdot.
 * The plan is that of the (G, c) solve: it supplies n, k, m, dtype and device; no m_r requirement.  J_stride / r_stride and every tangent
 * stride: per problem in elements, 0 = shared by the batch.  A NULL tangent member is a zero tangent and its inputs are not read:
 * J_blocks is read only with dJ_blocks or dr, r only with dJ_blocks.  With k = 0 the equality members and eq_layout, with m = 0 the
 * inequality members are ignored.  rho: [batch][V], all V values written, nothing beyond V.
 * Arguments are judged before the plan is looked at.  MO_ERR_INVALID_ARGUMENT: NULL cost_layout / t / vars / rho; dJ_blocks or dr without
 * J_blocks and r; dJ_eq_blocks or dr_eq without eq_layout; dcons_a without cons_var.  MO_ERR_DIMENSION: a layout's n differs from the
 * plan's; eq_layout's rows differ from the plan's k.  MO_ERR_UNSUPPORTED, with nothing launched, if the vectors the kernel always keeps in
 * LDS exceed 64 KiB:  (2 n + 2 k + m + 2 sum R_b) values (x, rho_d; y, rho_pe; dcons_a z; t, tdot) + 4 m bytes (the indices); partial
 * sums live in registers.  Below that, J_blocks, dJ_blocks, r and dr go through LDS when 2 (sum R_b P_b + sum R_b) values fit 48 KiB and
 * the total fits 64 KiB, and are read from global memory otherwise.
 * One workgroup per problem in turn; every element of rho has one owner (a fixed-width group of lanes walks variable i's contribution
 * list in the layout's order and adds its partial sums in a shuffle tree of fixed shape), products are rounded before they are added: no
 * atomics, two launches give the same bits.  No allocation and no synchronisation on the launch path: the schedule is part of the
 * layouts. */
typedef struct {                      /* every member optional: NULL = zero tangent; strides per problem in elements, 0 = one direction shared by the batch */
  const void* dJ_blocks;    int64_t dJ_stride;      /* packing of J_blocks */
  const void* dr;           int64_t dr_stride;
  const void* dlambda;      int64_t dlambda_stride;
  const void* dJ_eq_blocks; int64_t dJ_eq_stride;   /* packing of J_eq_blocks */
  const void* dr_eq;        int64_t dr_eq_stride;
  const void* dcons_a; const void* dcons_b; int64_t dcons_stride;
} mo_block_tangents;
int mo_qp_tangent_rhs_blocks(mo_plan* plan, const mo_residual_layout* cost_layout, const void* J_blocks, int64_t J_stride,
                             const void* r, int64_t r_stride, const mo_residual_layout* eq_layout,
                             const int32_t* cons_var, int64_t cons_stride, int64_t batch, const void* vars, int64_t vars_stride,
                             const mo_block_tangents* t, void* rho, int64_t rho_stride, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Per-row weights for residual-block costs: the cost  1/2 sum_i w_i (J x + r)_i^2 + 1/2 lambda |x|^2  with one weight per stacked residual
 * row of the cost layout (block order, the order of r), per problem.  A per-block weight is the caller's repeat of it over the block's
 * rows.  This is the pair rule of UpdateHessian with one factor per row, W_b the diagonal of block b's weights:
 *   per block and local pair q <= p:   G_low[max(i, j), min(i, j)] += sum_rho w_rho J_b[rho, p] J_b[rho, q]      (i = idx_b[p], j = idx_b[q])
 *   c[idx_b[p]] += sum_rho w_rho J_b[rho, p] r_rho       lambda on the diagonal after the sum, where > 0       half_sq = 1/2 sum w_rho r_rho^2
 * A pair of local columns on one variable still lands once, on the diagonal; the order of every sum is that of the unweighted kernels.
 * Every term is formed as (w_rho J_b[rho, p]) * (.): with every weight 1 the calls below compute the bits of their unweighted siblings, and
 * with weights that are powers of four the bits of the siblings on (sqrt(w) J, sqrt(w) r).
 * ZERO WEIGHTS.  A row whose weight is exactly 0 contributes exactly nothing: the forward never multiplies that row's J values or r (they
 * may hold NaN or Inf: a measurement that is missing in some problems of the batch, under one layout), and in the backward dJ_blocks and dr
 * at that row are exactly 0.  dweights at that row is computed like any other row, from whatever the data hold -- a caller that masks does
 * not ask for it.  No sign or range is asked of w; a negative weight can make G indefinite (the solve then reports it in its status).
 * weights: [batch][sum R_b] with weights_stride in elements, 0 = one instance for the batch.  weights == NULL: each call IS its sibling,
 * bit for bit (dweights, as an output or as a tangent, is then MO_ERR_INVALID_ARGUMENT: "... weights is NULL").  J_stride = 0 with per-problem
 * weights -- one fixed linear model, per-problem confidences -- is the main case: J is read in place, never expanded.
 * No allocation and no synchronisation on any launch path; argument errors are judged before the plan is looked at, as the siblings do.
 *
 * mo_linearize_blocks_weighted: mo_linearize_blocks with the weights (G_out == NULL included).  No LDS rule: J_blocks, r and the weights go
 * through LDS when (sum R_b P_b + 2 sum R_b) values fit 48 KiB (rows more than the sibling) and are read from global memory otherwise. */
int mo_linearize_blocks_weighted(mo_plan* plan, const mo_residual_layout* layout, const void* J_blocks, int64_t J_stride, const void* r,
                                 int64_t r_stride, const void* weights, int64_t weights_stride, double lambda, const void* lambda_vec,
                                 int64_t lambda_stride, int64_t batch, void* G_out, int64_t G_stride, int32_t G_ld, void* c_out, int64_t c_stride,
                                 void* half_sq_out, void* stream);
/* mo_qp_gradients_blocks_weighted: mo_qp_gradients_blocks for the weighted cost.  With t = J_b x_loc + r_b and s = J_b u_loc (the kernel's t
 * and w), per stacked row:
 *   dJ_blocks[e] = w_row x (the unweighted value, repeated-variable term included)        dr[row] = -w_row s[row]        dlambda unchanged
 *   dweights[row] = -s[row] t[row] + sum over the pairs {p, p'} of local columns of the row's block on ONE variable i of  u_i x_i J[row, p] J[row, p']
 * The last sum is the derivative of the pair rule: such a pair lands once on the diagonal, so G lacks one w J_p . J_p' against the dense
 * J^T W J, whose derivative -s t would count it twice; it exists only for blocks that name a variable twice (the pair lists are built by
 * mo_residual_layout_create and are empty for almost every layout).  J_blocks and r are read for dJ_blocks, dr and dweights.
 * MO_ERR_UNSUPPORTED if (2 n + 3 sum R_b) values (x, u_x; t, s, the weights) exceed 63 KiB -- sum R_b values more than the sibling. */
typedef struct {
  void* dJ_blocks; int64_t dJ_stride;
  void* dr;        int64_t dr_stride;
  void* dlambda;   int64_t dlambda_stride;
  void* dweights;  int64_t dweights_stride;   /* sum R_b per problem */
} mo_block_weighted_grads;
int mo_qp_gradients_blocks_weighted(mo_plan* plan, const mo_residual_layout* cost_layout, const void* J_blocks, int64_t J_stride, const void* r,
                                    int64_t r_stride, const void* weights, int64_t weights_stride, int64_t batch, const void* vars,
                                    int64_t vars_stride, const void* u, int64_t u_stride, const mo_block_weighted_grads* out, void* stream);
/* mo_qp_tangent_rhs_blocks_weighted: mo_qp_tangent_rhs_blocks for the weighted cost, rho_d += Gdot x + cdot with
 *   Gdot = sum_b (dJ_b^T W_b J_b + J_b^T W_b dJ_b + J_b^T Wdot_b J_b)  (pair rule)      cdot = sum_b (dJ_b^T W_b r_b + J_b^T Wdot_b r_b + J_b^T W_b dr_b)
 * i.e. the sibling's walk with  t := w t  and  tdot := w tdot + wdot t  per stacked row, the repeated-variable correction carrying the row's
 * weight (and wdot, each pair once).  dweights is the tangent of the weights (NULL: zero; stride 0 = one direction for the batch); J_blocks
 * is read with dJ_blocks, dr or dweights, r with dJ_blocks or dweights.  A row whose weight is 0 and whose wdot is 0 or absent is skipped.
 * The transpose identity of the sibling holds with dweights among the members.
 * MO_ERR_UNSUPPORTED if (2 n + 2 k + m + 3 sum R_b) values + 4 m bytes exceed 64 KiB -- sum R_b values more than the sibling. */
typedef struct {
  const void* dJ_blocks;    int64_t dJ_stride;
  const void* dr;           int64_t dr_stride;
  const void* dlambda;      int64_t dlambda_stride;
  const void* dJ_eq_blocks; int64_t dJ_eq_stride;
  const void* dr_eq;        int64_t dr_eq_stride;
  const void* dcons_a; const void* dcons_b; int64_t dcons_stride;
  const void* dweights;     int64_t dweights_stride;   /* sum R_b */
} mo_block_weighted_tangents;
int mo_qp_tangent_rhs_blocks_weighted(mo_plan* plan, const mo_residual_layout* cost_layout, const void* J_blocks, int64_t J_stride,
                                      const void* r, int64_t r_stride, const void* weights, int64_t weights_stride,
                                      const mo_residual_layout* eq_layout, const int32_t* cons_var, int64_t cons_stride, int64_t batch,
                                      const void* vars, int64_t vars_stride, const mo_block_weighted_tangents* t, void* rho, int64_t rho_stride,
                                      void* stream);

/* mo_qp_gradients_blocks_weighted_shared: the outputs of mo_qp_gradients_blocks_weighted SUMMED over the batch, for ONE instance of J_blocks
 * under weights and residuals per problem (weights_stride, r_stride != 0) or given once (stride 0).  Stacked row rho lies in block b with
 * local columns p on the variables i_p = idx_b[p]; the sums run over the problems k that count (every given status word is
 * MO_STATUS_OK); x, u are the x parts of vars, u.  Per problem
 *   t_rho = sum_p J[rho, p] x[i_p] + r_rho        s_rho = sum_p J[rho, p] u[i_p]
 *   a_rho = w_rho t_rho,  c_rho = w_rho s_rho     both exactly 0, formed without a multiplication, where w_rho == 0
 * and
 *   dJ_blocks[rho, p] = -sum_k (u[i_p] a_rho + x[i_p] c_rho) + (sum over the OTHER local columns q' on p's variable of J[rho, q']) sum_k w_rho u[i_p] x[i_p]
 *   dr[rho]           = -sum_k c_rho                                  (only with r_stride == 0)
 *   dweights[rho]     = -sum_k s_rho t_rho + sum over the pairs {p, p'} of the row's block on ONE variable i of J[rho, p] J[rho, p'] sum_k u_i x_i     (only with weights_stride == 0)
 *   dlambda           = -sum_k sum_i u_i x_i                          (ONE value: the caller masks it where lambda <= 0)
 * The second terms of dJ_blocks and dweights exist only for layouts whose partner / pair lists are non-empty; the partner sums and pair
 * products of J leave the batch sum because J is one instance.  The weights do not: sum_k w_rho u x^T is another matrix for every row, so
 * nothing factors through the moments of mo_qp_gradients_blocks_shared, and every problem's t and s are formed on chip and consumed at the
 * packed positions at once (values multiply-adds each; no rows x n product, no [batch][values] gradient).
 * ZERO WEIGHTS as in the sibling, per problem: a row with w_rho == 0 in problem k may hold NaN in that problem's r and contributes exactly
 * nothing to dJ_blocks and dr; dweights at a row is computed from whatever the data hold.  A problem that does not count contributes
 * exactly nothing, whatever its rows of vars / u / r / weights hold.
 * The plan is that of the (G, c) solve.  The equality and constraint members are not part of this call: they go through
 * mo_qp_gradients_blocks_shared / mo_qp_gradients_shared, which read no weights.
 * Arguments are judged before the plan is looked at.  MO_ERR_INVALID_ARGUMENT, with nothing written: NULL cost_layout / out / J_blocks /
 * r / weights; dr with r_stride != 0; dweights with weights_stride != 0; a workspace smaller than the query reports for the same
 * arguments, or not 16-byte aligned.  MO_ERR_DIMENSION: the layout's n differs from the plan's; vars_stride / u_stride < V.
 * MO_ERR_UNSUPPORTED, before any launch: ONE staged problem -- (2 n + 2 sum R_b) values (x, u_x, r, w), and sum R_b values more when
 * dweights is asked for (s t) -- exceeds 64 KiB less the 64 bytes of the kernel's flags.  The kernel stages the largest of 16, 8, 4, 2
 * problems whose rows fit 48 KiB, else 1.  J_blocks is not kept in LDS: it is read in place (one instance, the same addresses for every
 * problem), so `values` has no LDS rule.  batch == 0 writes zeros.
 * The chunks are those of mo_qp_gradients_shared (a function of batch and CU count alone).  Partial kernel: a workgroup owns a chunk and
 * 2048 packed values in registers; t, s per (problem, row), then every value's sum in problem order, each product rounded before it is
 * added; a masked problem is skipped whole.  The finish sums the chunk partials in chunk order in double, forms every output in double
 * through the layout's schedules and rounds once.  One owner per workspace and output element: no atomics, no memset, the same bits on
 * every launch of one device, and each member alone gets the bits it gets beside the others.  No allocation and no synchronisation on
 * the launch path: at most three kernels on `stream`.  The workspace's contents are scratch. */
typedef struct {            /* ONE instance per member; NULL = neither computed nor written */
  void* dJ_blocks;          /* cost_layout values, the packing of J_blocks */
  void* dr;                 /* cost_layout rows; only with r_stride == 0 */
  void* dlambda;            /* 1 */
  void* dweights;           /* cost_layout rows; only with weights_stride == 0 */
} mo_block_weighted_shared_grads;
int mo_qp_gradients_blocks_weighted_shared_workspace(const mo_plan* plan, const mo_residual_layout* cost_layout, int64_t r_stride,
                                                     int64_t weights_stride, int64_t batch, const mo_block_weighted_shared_grads* out,
                                                     int64_t* bytes);
int mo_qp_gradients_blocks_weighted_shared(mo_plan* plan, const mo_residual_layout* cost_layout, const void* J_blocks /* one instance */,
                                           const void* r, int64_t r_stride, const void* weights, int64_t weights_stride, int64_t batch,
                                           const void* vars, int64_t vars_stride, const void* u, int64_t u_stride,
                                           const int32_t* status_fwd, const int32_t* status_adj,
                                           const mo_block_weighted_shared_grads* out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Robust loss functions for residual-block costs (the reference has none): the weights of the weighted cost above
 * derived from the residuals themselves, one loss per block b in the rho(s) convention with s_b = |r_b|^2 (all R_b rows) and scale a_b > 0,
 *   f = 1/2 sum_b rho_b(s_b)        w_b = rho_b'(s_b)        G = sum_b w_b J_b^T J_b (+ lambda I)        c = sum_b w_b J_b^T r_b
 *   TRIVIAL  rho = s                                                   rho' = 1
 *   HUBER    rho = s (s <= a^2), 2 a sqrt(s) - a^2                     rho' = 1 (s <= a^2), a / sqrt(s)
 *   SOFT_L1  rho = 2 a^2 (sqrt(1 + s / a^2) - 1)                       rho' = 1 / sqrt(1 + s / a^2)
 *   CAUCHY   rho = a^2 log1p(s / a^2)                                  rho' = 1 / (1 + s / a^2)
 *   TUKEY    rho = (a^2 / 3)(1 - (1 - s / a^2)^3) (s <= a^2), a^2 / 3  rho' = (1 - s / a^2)^2 (s <= a^2), 0
 * Every row of a block carries the block's w_b; c is the exact gradient of f, G the positive semidefinite IRLS model (no rho'' term).
 * TUKEY beyond its cutoff gives w_b EXACTLY 0 and falls under the ZERO WEIGHTS rule above.  A NaN in r_b makes w_b and f NaN.
 * Fixed summation orders, the same bits on every launch: s_b adds the squares of its rows in order, each rounded before it is added; a lane
 * adds the rho_b of blocks tid, tid + 256, ... in that order and the workgroup sums the lanes like half_sq_out of mo_linearize_blocks. */
typedef enum { MO_LOSS_TRIVIAL = 0, MO_LOSS_HUBER = 1, MO_LOSS_SOFT_L1 = 2, MO_LOSS_CAUCHY = 3, MO_LOSS_TUKEY = 4 } mo_loss_kind;
typedef struct mo_residual_loss mo_residual_loss;
/* kinds[b] (mo_loss_kind), scales[b] = a_b: HOST arrays of the layout's num_blocks entries; the table is uploaded once, as double and as
 * float (it serves plans of either dtype on the layout's device): all allocation happens here, none in a launch.  The layout is read here
 * only.  MO_ERR_INVALID_ARGUMENT naming the block: an unknown kind; a scale that is not finite or not > 0 on a non-TRIVIAL block (a
 * TRIVIAL block's scale is ignored).  A table whose every entry is TRIVIAL is flagged: every call below then IS its sibling, bit for bit. */
int mo_residual_loss_create(const mo_residual_layout* layout, const int32_t* kinds, const double* scales, mo_residual_loss** out);
int mo_residual_loss_destroy(mo_residual_loss* loss);
/* weights_out [batch][sum R_b] (may be NULL; weights_stride in elements): w_b repeated over the block's rows, the layout
 * mo_linearize_blocks_weighted reads.  rho_out [batch] (may be NULL) = 1/2 sum_b rho_b(s_b).  fp64 and fp32 plans; r_stride 0 = one
 * instance.  For callers who run their own IRLS through the weighted calls, and the second route of mo_linearize_blocks_robust. */
int mo_residual_loss_eval(mo_plan* plan, const mo_residual_layout* layout, const mo_residual_loss* loss, const void* r, int64_t r_stride,
                          int64_t batch, void* weights_out, int64_t weights_stride, void* rho_out, void* stream);
/* mo_linearize_blocks with the loss: ONE kernel stages r, forms s_b, w_b, rho_b per block into the LDS slot of the weighted kernel's weights
 * and proceeds as mo_linearize_blocks_weighted -- no [batch][rows] weights go through memory.  half_sq_out = 1/2 sum rho.
 * BITS: G_out, c_out and half_sq_out equal what mo_residual_loss_eval followed by mo_linearize_blocks_weighted (G, c) and rho_out
 * (half_sq_out) give.  weights_out (may be NULL): the weights the kernel used, for outlier diagnosis.  Staging rule of the weighted sibling,
 * (sum R_b P_b + 2 sum R_b) values within 48 KiB; a layout beyond it runs the two launches above through weights_out, and with weights_out
 * NULL there the call returns MO_ERR_UNSUPPORTED before any launch ("... pass weights_out").  G_out == NULL, lambda_vec and J_stride == 0
 * as in the siblings.  loss == NULL or all TRIVIAL: mo_linearize_blocks (weights_out, when given, is filled with 1 on the stream). */
int mo_linearize_blocks_robust(mo_plan* plan, const mo_residual_layout* layout, const void* J_blocks, int64_t J_stride, const void* r,
                               int64_t r_stride, double lambda, const void* lambda_vec, int64_t lambda_stride, int64_t batch, void* G_out,
                               int64_t G_stride, int32_t G_ld, void* c_out, int64_t c_stride, void* half_sq_out, const mo_residual_loss* loss,
                               void* weights_out, int64_t weights_stride, void* stream);
/* mo_nls_solve_blocks minimising f = 1/2 sum_b rho_b(|r_b|^2) over the cost blocks: every outer iteration linearises with
 * mo_linearize_blocks_robust (errors_pre.f = its 1/2 sum rho), every line-search candidate's f is mo_residual_loss_eval's rho_out on r_cand;
 * penalty selection, directional derivatives (c^T dx is exact: c is the gradient of f), eigenvalue logging and the QP read the assembled
 * (G, c) as before.  Equality residuals take no loss.  cost_loss NULL or all TRIVIAL: mo_nls_solve_blocks, same launches, same bits.
 * The per-call scratch gains a [batch][sum R_b] weight buffer only when the cost layout does not stage. */
int mo_nls_solve_blocks_robust(mo_plan* plan, const mo_nls_problem* np, const mo_residual_layout* cost_layout,
                               const mo_residual_loss* cost_loss, const mo_residual_layout* eq_layout, int64_t batch,
                               const mo_nls_params* params, mo_nls_eval_fn eval, void* user, int32_t* termination, int32_t* num_iterations,
                               void* iterations, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MINI_OPT_HIP_H_ */
