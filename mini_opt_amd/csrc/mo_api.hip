// mo_api.hip -- implementation of the C ABI declared in include/mini_opt_hip.h.
// Validation mirrors QPInteriorPointSolver::Setup (qp.cc:20-73) and CheckParams (qp.cc:76-82); everything numeric
// happens in the gfx950 kernels (kkt_generic.hip, kkt_fused*.hip; which one serves a call: mo::decide_kernel, mo_fused_select.h).  There is NO CPU fallback: without a usable HIP
// device every entry point fails with MO_ERR_NO_DEVICE / MO_ERR_HIP.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <new>
#include <vector>

#include "mo_fused_select.h"
#include "mo_kernels.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

#define MO_HIP_CHECK(expr)                                                                     \
  do {                                                                                         \
    hipError_t e__ = (expr);                                                                   \
    if (e__ != hipSuccess) return fail(MO_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e__)); \
  } while (0)

}  // namespace

struct mo_plan {
  mo_plan_desc desc;
  int num_cus;
  int elem;
  size_t generic_lds;
  // scratch for mo_qp_solve with J-level input: G [max_batch][n*n], c [max_batch][n]
  void* G_scratch;
  void* c_scratch;
  // generic kernel beyond its LDS-resident range: one H workspace per workgroup of the persistent grid.  Sized and allocated ONCE, in
  // mo_plan_create, for every launch shape the plan can produce (the full system and the k = m = 0 system of mo_linearize / mo_fill_qp);
  // launches only read these three fields -- no allocation, no synchronisation, nothing plan-owned changes on the launch path.
  void* H_work;
  size_t H_work_slot_bytes; // bytes per workgroup slot (also the eigenvalue kernel's n x n fp64 matrix beyond the LDS)
  long long H_work_slots;   // workgroup slots allocated: a launch's grid is clamped to it
  void* tile_scratch;  // fused Solve: per wave slot of the persistent grid, the G tiles a wave cannot park in LDS between passes
  unsigned long long* ticket;  // device work counter of the fused kernels (zeroed on the stream before each launch)
};

// Residual-block layout: the gather schedule of residual_blocks.hip, built once on the host and uploaded in one allocation.
struct mo_residual_layout {
  int device, n, num_blocks, rows;
  long long values;
  void* dev;
  const int* g_ptr; const int4* g_ent; const int* c_ptr; const int4* c_ent; const int2* row_info; const int* win;
  // the backward schedule (mo_qp_gradients_blocks / mo_qp_gradients_eq_blocks, mo::BlockGradArgs)
  const int4* d_row; const int4* d_val; const int2* e_val; const int* d_idx; const int* d_dup;
  // the pairs of local columns on one variable, per stacked row (mo_qp_gradients_blocks_weighted: dweights)
  const int* d_pair; const int* d_plist;
  // the forward-mode schedule of an equality layout (mo_qp_tangent_rhs_blocks, mo::BlockTangentArgs): c_ptr / c_ent filtered by winners
  const int* w_ptr; const int4* w_ent;
  int has_dup;   // some block names a variable twice: d_dup and d_plist are non-empty (mo_qp_gradients_blocks_weighted_shared)
  std::vector<int> block_rows;   // R_b on the host: what mo_residual_loss_create builds its table from
};

// Loss table of a layout's blocks (mo_loss_device.h): one device allocation [blk | scales as double | scales as float]
struct mo_residual_loss {
  int device, num_blocks, rows, all_trivial;
  void* dev;
  const int4* blk; const double* scale_d; const float* scale_f;
};

namespace {

int check_plan(const mo_plan* plan) {
  if (!plan) return fail(MO_ERR_INVALID_ARGUMENT, "plan is NULL");
  return MO_OK;
}

// The product library reads NO environment variable (the reference has none): kernel selection and scheduling follow the
// plan flags of include/mini_opt_hip.h only.  The getenv knobs of the A/B scripts exist in builds with -DMO_TUNING (tools/ab_build.sh).
bool generic_forced(const mo_plan* plan) {
#ifdef MO_TUNING
  static const bool env_force_generic = getenv("MO_FORCE_GENERIC") != nullptr;  // A/B and bisection knob
  if (env_force_generic) return true;
#endif
  return (plan->desc.flags & MO_PLAN_FORCE_GENERIC) != 0;
}

// Launches of at most this many problems per wave of the persistent grid are split statically (KernelArgs::static_rounds): -1 = the selector's
// own choice per kernel family (mo_fused_select.h); MO_PLAN_TICKETS_ALWAYS -> 0, MO_PLAN_STATIC_ROUNDS_ALWAYS -> every launch
int fused_static_rounds(const mo_plan* plan) {
#ifdef MO_TUNING
  static const int v = [] { const char* e = getenv("MO_FUSED_STATIC_ROUNDS"); return e ? atoi(e) : -1; }();
  if (v >= 0) return v;
#endif
  if (plan->desc.flags & MO_PLAN_TICKETS_ALWAYS) return 0;
  if (plan->desc.flags & MO_PLAN_STATIC_ROUNDS_ALWAYS) return 1 << 30;
  return -1;
}

// The equality and inequality rows of the system a call works on, where that is not the plan's own: the cost alone (mo_linearize, the
// eigenvalue statistics) or the problem without its inequalities (the null-space solver).  -1: the plan's.
struct Dims { int k = -1, m = -1; };

// Every KernelArgs starts here: the dimension / pointer checks shared by every batched entry point (the F_ASSERTs of qp.cc:21-34) and the
// plan-scoped fields of the fused kernels.
int fill_problem(const mo_plan* plan, const mo_problem* prob, int64_t batch, bool need_cost, bool need_constraints,
                 mo::KernelArgs* a, Dims dims = Dims()) {
  if (!prob) return fail(MO_ERR_INVALID_ARGUMENT, "Must pass a non-null problem");
  if (batch < 0) return fail(MO_ERR_INVALID_ARGUMENT, "batch must be >= 0");
  const mo_plan_desc& d = plan->desc;
  const int k = dims.k >= 0 ? dims.k : d.k, m = dims.m >= 0 ? dims.m : d.m;
  memset(a, 0, sizeof(*a));
  a->n = d.n; a->k = k; a->m = m; a->m_r = 0;
  a->batch = batch;
  a->ticket = plan->ticket; a->static_rounds = fused_static_rounds(plan); a->no_tiny = (d.flags & MO_PLAN_NO_TINY) != 0;
  if (need_cost) {
    if (prob->J) {
      if (d.m_r <= 0) return fail(MO_ERR_DIMENSION, "J given but the plan was created with m_r = 0");
      if (!prob->r) return fail(MO_ERR_INVALID_ARGUMENT, "J given without r");
      if (prob->J_layout != MO_ROW_MAJOR && prob->J_layout != MO_COL_MAJOR)
        return fail(MO_ERR_INVALID_ARGUMENT, "bad J_layout");
      const int min_ld = prob->J_layout == MO_ROW_MAJOR ? d.n : d.m_r;
      if (prob->J_ld < min_ld) return fail(MO_ERR_DIMENSION, "J_ld %d < %d", prob->J_ld, min_ld);
      a->J = prob->J; a->J_stride = prob->J_stride; a->J_ld = prob->J_ld; a->J_row_major = prob->J_layout == MO_ROW_MAJOR;
      a->r = prob->r; a->r_stride = prob->r_stride; a->lambda = prob->lambda; a->m_r = d.m_r;
      a->lambda_vec = prob->lambda_vec; a->lambda_vec_stride = prob->lambda_stride;
    } else {
      if (!prob->G || !prob->c) return fail(MO_ERR_INVALID_ARGUMENT, "need either (J, r) or (G, c)");
      if (prob->G_ld < d.n) return fail(MO_ERR_DIMENSION, "G must be square: G_ld %d < n %d", prob->G_ld, d.n);
      a->G = prob->G; a->G_stride = prob->G_stride; a->G_ld = prob->G_ld;
      a->c = prob->c; a->c_stride = prob->c_stride;
    }
  }
  if (k > 0) {
    if (!prob->A_eq || !prob->b_eq) return fail(MO_ERR_DIMENSION, "Rows of A_e and b_e must match (k = %d but NULL given)", k);
    if (prob->A_ld < k) return fail(MO_ERR_DIMENSION, "A_ld %d < k %d", prob->A_ld, k);
    a->A = prob->A_eq; a->A_stride = prob->A_stride; a->A_ld = prob->A_ld;
    a->b = prob->b_eq; a->b_stride = prob->b_stride;
  }
  if (m > 0 && need_constraints) {
    if (!prob->cons_var || !prob->cons_a || !prob->cons_b)
      return fail(MO_ERR_INVALID_ARGUMENT, "m = %d but constraint arrays are NULL", m);
    a->cons_var = prob->cons_var; a->cons_a = prob->cons_a; a->cons_b = prob->cons_b; a->cons_stride = prob->cons_stride;
  }
  return MO_OK;
}

// Which kernel serves a call is decided ONCE, by mo::decide_kernel (mo_fused_select.h) from the arguments, the plan's dtype and the
// force-generic flag (read a single time: the scratch a call prepares and the kernel that consumes it must come from the same decision).
mo::KernelDecision decide(const mo_plan* plan, const mo::KernelArgs& a) {
  return mo::decide_kernel(a, plan->desc.dtype, generic_forced(plan), plan->num_cus);
}

int launch(const mo_plan* plan, mo::KernelArgs a, const mo::KernelDecision& d, void* stream) {
  if (a.batch == 0) return MO_OK;
  MO_HIP_CHECK(hipSetDevice(plan->desc.device));
  hipStream_t s = (hipStream_t)stream;
  if (d.kind == mo::KERNEL_FUSED_F64) {
    MO_HIP_CHECK(mo::launch_fused(a, plan->desc.dtype, plan->num_cus, s));
  } else if (d.kind == mo::KERNEL_FUSED_F32) {
    MO_HIP_CHECK(mo::launch_fused_f32(a, plan->num_cus, s));
  } else if (d.kind == mo::KERNEL_FUSED_RHS) {
    MO_HIP_CHECK(mo::launch_fused_rhs(a, plan->desc.dtype, plan->num_cus, s));
  } else {
    if (mo::generic_needs_large(a, plan->elem)) {  // H in a global workspace per workgroup: plan-owned, allocated by mo_plan_create
      const size_t need = mo::generic_large_lds_bytes(a, plan->elem);
      if (need > mo::kLdsBytes)
        return fail(MO_ERR_UNSUPPORTED, "n = %d, k = %d, m = %d: not even the state / residual vectors of one problem fit the 160 KiB of LDS", a.n, a.k, a.m);
      if (!plan->H_work || mo::generic_large_workspace_elems(a) * plan->elem > plan->H_work_slot_bytes)
        return fail(MO_ERR_UNSUPPORTED, "the plan owns no H workspace for n = %d, k = %d (created for n = %d, k = %d)", a.n, a.k, plan->desc.n, plan->desc.k);
      a.H_work = plan->H_work; a.H_work_stride = (long long)(plan->H_work_slot_bytes / plan->elem); a.H_work_slots = plan->H_work_slots;
    }
    MO_HIP_CHECK(mo::launch_generic(a, plan->desc.dtype, plan->num_cus, s));
  }
  return MO_OK;
}

int launch(const mo_plan* plan, const mo::KernelArgs& a, void* stream) { return launch(plan, a, decide(plan, a), stream); }

// What mo_plan_step_kernel / mo_plan_solve_kernel / mo_plan_kkt_solve_kernel report: the name of the decision for a one-problem call.
const char* plan_kernel_name(const mo_plan* plan, const mo_problem* prob, int mode) {
  if (!plan || !prob) return "invalid";
  mo::KernelArgs a;
  if (fill_problem(plan, prob, 1, true, true, &a) != MO_OK) return "invalid";
  a.mode = mode;
  // layout query only: assume a 16-byte aligned, densely packed state / output (the right-hand side of mo_kkt_solve has no alignment rule)
  a.vars = a.delta = reinterpret_cast<void*>(16);
  a.rhs = reinterpret_cast<const void*>(32);
  a.vars_stride = a.delta_stride = a.rhs_stride = plan->desc.n + 2 * plan->desc.m + plan->desc.k;
  return decide(plan, a).name;
}

// What mo_qp_gradients and mo_qp_tangent_rhs share once their own argument checks have passed: the plan, the shape, the state, and the rule
// of who reads J.  `mem` is the caller's copy of its mo_qp_grads / mo_qp_tangents (the members named here carry the same names in both): the
// members of rows the plan does not have are dropped, and J, r are checked and handed over only if dJ or dr is among the rest.
template <typename Members>
int sens_args(const mo_plan* plan, const mo_problem* prob, int64_t batch, const void* vars, int64_t vars_stride, Members* mem, mo::SensArgs* a) {
  if (int rc = check_plan(plan)) return rc;
  const mo_plan_desc& d = plan->desc;
  a->n = d.n; a->k = d.k; a->m = d.m; a->batch = batch;
  a->vars = vars; a->vars_stride = vars_stride;
  if (d.k == 0) { mem->dA_eq = nullptr; mem->db_eq = nullptr; }
  if (d.m == 0) { mem->dcons_a = nullptr; mem->dcons_b = nullptr; }
  if (mem->dJ || mem->dr) {
    if (d.m_r <= 0) return fail(MO_ERR_DIMENSION, "J given but the plan was created with m_r = 0");
    if (prob->J_layout != MO_ROW_MAJOR && prob->J_layout != MO_COL_MAJOR) return fail(MO_ERR_INVALID_ARGUMENT, "bad J_layout");
    const int min_ld = prob->J_layout == MO_ROW_MAJOR ? d.n : d.m_r;
    if (prob->J_ld < min_ld) return fail(MO_ERR_DIMENSION, "J_ld %d < %d", prob->J_ld, min_ld);
    a->m_r = d.m_r;
    a->J = prob->J; a->J_stride = prob->J_stride; a->J_ld = prob->J_ld; a->J_row_major = prob->J_layout == MO_ROW_MAJOR;
    a->r = prob->r; a->r_stride = prob->r_stride;
  }
  return MO_OK;
}

// ... and after their checks of dJ: the leading dimensions of the other two matrix members
template <typename Members> int check_dG_dA_ld(const mo_plan_desc& d, const Members& mem) {
  if (mem.dG && mem.dG_ld < d.n) return fail(MO_ERR_DIMENSION, "dG_ld %d < n %d", mem.dG_ld, d.n);
  if (mem.dA_eq && mem.dA_ld < d.k) return fail(MO_ERR_DIMENSION, "dA_ld %d < k %d", mem.dA_ld, d.k);
  return MO_OK;
}

// The one judge of the dense gradient members (mo_qp_gradients, mo_qp_gradients_shared and its workspace query): what the arguments alone
// tell, then the plan (sens_args) and the members against it.  summed: ONE instance per member, summed over the batch -- J and the constraint
// set must then have stride 0.  `a` (a GradArgs or the SharedGradArgs derived from it) arrives zeroed; the LDS rules stay with the callers.
int grad_args(const mo_plan* plan, const mo_problem* prob, int64_t batch, const void* vars, int64_t vars_stride, const mo_qp_grads* out,
              bool summed, mo::GradArgs* a) {
  if (!prob) return fail(MO_ERR_INVALID_ARGUMENT, "Must pass a non-null problem");
  if (!out) return fail(MO_ERR_INVALID_ARGUMENT, "out is NULL");
  if (batch < 0) return fail(MO_ERR_INVALID_ARGUMENT, "batch must be >= 0");
  const bool j_level = prob->J != nullptr;
  if (j_level && out->dG) return fail(MO_ERR_INVALID_ARGUMENT, "dG asked for with J-level input: ask for dJ / dr / dlambda");
  if (!j_level && (out->dJ || out->dr || out->dlambda))
    return fail(MO_ERR_INVALID_ARGUMENT, "dJ / dr / dlambda asked for with (G, c) input: ask for dG / dc");
  if (summed && (out->dJ || out->dr) && prob->J_stride != 0)
    return fail(MO_ERR_INVALID_ARGUMENT, "dJ / dr summed over the batch need one J for the batch: J_stride is %lld, not 0", (long long)prob->J_stride);
  a->out = *out;
  if (int rc = sens_args(plan, prob, batch, vars, vars_stride, &a->out, a)) return rc;
  const mo_plan_desc& d = plan->desc;
  if (summed && (a->out.dcons_a || a->out.dcons_b) && prob->cons_stride != 0)
    return fail(MO_ERR_INVALID_ARGUMENT, "dcons_a / dcons_b summed over the batch need one constraint set for the batch: cons_stride is %lld, not 0",
                (long long)prob->cons_stride);
  if (a->J && !prob->r) return fail(MO_ERR_INVALID_ARGUMENT, "J given without r");   // (t, w = J x + r: both outputs that read J read r)
  if (a->out.dJ) {
    if (a->out.dJ_layout != MO_ROW_MAJOR && a->out.dJ_layout != MO_COL_MAJOR) return fail(MO_ERR_INVALID_ARGUMENT, "bad dJ_layout");
    const int min_dld = a->out.dJ_layout == MO_ROW_MAJOR ? d.n : d.m_r;
    if (a->out.dJ_ld < min_dld) return fail(MO_ERR_DIMENSION, "dJ_ld %d < %d", a->out.dJ_ld, min_dld);
  }
  if (int rc = check_dG_dA_ld(d, a->out)) return rc;
  if (a->out.dcons_a) {
    if (!prob->cons_var) return fail(MO_ERR_INVALID_ARGUMENT, "dcons_a asked for but cons_var is NULL");
    a->cons_var = prob->cons_var; a->cons_stride = summed ? 0 : prob->cons_stride;
  }
  return MO_OK;
}

// The tail of the two batch-reduced launches, once their members are judged: vars, u and the workspace (`query` names its `need` bytes)
int reduced_call_tail(const mo_plan* plan, int64_t batch, const void* vars, int64_t vars_stride, const void* u, int64_t u_stride,
                      const void* workspace, int64_t workspace_bytes, size_t need, const char* query) {
  if (batch > 0 && (!vars || !u)) return fail(MO_ERR_INVALID_ARGUMENT, "vars / u is NULL");
  const int V = plan->desc.n + 2 * plan->desc.m + plan->desc.k;
  if (batch > 1 && (vars_stride < V || u_stride < V)) return fail(MO_ERR_DIMENSION, "vars_stride %lld / u_stride %lld < V = %d", (long long)vars_stride, (long long)u_stride, V);
  if (!workspace || workspace_bytes < (int64_t)need)
    return fail(MO_ERR_INVALID_ARGUMENT, "workspace too small: %lld bytes given, %lld needed (%s)", (long long)(workspace ? workspace_bytes : 0), (long long)need, query);
  if ((uintptr_t)workspace & 15) return fail(MO_ERR_INVALID_ARGUMENT, "workspace is not 16-byte aligned");
  return MO_OK;
}

}  // namespace

namespace {
// scratch of one mo_nls_solve call, released on every exit path
struct NlsScratch {  // one allocation carved into 256-byte aligned pieces
  char* base = nullptr;
  size_t used = 0, capacity = 0;
  ~NlsScratch() { if (base) (void)hipFree(base); }
  static size_t padded(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
  template <typename T> void reserve(size_t elems) { capacity += padded((elems ? elems : 1) * sizeof(T)); }
  hipError_t commit() { return hipMalloc((void**)&base, capacity ? capacity : 256); }
  template <typename T> hipError_t alloc(T** out, size_t elems) {
    const size_t bytes = padded((elems ? elems : 1) * sizeof(T));
    if (!base || used + bytes > capacity) return hipErrorOutOfMemory;
    *out = reinterpret_cast<T*>(base + used);
    used += bytes;
    return hipSuccess;
  }
};
}  // namespace

extern "C" {

const char* mo_version_string(void) { return "mini_opt_hip 0.5 (gfx950)"; }

const char* mo_status_string(int32_t status) {
  switch (status) {
    case MO_STATUS_OK: return "OK";
    case MO_STATUS_NONPOSITIVE_SLACK: return "NONPOSITIVE_SLACK";
    case MO_STATUS_FACTORIZATION_FAILED: return "FACTORIZATION_FAILED";
    case MO_STATUS_NONFINITE: return "NONFINITE";
    case MO_STATUS_BAD_INDEX: return "BAD_INDEX";
    case MO_STATUS_NOT_POSITIVE_DEFINITE: return "NOT_POSITIVE_DEFINITE";
    default: return "UNKNOWN";
  }
}

const char* mo_last_error(void) { return g_err; }

void mo_default_solve_params(mo_solve_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->initial_mu = 1.0;  // qp.hpp:134-164
  p->sigma = 0.5;
  p->termination_kkt_tol = 1.0e-9;
  p->termination_complementarity_tol = 1.0e-6;
  p->max_iterations = 10;
  p->barrier_strategy = MO_COMPLEMENTARITY;
  p->decrease_mu_only_on_small_error = 0;
  p->initial_guess_method = MO_GUESS_NAIVE;
  p->initialize_mu_with_complementarity = 0;
}

int mo_plan_create(const mo_plan_desc* desc, mo_plan** out) {
  g_err[0] = 0;
  if (!desc || !out) return fail(MO_ERR_INVALID_ARGUMENT, "desc/out is NULL");
  *out = nullptr;
  if (desc->n <= 0 || desc->k < 0 || desc->m < 0 || desc->m_r < 0)
    return fail(MO_ERR_DIMENSION, "bad dimensions n=%d k=%d m=%d m_r=%d", desc->n, desc->k, desc->m, desc->m_r);
  if (desc->dtype != MO_F64 && desc->dtype != MO_F32) return fail(MO_ERR_UNSUPPORTED, "unknown dtype %d", desc->dtype);
  if (desc->max_batch < 0) return fail(MO_ERR_INVALID_ARGUMENT, "max_batch must be >= 0 (got %lld)", (long long)desc->max_batch);
  {
    // Any size Setup accepts (qp.cc:36-48 resizes to any N, K): beyond the fused kernels and the LDS-resident generic kernel (n + k <= 192,
    // H in LDS) the generic kernel keeps H in a global workspace; only a problem whose state / residual vectors alone exceed the LDS is refused.
    mo::KernelArgs sz;
    memset(&sz, 0, sizeof(sz));
    sz.n = desc->n; sz.k = desc->k; sz.m = desc->m; sz.m_r = desc->m_r;
    const int elem = desc->dtype == MO_F64 ? 8 : 4;
    if (mo::generic_needs_large(sz, elem) && mo::generic_large_lds_bytes(sz, elem) > mo::kLdsBytes)
      return fail(MO_ERR_UNSUPPORTED, "n = %d, k = %d, m = %d: the state / residual vectors of one problem exceed the 160 KiB of LDS", desc->n, desc->k, desc->m);
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(MO_ERR_NO_DEVICE, "no HIP device available (the HIP path has no CPU fallback)");
  if (desc->device < 0 || desc->device >= ndev) return fail(MO_ERR_INVALID_ARGUMENT, "device %d out of range [0,%d)", desc->device, ndev);
  MO_HIP_CHECK(hipSetDevice(desc->device));
  hipDeviceProp_t prop;
  MO_HIP_CHECK(hipGetDeviceProperties(&prop, desc->device));
  mo_plan* p = new (std::nothrow) mo_plan();
  if (!p) return fail(MO_ERR_HIP, "out of host memory");
  p->desc = *desc;
  p->num_cus = prop.multiProcessorCount;
  p->elem = desc->dtype == MO_F64 ? 8 : 4;
  p->G_scratch = nullptr;
  p->c_scratch = nullptr;
  p->tile_scratch = nullptr;
  p->H_work = nullptr;
  p->H_work_slot_bytes = 0;
  p->H_work_slots = 0;
  p->ticket = nullptr;
  if (hipMalloc((void**)&p->ticket, 256) != hipSuccess) {
    delete p;
    return fail(MO_ERR_HIP, "hipMalloc of the work counter failed");
  }
  mo::KernelArgs a;
  memset(&a, 0, sizeof(a));
  a.n = desc->n; a.k = desc->k; a.m = desc->m; a.m_r = desc->m_r;
  p->generic_lds = mo::generic_lds_bytes(a, p->elem);
  // fp64 systems up to n = 128 (k <= 63, m <= 256) run on the fused kernels even when the LDS-resident generic kernel cannot hold them.
  // Beyond the LDS-resident range the generic kernel keeps H in a global workspace per workgroup of its persistent grid: everything that
  // sizes it is known here (shape, dtype, CU count), so it is allocated now -- for the larger of the two systems a plan launches there, the
  // full one and the k = m = 0 one of mo_linearize / mo_fill_qp (fewer LDS bytes per workgroup, hence possibly MORE workgroups per CU) --
  // and never touched again.  max_batch > 0 bounds the number of slots (a launch's grid never exceeds its batch).
  // (mo_qp_eigenvalue_stats keeps its n x n fp64 matrix in the same slots once it exceeds the LDS: n <= 140 is LDS resident, n >= 141 is not)
  if (mo::generic_needs_large(a, p->elem) || mo::eig_needs_global(desc->n)) {
    mo::KernelArgs lin = a;
    lin.k = 0; lin.m = 0;
    long long slots = 0;
    size_t slot_bytes = 0;
    if (mo::generic_needs_large(a, p->elem)) {
      slots = mo::generic_large_grid(a, p->elem, p->num_cus);
      if (desc->m_r > 0 && mo::generic_needs_large(lin, p->elem)) {
        const long long ls = mo::generic_large_grid(lin, p->elem, p->num_cus);
        if (ls > slots) slots = ls;
      }
      slot_bytes = mo::generic_large_workspace_elems(a) * p->elem;   // (n + k) x ld: covers the n x ld(n) of the k = 0 system
    }
    if (mo::eig_needs_global(desc->n)) {
      const long long es = mo::eig_grid(desc->n, p->num_cus);
      if (es > slots) slots = es;
      if (mo::eig_workspace_bytes(desc->n) > slot_bytes) slot_bytes = mo::eig_workspace_bytes(desc->n);
    }
    if (desc->max_batch > 0 && slots > desc->max_batch) slots = desc->max_batch;
    slot_bytes = (slot_bytes + 255) & ~(size_t)255;
    const size_t bytes = (size_t)slots * slot_bytes;
    if (hipMalloc(&p->H_work, bytes) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(p->ticket);
      delete p;
      return fail(MO_ERR_HIP, "hipMalloc of the %zu B workspace of H (n = %d, k = %d: %lld workgroup slots) failed", bytes, desc->n, desc->k, slots);
    }
    p->H_work_slot_bytes = slot_bytes;
    p->H_work_slots = slots;
  }
  // Tile park of the fused fp64 Solve kernels beyond the 32 grid (qp_solve_impl; geometry: mo_fused_select.h): one slot per wave of the
  // persistent grid, 22.5 KB at n = 64, 78 KB at n = 128.  Optional -- without it the kernels rebuild the tiles every
  // pass -- so a failed allocation is not an error.
  if (desc->dtype == MO_F64 && desc->n > 32 && desc->n <= 128 && desc->k <= 63 && desc->m <= 256) {
    if (hipMalloc(&p->tile_scratch, mo::fused_tile_park_slots(p->num_cus) * mo::fused_tile_park_slot_elems(desc->n) * p->elem) != hipSuccess) {
      p->tile_scratch = nullptr;
      (void)hipGetLastError();
    }
  }

  *out = p;
  return MO_OK;
}

int mo_plan_destroy(mo_plan* plan) {
  if (!plan) return MO_OK;
  if (plan->G_scratch) (void)hipFree(plan->G_scratch);
  if (plan->c_scratch) (void)hipFree(plan->c_scratch);
  if (plan->tile_scratch) (void)hipFree(plan->tile_scratch);
  if (plan->H_work) (void)hipFree(plan->H_work);
  if (plan->ticket) (void)hipFree(plan->ticket);
  delete plan;
  return MO_OK;
}

const char* mo_plan_step_kernel(const mo_plan* plan, const mo_problem* prob) { return plan_kernel_name(plan, prob, mo::MODE_STEP); }
const char* mo_plan_solve_kernel(const mo_plan* plan, const mo_problem* prob) { return plan_kernel_name(plan, prob, mo::MODE_SOLVE); }
const char* mo_plan_kkt_solve_kernel(const mo_plan* plan, const mo_problem* prob) { return plan_kernel_name(plan, prob, mo::MODE_RHS); }

int mo_linearize(mo_plan* plan, const mo_problem* prob, int64_t batch, void* G_out, int64_t G_stride, int32_t G_ld,
                 void* c_out, int64_t c_stride, void* half_sq_out, void* stream) {
  g_err[0] = 0;
  if (int rc = check_plan(plan)) return rc;
  mo::KernelArgs a;
  if (prob && !prob->J) return fail(MO_ERR_INVALID_ARGUMENT, "mo_linearize needs J-level input");
  // A_eq / constraints are not touched by the linearisation of the cost
  if (int rc = fill_problem(plan, prob, batch, true, false, &a, Dims{0, 0})) return rc;
  if (!G_out || !c_out) return fail(MO_ERR_INVALID_ARGUMENT, "G_out / c_out is NULL");
  if (G_ld < plan->desc.n) return fail(MO_ERR_DIMENSION, "G_ld %d < n", G_ld);
  a.mode = mo::MODE_LINEARIZE;
  a.G_out = G_out; a.G_out_stride = G_stride; a.G_out_ld = G_ld;
  a.c_out = c_out; a.c_out_stride = c_stride; a.half_sq_out = half_sq_out;
  return launch(plan, a, stream);
}

int mo_fill_qp(mo_plan* plan, const mo_problem* prob, int64_t batch, const void* x, int64_t x_stride, void* G_out,
               int64_t G_stride, int32_t G_ld, void* c_out, int64_t c_stride, void* cons_b_out, int64_t cons_b_stride,
               void* errors_out, int32_t* status, void* stream) {
  g_err[0] = 0;
  if (int rc = check_plan(plan)) return rc;
  if (!prob || !prob->J) return fail(MO_ERR_INVALID_ARGUMENT, "mo_fill_qp needs the cost residual stack (J, r)");
  if (!errors_out) return fail(MO_ERR_INVALID_ARGUMENT, "errors_out is NULL");
  const mo_plan_desc& d = plan->desc;
  if (d.m > 0 && (!x || !cons_b_out)) return fail(MO_ERR_INVALID_ARGUMENT, "x / cons_b_out is NULL");
  mo::KernelArgs ka;
  if (int rc = fill_problem(plan, prob, batch, true, true, &ka)) return rc;  // validates A_eq / b_eq / constraints too
  // cost part: G = J^T J + lambda I, c = J^T r, f = 0.5 |r|^2 (nonlinear.cc:182-189) -> errors_out[2 p]
  mo::KernelArgs a;
  if (int rc = fill_problem(plan, prob, batch, true, false, &a, Dims{0, 0})) return rc;
  if (!G_out || !c_out) return fail(MO_ERR_INVALID_ARGUMENT, "G_out / c_out is NULL");
  if (G_ld < d.n) return fail(MO_ERR_DIMENSION, "G_ld %d < n", G_ld);
  a.mode = mo::MODE_LINEARIZE;
  a.G_out = G_out; a.G_out_stride = G_stride; a.G_out_ld = G_ld;
  a.c_out = c_out; a.c_out_stride = c_stride; a.half_sq_out = errors_out; a.half_sq_stride = 2;
  if (int rc = launch(plan, a, stream)) return rc;
  if (batch == 0) return MO_OK;
  // tail: shifted constraints and the equality L1 norm (nonlinear.cc:192-212)
  mo::AuxArgs x_args;
  memset(&x_args, 0, sizeof(x_args));
  x_args.n = d.n; x_args.k = d.k; x_args.m = d.m; x_args.batch = batch;
  x_args.x = x; x_args.x_stride = x_stride;
  x_args.b = ka.b; x_args.b_stride = ka.b_stride;
  x_args.cons_var = ka.cons_var; x_args.cons_a = ka.cons_a; x_args.cons_b = ka.cons_b; x_args.cons_stride = ka.cons_stride;
  x_args.cons_b_out = cons_b_out; x_args.cons_b_out_stride = cons_b_stride;
  x_args.out2 = errors_out; x_args.status = status;
  MO_HIP_CHECK(mo::launch_shift_constraints(x_args, d.dtype, (hipStream_t)stream));
  return MO_OK;
}

int mo_nonlinear_errors(mo_plan* plan, const void* r, int64_t r_stride, const void* r_eq, int64_t r_eq_stride,
                        int64_t batch, void* errors_out, void* stream) {
  g_err[0] = 0;
  if (int rc = check_plan(plan)) return rc;
  const mo_plan_desc& d = plan->desc;
  if (batch < 0) return fail(MO_ERR_INVALID_ARGUMENT, "batch must be >= 0");
  if (!errors_out) return fail(MO_ERR_INVALID_ARGUMENT, "errors_out is NULL");
  if (d.m_r > 0 && !r) return fail(MO_ERR_INVALID_ARGUMENT, "r is NULL");
  if (d.k > 0 && !r_eq) return fail(MO_ERR_DIMENSION, "k = %d but r_eq is NULL", d.k);
  mo::AuxArgs a;
  memset(&a, 0, sizeof(a));
  a.n = d.n; a.k = d.k; a.m = d.m; a.m_r = d.m_r; a.batch = batch;
  a.r = r; a.r_stride = r_stride; a.b = r_eq; a.b_stride = r_eq_stride; a.out2 = errors_out;
  MO_HIP_CHECK(hipSetDevice(d.device));
  MO_HIP_CHECK(mo::launch_nonlinear_errors(a, d.dtype, (hipStream_t)stream));
  return MO_OK;
}

int mo_qp_cost_derivative(mo_plan* plan, const mo_problem* prob, int64_t batch, const void* dx, int64_t dx_stride,
                          void* deriv_out, void* quad_out, void* stream) {
  g_err[0] = 0;
  if (int rc = check_plan(plan)) return rc;
  const mo_plan_desc& d = plan->desc;
  mo::KernelArgs ka;
  if (int rc = fill_problem(plan, prob, batch, true, false, &ka)) return rc;
  if (!dx || !deriv_out) return fail(MO_ERR_INVALID_ARGUMENT, "dx / deriv_out is NULL");  // F_ASSERT_EQ(qp.c.rows(), dx.rows())
  mo::AuxArgs a;
  memset(&a, 0, sizeof(a));
  a.n = d.n; a.k = d.k; a.m = d.m; a.m_r = ka.m_r; a.batch = batch;
  a.x = dx; a.x_stride = dx_stride;
  a.J = ka.J; a.J_stride = ka.J_stride; a.J_ld = ka.J_ld; a.J_row_major = ka.J_row_major; a.r = ka.r; a.r_stride = ka.r_stride;
  a.G = ka.G; a.G_stride = ka.G_stride; a.G_ld = ka.G_ld; a.c = ka.c; a.c_stride = ka.c_stride;
  a.A = ka.A; a.A_stride = ka.A_stride; a.A_ld = ka.A_ld; a.b = ka.b; a.b_stride = ka.b_stride;
  a.lambda = ka.lambda; a.lambda_vec = ka.lambda_vec; a.lambda_vec_stride = ka.lambda_vec_stride;
  a.out2 = deriv_out; a.quad_out = quad_out;
  MO_HIP_CHECK(hipSetDevice(d.device));
  MO_HIP_CHECK(mo::launch_cost_derivative(a, d.dtype, (hipStream_t)stream));
  return MO_OK;
}

int mo_kkt_residual(mo_plan* plan, const mo_problem* prob, int64_t batch, const void* vars, int64_t vars_stride,
                    const void* mu, int64_t mu_stride, uint32_t flags, void* r_out, int64_t r_stride, void* kkt_out,
                    void* stream) {
  g_err[0] = 0;
  if (int rc = check_plan(plan)) return rc;
  mo::KernelArgs a;
  if (int rc = fill_problem(plan, prob, batch, true, true, &a)) return rc;
  if (!vars || !r_out) return fail(MO_ERR_INVALID_ARGUMENT, "vars / r_out is NULL");
  a.mode = mo::MODE_RESIDUAL;
  a.flags = flags;
  a.vars = const_cast<void*>(vars); a.vars_stride = vars_stride;
  a.mu = mu; a.mu_stride = mu_stride;
  a.r_out = r_out; a.r_out_stride = r_stride; a.kkt_out = kkt_out;
  return launch(plan, a, stream);
}

int mo_qp_eigenvalue_stats(mo_plan* plan, const mo_problem* prob, int64_t batch, void* out, void* stream) {
  g_err[0] = 0;
  if (int rc = check_plan(plan)) return rc;
  if (!out) return fail(MO_ERR_INVALID_ARGUMENT, "out is NULL");
  mo::KernelArgs a;
  if (int rc = fill_problem(plan, prob, batch, true, false, &a, Dims{0, 0})) return rc;   // only the cost (G, or J with its damping) takes part
  if (batch == 0) return MO_OK;
  if (mo::eig_lds_bytes(plan->desc.n, false) > mo::kLdsBytes)
    return fail(MO_ERR_UNSUPPORTED, "n = %d: not even the vectors of the tridiagonal eigenvalue problem fit the 160 KiB of LDS", plan->desc.n);
  MO_HIP_CHECK(hipSetDevice(plan->desc.device));
  MO_HIP_CHECK(mo::launch_qp_eig(a, plan->desc.dtype, plan->num_cus, out, 3, plan->H_work, plan->H_work_slot_bytes, plan->H_work_slots,
                                 (hipStream_t)stream));
  return MO_OK;
}

int mo_newton_step(mo_plan* plan, const mo_problem* prob, int64_t batch, const void* vars, int64_t vars_stride,
                   const void* mu, int64_t mu_stride, double tau, uint32_t flags, void* delta, int64_t delta_stride,
                   void* alpha, int32_t* status, void* stream) {
  g_err[0] = 0;
  if (int rc = check_plan(plan)) return rc;
  mo::KernelArgs a;
  if (int rc = fill_problem(plan, prob, batch, true, true, &a)) return rc;
  if (!vars || !delta) return fail(MO_ERR_INVALID_ARGUMENT, "vars / delta is NULL");
  if (flags & ~MO_STEP_NO_INEQUALITIES) return fail(MO_ERR_INVALID_ARGUMENT, "unsupported flags 0x%x for mo_newton_step", flags);
  if (!(tau > 0) || !(tau <= 1)) return fail(MO_ERR_INVALID_ARGUMENT, "tau must be in (0, 1]");  // qp.cc:494-495
  if (plan->desc.m > 0 && !mu && !(flags & MO_STEP_NO_INEQUALITIES)) return fail(MO_ERR_INVALID_ARGUMENT, "mu is NULL");
  a.mode = mo::MODE_STEP;
  a.flags = flags;
  a.vars = const_cast<void*>(vars); a.vars_stride = vars_stride;
  a.mu = mu; a.mu_stride = mu_stride; a.tau = tau;
  a.barrier_strategy = MO_COMPLEMENTARITY;
  a.delta = delta; a.delta_stride = delta_stride; a.alpha = alpha; a.status = status;
  return launch(plan, a, stream);
}

int mo_iterate(mo_plan* plan, const mo_problem* prob, int64_t batch, void* vars, int64_t vars_stride, const void* mu,
               int64_t mu_stride, int32_t barrier_strategy, void* delta, int64_t delta_stride, void* ip_out,
               int32_t* status, void* stream) {
  g_err[0] = 0;
  if (int rc = check_plan(plan)) return rc;
  mo::KernelArgs a;
  if (int rc = fill_problem(plan, prob, batch, true, true, &a)) return rc;
  if (!vars) return fail(MO_ERR_INVALID_ARGUMENT, "vars is NULL");
  if (barrier_strategy < MO_COMPLEMENTARITY || barrier_strategy > MO_PREDICTOR_CORRECTOR)
    return fail(MO_ERR_INVALID_ARGUMENT, "bad barrier_strategy %d", barrier_strategy);
  if (plan->desc.m > 0 && !mu) return fail(MO_ERR_INVALID_ARGUMENT, "mu is NULL");
  a.mode = mo::MODE_ITERATE;
  a.vars = vars; a.vars_stride = vars_stride;
  a.mu = mu; a.mu_stride = mu_stride; a.tau = 0.995;  // qp.cc:192
  a.barrier_strategy = barrier_strategy;
  a.delta = delta; a.delta_stride = delta_stride; a.ip_out = ip_out; a.status = status;
  return launch(plan, a, stream);
}

int mo_kkt_solve(mo_plan* plan, const mo_problem* prob, int64_t batch, const void* vars, int64_t vars_stride, const void* rhs,
                 int64_t rhs_stride, uint32_t flags, void* out, int64_t out_stride, int32_t* status, void* stream) {
  g_err[0] = 0;
  // (what can be judged from the arguments alone comes first)
  if (!vars || !rhs || !out) return fail(MO_ERR_INVALID_ARGUMENT, "vars / rhs / out is NULL");
  if (flags & ~(MO_STEP_NO_INEQUALITIES | MO_KKT_TRANSPOSE)) return fail(MO_ERR_INVALID_ARGUMENT, "unsupported flags 0x%x for mo_kkt_solve", flags);
  if (rhs == out || rhs == vars) return fail(MO_ERR_INVALID_ARGUMENT, "rhs may alias neither vars nor out");
  if (int rc = check_plan(plan)) return rc;
  mo::KernelArgs a;
  if (int rc = fill_problem(plan, prob, batch, true, true, &a)) return rc;
  a.mode = mo::MODE_RHS;
  a.flags = flags;
  a.vars = const_cast<void*>(vars); a.vars_stride = vars_stride;
  a.rhs = rhs; a.rhs_stride = rhs_stride;
  a.delta = out; a.delta_stride = out_stride; a.status = status;
  // one decision per call (decide_kernel): the step kernel's right-hand-side twin on the shapes fused_rhs_supported names, else the generic kernel
  return launch(plan, a, stream);
}

int mo_qp_gradients(mo_plan* plan, const mo_problem* prob, int64_t batch, const void* vars, int64_t vars_stride, const void* u,
                    int64_t u_stride, const mo_qp_grads* out, void* stream) {
  g_err[0] = 0;
  // (what can be judged from the arguments alone comes first)
  if (!vars || !u) return fail(MO_ERR_INVALID_ARGUMENT, "vars / u is NULL");
  mo::GradArgs a;
  memset(&a, 0, sizeof(a));
  a.u = u; a.u_stride = u_stride;
  if (int rc = grad_args(plan, prob, batch, vars, vars_stride, out, false, &a)) return rc;
  const mo_plan_desc& d = plan->desc;
  if (mo::qp_grad_lds_bytes(a, plan->elem) > 64 * 1024)
    return fail(MO_ERR_UNSUPPORTED, "n = %d, k = %d, m = %d, m_r = %d: the vectors of one problem exceed the 64 KiB of LDS the gradient kernel uses", d.n, d.k, d.m, a.m_r);
  if (batch == 0) return MO_OK;
  MO_HIP_CHECK(hipSetDevice(d.device));
  MO_HIP_CHECK(mo::launch_qp_gradients(a, d.dtype, plan->num_cus, (hipStream_t)stream));
  return MO_OK;
}

}  // extern "C"

namespace {
// What mo_qp_gradients_shared and its workspace query judge alike: grad_args with the rules of a sum over the batch, then the LDS rule of
// the moment kernel.  vars / u are not looked at here.
int shared_grad_args(const mo_plan* plan, const mo_problem* prob, int64_t batch, const mo_qp_grads* out, mo::SharedGradArgs* a) {
  memset(a, 0, sizeof(*a));
  if (int rc = grad_args(plan, prob, batch, nullptr, 0, out, true, a)) return rc;
  const mo_plan_desc& d = plan->desc;
  if (mo::shared_grad_lds_bytes(*a, plan->elem) > 64 * 1024)
    return fail(MO_ERR_UNSUPPORTED, "n = %d, k = %d, m = %d, m_r = %d: four problems' vectors exceed the 64 KiB of LDS the moment kernel uses", d.n, d.k, d.m, a->m_r);
  return MO_OK;
}
}  // namespace

extern "C" {

int mo_qp_gradients_shared_workspace(const mo_plan* plan, const mo_problem* prob, int64_t batch, const mo_qp_grads* out, int64_t* bytes) {
  g_err[0] = 0;
  if (!bytes) return fail(MO_ERR_INVALID_ARGUMENT, "bytes is NULL");
  mo::SharedGradArgs a;
  if (int rc = shared_grad_args(plan, prob, batch, out, &a)) return rc;
  *bytes = (int64_t)mo::shared_grad_workspace_bytes(a, plan->elem, plan->num_cus);
  return MO_OK;
}

int mo_qp_gradients_shared(mo_plan* plan, const mo_problem* prob, int64_t batch, const void* vars, int64_t vars_stride, const void* u,
                           int64_t u_stride, const int32_t* status_fwd, const int32_t* status_adj, const mo_qp_grads* out, void* workspace,
                           int64_t workspace_bytes, void* stream) {
  g_err[0] = 0;
  mo::SharedGradArgs a;
  if (int rc = shared_grad_args(plan, prob, batch, out, &a)) return rc;
  if (int rc = reduced_call_tail(plan, batch, vars, vars_stride, u, u_stride, workspace, workspace_bytes,
                                 mo::shared_grad_workspace_bytes(a, plan->elem, plan->num_cus), "mo_qp_gradients_shared_workspace")) return rc;
  a.vars = vars; a.vars_stride = vars_stride;
  a.u = u; a.u_stride = u_stride;
  a.status_fwd = status_fwd; a.status_adj = status_adj;
  a.workspace = workspace;
  MO_HIP_CHECK(hipSetDevice(plan->desc.device));
  MO_HIP_CHECK(mo::launch_qp_gradients_shared(a, plan->desc.dtype, plan->num_cus, (hipStream_t)stream));
  return MO_OK;
}

int mo_qp_tangent_rhs(mo_plan* plan, const mo_problem* prob, int64_t batch, const void* vars, int64_t vars_stride,
                      const mo_qp_tangents* t, void* rho, int64_t rho_stride, void* stream) {
  g_err[0] = 0;
  // (what can be judged from the arguments alone comes first)
  if (!prob) return fail(MO_ERR_INVALID_ARGUMENT, "Must pass a non-null problem");
  if (!t) return fail(MO_ERR_INVALID_ARGUMENT, "t is NULL");
  if (!vars || !rho) return fail(MO_ERR_INVALID_ARGUMENT, "vars / rho is NULL");
  if (batch < 0) return fail(MO_ERR_INVALID_ARGUMENT, "batch must be >= 0");
  const bool j_level = prob->J != nullptr;
  if (j_level && t->dG) return fail(MO_ERR_INVALID_ARGUMENT, "dG given with J-level input: give dJ / dr / dlambda");
  if (!j_level && (t->dJ || t->dr || t->dlambda))
    return fail(MO_ERR_INVALID_ARGUMENT, "dJ / dr / dlambda given with (G, c) input (prob->J is NULL): give dG / dc");
  if (t->dJ && !prob->r) return fail(MO_ERR_INVALID_ARGUMENT, "dJ given without prob->r");
  if (t->dcons_a && !prob->cons_var) return fail(MO_ERR_INVALID_ARGUMENT, "dcons_a given but cons_var is NULL");
  mo::TangentArgs a;
  memset(&a, 0, sizeof(a));
  a.rho = rho; a.rho_stride = rho_stride;
  a.t = *t;
  if (int rc = sens_args(plan, prob, batch, vars, vars_stride, &a.t, &a)) return rc;
  const mo_plan_desc& d = plan->desc;
  if (a.t.dJ) {   // (in J's layout)
    const int min_ld = a.J_row_major ? d.n : d.m_r;
    if (a.t.dJ_ld < min_ld) return fail(MO_ERR_DIMENSION, "dJ_ld %d < %d", a.t.dJ_ld, min_ld);
  } else {
    a.r = nullptr;   // (w = J x + r is needed only against dJ)
  }
  if (int rc = check_dG_dA_ld(d, a.t)) return rc;
  if (d.m > 0 && prob->cons_var) { a.cons_var = prob->cons_var; a.cons_stride = prob->cons_stride; }
  if (mo::qp_tangent_lds_bytes(a, plan->elem) > 64 * 1024)
    return fail(MO_ERR_UNSUPPORTED, "n = %d, k = %d, m = %d, m_r = %d: the vectors of one problem exceed the 64 KiB of LDS the tangent kernel uses", d.n, d.k, d.m, a.m_r);
  if (batch == 0) return MO_OK;
  MO_HIP_CHECK(hipSetDevice(d.device));
  MO_HIP_CHECK(mo::launch_qp_tangent(a, d.dtype, plan->num_cus, (hipStream_t)stream));
  return MO_OK;
}

}  // extern "C"

namespace {
int qp_solve_impl(mo_plan* plan, const mo_problem* prob, int64_t batch, const mo_solve_params* params, void* vars,
                  int64_t vars_stride, int32_t* termination, int32_t* num_iterations, void* iterations, void* lagrange,
                  int32_t* status, const int* skip, long long skip_stride, long long skip_active, void* stream) {
  g_err[0] = 0;
  if (int rc = check_plan(plan)) return rc;
  if (!params) return fail(MO_ERR_INVALID_ARGUMENT, "params is NULL");
  // CheckParams, qp.cc:76-82
  if (!(params->initial_mu > 0)) return fail(MO_ERR_INVALID_ARGUMENT, "initial_mu must be > 0");
  if (!(params->sigma > 0) || !(params->sigma <= 1.0)) return fail(MO_ERR_INVALID_ARGUMENT, "sigma must be in (0, 1]");
  if (!(params->termination_kkt_tol > 0)) return fail(MO_ERR_INVALID_ARGUMENT, "termination_kkt_tol must be > 0");
  if (!(params->max_iterations > 0)) return fail(MO_ERR_INVALID_ARGUMENT, "max_iterations must be > 0");
  if (params->barrier_strategy < MO_COMPLEMENTARITY || params->barrier_strategy > MO_PREDICTOR_CORRECTOR)
    return fail(MO_ERR_INVALID_ARGUMENT, "bad barrier_strategy");
  if (params->initial_guess_method < MO_GUESS_NAIVE || params->initial_guess_method > MO_GUESS_USER_PROVIDED)
    return fail(MO_ERR_INVALID_ARGUMENT, "bad initial_guess_method");
  mo::KernelArgs a;
  if (int rc = fill_problem(plan, prob, batch, true, true, &a)) return rc;
  if (!vars) return fail(MO_ERR_INVALID_ARGUMENT, "vars is NULL");
  a.mode = mo::MODE_SOLVE;
  a.vars = vars; a.vars_stride = vars_stride;
  a.sp = *params;
  a.termination = termination; a.num_iterations = num_iterations; a.iterations = iterations; a.lagrange = lagrange;
  a.status = status;
  a.skip = skip; a.skip_stride = skip_stride; a.skip_active = skip_active;
  const mo::KernelDecision d = decide(plan, a);
  if (a.J && d.kind == mo::KERNEL_GENERIC) {  // the generic loop re-reads G after every factorisation: keep the linearised G, c in plan scratch
    if (batch > plan->desc.max_batch) return fail(MO_ERR_INVALID_ARGUMENT, "batch %lld > plan max_batch %lld", (long long)batch, (long long)plan->desc.max_batch);
    const size_t n = (size_t)plan->desc.n;
    MO_HIP_CHECK(hipSetDevice(plan->desc.device));
    if (!plan->G_scratch || !plan->c_scratch) {  // both or neither: a half-made pair would hand the kernel a NULL c_out
      void *g = nullptr, *c = nullptr;
      if (hipMalloc(&g, (size_t)plan->desc.max_batch * n * n * plan->elem) != hipSuccess ||
          hipMalloc(&c, (size_t)plan->desc.max_batch * n * plan->elem) != hipSuccess) {
        if (g) (void)hipFree(g);
        (void)hipGetLastError();
        return fail(MO_ERR_HIP, "hipMalloc of the linearisation scratch failed (max_batch %lld, n %zu)", (long long)plan->desc.max_batch, n);
      }
      if (plan->G_scratch) (void)hipFree(plan->G_scratch);
      if (plan->c_scratch) (void)hipFree(plan->c_scratch);
      plan->G_scratch = g; plan->c_scratch = c;
    }
    a.G_out = plan->G_scratch; a.G_out_stride = (long long)(n * n); a.G_out_ld = (int)n;
    a.c_out = plan->c_scratch; a.c_out_stride = (long long)n;
  }
  if (d.kind == mo::KERNEL_FUSED_F64 && plan->desc.n > 32) {   // (fp32 and the 32 grid park every tile in LDS)
    // Tile park of the fused Solve kernels: the G tiles a wave cannot keep in LDS between the passes go to a scratch indexed by the
    // wave's slot in the persistent grid (one workgroup per CU, at most twelve waves each), so its size does not depend on the batch
    // and the lines a wave re-reads every pass stay in its XCD's L2.  Optional: without it the kernel rebuilds the tiles every pass.
    // Plan-owned: mo_plan_create allocates it, with the geometry of mo_fused_select.h.
    a.G_out = plan->tile_scratch; a.G_out_stride = (long long)mo::fused_tile_park_slot_elems(plan->desc.n);
  }
  return launch(plan, a, d, stream);  // fused Solve kernel (fp64: n <= 128; fp32: n = 64 / 128), generic kernel otherwise
}
}  // namespace

extern "C" {

int mo_qp_solve(mo_plan* plan, const mo_problem* prob, int64_t batch, const mo_solve_params* params, void* vars,
                int64_t vars_stride, int32_t* termination, int32_t* num_iterations, void* iterations, void* lagrange,
                int32_t* status, void* stream) {
  return qp_solve_impl(plan, prob, batch, params, vars, vars_stride, termination, num_iterations, iterations, lagrange, status, nullptr, 0, -1,
                       stream);
}

int mo_nullspace_solve(mo_plan* plan, const mo_problem* prob, int64_t batch, void* x_out, int64_t x_stride,
                       int32_t* termination, void* stream) {
  g_err[0] = 0;
  if (int rc = check_plan(plan)) return rc;
  if (plan->desc.k <= 0) return fail(MO_ERR_DIMENSION, "Problem must have at least one equality constraint");  // F_ASSERT_GT qp.cc:680
  if (plan->desc.k > plan->desc.n) return fail(MO_ERR_DIMENSION, "k = %d equality rows for n = %d variables", plan->desc.k, plan->desc.n);
  if (!x_out || !termination) return fail(MO_ERR_INVALID_ARGUMENT, "x_out / termination is NULL");
  mo::KernelArgs a;
  if (int rc = fill_problem(plan, prob, batch, true, false, &a, Dims{-1, 0})) return rc;  // no inequalities on this path
  if (batch == 0) return MO_OK;
  a.delta = x_out; a.delta_stride = x_stride;
  a.status = termination;  // MO_STATUS_* first; translated to QPNullSpaceTerminationState below
  const size_t need = mo::nullspace_lds_bytes(plan->desc.n, plan->desc.k, a.m_r, plan->elem);
  if (need > mo::kLdsBytes) return fail(MO_ERR_UNSUPPORTED, "the null-space solver keeps G and A_eq^T in LDS: %zu B needed (> 160 KiB)", need);
  MO_HIP_CHECK(hipSetDevice(plan->desc.device));
  MO_HIP_CHECK(mo::launch_nullspace(a, plan->desc.dtype, plan->num_cus, (hipStream_t)stream));
  mo::AuxArgs t;
  memset(&t, 0, sizeof(t));
  t.batch = batch; t.status = termination;
  MO_HIP_CHECK(mo::launch_nullspace_termination(t, (hipStream_t)stream));
  return MO_OK;
}

int mo_qp_covariance(mo_plan* plan, const mo_problem* prob, int64_t batch, const int32_t* sel, int32_t q, const void* scale,
                     int64_t scale_stride, void* cov_out, int64_t cov_stride, int32_t cov_ld, void* var_out, int64_t var_stride,
                     int32_t* status, void* stream) {
  g_err[0] = 0;
  // (what can be judged from the arguments alone comes first)
  if (!cov_out && !var_out) return fail(MO_ERR_INVALID_ARGUMENT, "cov_out and var_out are both NULL");
  if (!prob) return fail(MO_ERR_INVALID_ARGUMENT, "Must pass a non-null problem");
  if (prob->J) return fail(MO_ERR_INVALID_ARGUMENT, "J given: mo_qp_covariance takes (G, A_eq) input only (linearise first)");
  if (batch < 0) return fail(MO_ERR_INVALID_ARGUMENT, "batch must be >= 0");
  if (q < 1) return fail(MO_ERR_INVALID_ARGUMENT, "q = %d: at least one variable must be selected", q);
  if (cov_out && cov_ld < q) return fail(MO_ERR_DIMENSION, "cov_ld %d < q %d", cov_ld, q);
  if (int rc = check_plan(plan)) return rc;
  const mo_plan_desc& d = plan->desc;
  if (!sel && q != d.n) return fail(MO_ERR_INVALID_ARGUMENT, "sel is NULL but q = %d is not n = %d", q, d.n);
  if (d.k > d.n) return fail(MO_ERR_DIMENSION, "k = %d equality rows for n = %d variables", d.k, d.n);
  if (!prob->G) return fail(MO_ERR_INVALID_ARGUMENT, "G is NULL");
  if (prob->G_ld < d.n) return fail(MO_ERR_DIMENSION, "G must be square: G_ld %d < n %d", prob->G_ld, d.n);
  if (d.k > 0) {
    if (!prob->A_eq) return fail(MO_ERR_DIMENSION, "k = %d but A_eq is NULL", d.k);
    if (prob->A_ld < d.k) return fail(MO_ERR_DIMENSION, "A_ld %d < k %d", prob->A_ld, d.k);
  }
  const size_t need = mo::qp_covariance_lds_bytes(d.n, d.k, q, plan->elem);
  if (need > mo::kLdsBytes)
    return fail(MO_ERR_UNSUPPORTED, "the covariance kernel keeps G and A_eq^T in LDS: n = %d, k = %d, q = %d need %zu B (> 160 KiB)", d.n, d.k, q, need);
  if (batch == 0) return MO_OK;
  mo::CovArgs a;
  memset(&a, 0, sizeof(a));
  a.n = d.n; a.k = d.k; a.q = q; a.batch = batch;
  a.G = prob->G; a.G_stride = prob->G_stride; a.G_ld = prob->G_ld;
  if (d.k > 0) { a.A = prob->A_eq; a.A_stride = prob->A_stride; a.A_ld = prob->A_ld; }
  a.sel = sel;
  a.scale = scale; a.scale_stride = scale_stride;
  a.cov = cov_out; a.cov_stride = cov_stride; a.cov_ld = cov_ld;
  a.var = var_out; a.var_stride = var_stride;
  a.status = status;
  MO_HIP_CHECK(hipSetDevice(d.device));
  MO_HIP_CHECK(mo::launch_qp_covariance(a, d.dtype, plan->num_cus, (hipStream_t)stream));
  return MO_OK;
}

void mo_default_nls_params(mo_nls_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->max_iterations = 10;  // nonlinear.hpp:64-124
  p->max_qp_iterations = 10;
  p->termination_kkt_tolerance = 1.0e-6;
  p->absolute_exit_tol = 1.0e-12;
  p->relative_exit_tol = 1.0e-5;
  p->absolute_first_derivative_tol = 1.0e-6;
  p->max_line_search_iterations = 2;
  p->line_search_strategy = MO_POLYNOMIAL_APPROXIMATION;
  p->armijo_search_tau = 0.8;
  p->equality_penalty_initial = 1.0;
  p->equality_penalty_scale_factor = 1.01;
  p->equality_penalty_rho = 0.1;
  p->lambda_initial = 0.0;
  p->lambda_failure_init = 1.0e-2;
  p->lambda_decrease_on_success = 0.1;
  p->lambda_decrease_on_restore = 0.8;
  p->max_lambda = 1.0;
  p->min_lambda = 0.0;
  p->retraction = MO_RETRACT_EUCLIDEAN;
}


static bool nls_takes_nullspace_path(const mo_plan* plan) {
  const mo_plan_desc& d = plan->desc;
  return d.m == 0 && d.k > 0 && d.k <= d.n && mo::nullspace_lds_bytes(d.n, d.k, d.m_r, plan->elem) <= mo::kLdsBytes;
}

int mo_plan_nls_uses_nullspace(const mo_plan* plan) { return plan && nls_takes_nullspace_path(plan) ? 1 : 0; }

}  // extern "C"

namespace {
mo::BlocksArgs blocks_args(const mo_residual_layout* l, long long batch) {
  mo::BlocksArgs b;
  memset(&b, 0, sizeof(b));
  b.n = l->n; b.rows = l->rows; b.values = l->values; b.batch = batch;
  b.g_ptr = l->g_ptr; b.g_ent = l->g_ent; b.c_ptr = l->c_ptr; b.c_ent = l->c_ent; b.row_info = l->row_info; b.win = l->win;
  return b;
}

int check_layout(const mo_plan* plan, const mo_residual_layout* layout) {
  if (!layout) return fail(MO_ERR_INVALID_ARGUMENT, "layout is NULL");
  if (layout->n != plan->desc.n) return fail(MO_ERR_DIMENSION, "layout built for n = %d, plan n = %d", layout->n, plan->desc.n);
  if (layout->device != plan->desc.device) return fail(MO_ERR_INVALID_ARGUMENT, "layout lives on device %d, plan on %d", layout->device, plan->desc.device);
  return MO_OK;
}

// The admission of a cost layout and an optional equality layout: what the arguments alone tell (eq_members: the call has equality members,
// `verb` "asked for" / "given"), then the plan and both layouts against it.  *eq: the equality layout the call works with -- NULL without one
// and with k = 0, where the equality members and the layout are ignored.
int check_layout_pair(const mo_plan* plan, const mo_residual_layout* cost_layout, const mo_residual_layout* eq_layout, bool eq_members,
                      const char* verb, const mo_residual_layout** eq) {
  if (!cost_layout) return fail(MO_ERR_INVALID_ARGUMENT, "cost_layout is NULL");
  if (eq_members && !eq_layout) return fail(MO_ERR_INVALID_ARGUMENT, "dJ_eq_blocks / dr_eq %s but eq_layout is NULL", verb);
  if (int rc = check_plan(plan)) return rc;
  if (int rc = check_layout(plan, cost_layout)) return rc;
  *eq = eq_layout && plan->desc.k > 0 ? eq_layout : nullptr;
  if (*eq) {
    if (int rc = check_layout(plan, *eq)) return rc;
    if ((*eq)->rows != plan->desc.k) return fail(MO_ERR_DIMENSION, "eq_layout has %d rows, plan k = %d", (*eq)->rows, plan->desc.k);
  }
  return MO_OK;
}

mo::BlockGradArgs block_grad_args(const mo_plan* plan, const mo_residual_layout* l, int64_t batch, const void* vars, int64_t vars_stride,
                                  const void* u, int64_t u_stride) {
  mo::BlockGradArgs a;
  memset(&a, 0, sizeof(a));
  a.n = plan->desc.n; a.k = plan->desc.k; a.m = plan->desc.m; a.rows = l->rows; a.values = l->values; a.batch = batch;
  a.d_row = l->d_row; a.d_idx = l->d_idx; a.d_val = l->d_val; a.d_dup = l->d_dup; a.e_val = l->e_val;
  a.vars = vars; a.vars_stride = vars_stride; a.u = u; a.u_stride = u_stride;
  return a;
}

// The SQP loop of mo_nls_solve and mo_nls_solve_blocks.  Without block input (dense stacks) it launches exactly the kernels of
// mo_nls_solve; with block input every outer iteration first forms G, c and A_eq from the packed blocks into per-call scratch and the QP,
// the eigenvalue statistics and the directional derivatives read that (G, c) input.  cost_loss (block input only; NULL = none): the cost is
// 0.5 sum rho -- the linearise is the robust one and the f of both error pairs is the loss's, written over nonlinear_errors_kernel's.
int check_loss(const mo_residual_layout* layout, const mo_residual_loss* loss) {
  if (loss->device != layout->device) return fail(MO_ERR_INVALID_ARGUMENT, "loss table lives on device %d, layout on %d", loss->device, layout->device);
  if (loss->num_blocks != layout->num_blocks || loss->rows != layout->rows)
    return fail(MO_ERR_DIMENSION, "loss table built for %d blocks / %d rows, layout has %d / %d", loss->num_blocks, loss->rows,
                layout->num_blocks, layout->rows);
  return MO_OK;
}

mo::LossArgs loss_args(const mo_residual_loss* loss, int dtype, long long batch) {
  mo::LossArgs a;
  memset(&a, 0, sizeof(a));
  a.num_blocks = loss->num_blocks; a.rows = loss->rows; a.batch = batch;
  a.blk = loss->blk; a.scale = dtype == MO_F64 ? (const void*)loss->scale_d : (const void*)loss->scale_f;
  a.rho_stride = 1;
  return a;
}

void blocks_args_loss(mo::BlocksArgs* a, const mo_residual_loss* loss, int dtype) {
  a->loss_blk = loss->blk; a->loss_blocks = loss->num_blocks;
  a->loss_scale = dtype == MO_F64 ? (const void*)loss->scale_d : (const void*)loss->scale_f;
  a->half_sq_stride = 1;
}

int nls_solve_impl(mo_plan* plan, const mo_nls_problem* np, bool blocks, const mo_residual_layout* cost_layout,
                   const mo_residual_loss* cost_loss, const mo_residual_layout* eq_layout, int64_t batch, const mo_nls_params* prm, mo_nls_eval_fn eval, void* user, int32_t* termination, int32_t* num_iterations,
                   void* iterations, int32_t* status, void* stream) {
  g_err[0] = 0;
  if (int rc = check_plan(plan)) return rc;
  const mo_plan_desc& d = plan->desc;
  if (d.dtype != MO_F64) return fail(MO_ERR_UNSUPPORTED, "mo_nls_solve needs an fp64 plan");
  if (!np || !prm || !eval) return fail(MO_ERR_INVALID_ARGUMENT, "problem / params / eval is NULL");
  if (batch < 0) return fail(MO_ERR_INVALID_ARGUMENT, "batch must be >= 0");
  if (d.m_r <= 0) return fail(MO_ERR_DIMENSION, "the plan must be created with m_r > 0 (the cost residual stack)");
  // CheckParams, nonlinear.cc:48-73
  if (prm->max_iterations < 0) return fail(MO_ERR_INVALID_ARGUMENT, "max_iterations must be >= 0");
  if (prm->max_qp_iterations < 1) return fail(MO_ERR_INVALID_ARGUMENT, "max_qp_iterations must be >= 1");
  if (!(prm->termination_kkt_tolerance > 0)) return fail(MO_ERR_INVALID_ARGUMENT, "termination_kkt_tolerance must be > 0");
  if (!(prm->absolute_exit_tol > 0)) return fail(MO_ERR_INVALID_ARGUMENT, "absolute_exit_tol must be > 0");
  if (prm->max_line_search_iterations < 0) return fail(MO_ERR_INVALID_ARGUMENT, "max_line_search_iterations must be >= 0");
  if (!(prm->relative_exit_tol >= 0) || !(prm->relative_exit_tol <= 1)) return fail(MO_ERR_INVALID_ARGUMENT, "relative_exit_tol must be in [0, 1]");
  if (!(prm->absolute_first_derivative_tol >= 0)) return fail(MO_ERR_INVALID_ARGUMENT, "absolute_first_derivative_tol must be >= 0");
  if (!(prm->armijo_search_tau > 0) || !(prm->armijo_search_tau < 1)) return fail(MO_ERR_INVALID_ARGUMENT, "armijo_search_tau must be in (0, 1)");
  if (!(prm->equality_penalty_initial >= 0)) return fail(MO_ERR_INVALID_ARGUMENT, "equality_penalty_initial must be >= 0");
  if (!(prm->equality_penalty_scale_factor >= 1.0)) return fail(MO_ERR_INVALID_ARGUMENT, "equality_penalty_scale_factor must be >= 1");
  if (!(prm->equality_penalty_rho >= 0) || !(prm->equality_penalty_rho < 1)) return fail(MO_ERR_INVALID_ARGUMENT, "equality_penalty_rho must be in [0, 1)");
  if (!(prm->max_lambda >= 0) || !(prm->min_lambda <= prm->max_lambda)) return fail(MO_ERR_INVALID_ARGUMENT, "need 0 <= min_lambda <= max_lambda");
  if (!(prm->lambda_initial >= prm->min_lambda) || !(prm->lambda_initial <= prm->max_lambda)) return fail(MO_ERR_INVALID_ARGUMENT, "lambda_initial outside [min_lambda, max_lambda]");
  if (!(prm->lambda_failure_init >= 0)) return fail(MO_ERR_INVALID_ARGUMENT, "lambda_failure_init must be >= 0");
  if (!(prm->lambda_decrease_on_success >= 0) || !(prm->lambda_decrease_on_success < 1.0)) return fail(MO_ERR_INVALID_ARGUMENT, "lambda_decrease_on_success must be in [0, 1)");
  if (!(prm->lambda_decrease_on_restore >= 0) || !(prm->lambda_decrease_on_restore < 1.0)) return fail(MO_ERR_INVALID_ARGUMENT, "lambda_decrease_on_restore must be in [0, 1)");
  if (prm->line_search_strategy != MO_ARMIJO_BACKTRACK && prm->line_search_strategy != MO_POLYNOMIAL_APPROXIMATION)
    return fail(MO_ERR_INVALID_ARGUMENT, "bad line_search_strategy");
  if (prm->retraction < MO_RETRACT_EUCLIDEAN || prm->retraction > MO_RETRACT_CALLBACK) return fail(MO_ERR_INVALID_ARGUMENT, "bad retraction");
  if (prm->retraction == MO_RETRACT_CALLBACK && (!np->step || !np->step_alpha))
    return fail(MO_ERR_INVALID_ARGUMENT, "MO_RETRACT_CALLBACK needs the step / step_alpha buffers");
  if (!np->vars || !np->candidate || !np->J || !np->r || !np->r_cand) return fail(MO_ERR_INVALID_ARGUMENT, "vars / candidate / J / r / r_cand is NULL");
  if (d.k > 0 && (!np->J_eq || !np->r_eq || !np->r_eq_cand)) return fail(MO_ERR_DIMENSION, "k = %d but J_eq / r_eq / r_eq_cand is NULL", d.k);
  if (d.m > 0 && (!np->cons_var || !np->cons_a || !np->cons_b)) return fail(MO_ERR_INVALID_ARGUMENT, "m = %d but constraint arrays are NULL", d.m);
  if (prm->log_qp_eigenvalues && !np->qp_eigenvalues) return fail(MO_ERR_INVALID_ARGUMENT, "log_qp_eigenvalues needs the qp_eigenvalues buffer");
  if (!termination) return fail(MO_ERR_INVALID_ARGUMENT, "termination is NULL");
  if (blocks) {
    if (!cost_layout) return fail(MO_ERR_INVALID_ARGUMENT, "cost_layout is NULL");
    if (int rc = check_layout(plan, cost_layout)) return rc;
    if (cost_layout->rows != d.m_r) return fail(MO_ERR_DIMENSION, "cost layout has %d rows, plan m_r = %d", cost_layout->rows, d.m_r);
    if ((eq_layout != nullptr) != (d.k > 0)) return fail(MO_ERR_DIMENSION, "eq_layout must be given iff k > 0 (k = %d)", d.k);
    if (eq_layout) {
      if (int rc = check_layout(plan, eq_layout)) return rc;
      if (eq_layout->rows != d.k) return fail(MO_ERR_DIMENSION, "equality layout has %d rows, plan k = %d", eq_layout->rows, d.k);
    }
    if (cost_loss)
      if (int rc = check_loss(cost_layout, cost_loss)) return rc;
  }
  const bool loss_staged = cost_loss && mo::blocks_weighted_stages(cost_layout->values, cost_layout->rows, 8);
  if (batch == 0) return MO_OK;
  MO_HIP_CHECK(hipSetDevice(d.device));
  hipStream_t s = (hipStream_t)stream;
  const int n = d.n, k = d.k, m = d.m;
  const long long V = n + 2 * m + k, Vs = (V + 1) & ~1ll;  // even stride: the fused kernels want 16-byte aligned states

  NlsScratch scratch;
  double *qp_vars, *cons_b, *cons_a, *errors_pre, *errors_step, *deriv, *quad, *lagrange, *sd;
  int *qp_status, *qp_term, *qp_nit, *si, *counters, *cons_var;
  scratch.reserve<double>((size_t)batch * Vs);
  for (int i = 0; i < 2; ++i) scratch.reserve<double>((size_t)batch * m);
  scratch.reserve<int>((size_t)batch * m);
  for (int i = 0; i < 3; ++i) scratch.reserve<double>((size_t)batch * 2);
  scratch.reserve<double>((size_t)batch);
  scratch.reserve<double>((size_t)batch * 2);
  scratch.reserve<double>((size_t)batch * mo::NLS_SD);
  for (int i = 0; i < 3; ++i) scratch.reserve<int>((size_t)batch);
  scratch.reserve<int>((size_t)batch * mo::NLS_SI);
  scratch.reserve<int>(2);
  double *G_blk = nullptr, *c_blk = nullptr, *A_blk = nullptr;
  if (blocks) {  // the QP of every outer iteration as (G, c, A_eq)
    scratch.reserve<double>((size_t)batch * n * n);
    scratch.reserve<double>((size_t)batch * n);
    scratch.reserve<double>((size_t)batch * k * n);
    if (cost_loss && !loss_staged) scratch.reserve<double>((size_t)batch * d.m_r);
  }
  double* w_blk = nullptr;  // the weights of a robust cost whose layout does not stage: the two-launch route
  MO_HIP_CHECK(scratch.commit());
  MO_HIP_CHECK(scratch.alloc(&qp_vars, (size_t)batch * Vs));
  MO_HIP_CHECK(scratch.alloc(&cons_b, (size_t)batch * m));  // the QP's constraints: one stride for (variable, a, shifted b)
  MO_HIP_CHECK(scratch.alloc(&cons_a, (size_t)batch * m));
  MO_HIP_CHECK(scratch.alloc(&cons_var, (size_t)batch * m));
  MO_HIP_CHECK(scratch.alloc(&errors_pre, (size_t)batch * 2));
  MO_HIP_CHECK(scratch.alloc(&errors_step, (size_t)batch * 2));
  MO_HIP_CHECK(scratch.alloc(&deriv, (size_t)batch * 2));
  MO_HIP_CHECK(scratch.alloc(&quad, (size_t)batch));
  MO_HIP_CHECK(scratch.alloc(&lagrange, (size_t)batch * 2));
  MO_HIP_CHECK(scratch.alloc(&sd, (size_t)batch * mo::NLS_SD));
  MO_HIP_CHECK(scratch.alloc(&qp_status, (size_t)batch));
  MO_HIP_CHECK(scratch.alloc(&qp_term, (size_t)batch));
  MO_HIP_CHECK(scratch.alloc(&qp_nit, (size_t)batch));
  MO_HIP_CHECK(scratch.alloc(&si, (size_t)batch * mo::NLS_SI));
  MO_HIP_CHECK(scratch.alloc(&counters, 2));
  if (blocks) {
    MO_HIP_CHECK(scratch.alloc(&G_blk, (size_t)batch * n * n));
    MO_HIP_CHECK(scratch.alloc(&c_blk, (size_t)batch * n));
    MO_HIP_CHECK(scratch.alloc(&A_blk, (size_t)batch * k * n));
    if (cost_loss && !loss_staged) MO_HIP_CHECK(scratch.alloc(&w_blk, (size_t)batch * d.m_r));
  }

  mo::NlsArgs na;
  memset(&na, 0, sizeof(na));
  na.n = n; na.k = k; na.m = m; na.batch = batch; na.prm = *prm;
  na.vars = (double*)np->vars; na.vars_stride = np->vars_stride;
  na.cand = (double*)np->candidate; na.cand_stride = np->candidate_stride;
  na.qp_vars = qp_vars; na.qp_vars_stride = Vs;
  na.errors_pre = errors_pre; na.errors_step = errors_step; na.deriv = deriv; na.quad = quad; na.lagrange = lagrange;
  na.qp_status = qp_status; na.qp_term = qp_term; na.qp_nit = qp_nit;
  na.sd = sd; na.si = si;
  na.iterations = (double*)iterations; na.rec = MO_NLS_ITER_RECORD(prm->max_line_search_iterations);
  na.termination = termination; na.num_iterations = num_iterations; na.status = status;
  na.counters = counters;
  na.step = (double*)np->step; na.step_stride = np->step_stride; na.step_alpha = (double*)np->step_alpha;
  na.user_exit = np->user_exit;
  const bool retract_cb = prm->retraction == MO_RETRACT_CALLBACK;
  if (retract_cb) MO_HIP_CHECK(hipMemsetAsync(np->step_alpha, 0, sizeof(double) * (size_t)batch, s));
  if (np->user_exit) MO_HIP_CHECK(hipMemsetAsync(np->user_exit, 0, sizeof(int32_t) * (size_t)batch, s));
  MO_HIP_CHECK(mo::launch_nls_init(na, s));
  if (prm->max_iterations == 0) {  // nonlinear.cc:97, 157: no iteration at all
    MO_HIP_CHECK(hipMemsetAsync(termination, 0, sizeof(int32_t) * (size_t)batch, s));
    if (num_iterations) MO_HIP_CHECK(hipMemsetAsync(num_iterations, 0, sizeof(int32_t) * (size_t)batch, s));
    return MO_OK;
  }

  // the QP of this outer iteration (LinearizeAndFillQP's output, nonlinear.cc:98) in J-level form
  mo_problem qp;
  memset(&qp, 0, sizeof(qp));
  qp.J = np->J; qp.J_stride = np->J_stride; qp.J_ld = np->J_ld; qp.J_layout = np->J_layout;
  qp.r = np->r; qp.r_stride = np->r_stride;
  qp.lambda_vec = sd + mo::NLS_SD_LAMBDA; qp.lambda_stride = mo::NLS_SD;
  qp.A_eq = np->J_eq; qp.A_stride = np->J_eq_stride; qp.A_ld = np->J_eq_ld;
  qp.b_eq = np->r_eq; qp.b_stride = np->r_eq_stride;
  qp.cons_var = cons_var; qp.cons_a = cons_a; qp.cons_b = cons_b; qp.cons_stride = m;
  mo::BlocksArgs cost_ba, eq_ba;
  if (blocks) {  // QP-level input: lambda is already on G's diagonal
    qp.J = nullptr; qp.r = nullptr; qp.lambda_vec = nullptr;
    qp.G = G_blk; qp.G_stride = (int64_t)n * n; qp.G_ld = n;
    qp.c = c_blk; qp.c_stride = n;
    if (k > 0) { qp.A_eq = A_blk; qp.A_stride = (int64_t)k * n; qp.A_ld = k; }
    cost_ba = blocks_args(cost_layout, batch);
    cost_ba.J = np->J; cost_ba.J_stride = np->J_stride; cost_ba.r = np->r; cost_ba.r_stride = np->r_stride;
    cost_ba.lambda_vec = sd + mo::NLS_SD_LAMBDA; cost_ba.lambda_vec_stride = mo::NLS_SD;
    cost_ba.G_out = G_blk; cost_ba.G_out_stride = (long long)n * n; cost_ba.G_out_ld = n;
    cost_ba.c_out = c_blk; cost_ba.c_out_stride = n;
    if (cost_loss) {
      if (loss_staged) {
        blocks_args_loss(&cost_ba, cost_loss, d.dtype);
        cost_ba.half_sq_out = errors_pre; cost_ba.half_sq_stride = 2;
      } else {
        cost_ba.weights = w_blk; cost_ba.weights_stride = d.m_r;
      }
    }
    if (k > 0) {
      eq_ba = blocks_args(eq_layout, batch);
      eq_ba.J = np->J_eq; eq_ba.J_stride = np->J_eq_stride; eq_ba.r = np->r_eq; eq_ba.r_stride = np->r_eq_stride;
      eq_ba.J_out = A_blk; eq_ba.J_out_stride = (long long)k * n; eq_ba.J_out_ld = k; eq_ba.J_out_row_major = 0;
    }
  }
  mo_solve_params sp;
  mo_default_solve_params(&sp);       // ComputeStepDirection, nonlinear.cc:226-241
  sp.max_iterations = prm->max_qp_iterations;
  sp.termination_kkt_tol = prm->termination_kkt_tolerance;
  sp.initial_mu = 1.0;
  sp.sigma = 0.1;
  sp.initialize_mu_with_complementarity = 0;
  sp.initial_guess_method = k > 0 ? MO_GUESS_SOLVE_EQUALITY_CONSTRAINED : MO_GUESS_NAIVE;

  mo::AuxArgs ea;  // errors at the linearisation point / at the candidate
  memset(&ea, 0, sizeof(ea));
  ea.n = n; ea.k = k; ea.m = m; ea.m_r = d.m_r; ea.batch = batch;
  mo::AuxArgs sa = ea;  // ShiftTo
  sa.x = np->vars; sa.x_stride = np->vars_stride;
  sa.cons_var = np->cons_var; sa.cons_a = np->cons_a; sa.cons_b = np->cons_b; sa.cons_stride = np->cons_stride;
  sa.cons_b_out = cons_b; sa.cons_b_out_stride = m; sa.cons_var_out = cons_var; sa.cons_a_out = cons_a;
  mo::AuxArgs da = ea;  // ComputeQPCostDerivative
  da.x = qp_vars; da.x_stride = Vs;
  da.J = np->J; da.J_stride = np->J_stride; da.J_ld = np->J_ld; da.J_row_major = np->J_layout == MO_ROW_MAJOR;
  da.r = np->r; da.r_stride = np->r_stride;
  da.A = np->J_eq; da.A_stride = np->J_eq_stride; da.A_ld = np->J_eq_ld; da.b = np->r_eq; da.b_stride = np->r_eq_stride;
  da.lambda_vec = sd + mo::NLS_SD_LAMBDA; da.lambda_vec_stride = mo::NLS_SD;
  da.out2 = deriv; da.quad_out = quad;
  if (blocks) {  // c^T dx and dx^T G dx from the assembled (G, c)
    da.J = nullptr; da.r = nullptr; da.lambda_vec = nullptr;
    da.G = G_blk; da.G_stride = (long long)n * n; da.G_ld = n;
    da.c = c_blk; da.c_stride = n;
    da.A = A_blk; da.A_stride = (long long)k * n; da.A_ld = k;
  }

  mo::LossArgs la{};  // 0.5 sum rho over nonlinear_errors_kernel's f
  if (cost_loss) {
    la = loss_args(cost_loss, d.dtype, batch);
    la.rho_stride = 2;
  }

  int host_counters[2];
  long long still_active = batch;  // problems the previous outer iteration left active (a hint for the QP kernel's ticket size)
  for (int iter = 0; iter < prm->max_iterations; ++iter) {
    na.iter = iter;
    if (eval(user, MO_NLS_EVAL_LINEARIZE, stream) != 0) return fail(MO_ERR_CALLBACK, "eval(LINEARIZE) failed at iteration %d", iter);
    if (blocks && !cost_loss) {  // LinearizeAndFillQP (nonlinear.cc:182-206) from the packed blocks
      MO_HIP_CHECK(mo::launch_blocks_linearize(cost_ba, d.dtype, plan->num_cus, s));
      if (k > 0) MO_HIP_CHECK(mo::launch_blocks_jacobian(eq_ba, d.dtype, plan->num_cus, s));
    }
    // errors_pre (nonlinear.cc:184-186, 203) and the shifted constraints (:209-212)
    ea.r = np->r; ea.r_stride = np->r_stride; ea.b = np->r_eq; ea.b_stride = np->r_eq_stride; ea.out2 = errors_pre;
    MO_HIP_CHECK(mo::launch_nonlinear_errors(ea, d.dtype, s));
    if (cost_loss) {  // the robust linearise, after the errors: its 0.5 sum rho replaces their f
      if (!loss_staged) {
        la.r = np->r; la.r_stride = np->r_stride; la.weights_out = w_blk; la.weights_stride = d.m_r; la.rho_out = errors_pre;
        MO_HIP_CHECK(mo::launch_residual_loss(la, d.dtype, plan->num_cus, s));
      }
      MO_HIP_CHECK(mo::launch_blocks_linearize(cost_ba, d.dtype, plan->num_cus, s));
      if (k > 0) MO_HIP_CHECK(mo::launch_blocks_jacobian(eq_ba, d.dtype, plan->num_cus, s));
    }
    if (m > 0) MO_HIP_CHECK(mo::launch_shift_constraints(sa, d.dtype, s));
    // ComputeStepDirection (nonlinear.cc:216-247): the interior-point QP on device
    if (nls_takes_nullspace_path(plan)) {
      // equality constraints only: QPNullSpaceSolver (nonlinear.cc:83-86, 249-258) -- singular G = J^T J is fine as long as
      // the reduced Hessian is positive definite; NOT_POSITIVE_DEFINITE ends the problem with QP_INDEFINITE (:103-105)
      mo::KernelArgs ka;
      if (int rc = fill_problem(plan, &qp, batch, true, false, &ka)) return rc;
      ka.delta = qp_vars; ka.delta_stride = Vs; ka.status = qp_status;
      MO_HIP_CHECK(hipMemsetAsync(qp_term, 0, sizeof(int) * (size_t)batch, s));
      MO_HIP_CHECK(hipMemsetAsync(qp_nit, 0, sizeof(int) * (size_t)batch, s));
      MO_HIP_CHECK(mo::launch_nullspace(ka, d.dtype, plan->num_cus, s));
    } else {
      void* qp_records = np->qp_iterations ? (void*)((double*)np->qp_iterations + (size_t)iter * (size_t)batch * sp.max_iterations * MO_ITER_RECORD) : nullptr;
      if (int rc = qp_solve_impl(plan, &qp, batch, &sp, qp_vars, Vs, qp_term, qp_nit, qp_records, lagrange, qp_status,
                                 si + mo::NLS_SI_TERM, mo::NLS_SI, still_active, stream)) return rc;  // terminated problems are skipped
      if (np->qp_lagrange && k > 0)
        MO_HIP_CHECK(hipMemcpyAsync((double*)np->qp_lagrange + (size_t)iter * (size_t)batch * 2, lagrange, sizeof(double) * 2 * (size_t)batch,
                                    hipMemcpyDeviceToDevice, s));
    }
    if (prm->log_qp_eigenvalues) {   // qp_.ComputeEigenvalueStats() of this iteration's QP (nonlinear.cc:138), still-active problems only
      mo::KernelArgs ka;
      if (int rc = fill_problem(plan, &qp, batch, true, false, &ka, Dims{0, 0})) return rc;
      ka.skip = si + mo::NLS_SI_TERM; ka.skip_stride = mo::NLS_SI;
      MO_HIP_CHECK(mo::launch_qp_eig(ka, d.dtype, plan->num_cus, (double*)np->qp_eigenvalues + (size_t)iter * (size_t)batch * 3, 3, plan->H_work,
                                     plan->H_work_slot_bytes, plan->H_work_slots, s));
    }
    MO_HIP_CHECK(mo::launch_cost_derivative(da, d.dtype, s));
    MO_HIP_CHECK(hipMemsetAsync(counters, 0, 2 * sizeof(int), s));
    MO_HIP_CHECK(mo::launch_nls_begin_search(na, s));
    if (retract_cb && eval(user, MO_NLS_EVAL_RETRACT, stream) != 0) return fail(MO_ERR_CALLBACK, "eval(RETRACT) failed at iteration %d", iter);
    // SelectStepSize (nonlinear.cc:346-412)
    for (int ls = 0; ls <= prm->max_line_search_iterations; ++ls) {
      MO_HIP_CHECK(hipMemcpyAsync(host_counters, counters, sizeof(int), hipMemcpyDeviceToHost, s));
      MO_HIP_CHECK(hipStreamSynchronize(s));
      if (host_counters[0] == 0) break;  // nobody is searching any more
      na.ls = ls;
      if (eval(user, MO_NLS_EVAL_ERRORS, stream) != 0) return fail(MO_ERR_CALLBACK, "eval(ERRORS) failed at iteration %d", iter);
      ea.r = np->r_cand; ea.r_stride = np->r_cand_stride; ea.b = np->r_eq_cand; ea.b_stride = np->r_eq_cand_stride; ea.out2 = errors_step;
      MO_HIP_CHECK(mo::launch_nonlinear_errors(ea, d.dtype, s));
      if (cost_loss) {
        la.r = np->r_cand; la.r_stride = np->r_cand_stride; la.weights_out = nullptr; la.rho_out = errors_step;
        MO_HIP_CHECK(mo::launch_residual_loss(la, d.dtype, plan->num_cus, s));
      }
      MO_HIP_CHECK(hipMemsetAsync(counters, 0, sizeof(int), s));
      MO_HIP_CHECK(mo::launch_nls_search_step(na, s));
      if (retract_cb && eval(user, MO_NLS_EVAL_RETRACT, stream) != 0) return fail(MO_ERR_CALLBACK, "eval(RETRACT) failed at iteration %d", iter);
    }
    MO_HIP_CHECK(mo::launch_nls_update(na, s));
    if (np->user_exit) {  // SetUserExitCallback, nonlinear.cc:142-149
      if (eval(user, MO_NLS_EVAL_ITERATION_DONE, stream) != 0) return fail(MO_ERR_CALLBACK, "eval(ITERATION_DONE) failed at iteration %d", iter);
      MO_HIP_CHECK(mo::launch_nls_user_exit(na, s));
    }
    MO_HIP_CHECK(hipMemcpyAsync(host_counters, counters, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    MO_HIP_CHECK(hipStreamSynchronize(s));
    if (host_counters[1] == 0) break;  // every problem has terminated
    still_active = host_counters[1];
  }
  MO_HIP_CHECK(hipStreamSynchronize(s));  // the scratch is released on return
  return MO_OK;
}
}  // namespace

extern "C" {

int mo_nls_solve(mo_plan* plan, const mo_nls_problem* np, int64_t batch, const mo_nls_params* prm, mo_nls_eval_fn eval,
                 void* user, int32_t* termination, int32_t* num_iterations, void* iterations, int32_t* status, void* stream) {
  return nls_solve_impl(plan, np, false, nullptr, nullptr, nullptr, batch, prm, eval, user, termination, num_iterations, iterations, status, stream);
}

int mo_nls_solve_blocks(mo_plan* plan, const mo_nls_problem* np, const mo_residual_layout* cost_layout,
                        const mo_residual_layout* eq_layout, int64_t batch, const mo_nls_params* params, mo_nls_eval_fn eval, void* user,
                        int32_t* termination, int32_t* num_iterations, void* iterations, int32_t* status, void* stream) {
  return nls_solve_impl(plan, np, true, cost_layout, nullptr, eq_layout, batch, params, eval, user, termination, num_iterations, iterations,
                        status, stream);
}

int mo_nls_solve_blocks_robust(mo_plan* plan, const mo_nls_problem* np, const mo_residual_layout* cost_layout,
                               const mo_residual_loss* cost_loss, const mo_residual_layout* eq_layout, int64_t batch,
                               const mo_nls_params* params, mo_nls_eval_fn eval, void* user, int32_t* termination, int32_t* num_iterations,
                               void* iterations, int32_t* status, void* stream) {
  return nls_solve_impl(plan, np, true, cost_layout, cost_loss && !cost_loss->all_trivial ? cost_loss : nullptr, eq_layout, batch, params, eval,
                        user, termination, num_iterations, iterations, status, stream);
}

int mo_residual_layout_create(const mo_plan* plan, int32_t num_blocks, const int32_t* rows, const int32_t* params,
                              const int32_t* index, mo_residual_layout** out) {
  g_err[0] = 0;
  if (!out) return fail(MO_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  if (int rc = check_plan(plan)) return rc;
  if (!rows || !params || !index) return fail(MO_ERR_INVALID_ARGUMENT, "rows / params / index is NULL");
  if (num_blocks <= 0) return fail(MO_ERR_INVALID_ARGUMENT, "num_blocks must be >= 1 (got %d)", num_blocks);
  const int n = plan->desc.n;
  long long values = 0, total_rows = 0, total_idx = 0, pairs = 0;
  for (int b = 0; b < num_blocks; ++b) {
    if (rows[b] <= 0 || params[b] <= 0) return fail(MO_ERR_INVALID_ARGUMENT, "block %d: R = %d, P = %d (both must be >= 1)", b, rows[b], params[b]);
    values += (long long)rows[b] * params[b];
    total_rows += rows[b];
    total_idx += params[b];
    pairs += (long long)params[b] * (params[b] + 1) / 2;
  }
  const long long lim = 0x7fffffffll;
  if (values + total_rows > lim || total_rows * n > lim || pairs > lim || (long long)num_blocks * n > lim)
    return fail(MO_ERR_UNSUPPORTED, "layout too large for 32-bit offsets (%lld values, %lld rows)", values, total_rows);
  for (long long i = 0; i < total_idx; ++i)
    if (index[i] < 0 || index[i] >= n) return fail(MO_ERR_DIMENSION, "index[%lld] = %d outside [0, %d)", i, index[i], n);

  // contributions in the reference's order: blocks in order, then row_local, col_local <= row_local (residual.hpp:206-222)
  const size_t nn = (size_t)n * n;
  std::vector<int> g_ptr(nn + 1, 0), c_ptr((size_t)n + 1, 0);
  auto cell_of = [n](int rg, int cg) { return cg <= rg ? (size_t)cg * n + rg : (size_t)rg * n + cg; };  // lower triangle, column-major
  {
    long long ib = 0;
    for (int b = 0; b < num_blocks; ++b) {
      const int32_t* idx = index + ib;
      for (int a = 0; a < params[b]; ++a) {
        for (int c = 0; c <= a; ++c) ++g_ptr[cell_of(idx[a], idx[c]) + 1];
        ++c_ptr[(size_t)idx[a] + 1];
      }
      ib += params[b];
    }
  }
  for (size_t i = 0; i < nn; ++i) g_ptr[i + 1] += g_ptr[i];
  for (int i = 0; i < n; ++i) c_ptr[i + 1] += c_ptr[i];
  std::vector<int4> g_ent((size_t)g_ptr[nn]), c_ent((size_t)c_ptr[n]);
  std::vector<int> g_cur(g_ptr.begin(), g_ptr.end() - 1), c_cur(c_ptr.begin(), c_ptr.end() - 1);
  std::vector<int2> row_info((size_t)total_rows);
  std::vector<int> win((size_t)num_blocks * n, -1);
  {
    long long ib = 0, off = 0, roff = 0;
    for (int b = 0; b < num_blocks; ++b) {
      const int R = rows[b], P = params[b];
      const int32_t* idx = index + ib;
      for (int a = 0; a < P; ++a) {
        for (int c = 0; c <= a; ++c) g_ent[g_cur[cell_of(idx[a], idx[c])]++] = make_int4((int)(off + (long long)a * R), (int)(off + (long long)c * R), R, (int)roff);
        c_ent[c_cur[idx[a]]++] = make_int4((int)(off + (long long)a * R), (int)roff, R, 0);
        win[(size_t)b * n + idx[a]] = (int)(off + (long long)a * R);  // UpdateJacobian assigns: the last local column wins
      }
      for (int q = 0; q < R; ++q) row_info[(size_t)(roff + q)] = make_int2(b * n, q);
      ib += P; off += (long long)R * P; roff += R;
    }
  }
  // the backward schedule: per stacked row where its block lives, per packed value its row, its variable and the other local columns on
  // that variable (almost always none), and for equality blocks whether the value's column is the one that won its global column
  std::vector<int4> d_row((size_t)total_rows), d_val((size_t)values);
  std::vector<int2> e_val((size_t)values);
  std::vector<int> d_idx(index, index + total_idx), d_dup, d_pair((size_t)total_rows, -1), d_plist;
  {
    long long ib = 0, off = 0, roff = 0;
    for (int b = 0; b < num_blocks; ++b) {
      const int R = rows[b], P = params[b];
      const int32_t* idx = index + ib;
      for (int q = 0; q < R; ++q) d_row[(size_t)(roff + q)] = make_int4((int)(off + q), R, P, (int)ib);
      for (int a = 0; a < P; ++a) {
        int partners = 0;
        for (int c = 0; c < P; ++c) partners += c != a && idx[c] == idx[a];
        int dup = -1;
        if (partners) {
          dup = (int)d_dup.size();
          d_dup.push_back(partners);
          for (int c = 0; c < P; ++c)
            if (c != a && idx[c] == idx[a]) d_dup.push_back((int)(off + (long long)c * R));
        }
        const bool wins = win[(size_t)b * n + idx[a]] == (int)(off + (long long)a * R);
        for (int q = 0; q < R; ++q) {
          d_val[(size_t)(off + (long long)a * R + q)] = make_int4((int)(roff + q), idx[a], q, dup);
          e_val[(size_t)(off + (long long)a * R + q)] = make_int2((int)(roff + q), wins ? idx[a] : -1);
        }
      }
      // the pairs p' < p of local columns on one variable, as offsets from the row's first value: {count, count x {p R, p' R, variable}}
      int pairs_b = 0;
      for (int a = 0; a < P; ++a)
        for (int c = 0; c < a; ++c) pairs_b += idx[c] == idx[a];
      if (pairs_b) {
        const int start = (int)d_plist.size();
        d_plist.push_back(pairs_b);
        for (int a = 0; a < P; ++a)
          for (int c = 0; c < a; ++c)
            if (idx[c] == idx[a]) { d_plist.push_back(a * R); d_plist.push_back(c * R); d_plist.push_back(idx[a]); }
        for (int q = 0; q < R; ++q) d_pair[(size_t)(roff + q)] = start;
      }
      ib += P; off += (long long)R * P; roff += R;
    }
  }
  // the forward-mode schedule: every entry of a variable's list carries its column's partner list (mo_qp_tangent_rhs_blocks walks the list
  // and needs no second look-up), and per variable, in the layout's order, the local columns that WIN it (the columns mo_jacobian_blocks copies)
  for (size_t e = 0; e < c_ent.size(); ++e) c_ent[e].w = d_val[(size_t)c_ent[e].x].w;
  std::vector<int> w_ptr((size_t)n + 1, 0);
  std::vector<int4> w_ent;
  {
    for (int i = 0; i < n; ++i) {
      for (int e = c_ptr[i]; e < c_ptr[i + 1]; ++e)
        if (e_val[(size_t)c_ent[e].x].y >= 0) w_ent.push_back(c_ent[e]);
      w_ptr[(size_t)i + 1] = (int)w_ent.size();
    }
  }
  // one device allocation: [g_ent | c_ent | g_ptr | c_ptr | row_info | win | d_row | d_val | e_val | d_idx | d_dup | w_ent | w_ptr | d_pair | d_plist], 16-byte aligned pieces
  auto pad = [](size_t bytes) { return (bytes + 15) & ~(size_t)15; };
  const size_t b_ge = pad(g_ent.size() * sizeof(int4)), b_ce = pad(c_ent.size() * sizeof(int4)), b_gp = pad(g_ptr.size() * sizeof(int)),
               b_cp = pad(c_ptr.size() * sizeof(int)), b_ri = pad(row_info.size() * sizeof(int2)), b_w = pad(win.size() * sizeof(int)),
               b_dr = pad(d_row.size() * sizeof(int4)), b_dv = pad(d_val.size() * sizeof(int4)), b_ev = pad(e_val.size() * sizeof(int2)),
               b_di = pad(d_idx.size() * sizeof(int)), b_dd = pad(d_dup.size() * sizeof(int)),
               b_we = pad(w_ent.size() * sizeof(int4)), b_wp = pad(w_ptr.size() * sizeof(int)),
               b_dp = pad(d_pair.size() * sizeof(int)), b_dl = pad(d_plist.size() * sizeof(int));
  mo_residual_layout* L = new (std::nothrow) mo_residual_layout();
  if (!L) return fail(MO_ERR_HIP, "out of host memory");
  L->device = plan->desc.device; L->n = n; L->num_blocks = num_blocks; L->rows = (int)total_rows; L->values = values;
  L->dev = nullptr;
  const size_t total = b_ge + b_ce + b_gp + b_cp + b_ri + b_w + b_dr + b_dv + b_ev + b_di + b_dd + b_we + b_wp + b_dp + b_dl;
  if (hipSetDevice(plan->desc.device) != hipSuccess || hipMalloc(&L->dev, total) != hipSuccess) {
    (void)hipGetLastError();
    delete L;
    return fail(MO_ERR_HIP, "hipMalloc of the %zu B layout schedule failed", total);
  }
  char* base = (char*)L->dev;
  struct Piece { const void* src; size_t bytes, padded; } pieces[] = {
      {g_ent.data(), g_ent.size() * sizeof(int4), b_ge}, {c_ent.data(), c_ent.size() * sizeof(int4), b_ce},
      {g_ptr.data(), g_ptr.size() * sizeof(int), b_gp},  {c_ptr.data(), c_ptr.size() * sizeof(int), b_cp},
      {row_info.data(), row_info.size() * sizeof(int2), b_ri}, {win.data(), win.size() * sizeof(int), b_w},
      {d_row.data(), d_row.size() * sizeof(int4), b_dr}, {d_val.data(), d_val.size() * sizeof(int4), b_dv},
      {e_val.data(), e_val.size() * sizeof(int2), b_ev}, {d_idx.data(), d_idx.size() * sizeof(int), b_di},
      {d_dup.data(), d_dup.size() * sizeof(int), b_dd},  {w_ent.data(), w_ent.size() * sizeof(int4), b_we},
      {w_ptr.data(), w_ptr.size() * sizeof(int), b_wp},  {d_pair.data(), d_pair.size() * sizeof(int), b_dp},
      {d_plist.data(), d_plist.size() * sizeof(int), b_dl}};
  size_t at = 0;
  const void* dst[15];
  for (int i = 0; i < 15; ++i) {
    dst[i] = base + at;
    if (pieces[i].bytes && hipMemcpy(base + at, pieces[i].src, pieces[i].bytes, hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(L->dev);
      delete L;
      return fail(MO_ERR_HIP, "upload of the layout schedule failed");
    }
    at += pieces[i].padded;
  }
  L->g_ent = (const int4*)dst[0]; L->c_ent = (const int4*)dst[1]; L->g_ptr = (const int*)dst[2]; L->c_ptr = (const int*)dst[3];
  L->row_info = (const int2*)dst[4]; L->win = (const int*)dst[5];
  L->d_row = (const int4*)dst[6]; L->d_val = (const int4*)dst[7]; L->e_val = (const int2*)dst[8]; L->d_idx = (const int*)dst[9];
  L->d_dup = (const int*)dst[10];
  L->w_ent = (const int4*)dst[11]; L->w_ptr = (const int*)dst[12];
  L->d_pair = (const int*)dst[13]; L->d_plist = (const int*)dst[14];
  L->has_dup = !d_dup.empty();
  L->block_rows.assign(rows, rows + num_blocks);
  *out = L;
  return MO_OK;
}

int mo_residual_layout_destroy(mo_residual_layout* layout) {
  if (!layout) return MO_OK;
  if (layout->dev) {
    (void)hipSetDevice(layout->device);
    (void)hipFree(layout->dev);
  }
  delete layout;
  return MO_OK;
}

int64_t mo_residual_layout_values(const mo_residual_layout* layout) { return layout ? layout->values : -1; }
int32_t mo_residual_layout_rows(const mo_residual_layout* layout) { return layout ? layout->rows : -1; }

int mo_linearize_blocks(mo_plan* plan, const mo_residual_layout* layout, const void* J_blocks, int64_t J_stride, const void* r,
                        int64_t r_stride, double lambda, const void* lambda_vec, int64_t lambda_stride, int64_t batch, void* G_out,
                        int64_t G_stride, int32_t G_ld, void* c_out, int64_t c_stride, void* half_sq_out, void* stream) {
  g_err[0] = 0;
  if (int rc = check_plan(plan)) return rc;
  if (int rc = check_layout(plan, layout)) return rc;
  if (batch < 0) return fail(MO_ERR_INVALID_ARGUMENT, "batch must be >= 0");
  if (layout->rows != plan->desc.m_r) return fail(MO_ERR_DIMENSION, "layout has %d rows, plan m_r = %d", layout->rows, plan->desc.m_r);
  if (!J_blocks || !r) return fail(MO_ERR_INVALID_ARGUMENT, "J_blocks / r is NULL");
  if (!c_out) return fail(MO_ERR_INVALID_ARGUMENT, "c_out is NULL");
  if (G_out && G_ld < plan->desc.n) return fail(MO_ERR_DIMENSION, "G_ld %d < n", G_ld);   // (G_out NULL: c_out and half_sq_out only)
  if (batch == 0) return MO_OK;
  mo::BlocksArgs a = blocks_args(layout, batch);
  a.J = J_blocks; a.J_stride = J_stride; a.r = r; a.r_stride = r_stride;
  a.lambda = lambda; a.lambda_vec = lambda_vec; a.lambda_vec_stride = lambda_stride;
  a.G_out = G_out; a.G_out_stride = G_stride; a.G_out_ld = G_ld;
  a.c_out = c_out; a.c_out_stride = c_stride; a.half_sq_out = half_sq_out;
  MO_HIP_CHECK(hipSetDevice(plan->desc.device));
  MO_HIP_CHECK(mo::launch_blocks_linearize(a, plan->desc.dtype, plan->num_cus, (hipStream_t)stream));
  return MO_OK;
}

int mo_jacobian_blocks(mo_plan* plan, const mo_residual_layout* layout, const void* J_blocks, int64_t J_stride, const void* r,
                       int64_t r_stride, int64_t batch, void* J_out, int64_t J_out_stride, int32_t J_out_ld, int32_t J_out_layout,
                       void* abs_sum_out, void* stream) {
  g_err[0] = 0;
  if (int rc = check_plan(plan)) return rc;
  if (int rc = check_layout(plan, layout)) return rc;
  if (batch < 0) return fail(MO_ERR_INVALID_ARGUMENT, "batch must be >= 0");
  if (!J_blocks || !J_out) return fail(MO_ERR_INVALID_ARGUMENT, "J_blocks / J_out is NULL");
  if (abs_sum_out && !r) return fail(MO_ERR_INVALID_ARGUMENT, "abs_sum_out needs r");
  if (J_out_layout != MO_ROW_MAJOR && J_out_layout != MO_COL_MAJOR) return fail(MO_ERR_INVALID_ARGUMENT, "bad J_out_layout");
  const int min_ld = J_out_layout == MO_ROW_MAJOR ? plan->desc.n : layout->rows;
  if (J_out_ld < min_ld) return fail(MO_ERR_DIMENSION, "J_out_ld %d < %d", J_out_ld, min_ld);
  if (batch == 0) return MO_OK;
  mo::BlocksArgs a = blocks_args(layout, batch);
  a.J = J_blocks; a.J_stride = J_stride; a.r = r; a.r_stride = r_stride;
  a.J_out = J_out; a.J_out_stride = J_out_stride; a.J_out_ld = J_out_ld; a.J_out_row_major = J_out_layout == MO_ROW_MAJOR;
  a.abs_sum_out = abs_sum_out;
  MO_HIP_CHECK(hipSetDevice(plan->desc.device));
  MO_HIP_CHECK(mo::launch_blocks_jacobian(a, plan->desc.dtype, plan->num_cus, (hipStream_t)stream));
  return MO_OK;
}

int mo_qp_gradients_blocks(mo_plan* plan, const mo_residual_layout* cost_layout, const void* J_blocks, int64_t J_stride, const void* r,
                           int64_t r_stride, int64_t batch, const void* vars, int64_t vars_stride, const void* u, int64_t u_stride,
                           const mo_block_grads* out, void* stream) {
  g_err[0] = 0;
  // (what can be judged from the arguments alone comes first)
  if (!cost_layout) return fail(MO_ERR_INVALID_ARGUMENT, "cost_layout is NULL");
  if (!vars) return fail(MO_ERR_INVALID_ARGUMENT, "vars is NULL");
  if (!u) return fail(MO_ERR_INVALID_ARGUMENT, "u is NULL");
  if (!out) return fail(MO_ERR_INVALID_ARGUMENT, "out is NULL");
  if (batch < 0) return fail(MO_ERR_INVALID_ARGUMENT, "batch must be >= 0");
  if ((out->dJ_blocks || out->dr) && (!J_blocks || !r)) return fail(MO_ERR_INVALID_ARGUMENT, "dJ_blocks / dr asked for but J_blocks / r is NULL");
  if (int rc = check_plan(plan)) return rc;
  if (int rc = check_layout(plan, cost_layout)) return rc;
  if (!mo::blocks_grad_fits(plan->desc.n, cost_layout->rows, plan->elem))
    return fail(MO_ERR_UNSUPPORTED, "n = %d, %d residual rows: the vectors of one problem exceed the 63 KiB of LDS the block gradient kernel uses", plan->desc.n, cost_layout->rows);
  if (batch == 0 || (!out->dJ_blocks && !out->dr && !out->dlambda)) return MO_OK;
  mo::BlockGradArgs a = block_grad_args(plan, cost_layout, batch, vars, vars_stride, u, u_stride);
  a.J = J_blocks; a.J_stride = J_stride; a.r = r; a.r_stride = r_stride;
  a.dJ = out->dJ_blocks; a.dJ_stride = out->dJ_stride; a.dr = out->dr; a.dr_stride = out->dr_stride;
  a.dlambda = out->dlambda; a.dlambda_stride = out->dlambda_stride;
  MO_HIP_CHECK(hipSetDevice(plan->desc.device));
  MO_HIP_CHECK(mo::launch_blocks_grad(a, plan->desc.dtype, plan->num_cus, (hipStream_t)stream));
  return MO_OK;
}

int mo_linearize_blocks_weighted(mo_plan* plan, const mo_residual_layout* layout, const void* J_blocks, int64_t J_stride, const void* r,
                                 int64_t r_stride, const void* weights, int64_t weights_stride, double lambda, const void* lambda_vec,
                                 int64_t lambda_stride, int64_t batch, void* G_out, int64_t G_stride, int32_t G_ld, void* c_out, int64_t c_stride,
                                 void* half_sq_out, void* stream) {
  if (!weights)
    return mo_linearize_blocks(plan, layout, J_blocks, J_stride, r, r_stride, lambda, lambda_vec, lambda_stride, batch, G_out, G_stride, G_ld,
                               c_out, c_stride, half_sq_out, stream);
  g_err[0] = 0;
  if (int rc = check_plan(plan)) return rc;
  if (int rc = check_layout(plan, layout)) return rc;
  if (batch < 0) return fail(MO_ERR_INVALID_ARGUMENT, "batch must be >= 0");
  if (layout->rows != plan->desc.m_r) return fail(MO_ERR_DIMENSION, "layout has %d rows, plan m_r = %d", layout->rows, plan->desc.m_r);
  if (!J_blocks || !r) return fail(MO_ERR_INVALID_ARGUMENT, "J_blocks / r is NULL");
  if (!c_out) return fail(MO_ERR_INVALID_ARGUMENT, "c_out is NULL");
  if (G_out && G_ld < plan->desc.n) return fail(MO_ERR_DIMENSION, "G_ld %d < n", G_ld);
  if (batch == 0) return MO_OK;
  mo::BlocksArgs a = blocks_args(layout, batch);
  a.J = J_blocks; a.J_stride = J_stride; a.r = r; a.r_stride = r_stride;
  a.weights = weights; a.weights_stride = weights_stride;
  a.lambda = lambda; a.lambda_vec = lambda_vec; a.lambda_vec_stride = lambda_stride;
  a.G_out = G_out; a.G_out_stride = G_stride; a.G_out_ld = G_ld;
  a.c_out = c_out; a.c_out_stride = c_stride; a.half_sq_out = half_sq_out;
  MO_HIP_CHECK(hipSetDevice(plan->desc.device));
  MO_HIP_CHECK(mo::launch_blocks_linearize(a, plan->desc.dtype, plan->num_cus, (hipStream_t)stream));
  return MO_OK;
}

int mo_qp_gradients_blocks_weighted(mo_plan* plan, const mo_residual_layout* cost_layout, const void* J_blocks, int64_t J_stride, const void* r,
                                    int64_t r_stride, const void* weights, int64_t weights_stride, int64_t batch, const void* vars,
                                    int64_t vars_stride, const void* u, int64_t u_stride, const mo_block_weighted_grads* out, void* stream) {
  g_err[0] = 0;
  // (what can be judged from the arguments alone comes first)
  if (!weights) {
    if (out && out->dweights) return fail(MO_ERR_INVALID_ARGUMENT, "dweights asked for but weights is NULL");
    if (!out) return fail(MO_ERR_INVALID_ARGUMENT, "out is NULL");
    const mo_block_grads g = {out->dJ_blocks, out->dJ_stride, out->dr, out->dr_stride, out->dlambda, out->dlambda_stride};
    return mo_qp_gradients_blocks(plan, cost_layout, J_blocks, J_stride, r, r_stride, batch, vars, vars_stride, u, u_stride, &g, stream);
  }
  if (!cost_layout) return fail(MO_ERR_INVALID_ARGUMENT, "cost_layout is NULL");
  if (!vars) return fail(MO_ERR_INVALID_ARGUMENT, "vars is NULL");
  if (!u) return fail(MO_ERR_INVALID_ARGUMENT, "u is NULL");
  if (!out) return fail(MO_ERR_INVALID_ARGUMENT, "out is NULL");
  if (batch < 0) return fail(MO_ERR_INVALID_ARGUMENT, "batch must be >= 0");
  if ((out->dJ_blocks || out->dr || out->dweights) && (!J_blocks || !r))
    return fail(MO_ERR_INVALID_ARGUMENT, "dJ_blocks / dr / dweights asked for but J_blocks / r is NULL");
  if (int rc = check_plan(plan)) return rc;
  if (int rc = check_layout(plan, cost_layout)) return rc;
  if (!mo::blocks_grad_fits(plan->desc.n, cost_layout->rows, plan->elem, true))
    return fail(MO_ERR_UNSUPPORTED, "n = %d, %d residual rows: the vectors of one problem (2 n + 3 rows values) exceed the 63 KiB of LDS the weighted block gradient kernel uses", plan->desc.n, cost_layout->rows);
  if (batch == 0 || (!out->dJ_blocks && !out->dr && !out->dlambda && !out->dweights)) return MO_OK;
  mo::BlockGradArgs a = block_grad_args(plan, cost_layout, batch, vars, vars_stride, u, u_stride);
  a.J = J_blocks; a.J_stride = J_stride; a.r = r; a.r_stride = r_stride;
  a.weights = weights; a.weights_stride = weights_stride;
  a.d_pair = cost_layout->d_pair; a.d_plist = cost_layout->d_plist;
  a.dJ = out->dJ_blocks; a.dJ_stride = out->dJ_stride; a.dr = out->dr; a.dr_stride = out->dr_stride;
  a.dlambda = out->dlambda; a.dlambda_stride = out->dlambda_stride;
  a.dw = out->dweights; a.dw_stride = out->dweights_stride;
  MO_HIP_CHECK(hipSetDevice(plan->desc.device));
  MO_HIP_CHECK(mo::launch_blocks_grad(a, plan->desc.dtype, plan->num_cus, (hipStream_t)stream));
  return MO_OK;
}

int mo_qp_gradients_eq_blocks(mo_plan* plan, const mo_residual_layout* eq_layout, int64_t batch, const void* vars, int64_t vars_stride,
                              const void* u, int64_t u_stride, void* dJ_eq_blocks, int64_t dJ_eq_stride, void* dr_eq,
                              int64_t dr_eq_stride, void* stream) {
  g_err[0] = 0;
  if (!eq_layout) return fail(MO_ERR_INVALID_ARGUMENT, "eq_layout is NULL");
  if (!vars) return fail(MO_ERR_INVALID_ARGUMENT, "vars is NULL");
  if (!u) return fail(MO_ERR_INVALID_ARGUMENT, "u is NULL");
  if (batch < 0) return fail(MO_ERR_INVALID_ARGUMENT, "batch must be >= 0");
  if (int rc = check_plan(plan)) return rc;
  if (int rc = check_layout(plan, eq_layout)) return rc;
  if (eq_layout->rows != plan->desc.k) return fail(MO_ERR_DIMENSION, "eq_layout has %d rows, plan k = %d", eq_layout->rows, plan->desc.k);
  if (batch == 0 || (!dJ_eq_blocks && !dr_eq)) return MO_OK;
  mo::BlockGradArgs a = block_grad_args(plan, eq_layout, batch, vars, vars_stride, u, u_stride);
  a.dJ = dJ_eq_blocks; a.dJ_stride = dJ_eq_stride; a.dr = dr_eq; a.dr_stride = dr_eq_stride;
  MO_HIP_CHECK(hipSetDevice(plan->desc.device));
  MO_HIP_CHECK(mo::launch_blocks_eq_grad(a, plan->desc.dtype, plan->num_cus, (hipStream_t)stream));
  return MO_OK;
}

}  // extern "C"

namespace {
// What mo_qp_gradients_blocks_shared and its workspace query judge alike: first what the arguments alone tell, then the plan, the layouts
// and the LDS rule.  J_blocks / r / vars / u / the workspace are not looked at here.
int block_shared_args(const mo_plan* plan, const mo_residual_layout* cost_layout, const mo_residual_layout* eq_layout, int64_t r_stride,
                      int64_t batch, const mo_block_shared_grads* out, mo::BlockSharedArgs* a) {
  if (!out) return fail(MO_ERR_INVALID_ARGUMENT, "out is NULL");
  if (batch < 0) return fail(MO_ERR_INVALID_ARGUMENT, "batch must be >= 0");
  if (out->dr && r_stride != 0)
    return fail(MO_ERR_INVALID_ARGUMENT, "dr summed over the batch needs one r for the batch: r_stride is %lld, not 0", (long long)r_stride);
  const mo_residual_layout* eq;
  if (int rc = check_layout_pair(plan, cost_layout, eq_layout, out->dJ_eq_blocks || out->dr_eq, "asked for", &eq)) return rc;
  const mo_plan_desc& d = plan->desc;
  memset(a, 0, sizeof(*a));
  a->out = *out;
  if (eq) { a->e_val = eq->e_val; a->eq_values = eq->values; }
  if (d.k == 0) { a->out.dJ_eq_blocks = nullptr; a->out.dr_eq = nullptr; }
  a->n = d.n; a->k = d.k; a->m = d.m; a->rows = cost_layout->rows; a->values = cost_layout->values; a->batch = batch;
  a->d_row = cost_layout->d_row; a->d_idx = cost_layout->d_idx; a->d_val = cost_layout->d_val; a->d_dup = cost_layout->d_dup;
  a->r_stride = r_stride;
  if (!mo::blocks_shared_fits(*a, plan->elem))
    return fail(MO_ERR_UNSUPPORTED, "n = %d, k = %d, %d residual rows: four problems' moment rows, or the r and u_x of one problem beside 64 bytes of flags, exceed the 64 KiB of LDS the batch-reduced block gradient uses",
                d.n, d.k, cost_layout->rows);
  return MO_OK;
}
}  // namespace

extern "C" {

int mo_qp_gradients_blocks_shared_workspace(const mo_plan* plan, const mo_residual_layout* cost_layout, const mo_residual_layout* eq_layout,
                                            int64_t r_stride, int64_t batch, const mo_block_shared_grads* out, int64_t* bytes) {
  g_err[0] = 0;
  if (!bytes) return fail(MO_ERR_INVALID_ARGUMENT, "bytes is NULL");
  mo::BlockSharedArgs a;
  if (int rc = block_shared_args(plan, cost_layout, eq_layout, r_stride, batch, out, &a)) return rc;
  *bytes = (int64_t)mo::blocks_shared_workspace_bytes(a, plan->elem, plan->num_cus);
  return MO_OK;
}

int mo_qp_gradients_blocks_shared(mo_plan* plan, const mo_residual_layout* cost_layout, const void* J_blocks, const void* r, int64_t r_stride,
                                  const mo_residual_layout* eq_layout, int64_t batch, const void* vars, int64_t vars_stride, const void* u,
                                  int64_t u_stride, const int32_t* status_fwd, const int32_t* status_adj, const mo_block_shared_grads* out,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  g_err[0] = 0;
  // (what can be judged from the arguments alone comes first)
  if (out && (out->dJ_blocks || out->dr) && (!J_blocks || !r)) return fail(MO_ERR_INVALID_ARGUMENT, "dJ_blocks / dr asked for but J_blocks / r is NULL");
  mo::BlockSharedArgs a;
  if (int rc = block_shared_args(plan, cost_layout, eq_layout, r_stride, batch, out, &a)) return rc;
  if (int rc = reduced_call_tail(plan, batch, vars, vars_stride, u, u_stride, workspace, workspace_bytes,
                                 mo::blocks_shared_workspace_bytes(a, plan->elem, plan->num_cus), "mo_qp_gradients_blocks_shared_workspace")) return rc;
  const mo_block_shared_grads& o = a.out;
  if (!o.dJ_blocks && !o.dr && !o.dlambda && !o.dJ_eq_blocks && !o.dr_eq) return MO_OK;
  a.J = J_blocks; a.r = r;
  a.vars = vars; a.vars_stride = vars_stride; a.u = u; a.u_stride = u_stride;
  a.status_fwd = status_fwd; a.status_adj = status_adj;
  a.workspace = workspace;
  MO_HIP_CHECK(hipSetDevice(plan->desc.device));
  MO_HIP_CHECK(mo::launch_blocks_shared_grad(a, plan->desc.dtype, plan->num_cus, (hipStream_t)stream));
  return MO_OK;
}

}  // extern "C"

namespace {
// What mo_qp_gradients_blocks_weighted_shared and its workspace query judge alike: what the arguments alone tell, then the plan, the layout
// and the LDS rule.  J_blocks / r / weights / vars / u / the workspace are not looked at here.
int block_wshared_args(const mo_plan* plan, const mo_residual_layout* cost_layout, int64_t r_stride, int64_t weights_stride, int64_t batch,
                       const mo_block_weighted_shared_grads* out, mo::BlockWSharedArgs* a) {
  if (!cost_layout) return fail(MO_ERR_INVALID_ARGUMENT, "cost_layout is NULL");
  if (!out) return fail(MO_ERR_INVALID_ARGUMENT, "out is NULL");
  if (batch < 0) return fail(MO_ERR_INVALID_ARGUMENT, "batch must be >= 0");
  if (out->dr && r_stride != 0)
    return fail(MO_ERR_INVALID_ARGUMENT, "dr summed over the batch needs one r for the batch: r_stride is %lld, not 0", (long long)r_stride);
  if (out->dweights && weights_stride != 0)
    return fail(MO_ERR_INVALID_ARGUMENT, "dweights summed over the batch needs one instance of the weights: weights_stride is %lld, not 0", (long long)weights_stride);
  if (int rc = check_plan(plan)) return rc;
  if (int rc = check_layout(plan, cost_layout)) return rc;
  const mo_plan_desc& d = plan->desc;
  memset(a, 0, sizeof(*a));
  a->out = *out;
  a->n = d.n; a->k = d.k; a->m = d.m; a->rows = cost_layout->rows; a->values = cost_layout->values; a->batch = batch;
  a->d_row = cost_layout->d_row; a->d_idx = cost_layout->d_idx; a->d_val = cost_layout->d_val; a->d_dup = cost_layout->d_dup;
  a->d_pair = cost_layout->d_pair; a->d_plist = cost_layout->d_plist; a->has_dup = cost_layout->has_dup;
  a->r_stride = r_stride; a->weights_stride = weights_stride;
  if (!mo::blocks_wshared_fits(*a, plan->elem))
    return fail(MO_ERR_UNSUPPORTED, "n = %d, %d residual rows: one staged problem (2 n + 2 rows values, rows more with dweights) beside 64 bytes of flags exceeds the 64 KiB of LDS the batch-reduced weighted block gradient uses",
                d.n, cost_layout->rows);
  return MO_OK;
}
}  // namespace

extern "C" {

int mo_qp_gradients_blocks_weighted_shared_workspace(const mo_plan* plan, const mo_residual_layout* cost_layout, int64_t r_stride,
                                                     int64_t weights_stride, int64_t batch, const mo_block_weighted_shared_grads* out,
                                                     int64_t* bytes) {
  g_err[0] = 0;
  if (!bytes) return fail(MO_ERR_INVALID_ARGUMENT, "bytes is NULL");
  mo::BlockWSharedArgs a;
  if (int rc = block_wshared_args(plan, cost_layout, r_stride, weights_stride, batch, out, &a)) return rc;
  *bytes = (int64_t)mo::blocks_wshared_workspace_bytes(a, plan->elem, plan->num_cus);
  return MO_OK;
}

int mo_qp_gradients_blocks_weighted_shared(mo_plan* plan, const mo_residual_layout* cost_layout, const void* J_blocks, const void* r,
                                           int64_t r_stride, const void* weights, int64_t weights_stride, int64_t batch, const void* vars,
                                           int64_t vars_stride, const void* u, int64_t u_stride, const int32_t* status_fwd,
                                           const int32_t* status_adj, const mo_block_weighted_shared_grads* out, void* workspace,
                                           int64_t workspace_bytes, void* stream) {
  g_err[0] = 0;
  // (what can be judged from the arguments alone comes first)
  if (!J_blocks || !r) return fail(MO_ERR_INVALID_ARGUMENT, "J_blocks / r is NULL");
  if (!weights) return fail(MO_ERR_INVALID_ARGUMENT, "weights is NULL (the unweighted call is mo_qp_gradients_blocks_shared)");
  mo::BlockWSharedArgs a;
  if (int rc = block_wshared_args(plan, cost_layout, r_stride, weights_stride, batch, out, &a)) return rc;
  if (int rc = reduced_call_tail(plan, batch, vars, vars_stride, u, u_stride, workspace, workspace_bytes,
                                 mo::blocks_wshared_workspace_bytes(a, plan->elem, plan->num_cus), "mo_qp_gradients_blocks_weighted_shared_workspace")) return rc;
  const mo_block_weighted_shared_grads& o = a.out;
  if (!o.dJ_blocks && !o.dr && !o.dlambda && !o.dweights) return MO_OK;
  a.J = J_blocks; a.r = r; a.weights = weights;
  a.vars = vars; a.vars_stride = vars_stride; a.u = u; a.u_stride = u_stride;
  a.status_fwd = status_fwd; a.status_adj = status_adj;
  a.workspace = workspace;
  MO_HIP_CHECK(hipSetDevice(plan->desc.device));
  MO_HIP_CHECK(mo::launch_blocks_wshared_grad(a, plan->desc.dtype, plan->num_cus, (hipStream_t)stream));
  return MO_OK;
}

}  // extern "C"

namespace {
int tangent_rhs_blocks(mo_plan* plan, const mo_residual_layout* cost_layout, const void* J_blocks, int64_t J_stride, const void* r,
                       int64_t r_stride, const void* weights, int64_t weights_stride, const void* dweights, int64_t dweights_stride,
                       const mo_residual_layout* eq_layout, const int32_t* cons_var, int64_t cons_stride, int64_t batch, const void* vars,
                       int64_t vars_stride, const mo_block_tangents* t, void* rho, int64_t rho_stride, void* stream);
}  // namespace

extern "C" {

int mo_qp_tangent_rhs_blocks_weighted(mo_plan* plan, const mo_residual_layout* cost_layout, const void* J_blocks, int64_t J_stride,
                                      const void* r, int64_t r_stride, const void* weights, int64_t weights_stride,
                                      const mo_residual_layout* eq_layout, const int32_t* cons_var, int64_t cons_stride, int64_t batch,
                                      const void* vars, int64_t vars_stride, const mo_block_weighted_tangents* wt, void* rho, int64_t rho_stride,
                                      void* stream) {
  g_err[0] = 0;
  if (!wt) return fail(MO_ERR_INVALID_ARGUMENT, "t is NULL");
  if (wt->dweights && !weights) return fail(MO_ERR_INVALID_ARGUMENT, "dweights given but weights is NULL");
  const mo_block_tangents t = {wt->dJ_blocks, wt->dJ_stride, wt->dr, wt->dr_stride, wt->dlambda, wt->dlambda_stride, wt->dJ_eq_blocks,
                               wt->dJ_eq_stride, wt->dr_eq, wt->dr_eq_stride, wt->dcons_a, wt->dcons_b, wt->dcons_stride};
  return tangent_rhs_blocks(plan, cost_layout, J_blocks, J_stride, r, r_stride, weights, weights_stride, wt->dweights, wt->dweights_stride,
                            eq_layout, cons_var, cons_stride, batch, vars, vars_stride, &t, rho, rho_stride, stream);
}

int mo_qp_tangent_rhs_blocks(mo_plan* plan, const mo_residual_layout* cost_layout, const void* J_blocks, int64_t J_stride,
                             const void* r, int64_t r_stride, const mo_residual_layout* eq_layout, const int32_t* cons_var,
                             int64_t cons_stride, int64_t batch, const void* vars, int64_t vars_stride, const mo_block_tangents* t, void* rho,
                             int64_t rho_stride, void* stream) {
  g_err[0] = 0;
  return tangent_rhs_blocks(plan, cost_layout, J_blocks, J_stride, r, r_stride, nullptr, 0, nullptr, 0, eq_layout, cons_var, cons_stride, batch,
                            vars, vars_stride, t, rho, rho_stride, stream);
}

}  // extern "C"

namespace {
// mo_qp_tangent_rhs_blocks (weights NULL) and mo_qp_tangent_rhs_blocks_weighted: one admission, one launch
int tangent_rhs_blocks(mo_plan* plan, const mo_residual_layout* cost_layout, const void* J_blocks, int64_t J_stride, const void* r,
                       int64_t r_stride, const void* weights, int64_t weights_stride, const void* dweights, int64_t dweights_stride,
                       const mo_residual_layout* eq_layout, const int32_t* cons_var, int64_t cons_stride, int64_t batch, const void* vars,
                       int64_t vars_stride, const mo_block_tangents* t, void* rho, int64_t rho_stride, void* stream) {
  // (what can be judged from the arguments alone comes first)
  if (!t) return fail(MO_ERR_INVALID_ARGUMENT, "t is NULL");
  if (!vars || !rho) return fail(MO_ERR_INVALID_ARGUMENT, "vars / rho is NULL");
  if (batch < 0) return fail(MO_ERR_INVALID_ARGUMENT, "batch must be >= 0");
  if ((t->dJ_blocks || t->dr || dweights) && (!J_blocks || !r))
    return fail(MO_ERR_INVALID_ARGUMENT, weights ? "dJ_blocks / dr / dweights given but J_blocks / r is NULL" : "dJ_blocks / dr given but J_blocks / r is NULL");
  if (t->dcons_a && !cons_var) return fail(MO_ERR_INVALID_ARGUMENT, "dcons_a given but cons_var is NULL");
  const mo_residual_layout* eq;
  if (int rc = check_layout_pair(plan, cost_layout, eq_layout, t->dJ_eq_blocks || t->dr_eq, "given", &eq)) return rc;
  const mo_plan_desc& d = plan->desc;
  const bool weighted = weights != nullptr;
  if (!mo::blocks_tangent_fits(d.n, d.k, d.m, cost_layout->rows, plan->elem, weighted))
    return fail(MO_ERR_UNSUPPORTED, "n = %d, k = %d, m = %d, %d residual rows: the vectors of one problem (%zu B) exceed the 64 KiB of LDS the block tangent kernel uses",
                d.n, d.k, d.m, cost_layout->rows, mo::blocks_tangent_lds_bytes(d.n, d.k, d.m, cost_layout->rows, plan->elem, weighted));
  if (batch == 0) return MO_OK;
  mo::BlockTangentArgs a;
  memset(&a, 0, sizeof(a));
  a.n = d.n; a.k = d.k; a.m = d.m; a.rows = cost_layout->rows; a.values = cost_layout->values; a.batch = batch;
  a.d_row = cost_layout->d_row; a.d_idx = cost_layout->d_idx; a.d_dup = cost_layout->d_dup;
  a.c_ptr = cost_layout->c_ptr; a.c_ent = cost_layout->c_ent;
  a.vars = vars; a.vars_stride = vars_stride; a.rho = rho; a.rho_stride = rho_stride;
  a.t = *t;
  if (!eq) { a.t.dJ_eq_blocks = nullptr; a.t.dr_eq = nullptr; }
  else { a.e_row = eq->d_row; a.e_val = eq->e_val; a.w_ptr = eq->w_ptr; a.w_ent = eq->w_ent; }
  if (d.m == 0) { a.t.dcons_a = nullptr; a.t.dcons_b = nullptr; }
  else if (cons_var) { a.cons_var = cons_var; a.cons_stride = cons_stride; }
  a.weights = weights; a.weights_stride = weights_stride; a.dw = dweights; a.dw_stride = dweights_stride;
  if (a.t.dJ_blocks || a.t.dr || a.dw) {  // the only tangents that read the blocks; r only against dJ_blocks and dweights
    a.J = J_blocks; a.J_stride = J_stride;
    if (a.t.dJ_blocks || a.dw) { a.r = r; a.r_stride = r_stride; }
  }
  MO_HIP_CHECK(hipSetDevice(d.device));
  MO_HIP_CHECK(mo::launch_blocks_tangent(a, d.dtype, plan->num_cus, (hipStream_t)stream));
  return MO_OK;
}
}  // namespace

extern "C" {

int mo_residual_eval(mo_plan* plan, int32_t family, int32_t rows, const void* params, const void* x, int64_t x_stride,
                     int64_t batch, void* r, int64_t r_stride, void* J, int64_t J_stride, int32_t J_ld, int32_t J_layout,
                     void* stream) {
  g_err[0] = 0;
  if (int rc = check_plan(plan)) return rc;
  const mo_plan_desc& d = plan->desc;
  if (batch < 0) return fail(MO_ERR_INVALID_ARGUMENT, "batch must be >= 0");
  if (!x || !r) return fail(MO_ERR_INVALID_ARGUMENT, "x / r is NULL");
  const int want = mo::residual_family_rows(family, d.n, rows);
  if (want < 0 || want != rows) return fail(MO_ERR_DIMENSION, "residual family %d with n = %d has %d rows, not %d", family, d.n, want, rows);
  if (family == MO_RESIDUAL_PRODUCT_PAIRS && !params) return fail(MO_ERR_INVALID_ARGUMENT, "PRODUCT_PAIRS needs params");
  if (family == MO_RESIDUAL_ACTUATOR_CHAIN && !params) return fail(MO_ERR_INVALID_ARGUMENT, "ACTUATOR_CHAIN needs its parameter block");
  if (J) {
    if (J_layout != MO_ROW_MAJOR && J_layout != MO_COL_MAJOR) return fail(MO_ERR_INVALID_ARGUMENT, "bad J_layout");
    const int min_ld = J_layout == MO_ROW_MAJOR ? d.n : rows;
    if (J_ld < min_ld) return fail(MO_ERR_DIMENSION, "J_ld %d < %d", J_ld, min_ld);
  }
  MO_HIP_CHECK(hipSetDevice(d.device));
  MO_HIP_CHECK(mo::launch_residual_family(family, d.n, rows, batch, d.dtype, params, x, x_stride, r, r_stride, J, J_stride, J_ld,
                                          J_layout == MO_ROW_MAJOR, (hipStream_t)stream));
  return MO_OK;
}

// ---- robust loss functions for residual-block costs

int mo_residual_loss_create(const mo_residual_layout* layout, const int32_t* kinds, const double* scales, mo_residual_loss** out) {
  g_err[0] = 0;
  if (!out) return fail(MO_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  if (!layout) return fail(MO_ERR_INVALID_ARGUMENT, "layout is NULL");
  if (!kinds || !scales) return fail(MO_ERR_INVALID_ARGUMENT, "kinds / scales is NULL");
  const int nb = layout->num_blocks;
  std::vector<int4> blk((size_t)nb);
  std::vector<double> sd((size_t)nb);
  std::vector<float> sf((size_t)nb);
  int trivial = 1, row = 0;
  for (int b = 0; b < nb; ++b) {
    if (kinds[b] < MO_LOSS_TRIVIAL || kinds[b] > MO_LOSS_TUKEY) return fail(MO_ERR_INVALID_ARGUMENT, "block %d: unknown loss kind %d", b, kinds[b]);
    double a = 1.0;  // a TRIVIAL block's scale is ignored
    if (kinds[b] != MO_LOSS_TRIVIAL) {
      a = scales[b];
      if (!(a > 0) || !std::isfinite(a)) return fail(MO_ERR_INVALID_ARGUMENT, "block %d: loss scale %g must be finite and > 0", b, a);
      if (!((float)a > 0) || !std::isfinite((float)a))
        return fail(MO_ERR_INVALID_ARGUMENT, "block %d: loss scale %g is not a finite positive float (the table serves fp32 plans too)", b, a);
      trivial = 0;
    }
    blk[(size_t)b] = make_int4(row, layout->block_rows[(size_t)b], kinds[b], 0);
    sd[(size_t)b] = a;
    sf[(size_t)b] = (float)a;
    row += layout->block_rows[(size_t)b];
  }
  mo_residual_loss* T = new (std::nothrow) mo_residual_loss();
  if (!T) return fail(MO_ERR_HIP, "out of host memory");
  T->device = layout->device; T->num_blocks = nb; T->rows = layout->rows; T->all_trivial = trivial; T->dev = nullptr;
  auto pad = [](size_t bytes) { return (bytes + 15) & ~(size_t)15; };
  const size_t b_blk = pad(blk.size() * sizeof(int4)), b_d = pad(sd.size() * sizeof(double)), b_f = pad(sf.size() * sizeof(float));
  if (hipSetDevice(layout->device) != hipSuccess || hipMalloc(&T->dev, b_blk + b_d + b_f) != hipSuccess) {
    (void)hipGetLastError();
    delete T;
    return fail(MO_ERR_HIP, "hipMalloc of the %zu B loss table failed", b_blk + b_d + b_f);
  }
  char* base = (char*)T->dev;
  if (hipMemcpy(base, blk.data(), blk.size() * sizeof(int4), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(base + b_blk, sd.data(), sd.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(base + b_blk + b_d, sf.data(), sf.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(T->dev);
    delete T;
    return fail(MO_ERR_HIP, "upload of the loss table failed");
  }
  T->blk = (const int4*)base; T->scale_d = (const double*)(base + b_blk); T->scale_f = (const float*)(base + b_blk + b_d);
  *out = T;
  return MO_OK;
}

int mo_residual_loss_destroy(mo_residual_loss* loss) {
  if (!loss) return MO_OK;
  if (loss->dev) {
    (void)hipSetDevice(loss->device);
    (void)hipFree(loss->dev);
  }
  delete loss;
  return MO_OK;
}

int mo_residual_loss_eval(mo_plan* plan, const mo_residual_layout* layout, const mo_residual_loss* loss, const void* r, int64_t r_stride,
                          int64_t batch, void* weights_out, int64_t weights_stride, void* rho_out, void* stream) {
  g_err[0] = 0;
  if (!loss) return fail(MO_ERR_INVALID_ARGUMENT, "loss is NULL");
  if (!r) return fail(MO_ERR_INVALID_ARGUMENT, "r is NULL");
  if (batch < 0) return fail(MO_ERR_INVALID_ARGUMENT, "batch must be >= 0");
  if (int rc = check_plan(plan)) return rc;
  if (int rc = check_layout(plan, layout)) return rc;
  if (int rc = check_loss(layout, loss)) return rc;
  if (weights_out && weights_stride < layout->rows) return fail(MO_ERR_DIMENSION, "weights_stride %lld < rows %d", (long long)weights_stride, layout->rows);
  if (batch == 0 || (!weights_out && !rho_out)) return MO_OK;
  mo::LossArgs a = loss_args(loss, plan->desc.dtype, batch);
  a.r = r; a.r_stride = r_stride; a.weights_out = weights_out; a.weights_stride = weights_stride; a.rho_out = rho_out;
  MO_HIP_CHECK(hipSetDevice(plan->desc.device));
  MO_HIP_CHECK(mo::launch_residual_loss(a, plan->desc.dtype, plan->num_cus, (hipStream_t)stream));
  return MO_OK;
}

int mo_linearize_blocks_robust(mo_plan* plan, const mo_residual_layout* layout, const void* J_blocks, int64_t J_stride, const void* r,
                               int64_t r_stride, double lambda, const void* lambda_vec, int64_t lambda_stride, int64_t batch, void* G_out,
                               int64_t G_stride, int32_t G_ld, void* c_out, int64_t c_stride, void* half_sq_out, const mo_residual_loss* loss,
                               void* weights_out, int64_t weights_stride, void* stream) {
  if (!loss || loss->all_trivial) {  // the sibling itself; the weights asked for are the table's (all 1)
    if (int rc = mo_linearize_blocks(plan, layout, J_blocks, J_stride, r, r_stride, lambda, lambda_vec, lambda_stride, batch, G_out, G_stride,
                                     G_ld, c_out, c_stride, half_sq_out, stream)) return rc;
    if (!loss || !weights_out) return MO_OK;
    return mo_residual_loss_eval(plan, layout, loss, r, r_stride, batch, weights_out, weights_stride, nullptr, stream);
  }
  g_err[0] = 0;
  if (int rc = check_plan(plan)) return rc;
  if (int rc = check_layout(plan, layout)) return rc;
  if (int rc = check_loss(layout, loss)) return rc;
  if (batch < 0) return fail(MO_ERR_INVALID_ARGUMENT, "batch must be >= 0");
  if (layout->rows != plan->desc.m_r) return fail(MO_ERR_DIMENSION, "layout has %d rows, plan m_r = %d", layout->rows, plan->desc.m_r);
  if (!J_blocks || !r) return fail(MO_ERR_INVALID_ARGUMENT, "J_blocks / r is NULL");
  if (!c_out) return fail(MO_ERR_INVALID_ARGUMENT, "c_out is NULL");
  if (G_out && G_ld < plan->desc.n) return fail(MO_ERR_DIMENSION, "G_ld %d < n", G_ld);
  if (weights_out && weights_stride < layout->rows) return fail(MO_ERR_DIMENSION, "weights_stride %lld < rows %d", (long long)weights_stride, layout->rows);
  const int dtype = plan->desc.dtype;
  const bool staged = mo::blocks_weighted_stages(layout->values, layout->rows, plan->elem);
  if (!staged && !weights_out)
    return fail(MO_ERR_UNSUPPORTED, "the layout (%lld values + 2 x %d rows) does not fit the 48 KiB stage of the fused robust linearise: pass weights_out "
                "(the weights then go through it: mo_residual_loss_eval, then mo_linearize_blocks_weighted)", layout->values, layout->rows);
  if (batch == 0) return MO_OK;
  MO_HIP_CHECK(hipSetDevice(plan->desc.device));
  mo::BlocksArgs a = blocks_args(layout, batch);
  a.J = J_blocks; a.J_stride = J_stride; a.r = r; a.r_stride = r_stride;
  a.lambda = lambda; a.lambda_vec = lambda_vec; a.lambda_vec_stride = lambda_stride;
  a.G_out = G_out; a.G_out_stride = G_stride; a.G_out_ld = G_ld;
  a.c_out = c_out; a.c_out_stride = c_stride;
  if (staged) {
    blocks_args_loss(&a, loss, dtype);
    a.half_sq_out = half_sq_out;
    a.weights_out = weights_out; a.weights_out_stride = weights_stride;
  } else {
    mo::LossArgs la = loss_args(loss, dtype, batch);
    la.r = r; la.r_stride = r_stride; la.weights_out = weights_out; la.weights_stride = weights_stride; la.rho_out = half_sq_out;
    MO_HIP_CHECK(mo::launch_residual_loss(la, dtype, plan->num_cus, (hipStream_t)stream));
    a.weights = weights_out; a.weights_stride = weights_stride;
  }
  MO_HIP_CHECK(mo::launch_blocks_linearize(a, dtype, plan->num_cus, (hipStream_t)stream));
  return MO_OK;
}

}  // extern "C"
