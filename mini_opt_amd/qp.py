"""Host-side (Python) mirror of mini_opt's QP interface for BATCHES of problems resident on one MI355X.

    reference (C++)                                   here
    ----------------------------------------------    -------------------------------------------------
    mini_opt::QP                       qp.hpp:104-124  BatchedQP       (G, c | J, r, lambda; A_eq, b_eq; constraints)
    QPInteriorPointSolver              qp.hpp:132-295  QPInteriorPointSolver (Setup / Solve / x_block ... / SetVariables)
      ::Params                         qp.hpp:134-164  Params (same names and defaults)
      private step functions via `friend QPSolverTest` NewtonStep / Iterate / EvaluateKKTConditions (public test hooks)
    ConstrainedNonlinearLeastSquares::LinearizeAndFillQP (cost part, nonlinear.cc:182-189)   BatchedQP.linearize()

All arithmetic happens in the HIP library behind the C ABI (include/mini_opt_hip.h); torch is used only to own device
memory and streams.  There is no CPU path here.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import NamedTuple, Optional

import torch

from . import _lib as L

COMPLEMENTARITY, FIXED_DECREASE, PREDICTOR_CORRECTOR = 0, 1, 2
NAIVE, SOLVE_EQUALITY_CONSTRAINED, USER_PROVIDED = 0, 1, 2
SATISFIED_KKT_TOL, MAX_ITERATIONS = 0, 1

_DT = {torch.float64: L.MO_F64, torch.float32: L.MO_F32}


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@dataclass
class BatchedQP:
    """A batch of QPs of identical shape on one GPU (mini_opt::QP, qp.hpp:104-124).

    Tensor layouts (contiguous, problem index first):
      J    [B, m_r, n]  stacked Jacobian rows (row-major)         r  [B, m_r]      lam: LM damping (nonlinear.cc:187-189)
           other layouts the C ABI takes: J_layout = "row" with J [B, m_r, ld >= n] (a leading dimension beyond n), or
           J_layout = "col" with J [B, n, ld >= m_r] (column-major: tensor row i is column i of J; J_rows = m_r if ld > m_r)
      G    [B, n, n]    memory = n x n COLUMN-major, lower triangle read (pass G_colmajor[b] = G.T for a symmetric G)
      c    [B, n]
      A_eq [B, n, k]    memory = k x n COLUMN-major (A_eq[b] = A.T)  b_eq [B, k]
      cons_var [B, m] int32, cons_a [B, m], cons_b [B, m]          a * x[var] + b >= 0  (qp.hpp:28-70)
    Any of the constraint tensors may have B = 1 to be shared by the whole batch (stride 0).
    """
    n: int
    k: int = 0
    m: int = 0
    J: Optional[torch.Tensor] = None
    r: Optional[torch.Tensor] = None
    lam: float = 0.0
    lam_vec: Optional[torch.Tensor] = None   # [B] per-problem damping; overrides lam (the lambda state of nonlinear.cc:92-96)
    G: Optional[torch.Tensor] = None
    c: Optional[torch.Tensor] = None
    A_eq: Optional[torch.Tensor] = None
    b_eq: Optional[torch.Tensor] = None
    cons_var: Optional[torch.Tensor] = None
    cons_a: Optional[torch.Tensor] = None
    cons_b: Optional[torch.Tensor] = None
    J_layout: str = "row"
    J_rows: Optional[int] = None

    @property
    def m_r(self) -> int:
        if self.J is None:
            return 0
        if self.J_layout == "col":
            return int(self.J_rows if self.J_rows is not None else self.J.shape[2])
        return int(self.J.shape[1])

    @property
    def V(self) -> int:
        return self.n + 2 * self.m + self.k

    def ComputeEigenvalueStats(self) -> torch.Tensor:
        """QP::ComputeEigenvalueStats (qp.hpp:122-123): [B, 3] = QPEigenvalues {min, max, abs_min} of the Hessian of every QP of the batch."""
        return eigenvalue_stats(self)

    def _any(self) -> torch.Tensor:
        for t in (self.J, self.G):
            if t is not None:
                return t
        raise ValueError("BatchedQP needs J or G")

    @property
    def dtype(self):
        return self._any().dtype

    @property
    def device(self):
        return self._any().device

    def batch_of(self, t):
        return int(t.shape[0])

    def as_struct(self) -> L.Problem:
        p = L.Problem()
        ref = self._any()

        def chk(t, shape_tail, dtype=None):
            if t is None:
                return
            if not t.is_cuda or t.device != ref.device:
                raise ValueError("all tensors must live on the same GPU")
            if not t.is_contiguous():
                raise ValueError("tensors must be contiguous")
            if tuple(t.shape[1:]) != tuple(shape_tail):
                raise ValueError(f"bad shape {tuple(t.shape)}, expected [B,{shape_tail}]")
            if t.dtype != (dtype or ref.dtype):
                raise ValueError(f"bad dtype {t.dtype}")

        def stride(t, per):
            return 0 if t.shape[0] == 1 else per

        n, k, m = self.n, self.k, self.m
        if self.J is not None:
            chk(self.r, (self.m_r,))
            ld = int(self.J.shape[2])
            if self.J_layout == "col":
                chk(self.J, (n, ld))
                if ld < self.m_r:
                    raise ValueError("column-major J: leading dimension < m_r")
                p.J, p.J_stride, p.J_ld, p.J_layout = _ptr(self.J), stride(self.J, n * ld), ld, L.MO_COL_MAJOR
            else:
                chk(self.J, (self.m_r, ld))
                if ld < n:
                    raise ValueError("row-major J: leading dimension < n")
                p.J, p.J_stride, p.J_ld, p.J_layout = _ptr(self.J), stride(self.J, self.m_r * ld), ld, L.MO_ROW_MAJOR
            p.r, p.r_stride = _ptr(self.r), stride(self.r, self.m_r)
            p.lam = float(self.lam)
            if self.lam_vec is not None:
                chk(self.lam_vec, ())
                p.lambda_vec, p.lambda_stride = _ptr(self.lam_vec), stride(self.lam_vec, 1)
        else:
            chk(self.G, (n, n)); chk(self.c, (n,))
            p.G, p.G_stride, p.G_ld = _ptr(self.G), stride(self.G, n * n), n
            p.c, p.c_stride = _ptr(self.c), stride(self.c, n)
        if k > 0:
            chk(self.A_eq, (n, k)); chk(self.b_eq, (k,))
            p.A_eq, p.A_stride, p.A_ld = _ptr(self.A_eq), stride(self.A_eq, n * k), k
            p.b_eq, p.b_stride = _ptr(self.b_eq), stride(self.b_eq, k)
        if m > 0:
            chk(self.cons_var, (m,), torch.int32); chk(self.cons_a, (m,)); chk(self.cons_b, (m,))
            if not (self.cons_var.shape[0] == self.cons_a.shape[0] == self.cons_b.shape[0]):
                raise ValueError("constraint tensors must share their batch dimension")
            p.cons_var, p.cons_a, p.cons_b = _ptr(self.cons_var), _ptr(self.cons_a), _ptr(self.cons_b)
            p.cons_stride = stride(self.cons_var, m)
        return p


@dataclass
class Params:
    """QPInteriorPointSolver::Params, qp.hpp:134-164 (same names, same defaults)."""
    initial_mu: float = 1.0
    sigma: float = 0.5
    termination_kkt_tol: float = 1.0e-9
    termination_complementarity_tol: float = 1.0e-6
    max_iterations: int = 10
    barrier_strategy: int = COMPLEMENTARITY
    decrease_mu_only_on_small_error: bool = False
    initial_guess_method: int = NAIVE
    initialize_mu_with_complementarity: bool = False

    def as_struct(self) -> L.SolveParams:
        s = L.SolveParams()
        for f in ("initial_mu", "sigma", "termination_kkt_tol", "termination_complementarity_tol"):
            setattr(s, f, float(getattr(self, f)))
        for f in ("max_iterations", "barrier_strategy", "decrease_mu_only_on_small_error", "initial_guess_method",
                  "initialize_mu_with_complementarity"):
            setattr(s, f, int(getattr(self, f)))
        return s


@dataclass
class SolverOutputs:
    """QPInteriorPointSolverOutputs (structs.hpp:116-134), one entry per problem of the batch."""
    termination_state: torch.Tensor          # [B] int32
    num_iterations: torch.Tensor             # [B] int32
    iterations: torch.Tensor                 # [B, max_iterations, 14]  (kkt_initial[4], kkt_final[4], ip[6])
    lagrange_multipliers: Optional[torch.Tensor]  # [B, 2] {min, l_infinity} or None if k == 0
    status: torch.Tensor                     # [B] int32 MO_STATUS_*


class FailedFactorization(RuntimeError):
    """qp.hpp:331-333; raised for batch == 1 (larger batches report per-problem status words)."""


class QPInteriorPointSolver:
    """Batched mirror of mini_opt::QPInteriorPointSolver (qp.hpp:132-295)."""

    def __init__(self, problem: Optional[BatchedQP] = None, batch: Optional[int] = None, force_generic: bool = False, no_tiny: bool = False):
        self._plan = None
        self._force_generic = force_generic
        self._no_tiny = no_tiny
        self.p_: Optional[BatchedQP] = None
        if problem is not None:
            self.Setup(problem, batch)

    # -- Setup, qp.cc:20-73 ------------------------------------------------------------------------------------
    def Setup(self, problem: BatchedQP, batch: Optional[int] = None) -> None:
        if problem is None:
            raise L.MiniOptError(-1, "Must pass a non-null problem")
        lib = L.lib()
        self._destroy()
        self.p_ = problem
        ref = problem._any()
        self.batch = int(batch if batch is not None else ref.shape[0])
        desc = L.PlanDesc(problem.n, problem.k, problem.m, problem.m_r, _DT[problem.dtype],
                          ref.device.index or 0, (L.MO_PLAN_FORCE_GENERIC if self._force_generic else 0) | (L.MO_PLAN_NO_TINY if self._no_tiny else 0) | L.EXTRA_PLAN_FLAGS, 0, self.batch)
        plan = C.c_void_p()
        L.check(lib.mo_plan_create(C.byref(desc), C.byref(plan)))
        self._plan = plan
        self._prob = problem.as_struct()
        self.variables_ = torch.zeros(self.batch, problem.V, dtype=problem.dtype, device=ref.device)
        self.delta_ = torch.zeros_like(self.variables_)
        self.r_ = torch.zeros_like(self.variables_)
        self.status_ = torch.zeros(self.batch, dtype=torch.int32, device=ref.device)

    def _destroy(self):
        if self._plan is not None:
            L.lib().mo_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    # -- accessors, qp.cc:205-226 ------------------------------------------------------------------------------
    def _blk(self, t, which):
        n, m, k = self.p_.n, self.p_.m, self.p_.k
        lo, hi = {"x": (0, n), "s": (n, n + m), "y": (n + m, n + m + k), "z": (n + m + k, n + 2 * m + k)}[which]
        return t[:, lo:hi]

    def x_block(self): return self._blk(self.variables_, "x")
    def s_block(self): return self._blk(self.variables_, "s")
    def y_block(self): return self._blk(self.variables_, "y")
    def z_block(self): return self._blk(self.variables_, "z")
    def variables(self): return self.variables_

    def SetVariables(self, v: torch.Tensor) -> None:
        self.variables_.copy_(v)

    def problem(self) -> BatchedQP:
        if self.p_ is None:
            raise L.MiniOptError(-1, "Cannot call unless initialized")
        return self.p_

    def step_kernel(self) -> str:
        return L.lib().mo_plan_step_kernel(self._plan, C.byref(self._prob)).decode()

    def solve_kernel(self) -> str:
        return L.lib().mo_plan_solve_kernel(self._plan, C.byref(self._prob)).decode()

    def _mu_arg(self, mu):
        if isinstance(mu, torch.Tensor):
            assert mu.dtype == self.p_.dtype and mu.is_cuda and mu.is_contiguous()
            return mu, (0 if mu.numel() == 1 else 1)
        t = torch.full((1,), float(mu), dtype=self.p_.dtype, device=self.variables_.device)
        return t, 0

    # -- test hooks replacing `friend class QPSolverTest` (qp.hpp:293) -------------------------------------------
    def EvaluateKKTConditions(self, mu=0.0, include_inequalities: bool = True):
        """qp.cc:391-420 + ComputeErrors qp.cc:423-437. Returns (r_ [B,V], kkt [B,4])."""
        mu_t, mu_s = self._mu_arg(mu)
        kkt = torch.zeros(self.batch, 4, dtype=self.p_.dtype, device=self.variables_.device)
        flags = 0 if include_inequalities else L.MO_STEP_NO_INEQUALITIES
        L.check(L.lib().mo_kkt_residual(self._plan, C.byref(self._prob), self.batch, _ptr(self.variables_), self.p_.V,
                                        _ptr(mu_t), mu_s, flags, _ptr(self.r_), self.p_.V, _ptr(kkt), _stream()))
        return self.r_, kkt

    def NewtonStep(self, mu=0.0, tau: float = 0.995, include_inequalities: bool = True):
        """EvaluateKKTConditions -> ComputeLDLT -> SolveForUpdate(mu) -> ComputeAlpha(tau) on the current state
        (qp_test.cc:132-134, qp.cc:192). Returns (delta_ [B,V], alpha [B,2], status [B])."""
        mu_t, mu_s = self._mu_arg(mu)
        alpha = torch.zeros(self.batch, 2, dtype=self.p_.dtype, device=self.variables_.device)
        flags = 0 if include_inequalities else L.MO_STEP_NO_INEQUALITIES
        L.check(L.lib().mo_newton_step(self._plan, C.byref(self._prob), self.batch, _ptr(self.variables_), self.p_.V,
                                       _ptr(mu_t), mu_s, float(tau), flags, _ptr(self.delta_), self.p_.V, _ptr(alpha),
                                       _ptr(self.status_), _stream()))
        return self.delta_, alpha, self.status_

    def Iterate(self, mu, strategy: int = COMPLEMENTARITY):
        """qp.cc:153-201: updates variables_ in place. Returns (ip_outputs [B,6], status [B])."""
        mu_t, mu_s = self._mu_arg(mu)
        ip = torch.zeros(self.batch, 6, dtype=self.p_.dtype, device=self.variables_.device)
        L.check(L.lib().mo_iterate(self._plan, C.byref(self._prob), self.batch, _ptr(self.variables_), self.p_.V,
                                   _ptr(mu_t), mu_s, int(strategy), _ptr(self.delta_), self.p_.V, _ptr(ip),
                                   _ptr(self.status_), _stream()))
        return ip, self.status_

    # -- Solve, qp.cc:100-151 ----------------------------------------------------------------------------------
    def Solve(self, params: Params, record_iterations: bool = True) -> SolverOutputs:
        """qp.cc:100-151.  record_iterations=False skips the per-iteration QPInteriorPointIteration records (outputs.iterations is None):
        the kernel then never takes the square roots of the KKT norms."""
        if self.p_ is None:
            raise L.MiniOptError(-1, "Must have a valid problem")
        dev, dt = self.variables_.device, self.p_.dtype
        term = torch.zeros(self.batch, dtype=torch.int32, device=dev)
        nit = torch.zeros(self.batch, dtype=torch.int32, device=dev)
        its = torch.full((self.batch, max(int(params.max_iterations), 1), L.MO_ITER_RECORD), float("nan"), dtype=dt,
                         device=dev) if record_iterations else None
        lag = torch.zeros(self.batch, 2, dtype=dt, device=dev) if self.p_.k > 0 else None
        sp = params.as_struct()
        L.check(L.lib().mo_qp_solve(self._plan, C.byref(self._prob), self.batch, C.byref(sp), _ptr(self.variables_),
                                    self.p_.V, _ptr(term), _ptr(nit), _ptr(its), _ptr(lag), _ptr(self.status_),
                                    _stream()))
        if self.batch == 1:
            st = int(self.status_[0])
            if st == L.MO_STATUS_FACTORIZATION_FAILED:
                raise FailedFactorization("Failed to solve self-adjoint (lower) system. The hessian may not be semi-definite.")
            if st != L.MO_STATUS_OK:
                raise L.MiniOptError(-1, L.lib().mo_status_string(st).decode())
        return SolverOutputs(term, nit, its, lag, self.status_)


class QPNullSpaceSolver:
    """Batched mirror of mini_opt::QPNullSpaceSolver (qp.hpp:296-315, qp.cc:679-729): equality-constrained QPs, no inequalities.
    Solve returns QPNullSpaceTerminationState per problem (0 SUCCESS, 1 NOT_POSITIVE_DEFINITE); variables() is x [B, n]."""
    SUCCESS, NOT_POSITIVE_DEFINITE = 0, 1

    def __init__(self):
        self.x_ = None

    def Solve(self, p: BatchedQP) -> torch.Tensor:
        lib = L.lib()
        ref = p._any()
        B = max(int(t.shape[0]) for t in (p.J, p.G, p.A_eq) if t is not None)
        desc = L.PlanDesc(p.n, p.k, 0, p.m_r, _DT[p.dtype], ref.device.index or 0, L.EXTRA_PLAN_FLAGS, 0, B)
        plan = C.c_void_p()
        L.check(lib.mo_plan_create(C.byref(desc), C.byref(plan)))
        try:
            q = BatchedQP(n=p.n, k=p.k, J=p.J, r=p.r, lam=p.lam, lam_vec=p.lam_vec, G=p.G, c=p.c, A_eq=p.A_eq, b_eq=p.b_eq)
            prob = q.as_struct()
            self.x_ = torch.empty(B, p.n, dtype=ref.dtype, device=ref.device)
            term = torch.empty(B, dtype=torch.int32, device=ref.device)
            L.check(lib.mo_nullspace_solve(plan, C.byref(prob), B, _ptr(self.x_), p.n, _ptr(term), _stream()))
        finally:
            lib.mo_plan_destroy(plan)
        return term

    def variables(self) -> torch.Tensor:
        return self.x_


def eigenvalue_stats(problem: BatchedQP) -> torch.Tensor:
    """QP::ComputeEigenvalueStats (qp.hpp:122-123, qp.cc:12-16) for every QP of the batch: [B, 3] = QPEigenvalues {min, max, abs_min} of the
    Hessian -- sym(G) from the lower triangle of (G, c) input, or J^T J + lambda I for (J, r, lambda) input.

    A NaN or +-inf among the entries read (the lower triangle of G -- the strict upper triangle is never read -- or anywhere in J, or a
    J^T J that overflows) gives [NaN, NaN, NaN] for that problem alone, as Eigen's solver propagates it; a NaN or negative lambda acts as 0.
    The matrix is scaled by an exact power of two before the factorisation and the results are scaled back: 2^s G gives 2^s times the
    results of G bit for bit, at any magnitude the dtype can hold."""
    lib = L.lib()
    ref = problem.J if problem.J is not None else problem.G
    B = int(ref.shape[0])
    desc = L.PlanDesc(problem.n, 0, 0, problem.m_r, _DT[problem.dtype], ref.device.index or 0, L.EXTRA_PLAN_FLAGS, 0, B)
    plan = C.c_void_p()
    L.check(lib.mo_plan_create(C.byref(desc), C.byref(plan)))
    try:
        out = torch.empty(B, 3, dtype=problem.dtype, device=ref.device)
        prob = problem.as_struct()   # (only the cost part is read)
        L.check(lib.mo_qp_eigenvalue_stats(plan, C.byref(prob), B, _ptr(out), _stream()))
        return out
    finally:
        lib.mo_plan_destroy(plan)


class Covariance(NamedTuple):
    """Result of covariance(): cov [B, q, q] or None, var [B, q] or None, status [B] int32 (MO_STATUS_*)."""
    cov: Optional[torch.Tensor]
    var: Optional[torch.Tensor]
    status: torch.Tensor


def covariance(G: torch.Tensor, A_eq: Optional[torch.Tensor] = None, select=None, scale=None, full: bool = True, diag: bool = False) -> Covariance:
    """Parameter covariance of a fit (mo_qp_covariance): C = scale Z (Z^T S Z)^-1 Z^T per problem, with S = sym(G) from the lower triangle
    and Z an orthonormal basis of null(A_eq) (no A_eq: C = scale S^-1) -- the top-left block of the inverse of [[S, A^T], [A, 0]].

    G [B or 1, n, n] in BatchedQP's convention (column-major, lower triangle read), A_eq [B or 1, n, k] as BatchedQP.A_eq.  select: the
    variables wanted (a sequence or int tensor, unsorted and repeated indices allowed; None = all n).  scale: None, a number or a [B] tensor.
    full / diag choose the outputs: cov [B, q, q] (symmetric to the bit) and var [B, q] (the bits of its diagonal).  status [B]:
    MO_STATUS_OK, NOT_POSITIVE_DEFINITE (the reduced Hessian has a pivot <= 0), NONFINITE or BAD_INDEX; the outputs of a failed problem are
    NaN.  A singular G that is positive definite on null(A_eq) succeeds; a rank-deficient A_eq lowers the rank and does not fail.
    Inequality constraints are not part of this: pass an active bound that is to be pinned as an equality row."""
    if not (full or diag):
        raise ValueError("nothing asked for: full and diag are both False")
    if G.dim() != 3 or G.shape[1] != G.shape[2] or not G.is_cuda or not G.is_contiguous() or G.dtype not in _DT:
        raise ValueError(f"G: expected a contiguous [B or 1, n, n] float tensor on a GPU, got {tuple(G.shape)} {G.dtype}")
    n, dev, dt = int(G.shape[1]), G.device, G.dtype
    k = 0
    B = int(G.shape[0])
    if A_eq is not None:
        if A_eq.dim() != 3 or int(A_eq.shape[1]) != n or A_eq.device != dev or A_eq.dtype != dt or not A_eq.is_contiguous():
            raise ValueError(f"A_eq: expected a contiguous [B or 1, {n}, k] {dt} tensor on {dev}, got {tuple(A_eq.shape)} {A_eq.dtype}")
        k = int(A_eq.shape[2])
        B = max(B, int(A_eq.shape[0]))
    scale_t, scale_stride = None, 0
    if scale is not None:
        scale_t = scale if isinstance(scale, torch.Tensor) else torch.full((1,), float(scale), dtype=dt, device=dev)
        if scale_t.dim() != 1 or scale_t.dtype != dt or scale_t.device != dev or not scale_t.is_contiguous():
            raise ValueError(f"scale: expected a number or a contiguous [B] {dt} tensor on {dev}")
        B = max(B, int(scale_t.shape[0]))
        scale_stride = 0 if scale_t.shape[0] == 1 else 1
    for t in (G, A_eq, scale_t):
        if t is not None and int(t.shape[0]) not in (1, B):
            raise ValueError(f"leading dimension {int(t.shape[0])}: expected {B} or 1")
    sel_t, q = None, n
    if select is not None:
        sel_t = torch.as_tensor(select).to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
        q = int(sel_t.numel())
    lib = L.lib()
    desc = L.PlanDesc(n, k, 0, 0, _DT[dt], dev.index or 0, L.EXTRA_PLAN_FLAGS, 0, B)
    plan = C.c_void_p()
    L.check(lib.mo_plan_create(C.byref(desc), C.byref(plan)))
    try:
        prob = L.Problem()
        prob.G, prob.G_stride, prob.G_ld = _ptr(G), (0 if G.shape[0] == 1 else n * n), n
        if k > 0:
            prob.A_eq, prob.A_stride, prob.A_ld = _ptr(A_eq), (0 if A_eq.shape[0] == 1 else n * k), k
        cov = torch.empty(B, q, q, dtype=dt, device=dev) if full else None
        var = torch.empty(B, q, dtype=dt, device=dev) if diag else None
        status = torch.empty(B, dtype=torch.int32, device=dev)
        L.check(lib.mo_qp_covariance(plan, C.byref(prob), B, _ptr(sel_t), q, _ptr(scale_t), scale_stride, _ptr(cov), q * q, q, _ptr(var), q,
                                     _ptr(status), _stream()))
    finally:
        lib.mo_plan_destroy(plan)
    return Covariance(cov, var, status)


def linearize(problem: BatchedQP, force_generic: bool = False):
    """Cost part of LinearizeAndFillQP (nonlinear.cc:182-189): returns (G [B,n,n] col-major lower, c [B,n], 0.5|r|^2 [B])."""
    lib = L.lib()
    ref = problem.J
    B, n = int(ref.shape[0]), problem.n
    desc = L.PlanDesc(n, 0, 0, problem.m_r, _DT[problem.dtype], ref.device.index or 0,
                      (L.MO_PLAN_FORCE_GENERIC if force_generic else 0) | L.EXTRA_PLAN_FLAGS, 0, B)
    plan = C.c_void_p()
    L.check(lib.mo_plan_create(C.byref(desc), C.byref(plan)))
    try:
        G = torch.empty(B, n, n, dtype=ref.dtype, device=ref.device)
        c = torch.empty(B, n, dtype=ref.dtype, device=ref.device)
        f = torch.empty(B, dtype=ref.dtype, device=ref.device)
        q = BatchedQP(n=n, J=problem.J, r=problem.r, lam=problem.lam, J_layout=problem.J_layout, J_rows=problem.J_rows)
        prob = q.as_struct()
        L.check(lib.mo_linearize(plan, C.byref(prob), B, _ptr(G), n * n, n, _ptr(c), n, _ptr(f), _stream()))
    finally:
        lib.mo_plan_destroy(plan)
    return G, c, f


# ---- residual-block input (mini_opt::Problem::costs: residual.hpp:60-250, nonlinear.cc:170-214) ---------------------------------------
def pack_blocks(J_blocks) -> torch.Tensor:
    """Packed values of a list of residual Jacobians [B, R_b, P_b] (each the local Jacobian a Residual's functor fills): [B, sum R_b P_b],
    block b column-major at offset sum_{b' < b} R_b' P_b' -- the J_blocks input of linearize_blocks / jacobian_blocks."""
    return torch.cat([J.transpose(1, 2).reshape(J.shape[0], -1) for J in J_blocks], dim=1).contiguous()


def unpack_blocks(packed: torch.Tensor, shapes):
    """Inverse of pack_blocks: shapes = [(R_b, P_b), ...] -> list of [B, R_b, P_b] views."""
    out, off = [], 0
    for R, P in shapes:
        out.append(packed[:, off:off + R * P].reshape(packed.shape[0], P, R).transpose(1, 2))
        off += R * P
    return out


class ResidualLayout:
    """A residual-block layout (mo_residual_layout): blocks = [(index, rows), ...], one per Residual in order, shared by every problem of a
    batch.  Owns an n-variable plan with m_r = sum rows on `device`, which linearize_blocks / jacobian_blocks launch on."""

    def __init__(self, n: int, blocks, dtype=torch.float64, device="cuda:0"):
        lib = L.lib()
        self.n = int(n)
        self.blocks = [(tuple(int(i) for i in idx), int(R)) for idx, R in blocks]
        self.dtype = dtype
        self.device = torch.device(device)
        self.shapes = [(R, len(idx)) for idx, R in self.blocks]
        self.rows = sum(R for _, R in self.blocks)
        self._plan = None
        self.h = None
        desc = L.PlanDesc(self.n, 0, 0, max(self.rows, 1), _DT[dtype], self.device.index or 0, L.EXTRA_PLAN_FLAGS, 0, 0)
        plan = C.c_void_p()
        L.check(lib.mo_plan_create(C.byref(desc), C.byref(plan)))
        self._plan = plan
        self.h = create_layout(plan, self.blocks)
        self.values = int(lib.mo_residual_layout_values(self.h))

    def __del__(self):
        try:
            if self.h is not None:
                L.lib().mo_residual_layout_destroy(self.h)
            if self._plan is not None:
                L.lib().mo_plan_destroy(self._plan)
        except Exception:
            pass


def create_layout(plan, blocks) -> C.c_void_p:
    """mo_residual_layout_create for a plan handle and [(index, rows), ...]; the caller destroys the handle."""
    rows = (C.c_int32 * len(blocks))(*[int(R) for _, R in blocks])
    params = (C.c_int32 * len(blocks))(*[len(idx) for idx, _ in blocks])
    flat = [int(i) for idx, _ in blocks for i in idx]
    index = (C.c_int32 * max(len(flat), 1))(*flat)
    h = C.c_void_p()
    L.check(L.lib().mo_residual_layout_create(plan, len(blocks), rows, params, index, C.byref(h)))
    return h


TRIVIAL, HUBER, SOFT_L1, CAUCHY, TUKEY = range(5)   # mo_loss_kind


def create_loss(layout_handle, losses) -> C.c_void_p:
    """mo_residual_loss_create for a layout handle and [(kind, scale), ...], one per block; the caller destroys the handle."""
    kinds = (C.c_int32 * max(len(losses), 1))(*[int(k) for k, _ in losses])
    scales = (C.c_double * max(len(losses), 1))(*[float(a) for _, a in losses])
    h = C.c_void_p()
    L.check(L.lib().mo_residual_loss_create(layout_handle, kinds, scales, C.byref(h)))
    return h


class ResidualLoss:
    """A robust-loss table (mo_residual_loss) for the blocks of `layout`: losses = [(kind, scale), ...], one per block, kind one of TRIVIAL,
    HUBER, SOFT_L1, CAUCHY, TUKEY (rho(s) with s = |r_b|^2; the table: include/mini_opt_hip.h).  Serves fp64 and fp32 layouts of the same
    blocks on the same device."""

    def __init__(self, layout: ResidualLayout, losses):
        self.h = None
        self.losses = [(int(k), float(a)) for k, a in losses]
        if len(self.losses) != len(layout.blocks):
            raise L.MiniOptError(-2, f"{len(self.losses)} losses for a layout of {len(layout.blocks)} blocks")
        self.layout = layout
        self.h = create_loss(layout.h, self.losses)

    def __del__(self):
        try:
            if self.h is not None:
                L.lib().mo_residual_loss_destroy(self.h)
        except Exception:
            pass


def loss_weights(layout: ResidualLayout, loss: ResidualLoss, r: torch.Tensor):
    """mo_residual_loss_eval: (weights [B, rows], rho [B]) for r [B, rows] -- w_b = rho_b'(|r_b|^2) repeated over the block's rows (the
    `weights` of linearize_blocks and solve_qp) and 0.5 sum_b rho_b(|r_b|^2)."""
    if r.dim() != 2 or int(r.shape[1]) != layout.rows or not r.is_contiguous() or r.dtype != layout.dtype or r.device != layout.device:
        raise ValueError(f"expected a contiguous [B, {layout.rows}] {layout.dtype} tensor on {layout.device}, got {tuple(r.shape)} {r.dtype}")
    B = int(r.shape[0])
    w = torch.empty(B, layout.rows, dtype=layout.dtype, device=layout.device)
    f = torch.empty(B, dtype=layout.dtype, device=layout.device)
    L.check(L.lib().mo_residual_loss_eval(layout._plan, layout.h, loss.h, _ptr(r), layout.rows, B, _ptr(w), layout.rows, _ptr(f), _stream()))
    return w, f


def _check_blocks(layout: ResidualLayout, J_blocks: torch.Tensor, r: torch.Tensor):
    for t, w in ((J_blocks, layout.values), (r, layout.rows)):
        if t.dim() != 2 or int(t.shape[1]) != w or not t.is_contiguous() or t.dtype != layout.dtype or t.device != layout.device:
            raise ValueError(f"expected a contiguous [B, {w}] {layout.dtype} tensor on {layout.device}, got {tuple(t.shape)} {t.dtype}")
    B = max(int(J_blocks.shape[0]), int(r.shape[0]))
    return B, (0 if J_blocks.shape[0] == 1 else layout.values), (0 if r.shape[0] == 1 else layout.rows)


def linearize_blocks(layout: ResidualLayout, J_blocks: torch.Tensor, r: torch.Tensor, lam: float = 0.0, lam_vec: Optional[torch.Tensor] = None,
                     want_G: bool = True, batch: Optional[int] = None, weights: Optional[torch.Tensor] = None,
                     loss: Optional["ResidualLoss"] = None, return_weights: bool = False):
    """Cost part of LinearizeAndFillQP (nonlinear.cc:182-189) from packed residual blocks: sum_b UpdateHessian (residual.hpp:186-226) +
    lambda I.  Returns (G [B,n,n] col-major lower, strict upper 0; c [B,n]; sum_b 0.5 |r_b|^2 [B]).  J_blocks / r / lam_vec with a leading
    dimension of 1 are read with stride 0; B is the largest leading dimension (or `batch`, if that is larger).  want_G=False: G is not
    formed (returned as None); c has the bits of the full call.  weights [B or 1, rows]: one weight per stacked residual row
    (mo_linearize_blocks_weighted): G = sum_b J_b^T W_b J_b by the same pair rule, c = sum_b J_b^T W_b r_b, the third result 0.5 sum w r^2; a
    row whose weight is exactly 0 is never read into the arithmetic (its J values and r may be NaN).
    loss (a ResidualLoss; not together with weights): the robust cost, mo_linearize_blocks_robust -- the weights are rho_b'(|r_b|^2), formed
    inside the kernel; the third result is 0.5 sum_b rho_b.  return_weights=True appends the weights the kernel used ([B, rows]) to the
    results; a layout too large for the kernel's LDS stage needs it (the weights then go through that tensor)."""
    if loss is not None and weights is not None:
        raise ValueError("weights and loss cannot be combined")
    if return_weights and loss is None:
        raise ValueError("return_weights needs a loss")
    B, js, rs = _check_blocks(layout, J_blocks, r)
    ws = 0
    if weights is not None:
        if (weights.dim() != 2 or int(weights.shape[1]) != layout.rows or not weights.is_contiguous() or weights.dtype != layout.dtype
                or weights.device != layout.device):
            raise ValueError(f"weights: expected a contiguous [B or 1, {layout.rows}] {layout.dtype} tensor on {layout.device}")
        ws = 0 if weights.shape[0] == 1 else layout.rows
        B = max(B, int(weights.shape[0]))
    n = layout.n
    ls = 0
    if lam_vec is not None:
        if lam_vec.dtype != layout.dtype or not lam_vec.is_contiguous() or lam_vec.dim() != 1:
            raise ValueError("lam_vec must be a contiguous [B] tensor of the layout's dtype")
        ls = 0 if lam_vec.shape[0] == 1 else 1
        B = max(B, int(lam_vec.shape[0]))
    if batch is not None:
        B = max(B, int(batch))
    for t in (J_blocks, r, lam_vec, weights):
        if t is not None and int(t.shape[0]) not in (1, B):
            raise ValueError(f"leading dimension {int(t.shape[0])}: expected {B} or 1")
    G = torch.empty(B, n, n, dtype=layout.dtype, device=layout.device) if want_G else None
    c = torch.empty(B, n, dtype=layout.dtype, device=layout.device)
    f = torch.empty(B, dtype=layout.dtype, device=layout.device)
    if loss is not None:
        w = torch.empty(B, layout.rows, dtype=layout.dtype, device=layout.device) if return_weights else None
        L.check(L.lib().mo_linearize_blocks_robust(layout._plan, layout.h, _ptr(J_blocks), js, _ptr(r), rs, float(lam), _ptr(lam_vec), ls, B,
                                                   _ptr(G), n * n, n, _ptr(c), n, _ptr(f), loss.h, _ptr(w), layout.rows, _stream()))
        return (G, c, f, w) if return_weights else (G, c, f)
    if weights is not None:
        L.check(L.lib().mo_linearize_blocks_weighted(layout._plan, layout.h, _ptr(J_blocks), js, _ptr(r), rs, _ptr(weights), ws, float(lam),
                                                     _ptr(lam_vec), ls, B, _ptr(G), n * n, n, _ptr(c), n, _ptr(f), _stream()))
        return G, c, f
    L.check(L.lib().mo_linearize_blocks(layout._plan, layout.h, _ptr(J_blocks), js, _ptr(r), rs, float(lam), _ptr(lam_vec), ls, B,
                                        _ptr(G), n * n, n, _ptr(c), n, _ptr(f), _stream()))
    return G, c, f


def jacobian_blocks(layout: ResidualLayout, J_blocks: torch.Tensor, r: torch.Tensor, row_major: bool = False):
    """UpdateJacobian stacked (residual.hpp:230-250, nonlinear.cc:191-206): the dense (sum R_b) x n matrix with every block's columns
    assigned (the last of a repeated index wins) and |r|_1 [B].  row_major=False: [B, n, rows] (memory = rows x n column-major, QP::A_eq);
    row_major=True: [B, rows, n]."""
    B, js, rs = _check_blocks(layout, J_blocks, r)
    n, m = layout.n, layout.rows
    J = torch.empty((B, m, n) if row_major else (B, n, m), dtype=layout.dtype, device=layout.device)
    s = torch.empty(B, dtype=layout.dtype, device=layout.device)
    L.check(L.lib().mo_jacobian_blocks(layout._plan, layout.h, _ptr(J_blocks), js, _ptr(r), rs, B, _ptr(J), m * n, n if row_major else m,
                                       L.MO_ROW_MAJOR if row_major else L.MO_COL_MAJOR, _ptr(s), _stream()))
    return J, s
