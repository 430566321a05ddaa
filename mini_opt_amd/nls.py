"""Host-side (Python) mirror of mini_opt's constrained nonlinear least squares for BATCHES of problems on one MI355X.

    reference (C++)                                              here
    ---------------------------------------------------------    ------------------------------------------------------
    mini_opt::Problem                      nonlinear.hpp:33-52    Problem (dimension, cost, equality, inequality_constraints)
    ConstrainedNonlinearLeastSquares       nonlinear.hpp:127-230  ConstrainedNonlinearLeastSquares (Solve / variables /
      ::Params                             nonlinear.hpp:64-124     EvaluateNonlinearErrors), Params (same names, defaults)
      ::LinearizeAndFillQP (static)        nonlinear.cc:170-214   fill_qp
      ::ComputeQPCostDerivative (static)   nonlinear.cc:452-483   qp_cost_derivative
    NLSSolverOutputs / NLSIteration        structs.hpp:277-347    NLSSolverOutputs (tensors, one row per problem)

The residual functions are the caller's (the reference's Residual objects are host functors, residual.hpp:28-143): here they
are callables on torch batches, cost(x [B, n], want_J) -> (r [B, m_r], J [B, m_r, n] | None) and equality(...) ->
(r_eq [B, k], J_eq [B, k, n] | None), enqueuing device work on the current stream.  Everything else runs in the HIP library
behind mo_nls_solve (include/mini_opt_hip.h); there is no CPU path here.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Callable, Optional, Sequence, Tuple

import torch

from . import _lib as L
from .qp import BatchedQP, _DT, _ptr, _stream

# NLSTerminationState (structs.hpp:233-248) + MO_NLS_QP_FAILURE (the reference throws there)
(MAX_ITERATIONS, SATISFIED_ABSOLUTE_TOL, SATISFIED_RELATIVE_TOL, SATISFIED_FIRST_ORDER_TOL, MAX_LAMBDA, QP_INDEFINITE,
 USER_CALLBACK, QP_FAILURE) = range(8)
# StepSizeSelectionResult (structs.hpp:215-228)
(STEP_SUCCESS, STEP_MAX_ITERATIONS, STEP_FIRST_ORDER_SATISFIED, STEP_POSITIVE_DERIVATIVE, STEP_FAILURE_NON_FINITE_COST,
 STEP_FAILURE_INVALID_ALPHA) = range(6)
ARMIJO_BACKTRACK, POLYNOMIAL_APPROXIMATION = 0, 1  # LineSearchStrategy (structs.hpp:148-153)


def TerminationStateIndicatesSatisfiedTol(state) -> torch.Tensor:
    """structs.hpp:250-262, element-wise."""
    return (state == SATISFIED_ABSOLUTE_TOL) | (state == SATISFIED_RELATIVE_TOL) | (state == SATISFIED_FIRST_ORDER_TOL)


@dataclass
class Params:
    """ConstrainedNonlinearLeastSquares::Params, nonlinear.hpp:64-124 (same names, same defaults)."""
    max_iterations: int = 10
    max_qp_iterations: int = 10
    termination_kkt_tolerance: float = 1.0e-6
    absolute_exit_tol: float = 1.0e-12
    relative_exit_tol: float = 1.0e-5
    absolute_first_derivative_tol: float = 1.0e-6
    max_line_search_iterations: int = 2
    line_search_strategy: int = POLYNOMIAL_APPROXIMATION
    armijo_search_tau: float = 0.8
    equality_penalty_initial: float = 1.0
    equality_penalty_scale_factor: float = 1.01
    equality_penalty_rho: float = 0.1
    lambda_initial: float = 0.0
    lambda_failure_init: float = 1.0e-2
    lambda_decrease_on_success: float = 0.1
    lambda_decrease_on_restore: float = 0.8
    max_lambda: float = 1.0
    min_lambda: float = 0.0
    log_qp_eigenvalues: bool = False   # nonlinear.hpp:122-123: record the QPEigenvalues of every iteration's QP Hessian

    def as_struct(self, retraction: int = L.MO_RETRACT_EUCLIDEAN) -> L.NlsParams:
        p = L.NlsParams()
        L.lib().mo_default_nls_params(C.byref(p))
        for name, _ in L.NlsParams._fields_:
            if hasattr(self, name):
                setattr(p, name, int(getattr(self, name)) if name == "log_qp_eigenvalues" else getattr(self, name))
        p.retraction = int(retraction)   # the Retraction is a constructor argument of the solver (nonlinear.hpp:127), not a Param
        return p


ResidualFn = Callable[[torch.Tensor, bool], Tuple[torch.Tensor, Optional[torch.Tensor]]]

ROSENBROCK, HIMMELBLAU, SPHERE, PRODUCT_PAIRS, ACTUATOR_CHAIN = range(5)  # mo_residual_family
WRAP_PI = "wrap_pi"  # built-in retraction: x + alpha dx wrapped into [-pi, pi) (the reference's robot tests, nonlinear_test.cc:874-880)


def actuator_chain_params(chains, rows, dtype=torch.float64, device="cuda:0") -> torch.Tensor:
    """Parameter block of the ACTUATOR_CHAIN device family (layout: include/mini_opt_hip.h).
    chains: list of chains, each a list of links dict(rotation_xyz=(3), translation=(3), mask=(6 flags), params=(x index per active flag));
    rows:   list of dict(const=float, lin={x index: coefficient}, terms=[(chain, wx, wy, wz), ...])."""
    out = [float(len(chains))]
    for links in chains:
        if len(links) > 8:
            raise L.MiniOptError(-3, "ACTUATOR_CHAIN: at most 8 links per chain")
        out.append(float(len(links)))
        for l in links:
            out.extend(float(v) for v in l["rotation_xyz"])
            out.extend(float(v) for v in l["translation"])
            idx = iter(l["params"])
            out.extend(float(next(idx)) if flag else -1.0 for flag in l["mask"])
    for row in rows:
        out.append(float(row["const"]))
        out.append(float(len(row["lin"])))
        for i, cf in row["lin"].items():
            out.extend((float(i), float(cf)))
        out.append(float(len(row["terms"])))
        for c, wx, wy, wz in row["terms"]:
            out.extend((float(c), float(wx), float(wy), float(wz)))
    return torch.tensor(out, dtype=dtype, device=device)


@dataclass
class DeviceFamily:
    """One of the library's device residual families (mo_residual_eval): evaluated by a HIP kernel straight into the solver's
    buffers -- no torch ops, no copies.  `params`: device tensor of family parameters (PRODUCT_PAIRS: the products v_q)."""
    family: int
    rows: int
    params: Optional[torch.Tensor] = None

    def eval_into(self, plan, x: torch.Tensor, r: torch.Tensor, J: Optional[torch.Tensor], n: int, row_major: bool) -> None:
        B = int(x.shape[0])
        L.check(L.lib().mo_residual_eval(plan.h, self.family, self.rows, _ptr(self.params), _ptr(x), int(x.stride(0)), B, _ptr(r),
                                         self.rows, _ptr(J), self.rows * n, n if row_major else self.rows,
                                         L.MO_ROW_MAJOR if row_major else L.MO_COL_MAJOR, _stream()))

    def __call__(self, x: torch.Tensor, want_J: bool):
        """The ResidualFn contract, for use outside mo_nls_solve (returns J as [B, rows, n])."""
        B, n = int(x.shape[0]), int(x.shape[1])
        plan = _Plan(n, 0, 0, max(self.rows, 1), x.dtype, x.device, B)
        r = torch.empty(B, self.rows, dtype=x.dtype, device=x.device)
        J = torch.empty(B, self.rows, n, dtype=x.dtype, device=x.device) if want_J else None
        self.eval_into(plan, x.contiguous(), r, J, n, True)
        return r, J


@dataclass(frozen=True)
class Loss:
    """A robust loss rho(s) on s = |r|^2 of ONE residual (all its rows) with scale a > 0 (the reference has none; the table:
    include/mini_opt_hip.h).  Built by Huber / SoftL1 / Cauchy / Tukey below; the solver minimises 0.5 sum_b rho_b(|r_b|^2)."""
    kind: int
    scale: float


def Huber(a: float) -> Loss:
    return Loss(L.MO_LOSS_HUBER, float(a))


def SoftL1(a: float) -> Loss:
    return Loss(L.MO_LOSS_SOFT_L1, float(a))


def Cauchy(a: float) -> Loss:
    return Loss(L.MO_LOSS_CAUCHY, float(a))


def Tukey(a: float) -> Loss:
    return Loss(L.MO_LOSS_TUKEY, float(a))


@dataclass
class Residual:
    """mini_opt::Residual as MakeResidual<R, P>(index, functor) builds it (residual.hpp:28-143): `fn(params [B, P], want_J) ->
    (r [B, R], J [B, R, P] | None)` sees only the residual's own parameters, picked out of the full vector by `index`.
    loss: a robust Loss on this residual as a cost (None: the plain 0.5 |r|^2); needs ConstrainedNonlinearLeastSquares(residual_blocks=True)."""
    index: Sequence[int]
    fn: ResidualFn
    rows: int
    loss: Optional[Loss] = None

    def Dimension(self) -> int:
        return self.rows

    def QuadraticError(self, params: torch.Tensor) -> torch.Tensor:
        r, _ = self.fn(params[:, list(self.index)], False)
        return 0.5 * (r * r).sum(dim=1)


def MakeResidual(index: Sequence[int], fn: ResidualFn, rows: int, loss: Optional[Loss] = None) -> Residual:
    return Residual(tuple(int(i) for i in index), fn, int(rows), loss)


def stack_residuals(residuals: Sequence[Residual], n: int) -> ResidualFn:
    """The dense stack of a list of Residuals: values concatenated, every residual's Jacobian columns scattered to its index list
    (UpdateJacobian's J_out.col(index[l]) = J.col(l), residual.hpp:230-250; summing J^T J over residuals, residual.hpp:206-224, is the
    J^T J of the stacked rows)."""
    def fn(x, want_J):
        rs, Js = [], []
        for res in residuals:
            idx = torch.as_tensor(list(res.index), dtype=torch.long, device=x.device)
            r, Jl = res.fn(x.index_select(1, idx), want_J)
            rs.append(r)
            if want_J:
                J = torch.zeros(x.shape[0], res.rows, n, dtype=x.dtype, device=x.device)
                J.index_copy_(2, idx, Jl)
                Js.append(J)
        return torch.cat(rs, dim=1), (torch.cat(Js, dim=1) if want_J else None)
    return fn


@dataclass
class Problem:
    """mini_opt::Problem (nonlinear.hpp:33-52) for a batch of independent problems sharing one structure."""
    dimension: int
    cost: ResidualFn
    cost_rows: int                                  # m_r: stacked rows of all cost residuals
    equality: Optional[ResidualFn] = None
    equality_rows: int = 0                          # k
    inequality_constraints: Sequence[Tuple[int, float, float]] = field(default_factory=list)  # (variable, a, b): a x + b >= 0
    cost_residuals: Optional[Sequence[Residual]] = None        # the Residual lists of FromResiduals (Problem::costs / equality_constraints):
    equality_residuals: Optional[Sequence[Residual]] = None    # what ConstrainedNonlinearLeastSquares(residual_blocks=True) evaluates

    @staticmethod
    def FromResiduals(dimension: int, costs: Sequence[Residual], equality_constraints: Sequence[Residual] = (),
                      inequality_constraints: Sequence[Tuple[int, float, float]] = ()) -> "Problem":
        """The reference's own shape: Problem{costs, inequality_constraints, equality_constraints, dimension} of Residuals."""
        k = sum(r.rows for r in equality_constraints)
        return Problem(dimension, stack_residuals(costs, dimension), sum(r.rows for r in costs),
                       stack_residuals(equality_constraints, dimension) if k else None, k, list(inequality_constraints),
                       list(costs), list(equality_constraints))


@dataclass
class NLSSolverOutputs:
    """NLSSolverOutputs (structs.hpp:332-347), one row per problem."""
    termination_state: torch.Tensor  # [B] int32
    num_iterations: torch.Tensor     # [B] int32
    iterations: torch.Tensor         # [B, max_iterations, 12 + 3 (max_line_search_iterations + 1)] NLSIteration records
    status: torch.Tensor             # [B] int32 QP status of a problem that ended with QP_FAILURE
    qp_iterations: Optional[torch.Tensor] = None   # [max_iterations, B, max_qp_iterations, 14] QPInteriorPointIteration records (on request)
    qp_lagrange: Optional[torch.Tensor] = None     # [max_iterations, B, 2] {min, l_infinity} of each QP's multipliers (k > 0, on request)
    qp_eigenvalues: Optional[torch.Tensor] = None  # [max_iterations, B, 3] QPEigenvalues {min, max, abs_min} (Params.log_qp_eigenvalues)
    null_space_path: bool = False                  # equality-only problems: the QP of every iteration is QPNullSpaceSolver's

    def NumQPIterations(self) -> torch.Tensor:
        it = torch.nan_to_num(self.iterations[:, :, 10], nan=0.0)
        return it.sum(dim=1).to(torch.int64)

    def NumLineSearchSteps(self) -> torch.Tensor:
        return torch.nan_to_num(self.iterations[:, :, 8], nan=0.0).sum(dim=1).to(torch.int64)

    def NumFailedLineSearches(self) -> torch.Tensor:
        r = self.iterations[:, :, 7]
        return ((r == STEP_MAX_ITERATIONS) | (r == STEP_POSITIVE_DERIVATIVE)).sum(dim=1)


class _Plan:
    def __init__(self, n, k, m, m_r, dtype, device, batch):
        desc = L.PlanDesc(n, k, m, m_r, _DT[dtype], device.index or 0, L.EXTRA_PLAN_FLAGS, 0, batch)
        self.h = C.c_void_p()
        L.check(L.lib().mo_plan_create(C.byref(desc), C.byref(self.h)))

    def __del__(self):
        try:
            L.lib().mo_plan_destroy(self.h)
        except Exception:
            pass


class ConstrainedNonlinearLeastSquares:
    """Batched mirror of mini_opt::ConstrainedNonlinearLeastSquares (nonlinear.hpp:127-230)."""

    def __init__(self, problem: Problem, batch: int, device=None, dtype=torch.float64, retraction=None, residual_blocks: bool = False):
        """retraction: None = x + alpha dx; WRAP_PI = the built-in angle wrap; or a callable (x [B, n], dx [B, n], alpha [B]) ->
        candidate [B, n] on torch tensors -- the reference's custom Retraction (nonlinear.hpp:127, nonlinear.cc:160-168).
        residual_blocks: for a Problem.FromResiduals, hand every residual's local Jacobian to the library as a packed block
        (mo_nls_solve_blocks: UpdateHessian / UpdateJacobian on device) instead of scattering it into a dense stack."""
        if problem is None:
            raise L.MiniOptError(-1, "Must have a valid problem")          # F_ASSERT nonlinear.cc:78
        if dtype != torch.float64:
            raise L.MiniOptError(-3, "mo_nls_solve needs fp64")
        self.p_ = problem
        self.batch = int(batch)
        dev = torch.device(device if device is not None else "cuda:0")
        n, k, m, m_r = problem.dimension, problem.equality_rows, len(problem.inequality_constraints), problem.cost_rows
        self.n, self.k, self.m, self.m_r = n, k, m, m_r
        self._plan = _Plan(n, k, m, m_r, dtype, dev, self.batch)
        z = lambda *shape, dt=dtype: torch.zeros(*shape, dtype=dt, device=dev)
        B = self.batch
        self.variables_ = z(B, n)
        self.candidate_vars_ = z(B, n)
        self.residual_blocks = bool(residual_blocks)
        self._cost_layout = self._eq_layout = self._cost_loss = None
        if any(res.loss is not None for res in (problem.equality_residuals or ())):
            raise L.MiniOptError(-1, "a loss on an equality residual: equality residuals take no loss")
        has_loss = any(res.loss is not None for res in (problem.cost_residuals or ()))
        if has_loss and not self.residual_blocks:
            raise L.MiniOptError(-1, "a cost residual has a loss: robust losses need residual_blocks=True")
        if self.residual_blocks:
            if problem.cost_residuals is None or (k and problem.equality_residuals is None):
                raise L.MiniOptError(-1, "residual_blocks needs a Problem built by Problem.FromResiduals")
            from .qp import create_layout
            self._cost_layout = create_layout(self._plan.h, [(res.index, res.rows) for res in problem.cost_residuals])
            self._eq_layout = create_layout(self._plan.h, [(res.index, res.rows) for res in problem.equality_residuals]) if k else None
            if has_loss:   # with no loss anywhere no table is built: the solver makes the calls it made before losses existed
                from .qp import create_loss
                self._cost_loss = create_loss(self._cost_layout, [(res.loss.kind, res.loss.scale) if res.loss is not None
                                                                  else (L.MO_LOSS_TRIVIAL, 1.0) for res in problem.cost_residuals])
            self._vals = int(L.lib().mo_residual_layout_values(self._cost_layout))
            self._vals_eq = int(L.lib().mo_residual_layout_values(self._eq_layout)) if k else 0
            self.J, self.r, self.r_cand = z(B, self._vals), z(B, m_r), z(B, m_r)            # J: packed blocks
            self.J_eq, self.r_eq, self.r_eq_cand = (z(B, self._vals_eq), z(B, k), z(B, k)) if k else (None, None, None)
        else:
            self.J, self.r, self.r_cand = z(B, m_r, n), z(B, m_r), z(B, m_r)
            self.J_eq, self.r_eq, self.r_eq_cand = (z(B, n, k), z(B, k), z(B, k)) if k else (None, None, None)   # J_eq: k x n col-major
        if m:
            self.cons_var = torch.tensor([[c[0] for c in problem.inequality_constraints]], dtype=torch.int32, device=dev)
            self.cons_a = torch.tensor([[c[1] for c in problem.inequality_constraints]], dtype=dtype, device=dev)
            self.cons_b = torch.tensor([[c[2] for c in problem.inequality_constraints]], dtype=dtype, device=dev)
        else:
            self.cons_var = self.cons_a = self.cons_b = None
        self.retraction_ = retraction
        self._retract_code = (L.MO_RETRACT_EUCLIDEAN if retraction is None else L.MO_RETRACT_WRAP_PI if retraction == WRAP_PI
                              else L.MO_RETRACT_CALLBACK)
        self.step_, self.step_alpha_ = (z(B, n), z(B)) if self._retract_code == L.MO_RETRACT_CALLBACK else (None, None)
        self.user_exit_callback_ = None
        self.user_exit_ = None
        self._outputs_view = None

    def SetUserExitCallback(self, callback) -> None:
        """nonlinear.hpp:157: callback(iteration index, NLSSolverOutputs view of the records so far) -> bool, or a bool tensor [B]
        (False = stop that problem).  A stopped problem ends with USER_CALLBACK unless the iteration terminated it anyway."""
        self.user_exit_callback_ = callback
        self.user_exit_ = torch.zeros(self.batch, dtype=torch.int32, device=self.variables_.device) if callback is not None else None

    # ---- callbacks: enqueue the user's residual evaluation on the stream the library works on
    def _eval(self, user, what, stream):
        try:
            if what == L.MO_NLS_EVAL_RETRACT:                  # the caller's Retraction, nonlinear.cc:160-168
                self.candidate_vars_.copy_(self.retraction_(self.variables_, self.step_, self.step_alpha_))
                return 0
            if what == L.MO_NLS_EVAL_ITERATION_DONE:           # SetUserExitCallback, nonlinear.cc:142-149
                self._iter_done += 1
                proceed = self.user_exit_callback_(self._iter_done - 1, self._outputs_view)
                if isinstance(proceed, torch.Tensor):
                    self.user_exit_.copy_((~proceed.to(torch.bool)).to(torch.int32))
                else:
                    self.user_exit_.fill_(0 if proceed else 1)
                return 0
            lin = what == L.MO_NLS_EVAL_LINEARIZE
            x = self.variables_ if lin else self.candidate_vars_
            r_buf = self.r if lin else self.r_cand
            if self.residual_blocks and lin:   # every residual's local J straight into its packed block: no dense scatter
                self._eval_blocks(x, self.p_.cost_residuals, self.r, self.J)
                if self.k:
                    self._eval_blocks(x, self.p_.equality_residuals, self.r_eq, self.J_eq)
                return 0
            if isinstance(self.p_.cost, DeviceFamily):          # a HIP kernel writes the solver's buffers directly
                self.p_.cost.eval_into(self._plan, x, r_buf, self.J if lin else None, self.n, True)
            else:
                r, J = self.p_.cost(x, lin)
                r_buf.copy_(r)
                if lin:
                    self.J.copy_(J)
            if self.k:
                req_buf = self.r_eq if lin else self.r_eq_cand
                if isinstance(self.p_.equality, DeviceFamily):
                    self.p_.equality.eval_into(self._plan, x, req_buf, self.J_eq if lin else None, self.n, False)  # k x n col-major
                else:
                    r_eq, J_eq = self.p_.equality(x, lin)
                    req_buf.copy_(r_eq)
                    if lin:
                        self.J_eq.copy_(J_eq.transpose(1, 2))
            return 0
        except Exception as e:  # an exception must not unwind through the C frames
            self._callback_error = e
            return 1

    @staticmethod
    def _eval_blocks(x, residuals, r_buf, J_buf):
        B, row, off = int(x.shape[0]), 0, 0
        for res in residuals:
            R, P = res.rows, len(res.index)
            r, Jl = res.fn(x[:, list(res.index)], True)
            r_buf[:, row:row + R].copy_(r)
            J_buf[:, off:off + R * P].view(B, P, R).copy_(Jl.transpose(1, 2))   # column-major R x P
            row += R
            off += R * P

    def __del__(self):
        try:
            if self._cost_loss is not None:
                L.lib().mo_residual_loss_destroy(self._cost_loss)
            for h in (self._cost_layout, self._eq_layout):
                if h is not None:
                    L.lib().mo_residual_layout_destroy(h)
        except Exception:
            pass

    def _problem_struct(self) -> L.NlsProblem:
        n, k, m, m_r = self.n, self.k, self.m, self.m_r
        p = L.NlsProblem()
        p.vars, p.vars_stride = _ptr(self.variables_), n
        p.candidate, p.candidate_stride = _ptr(self.candidate_vars_), n
        p.J, p.J_stride, p.J_ld, p.J_layout = _ptr(self.J), m_r * n, n, L.MO_ROW_MAJOR
        p.r, p.r_stride = _ptr(self.r), m_r
        p.r_cand, p.r_cand_stride = _ptr(self.r_cand), m_r
        if self.residual_blocks:
            p.J_stride = self._vals
        if k:
            p.J_eq, p.J_eq_stride, p.J_eq_ld = _ptr(self.J_eq), (self._vals_eq if self.residual_blocks else n * k), k
            p.r_eq, p.r_eq_stride = _ptr(self.r_eq), k
            p.r_eq_cand, p.r_eq_cand_stride = _ptr(self.r_eq_cand), k
        if m:
            p.cons_var, p.cons_a, p.cons_b, p.cons_stride = _ptr(self.cons_var), _ptr(self.cons_a), _ptr(self.cons_b), 0
        if self.step_ is not None:
            p.step, p.step_stride, p.step_alpha = _ptr(self.step_), n, _ptr(self.step_alpha_)
        if self.user_exit_ is not None:
            p.user_exit = _ptr(self.user_exit_)
        return p

    def Solve(self, params: Params, variables: torch.Tensor, record_qp_iterations: bool = False) -> NLSSolverOutputs:
        """nonlinear.cc:75-158 for every problem of the batch.  record_qp_iterations keeps every QP's QPInteriorPointIteration records
        (NLSIteration::qp_outputs) for mini_opt_amd.serialization."""
        if tuple(variables.shape) != (self.batch, self.n):
            raise L.MiniOptError(-2, f"variables must be [{self.batch}, {self.n}]")
        self.variables_.copy_(variables)
        dev = self.variables_.device
        B = self.batch
        rec = L.MO_NLS_ITER_HEADER + 3 * (params.max_line_search_iterations + 1)
        term = torch.zeros(B, dtype=torch.int32, device=dev)
        nit = torch.zeros(B, dtype=torch.int32, device=dev)
        status = torch.zeros(B, dtype=torch.int32, device=dev)
        its = torch.full((B, max(params.max_iterations, 1), rec), float("nan"), dtype=torch.float64, device=dev)
        sp = params.as_struct(self._retract_code)
        prob = self._problem_struct()
        qp_its = qp_lag = None
        if record_qp_iterations:
            qp_its = torch.full((max(params.max_iterations, 1), B, max(params.max_qp_iterations, 1), L.MO_ITER_RECORD), float("nan"),
                                dtype=torch.float64, device=dev)
            prob.qp_iterations = _ptr(qp_its)
            if self.k:
                qp_lag = torch.full((max(params.max_iterations, 1), B, 2), float("nan"), dtype=torch.float64, device=dev)
                prob.qp_lagrange = _ptr(qp_lag)
        qp_eig = None
        if params.log_qp_eigenvalues:   # NLSIteration::qp_eigenvalues (structs.hpp:267-310), NaN where a problem never ran the iteration
            qp_eig = torch.full((max(params.max_iterations, 1), B, 3), float("nan"), dtype=torch.float64, device=dev)
            prob.qp_eigenvalues = _ptr(qp_eig)
        self._callback_error = None
        self._iter_done = 0
        null_path = bool(L.lib().mo_plan_nls_uses_nullspace(self._plan.h))   # the C side's own predicate (shape AND kernel capacity)
        self._outputs_view = NLSSolverOutputs(term, nit, its, status, qp_its, qp_lag, qp_eig, null_path)
        cb = L.NLS_EVAL_FN(self._eval)
        if self._cost_loss is not None:
            rc = L.lib().mo_nls_solve_blocks_robust(self._plan.h, C.byref(prob), self._cost_layout, self._cost_loss, self._eq_layout, B,
                                                    C.byref(sp), cb, None, _ptr(term), _ptr(nit), _ptr(its), _ptr(status), _stream())
        elif self.residual_blocks:
            rc = L.lib().mo_nls_solve_blocks(self._plan.h, C.byref(prob), self._cost_layout, self._eq_layout, B, C.byref(sp), cb, None,
                                             _ptr(term), _ptr(nit), _ptr(its), _ptr(status), _stream())
        else:
            rc = L.lib().mo_nls_solve(self._plan.h, C.byref(prob), B, C.byref(sp), cb, None, _ptr(term), _ptr(nit), _ptr(its),
                                      _ptr(status), _stream())
        if self._callback_error is not None:
            raise self._callback_error
        L.check(rc)
        return self._outputs_view

    def variables(self) -> torch.Tensor:
        return self.variables_

    def EvaluateNonlinearErrors(self, vars_: torch.Tensor) -> torch.Tensor:
        """nonlinear.cc:279-293: [B, 2] = {f, equality}; with losses f is the robust cost 0.5 sum_b rho_b(|r_b|^2)."""
        r, _ = self.p_.cost(vars_, False)
        r_eq = self.p_.equality(vars_, False)[0] if self.k else None
        out = nonlinear_errors(self._plan, r.contiguous(), None if r_eq is None else r_eq.contiguous())
        if self._cost_loss is not None:
            out[:, 0] = self._loss_eval(r.contiguous(), want_weights=False)[1]
        return out

    def _loss_eval(self, r: torch.Tensor, want_weights: bool):
        B = int(r.shape[0])
        w = torch.empty(B, self.m_r, dtype=r.dtype, device=r.device) if want_weights else None
        f = torch.empty(B, dtype=r.dtype, device=r.device)
        L.check(L.lib().mo_residual_loss_eval(self._plan.h, self._cost_layout, self._cost_loss, _ptr(r), self.m_r, B, _ptr(w), self.m_r,
                                              _ptr(f), _stream()))
        return w, f

    def LossWeights(self) -> torch.Tensor:
        """[B, m_r]: the weight rho_b'(|r_b|^2) of every stacked cost row at the current variables (1 everywhere without losses): small
        weights mark the residuals the fit treats as outliers."""
        r, _ = self.p_.cost(self.variables_, False)
        if self._cost_loss is None:
            return torch.ones_like(r)
        return self._loss_eval(r.contiguous(), want_weights=True)[0]

    def Covariance(self, select=None, scale=None):
        """The covariance of the fitted parameters at the current variables(): (cov [B, q, q], status [B]), mo_qp_covariance on the
        problem re-linearised there with lambda = 0 (the damping is a device of the algorithm, not part of the model):
            C = scale Z (Z^T G Z)^-1 Z^T,   G = sum_b w_b J_b^T J_b,   Z a basis of null(J_eq)
        -- dense input through mo_linearize, residual blocks through mo_linearize_blocks, losses through mo_linearize_blocks_robust
        (w_b = rho_b', the Gauss-Newton form without the Triggs term), the equality Jacobian through mo_jacobian_blocks or the dense J_eq.
        Inequality constraints are not part of it: model an active bound that is to be pinned as an equality residual.
        select: the variables wanted (None: all).  scale: None, a [B] tensor, or "residual" = 2 f / (m_r - n + k) with f the (robust) cost
        at the solution, the usual estimate of the residual variance; raises when m_r - n + k <= 0.
        status: MO_STATUS_OK, NOT_POSITIVE_DEFINITE (the reduced Hessian has a pivot <= 0), NONFINITE; cov of a failed problem is NaN."""
        lib = L.lib()
        B, n, k, m_r = self.batch, self.n, self.k, self.m_r
        dev, dt = self.variables_.device, self.variables_.dtype
        if isinstance(scale, str):
            if scale != "residual":
                raise ValueError(f"scale = {scale!r}: expected None, a tensor [B] or \"residual\"")
            if m_r - n + k <= 0:
                raise ValueError(f"scale = \"residual\" needs m_r - n + k > 0 degrees of freedom (m_r = {m_r}, n = {n}, k = {k})")
        self._callback_error = None
        if self._eval(None, L.MO_NLS_EVAL_LINEARIZE, None):          # J, r (and J_eq) at variables()
            raise self._callback_error
        G = torch.empty(B, n, n, dtype=dt, device=dev)
        c = torch.empty(B, n, dtype=dt, device=dev)
        f = torch.empty(B, dtype=dt, device=dev)
        A = self.J_eq
        if self.residual_blocks:
            if self._cost_loss is not None:
                w = torch.empty(B, m_r, dtype=dt, device=dev)
                L.check(lib.mo_linearize_blocks_robust(self._plan.h, self._cost_layout, _ptr(self.J), self._vals, _ptr(self.r), m_r, 0.0, None, 0,
                                                       B, _ptr(G), n * n, n, _ptr(c), n, _ptr(f), self._cost_loss, _ptr(w), m_r, _stream()))
            else:
                L.check(lib.mo_linearize_blocks(self._plan.h, self._cost_layout, _ptr(self.J), self._vals, _ptr(self.r), m_r, 0.0, None, 0, B,
                                                _ptr(G), n * n, n, _ptr(c), n, _ptr(f), _stream()))
            if k:
                A = torch.empty(B, n, k, dtype=dt, device=dev)
                s = torch.empty(B, dtype=dt, device=dev)
                L.check(lib.mo_jacobian_blocks(self._plan.h, self._eq_layout, _ptr(self.J_eq), self._vals_eq, _ptr(self.r_eq), k, B, _ptr(A),
                                               k * n, k, L.MO_COL_MAJOR, _ptr(s), _stream()))
        else:
            lin = L.Problem()
            lin.J, lin.J_stride, lin.J_ld, lin.J_layout = _ptr(self.J), m_r * n, n, L.MO_ROW_MAJOR
            lin.r, lin.r_stride, lin.lam = _ptr(self.r), m_r, 0.0
            L.check(lib.mo_linearize(self._plan.h, C.byref(lin), B, _ptr(G), n * n, n, _ptr(c), n, _ptr(f), _stream()))
        scale_t = None
        if isinstance(scale, str):
            scale_t = f * (2.0 / (m_r - n + k))
        elif scale is not None:
            scale_t = scale
            if not isinstance(scale_t, torch.Tensor) or tuple(scale_t.shape) != (B,) or scale_t.dtype != dt or scale_t.device != dev:
                raise ValueError(f"scale: expected None, \"residual\" or a [{B}] {dt} tensor on {dev}")
            scale_t = scale_t.contiguous()
        sel_t, q = None, n
        if select is not None:
            sel_t = torch.as_tensor(select).to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
            q = int(sel_t.numel())
        prob = L.Problem()
        prob.G, prob.G_stride, prob.G_ld = _ptr(G), n * n, n
        if k:
            prob.A_eq, prob.A_stride, prob.A_ld = _ptr(A), n * k, k
        cov = torch.empty(B, q, q, dtype=dt, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        L.check(lib.mo_qp_covariance(self._plan.h, C.byref(prob), B, _ptr(sel_t), q, _ptr(scale_t), 1, _ptr(cov), q * q, q, None, 0,
                                     _ptr(status), _stream()))
        return cov, status


# ---- the static pieces, usable on their own ----------------------------------------------------------------------
def nonlinear_errors(plan: _Plan, r: torch.Tensor, r_eq: Optional[torch.Tensor]) -> torch.Tensor:
    B = int(r.shape[0])
    out = torch.empty(B, 2, dtype=r.dtype, device=r.device)
    L.check(L.lib().mo_nonlinear_errors(plan.h, _ptr(r), int(r.shape[1]), _ptr(r_eq), 0 if r_eq is None else int(r_eq.shape[1]),
                                        B, _ptr(out), _stream()))
    return out


def fill_qp(problem: BatchedQP, x: torch.Tensor):
    """LinearizeAndFillQP (nonlinear.cc:170-214) for dense stacks: `problem` carries (J, r, lam), the equality stack as
    (A_eq, b_eq) and the UNSHIFTED constraints.  Returns (G, c, shifted cons_b, errors [B, 2], status [B])."""
    ref = problem.J
    B, n, m = int(ref.shape[0]), problem.n, problem.m
    plan = _Plan(n, problem.k, m, problem.m_r, ref.dtype, ref.device, B)
    G = torch.empty(B, n, n, dtype=ref.dtype, device=ref.device)
    c = torch.empty(B, n, dtype=ref.dtype, device=ref.device)
    cb = torch.empty(B, m, dtype=ref.dtype, device=ref.device)
    err = torch.empty(B, 2, dtype=ref.dtype, device=ref.device)
    status = torch.empty(B, dtype=torch.int32, device=ref.device)
    prob = problem.as_struct()
    L.check(L.lib().mo_fill_qp(plan.h, C.byref(prob), B, _ptr(x), n, _ptr(G), n * n, n, _ptr(c), n, _ptr(cb), m, _ptr(err),
                               _ptr(status), _stream()))
    return G, c, cb, err, status


def qp_cost_derivative(problem: BatchedQP, dx: torch.Tensor):
    """ComputeQPCostDerivative (nonlinear.cc:452-483): ([B, 2] = {d_f, d_equality}, dx^T G dx [B])."""
    ref = problem._any()
    B, n = int(ref.shape[0]), problem.n
    plan = _Plan(n, problem.k, 0, problem.m_r, ref.dtype, ref.device, B)
    out = torch.empty(B, 2, dtype=ref.dtype, device=ref.device)
    quad = torch.empty(B, dtype=ref.dtype, device=ref.device)
    q = BatchedQP(n=n, k=problem.k, J=problem.J, r=problem.r, lam=problem.lam, lam_vec=problem.lam_vec, G=problem.G, c=problem.c,
                  A_eq=problem.A_eq, b_eq=problem.b_eq, J_layout=problem.J_layout, J_rows=problem.J_rows)
    prob = q.as_struct()
    L.check(L.lib().mo_qp_cost_derivative(plan.h, C.byref(prob), B, _ptr(dx), n, _ptr(out), _ptr(quad), _stream()))
    return out, quad
