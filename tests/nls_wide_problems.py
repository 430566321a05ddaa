"""Problem families for the SQP outer loop at any number of variables n, each as a numpy residual function (oracle side) and a torch
one on batches (device side), with seeded starts.  tests/test_gpu_nls_wide.py runs them on both sides of n = 32 -- the size at which
mo_nls_solve changes from one thread per problem to one wavefront per problem -- and tests/test_nls_wide_oracle_cpu.py checks with the
oracle alone that every case reaches the branch of the outer loop it is there for and that its starts are decided clear of every threshold.
These are fixtures (problem definitions), not product code."""
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional, Sequence, Tuple

import numpy as np

SQRT_B = 10.0


# ---- chained Rosenbrock (nonlinear_test.cc:502-521 for any n): rows 2i = 1 - x_i, 2i + 1 = sqrt(b) (x_{i+1} - x_i^2); also NLS.ROSENBROCK
def rosenbrock_np(n):
    i = np.arange(n - 1)

    def fn(x, want_J):
        x = np.asarray(x, float)
        r = np.empty(2 * (n - 1))
        r[0::2] = 1.0 - x[:-1]
        r[1::2] = SQRT_B * (x[1:] - x[:-1] * x[:-1])
        J = None
        if want_J:
            J = np.zeros((2 * (n - 1), n))
            J[2 * i, i] = -1.0
            J[2 * i + 1, i] = -2.0 * x[:-1] * SQRT_B
            J[2 * i + 1, i + 1] = SQRT_B
        return r, J
    return fn


def rosenbrock_torch(n):
    def fn(x, want_J):
        import torch
        B = x.shape[0]
        i = torch.arange(n - 1, device=x.device)
        r = torch.empty(B, 2 * (n - 1), dtype=x.dtype, device=x.device)
        r[:, 0::2] = 1.0 - x[:, :-1]
        r[:, 1::2] = SQRT_B * (x[:, 1:] - x[:, :-1] * x[:, :-1])
        J = None
        if want_J:
            J = torch.zeros(B, 2 * (n - 1), n, dtype=x.dtype, device=x.device)
            J[:, 2 * i, i] = -1.0
            J[:, 2 * i + 1, i] = -2.0 * x[:, :-1] * SQRT_B
            J[:, 2 * i + 1, i + 1] = SQRT_B
        return r, J
    return fn


def rosenbrock_residual_blocks(n):
    """The same rows as Residuals on their own parameters: blocks (i,) and (i, i + 1) for every i < n - 1."""
    import torch
    from mini_opt_amd import nls as NLS

    def r0(x, want_J):
        return (1.0 - x[:, 0]).unsqueeze(1), (-torch.ones(x.shape[0], 1, 1, dtype=x.dtype, device=x.device) if want_J else None)

    def r1(x, want_J):
        r = (SQRT_B * (x[:, 1] - x[:, 0] * x[:, 0])).unsqueeze(1)
        J = torch.stack([-2.0 * x[:, 0] * SQRT_B, torch.full_like(x[:, 0], SQRT_B)], dim=1).unsqueeze(1) if want_J else None
        return r, J
    out = []
    for i in range(n - 1):
        out.append(NLS.MakeResidual((i,), r0, 1))
        out.append(NLS.MakeResidual((i, i + 1), r1, 1))
    return out


def tight_box(n, nvars=32):
    """-1 <= x_i <= 1.5 on the first min(n, nvars) variables as (variable, a, b) with a x + b >= 0: m = 64 from n = 32 on."""
    out = []
    for i in range(min(n, nvars)):
        out.append((i, 1.0, 1.0))
        out.append((i, -1.0, 1.5))
    return out


# ---- "pole": r = [1 / (x_i^2 + 0.01) - s, 0.5 x_i x_{i+1}], rows 2n - 1.  Steep and far from quadratic along a step: the polynomial line
# search needs its cubic step (a third and a fourth trial point)
def pole_np(n, s):
    i = np.arange(n - 1)

    def fn(x, want_J):
        x = np.asarray(x, float)
        d = x * x + 0.01
        r = np.concatenate([1.0 / d - s, 0.5 * x[:-1] * x[1:]])
        J = None
        if want_J:
            J = np.zeros((2 * n - 1, n))
            J[np.arange(n), np.arange(n)] = -2.0 * x / (d * d)
            J[n + i, i] = 0.5 * x[1:]
            J[n + i, i + 1] = 0.5 * x[:-1]
        return r, J
    return fn


def pole_torch(n, s):
    def fn(x, want_J):
        import torch
        B = x.shape[0]
        d = x * x + 0.01
        r = torch.cat([1.0 / d - s, 0.5 * x[:, :-1] * x[:, 1:]], dim=1)
        J = None
        if want_J:
            i, j = torch.arange(n - 1, device=x.device), torch.arange(n, device=x.device)
            J = torch.zeros(B, 2 * n - 1, n, dtype=x.dtype, device=x.device)
            J[:, j, j] = -2.0 * x / (d * d)
            J[:, n + i, i] = 0.5 * x[:, 1:]
            J[:, n + i, i + 1] = 0.5 * x[:, :-1]
        return r, J
    return fn


# ---- r_i = log(x_i): the Gauss-Newton step x_i (1 - log x_i) is negative for x_i > e, so the first trial point has a NaN cost
def log_np(n):
    def fn(x, want_J):
        with np.errstate(all="ignore"):
            x = np.asarray(x, float)
            return np.log(x), (np.diag(1.0 / x) if want_J else None)
    return fn


def log_torch(n):
    def fn(x, want_J):
        import torch
        return torch.log(x), (torch.diag_embed(1.0 / x) if want_J else None)
    return fn


# ---- rank-deficient cost (rows x_0 - 1 and x_1 + x_2) with the equality x_0 x_1 = 2 and no inequalities: the null-space path, whose
# reduced Hessian is singular without damping for every n > 3
def deficient_np(n):
    def cost(x, want_J):
        J = None
        if want_J:
            J = np.zeros((2, n))
            J[0, 0] = J[1, 1] = J[1, 2] = 1.0
        return np.array([x[0] - 1.0, x[1] + x[2]]), J

    def eq(x, want_J):
        J = None
        if want_J:
            J = np.zeros((1, n))
            J[0, 0], J[0, 1] = x[1], x[0]
        return np.array([x[0] * x[1] - 2.0]), J
    return cost, eq


def deficient_torch(n):
    def cost(x, want_J):
        import torch
        J = None
        if want_J:
            J = torch.zeros(x.shape[0], 2, n, dtype=x.dtype, device=x.device)
            J[:, 0, 0] = J[:, 1, 1] = J[:, 1, 2] = 1.0
        return torch.stack([x[:, 0] - 1.0, x[:, 1] + x[:, 2]], dim=1), J

    def eq(x, want_J):
        import torch
        J = None
        if want_J:
            J = torch.zeros(x.shape[0], 1, n, dtype=x.dtype, device=x.device)
            J[:, 0, 0], J[:, 0, 1] = x[:, 1], x[:, 0]
        return (x[:, 0] * x[:, 1] - 2.0).unsqueeze(1), J
    return cost, eq


# ---- sphere cost h(x) = x with product-pair equalities x_{2q} x_{2q+1} = v_q (nonlinear_test.cc:722-743 for any n); on the device these
# are the families NLS.SPHERE and NLS.PRODUCT_PAIRS
PRODUCTS = (4.0, 9.0, 1.0, 2.25)


def sphere_np(n):
    def fn(x, want_J):
        return np.array(x, float), (np.eye(n) if want_J else None)
    return fn


def product_pairs_np(n, prods=PRODUCTS):
    k = len(prods)

    def fn(x, want_J):
        r = np.array([x[2 * q] * x[2 * q + 1] - prods[q] for q in range(k)])
        J = None
        if want_J:
            J = np.zeros((k, n))
            for q in range(k):
                J[q, 2 * q], J[q, 2 * q + 1] = x[2 * q + 1], x[2 * q]
        return r, J
    return fn


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
# Branches of the outer loop a case can claim.  Both sides log the same record per outer iteration (oracle: IterationLog, device:
# NLSIteration rows [state after the update, ..., step result at 7, number of trial points at 8]), so one function names the branches of both.
POLY_CUBIC = "polynomial search with a third trial point (cubic step)"
POLY_CUBIC_2 = "polynomial search with a fourth trial point (cubic step from two earlier trial points)"
ARMIJO_3 = "Armijo backtracking with a third trial point"
LS_MAX_ITERATIONS = "MO_LS_MAX_ITERATIONS"
LS_POSITIVE_DERIVATIVE = "MO_LS_POSITIVE_DERIVATIVE"
LS_NON_FINITE = "MO_LS_FAILURE_NON_FINITE_COST"
LS_INVALID_ALPHA = "MO_LS_FAILURE_INVALID_ALPHA"
RESTORE_THEN_SUCCESS = "ATTEMPTING_RESTORE_LM followed by a successful step"
TERM_MAX_LAMBDA = "MO_NLS_MAX_LAMBDA"
TERM_QP_INDEFINITE = "MO_NLS_QP_INDEFINITE"


def branches(polynomial: bool, termination: int, rows: Sequence[Tuple[int, int, int]]):
    """The set of branches one problem's run went through; rows = [(state after the update, step result, trial points)] per outer iteration."""
    out = set()
    for i, (state, result, nsteps) in enumerate(rows):
        if nsteps >= 3:
            out.add(POLY_CUBIC if polynomial else ARMIJO_3)
        if nsteps >= 4 and polynomial:
            out.add(POLY_CUBIC_2)
        for code, name in ((1, LS_MAX_ITERATIONS), (3, LS_POSITIVE_DERIVATIVE), (4, LS_NON_FINITE), (5, LS_INVALID_ALPHA)):
            if result == code:
                out.add(name)
        if state == 1 and i + 1 < len(rows) and rows[i + 1][1] == 0:
            out.add(RESTORE_THEN_SUCCESS)
    if termination == 4:
        out.add(TERM_MAX_LAMBDA)
    if termination == 5:
        out.add(TERM_QP_INDEFINITE)
    return out


def branches_of_oracle_run(case, termination, logs):
    return branches(case.polynomial, termination, [(lg.state, lg.step_result, len(lg.steps)) for lg in logs])


def branches_of_device_run(case, termination, num_iterations, records):
    return branches(case.polynomial, int(termination), [(int(r[0]), int(r[7]), int(r[8])) for r in records[:int(num_iterations)]])


@dataclass
class Case:
    name: str
    n: int
    cost_np: Callable
    cost_torch: Callable
    cost_rows: int
    params: Dict
    start: Callable                     # (rng, count, n) -> [count, n] starts
    seed: int
    count: int                          # never a multiple of four: the last workgroup of the wave path has idle waves
    claims: Tuple[str, ...] = ()        # the branches at least one start must go through
    constraints: Sequence[Tuple[int, float, float]] = field(default_factory=list)
    equality_np: Optional[Callable] = None
    equality_torch: Optional[Callable] = None
    equality_rows: int = 0

    @property
    def polynomial(self):
        return self.params.get("line_search_strategy", 1) == 1

    def guesses(self):
        return self.start(np.random.default_rng(self.seed), self.count, self.n)

    def oracle_problem(self):
        from oracle import nls_oracle as N
        return N.Problem(self.n, self.cost_np, equality=self.equality_np, inequality_constraints=list(self.constraints))

    def device_problem(self):
        from mini_opt_amd import nls as NLS
        return NLS.Problem(self.n, self.cost_torch, cost_rows=self.cost_rows, equality=self.equality_torch, equality_rows=self.equality_rows,
                           inequality_constraints=list(self.constraints))


def _around_one(lo, hi):
    return lambda rng, count, n: 1.0 + rng.uniform(lo, hi, (count, n))


def _uniform(lo, hi):
    return lambda rng, count, n: rng.uniform(lo, hi, (count, n))


CONTROL, FIRST_WAVE, WRAPPING = 24, 33, 72     # thread path; first size on the wave path (lanes 33 .. 63 idle); lane loops take a second trip
SIZES = (CONTROL, FIRST_WAVE, WRAPPING)

# max_iterations of the undamped cases (lambda_initial = 0, lambda falling after every success) is short on purpose.  Far from the optimum the
# Gauss-Newton iteration on these costs is chaotic: the rounding-level difference between two correct solves of the first, ill-conditioned
# QP (1e-13 relative in d_f) grows two- to threefold per outer iteration on the thread path and the wave path alike, and reached the 1e-6 of
# check_records after 20 iterations of Rosenbrock and 12 of the pole cost.  12 and 6 iterations keep two orders of magnitude below it; the
# damped and the boxed cases (lambda >= 0.01 or an interior-point QP that pins the variables) do not amplify and keep their length.
ROSENBROCK_POLY = dict(max_iterations=12, max_qp_iterations=1, max_line_search_iterations=4)
ROSENBROCK_ARMIJO = dict(max_iterations=12, max_qp_iterations=1, max_line_search_iterations=6, line_search_strategy=0, armijo_search_tau=0.5)
# no trial point beyond the first: MAX_ITERATIONS of the search, lambda x 10 in the restore state, MAX_LAMBDA.  max_lambda = 5 is no power of
# ten times lambda_failure_init, so `lambda > max_lambda` is never decided at equality
ROSENBROCK_LS0 = dict(max_iterations=20, max_qp_iterations=1, max_line_search_iterations=0, max_lambda=5.0)
TIGHT_BOX = dict(max_iterations=14, max_qp_iterations=1, max_line_search_iterations=3, max_lambda=5.0e3)
POLE = dict(max_iterations=6, max_qp_iterations=1, max_line_search_iterations=5, max_lambda=5.0e3)
LOG = dict(max_iterations=12, max_qp_iterations=1, max_line_search_iterations=4, max_lambda=5.0e3)

# Seeds were chosen with the oracle alone (tests/test_nls_wide_oracle_cpu.py states the two conditions): every start of a strict case is
# decided clear of every threshold, and the case goes through the branches it claims.
_RESTORE = (LS_POSITIVE_DERIVATIVE, RESTORE_THEN_SUCCESS, TERM_MAX_LAMBDA)
# n -> (seed, starts, claims).  At n = 72 none of 140 seeds gave all three in nine starts: the restore state followed by a success is
# claimed there by the "ls0" case
TIGHT_BOX_STARTS = {CONTROL: (25, 13, _RESTORE), FIRST_WAVE: (33, 13, _RESTORE), WRAPPING: (132, 9, (LS_POSITIVE_DERIVATIVE, TERM_MAX_LAMBDA))}
POLE_SEEDS = {CONTROL: 8, FIRST_WAVE: 3, WRAPPING: 7}


def rosenbrock_case(n, kind):
    params, claims = {"poly": (ROSENBROCK_POLY, ()), "armijo": (ROSENBROCK_ARMIJO, (ARMIJO_3,)),
                      "ls0": (ROSENBROCK_LS0, (LS_MAX_ITERATIONS, RESTORE_THEN_SUCCESS, TERM_MAX_LAMBDA))}[kind]
    return Case(f"rosenbrock {kind} n={n}", n, rosenbrock_np(n), rosenbrock_torch(n), 2 * (n - 1), params, _around_one(-1.5, 1.5), 3 + n, 13,
                claims=claims)


def wrap_pi_case(seed=3 + WRAPPING):
    """Chained Rosenbrock at n = 72 under the ModPi retraction: starts inside (-pi, pi), trial points x + alpha dx outside it."""
    case = rosenbrock_case(WRAPPING, "poly")
    case.name, case.seed = f"rosenbrock wrap-pi n={WRAPPING}", seed
    return case


def tight_box_case(n):
    seed, count, claims = TIGHT_BOX_STARTS[n]
    return Case(f"tight-box rosenbrock n={n}", n, rosenbrock_np(n), rosenbrock_torch(n), 2 * (n - 1), TIGHT_BOX, _around_one(-1.9, 0.4), seed, count,
                claims=claims, constraints=tight_box(n))


def pole_case(n, s=20.0):
    return Case(f"pole s={s} n={n}", n, pole_np(n, s), pole_torch(n, s), 2 * n - 1, POLE, _uniform(-2.0, 2.0), POLE_SEEDS[n], 13,
                claims=(POLY_CUBIC, POLY_CUBIC_2))


def log_case(n):
    return Case(f"log n={n}", n, log_np(n), log_torch(n), n, LOG, _uniform(0.5, 6.0), 5 + n, 13, claims=(LS_NON_FINITE,))


STRICT_KINDS = ("rosenbrock poly", "rosenbrock armijo", "rosenbrock ls0", "tight box", "pole", "log")


def strict_case(kind, n):
    """The unconstrained and box-only families: the device must reproduce the oracle's run of every start, decision by decision."""
    if kind.startswith("rosenbrock "):
        return rosenbrock_case(n, kind.split()[1])
    return {"tight box": tight_box_case, "pole": pole_case, "log": log_case}[kind](n)


# The equality-constrained families are not strict: oracle/margins.py classes their interior-point QPs as knife-edge and the null-space runs
# sit on Armijo margins near convergence (tests/test_gpu_nls.py::knife_edge_rule is the rule they are held to).
def deficient_case(n, damped):
    cost, eq = deficient_np(n)
    cost_t, eq_t = deficient_torch(n)
    params = (dict(max_iterations=8, max_qp_iterations=1, lambda_initial=0.01, min_lambda=1e-3) if damped
              else dict(max_iterations=5, max_qp_iterations=1))
    return Case(f"rank-deficient {'damped' if damped else 'undamped'} n={n}", n, cost, cost_t, 2, params, _uniform(1.0, 2.0), 7 + n, 5,
                claims=() if damped else (TERM_QP_INDEFINITE,), equality_np=eq, equality_torch=eq_t, equality_rows=1)


SPHERE = dict(max_iterations=25, relative_exit_tol=1e-6, absolute_first_derivative_tol=1e-6, lambda_initial=0.001, max_line_search_iterations=4)


def sphere_case(n, boxed):
    """boxed: -6 <= x_i <= 6 on the first eight variables (the interior-point path); otherwise m = 0, the null-space path.  The torch side
    is left to the device families NLS.SPHERE / NLS.PRODUCT_PAIRS (tests/test_gpu_nls_wide.py)."""
    cons = [c for i in range(8) for c in ((i, 1.0, 6.0), (i, -1.0, 6.0))] if boxed else []
    params = dict(SPHERE, max_qp_iterations=10 if boxed else 1)
    return Case(f"sphere with product pairs {'boxed' if boxed else 'null-space'} n={n}", n, sphere_np(n), None, n, params, _uniform(-5.0, 5.0),
                21 + n, 13, constraints=cons, equality_np=product_pairs_np(n), equality_torch=None, equality_rows=len(PRODUCTS))
