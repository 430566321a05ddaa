"""Robust loss functions for residual-block costs: the numpy reference of the tests (tests/test_robust_loss_cpu.py,
tests/test_gpu_robust_loss.py) and the problems both run.

The reference project has no loss functions, so the yardstick is the project's own oracle/nls_oracle.py, UNMODIFIED, on a WRAPPED cost:
  linearisation call (want_J=True)   (sqrt(w) r (+) e, sqrt(w) J (+) 0^T): the extra row has a zero Jacobian, so J^T J and J^T r are the IRLS
                                     model sum_b w_b J_b^T J_b, sum_b w_b J_b^T r_b, and e = sqrt(max(0, sum_b (rho_b - w_b s_b))) makes
                                     0.5 |.|^2 = 0.5 sum_b rho_b.  (rho_b >= w_b s_b: every loss is concave in s with rho(0) = 0.)
  cost call (want_J=False)           sqrt(rho_b / s_b) r_b (0 where s_b = 0): 0.5 |.|^2 = 0.5 sum_b rho_b.
rho and rho' follow the table of include/mini_opt_hip.h, in the textbook forms (the kernels use rearranged ones), for any numpy float type:
np.longdouble is the referee of the kernel tests.
"""
import math

import numpy as np

TRIVIAL, HUBER, SOFT_L1, CAUCHY, TUKEY = range(5)
KINDS = (TRIVIAL, HUBER, SOFT_L1, CAUCHY, TUKEY)
KIND_NAMES = {TRIVIAL: "trivial", HUBER: "huber", SOFT_L1: "soft_l1", CAUCHY: "cauchy", TUKEY: "tukey"}


def rho(kind, a, s, dtype=np.float64):
    """rho(s) for scale a, element-wise in `dtype`."""
    s = np.asarray(s, dtype=dtype)
    a = dtype(a)
    a2 = a * a
    one = dtype(1)
    with np.errstate(all="ignore"):
        if kind == TRIVIAL:
            return s.copy()
        if kind == HUBER:
            return np.where(s <= a2, s, 2 * a * np.sqrt(s) - a2)
        if kind == SOFT_L1:
            # 2 a^2 (sqrt(1 + t) - 1) = 2 s / (sqrt(1 + t) + 1): the same function without the cancellation at small t
            return 2 * s / (np.sqrt(one + s / a2) + one)
        if kind == CAUCHY:
            return a2 * np.log1p(s / a2)
        if kind == TUKEY:
            t = s / a2
            # (a^2 / 3)(1 - (1 - t)^3) = s (1 - t + t^2 / 3): the same polynomial without the cancellation at small t
            return np.where(s <= a2, s * (one - t + t * t / 3), a2 / 3)
    raise ValueError(kind)


def rho_prime(kind, a, s, dtype=np.float64):
    """rho'(s) for scale a, element-wise in `dtype`."""
    s = np.asarray(s, dtype=dtype)
    a = dtype(a)
    a2 = a * a
    one = dtype(1)
    with np.errstate(all="ignore"):
        if kind == TRIVIAL:
            return np.ones_like(s)
        if kind == HUBER:
            return np.where(s <= a2, one, a / np.sqrt(np.where(s <= a2, one, s)))
        if kind == SOFT_L1:
            return one / np.sqrt(one + s / a2)
        if kind == CAUCHY:
            return one / (one + s / a2)
        if kind == TUKEY:
            return np.where(s <= a2, ((a2 - s) / a2) ** 2, dtype(0))
    raise ValueError(kind)


def block_offsets(rows):
    return np.concatenate([[0], np.cumsum(rows)]).astype(int)


def loss_eval(rows, losses, r, dtype=np.longdouble):
    """(weights [B, sum rows], rho [B]) of mo_residual_loss_eval for r [B, sum rows], in `dtype` (exact products: r is promoted first).
    NaN in a block makes that block's weights and the problem's rho NaN."""
    r = np.asarray(r).astype(dtype)
    off = block_offsets(rows)
    w = np.empty_like(r)
    f = np.zeros(r.shape[0], dtype=dtype)
    absf = np.zeros(r.shape[0], dtype=dtype)
    for b, (kind, a) in enumerate(losses):
        rb = r[:, off[b]:off[b + 1]]
        s = (rb * rb).sum(axis=1)
        wb = rho_prime(kind, a, s, dtype)
        fb = rho(kind, a, s, dtype)
        wb = np.where(np.isnan(s), dtype(np.nan), wb)
        fb = np.where(np.isnan(s), dtype(np.nan), fb)
        w[:, off[b]:off[b + 1]] = wb[:, None]
        f += fb
        absf += np.abs(fb)
    return w, f / 2, absf / 2


def wrap_cost(cost, rows, losses):
    """The wrapped cost described above for a numpy ResidualFn of the oracle: rows = [R_b], losses = [(kind, a)] per block."""
    off = block_offsets(rows)

    def fn(x, want_J):
        r, J = cost(x, want_J)
        r = np.asarray(r, float)
        s = np.array([float(r[off[b]:off[b + 1]] @ r[off[b]:off[b + 1]]) for b in range(len(rows))])
        f = np.array([float(rho(k, a, s[b])) for b, (k, a) in enumerate(losses)])
        if want_J:
            w = np.array([float(rho_prime(k, a, s[b])) for b, (k, a) in enumerate(losses)])
            sw = np.sqrt(np.repeat(w, rows))
            e = math.sqrt(max(0.0, float(np.sum(f - w * s))))
            return np.concatenate([sw * r, [e]]), np.vstack([sw[:, None] * J, np.zeros((1, J.shape[1]))])
        with np.errstate(all="ignore"):
            g = np.where(s > 0, np.sqrt(f / np.where(s > 0, s, 1.0)), 0.0)
        return np.repeat(g, rows) * r, None
    return fn


# ---- the problems of the loop tests: numpy cost for the oracle, torch residual blocks for the device ------------------------------------
class Case:
    """One problem family: blocks = [(index, rows)], losses = [(kind, a)] per block, per-start data, the numpy cost of start p and the
    torch residual functions of the whole batch."""

    def __init__(self, name, n, blocks, losses, starts, cost_np, block_fns_torch, params=None, equality_np=None, eq_blocks=(),
                 eq_fns_torch=(), constraints=()):
        self.name, self.n, self.blocks, self.losses, self.starts = name, n, blocks, losses, np.asarray(starts, float)
        self.cost_np, self.block_fns_torch, self.params = cost_np, block_fns_torch, dict(params or {})
        self.equality_np, self.eq_blocks, self.eq_fns_torch, self.constraints = equality_np, list(eq_blocks), eq_fns_torch, list(constraints)
        self.rows = [R for _, R in blocks]

    def oracle_problem(self, p, robust=True):
        from oracle import nls_oracle as N
        cost = self.cost_np(p)
        if robust:
            cost = wrap_cost(cost, self.rows, self.losses)
        return N.Problem(self.n, cost, equality=self.equality_np, inequality_constraints=self.constraints)

    def device_problem(self, NLS, device, with_loss=True):
        """NLS.Problem.FromResiduals of torch residuals for the whole batch of starts."""
        mk = {HUBER: NLS.Huber, SOFT_L1: NLS.SoftL1, CAUCHY: NLS.Cauchy, TUKEY: NLS.Tukey} if with_loss else {}
        costs = []
        for (idx, R), (kind, a), fn in zip(self.blocks, self.losses, self.block_fns_torch(device)):
            if with_loss and kind != TRIVIAL:
                costs.append(NLS.MakeResidual(idx, fn, R, loss=mk[kind](a)))
            else:
                costs.append(NLS.MakeResidual(idx, fn, R))
        eqs = [NLS.MakeResidual(idx, fn, R) for (idx, R), fn in zip(self.eq_blocks, self.eq_fns_torch(device) if self.eq_blocks else [])]
        return NLS.Problem.FromResiduals(self.n, costs, eqs, self.constraints)


# -- the outlier fit: y = a exp(b t) at 12 points, 3 of them gross outliers; 12 blocks of 1 x 2; one data set per start
FIT_T = np.linspace(0.0, 2.0, 12)
FIT_START = (1.0, 0.0)


def fit_data(seed):
    """(y [12], inlier mask [12], true (a, b)) of data set `seed`."""
    rng = np.random.default_rng(1000 + seed)
    a, b = rng.uniform(1.0, 2.0), rng.uniform(-1.0, -0.3)
    y = a * np.exp(b * FIT_T) + rng.normal(0.0, 0.01, 12)
    out = rng.choice(12, 3, replace=False)
    y[out] += rng.choice([-1.0, 1.0], 3) * rng.uniform(1.0, 2.0, 3)
    mask = np.ones(12, bool)
    mask[out] = False
    return y, mask, (a, b)


def fit_cost_np(y, mask=None):
    t = FIT_T if mask is None else FIT_T[mask]
    yy = y if mask is None else y[mask]

    def fn(x, want_J):
        e = np.exp(x[1] * t)
        return x[0] * e - yy, (np.stack([e, x[0] * t * e], axis=1) if want_J else None)
    return fn


def fit_case(kind, seeds):
    scale = 1.0 if kind == TUKEY else 0.05
    ys = np.array([fit_data(s)[0] for s in seeds])

    def fns(device):
        import torch
        Y = torch.as_tensor(ys, dtype=torch.float64, device=device)

        def make(i):
            ti = float(FIT_T[i])

            def fn(x, want_J):
                e = torch.exp(x[:, 1] * ti)
                r = (x[:, 0] * e - Y[:, i]).unsqueeze(1)
                J = torch.stack([e, x[:, 0] * ti * e], dim=1).unsqueeze(1) if want_J else None
                return r, J
            return fn
        return [make(i) for i in range(12)]
    return Case(f"fit_{KIND_NAMES[kind]}", 2, [((0, 1), 1)] * 12, [(kind, scale)] * 12, [FIT_START] * len(seeds),
                lambda p: fit_cost_np(ys[p]), fns)


# -- Rosenbrock in n = 6 as 5 blocks of 2 x 2 on (i, i + 1): r = [1 - x_i, 10 (x_i+1 - x_i^2)]
def rosen_blocks_np(n):
    def fn(x, want_J):
        r = np.zeros(2 * (n - 1))
        J = np.zeros((2 * (n - 1), n)) if want_J else None
        for i in range(n - 1):
            r[2 * i], r[2 * i + 1] = 1.0 - x[i], 10.0 * (x[i + 1] - x[i] * x[i])
            if want_J:
                J[2 * i, i] = -1.0
                J[2 * i + 1, i], J[2 * i + 1, i + 1] = -20.0 * x[i], 10.0
        return r, J
    return fn


def rosen_block_torch(x, want_J):
    import torch
    r = torch.stack([1.0 - x[:, 0], 10.0 * (x[:, 1] - x[:, 0] * x[:, 0])], dim=1)
    J = None
    if want_J:
        J = torch.zeros(x.shape[0], 2, 2, dtype=x.dtype, device=x.device)
        J[:, 0, 0] = -1.0
        J[:, 1, 0] = -20.0 * x[:, 0]
        J[:, 1, 1] = 10.0
    return r, J


def rosen_starts(n, seeds):
    return [np.random.default_rng(2000 + s).uniform(-2.0, 3.0, n) for s in seeds]


def rosen_case(seeds, kind=HUBER, scale=1.0, n=6):
    """HUBER at a = 1: the starts have |r_b| of order 10 ... 100 (the loss is active), the solution has r = 0 (inactive)."""
    nb = n - 1
    return Case("rosenbrock_huber", n, [((i, i + 1), 2) for i in range(nb)], [(kind, scale)] * nb, rosen_starts(n, seeds),
                lambda p: rosen_blocks_np(n), lambda device: [rosen_block_torch] * nb, params=dict(max_iterations=30))


# -- the inequality-constrained Rosenbrock (x0 >= 1.2, x1 <= 0.5: the interior-point path), one 2 x 2 block, CAUCHY at a = 5
def rosen_con_case(seeds):
    starts = [np.random.default_rng(3000 + s).uniform(-3.0, 3.0, 2) + np.array([4.0, -3.0]) for s in seeds]
    return Case("rosenbrock_constrained_cauchy", 2, [((0, 1), 2)], [(CAUCHY, 5.0)], starts, lambda p: rosen_blocks_np(2),
                lambda device: [rosen_block_torch], params=dict(max_iterations=20, max_qp_iterations=10),
                constraints=[(0, 1.0, -1.2), (1, -1.0, 0.5)])


# -- the sphere with product equalities x0 x1 = 4, x2 x3 = 9 (the null-space path): cost r = x as 3 blocks of 2 x 2, SOFT_L1 at a = 2
def sphere_case(seeds):
    starts = [np.random.default_rng(4000 + s).uniform(-10.0, 10.0, 6) for s in seeds]

    def ident(x, want_J):
        import torch
        return x.clone(), (torch.eye(2, dtype=x.dtype, device=x.device).expand(x.shape[0], 2, 2).contiguous() if want_J else None)

    def product(target):
        def fn(x, want_J):
            import torch
            r = (x[:, 0] * x[:, 1] - target).unsqueeze(1)
            J = torch.stack([x[:, 1], x[:, 0]], dim=1).unsqueeze(1) if want_J else None
            return r, J
        return fn

    def eq_np(x, want_J):
        r = np.array([x[0] * x[1] - 4.0, x[2] * x[3] - 9.0])
        J = None
        if want_J:
            J = np.zeros((2, 6))
            J[0, 0], J[0, 1] = x[1], x[0]
            J[1, 2], J[1, 3] = x[3], x[2]
        return r, J
    return Case("sphere_soft_l1", 6, [((0, 1), 2), ((2, 3), 2), ((4, 5), 2)], [(SOFT_L1, 2.0)] * 3, starts,
                lambda p: (lambda x, want_J: (np.array(x, float), np.eye(6) if want_J else None)), lambda device: [ident] * 3,
                params=dict(max_iterations=60, max_qp_iterations=1, lambda_initial=0.001),
                equality_np=eq_np, eq_blocks=[((0, 1), 1), ((2, 3), 1)], eq_fns_torch=lambda device: [product(4.0), product(9.0)])


# The strict starts: seeds whose oracle run has every outer-loop decision margin >= 1e-6 and every inner-QP ratio >= 1 (the rule of
# tests/test_nls_wide_oracle_cpu.py).  tests/test_robust_loss_cpu.py checks the table; tests/test_gpu_robust_loss.py runs it with no start
# exempted.  Chosen by running that check over seeds 0 ... 59 (fit) / 0 ... 39 and dropping the seeds that fail it; the fit keeps one list
# for its four losses: the data sets whose plain fit ends more than 0.2 from the inlier parameters and every robust fit within 0.05.
FIT_SEEDS = [0, 4, 7, 8, 14, 15, 16, 18, 20, 23, 25, 26, 27, 28, 29, 31, 38, 41, 43, 48, 49, 52, 53, 55]
STRICT_SEEDS = {
    "fit_huber": FIT_SEEDS,
    "fit_soft_l1": FIT_SEEDS,
    "fit_cauchy": FIT_SEEDS,
    "fit_tukey": FIT_SEEDS,
    "rosenbrock_huber": [0, 2, 5, 6, 7, 8, 13, 14],
    "rosenbrock_constrained_cauchy": [0, 1, 2, 8, 9, 10, 11, 12],
    "sphere_soft_l1": [1, 3, 5, 10, 13, 15, 19, 20],
}


def strict_cases():
    return [fit_case(HUBER, STRICT_SEEDS["fit_huber"]), fit_case(SOFT_L1, STRICT_SEEDS["fit_soft_l1"]),
            fit_case(CAUCHY, STRICT_SEEDS["fit_cauchy"]), fit_case(TUKEY, STRICT_SEEDS["fit_tukey"]),
            rosen_case(STRICT_SEEDS["rosenbrock_huber"]), rosen_con_case(STRICT_SEEDS["rosenbrock_constrained_cauchy"]),
            sphere_case(STRICT_SEEDS["sphere_soft_l1"])]
