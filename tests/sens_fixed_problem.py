"""The fixed numpy barrier problem of the CPU formula tests (test_diff_cpu, test_tangent_cpu): no product code involved.  Not a test
module: nothing here asserts but the Newton iteration's own convergence."""
import numpy as np

from tests import diff_reference as R

N, K, M, MR = 8, 2, 5, 12
MU = 1e-3
LAM = 1e-3


def fixed_problem():
    rng = np.random.default_rng(20261016)
    J = rng.uniform(-1, 1, (MR, N))
    r = rng.uniform(-1, 1, MR)
    A = rng.uniform(-1, 1, (K, N))
    b_eq = rng.uniform(-0.5, 0.5, K)
    var = rng.permutation(N)[:M]
    a = rng.choice([-1.0, 1.0], M) * rng.uniform(0.5, 1.5, M)
    b = rng.uniform(0.1, 1.0, M)
    g = rng.normal(size=N + 2 * M + K)
    return dict(J=J, r=r, A=A, b_eq=b_eq, var=var, a=a, b=b), g


def cost(th):
    """(G, c) of a parameter set: given directly, or formed from (J, r, lam) as LinearizeAndFillQP does."""
    if "G" in th:
        return th["G"], th["c"]
    return th["J"].T @ th["J"] + th.get("lam", LAM) * np.eye(N), th["J"].T @ th["r"]


def root(th, v0=None):
    """v* with F(v*; theta) = 0 at fixed mu: damped Newton (fraction to the boundary 0.9) to |F|_inf < 1e-14."""
    G, c = cost(th)
    v = np.concatenate([np.zeros(N), np.ones(M), np.zeros(K), np.ones(M)]) if v0 is None else v0.copy()
    best = np.inf
    for _ in range(200):
        F = R.residual(G, c, th["A"], th["b_eq"], th["var"], th["a"], th["b"], v, MU)
        best = np.max(np.abs(F))
        if best < 1e-14:
            return v
        d = np.linalg.solve(R.kkt_matrix(G, th["A"], th["var"], th["a"], v), -F)
        alpha = 1.0
        for lo, hi in ((N, N + M), (N + M + K, N + 2 * M + K)):
            neg = d[lo:hi] < 0
            if neg.any():
                alpha = min(alpha, 0.9 * np.min(-v[lo:hi][neg] / d[lo:hi][neg]))
        v = v + alpha * d
    raise AssertionError(f"Newton stalled at |F|_inf = {best:.3e}")
