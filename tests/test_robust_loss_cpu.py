"""Robust loss functions, the part that needs no GPU: the numpy reference itself (tests/robust_loss_reference.py), the wrapped-oracle
yardstick of the loop tests, the strict starts the GPU loop test runs, and the library's exports."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import nls_oracle as N
from tests import robust_loss_reference as R

ROBUST = (R.HUBER, R.SOFT_L1, R.CAUCHY, R.TUKEY)
MIN_OUTER_MARGIN = 1.0e-6   # the rule and threshold of tests/test_nls_wide_oracle_cpu.py


@pytest.mark.parametrize("kind", R.KINDS)
def test_rho_prime_is_the_derivative_of_rho(kind):
    """Central difference of rho in long double on a grid of s / a^2 from 1e-6 to 1e6.  With h = 1e-5 s the truncation error is
    h^2 |rho'''| / 6 <= 1e-10 rho' x (a constant of order 1 for these losses, away from the C^1 joints) and the rounding error
    eps_ld rho / h ~ 1e-14; grid points within h of a joint (s = a^2) are moved off it."""
    a = 1.5
    ld = np.longdouble
    t = np.logspace(-6, 6, 97).astype(ld)
    t = np.where(np.abs(t - 1) < 1e-3, ld(1.01), t)
    s = t * ld(a) ** 2
    h = s * ld(1e-5)
    d = (R.rho(kind, a, s + h, ld) - R.rho(kind, a, s - h, ld)) / (2 * h)
    w = R.rho_prime(kind, a, s, ld)
    if kind == R.TUKEY:   # beyond the cutoff both are exactly 0
        assert np.all(w[t > 1] == 0) and np.all(d[t > 1] == 0)
    np.testing.assert_allclose(d.astype(float), w.astype(float), rtol=1e-8, atol=1e-12)


@pytest.mark.parametrize("kind", R.KINDS)
def test_rho_dominates_s_rho_prime(kind):
    """rho(s) >= s rho'(s): what makes the term under the wrapper's root non-negative (concave, rho(0) = 0)."""
    a = 0.75
    ld = np.longdouble
    s = np.concatenate([[0.0], np.logspace(-6, 6, 193) * a * a]).astype(ld)
    f, w = R.rho(kind, a, s, ld), R.rho_prime(kind, a, s, ld)
    assert np.all(f - s * w >= -4 * np.finfo(ld).eps * f)
    assert R.rho(kind, a, ld(0), ld) == 0


@pytest.mark.parametrize("kind", (R.HUBER, R.TUKEY))
def test_huber_and_tukey_are_continuous_across_the_joint(kind):
    """rho and rho' at the two doubles either side of s = a^2 differ from the values at a^2 by a few ulps of the values' own scale."""
    a = 1.5
    a2 = a * a
    eps = np.finfo(float).eps
    lo, hi = np.nextafter(a2, 0.0), np.nextafter(a2, np.inf)
    f = [float(R.rho(kind, a, s)) for s in (lo, a2, hi)]
    w = [float(R.rho_prime(kind, a, s)) for s in (lo, a2, hi)]
    assert abs(f[0] - f[1]) <= 4 * eps * a2 and abs(f[2] - f[1]) <= 4 * eps * a2
    assert abs(w[0] - w[1]) <= 4 * eps and abs(w[2] - w[1]) <= 4 * eps


def _solve(problem, params, x0, **kw):
    o = N.ConstrainedNonlinearLeastSquares(problem, **kw)
    term, logs = o.solve(params, x0)
    return o, term, logs


def test_all_trivial_wrapper_reproduces_the_plain_oracle_on_the_rosenbrock_blocks():
    case = R.rosen_case(R.STRICT_SEEDS["rosenbrock_huber"], kind=R.TRIVIAL)
    prm = N.Params(**case.params)
    for p in range(len(case.starts)):
        a, ta, la = _solve(case.oracle_problem(p, robust=True), prm, case.starts[p])
        b, tb, lb = _solve(case.oracle_problem(p, robust=False), prm, case.starts[p])
        assert ta == tb and len(la) == len(lb), p
        np.testing.assert_allclose(a.variables, b.variables, rtol=0, atol=1e-12)


def test_the_wrapper_is_the_irls_model():
    """The wrapped linearisation gives G = sum w J^T J, c = sum w J^T r and f = 0.5 sum rho; the wrapped cost call the same f."""
    rng = np.random.default_rng(5)
    rows = [1, 2, 3, 7]
    losses = [(R.HUBER, 0.5), (R.SOFT_L1, 1.5), (R.CAUCHY, 0.75), (R.TUKEY, 4.0)]
    J, r0 = rng.normal(size=(13, 5)), rng.normal(size=13)
    cost = lambda x, want_J: (J @ x + r0, J if want_J else None)
    x = rng.normal(size=5)
    wrapped = R.wrap_cost(cost, rows, losses)
    w, f, _ = R.loss_eval(rows, losses, (J @ x + r0)[None], np.float64)
    rw, Jw = wrapped(x, True)
    np.testing.assert_allclose(Jw.T @ Jw, J.T @ (w[0][:, None] * J), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(Jw.T @ rw, J.T @ (w[0] * (J @ x + r0)), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(0.5 * rw @ rw, f[0], rtol=1e-13)
    rc, _ = wrapped(x, False)
    np.testing.assert_allclose(0.5 * rc @ rc, f[0], rtol=1e-13)


@functools.lru_cache(maxsize=None)
def _inlier_parameters(seed):
    y, mask, true = R.fit_data(seed)
    o, _, _ = _solve(N.Problem(2, R.fit_cost_np(y, mask)), N.Params(max_iterations=30), np.array(true))
    return o.variables.copy()


def test_outlier_fit_plain_is_dragged_and_every_robust_loss_is_not():
    """12 points of a exp(b t), 3 gross outliers, loss scale 0.05 (Tukey 1.0), default Params: against the plain fit of the 9 inliers."""
    seeds = R.FIT_SEEDS
    plain = R.fit_case(R.HUBER, seeds)
    for p, s in enumerate(seeds):
        o, _, _ = _solve(plain.oracle_problem(p, robust=False), N.Params(), plain.starts[p])
        assert np.max(np.abs(o.variables - _inlier_parameters(s))) > 0.2, (s, o.variables)
    for kind in ROBUST:
        case = R.fit_case(kind, seeds)
        for p, s in enumerate(seeds):
            o, _, logs = _solve(case.oracle_problem(p), N.Params(**case.params), case.starts[p])
            assert np.max(np.abs(o.variables - _inlier_parameters(s))) < 0.05, (case.name, s, o.variables)
            assert 2 <= len(logs) <= 8


@pytest.mark.parametrize("case", R.strict_cases(), ids=lambda c: c.name)
def test_strict_starts_have_no_decision_near_its_threshold(case):
    """Every start the GPU loop test runs: no inner QP on a knife edge (ratio >= 1, oracle/margins.py) and no outer-loop decision within
    1e-6 (relative) of its threshold -- so the GPU test may demand the oracle's termination and iteration count on every start."""
    assert len(case.starts) == len(R.STRICT_SEEDS[case.name])
    for p in range(len(case.starts)):
        o, term, logs = _solve(case.oracle_problem(p), N.Params(**case.params), case.starts[p], track_margins=True)
        qp = min([m[2] for m in o.margins if m[1] == "qp"], default=np.inf)
        outer = min([(m[2], m[0], m[1]) for m in o.margins if m[1] != "qp"], default=(np.inf, -1, ""))
        assert qp >= 1.0, (case.name, p, qp)
        assert outer[0] >= MIN_OUTER_MARGIN, (case.name, p, outer)
        assert term != N.MAX_ITERATIONS and term != N.MAX_LAMBDA, (case.name, p, term)


def test_the_rosenbrock_huber_loss_is_active_at_the_start_and_inactive_at_the_solution():
    case = R.rosen_case(R.STRICT_SEEDS["rosenbrock_huber"])
    at_one = 0
    for p in range(len(case.starts)):
        r0, _ = case.cost_np(p)(case.starts[p], False)
        s0 = (r0.reshape(-1, 2) ** 2).sum(axis=1)
        assert np.any(s0 > 1.0), p
        o, _, _ = _solve(case.oracle_problem(p), N.Params(**case.params), case.starts[p])
        r1, _ = case.cost_np(p)(o.variables, False)
        if np.all((r1.reshape(-1, 2) ** 2).sum(axis=1) <= 1.0):
            at_one += 1
    assert at_one >= len(case.starts) // 2


def test_library_exports_the_robust_loss_entry_points():
    from mini_opt_amd import _lib as L
    L.build()
    lib = C.CDLL(L.LIB_PATH)
    for name in ("mo_residual_loss_create", "mo_residual_loss_destroy", "mo_residual_loss_eval", "mo_linearize_blocks_robust",
                 "mo_nls_solve_blocks_robust"):
        assert hasattr(lib, name), name
        assert name in L.EXPORTS
