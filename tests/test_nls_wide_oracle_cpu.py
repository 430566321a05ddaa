"""Conditions on the INPUTS of tests/test_gpu_nls_wide.py, checked with the oracle alone (oracle/nls_oracle.py, no GPU), so that the GPU
tests cannot pass vacuously: every case goes through the branch of the outer loop it is there for -- on the thread path (n <= 32) and on the
wave path (n > 32) -- and every start of a strict case is decided clear of every threshold, so the device has no excuse to differ."""
import functools

import numpy as np
import pytest

from oracle import nls_oracle as N
from tests import nls_wide_problems as W

# Every outer-loop decision of a strict start keeps this relative distance from its threshold: 100 x the NLS_KNIFE_EDGE = 1e-8 below which
# tests/test_gpu_nls.py::knife_edge_rule lets the device differ.
MIN_OUTER_MARGIN = 1.0e-6


@functools.lru_cache(maxsize=None)
def oracle_runs(kind, n):
    """[(termination, logs, decision margins)] of every start of a strict case, computed once for both tests below."""
    case = W.strict_case(kind, n)
    out = []
    for x0 in case.guesses():
        o = N.ConstrainedNonlinearLeastSquares(case.oracle_problem(), track_margins=True)
        term, logs = o.solve(N.Params(**case.params), x0)
        out.append((term, logs, list(o.margins)))
    return case, out


def _reached(case, runs):
    got = set()
    for term, logs, _ in runs:
        got |= W.branches_of_oracle_run(case, term, logs)
    return got


@pytest.mark.parametrize("n", W.SIZES)
@pytest.mark.parametrize("kind", W.STRICT_KINDS)
def test_strict_case_reaches_the_branches_it_claims(kind, n):
    case, runs = oracle_runs(kind, n)
    assert len(runs) % 4 != 0 and len(runs) <= 16                 # idle waves in the last workgroup of the wave path
    missing = [c for c in case.claims if c not in _reached(case, runs)]
    assert not missing, (case.name, missing)


@pytest.mark.parametrize("n", W.SIZES)
@pytest.mark.parametrize("kind", W.STRICT_KINDS)
def test_every_start_of_a_strict_case_is_determinate(kind, n):
    """No inner QP on a knife edge (oracle/margins.py: margin / threshold of its kind >= 1) and no outer decision within 1e-6 (relative) of
    its threshold."""
    case, runs = oracle_runs(kind, n)
    for p, (_, _, margins) in enumerate(runs):
        qp = min([m[2] for m in margins if m[1] == "qp"], default=np.inf)
        outer = min([(m[2], m[0], m[1]) for m in margins if m[1] != "qp"], default=(np.inf, -1, ""))
        assert qp >= 1.0, (case.name, p, qp)
        assert outer[0] >= MIN_OUTER_MARGIN, (case.name, p, outer)


def test_every_branch_is_claimed_on_the_thread_path_and_on_the_wave_path():
    """Each branch the wide tests are there for is claimed by a case at a size <= 32 and by a case at a size > 32; the lane loops of the wave
    path wrap only beyond 64, so the branches that move the n-vectors (a trial point beyond the first, the accepted step) are also claimed
    at n = 72.  MO_LS_FAILURE_INVALID_ALPHA is not in the list: a search of some 1400 starts of the pole family found none."""
    wanted = (W.POLY_CUBIC, W.POLY_CUBIC_2, W.ARMIJO_3, W.LS_MAX_ITERATIONS, W.LS_POSITIVE_DERIVATIVE, W.LS_NON_FINITE, W.RESTORE_THEN_SUCCESS,
              W.TERM_MAX_LAMBDA)
    claimed = {n: set().union(*(W.strict_case(kind, n).claims for kind in W.STRICT_KINDS)) for n in W.SIZES}
    assert W.CONTROL <= 32 < W.FIRST_WAVE <= 64 < W.WRAPPING
    for branch in wanted:
        assert branch in claimed[W.CONTROL] and branch in claimed[W.FIRST_WAVE] and branch in claimed[W.WRAPPING], branch


@pytest.mark.parametrize("n", W.SIZES)
def test_rank_deficient_case_ends_indefinite_without_damping_and_first_order_with_it(n):
    ref = N.ConstrainedNonlinearLeastSquares(W.deficient_case(n, False).oracle_problem())
    for x0 in W.deficient_case(n, False).guesses():
        term, logs = ref.solve(N.Params(**W.deficient_case(n, False).params), x0)
        assert term == N.QP_INDEFINITE and len(logs) == 0
    damped = W.deficient_case(n, True)
    ref = N.ConstrainedNonlinearLeastSquares(damped.oracle_problem())
    for x0 in damped.guesses():
        term, logs = ref.solve(N.Params(**damped.params), x0)
        assert term == N.SATISFIED_FIRST_ORDER_TOL and len(logs) >= 2


def test_wrap_pi_case_has_trial_points_outside_the_interval_and_is_determinate():
    """The WRAP_PI case of the GPU test is only a test of the wrap if trial points x + alpha dx leave [-pi, pi) from starts inside it; and,
    as a strict case, the oracle's run under the ModPi retraction keeps clear of every threshold."""
    from tests import nls_problems as P
    case = W.wrap_pi_case()
    g = case.guesses()
    assert np.all(np.abs(g) < np.pi)
    for p, x0 in enumerate(g):
        outside = []

        def retraction(x, dx, alpha):
            outside.append(bool(np.any(np.abs(x + dx * alpha) > np.pi)))
            return P.mod_pi_retraction_np(x, dx, alpha)
        o = N.ConstrainedNonlinearLeastSquares(case.oracle_problem(), retraction=retraction, track_margins=True)
        o.solve(N.Params(**case.params), x0)
        assert any(outside), p
        assert np.all(np.abs(o.variables) <= np.pi)
        assert min(m[2] for m in o.margins if m[1] != "qp") >= MIN_OUTER_MARGIN, p
