"""The formulas of the fused kernel's right-hand-side mode (tests/fused_rhs_reference.py restates them in numpy) against LU on the full K
of tests/diff_reference.py: direct and transposed, with and without inequalities, on every shape of tests/test_gpu_fused_rhs.py.
Bound 1e-11 rel-inf: the inputs (synth.make_batch, stream 41) are well-posed -- cond K <= 1.2e5, the reduced system agrees with LU to
<= 3.6e-15 everywhere but (33, 31, 66, 66) at 2.4e-13 -- so a wrong sign, scaling or index shows up twelve orders above it."""
import numpy as np
import pytest

from mini_opt_amd import synth
from tests import diff_reference as R
from tests import fused_rhs_reference as F

BOUND = 1e-11


def rel_inf(got, ref):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("shape", F.SHAPES, ids=lambda s: "n%dk%dm%d" % s[:3])
def test_reduced_right_hand_side_against_lu_on_the_full_matrix(shape):
    n, k, m, m_r = shape
    hb = synth.make_batch(n, k, m, m_r, 6, stream=41)
    rng = np.random.default_rng(41)
    worst = {}
    for p in range(6):
        G = hb.J[p].T @ hb.J[p] + hb.lam * np.eye(n)
        A = hb.A_eq[p].T
        v = hb.vars[p]
        rhs = rng.normal(size=v.shape)
        K = R.kkt_matrix(G, A, hb.cons_var[p], hb.cons_a[p], v)
        cases = {"direct": (F.fused_rhs_solve(G, A, hb.cons_var[p], hb.cons_a[p], v, rhs), R.solve_direct(K, rhs)),
                 "transposed": (F.fused_rhs_solve(G, A, hb.cons_var[p], hb.cons_a[p], v, rhs, transpose=True), R.solve_transposed(K, rhs))}
        # MO_STEP_NO_INEQUALITIES: the system of [x | y] alone, the s and z blocks ignored and returned as 0
        v0, rhs0 = np.concatenate([v[:n], v[n + m:n + m + k]]), np.concatenate([rhs[:n], rhs[n + m:n + m + k]])
        K0 = R.kkt_matrix(G, A, np.zeros(0, dtype=np.int32), np.zeros(0), v0)
        embed = lambda d: np.concatenate([d[:n], np.zeros(m), d[n:], np.zeros(m)])
        cases["direct, no inequalities"] = (F.fused_rhs_solve(G, A, hb.cons_var[p], hb.cons_a[p], v, rhs, include_inequalities=False),
                                            embed(R.solve_direct(K0, rhs0)))
        cases["transposed, no inequalities"] = (F.fused_rhs_solve(G, A, hb.cons_var[p], hb.cons_a[p], v, rhs, transpose=True, include_inequalities=False),
                                                embed(R.solve_transposed(K0, rhs0)))
        for tag, (got, ref) in cases.items():
            worst[tag] = max(worst.get(tag, 0.0), rel_inf(got, ref))
    print(f"fused rhs restatement vs LU {shape}: {worst}")
    assert max(worst.values()) < BOUND, worst
