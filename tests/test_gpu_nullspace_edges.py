"""nullspace_kernel (csrc/kkt_generic.hip, mo_nullspace_solve) at its edge cases against the long-double referee of tests/nullspace_cases.py,
whose docstring has the families, the reference and the two bounds:

    forward error   |x - x_ref|_inf / |x_ref|_inf         <= 8 max(E_case, 8 eps)
    backward error  |A x + b|_2 / (|A|_F |x|_2 + |b|_2)   <= 8 max(BE_case, 1 eps)

with E_case / BE_case the worst errors of oracle.nls_oracle.null_space_solve over the case's batch (tests/test_nullspace_cases_cpu.py
measures them and asserts E_case <= 64 eps outside family F), and the same multiples of 2^-23 for fp32 plans.  Terminations match exactly, a
NOT_POSITIVE_DEFINITE problem has an all-NaN x, family B's constrained entries are -b / a to the bit, and no output word keeps its prefill
(x is prefilled with a NaN of another payload than the kernel's, the terminations with -1).  The calls go to the C ABI, because
QPNullSpaceSolver.Solve allocates its outputs itself and passes no J layout on.

Measured on an MI355X, worst case of each family, in eps of the plan's type (the oracle's columns are E_case and BE_case; every test prints
its own line):

    family  type  cases   forward: oracle   device      backward: oracle   device     device before the two fixes below
    A       f64     6              20.4      19.2                0.39      0.59      forward 7.4e6 .. 3.4e7, backward 1.1e6 .. 3.2e6
    A       f32     6              24.0      15.5                1.11      0.80      forward 843 .. 3119, backward 84 .. 742
    B       f64     2               3.7       5.6                0         0
    B       f32     2               9.3      15.6                0         0.005
    C       f64     3              17.8      19.4                0.48      0.42      negligible_rows: forward 1.6e16 (a wrong x)
    C       f32     2              19.3      25.9                0.37      0.34
    D       f64     4               8.2      10.7                0.48      0.85
    E       f64    10              40.7      33.8                0.74      0.52
    E       f32     9              40.4      33.4                0.70      0.68
    F       f64     3          305377    304409                  0.27      0.35
    G       f64     2               9.3       7.0                0.53      0.55

The two defects this table found in nullspace_kernel, both fixed with it: a Householder tail below sqrt(eps) of its pivot was set to zero
(the tail's squared norm came from big - c0^2; family A), and a reflector beyond the rank left the rows rank .. j - 1 of G untransformed, so
the reduced Hessian of a numerically rank-deficient A_eq was not Q2^T G Q2 (C negligible_rows; the fp32 plans of family C at the fp64
spread 2^-20 .. 2^20, which is beyond the fp32 rank rule, answered NOT_POSITIVE_DEFINITE for a positive definite G).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from mini_opt_amd import _lib as L
from mini_opt_amd import qp as Q
from tests import nullspace_cases as NC
from tests.sens_fixtures import Plan, T

pytestmark = pytest.mark.gpu
DT = {"f64": torch.float64, "f32": torch.float32}
PREFILL = {"f64": (torch.int64, 0x7FF80000DEADBEEF), "f32": (torch.int32, 0x7FC0BEEF)}   # quiet NaNs the kernel never writes


def device_problem(case, k=None):
    """The case on the device; k: only the first k equality rows (zero rows beyond the case's own)."""
    dt = DT[case.dtype]
    A, b = case.A, case.b
    if k is not None:
        A = np.zeros((case.B, k, case.n)); b = np.zeros((case.B, k))
        A[:, :min(k, case.k)] = case.A[:, :k]; b[:, :min(k, case.k)] = case.b[:, :k]
    eq = dict(A_eq=T(A.transpose(0, 2, 1), dt), b_eq=T(b, dt))
    if case.J is None:
        return Q.BatchedQP(n=case.n, k=A.shape[1], G=T(np.tril(case.G).transpose(0, 2, 1), dt), c=T(case.c, dt), **eq)
    J = case.J.transpose(0, 2, 1) if case.J_layout == "col" else case.J        # column-major: tensor row i is column i of J
    return Q.BatchedQP(n=case.n, k=A.shape[1], J=T(J, dt), r=T(case.r, dt), lam_vec=T(case.lam, dt), J_layout=case.J_layout, **eq)


def solve(case, k=None):
    """mo_nullspace_solve with prefilled outputs: (return code, x [B, n] float64 numpy, raw x tensor, termination numpy)."""
    prob = device_problem(case, k)
    it, pattern = PREFILL[case.dtype]
    raw = torch.full((case.B, case.n), pattern, dtype=it, device="cuda:0")
    x = raw.view(DT[case.dtype])
    term = torch.full((case.B,), -1, dtype=torch.int32, device="cuda:0")
    with Plan(case.n, prob.k, 0, prob.m_r, DT[case.dtype], case.B) as plan:
        ps = prob.as_struct()
        rc = L.lib().mo_nullspace_solve(plan.h, C.byref(ps), case.B, Q._ptr(x), case.n, Q._ptr(term), Q._stream())
        torch.cuda.synchronize()
    return rc, x.cpu().numpy().astype(np.float64), raw.cpu().numpy(), term.cpu().numpy()


def check(case, x, raw, term):
    name = case.name
    x_ref, _ = NC.reference(name)
    o = NC.oracle_errors(name)
    ok = case.term == NC.SUCCESS
    fwd = np.array([NC.forward_error(x[p], x_ref[p]) if ok[p] and np.all(np.isfinite(x[p])) else np.nan for p in range(case.B)]) / case.eps
    be = np.array([NC.backward_error(case.A[p], case.b[p], x[p]) if ok[p] and np.all(np.isfinite(x[p])) else np.nan for p in range(case.B)]) / case.eps
    print(f"nullspace-edge {name} family {case.family} {case.dtype}: forward error oracle {o.E_case:.2f} device {np.nanmax(fwd) if ok.any() else 0:.2f} "
          f"(bound {NC.forward_bound(name):.0f}) eps, backward error oracle {o.BE_case:.3f} device {np.nanmax(be) if ok.any() else 0:.3f} "
          f"(bound {NC.backward_bound(name):.0f}) eps")
    assert np.array_equal(term, case.term), (name, term)
    assert not np.any(raw == PREFILL[case.dtype][1]), name
    assert np.all(np.isfinite(x[ok])) and np.all(np.isnan(x[~ok])), name
    assert np.all(fwd[ok] <= NC.forward_bound(name)), (name, fwd)
    assert np.all(be[ok] <= NC.backward_bound(name)), (name, be)
    if case.exact_idx is not None:                                             # family B, the zero-tail half: -b / a at 0 ulp
        assert np.array_equal(np.take_along_axis(x[:len(case.exact_idx)], case.exact_idx, axis=1), case.exact_val), name


@pytest.mark.parametrize("name", NC.names())
def test_nullspace_edge_case(name):
    case = NC.by_name(name)
    rc, x, raw, term = solve(case)
    assert rc == L.MO_OK, (name, rc, L.lib().mo_last_error().decode())
    check(case, x, raw, term)


def test_capacity_at_n128_fp64():
    """n = 128 in fp64, given (G, c): k is raised until mo_nullspace_solve answers MO_ERR_UNSUPPORTED (the check precedes the launch: no output
    word is touched).  The last k it takes is the table's CAPACITY_K and solves to the bound; mo_plan_nls_uses_nullspace flips at the same k."""
    case = NC.by_name(NC.CAPACITY_CASE)
    k = 17
    while True:
        rc, x, raw, term = solve(case, k)
        if rc != L.MO_OK:
            break
        assert np.array_equal(term, case.term) and np.all(np.isfinite(x)), k
        if k == case.k:
            check(case, x, raw, term)
        k += 1
        assert k <= 40
    assert rc == -3 and k - 1 == NC.CAPACITY_K                                 # MO_ERR_UNSUPPORTED
    assert np.all(raw == PREFILL["f64"][1]) and np.all(term == -1)
    for kk in range(17, k + 2):
        with Plan(case.n, kk, 0, 0, torch.float64, case.B) as plan:
            assert bool(L.lib().mo_plan_nls_uses_nullspace(plan.h)) == (kk < k), kk
