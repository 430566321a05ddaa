"""The covariance reference (tests/covariance_reference.py) held to itself, and what mo_qp_covariance decides without a GPU: the long-double
truth satisfies the identities that define C, the restatement in the plan's dtype stays within 64 eps of it on the well-conditioned families
(the condition the device bound 8 max(E_case, 8 eps) rests on), the symbol is declared and exported under ABI 0.5, and the argument errors
come in the order of the sibling calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import covariance_reference as CR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LD = CR.LD
# the truth's own rounding: n cond eps_ld is below 1e-16 on these cases (n <= 33, cond(J^T J) of a 2n x n normal J about 34); two orders of margin
TRUTH_TOL = 1e-14
IDENTITY_CASES = ("k0_n17_f64", "eq_n7_k3_f64", "eq_n33_k5_f64", "deficient_n7_k3_f64", "singular_G_n7_mr5_k3_f64")


def test_long_double_is_extended():
    assert np.finfo(LD).eps < 2e-19


@pytest.mark.parametrize("name", IDENTITY_CASES)
def test_truth_identities(name):
    case, Ct = CR.by_name(name), CR.reference(name)
    for p in range(case.B):
        S = CR.sym_lower(case.G[p].astype(LD))
        Cp = Ct[p]
        cmax = np.abs(Cp).max()
        assert np.array_equal(Cp, Cp.T)
        csc = CR.ld_matmul(CR.ld_matmul(Cp, S), Cp)
        scale = np.abs(S).max() * cmax * cmax * case.n * case.n
        assert np.abs(csc - Cp).max() <= TRUTH_TOL * max(scale, cmax), (name, p)                 # C S C = C
        A = case.rows(p)
        if A is None or A.shape[0] == 0:
            I = CR.ld_matmul(Cp, S)
            assert np.abs(I - np.eye(case.n)).max() <= TRUTH_TOL * np.abs(S).max() * cmax * case.n, (name, p)   # k = 0: C = S^-1
            continue
        AC = CR.ld_matmul(A.astype(LD), Cp)
        assert np.abs(AC).max() <= TRUTH_TOL * np.abs(A).max() * cmax * case.n, (name, p)       # A C = 0
        if name.startswith("singular") or name.startswith("eq"):
            K = CR.kkt_inverse_block(case.G[p], A.astype(LD))
            assert CR.error(K, Cp) <= 1e-12, (name, p, CR.error(K, Cp))                          # the top-left block of the KKT inverse


def test_rank_n_gives_zero():
    for name in ("full_rank_n3_k3_f64", "full_rank_n16_k16_f64"):
        assert not CR.reference(name).any()


@pytest.mark.parametrize("name", [c.name for c in CR.cases() if c.well_conditioned])
def test_restatement_on_the_well_conditioned_families(name):
    case = CR.by_name(name)
    E = CR.restatement_errors(name).max() / case.eps
    print(f"{name}: restatement error {E:.2f} eps")
    assert E <= CR.WELL_CONDITIONED_MAX, (name, E)


def test_capacity_rule():
    assert CR.lds_bytes(128, 16, 128, 8) == 151456 and CR.lds_bytes(128, 16, 128, 8) <= CR.LDS_BYTES     # mo_nullspace_solve's own limit fits
    assert all(CR.lds_bytes(n, 112 - n, n, 8) <= CR.LDS_BYTES for n in range(56, 113))                   # every n + k <= 112 (k <= n) in fp64
    assert CR.lds_bytes(CR.CAPACITY_N, CR.CAPACITY_K, CR.CAPACITY_N, 8) <= CR.LDS_BYTES < CR.lds_bytes(CR.CAPACITY_N + 1, CR.CAPACITY_K, CR.CAPACITY_N + 1, 8)


def test_symbol_is_declared_and_exported_under_abi_0_5():
    from mini_opt_amd import _lib as L
    L.build()
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "mini_opt_hip.h")).read()
    declared = set(re.findall(r"\b(mo_[a-z_]+)\s*\(", header))
    assert "mo_qp_covariance" in declared and "mo_qp_covariance" in L.EXPORTS and hasattr(lib, "mo_qp_covariance")
    assert (int(re.search(r"#define MO_VERSION_MAJOR (\d+)", header).group(1)), int(re.search(r"#define MO_VERSION_MINOR (\d+)", header).group(1))) == (0, 5)
    assert lib.mo_version_string().startswith(b"mini_opt_hip 0.5")
    import mini_opt_amd
    assert callable(mini_opt_amd.covariance)


def test_argument_errors_without_gpu():
    """What the call judges from its arguments alone needs no device, in the order: both outputs NULL, J given, q < 1, cov_ld < q, the plan."""
    from mini_opt_amd import _lib as L
    L.build()
    lib = L.lib()
    p16 = C.c_void_p(16)
    qp = L.Problem()
    qp.G, qp.G_stride, qp.G_ld = 16, 64, 8
    jl = L.Problem()
    jl.J, jl.J_stride, jl.J_ld, jl.J_layout, jl.r, jl.r_stride = 16, 64, 8, L.MO_ROW_MAJOR, 16, 8

    def call(prob, q, cov, cov_ld, var):
        rc = lib.mo_qp_covariance(None, C.byref(prob), 4, None, q, None, 0, cov, 64, cov_ld, var, 8, None, None)
        return rc, lib.mo_last_error()

    rc, msg = call(jl, 0, None, 0, None)                 # everything wrong at once: the outputs come first
    assert rc == -1 and b"both NULL" in msg, (rc, msg)
    rc, msg = call(jl, 0, p16, 0, None)
    assert rc == -1 and b"J given" in msg, (rc, msg)
    rc, msg = call(qp, 0, p16, 0, None)
    assert rc == -1 and b"q = 0" in msg, (rc, msg)
    rc, msg = call(qp, 8, p16, 7, p16)
    assert rc == -2 and b"cov_ld" in msg, (rc, msg)
    rc, msg = call(qp, 8, None, 0, p16)                  # cov_ld is not read without cov_out
    assert rc == -1 and b"plan" in msg, (rc, msg)
    rc, msg = call(qp, 8, p16, 8, None)
    assert rc == -1 and b"plan" in msg, (rc, msg)
