"""CPU checks of the differentiable solve for residual-block input: the gradient formulas of the packed local Jacobians (pinned by central
differences through a numpy barrier problem, no product code involved) and the two entry points of the C ABI (symbols, struct layout,
argument errors without a GPU)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import blocks_diff_reference as BR
from tests import diff_reference as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
N = 7
COST = [((3, 0, 5, 3), 3), ((6,), 2), ((1, 2, 4, 0, 6), 4), ((2, 2), 1), ((5, 4, 1), 6)]     # (3, 0, 5, 3) and (2, 2) repeat a variable
EQ = [((0, 4, 0), 1), ((2, 6), 1)]                                                            # the LAST column wins variable 0
K, M = 2, 3
MU = 1e-3
LAM = 0.05


def fixed_problem():
    rng = np.random.default_rng(20261018)
    th = dict(J=BR.pack([rng.uniform(-1, 1, (R_, len(idx))) for idx, R_ in COST]), r=rng.uniform(-1, 1, sum(R_ for _, R_ in COST)),
              Jeq=BR.pack([rng.uniform(-1, 1, (R_, len(idx))) for idx, R_ in EQ]), r_eq=rng.uniform(-0.5, 0.5, K), lam=np.array([LAM]),
              var=np.array([1, 5, 3]), a=np.array([1.0, -1.0, 1.0]) * rng.uniform(0.5, 1.5, M), b=rng.uniform(0.1, 1.0, M))
    return th, rng.normal(size=N + 2 * M + K)


def qp_of(th):
    """(sym G, c, A_eq, b_eq) of the packed parameters, as LinearizeAndFillQP forms them from residual blocks."""
    G_low, c = BR.linearize(N, COST, BR.unpack(th["J"], COST), BR.split_rows(th["r"], COST), float(th["lam"][0]))
    return BR.symmetric(G_low), c, BR.jacobian(N, EQ, BR.unpack(th["Jeq"], EQ)), th["r_eq"]


def root(th, v0=None):
    """v* with F(v*; theta) = 0 at fixed mu: damped Newton (fraction to the boundary 0.9) to |F|_inf < 1e-14, as tests/test_diff_cpu.py."""
    G, c, A, b_eq = qp_of(th)
    v = np.concatenate([np.zeros(N), np.ones(M), np.zeros(K), np.ones(M)]) if v0 is None else v0.copy()
    best = np.inf
    for _ in range(200):
        F = R.residual(G, c, A, b_eq, th["var"], th["a"], th["b"], v, MU)
        best = np.max(np.abs(F))
        if best < 1e-14:
            return v
        d = np.linalg.solve(R.kkt_matrix(G, A, th["var"], th["a"], v), -F)
        alpha = 1.0
        for lo, hi in ((N, N + M), (N + M + K, N + 2 * M + K)):
            neg = d[lo:hi] < 0
            if neg.any():
                alpha = min(alpha, 0.9 * np.min(-v[lo:hi][neg] / d[lo:hi][neg]))
        v = v + alpha * d
    raise AssertionError(f"Newton stalled at |F|_inf = {best:.3e}")


def test_block_formulas_against_central_differences():
    """l(theta) = g . v*(theta) over EVERY packed value of the cost and equality layouts, every r, r_eq and lambda, h = 1e-6.  Bound 1e-7 of
    the group's largest gradient entry, the bound of test_formulas_against_central_differences (finite-difference round-off eps |l| / h ~ 1e-9
    at gradients of order 1).  The equality column that loses its global column is exactly 0."""
    th, g = fixed_problem()
    v = root(th)
    G, _, A, _ = qp_of(th)
    u = R.solve_transposed(R.kkt_matrix(G, A, th["var"], th["a"], v), g)
    x, _, y, _ = R.split(v, N, K, M)
    ux, _, uy, _ = R.split(u, N, K, M)
    dJ, dr, dlam = BR.gradients_blocks(COST, BR.unpack(th["J"], COST), BR.split_rows(th["r"], COST), x, ux)
    dJeq, dr_eq = BR.gradients_eq_blocks(EQ, x, ux, y, uy)
    analytic = dict(J=BR.pack(dJ), r=np.concatenate(dr), lam=np.array([dlam]), Jeq=BR.pack(dJeq), r_eq=dr_eq)
    assert analytic["Jeq"][0] == 0.0 and np.all(analytic["Jeq"][1:] != 0.0)      # ((0, 4, 0), 1): local column 0 loses variable 0
    worst = {}
    for key, want in analytic.items():
        fd = np.zeros_like(want)
        for i in range(len(want)):
            vals = []
            for sign in (1.0, -1.0):
                t = {k_: (v_.astype(float, copy=True) if v_.dtype.kind == "f" else v_) for k_, v_ in th.items()}
                t[key][i] += sign * 1e-6
                vals.append(g @ root(t, v))
            fd[i] = (vals[0] - vals[1]) / 2e-6
        worst[key] = np.max(np.abs(fd - want)) / np.max(np.abs(want))
        print(f"{key}: max |fd - analytic| / max |analytic| = {worst[key]:.3e} (max |analytic| = {np.max(np.abs(want)):.3e})")
        if key == "Jeq":
            assert fd[0] == 0.0
    assert max(worst.values()) < 1e-7, worst


def test_collapsed_form_equals_the_pair_weights():
    """Without repeated indices dJ_b[:, p] = -u_p (J_b x_loc + r_b) - x_p (J_b u_loc); a repeated variable adds +u_i x_i J_b[:, q'] for every
    other local column q' on it -- the form the kernel evaluates."""
    rng = np.random.default_rng(3)
    Js = [rng.uniform(-1, 1, (R_, len(idx))) for idx, R_ in COST]
    rs = [rng.uniform(-1, 1, R_) for _, R_ in COST]
    x, ux = rng.normal(size=N), rng.normal(size=N)
    dJ, dr, _ = BR.gradients_blocks(COST, Js, rs, x, ux)
    for (idx, _), J, r, want, want_r in zip(COST, Js, rs, dJ, dr):
        ii = list(idx)
        t, w = J @ x[ii] + r, J @ ux[ii]
        got = -np.outer(t, ux[ii]) - np.outer(w, x[ii])
        for p, i in enumerate(ii):
            for q, j in enumerate(ii):
                if q != p and j == i:
                    got[:, p] += ux[i] * x[i] * J[:, q]
        assert np.max(np.abs(got - want)) <= 1e-14 * max(1.0, np.max(np.abs(want)))
        assert np.max(np.abs(-w - want_r)) <= 1e-14 * max(1.0, np.max(np.abs(want_r)))


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from mini_opt_amd import _lib as L
    L.build()
    return L.lib()


def test_block_gradient_symbols_are_declared_and_exported(lib):
    from mini_opt_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "mini_opt_hip.h")).read()
    declared = set(re.findall(r"\b(mo_[a-z_]+)\s*\(", header))
    for name in ("mo_qp_gradients_blocks", "mo_qp_gradients_eq_blocks"):
        assert name in declared and name in L.EXPORTS and hasattr(lib, name)
    major = int(re.search(r"#define\s+MO_VERSION_MAJOR\s+(\d+)", header).group(1))
    minor = int(re.search(r"#define\s+MO_VERSION_MINOR\s+(\d+)", header).group(1))
    assert (major, minor) >= (0, 3)
    assert f"{major}.{minor}".encode() in lib.mo_version_string()


def test_block_grads_mirror_matches_the_header_layout(tmp_path):
    from mini_opt_amd import _lib as L
    fields = [f for f, _ in L.BlockGrads._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mini_opt_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(mo_block_grads));']
    lines += [f'  printf("{f} %zu\\n", offsetof(mo_block_grads, {f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "bgrads.c", tmp_path / "bgrads"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["size"]) == C.sizeof(L.BlockGrads)
    for f in fields:
        assert int(out[f]) == getattr(L.BlockGrads, f).offset, f


def test_block_gradient_argument_errors_without_gpu(lib):
    """Both calls judge their arguments before they look at the plan or the layout, so the documented errors need no device."""
    from mini_opt_amd import _lib as L
    p16, p32, lay = C.c_void_p(16), C.c_void_p(32), C.c_void_p(64)
    out = L.BlockGrads()
    ref = C.byref(out)
    call = lib.mo_qp_gradients_blocks
    for args, name in (((None, lay, p16, 4, p16, 2, 1, p16, 8, p32, 8, ref, None), b"plan"),
                       ((None, None, p16, 4, p16, 2, 1, p16, 8, p32, 8, ref, None), b"layout"),
                       ((None, lay, p16, 4, p16, 2, 1, None, 8, p32, 8, ref, None), b"vars"),
                       ((None, lay, p16, 4, p16, 2, 1, p16, 8, None, 8, ref, None), b"u is"),
                       ((None, lay, p16, 4, p16, 2, 1, p16, 8, p32, 8, None, None), b"out"),
                       ((None, lay, p16, 4, p16, 2, -1, p16, 8, p32, 8, ref, None), b"batch")):
        assert call(*args) == -1, name
        assert name in lib.mo_last_error(), (name, lib.mo_last_error())
    out.dJ_blocks = 16
    assert call(None, lay, None, 4, p16, 2, 1, p16, 8, p32, 8, ref, None) == -1          # dJ_blocks without J_blocks
    assert b"J_blocks" in lib.mo_last_error()
    call = lib.mo_qp_gradients_eq_blocks
    for args, name in (((None, lay, 1, p16, 8, p32, 8, p16, 4, p16, 2, None), b"plan"),
                       ((None, None, 1, p16, 8, p32, 8, p16, 4, p16, 2, None), b"layout"),
                       ((None, lay, 1, None, 8, p32, 8, p16, 4, p16, 2, None), b"vars"),
                       ((None, lay, 1, p16, 8, None, 8, p16, 4, p16, 2, None), b"u is")):
        assert call(*args) == -1, name
        assert name in lib.mo_last_error(), (name, lib.mo_last_error())


def test_block_front_end_is_exported():
    import mini_opt_amd
    for name in ("qp_gradients_blocks", "qp_gradients_eq_blocks", "solve_qp"):
        assert callable(getattr(mini_opt_amd, name))
