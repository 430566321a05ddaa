"""CPU checks of the differentiable QP: the formulas (pinned by central differences on a numpy barrier problem, no product code involved)
and the two new entry points of the C ABI (symbols, struct layout, argument errors without a GPU)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import diff_reference as R
from tests.sens_fixed_problem import LAM, M, K, N, cost, fixed_problem, root

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
def central_difference(th, key, idx, g, v_star, h=1e-6, symmetric=False):
    vals = []
    for sign in (1.0, -1.0):
        t = {k_: (np.array(v_, dtype=float, copy=True) if isinstance(v_, np.ndarray) and v_.dtype.kind == "f" else v_) for k_, v_ in th.items()}
        t[key][idx] += sign * h
        if symmetric and idx[0] != idx[1]:
            t[key][idx[::-1]] += sign * h
        vals.append(g @ root(t, v_star))
    return (vals[0] - vals[1]) / (2 * h)


def test_formulas_against_central_differences():
    """l(theta) = g . v*(theta): every entry of c, G (symmetric perturbation), A_eq, b_eq, a, b with (G, c) input and of J, r (and lam) with
    J-level input.  Bound 1e-7 of the group's largest gradient entry: ~50 x the finite-difference round-off eps |l| / h ~ 1e-9 at gradients of
    order 1, seven digits below a wrong sign or a missing factor 1/2."""
    base, g = fixed_problem()
    G0, c0 = cost(base)
    th_qp = dict(G=G0.copy(), c=c0.copy(), A=base["A"], b_eq=base["b_eq"], var=base["var"], a=base["a"], b=base["b"])
    v = root(th_qp)
    Kmat = R.kkt_matrix(G0, base["A"], base["var"], base["a"], v)
    u = R.solve_transposed(Kmat, g)
    # the transpose identity the kernel uses
    _, s, _, _ = R.split(v, N, K, M)
    u2 = R.transposed_through_direct(Kmat, g, N, K, M, s)
    assert np.max(np.abs(u2 - u)) <= 1e-12 * np.max(np.abs(u)), np.max(np.abs(u2 - u))
    u3 = R.transposed_through_reduced(G0, base["A"], base["var"], base["a"], v, g)
    assert np.max(np.abs(u3 - u)) <= 1e-10 * np.max(np.abs(u))
    grads = R.gradients(N, K, M, base["var"], v, u, J=base["J"], r=base["r"])
    worst = {}

    def group(name, th, key, analytic, symmetric=False):
        fd = np.zeros_like(analytic)
        for idx in np.ndindex(*analytic.shape):
            fd[idx] = central_difference(th, key, idx, g, v, symmetric=symmetric)
        want = analytic
        if symmetric:   # both mirror entries move: dG[i][j] + dG[j][i]
            want = analytic + analytic.T - np.diag(np.diag(analytic))
        err = np.max(np.abs(fd - want)) / np.max(np.abs(want))
        worst[name] = err
        print(f"{name}: max |fd - analytic| / max |analytic| = {err:.3e} (max |analytic| = {np.max(np.abs(want)):.3e})")

    group("c", th_qp, "c", grads["c"])
    group("G", th_qp, "G", grads["G"], symmetric=True)
    group("A_eq", th_qp, "A", grads["A_eq"])
    group("b_eq", th_qp, "b_eq", grads["b_eq"])
    group("cons_a", th_qp, "a", grads["cons_a"])
    group("cons_b", th_qp, "b", grads["cons_b"])
    th_j = dict(base, lam=np.array([LAM]))
    assert np.max(np.abs(root(th_j, v) - v)) < 1e-12
    group("J", th_j, "J", grads["J"])
    group("r", th_j, "r", grads["r"])
    group("lam", th_j, "lam", np.array([grads["lam"]]))
    assert max(worst.values()) < 1e-7, worst


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from mini_opt_amd import _lib as L
    L.build()
    return L.lib()


def test_new_symbols_are_declared_and_exported(lib):
    from mini_opt_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "mini_opt_hip.h")).read()
    declared = set(re.findall(r"\b(mo_[a-z_]+)\s*\(", header))
    for name in ("mo_kkt_solve", "mo_qp_gradients"):
        assert name in declared and name in L.EXPORTS and hasattr(lib, name)
    assert re.search(r"#define\s+MO_KKT_TRANSPOSE\s+4u", header) and L.MO_KKT_TRANSPOSE == 4


def test_version_grew_with_the_abi(lib):
    header = open(os.path.join(ROOT, "include", "mini_opt_hip.h")).read()
    major = int(re.search(r"#define\s+MO_VERSION_MAJOR\s+(\d+)", header).group(1))
    minor = int(re.search(r"#define\s+MO_VERSION_MINOR\s+(\d+)", header).group(1))
    assert (major, minor) >= (0, 2)
    assert f"{major}.{minor}".encode() in lib.mo_version_string() and b"0.1 " not in lib.mo_version_string()


def test_qp_grads_mirror_matches_the_header_layout(tmp_path):
    from mini_opt_amd import _lib as L
    fields = [f for f, _ in L.QPGrads._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mini_opt_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(mo_qp_grads));']
    lines += [f'  printf("{f} %zu\\n", offsetof(mo_qp_grads, {f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "grads.c", tmp_path / "grads"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["size"]) == C.sizeof(L.QPGrads)
    for f in fields:
        assert int(out[f]) == getattr(L.QPGrads, f).offset, f


def test_argument_errors_without_gpu(lib):
    """Both calls judge their arguments before they look at the plan, so the documented errors need no device."""
    from mini_opt_amd import _lib as L
    p16, p32, p48 = C.c_void_p(16), C.c_void_p(32), C.c_void_p(48)
    qp = L.Problem()
    qp.G, qp.G_stride, qp.G_ld, qp.c, qp.c_stride = 16, 64, 8, 16, 8
    assert lib.mo_kkt_solve(None, C.byref(qp), 1, p16, 8, p32, 8, 0, p48, 8, None, None) == -1                 # NULL plan
    assert b"plan" in lib.mo_last_error()
    assert lib.mo_kkt_solve(None, C.byref(qp), 1, p16, 8, None, 8, 0, p48, 8, None, None) == -1                # NULL rhs
    assert b"rhs" in lib.mo_last_error()
    assert lib.mo_kkt_solve(None, C.byref(qp), 1, p16, 8, p32, 8, 8, p48, 8, None, None) == -1                 # unknown flag
    assert b"flags" in lib.mo_last_error()
    assert lib.mo_kkt_solve(None, C.byref(qp), 1, p16, 8, p32, 8, 0, p32, 8, None, None) == -1                 # rhs aliases out
    assert b"alias" in lib.mo_last_error()
    grads = L.QPGrads()
    assert lib.mo_qp_gradients(None, C.byref(qp), 1, p16, 8, p16, 8, C.byref(grads), None) == -1              # NULL plan
    assert b"plan" in lib.mo_last_error()
    jl = L.Problem()
    jl.J, jl.J_stride, jl.J_ld, jl.J_layout, jl.r, jl.r_stride = 16, 32, 8, L.MO_ROW_MAJOR, 16, 4
    grads.dG, grads.dG_stride, grads.dG_ld = 16, 64, 8
    assert lib.mo_qp_gradients(None, C.byref(jl), 1, p16, 8, p16, 8, C.byref(grads), None) == -1              # dG with J-level input
    assert b"dG" in lib.mo_last_error()
    grads = L.QPGrads()
    grads.dJ, grads.dJ_stride, grads.dJ_ld, grads.dJ_layout = 16, 32, 8, L.MO_ROW_MAJOR
    assert lib.mo_qp_gradients(None, C.byref(qp), 1, p16, 8, p16, 8, C.byref(grads), None) == -1              # dJ with (G, c) input
    assert b"dJ" in lib.mo_last_error()
    assert lib.mo_qp_gradients(None, C.byref(qp), 1, p16, 8, p16, 8, None, None) == -1                        # NULL out
    assert b"out" in lib.mo_last_error()


def test_python_front_end_is_exported():
    import mini_opt_amd
    for name in ("solve_qp", "kkt_solve", "qp_gradients", "QPSolveFunction"):
        assert callable(getattr(mini_opt_amd, name))
