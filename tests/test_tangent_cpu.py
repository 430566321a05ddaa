"""CPU checks of the forward-mode sensitivities of a QP solve: the formulas of tests/tangent_reference.py pinned by central differences of
the numpy barrier problem of test_diff_cpu.py and by the adjoint identity against diff_reference.gradients (no product code involved),
and the new entry point of the C ABI (struct layout, argument errors without a GPU)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import diff_reference as R
from tests import tangent_reference as T
from tests import sens_fixed_problem as D

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
N, K, M, MR = D.N, D.K, D.M, D.MR


def problem():
    """The (8, 2, 5, 12) problem of test_diff_cpu.py with two rows moved onto one variable (a box on it)."""
    base, g = D.fixed_problem()
    base["var"] = base["var"].copy()
    base["var"][1] = base["var"][0]
    base["a"] = base["a"].copy()
    base["a"][0], base["a"][1] = abs(base["a"][0]), -abs(base["a"][1])   # lower and upper side of the box
    return base, g


def directions(seed, j_level):
    """One direction touching every member of the input level at once.  The G direction is NOT symmetric: only its lower triangle counts."""
    rng = np.random.default_rng(seed)
    d = dict(A=rng.normal(size=(K, N)), b_eq=rng.normal(size=K), a=rng.normal(size=M), b=rng.normal(size=M))
    if j_level:
        d.update(J=rng.normal(size=(MR, N)), r=rng.normal(size=MR), lam=float(rng.normal()))
    else:
        d.update(G=rng.normal(size=(N, N)), c=rng.normal(size=N))
    return d


def moved(th, d, h):
    """theta + h thetadot, in the keys test_diff_cpu.root reads."""
    out = dict(th)
    for key, val in d.items():
        if key == "G":
            out["G"] = th["G"] + h * T.sym_lower(val)
        elif key == "lam":
            out["lam"] = th["lam"] + h * val
        else:
            out[key] = th[key] + h * val
    return out


def levels():
    base, g = problem()
    G0, c0 = D.cost(base)
    th_qp = dict(G=G0, c=c0, A=base["A"], b_eq=base["b_eq"], var=base["var"], a=base["a"], b=base["b"])
    th_j = dict(base, lam=np.array([D.LAM]))
    return (("(G, c)", th_qp, False), ("(J, r, lam)", th_j, True)), g


def analytic(th, d, v, j_level):
    G, _ = D.cost(th)
    rho = T.rho(N, K, M, th["var"], v, d, J=th["J"] if j_level else None, r=th["r"] if j_level else None)
    return T.vdot(G, th["A"], th["var"], th["a"], v, rho), rho


def test_vdot_against_central_differences():
    """vdot = -K^-1 rho against (v*(theta + h thetadot) - v*(theta - h thetadot)) / 2h, h = 1e-6, of the damped-Newton root at fixed mu; three
    seeded directions per input level, every member moving at once.  Bound 1e-7 of max |vdot|, test_diff_cpu's bound for the same finite
    difference (measured: at most 7.3e-11 for (G, c) and 5.3e-11 for J-level)."""
    lv, _ = levels()
    worst = 0.0
    for name, th, j_level in lv:
        v = D.root(th)
        for seed in (1, 2, 3):
            d = directions(20261019 + seed, j_level)
            vd, _ = analytic(th, d, v, j_level)
            h = 1e-6
            fd = (D.root(moved(th, d, h), v) - D.root(moved(th, d, -h), v)) / (2 * h)
            err = np.max(np.abs(fd - vd)) / np.max(np.abs(vd))
            print(f"{name} direction {seed}: max |fd - vdot| / max |vdot| = {err:.3e} (max |vdot| = {np.max(np.abs(vd)):.3e})")
            worst = max(worst, err)
    assert worst < 1e-7, worst


def test_adjoint_identity_against_the_gradient_formulas():
    """g . vdot = sum over the members of <gradient, tangent> with the gradients of diff_reference.gradients: the tangent map is the exact
    transpose of the gradient map.  |lhs - rhs| <= 1e-12 (|lhs| + |rhs|), the project's bound for its transpose identity."""
    lv, g = levels()
    for name, th, j_level in lv:
        v = D.root(th)
        G, _ = D.cost(th)
        u = R.solve_transposed(R.kkt_matrix(G, th["A"], th["var"], th["a"], v), g)
        grads = R.gradients(N, K, M, th["var"], v, u, J=th["J"] if j_level else None, r=th["r"] if j_level else None)
        for seed in (1, 2, 3):
            d = directions(20261019 + seed, j_level)
            vd, _ = analytic(th, d, v, j_level)
            lhs = float(g @ vd)
            pairs = [("A_eq", d["A"]), ("b_eq", d["b_eq"]), ("cons_a", d["a"]), ("cons_b", d["b"])]
            pairs += [("J", d["J"]), ("r", d["r"]), ("lam", d["lam"])] if j_level else [("G", T.sym_lower(d["G"])), ("c", d["c"])]
            rhs = float(sum(np.sum(grads[key] * val) for key, val in pairs))
            print(f"{name} direction {seed}: g . vdot = {lhs:.15e}, sum <grad, tangent> = {rhs:.15e}, diff {abs(lhs - rhs):.1e}")
            assert abs(lhs - rhs) <= 1e-12 * (abs(lhs) + abs(rhs)), (name, seed, lhs, rhs)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from mini_opt_amd import _lib as L
    L.build()
    return L.lib()


def test_tangent_abi_layout_and_argument_errors(lib, tmp_path):
    """sizeof and every member's offset of mo_qp_tangents, as gcc sees them, against the ctypes mirror; the symbol is declared, exported and
    mirrored; and every documented argument error is returned with a NULL plan: the call judges its arguments before it looks at the plan,
    so none of them needs a device."""
    from mini_opt_amd import _lib as L
    assert "mo_qp_tangent_rhs" in L.EXPORTS and hasattr(lib, "mo_qp_tangent_rhs")
    fields = [f for f, _ in L.QPTangents._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mini_opt_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(mo_qp_tangents));']
    lines += [f'  printf("{f} %zu\\n", offsetof(mo_qp_tangents, {f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "tangents.c", tmp_path / "tangents"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["size"]) == C.sizeof(L.QPTangents)
    for f in fields:
        assert int(out[f]) == getattr(L.QPTangents, f).offset, f

    p16, p32 = C.c_void_p(16), C.c_void_p(32)
    qp = L.Problem()
    qp.G, qp.G_stride, qp.G_ld, qp.c, qp.c_stride = 16, 64, 8, 16, 8
    jl = L.Problem()
    jl.J, jl.J_stride, jl.J_ld, jl.J_layout, jl.r, jl.r_stride = 16, 96, 8, L.MO_ROW_MAJOR, 16, 12

    def call(prob, t, vars_=p16, rho=p32):
        rc = lib.mo_qp_tangent_rhs(None, None if prob is None else C.byref(prob), 1, vars_, 22, None if t is None else C.byref(t), rho, 22, None)
        return rc, lib.mo_last_error()

    def tangents(**members):
        t = L.QPTangents()
        for key, val in members.items():
            setattr(t, key, val)
        return t

    INVALID = -1
    assert call(qp, tangents()) == (INVALID, b"plan is NULL")                      # everything else in order: only the plan is missing
    assert call(jl, tangents(dJ=16, dJ_stride=96, dJ_ld=8, dr=16, dr_stride=12, dlambda=16, dlambda_stride=1)) == (INVALID, b"plan is NULL")
    for (rc, msg), word in ((call(None, tangents()), b"problem"), (call(qp, None), b"t is NULL"), (call(qp, tangents(), vars_=None), b"vars"),
                            (call(qp, tangents(), rho=None), b"rho")):
        assert rc == INVALID and word in msg and b"plan" not in msg, (rc, msg)
    cases = [
        (jl, tangents(dG=16, dG_stride=64, dG_ld=8), b"dG"),                        # dG with J-level input
        (qp, tangents(dJ=16, dJ_stride=96, dJ_ld=8), b"dJ"),                        # dJ / dr / dlambda with (G, c) input: prob->J is NULL
        (qp, tangents(dr=16, dr_stride=12), b"dr"),
        (qp, tangents(dlambda=16, dlambda_stride=1), b"dlambda"),
        (qp, tangents(dcons_a=16, dcons_stride=5), b"cons_var"),                    # dcons_a without cons_var
    ]
    no_r = L.Problem()
    no_r.J, no_r.J_stride, no_r.J_ld, no_r.J_layout = 16, 96, 8, L.MO_ROW_MAJOR
    cases.append((no_r, tangents(dJ=16, dJ_stride=96, dJ_ld=8), b"prob->r"))        # dJ without prob->r
    for prob, t, word in cases:
        rc, msg = call(prob, t)
        assert rc == INVALID and word in msg and b"plan is NULL" not in msg, (rc, msg, word)
    # dr alone needs no prob->r (w = J x + r multiplies dJ only): the arguments pass, the plan is what is missing
    assert call(no_r, tangents(dr=16, dr_stride=12)) == (INVALID, b"plan is NULL")
    # the Python front end
    import mini_opt_amd
    for name in ("qp_tangent_rhs", "qp_jvp", "tangent_status"):
        assert callable(getattr(mini_opt_amd, name))
    assert hasattr(mini_opt_amd.QPSolveFunction, "jvp")
