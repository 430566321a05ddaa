"""CPU checks of forward mode for residual-block input: the pair-by-pair formulas of tests/blocks_tangent_reference.py pinned by central
differences of blocks_diff_reference.linearize / jacobian fed through tangent_reference.rho for (G, c) input, and by the transpose identity
against the block gradient formulas (no product code involved); then the new entry point of the C ABI (declared, exported, mirrored,
version 0.5, argument errors without a GPU)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import blocks_diff_reference as BR
from tests import blocks_tangent_reference as BT
from tests import diff_reference as R
from tests import tangent_reference as T

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
N = 7
N7_COST = [((3, 0, 5, 3), 3), ((6,), 2), ((1, 2, 4, 0, 6), 4), ((2, 2), 1), ((5, 4, 1), 6)]   # the layout of the block backward tests
N7_EQ = [((0, 4, 0), 1), ((2, 6, 1), 1)]      # the first local column of block 0 loses variable 0 to the last
K, M = 2, 3
VAR = np.array([2, 2, 5])                     # a pair of rows on one variable
LAM = 0.1
LD = np.longdouble                            # (numpy's long double: the x87 format here, plain double where the platform has no other)


def problem(seed):
    rng = np.random.default_rng(seed)
    Js = [rng.uniform(-1, 1, (R_, len(idx))) for idx, R_ in N7_COST]
    rs = [rng.uniform(-1, 1, R_) for _, R_ in N7_COST]
    Jeq = [rng.uniform(-1, 1, (R_, len(idx))) for idx, R_ in N7_EQ]
    v = rng.normal(size=N + 2 * M + K)
    return Js, rs, Jeq, v


def direction(seed):
    rng = np.random.default_rng(seed)
    d = {"J_blocks": [rng.normal(size=(R_, len(idx))) for idx, R_ in N7_COST], "r": [rng.normal(size=R_) for _, R_ in N7_COST],
         "lam": float(rng.normal()), "J_eq_blocks": [rng.normal(size=(R_, len(idx))) for idx, R_ in N7_EQ], "r_eq": rng.normal(size=K),
         "a": rng.normal(size=M), "b": rng.normal(size=M)}
    return d


def test_block_rho_against_central_differences_of_the_linearisation():
    """dG, dc, dA_eq as central differences (h = 1e-6, test_tangent_cpu's step) of linearize / jacobian along the packed direction, fed through
    tangent_reference.rho for (G, c) input, against the block formulas.  linearize is quadratic and jacobian linear in the packed values, so
    the central difference has no truncation error; the quotient is formed and the formulas are evaluated in long double, and what is left is
    the rounding of linearize itself (double) over h, about 1e-10.  Bound 1e-7 of max |rho|, test_tangent_cpu's bound for the same step."""
    worst = 0.0
    for seed in (1, 2, 3):
        Js, rs, Jeq, v = problem(100 + seed)
        d = direction(200 + seed)
        d["J_eq_blocks"][0][:, 0] = np.nan                       # the losing column: must not reach rho
        h = 1e-6
        lin = lambda s: BR.linearize(N, N7_COST, [J + s * dJ for J, dJ in zip(Js, d["J_blocks"])], [r + s * dr for r, dr in zip(rs, d["r"])],
                                     LAM + s * d["lam"])
        dJe_clean = [np.nan_to_num(a) for a in d["J_eq_blocks"]]   # (jacobian copies every column before a later one overwrites it)
        jac = lambda s: BR.jacobian(N, N7_EQ, [J + s * dJ for J, dJ in zip(Jeq, dJe_clean)])
        (Gp, cp), (Gm, cm) = lin(h), lin(-h)
        two_h = LD(2) * LD(h)
        dG = (Gp.astype(LD) - Gm.astype(LD)) / two_h
        dc = (cp.astype(LD) - cm.astype(LD)) / two_h
        dA = (jac(h).astype(LD) - jac(-h).astype(LD)) / two_h
        want = T.rho(N, K, M, VAR, v.astype(LD), {"G": dG, "c": dc, "A": dA, "b_eq": d["r_eq"], "a": d["a"], "b": d["b"]})
        got = BT.rho(N, K, M, N7_COST, Js, rs, v.astype(LD), d, eq_blocks=N7_EQ, var=VAR)
        assert np.all(np.isfinite(got.astype(np.float64)))
        err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        print(f"direction {seed}: max |block rho - rho of the differenced linearisation| / max |rho| = {err:.3e}")
        worst = max(worst, err)
        # every member alone adds up to all together (rho is linear in the direction)
        parts = sum(BT.rho(N, K, M, N7_COST, Js, rs, v, {key: d[key]}, eq_blocks=N7_EQ, var=VAR) for key in d)
        assert np.max(np.abs(parts - got.astype(np.float64))) <= 1e-13 * np.max(np.abs(want.astype(np.float64)))
    assert worst < 1e-7, worst


def test_transpose_identity_against_the_block_gradient_formulas():
    """u . rho = -sum over the members of <gradient from u, tangent> with gradients_blocks, gradients_eq_blocks and diff_reference.gradients
    (cons_a, cons_b) at the same (vars, u), for random u.  |lhs - rhs| <= 1e-12 (|lhs| + |rhs|), the project's bound for its transpose
    identities."""
    for seed in (1, 2, 3):
        Js, rs, Jeq, v = problem(300 + seed)
        d = direction(400 + seed)
        rng = np.random.default_rng(500 + seed)
        u = rng.normal(size=v.shape)
        x, _, y, _ = R.split(v, N, K, M)
        ux, _, uy, _ = R.split(u, N, K, M)
        dJ, dr, dlam = BR.gradients_blocks(N7_COST, Js, rs, x, ux)
        dJe, dre = BR.gradients_eq_blocks(N7_EQ, x, ux, y, uy)
        cons = R.gradients(N, K, M, VAR, v, u)
        assert dJe[0][0, 0] == 0.0                                # the loser's gradient is exactly 0 ...
        d["J_eq_blocks"][0][:, 0] = 1e30                          # ... and its tangent reaches nothing
        rhs = -(sum(np.sum(a * b) for a, b in zip(dJ, d["J_blocks"])) + sum(a @ b for a, b in zip(dr, d["r"])) + dlam * d["lam"]
                + sum(np.sum(a * b) for a, b in zip(dJe, d["J_eq_blocks"])) + dre @ d["r_eq"] + cons["cons_a"] @ d["a"] + cons["cons_b"] @ d["b"])
        lhs = float(u @ BT.rho(N, K, M, N7_COST, Js, rs, v, d, eq_blocks=N7_EQ, var=VAR))
        print(f"direction {seed}: u . rho = {lhs:.15e}, -sum <grad, tangent> = {float(rhs):.15e}, diff {abs(lhs - rhs):.1e}")
        assert abs(lhs - rhs) <= 1e-12 * (abs(lhs) + abs(rhs)), (seed, lhs, rhs)


def test_absolute_variant_dominates_and_counts_are_positive():
    Js, rs, Jeq, v = problem(600)
    d = direction(601)
    got = BT.rho(N, K, M, N7_COST, Js, rs, v, d, eq_blocks=N7_EQ, var=VAR)
    mag = BT.rho(N, K, M, N7_COST, Js, rs, v, d, eq_blocks=N7_EQ, var=VAR, absolute=True)
    assert np.all(mag >= np.abs(got)) and np.all(mag[:N] > 0)
    cnt = BT.term_counts(N, K, M, N7_COST, N7_EQ, VAR)
    assert cnt.shape == got.shape and np.all(cnt[:N] >= 8) and np.all(cnt[N:N + M] == 0)
    bad = BT.rho(N, K, M, N7_COST, Js, rs, v, d, eq_blocks=N7_EQ, var=np.array([2, -1, 5]))
    assert np.isnan(bad[N + M + K + 1]) and np.sum(np.isnan(bad)) == 1


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from mini_opt_amd import _lib as L
    L.build()
    return L.lib()


def test_block_tangent_symbol_is_declared_exported_and_versioned(lib):
    from mini_opt_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "mini_opt_hip.h")).read()
    declared = set(re.findall(r"\b(mo_[a-z_]+)\s*\(", header))
    assert "mo_qp_tangent_rhs_blocks" in declared and "mo_qp_tangent_rhs_blocks" in L.EXPORTS and hasattr(lib, "mo_qp_tangent_rhs_blocks")
    exported = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH]).decode()
    assert re.search(r"\bT mo_qp_tangent_rhs_blocks\b", exported)
    major = int(re.search(r"#define\s+MO_VERSION_MAJOR\s+(\d+)", header).group(1))
    minor = int(re.search(r"#define\s+MO_VERSION_MINOR\s+(\d+)", header).group(1))
    assert (major, minor) == (0, 5)
    assert b"0.5" in lib.mo_version_string()
    import mini_opt_amd
    for name in ("qp_tangent_rhs_blocks", "qp_jvp_blocks"):
        assert callable(getattr(mini_opt_amd, name))
    assert hasattr(mini_opt_amd.QPSolveBlocksFunction, "jvp")


def test_block_tangents_mirror_matches_the_header_layout(tmp_path):
    from mini_opt_amd import _lib as L
    fields = [f for f, _ in L.BlockTangents._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mini_opt_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(mo_block_tangents));']
    lines += [f'  printf("{f} %zu\\n", offsetof(mo_block_tangents, {f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "btangents.c", tmp_path / "btangents"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["size"]) == C.sizeof(L.BlockTangents)
    for f in fields:
        assert int(out[f]) == getattr(L.BlockTangents, f).offset, f


def test_block_tangent_argument_errors_without_gpu(lib):
    """The call judges its arguments before it looks at the plan or the layouts, so every MO_ERR_INVALID_ARGUMENT of the header is returned
    with a NULL plan and needs no device."""
    from mini_opt_amd import _lib as L
    p16, p32, lay, eq = C.c_void_p(16), C.c_void_p(32), C.c_void_p(64), C.c_void_p(128)

    def call(t, cost=lay, J=p16, r=p16, eq_layout=eq, cons_var=p16, vars_=p16, rho=p32, batch=1):
        rc = lib.mo_qp_tangent_rhs_blocks(None, cost, J, 4, r, 2, eq_layout, cons_var, 3, batch, vars_, 22, None if t is None else C.byref(t),
                                          rho, 22, None)
        return rc, lib.mo_last_error()

    def tangents(**members):
        t = L.BlockTangents()
        for key, val in members.items():
            setattr(t, key, val)
        return t

    INVALID = -1
    everything = tangents(dJ_blocks=16, dJ_stride=4, dr=16, dr_stride=2, dlambda=16, dlambda_stride=1, dJ_eq_blocks=16, dJ_eq_stride=3,
                          dr_eq=16, dr_eq_stride=2, dcons_a=16, dcons_b=16, dcons_stride=3)
    assert call(everything) == (INVALID, b"plan is NULL")       # everything else in order: only the plan is missing
    assert call(tangents(), J=None, r=None, eq_layout=None, cons_var=None) == (INVALID, b"plan is NULL")
    for (rc, msg), word in ((call(tangents(), cost=None), b"cost_layout"), (call(None), b"t is NULL"), (call(tangents(), vars_=None), b"vars"),
                            (call(tangents(), rho=None), b"rho"), (call(tangents(), batch=-1), b"batch"),
                            (call(tangents(dJ_blocks=16), J=None), b"J_blocks"), (call(tangents(dJ_blocks=16), r=None), b"J_blocks"),
                            (call(tangents(dr=16), J=None), b"J_blocks"), (call(tangents(dr=16), r=None), b"J_blocks"),
                            (call(tangents(dJ_eq_blocks=16), eq_layout=None), b"eq_layout"),
                            (call(tangents(dr_eq=16), eq_layout=None), b"eq_layout"),
                            (call(tangents(dcons_a=16), cons_var=None), b"cons_var")):
        assert rc == INVALID and word in msg and b"plan is NULL" not in msg, (rc, msg, word)
    # dcons_b alone needs no cons_var, dlambda no blocks
    assert call(tangents(dcons_b=16, dlambda=16), J=None, r=None, cons_var=None) == (INVALID, b"plan is NULL")
