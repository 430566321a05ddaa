"""CPU checks of the per-row weights of residual-block costs: the three entry points of the C ABI (symbols, struct layouts, argument errors
without a GPU) and the numpy restatement the GPU tests are held to (tests/weighted_blocks_reference.py) -- its gradients against torch
autograd through a torch restatement of the weighted pair rule, the transpose identity between its tangent and its gradients, and the
pair-rule correction of dweights, which the n = 7 layout must exercise."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import weighted_blocks_reference as WR
from tests.sens_fixtures import N7_COST, random_layout

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("mo_linearize_blocks_weighted", "mo_qp_gradients_blocks_weighted", "mo_qp_tangent_rhs_blocks_weighted")
LAM = 0.1


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from mini_opt_amd import _lib as L
    L.build()
    return L.lib()


def test_weighted_symbols_are_declared_exported_and_version_stays(lib):
    from mini_opt_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "mini_opt_hip.h")).read()
    declared = set(re.findall(r"\b(mo_[a-z_]+)\s*\(", header))
    dynamic = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH]).decode()
    for name in NAMES:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name)
        assert re.search(rf"\bT {name}\b", dynamic), name
    major = int(re.search(r"#define\s+MO_VERSION_MAJOR\s+(\d+)", header).group(1))
    minor = int(re.search(r"#define\s+MO_VERSION_MINOR\s+(\d+)", header).group(1))
    assert (major, minor) == (0, 5) and b"0.5" in lib.mo_version_string()


@pytest.mark.parametrize("mirror, ctype", [("BlockWeightedGrads", "mo_block_weighted_grads"), ("BlockWeightedTangents", "mo_block_weighted_tangents")])
def test_weighted_struct_mirrors_match_the_header_layout(tmp_path, mirror, ctype):
    from mini_opt_amd import _lib as L
    S = getattr(L, mirror)
    fields = [f for f, _ in S._fields_]
    assert fields[-2:] == ["dweights", "dweights_stride"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mini_opt_hip.h"', "int main(void) {", f'  printf("size %zu\\n", sizeof({ctype}));']
    lines += [f'  printf("{f} %zu\\n", offsetof({ctype}, {f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "w.c", tmp_path / "w"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["size"]) == C.sizeof(S)
    for f in fields:
        assert int(out[f]) == getattr(S, f).offset, f
    # the members the sibling's struct has sit where the sibling has them
    sibling = L.BlockGrads if mirror == "BlockWeightedGrads" else L.BlockTangents
    for f, _ in sibling._fields_:
        assert getattr(S, f).offset == getattr(sibling, f).offset, f


def test_weighted_argument_errors_without_gpu(lib):
    """The calls judge their arguments before they look at the plan or the layout, so the documented errors need no device: the plan is NULL
    in every call.  dweights without weights names `weights`."""
    from mini_opt_amd import _lib as L
    p16, p32, p48, lay = C.c_void_p(16), C.c_void_p(32), C.c_void_p(48), C.c_void_p(64)

    def expect(rc, name):
        assert rc == -1, (name, rc)
        assert name in lib.mo_last_error(), (name, lib.mo_last_error())

    lin = lib.mo_linearize_blocks_weighted
    expect(lin(None, lay, p16, 4, p16, 2, p48, 2, 0.0, None, 0, 1, p16, 4, 2, p16, 2, None, None), b"plan")
    expect(lin(None, lay, p16, 4, p16, 2, None, 0, 0.0, None, 0, 1, p16, 4, 2, p16, 2, None, None), b"plan")       # the sibling's judgement
    g = L.BlockWeightedGrads()
    ref = C.byref(g)
    grad = lib.mo_qp_gradients_blocks_weighted
    for args, name in (((None, None, p16, 4, p16, 2, p48, 2, 1, p16, 8, p32, 8, ref, None), b"layout"),
                       ((None, lay, p16, 4, p16, 2, p48, 2, 1, None, 8, p32, 8, ref, None), b"vars"),
                       ((None, lay, p16, 4, p16, 2, p48, 2, 1, p16, 8, None, 8, ref, None), b"u is"),
                       ((None, lay, p16, 4, p16, 2, p48, 2, 1, p16, 8, p32, 8, None, None), b"out"),
                       ((None, lay, p16, 4, p16, 2, None, 0, 1, p16, 8, p32, 8, None, None), b"out"),
                       ((None, lay, p16, 4, p16, 2, p48, 2, -1, p16, 8, p32, 8, ref, None), b"batch"),
                       ((None, lay, p16, 4, p16, 2, p48, 2, 1, p16, 8, p32, 8, ref, None), b"plan")):
        expect(grad(*args), name)
    g.dweights = 16
    expect(grad(None, lay, p16, 4, p16, 2, None, 0, 1, p16, 8, p32, 8, ref, None), b"weights")      # dweights without weights
    expect(grad(None, lay, None, 4, p16, 2, p48, 2, 1, p16, 8, p32, 8, ref, None), b"J_blocks")     # dweights without J_blocks
    t = L.BlockWeightedTangents()
    ref = C.byref(t)
    tan = lib.mo_qp_tangent_rhs_blocks_weighted
    for args, name in (((None, lay, p16, 4, p16, 2, p48, 2, None, None, 0, 1, p16, 8, None, p32, 8, None), b"t is"),
                       ((None, lay, p16, 4, p16, 2, p48, 2, None, None, 0, 1, None, 8, ref, p32, 8, None), b"vars"),
                       ((None, lay, p16, 4, p16, 2, p48, 2, None, None, 0, 1, p16, 8, ref, None, 8, None), b"rho"),
                       ((None, lay, p16, 4, p16, 2, p48, 2, None, None, 0, -1, p16, 8, ref, p32, 8, None), b"batch"),
                       ((None, None, p16, 4, p16, 2, p48, 2, None, None, 0, 1, p16, 8, ref, p32, 8, None), b"cost_layout"),
                       ((None, lay, p16, 4, p16, 2, p48, 2, None, None, 0, 1, p16, 8, ref, p32, 8, None), b"plan")):
        expect(tan(*args), name)
    t.dweights = 16
    expect(tan(None, lay, p16, 4, p16, 2, None, 0, None, None, 0, 1, p16, 8, ref, p32, 8, None), b"weights")       # dweights without weights
    expect(tan(None, lay, None, 4, p16, 2, p48, 2, None, None, 0, 1, p16, 8, ref, p32, 8, None), b"J_blocks")
    t.dweights, t.dcons_a = None, 16
    expect(tan(None, lay, p16, 4, p16, 2, p48, 2, None, None, 0, 1, p16, 8, ref, p32, 8, None), b"cons_var")


def test_weighted_front_end_is_exported_and_the_unweighted_tables_stay():
    import mini_opt_amd
    from mini_opt_amd import diff as D
    for name in ("qp_gradients_blocks_weighted", "qp_tangent_rhs_blocks_weighted", "qp_jvp_blocks_weighted", "solve_qp"):
        assert callable(getattr(mini_opt_amd, name))
    assert tuple(D._BLOCK) == ("J_blocks", "r", "lam", "J_eq_blocks", "r_eq", "cons_a", "cons_b") == D.QPSolveBlocksFunction.NAMES
    assert D.QPSolveWeightedBlocksFunction.NAMES == D.QPSolveBlocksFunction.NAMES + ("weights",)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def layouts():
    return [("n7", 7, N7_COST), ("n33", 33, random_layout(np.random.default_rng(33), 33, 14, repeats=True))]


def draw(rng, n, blocks, k=2):
    """Well conditioned by construction: G = J^T W J + 0.1 I with w in [0.5, 2], A_eq Gaussian."""
    Js = [rng.uniform(-1, 1, (R, len(idx))) for idx, R in blocks]
    rs = [rng.uniform(-1, 1, R) for _, R in blocks]
    ws = [rng.uniform(0.5, 2.0, R) for _, R in blocks]
    return Js, rs, ws, rng.normal(size=(k, n)), rng.uniform(-0.5, 0.5, k), rng.normal(size=n + k)


def torch_solution(n, blocks, Js, rs, ws, lam, A, b):
    """v = [x | y] of  min 1/2 x^T G x + c^T x  s.t.  A x + b = 0  through a torch restatement of the weighted pair rule and
    torch.linalg.solve on K = [[G, -A^T], [A, 0]]: F(v) = K v + [c | b] = 0."""
    G = torch.zeros(n, n, dtype=torch.float64)
    c = torch.zeros(n, dtype=torch.float64)
    rows, cols, vals = [], [], []
    for (idx, _), J, r, w in zip(blocks, Js, rs, ws):
        for p in range(len(idx)):
            for q in range(p + 1):
                i, j = idx[p], idx[q]
                rows.append(max(i, j)); cols.append(min(i, j)); vals.append((w * J[:, p] * J[:, q]).sum())
            c = c.index_add(0, torch.tensor([idx[p]]), (w * J[:, p] * r).sum().reshape(1))
    G = G.index_put((torch.tensor(rows), torch.tensor(cols)), torch.stack(vals), accumulate=True)
    G = G + torch.diag(lam.expand(n))
    Gs = G + G.T - torch.diag(torch.diagonal(G))
    k = A.shape[0]
    K = torch.cat([torch.cat([Gs, -A.T], 1), torch.cat([A, torch.zeros(k, k, dtype=torch.float64)], 1)], 0)
    return torch.linalg.solve(K, -torch.cat([c, b])), K


def autograd_case(n, blocks, seed, correction=True):
    """(worst relative error per member, cond K): the restatement's gradients against torch autograd of l = g . v."""
    rng = np.random.default_rng(seed)
    Js, rs, ws, A, b, g = draw(rng, n, blocks)
    leaf = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    tJ, tr, tw, tlam = [leaf(J) for J in Js], [leaf(r) for r in rs], [leaf(w) for w in ws], leaf(np.array(LAM))
    v, K = torch_solution(n, blocks, tJ, tr, tw, tlam, torch.tensor(A), torch.tensor(b))
    (v @ torch.tensor(g)).backward()
    Kn = K.detach().numpy()
    u = np.linalg.solve(Kn.T, g)
    dJ, dr, dlam, dw = WR.gradients(blocks, Js, rs, ws, v.detach().numpy()[:n], u[:n], correction=correction)
    rel = lambda got, want: float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    worst = dict(J=rel(WR.pack(dJ), WR.pack([t.grad.numpy() for t in tJ])), r=rel(np.concatenate(dr), np.concatenate([t.grad.numpy() for t in tr])),
                 lam=abs(dlam - float(tlam.grad)) / abs(float(tlam.grad)), w=rel(np.concatenate(dw), np.concatenate([t.grad.numpy() for t in tw])))
    return worst, float(np.linalg.cond(Kn))


@pytest.mark.parametrize("tag, n, blocks", layouts(), ids=["n7", "n33"])
def test_weighted_gradients_against_torch_autograd(tag, n, blocks):
    """dJ, dr, dlambda and dw to 1e-10 relative: the systems are well conditioned by construction (cond < 1e4 asserted), so autograd's own
    error is some 1e4 x 2^-53 ~ 1e-12 of the largest entry."""
    worst, cond = autograd_case(n, blocks, 4100 + n)
    print(f"{tag}: cond K = {cond:.3e}, worst relative errors {worst}")
    assert cond < 1e4
    assert max(worst.values()) < 1e-10, worst


def test_dweights_needs_the_pair_rule_correction_on_n7():
    """Without the correction dw = -s t is the dense J^T W J's: wrong on the blocks (3, 0, 5, 3) and (2, 2), right everywhere else."""
    worst, _ = autograd_case(7, N7_COST, 4107, correction=False)
    assert worst["w"] > 1e-6 and max(worst["J"], worst["r"], worst["lam"]) < 1e-10, worst
    blocks = [(idx, R) for idx, R in N7_COST if len(set(idx)) == len(idx)]
    worst, _ = autograd_case(7, blocks, 4107, correction=False)
    assert max(worst.values()) < 1e-10, worst


@pytest.mark.parametrize("tag, n, blocks", layouts(), ids=["n7", "n33"])
def test_weighted_transpose_identity(tag, n, blocks):
    """u^T rho(thetadot) = -sum over J, r, lam, w of <dl/dtheta, thetadot> for random u, x and random directions, to 1e-12 relative (of the
    sum of the magnitudes of both sides' terms); one weight is 0 with a direction in it, one is 0 without."""
    rng = np.random.default_rng(4200 + n)
    Js, rs, ws, _, _, _ = draw(rng, n, blocks)
    ws[0][0] = 0.0
    ws[-1][-1] = 0.0
    x, u = rng.normal(size=n), rng.normal(size=n)
    t = {"J_blocks": [rng.normal(size=J.shape) for J in Js], "r": [rng.normal(size=r.shape) for r in rs],
         "weights": [rng.normal(size=w.shape) for w in ws], "lam": rng.normal()}
    t["weights"][-1][-1] = 0.0
    dJ, dr, dlam, dw = WR.gradients(blocks, Js, rs, ws, x, u)
    for keys in (("J_blocks", "r", "weights", "lam"), ("weights",), ("J_blocks",), ("r", "lam")):
        sub = {key: t[key] for key in keys}
        lhs = float(u @ WR.tangent_rhs(n, blocks, Js, rs, ws, x, sub))
        mag = float(np.abs(u) @ WR.tangent_rhs(n, blocks, Js, rs, ws, x, sub, absolute=True))
        grads = {"J_blocks": (WR.pack(dJ), WR.pack(t["J_blocks"])), "r": (np.concatenate(dr), np.concatenate(t["r"])),
                 "weights": (np.concatenate(dw), np.concatenate(t["weights"])), "lam": (np.array([dlam]), np.array([t["lam"]]))}
        rhs = -sum(float(grads[key][0] @ grads[key][1]) for key in keys)
        assert abs(lhs - rhs) <= 1e-12 * mag, (tag, keys, lhs, rhs)


def test_zero_weight_rows_never_enter_the_restatement():
    rng = np.random.default_rng(4300)
    Js, rs, ws, _, _, _ = draw(rng, 7, N7_COST)
    ws[2][1] = 0.0
    clean = WR.linearize(7, N7_COST, Js, rs, ws, LAM)
    Js[2][1, :] = np.nan
    rs[2][1] = np.inf
    got = WR.linearize(7, N7_COST, Js, rs, ws, LAM)
    assert all(np.array_equal(a, b) for a, b in zip(got, clean))
    dJ, dr, _, _ = WR.gradients(N7_COST, Js, rs, ws, rng.normal(size=7), rng.normal(size=7))
    assert np.all(dJ[2][1] == 0.0) and dr[2][1] == 0.0 and np.all(np.isfinite(WR.pack(dJ)))
