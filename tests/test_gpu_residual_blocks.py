"""Residual-block input on the device (mo_residual_layout_create, mo_linearize_blocks, mo_jacobian_blocks, mo_nls_solve_blocks): the
reference's own cost model -- a list of R x P local Jacobians over index lists (residual.hpp:60-250, nonlinear.cc:170-214) -- against its
known answers (residual_test.cc:51-182), the oracle's restatements of UpdateHessian / UpdateJacobian, the dense path and the NLS oracle."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from mini_opt_amd import _lib as L
from mini_opt_amd import nls as NLS
from mini_opt_amd import qp as Q
from oracle import nls_oracle as N
from oracle import oracle as orc
from tests import nls_problems as P

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"


def T(a, dt=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=DEV).contiguous()


def pack_np(Js):
    """[B, R, P] numpy blocks -> [B, sum R P], each block column-major."""
    return np.concatenate([J.transpose(0, 2, 1).reshape(J.shape[0], -1) for J in Js], axis=1)


def oracle_hessian(n, blocks, Js, rs, p):
    """sum_b orc_update_hessian for problem p: (H lower, b, half_sq)."""
    H = np.zeros((n, n), order="F")
    b = np.zeros(n)
    f = 0.0
    for (idx, _), J, r in zip(blocks, Js, rs):
        f += orc.update_hessian(list(idx), J[p], r[p], H, b)
    return H, b, f


def oracle_jacobian(n, blocks, Js, rs, p, ld):
    """orc_update_jacobian of every block into its rows of one (sum R) x n column-major matrix (QP::A_eq, nonlinear.cc:191-206)."""
    lib = orc.lib()
    out = np.zeros((n, ld))          # column-major: out[col, row]
    bout = np.zeros(ld)
    dp = C.POINTER(C.c_double)
    row = 0
    for (idx, R), J, r in zip(blocks, Js, rs):
        idx32 = np.ascontiguousarray(idx, dtype=np.int32)
        Jf = np.asfortranarray(J[p], dtype=np.float64)
        rr = np.ascontiguousarray(r[p], dtype=np.float64)
        base = out.ctypes.data + 8 * row
        lib.orc_update_jacobian(C.c_int(R), C.c_int(len(idx)), idx32.ctypes.data_as(C.POINTER(C.c_int)), Jf.ctypes.data_as(dp),
                                rr.ctypes.data_as(dp), C.c_int(ld), C.cast(C.c_void_p(base), dp), C.cast(C.c_void_p(bout.ctypes.data + 8 * row), dp))
        row += R
    return out.T, bout               # [rows, n]


def random_layout(rng, n, count, repeats=False, dynamic=False):
    blocks = []
    for _ in range(count):
        R = int(rng.integers(1, 7))
        Pn = int(rng.integers(1, min(n, 8) + 1))
        if repeats and Pn >= 2 and rng.random() < 0.5:
            idx = list(rng.integers(0, n, Pn))
            idx[-1] = idx[0]         # a repeated variable inside the block
        else:
            idx = list(rng.permutation(n)[:Pn])   # out of order
        blocks.append((tuple(int(i) for i in idx), R))
    if dynamic:
        blocks.append((tuple(int(i) for i in rng.permutation(n)), n + 3))   # P = n, R = n + 3
    return blocks


def draw(rng, blocks, B, f32):
    Js = [rng.uniform(-1, 1, (B, R, len(idx))) for idx, R in blocks]
    rs = [rng.uniform(-1, 1, (B, R)) for _, R in blocks]
    if f32:
        Js = [J.astype(np.float32).astype(np.float64) for J in Js]
        rs = [r.astype(np.float32).astype(np.float64) for r in rs]
    return Js, rs


def bound_terms(n, blocks, Js, rs, p):
    """S_ij = sum over contributions of sum_q |J_qa J_qb| and L_ij = number of contributions (the same for c with r)."""
    S, Sc, _ = oracle_hessian(n, blocks, [np.abs(J) for J in Js], [np.abs(r) for r in rs], p)
    Lh, Lc, _ = oracle_hessian(n, [(idx, 1) for idx, _ in blocks], [np.ones((p + 1, 1, len(idx))) for idx, _ in blocks],
                               [np.ones((p + 1, 1)) for _ in blocks], p)
    return S, Sc, Lh, Lc


# ------------------------------------------------------------------ 1. known answers
@pytest.mark.parametrize("case", json.load(open(os.path.join(GOLDEN, "residual.json"))), ids=lambda c: c["name"])
def test_update_hessian_kat_through_blocks(case):
    n = case["full_size"]
    J = np.array(case["J"])
    lay = Q.ResidualLayout(n, [(case["index"], J.shape[0])])
    G, c, half = Q.linearize_blocks(lay, T(pack_np([J[None]])), T(np.array(case["r"])[None]))
    H = G.cpu().numpy()[0].T
    np.testing.assert_allclose(H, np.array(case["expected_H_lower"]), rtol=0, atol=case["tol_abs"])
    assert np.all(np.triu(H, 1) == 0)
    np.testing.assert_allclose(c.cpu().numpy()[0], case["expected_b"], rtol=0, atol=case["tol_abs"])
    assert abs(float(half[0]) - case["expected_half_sq"]) < 1e-14
    mask = np.zeros((n, n), bool)
    for i in case["index"]:
        for j in case["index"]:
            mask[i, j] = True
    assert np.all(H[~mask] == 0)


# ------------------------------------------------------------------ 2. against the oracle
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [3, 8, 15, 64, 100, 128, 200, 300])
def test_linearize_blocks_against_oracle(n, dtype):
    f32 = dtype == torch.float32
    rng = np.random.default_rng(1000 + n + (7 if f32 else 0))
    sparse = random_layout(rng, n, count=max(4, min(60, 2 * n)), repeats=True)
    # the sparse layout at batch 1 and a ragged 1 000 + 7; the same plus one dynamic block (P = n, R = n + 3: beyond the LDS staging budget
    # from n = 64 on) at batch 1 and 7
    for blocks, batches in ((sparse, (1, 1007)), (sparse + [(tuple(int(i) for i in rng.permutation(n)), n + 3)], (1, 7))):
        check_layout_against_oracle(rng, n, blocks, batches, dtype)
    # repeated indices: UpdateHessian is not J^T J of the scattered stack (the dense path counts the cross term twice)
    if not f32 and any(len(set(idx)) < len(idx) for idx, _ in sparse):
        blocks = sparse
        lay = Q.ResidualLayout(n, blocks)
        Js, rs = draw(rng, blocks, 1, False)
        Gb, _, _ = Q.linearize_blocks(lay, T(pack_np(Js)), T(np.concatenate(rs, 1)))
        Jd = np.zeros((1, lay.rows, n))
        row = 0
        for (idx, R), J in zip(blocks, Js):
            for l, g in enumerate(idx):
                Jd[0, row:row + R, g] += J[0, :, l]
            row += R
        Gd, _, _ = Q.linearize(Q.BatchedQP(n=n, J=T(Jd), r=T(np.concatenate(rs, 1))))
        assert (Gb - Gd).abs().max().item() > 1e-6


def check_layout_against_oracle(rng, n, blocks, batches, dtype):
    f32 = dtype == torch.float32
    u = 2.0 ** -24 if f32 else 2.0 ** -53
    R_max = max(R for _, R in blocks)
    lay = Q.ResidualLayout(n, blocks, dtype=dtype)
    assert lay.rows == sum(R for _, R in blocks) and lay.values == sum(R * len(i) for i, R in blocks)
    for B in batches:
        check = sorted({0, 1, B // 2, B - 2, B - 1} & set(range(B)))
        Js, rs = draw(rng, blocks, B, f32)
        Jp, r = T(pack_np(Js), dtype), T(np.concatenate(rs, 1), dtype)
        for lam, lam_vec in ((0.0, None), (0.37, None), (0.0, rng.uniform(0, 1, B))):
            if lam_vec is not None:
                lam_vec[::3] = 0.0
                if f32:
                    lam_vec = lam_vec.astype(np.float32).astype(np.float64)
            G, c, half = Q.linearize_blocks(lay, Jp, r, lam=lam, lam_vec=None if lam_vec is None else T(lam_vec, dtype))
            G, c, half = G.double().cpu().numpy(), c.double().cpu().numpy(), half.double().cpu().numpy()
            for p in check:
                H_ref, b_ref, f_ref = oracle_hessian(n, blocks, Js, rs, p)
                S, Sc, Lh, Lc = bound_terms(n, blocks, Js, rs, p)
                lp = float(lam_vec[p]) if lam_vec is not None else lam
                Hd = G[p].T
                H_ref = H_ref + (lp if lp > 0 else 0.0) * np.eye(n)
                tol = 2 * (R_max + Lh) * u * S + (u * abs(lp)) * np.eye(n)
                assert np.all(np.abs(Hd - H_ref) <= tol), (n, B, p, np.abs(Hd - H_ref).max())
                assert np.all(np.abs(c[p] - b_ref) <= 2 * (R_max + Lc) * u * Sc), (n, B, p)
                assert np.all(np.triu(Hd, 1) == 0)
                untouched = (Lh == 0) & ~np.eye(n, dtype=bool)
                assert np.all(Hd[untouched] == 0)
                assert np.all(c[p][Lc == 0] == 0)
                assert abs(half[p] - f_ref) <= 4 * (lay.rows + 2) * u * abs(f_ref) + 1e-300


# ------------------------------------------------------------------ 3. determinism, 4. agreement with the dense path
@pytest.mark.parametrize("n", [12, 64, 128])
def test_blocks_deterministic_and_match_dense_path(n):
    rng = np.random.default_rng(n)
    blocks = random_layout(rng, n, count=3 * n // 2)          # distinct indices inside every block
    lay = Q.ResidualLayout(n, blocks)
    B = 300
    Js, rs = draw(rng, blocks, B, False)
    Jp, r = T(pack_np(Js)), T(np.concatenate(rs, 1))
    G1, c1, f1 = Q.linearize_blocks(lay, Jp, r, lam=0.01)
    G2, c2, f2 = Q.linearize_blocks(lay, Jp, r, lam=0.01)
    assert torch.equal(G1, G2) and torch.equal(c1, c2) and torch.equal(f1, f2)
    Jd = np.zeros((B, lay.rows, n))
    row = 0
    for (idx, R), J in zip(blocks, Js):
        Jd[:, row:row + R, list(idx)] = J
        row += R
    Gd, cd, fd = Q.linearize(Q.BatchedQP(n=n, J=T(Jd), r=r, lam=0.01))
    scale = Gd.abs().max().item()
    assert (G1 - Gd).abs().max().item() <= 1e-12 * scale
    assert (c1 - cd).abs().max().item() <= 1e-12 * cd.abs().max().item()
    torch.testing.assert_close(f1, fd, rtol=1e-12, atol=0)


# ------------------------------------------------------------------ 5. mo_jacobian_blocks
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_jacobian_blocks_equals_update_jacobian(dtype):
    rng = np.random.default_rng(55)
    n = 20
    blocks = random_layout(rng, n, count=9, repeats=True) + [((4, 9, 4), 2)]   # duplicate index: the last column wins
    lay = Q.ResidualLayout(n, blocks, dtype=dtype)
    B = 37
    Js, rs = draw(rng, blocks, B, dtype == torch.float32)
    Jp, r = T(pack_np(Js), dtype), T(np.concatenate(rs, 1), dtype)
    Jc, s = Q.jacobian_blocks(lay, Jp, r)                     # [B, n, rows]: rows x n column-major
    Jr, s2 = Q.jacobian_blocks(lay, Jp, r, row_major=True)    # [B, rows, n]
    Jc, Jr = Jc.double().cpu().numpy(), Jr.double().cpu().numpy()
    for p in range(B):
        ref, bref = oracle_jacobian(n, blocks, Js, rs, p, lay.rows)
        assert np.array_equal(Jc[p].T, ref) and np.array_equal(Jr[p], ref)
        np.testing.assert_allclose(float(s[p]), np.abs(bref).sum(), rtol=1e-6 if dtype == torch.float32 else 1e-14)
    assert torch.equal(s, s2)


# ------------------------------------------------------------------ 6. QP end to end
def test_blocks_to_fused_qp_solve_matches_dense_solve():
    rng = np.random.default_rng(64)
    n, k, m, B = 64, 8, 32, 96
    blocks = [(tuple(int(i) for i in rng.permutation(n)[:4]), 2) for _ in range(96)]
    lay = Q.ResidualLayout(n, blocks)
    Js, rs = draw(rng, blocks, B, False)
    Jp, r = T(pack_np(Js)), T(np.concatenate(rs, 1))
    lam = 0.5
    G, c, _ = Q.linearize_blocks(lay, Jp, r, lam=lam)
    Jd = np.zeros((B, lay.rows, n))
    row = 0
    for (idx, R), J in zip(blocks, Js):
        Jd[:, row:row + R, list(idx)] = J
        row += R
    A = rng.uniform(-1, 1, (B, k, n)); b = rng.uniform(-1, 1, (B, k))
    cv = np.arange(m, dtype=np.int32)[None]; ca = np.ones((1, m)); cb = np.full((1, m), 2.0)     # x_i + 2 >= 0
    common = dict(n=n, k=k, m=m, A_eq=T(A.transpose(0, 2, 1)), b_eq=T(b), cons_var=T(cv, torch.int32), cons_a=T(ca), cons_b=T(cb))
    prm = Q.Params(max_iterations=20)
    sg = Q.QPInteriorPointSolver(Q.BatchedQP(G=G, c=c, **common))
    assert sg.solve_kernel().startswith("fused")
    og = sg.Solve(prm)
    sj = Q.QPInteriorPointSolver(Q.BatchedQP(J=T(Jd), r=r, lam=lam, **common))
    oj = sj.Solve(prm)
    assert torch.all(og.status == 0) and torch.all(oj.status == 0)
    assert torch.equal(og.termination_state, oj.termination_state)
    assert (sg.x_block() - sj.x_block()).abs().max().item() <= 1e-9


# ------------------------------------------------------------------ 7. NLS
def rosenbrock_residuals():
    def r0(x, want_J):   # 1 - x0
        return (1.0 - x[:, 0]).unsqueeze(1), (-torch.ones(x.shape[0], 1, 1, dtype=x.dtype, device=x.device) if want_J else None)

    def r1(x, want_J):   # sqrt(b) (x1 - x0^2)
        r = (P.SQRT_B * (x[:, 1] - x[:, 0] * x[:, 0])).unsqueeze(1)
        J = torch.stack([-2.0 * x[:, 0] * P.SQRT_B, torch.full_like(x[:, 0], P.SQRT_B)], dim=1).unsqueeze(1) if want_J else None
        return r, J
    return [NLS.MakeResidual((0,), r0, 1), NLS.MakeResidual((0, 1), r1, 1)]


def sphere_residuals():
    def sphere(x, want_J):
        return x.clone(), (torch.eye(x.shape[1], dtype=x.dtype, device=x.device).expand(x.shape[0], -1, -1).contiguous() if want_J else None)

    def product(target):
        def fn(x, want_J):
            return (x[:, 0] * x[:, 1] - target).unsqueeze(1), (torch.stack([x[:, 1], x[:, 0]], dim=1).unsqueeze(1) if want_J else None)
        return fn
    # the cost as three out-of-order blocks of the six variables
    return ([NLS.MakeResidual((0, 1), sphere, 2), NLS.MakeResidual((2, 3), sphere, 2), NLS.MakeResidual((4, 5), sphere, 2)],
            [NLS.MakeResidual((0, 1), product(4.0), 1), NLS.MakeResidual((2, 3), product(9.0), 1)])


def solve_three_ways(n, costs, eqs, cons, oprob, kw, guesses):
    guesses = np.array(guesses, dtype=float)
    B = len(guesses)
    prob = NLS.Problem.FromResiduals(n, costs, eqs, cons)
    blk = NLS.ConstrainedNonlinearLeastSquares(prob, batch=B, residual_blocks=True)
    den = NLS.ConstrainedNonlinearLeastSquares(prob, batch=B)
    ob, od = blk.Solve(NLS.Params(**kw), T(guesses)), den.Solve(NLS.Params(**kw), T(guesses))
    term, nit, x = ob.termination_state.cpu().numpy(), ob.num_iterations.cpu().numpy(), blk.variables().cpu().numpy()
    assert np.array_equal(term, od.termination_state.cpu().numpy())
    assert np.array_equal(nit, od.num_iterations.cpu().numpy())
    ref = N.ConstrainedNonlinearLeastSquares(oprob)
    rterm, rnit, rx = [], [], []
    for g in guesses:
        t, logs = ref.solve(N.Params(**kw), g)
        rterm.append(t); rnit.append(len(logs)); rx.append(ref.variables.copy())
    return term, nit, x, np.array(rterm), np.array(rnit), np.array(rx)


def test_nls_blocks_rosenbrock():
    for kw in (dict(max_iterations=5, max_qp_iterations=1),
               dict(max_iterations=10, max_qp_iterations=1, absolute_first_derivative_tol=1e-12, max_line_search_iterations=0)):
        term, nit, x, rterm, rnit, rx = solve_three_ways(2, rosenbrock_residuals(), [], [], N.Problem(2, P.rosenbrock_np), kw,
                                                         P.ROSENBROCK_GUESSES)
        assert np.all(term == NLS.SATISFIED_ABSOLUTE_TOL)
        np.testing.assert_allclose(x, np.ones_like(x), atol=1e-6)
        assert np.array_equal(term, rterm) and np.array_equal(nit, rnit)


def test_nls_blocks_inequality_constrained_rosenbrock():
    cons = [(0, 1.0, -1.2), (1, -1.0, 0.5)]
    term, nit, x, rterm, rnit, rx = solve_three_ways(2, rosenbrock_residuals(), [], cons, N.Problem(2, P.rosenbrock_np, inequality_constraints=cons),
                                                     dict(max_iterations=10, max_qp_iterations=10), P.ROSENBROCK_CONSTRAINED_GUESSES)
    assert np.array_equal(term, rterm) and np.array_equal(nit, rnit)
    np.testing.assert_allclose(x, rx, atol=1e-7)


def test_nls_blocks_sphere_with_product_equalities():
    from tests.test_gpu_nls import knife_edge_rule
    costs, eqs = sphere_residuals()
    kw = dict(max_iterations=100, max_qp_iterations=1, relative_exit_tol=1e-12, absolute_first_derivative_tol=1e-9,
              termination_kkt_tolerance=1e-6, lambda_initial=0.001)
    oprob = N.Problem(6, P.sphere_np, equality=P.sphere_eq_np)
    guesses = P.sphere_guesses(24)
    prob = NLS.Problem.FromResiduals(6, costs, eqs)
    assert bool(L.lib().mo_plan_nls_uses_nullspace(NLS.ConstrainedNonlinearLeastSquares(prob, batch=1, residual_blocks=True)._plan.h))
    term, nit, x, rterm, rnit, rx = solve_three_ways(6, costs, eqs, [], oprob, kw, guesses)
    assert np.all(NLS.TerminationStateIndicatesSatisfiedTol(torch.as_tensor(term)).numpy())
    same = knife_edge_rule("sphere blocks", oprob, N.Params(**kw), guesses, term, nit, rterm, rnit)
    np.testing.assert_allclose(x[same], rx[same], atol=1e-6)


# ------------------------------------------------------------------ 8. errors
def _plan(n, m_r, dtype=L.MO_F64, k=0):
    desc = L.PlanDesc(n, k, 0, m_r, dtype, 0, 0, 0, 0)
    h = C.c_void_p()
    L.check(L.lib().mo_plan_create(C.byref(desc), C.byref(h)))
    return h


def test_block_entry_point_errors():
    lib = L.lib()
    plan = _plan(5, 4)
    try:
        with pytest.raises(L.MiniOptError) as e:
            Q.create_layout(plan, [((0, 5), 2)])
        assert e.value.code == -2                                   # MO_ERR_DIMENSION: index >= n
        for bad in ([((0, 1), 0)], [((), 2)]):
            with pytest.raises(L.MiniOptError) as e:
                Q.create_layout(plan, bad)
            assert e.value.code == -1                               # R, P <= 0
        h = C.c_void_p()
        one = (C.c_int32 * 1)(1)
        assert lib.mo_residual_layout_create(plan, 1, None, one, one, C.byref(h)) == -1
        assert lib.mo_residual_layout_create(plan, 1, one, one, None, C.byref(h)) == -1
        lay = Q.create_layout(plan, [((0, 1), 3)])                  # 3 rows != plan m_r = 4
        try:
            buf = torch.zeros(8, dtype=torch.float64, device=DEV)
            ptr = C.c_void_p(buf.data_ptr())
            assert lib.mo_linearize_blocks(plan, lay, ptr, 0, ptr, 0, 0.0, None, 0, 1, ptr, 0, 5, ptr, 0, None, None) == -2
            lay4 = Q.create_layout(plan, [((0, 1), 3), ((4,), 1)])
            G = torch.full((1, 5, 5), 7.0, dtype=torch.float64, device=DEV)
            assert lib.mo_linearize_blocks(plan, lay4, ptr, 0, ptr, 0, 0.0, None, 0, 0, C.c_void_p(G.data_ptr()), 25, 5, ptr, 0, None,
                                           None) == 0                # batch 0: a no-op
            assert lib.mo_jacobian_blocks(plan, lay4, ptr, 0, ptr, 0, 0, C.c_void_p(G.data_ptr()), 25, 4, 0, None, None) == 0
            torch.cuda.synchronize()
            assert torch.all(G == 7.0)
            assert lib.mo_residual_layout_rows(lay4) == 4 and lib.mo_residual_layout_values(lay4) == 7
            lib.mo_residual_layout_destroy(lay4)
        finally:
            lib.mo_residual_layout_destroy(lay)
    finally:
        lib.mo_plan_destroy(plan)
    p32 = _plan(2, 2, L.MO_F32)
    try:
        lay = Q.create_layout(p32, [((0, 1), 2)])
        prm = L.NlsParams()
        lib.mo_default_nls_params(C.byref(prm))
        np_ = L.NlsProblem()
        cb = L.NLS_EVAL_FN(lambda u, w, s: 0)
        assert lib.mo_nls_solve_blocks(p32, C.byref(np_), lay, None, 1, C.byref(prm), cb, None, None, None, None, None, None) == -3
        lib.mo_residual_layout_destroy(lay)
    finally:
        lib.mo_plan_destroy(p32)
