"""GPU tests of the differentiable QP (run with -m gpu on an MI355X): mo_kkt_solve against the Newton step and against LU on the oracle's
full system, mo_qp_gradients against the numpy restatement (tests/diff_reference.py), and solve_qp's autograd end to end.
Bounds: TOL64 / TOL32 of tests/test_gpu_parity.py (what the Newton step meets against the same matrices on these shapes)."""
import ctypes as C

import numpy as np
import pytest
import torch

from mini_opt_amd import _lib as L
from mini_opt_amd import diff as D
from mini_opt_amd import qp as Q
from oracle import oracle as orc
from tests import diff_reference as R
from tests.sens_fixtures import (ACTIVE_SEED, PARAMS, T, active_set_problems, dev, device_problem, host_batch, oracle_kkt_solves,
                                 oracle_solver, rel_inf_rows)

pytestmark = pytest.mark.gpu
TOL64 = 1e-10
TOL32 = 2e-3
SHAPES = [(8, 2, 5, 12), (8, 0, 0, 12), (12, 3, 0, 20), (64, 8, 32, 128), (96, 40, 20, 128)]   # (n, k, m, m_r); the last two run LARGE
CASES = [(s, lvl, torch.float64) for s in SHAPES for lvl in ("J", "G")] + [(s, "J", torch.float32) for s in (SHAPES[0], SHAPES[3])]
IDS = [f"n{s[0]}k{s[1]}m{s[2]}-{lvl}-{'f64' if dt == torch.float64 else 'f32'}" for s, lvl, dt in CASES]


# ---- 1. the Newton direction through mo_kkt_solve -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,level,dt", CASES, ids=IDS)
def test_kkt_solve_of_the_residual_is_the_newton_step(shape, level, dt):
    n, k, m, m_r = shape
    f32 = dt == torch.float32
    hb = host_batch(n, k, m, m_r, 24, stream=31, f32=f32)
    prob = device_problem(hb, level, dt)
    s = Q.QPInteriorPointSolver(prob, force_generic=True)
    s.SetVariables(T(hb.vars, dt))
    mu = T(hb.mu, dt)
    delta, _, status = s.NewtonStep(mu, 0.995)
    assert s.step_kernel() == "generic" and torch.all(status == 0)
    r, _ = s.EvaluateKKTConditions(mu)
    rhs = r.clone()
    rhs[:, n:n + m] -= mu[:, None]
    out, st = D.kkt_solve(prob, s.variables(), rhs)
    assert torch.all(st == 0)
    err = rel_inf_rows(out.double().cpu().numpy(), delta.double().cpu().numpy())
    print(f"kkt_solve vs newton_step {shape} {level}: max rel-inf {err.max():.3e}, bitwise equal: {bool(torch.equal(out, delta))}")
    assert err.max() < (TOL32 if f32 else TOL64)
    if k:   # the equality-only system of the initial guess
        d0, _, st0 = s.NewtonStep(mu, 0.995, include_inequalities=False)
        r0 = s.EvaluateKKTConditions(mu, include_inequalities=False)[0].clone()
        out0, st1 = D.kkt_solve(prob, s.variables(), r0, include_inequalities=False)
        assert torch.all(st0 == 0) and torch.all(st1 == 0)
        assert rel_inf_rows(out0.double().cpu().numpy(), d0.double().cpu().numpy()).max() < (TOL32 if f32 else TOL64)


# ---- 2. random right-hand sides against LU on the oracle's matrix ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,level,dt", CASES, ids=IDS)
def test_kkt_solve_against_lu_on_the_oracle_matrix(shape, level, dt):
    n, k, m, m_r = shape
    f32 = dt == torch.float32
    B = 12
    hb = host_batch(n, k, m, m_r, B, stream=32, f32=f32)
    prob = device_problem(hb, level, dt)
    rng = np.random.default_rng(7)
    rhs = rng.normal(size=hb.vars.shape)
    if f32:
        rhs = rhs.astype(np.float32).astype(np.float64)
    v = T(hb.vars, dt)
    direct, st_d = D.kkt_solve(prob, v, T(rhs, dt))
    transposed, st_t = D.kkt_solve(prob, v, T(rhs, dt), transpose=True)
    assert torch.all(st_d == 0) and torch.all(st_t == 0)
    ref_d, ref_t = np.zeros_like(rhs), np.zeros_like(rhs)
    for p in range(B):
        ref_d[p], ref_t[p] = oracle_kkt_solves(oracle_solver(hb, p, hb.vars[p]), n, k, m, rhs[p], rhs[p])
        if p == 0:   # the oracle's matrix is the K of the header, up to the two diagonal scalings
            Kref = R.kkt_matrix(hb.G[p], hb.A_eq[p].T if k else np.zeros((0, n)), hb.cons_var[p], hb.cons_a[p], hb.vars[p])
            assert np.max(np.abs(Kref.T @ ref_t[p] - rhs[p])) < 1e-8 * max(1.0, np.max(np.abs(ref_t[p])))
    e_d = rel_inf_rows(direct.double().cpu().numpy(), ref_d)
    e_t = rel_inf_rows(transposed.double().cpu().numpy(), ref_t)
    print(f"kkt_solve vs LU {shape} {level}: direct {e_d.max():.3e} transposed {e_t.max():.3e}")
    tol = TOL32 if f32 else TOL64
    assert e_d.max() < tol and e_t.max() < tol


# ---- 3. status words ------------------------------------------------------------------------------------------------------------------------
def test_kkt_solve_status_words():
    n, k, m, m_r = 8, 2, 4, 16
    hb = host_batch(n, k, m, m_r, 8, stream=33)
    rng = np.random.default_rng(8)
    rhs = rng.normal(size=hb.vars.shape)
    good = device_problem(hb, "G")
    ref, st = D.kkt_solve(good, T(hb.vars), T(rhs))
    ref_t, _ = D.kkt_solve(good, T(hb.vars), T(rhs), transpose=True)
    assert torch.all(st == 0)
    hb.vars[1, n] = 0.0                         # s = 0 (F_ASSERT qp.cc:285)
    hb.cons_var[3, 0] = n + 3                   # constraint index out of range (qp.cc:70-72)
    hb.G[5] = 0.0                               # an indefinite G whose first pivot is zero above a non-zero column (qp.cc:303-307)
    hb.G[5, 0, 1] = hb.G[5, 1, 0] = 1.0
    hb.G[5][np.arange(2, n), np.arange(2, n)] = 1.0
    hb.cons_var[5][hb.cons_var[5] == 0] = 2     # (no Sigma on that pivot)
    bad = device_problem(hb, "G")
    for transpose, want in ((False, ref), (True, ref_t)):
        out, st = D.kkt_solve(bad, T(hb.vars), T(rhs), transpose=transpose)
        st, o = st.cpu().numpy(), out.cpu().numpy()
        assert st[1] == L.MO_STATUS_NONPOSITIVE_SLACK and st[3] == L.MO_STATUS_BAD_INDEX and st[5] == L.MO_STATUS_FACTORIZATION_FAILED, st
        others = [0, 2, 4, 6, 7]
        assert np.all(st[others] == 0)
        assert np.all(np.isnan(o[[1, 3, 5]]))
        assert np.array_equal(o[others], want.cpu().numpy()[others])   # the neighbours are unaffected, to the bit
    # a NaN in the caller's vector is that problem's alone
    rhs2 = rhs.copy(); rhs2[2, 0] = np.nan
    out, st = D.kkt_solve(good, T(host_batch(n, k, m, m_r, 8, stream=33).vars), T(rhs2))
    assert int(st[2]) == L.MO_STATUS_NONFINITE and torch.all(torch.isnan(out[2])) and torch.equal(out[0], ref[0])


# ---- 4. mo_qp_gradients ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(8, 2, 5, 12), (64, 8, 32, 128), (96, 40, 20, 128), (7, 3, 4, 9)], ids=lambda s: f"n{s[0]}k{s[1]}m{s[2]}")
def test_qp_gradients_against_the_numpy_restatement(shape, dt):
    n, k, m, m_r = shape
    f32 = dt == torch.float32
    B = 6
    hb = host_batch(n, k, m, m_r, B, stream=34, f32=f32)
    rng = np.random.default_rng(9)
    u = rng.normal(size=hb.vars.shape)
    if f32:
        u = u.astype(np.float32).astype(np.float64)
    tol = TOL32 if f32 else TOL64
    ref = [R.gradients(n, k, m, hb.cons_var[p], hb.vars[p], u[p], J=hb.J[p], r=hb.r[p]) for p in range(B)]
    stack = lambda key: np.stack([np.atleast_1d(ref[p][key]).reshape(-1) for p in range(B)])
    v_d, u_d = T(hb.vars, dt), T(u, dt)

    def check(got, key, tag):
        err = rel_inf_rows(got.double().cpu().numpy().reshape(B, -1), stack(key))
        assert err.max() < tol, (tag, key, err.max())

    g = D.qp_gradients(device_problem(hb, "G", dt), v_d, u_d)
    assert set(g) == {"G", "c", "A_eq", "b_eq", "cons_a", "cons_b"}
    for key in ("c", "b_eq", "cons_a", "cons_b", "G"):
        check(g[key], key, "G-level")
    check(g["A_eq"].transpose(1, 2), "A_eq", "G-level")          # [B, n, k] memory = k x n column-major
    assert torch.equal(g["G"], g["G"].transpose(1, 2))           # exactly symmetric
    g2 = D.qp_gradients(device_problem(hb, "G", dt), v_d, u_d)
    assert all(torch.equal(g[key], g2[key]) for key in g)        # two launches, the same bits
    # J-level, both layouts, dense and with padded leading dimensions
    for layout, ld in (("row", None), ("row", n + 3), ("col", None), ("col", m_r + 5)):
        prob = device_problem(hb, "J", dt, J_layout=layout, J_ld=ld)
        gj = D.qp_gradients(prob, v_d, u_d)
        assert set(gj) == {"J", "r", "lam", "A_eq", "b_eq", "cons_a", "cons_b"}
        dJ = gj["J"].transpose(1, 2)[:, :m_r, :n] if layout == "col" else gj["J"][:, :, :n]
        check(dJ.contiguous(), "J", (layout, ld))
        check(gj["r"], "r", (layout, ld)); check(gj["lam"], "lam", (layout, ld))
        if ld is not None:   # the padding is not written
            pad = gj["J"][:, :, m_r:] if layout == "col" else gj["J"][:, :, n:]
            assert torch.all(pad == 0)
        gj2 = D.qp_gradients(prob, v_d, u_d)
        assert all(torch.equal(gj[key], gj2[key]) for key in gj)


def test_qp_gradients_strides_and_null_members():
    """Through the C ABI: per-problem strides with padding, leading dimensions beyond the matrix, and NULL members that leave canary-filled
    buffers untouched."""
    n, k, m, m_r, B = 8, 2, 5, 12, 5
    hb = host_batch(n, k, m, m_r, B, stream=35)
    rng = np.random.default_rng(10)
    u = rng.normal(size=hb.vars.shape)
    prob = device_problem(hb, "G")
    plan = D.plan_for(prob, B)
    ps = prob.as_struct()
    CANARY = -777.25
    V = hb.vars.shape[1]
    buf = {key: torch.full((B, size), CANARY, dtype=torch.float64, device=dev()) for key, size in
           (("G", (n + 2) * n + 7), ("c", n + 3), ("A", (k + 1) * n + 5), ("b", k + 1), ("ca", m + 2), ("cb", m + 2))}
    v_d, u_d = T(hb.vars), T(u)
    ref = [R.gradients(n, k, m, hb.cons_var[p], hb.vars[p], u[p]) for p in range(B)]

    def launch(**members):
        g = L.QPGrads()
        for key, val in members.items():
            setattr(g, key, val)
        L.check(L.lib().mo_qp_gradients(plan, C.byref(ps), B, Q._ptr(v_d), V, Q._ptr(u_d), V, C.byref(g), Q._stream()))
        torch.cuda.synchronize()

    # only dc and dcons_b: everything else stays canary
    launch(dc=buf["c"].data_ptr(), dc_stride=n + 3, dcons_b=buf["cb"].data_ptr(), dcons_stride=m + 2)
    for key in ("G", "A", "b", "ca"):
        assert torch.all(buf[key] == CANARY), key
    got_c, got_cb = buf["c"].cpu().numpy(), buf["cb"].cpu().numpy()
    for p in range(B):
        assert np.max(np.abs(got_c[p, :n] - ref[p]["c"])) <= TOL64 * np.max(np.abs(ref[p]["c"]))
        assert np.max(np.abs(got_cb[p, :m] - ref[p]["cons_b"])) <= TOL64 * np.max(np.abs(ref[p]["cons_b"]))
    assert np.all(got_c[:, n:] == CANARY) and np.all(got_cb[:, m:] == CANARY)
    # the matrices with padded leading dimensions and strides
    launch(dG=buf["G"].data_ptr(), dG_stride=(n + 2) * n + 7, dG_ld=n + 2, dA_eq=buf["A"].data_ptr(), dA_stride=(k + 1) * n + 5, dA_ld=k + 1,
           db_eq=buf["b"].data_ptr(), db_stride=k + 1, dcons_a=buf["ca"].data_ptr(), dcons_stride=m + 2)
    G = buf["G"].cpu().numpy()[:, :(n + 2) * n].reshape(B, n, n + 2)        # [column][row]
    A = buf["A"].cpu().numpy()[:, :(k + 1) * n].reshape(B, n, k + 1)
    for p in range(B):
        assert np.max(np.abs(G[p, :, :n].T - ref[p]["G"])) <= TOL64 * np.max(np.abs(ref[p]["G"]))
        assert np.max(np.abs(A[p, :, :k].T - ref[p]["A_eq"])) <= TOL64 * np.max(np.abs(ref[p]["A_eq"]))
        assert np.max(np.abs(buf["ca"].cpu().numpy()[p, :m] - ref[p]["cons_a"])) <= TOL64 * np.max(np.abs(ref[p]["cons_a"]))
    assert np.all(G[:, :, n:] == CANARY) and np.all(A[:, :, k:] == CANARY)
    assert np.all(buf["G"].cpu().numpy()[:, (n + 2) * n:] == CANARY) and np.all(buf["ca"].cpu().numpy()[:, m:] == CANARY)
    assert torch.all(buf["cb"][:, m:] == CANARY)
    # the documented refusals, with a real plan
    g = L.QPGrads(); g.dJ = buf["G"].data_ptr(); g.dJ_ld = n
    assert L.lib().mo_qp_gradients(plan, C.byref(ps), B, Q._ptr(v_d), V, Q._ptr(u_d), V, C.byref(g), Q._stream()) == -1
    g = L.QPGrads(); g.dG = buf["G"].data_ptr(); g.dG_ld = n - 1
    assert L.lib().mo_qp_gradients(plan, C.byref(ps), B, Q._ptr(v_d), V, Q._ptr(u_d), V, C.byref(g), Q._stream()) == -2


# ---- 5. autograd end to end ------------------------------------------------------------------------------------------------------------------
def test_autograd_unconstrained_against_torch_linalg_solve():
    """(a) m = 0, k = 0, G = M M^T / n + I (cond(G) <= ~10): gradients with respect to M and c through solve_qp against autograd through
    torch.linalg.solve(G, -c), TOL64."""
    n, B = 8, 16
    gen = torch.Generator(device="cpu").manual_seed(5)
    M0 = (torch.rand(B, n, n, generator=gen, dtype=torch.float64) * 2 - 1).to(dev())
    c0 = torch.randn(B, n, generator=gen, dtype=torch.float64).to(dev())
    grads = []
    for which in ("device", "torch"):
        M, c = M0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
        G = M @ M.transpose(1, 2) / n + torch.eye(n, dtype=torch.float64, device=dev())
        x = D.solve_qp(G=G, c=c, params=Q.Params(**PARAMS)) if which == "device" else torch.linalg.solve(G, -c.unsqueeze(-1)).squeeze(-1)
        x.sum().backward()
        grads.append((x.detach(), M.grad, c.grad))
    (x_d, dM_d, dc_d), (x_t, dM_t, dc_t) = grads
    for a, b, tag in ((x_d, x_t, "x"), (dc_d, dc_t, "dc"), (dM_d.reshape(B, -1), dM_t.reshape(B, -1), "dM")):
        err = rel_inf_rows(a.cpu().numpy(), b.cpu().numpy())
        print(f"unconstrained {tag}: {err.max():.3e}")
        assert err.max() < TOL64, tag


def test_autograd_equality_only_against_the_dense_kkt_solve_in_torch():
    """(b) (12, 3, 0): gradients of a weighted sum of x with respect to M (G = M M^T / n + I), c, A_eq, b_eq against autograd through the
    dense KKT solve [[G, A^T], [A, 0]] [x; nu] = [-c; -b_eq] in torch, TOL64."""
    n, k, B = 12, 3, 16
    gen = torch.Generator(device="cpu").manual_seed(6)
    rnd = lambda *s: (torch.rand(*s, generator=gen, dtype=torch.float64) * 2 - 1).to(dev())
    M0, c0, A0, b0, wgt = rnd(B, n, n), rnd(B, n), rnd(B, k, n), rnd(B, k), rnd(B, n)
    res = []
    for which in ("device", "torch"):
        leaves = [t.clone().requires_grad_(True) for t in (M0, c0, A0, b0)]
        M, c, A, b = leaves
        G = M @ M.transpose(1, 2) / n + torch.eye(n, dtype=torch.float64, device=dev())
        if which == "device":
            x = D.solve_qp(G=G, c=c, A_eq=A, b_eq=b, params=Q.Params(**PARAMS))
        else:
            Kd = torch.cat([torch.cat([G, A.transpose(1, 2)], dim=2), torch.cat([A, torch.zeros(B, k, k, dtype=torch.float64, device=dev())], dim=2)], dim=1)
            x = torch.linalg.solve(Kd, -torch.cat([c, b], dim=1).unsqueeze(-1)).squeeze(-1)[:, :n]
        (x * wgt).sum().backward()
        res.append([x.detach()] + [t.grad for t in leaves])
    for a, b_, tag in zip(res[0], res[1], ("x", "dM", "dc", "dA_eq", "db_eq")):
        err = rel_inf_rows(a.reshape(B, -1).cpu().numpy(), b_.reshape(B, -1).cpu().numpy())
        print(f"equality-only {tag}: {err.max():.3e}")
        assert err.max() < TOL64, tag


def test_autograd_with_active_inequalities():
    """(c) Device gradients against tests/diff_reference.py evaluated AT THE DEVICE'S OWN v (LU on the full K), on problems with active rows.

    The bound is max(TOL64, 10 D).  D is measured on the CPU without the code under test: at the ORACLE's Solve output of the same problems,
    the largest rel_inf_rows between u from LU on the full matrix and u from the reduced system H = G + C^T S^-1 Z C in numpy; the factor 10
    covers an unpivoted LDL^T against a pivoted LU.  Seed 2024, 200 problems (25 for each m = 1 ... 8).  Measured (and printed by every
    run): D = 1.3e-15, so the bound is TOL64 itself; 150 of the 200 problems have an active row, the smallest slack is 3e-11; the device's
    worst rel-inf over G, c, a, b was 3.3e-15.  No problem is excused; at least half of the problems must have an active row (s < 1e-6)."""
    groups = active_set_problems()
    n = 8
    D_cpu, active, total, worst = 0.0, 0, 0, {}
    for grp in groups:
        m, cnt = grp["m"], grp["G"].shape[0]
        V = n + 2 * m
        g_full = np.concatenate([grp["gx"], np.zeros((cnt, 2 * m))], axis=1)
        # the CPU measurement of D at the oracle's optimum
        for p in range(cnt):
            o = orc.Solver(orc.QP(G=np.tril(grp["G"][p]), c=grp["c"][p], cons_var=grp["var"][p], cons_a=grp["a"][p], cons_b=grp["b"][p]))
            o.solve(**PARAMS)
            vo = np.array(o.variables)
            _, u_lu = oracle_kkt_solves(o, n, 0, m, g_full[p], g_full[p])
            u_red = R.transposed_through_reduced(grp["G"][p], np.zeros((0, n)), grp["var"][p], grp["a"][p], vo, g_full[p])
            D_cpu = max(D_cpu, float(rel_inf_rows(u_red[None], u_lu[None])[0]))
        # the device
        leaves = {key: T(grp[key]).requires_grad_(True) for key in ("G", "c", "a", "b")}
        x, s, y, z, status = D.solve_qp(G=leaves["G"], c=leaves["c"], cons_var=T(grp["var"], torch.int32), cons_a=leaves["a"], cons_b=leaves["b"],
                                        params=Q.Params(**PARAMS), return_all=True, return_status=True)
        assert torch.all(status == 0)
        (x * T(grp["gx"])).sum().backward()
        assert torch.all(D.adjoint_status(x) == 0)
        v = torch.cat([x, s, y, z], dim=1).detach().cpu().numpy()
        active += int(np.sum(np.min(v[:, n:n + m], axis=1) < 1e-6)); total += cnt
        ref = {key: np.zeros((cnt,) + tuple(leaves[key].shape[1:])) for key in leaves}
        for p in range(cnt):
            Kp = R.kkt_matrix(grp["G"][p], np.zeros((0, n)), grp["var"][p], grp["a"][p], v[p])
            gr = R.gradients(n, 0, m, grp["var"][p], v[p], R.solve_transposed(Kp, g_full[p]))
            ref["G"][p], ref["c"][p], ref["a"][p], ref["b"][p] = gr["G"], gr["c"], gr["cons_a"], gr["cons_b"]
        for key in leaves:
            err = rel_inf_rows(leaves[key].grad.cpu().numpy().reshape(cnt, -1), ref[key].reshape(cnt, -1)).max()
            worst[key] = max(worst.get(key, 0.0), float(err))
    bound = max(TOL64, 10 * D_cpu)
    print(f"active-set autograd: D = {D_cpu:.3e} (seed {ACTIVE_SEED}, {total} problems), bound {bound:.3e}, "
          f"{active} of {total} problems with an active row, worst rel-inf per input {worst}")
    assert 2 * active >= total, (active, total)
    assert max(worst.values()) < bound, (worst, bound)


def test_autograd_failing_problem_gets_zero_gradients():
    """(d) One problem whose forward fails (a constraint index outside [0, n): MO_STATUS_BAD_INDEX, NaN output) inside a healthy batch, and
    a loss gradient of ones for EVERY row: its gradient rows are zero, the others are to the bit what they are without it."""
    n, m, B = 8, 2, 6
    rng = np.random.default_rng(11)
    U = rng.uniform(-1, 1, (B, n, n))
    G = np.einsum("bik,bjk->bij", U, U) / n + np.eye(n)
    c = rng.normal(size=(B, n))
    a = np.tile(np.array([[1.0, -1.0]]), (B, 1))
    b = np.tile(np.array([[0.2, 2.0]]), (B, 1))            # -0.2 <= x_0 <= 2
    out = []
    for broken in (False, True):
        var = np.zeros((B, m), dtype=np.int32)
        if broken:
            var[3, 1] = n + 1
        leaves = [T(t).requires_grad_(True) for t in (G, c, a, b)]
        x, status = D.solve_qp(G=leaves[0], c=leaves[1], cons_var=T(var, torch.int32), cons_a=leaves[2], cons_b=leaves[3],
                               params=Q.Params(**PARAMS), return_status=True)
        x.backward(torch.ones_like(x))
        out.append(([t.grad.clone() for t in leaves], status.cpu().numpy(), D.adjoint_status(x).cpu().numpy()))
    (g_ok, st_ok, adj_ok), (g_bad, st_bad, adj_bad) = out
    assert np.all(st_ok == 0) and np.all(adj_ok == 0)
    assert st_bad[3] == L.MO_STATUS_BAD_INDEX and adj_bad[3] != 0, (st_bad, adj_bad)
    others = [0, 1, 2, 4, 5]
    assert np.all(st_bad[others] == 0) and np.all(adj_bad[others] == 0)
    for t_ok, t_bad in zip(g_ok, g_bad):
        assert torch.all(t_bad[3] == 0) and torch.all(torch.isfinite(t_bad))
        assert torch.equal(t_bad[others], t_ok[others]) and torch.any(t_ok[3] != 0)


def test_autograd_only_requested_inputs_and_repeatable_backward():
    """(e) Only inputs that require a gradient receive one; a second backward through the retained graph gives identical values; J-level
    input differentiates J, r and lam without forming G."""
    n, k, m, m_r, B = 8, 2, 5, 12, 8
    hb = host_batch(n, k, m, m_r, B, stream=36)
    J, r = T(hb.J).requires_grad_(True), T(hb.r)
    lam = torch.full((B,), 1e-3, dtype=torch.float64, device=dev(), requires_grad=True)
    A, b_eq = T(hb.A_eq.transpose(0, 2, 1)), T(hb.b_eq).requires_grad_(True)
    ca, cb = T(hb.cons_a), T(hb.cons_b).requires_grad_(True)
    x, s, y, z = D.solve_qp(J=J, r=r, lam=lam, A_eq=A, b_eq=b_eq, cons_var=T(hb.cons_var, torch.int32), cons_a=ca, cons_b=cb,
                            params=Q.Params(**PARAMS), return_all=True)
    loss = x.sum() + (y * y).sum()
    loss.backward(retain_graph=True)
    first = [t.grad.clone() for t in (J, lam, b_eq, cb)]
    assert r.grad is None and A.grad is None and ca.grad is None
    for t in (J, lam, b_eq, cb):
        t.grad = None
    loss.backward()
    assert all(torch.equal(a_, t.grad) for a_, t in zip(first, (J, lam, b_eq, cb)))
    # against the numpy restatement at the device's v
    v = torch.cat([x, s, y, z], dim=1).detach().cpu().numpy()
    g = np.concatenate([np.ones((B, n)), np.zeros((B, m)), 2 * v[:, n + m:n + m + k], np.zeros((B, m))], axis=1)
    for p in range(B):
        Gp = hb.J[p].T @ hb.J[p] + 1e-3 * np.eye(n)
        u = R.solve_transposed(R.kkt_matrix(Gp, hb.A_eq[p].T, hb.cons_var[p], hb.cons_a[p], v[p]), g[p])
        gr = R.gradients(n, k, m, hb.cons_var[p], v[p], u, J=hb.J[p], r=hb.r[p])
        eJ = np.max(np.abs(first[0][p].cpu().numpy() - gr["J"])) / np.max(np.abs(gr["J"]))
        el = abs(float(first[1][p]) - gr["lam"]) / abs(gr["lam"])
        print(f"J-level autograd, problem {p}: dJ {eJ:.3e} dlam {el:.3e}")
        assert eJ < TOL64 and el < TOL64


# ---- 6. nothing is allocated on the launch path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 8, 32, 128), (96, 40, 20, 128)], ids=["cfg3", "large"])
def test_first_kkt_solve_and_gradients_allocate_nothing(shape):
    n, k, m, m_r = shape
    B = 96
    hb = host_batch(n, k, m, m_r, B, stream=37)
    # what the HIP runtime reserves on its own account (module load, kernel code) happens on ANOTHER plan and shape-twin first
    warm = device_problem(hb, "J")
    v, rhs = T(hb.vars), T(np.random.default_rng(12).normal(size=hb.vars.shape))
    desc = L.PlanDesc(n, k, m, m_r, L.MO_F64, 0, L.EXTRA_PLAN_FLAGS, 0, B)
    plans = [C.c_void_p(), C.c_void_p()]
    for pl in plans:
        L.check(L.lib().mo_plan_create(C.byref(desc), C.byref(pl)))
    ps = warm.as_struct()
    V = hb.vars.shape[1]
    out = torch.empty_like(v); status = torch.empty(B, dtype=torch.int32, device=dev())
    dJ = torch.empty(B, m_r, n, dtype=torch.float64, device=dev()); dr = torch.empty(B, m_r, dtype=torch.float64, device=dev())
    g = L.QPGrads(); g.dJ, g.dJ_stride, g.dJ_ld, g.dJ_layout = dJ.data_ptr(), m_r * n, n, L.MO_ROW_MAJOR
    g.dr, g.dr_stride = dr.data_ptr(), m_r

    def both(plan):
        L.check(L.lib().mo_kkt_solve(plan, C.byref(ps), B, Q._ptr(v), V, Q._ptr(rhs), V, L.MO_KKT_TRANSPOSE, Q._ptr(out), V, Q._ptr(status), Q._stream()))
        L.check(L.lib().mo_qp_gradients(plan, C.byref(ps), B, Q._ptr(v), V, Q._ptr(out), V, C.byref(g), Q._stream()))
        torch.cuda.synchronize()

    try:
        both(plans[0])
        free0 = torch.cuda.mem_get_info()[0]
        both(plans[1])                                      # the FIRST launches of this plan
        assert torch.cuda.mem_get_info()[0] >= free0 - (1 << 20), (free0, torch.cuda.mem_get_info()[0])
        assert torch.all(status == 0) and torch.all(torch.isfinite(dJ))
    finally:
        for pl in plans:
            L.lib().mo_plan_destroy(pl)
