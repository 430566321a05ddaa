"""GPU tests of mo_kkt_solve on the fused fp64 kernels (run with -m gpu on an MI355X): the right-hand-side twin of the step kernel
(csrc/kkt_fused_rhs.hip) against LU on the oracle's full system, against the generic kernel on a MO_PLAN_FORCE_GENERIC plan and against the
fused Newton step; status words, layouts, scheduling, the launch path, solve_qp's autograd at n = 64 and one full-size launch.
Bound everywhere: TOL64 = 1e-10 rel-inf per problem, the project's BASELINE tolerance; every problem of every shape is held to it."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from mini_opt_amd import _lib as L
from mini_opt_amd import diff as D
from mini_opt_amd import qp as Q
from mini_opt_amd import synth
from oracle import oracle as orc
from tests import diff_reference as R
from tests import fused_rhs_reference as F
from tests import sens_fixtures as S
from tests.sens_fixtures import T, dev, device_problem, host_batch, oracle_kkt_solves, oracle_solver, rel_inf_rows

pytestmark = pytest.mark.gpu
TOL64 = 1e-10
CASES = [(s, lvl) for s, j_level in zip(F.SHAPES, F.J_LEVEL) for lvl in (("J", "G") if j_level else ("G",))]
IDS = [f"n{s[0]}k{s[1]}m{s[2]}-{lvl}" for s, lvl in CASES]
MO_STEP_NO_INEQUALITIES = 1


def expected_kernel(n, level):
    return "fused_rhs_%s_f64_n%d" % ("mfma" if level == "J" else "qp", 32 if n <= 32 else 64 if n <= 64 else 96 if n <= 96 else 128)


@contextlib.contextmanager
def Plan(prob, batch, flags=0, dtype=L.MO_F64):
    """The handle of a plan of this test's own (plan flags the cached plans of mini_opt_amd.diff do not have)."""
    with S.Plan(prob.n, prob.k, prob.m, prob.m_r, dtype, batch, flags) as plan:
        yield plan.h


def kkt_solve_on(plan, ps, v, rhs, flags=0, vars_stride=None, rhs_stride=None, out=None, out_stride=None):
    """mo_kkt_solve through the C ABI on `plan`; ps: the problem struct.  Returns (out, status)."""
    B, V = int(v.shape[0]), int(v.shape[1])
    out = torch.empty_like(v) if out is None else out
    status = torch.full((B,), -77, dtype=torch.int32, device=v.device)
    L.check(L.lib().mo_kkt_solve(plan, C.byref(ps), B, Q._ptr(v), vars_stride or V, Q._ptr(rhs), rhs_stride or V, flags, Q._ptr(out), out_stride or V,
                                 Q._ptr(status), Q._stream()))
    return out, status


def kernel_on(prob, flags=0, dtype=L.MO_F64, batch=8):
    ps = prob.as_struct()
    with Plan(prob, batch, flags, dtype) as plan:
        return L.lib().mo_plan_kkt_solve_kernel(plan, C.byref(ps)).decode()


def lu_references(hb, rhs, problems):
    n, k, m = hb.n, hb.k, hb.m
    ref_d, ref_t = np.zeros((len(problems), rhs.shape[1])), np.zeros((len(problems), rhs.shape[1]))
    for i, p in enumerate(problems):
        ref_d[i], ref_t[i] = oracle_kkt_solves(oracle_solver(hb, p, hb.vars[p]), n, k, m, rhs[p], rhs[p])
    return ref_d, ref_t


# ---- 1. which kernel serves the call -----------------------------------------------------------------------------------------------------------
def test_plan_names_the_fused_kernel_on_covered_shapes_and_generic_elsewhere():
    assert hasattr(L.lib(), "mo_plan_kkt_solve_kernel")
    for (n, k, m, m_r), level in CASES:
        prob = device_problem(host_batch(n, k, m, m_r, 2, stream=40), level)
        assert D.kkt_solve_kernel(prob, 2) == expected_kernel(n, level), ((n, k, m, m_r), level)
        assert kernel_on(prob) == expected_kernel(n, level)
        assert kernel_on(prob, L.MO_PLAN_FORCE_GENERIC) == "generic"
    for shape, level, kw in (((8, 2, 4, 16), "J", {}), ((8, 2, 4, 16), "G", {}), ((64, 32, 32, 128), "J", {}), ((64, 32, 32, 128), "G", {}),
                             ((80, 8, 130, 128), "J", {}), ((80, 8, 130, 128), "G", {}), ((64, 8, 32, 128), "J", dict(J_layout="col"))):
        prob = device_problem(host_batch(*shape, 2, stream=40), level, **kw)
        assert kernel_on(prob) == "generic", (shape, level, kw)
    prob32 = device_problem(host_batch(64, 8, 32, 128, 2, stream=40), "J", torch.float32)
    assert kernel_on(prob32, dtype=L.MO_F32) == "generic"


# ---- 2. random right-hand sides: LU on the oracle's matrix, and the generic kernel ---------------------------------------------------------------
@pytest.mark.parametrize("shape,level", CASES, ids=IDS)
def test_fused_kkt_solve_against_lu_and_against_the_generic_kernel(shape, level):
    n, k, m, m_r = shape
    B = 10
    hb = host_batch(n, k, m, m_r, B, stream=42)
    prob = device_problem(hb, level)
    ps = prob.as_struct()
    rhs = np.random.default_rng(42).normal(size=hb.vars.shape)
    v, rhs_d = T(hb.vars), T(rhs)
    ref_d, ref_t = lu_references(hb, rhs, range(B))
    with Plan(prob, B) as plan, Plan(prob, B, L.MO_PLAN_FORCE_GENERIC) as generic:
        assert L.lib().mo_plan_kkt_solve_kernel(plan, C.byref(ps)).decode() == expected_kernel(n, level)
        for flags, ref, tag in ((0, ref_d, "direct"), (L.MO_KKT_TRANSPOSE, ref_t, "transposed")):
            out, st = kkt_solve_on(plan, ps, v, rhs_d, flags)
            gen, st_g = kkt_solve_on(generic, ps, v, rhs_d, flags)
            assert torch.all(st == 0) and torch.all(st_g == 0), (tag, st, st_g)
            e_lu = rel_inf_rows(out.cpu().numpy(), ref)
            e_gen = rel_inf_rows(out.cpu().numpy(), gen.cpu().numpy())
            print(f"fused kkt_solve {shape} {level} {tag}: vs LU {e_lu.max():.3e}, vs generic {e_gen.max():.3e} (generic vs LU {rel_inf_rows(gen.cpu().numpy(), ref).max():.3e})")
            assert e_lu.max() < TOL64 and e_gen.max() < TOL64, (tag, e_lu, e_gen)
        if k:   # the system of [x | y] alone: the s and z blocks of rhs are ignored and written as 0
            for flags in (MO_STEP_NO_INEQUALITIES, MO_STEP_NO_INEQUALITIES | L.MO_KKT_TRANSPOSE):
                out, st = kkt_solve_on(plan, ps, v, rhs_d, flags)
                gen, _ = kkt_solve_on(generic, ps, v, rhs_d, flags)
                assert torch.all(st == 0)
                o = out.cpu().numpy()
                assert np.all(o[:, n:n + m] == 0) and np.all(o[:, n + m + k:] == 0)
                assert rel_inf_rows(o, gen.cpu().numpy()).max() < TOL64


# ---- 3. the Newton direction through the fused mo_kkt_solve ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,level", CASES, ids=IDS)
def test_fused_kkt_solve_of_the_residual_is_the_fused_newton_step(shape, level):
    n, k, m, m_r = shape
    hb = host_batch(n, k, m, m_r, 16, stream=43)
    prob = device_problem(hb, level)
    s = Q.QPInteriorPointSolver(prob)
    assert s.step_kernel().startswith("fused_") and D.kkt_solve_kernel(prob, 16) == expected_kernel(n, level)
    s.SetVariables(T(hb.vars))
    mu = T(hb.mu)
    delta, _, status = s.NewtonStep(mu, 0.995)
    assert torch.all(status == 0)
    rhs = s.EvaluateKKTConditions(mu)[0].clone()
    rhs[:, n:n + m] -= mu[:, None]
    out, st = D.kkt_solve(prob, s.variables(), rhs)
    assert torch.all(st == 0)
    err = rel_inf_rows(out.cpu().numpy(), delta.cpu().numpy())
    print(f"fused kkt_solve vs fused newton_step {shape} {level}: max rel-inf {err.max():.3e}")
    assert err.max() < TOL64
    if k:
        d0, _, st0 = s.NewtonStep(mu, 0.995, include_inequalities=False)
        r0 = s.EvaluateKKTConditions(mu, include_inequalities=False)[0].clone()
        out0, st1 = D.kkt_solve(prob, s.variables(), r0, include_inequalities=False)
        assert torch.all(st0 == 0) and torch.all(st1 == 0)
        assert rel_inf_rows(out0.cpu().numpy(), d0.cpu().numpy()).max() < TOL64


# ---- 4. status words -----------------------------------------------------------------------------------------------------------------------------
def test_fused_kkt_solve_status_words():
    n, k, m, m_r = 20, 3, 10, 22
    hb = host_batch(n, k, m, m_r, 8, stream=44)
    rhs = np.random.default_rng(44).normal(size=hb.vars.shape)
    good = device_problem(hb, "G")
    assert D.kkt_solve_kernel(good, 8) == "fused_rhs_qp_f64_n32"
    ref, st = D.kkt_solve(good, T(hb.vars), T(rhs))
    ref_t, st_t = D.kkt_solve(good, T(hb.vars), T(rhs), transpose=True)
    assert torch.all(st == 0) and torch.all(st_t == 0)
    clean_vars = hb.vars.copy()
    hb.vars[1, n] = 0.0                         # s = 0
    hb.cons_var[3, 0] = n + 3                   # constraint index out of range
    hb.G[5] = 0.0                               # an indefinite G whose first pivot is zero above a non-zero column
    hb.G[5, 0, 1] = hb.G[5, 1, 0] = 1.0
    hb.G[5][np.arange(2, n), np.arange(2, n)] = 1.0
    hb.cons_var[5][hb.cons_var[5] == 0] = 2     # (no Sigma on that pivot)
    bad = device_problem(hb, "G")
    others = [0, 2, 4, 6, 7]
    for transpose, want in ((False, ref), (True, ref_t)):
        out, st = D.kkt_solve(bad, T(hb.vars), T(rhs), transpose=transpose)
        st, o = st.cpu().numpy(), out.cpu().numpy()
        assert st[1] == L.MO_STATUS_NONPOSITIVE_SLACK and st[3] == L.MO_STATUS_BAD_INDEX and st[5] == L.MO_STATUS_FACTORIZATION_FAILED, st
        assert np.all(st[others] == 0)
        assert np.all(np.isnan(o[[1, 3, 5]]))
        assert np.array_equal(o[others], want.cpu().numpy()[others])   # the neighbours are unaffected, to the bit
        # a non-finite value in the caller's vector is that problem's alone, whichever block it sits in
        rhs2 = rhs.copy(); rhs2[2, 0] = np.nan; rhs2[4, n + m + k + 1] = np.nan; rhs2[6, n + m] = np.inf; rhs2[7, n + 2] = np.nan
        out, st = D.kkt_solve(good, T(clean_vars), T(rhs2), transpose=transpose)
        st, o = st.cpu().numpy(), out.cpu().numpy()
        assert np.all(st[[2, 4, 6, 7]] == L.MO_STATUS_NONFINITE) and np.all(st[[0, 1, 3, 5]] == 0), st
        assert np.all(np.isnan(o[[2, 4, 6, 7]]))
        assert np.array_equal(o[[0, 1, 3, 5]], want.cpu().numpy()[[0, 1, 3, 5]])


# ---- 5. layout -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,level", [((64, 8, 32, 128), "J"), ((20, 3, 10, 22), "G"), ((96, 31, 64, 192), "J")], ids=["cfg3-J", "n20-G", "n96k31-J"])
def test_fused_kkt_solve_strides_alignment_and_shared_equalities(shape, level):
    n, k, m, m_r = shape
    B = 9
    hb = host_batch(n, k, m, m_r, B, stream=45)
    hb.A_eq[:] = hb.A_eq[0]                     # one A_eq for the whole batch (stride 0)
    prob = device_problem(hb, level)
    ps = prob.as_struct()
    ps.A_stride = 0
    V = hb.vars.shape[1]
    rhs = np.random.default_rng(45).normal(size=hb.vars.shape)
    ref_d, ref_t = lu_references(hb, rhs, range(B))
    CANARY = -777.25
    sv, sr, so = V + 3, V + 5, V + 7            # strides beyond V; rhs and out start 8 bytes past a 16-byte boundary

    def padded(a, stride, offset):
        buf = torch.full((offset + B * stride,), CANARY, dtype=torch.float64, device=dev())
        view = buf[offset:].view(B, stride)
        if a is not None:
            view[:, :V] = T(a)
        return buf, view

    _, v_view = padded(hb.vars, sv, 0)
    _, rhs_view = padded(rhs, sr, 1)
    with Plan(prob, B) as plan:
        assert L.lib().mo_plan_kkt_solve_kernel(plan, C.byref(ps)).decode() == expected_kernel(n, level)
        for flags, ref in ((0, ref_d), (L.MO_KKT_TRANSPOSE, ref_t)):
            out_buf, out_view = padded(None, so, 1)
            assert rhs_view.data_ptr() % 16 == 8 and out_view.data_ptr() % 16 == 8
            status = torch.full((B,), -77, dtype=torch.int32, device=dev())
            L.check(L.lib().mo_kkt_solve(plan, C.byref(ps), B, v_view.data_ptr(), sv, rhs_view.data_ptr(), sr, flags, out_view.data_ptr(), so,
                                         Q._ptr(status), Q._stream()))
            torch.cuda.synchronize()
            assert torch.all(status == 0)
            o = out_view.cpu().numpy()
            assert rel_inf_rows(o[:, :V], ref).max() < TOL64
            assert np.all(o[:, V:] == CANARY) and float(out_buf[0]) == CANARY     # nothing is written outside the V values of a problem


# ---- 6. scheduling ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan_flag", [L.MO_PLAN_TICKETS_ALWAYS, L.MO_PLAN_STATIC_ROUNDS_ALWAYS, 0], ids=["tickets", "static-rounds", "default"])
@pytest.mark.parametrize("shape", [(64, 8, 32, 128), (32, 16, 40, 64)], ids=["cfg3", "n32k16"])
def test_fused_kkt_solve_under_both_schedules(shape, plan_flag):
    """13 000 problems on at most 3 072 waves: every wave takes several.  The batch is 250 distinct problems, repeated: every copy of a
    problem must give the bits of the first, whichever wave ran it; the distinct ones are held to LU and to the generic kernel."""
    n, k, m, m_r = shape
    U, B = 250, 13000
    hb = host_batch(n, k, m, m_r, U, stream=46)
    rhs = np.random.default_rng(46).normal(size=hb.vars.shape)
    rep = lambda t: t.repeat((B + U - 1) // U, *([1] * (t.dim() - 1)))[:B].contiguous()
    small = device_problem(hb, "J")
    big = Q.BatchedQP(n=n, k=k, m=m, J=rep(small.J), r=rep(small.r), lam=hb.lam, A_eq=rep(small.A_eq), b_eq=rep(small.b_eq),
                      cons_var=rep(small.cons_var), cons_a=rep(small.cons_a), cons_b=rep(small.cons_b))
    ps, ps_small = big.as_struct(), small.as_struct()
    v, rhs_d = rep(T(hb.vars)), rep(T(rhs))
    ref_d, ref_t = lu_references(hb, rhs, range(0, U, 5))
    with Plan(big, B, plan_flag) as plan, Plan(small, U, L.MO_PLAN_FORCE_GENERIC) as generic:
        assert L.lib().mo_plan_kkt_solve_kernel(plan, C.byref(ps)).decode() == expected_kernel(n, "J")
        for flags, ref in ((0, ref_d), (L.MO_KKT_TRANSPOSE, ref_t)):
            out, st = kkt_solve_on(plan, ps, v, rhs_d, flags)
            again, st2 = kkt_solve_on(plan, ps, v, rhs_d, flags)
            gen, st_g = kkt_solve_on(generic, ps_small, v[:U].contiguous(), rhs_d[:U].contiguous(), flags)
            assert torch.all(st == 0) and torch.all(st2 == 0) and torch.all(st_g == 0)
            assert torch.equal(out, again)                                      # two launches, the same bits
            assert torch.equal(out, rep(out[:U]))                               # every copy of a problem, the same bits
            o = out[:U].cpu().numpy()
            assert rel_inf_rows(o, gen.cpu().numpy()).max() < TOL64
            assert rel_inf_rows(o[::5], ref).max() < TOL64


# ---- 7. the launch path ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,level", [((64, 8, 32, 128), "J"), ((32, 16, 40, 64), "G")], ids=["cfg3-J", "n32k16-G"])
def test_fused_kkt_solve_is_graph_capturable(shape, level):
    """mo_kkt_solve enqueues at most an 8-byte memset and one kernel on the caller's stream: it can be captured into a HIP graph and
    replayed on new data in the same buffers."""
    n, k, m, m_r = shape
    B = 64
    hb = host_batch(n, k, m, m_r, B, stream=47)
    prob = device_problem(hb, level)
    ps = prob.as_struct()
    rhs = np.random.default_rng(47).normal(size=hb.vars.shape)
    v, rhs_d = T(hb.vars), T(rhs)
    out = torch.empty_like(v)
    with Plan(prob, B) as plan:
        assert L.lib().mo_plan_kkt_solve_kernel(plan, C.byref(ps)).decode() == expected_kernel(n, level)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            kkt_solve_on(plan, ps, v, rhs_d, L.MO_KKT_TRANSPOSE, out=out)     # warm-up outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _, status = kkt_solve_on(plan, ps, v, rhs_d, L.MO_KKT_TRANSPOSE, out=out)
        hb2 = host_batch(n, k, m, m_r, B, stream=48)
        rhs2 = np.random.default_rng(48).normal(size=hb.vars.shape)
        v.copy_(T(hb2.vars)); rhs_d.copy_(T(rhs2))
        if level == "J":
            prob.J.copy_(T(hb2.J)); prob.r.copy_(T(hb2.r))
        else:
            prob.G.copy_(T(hb2.G)); prob.c.copy_(T(hb2.c))
        prob.A_eq.copy_(T(hb2.A_eq)); prob.b_eq.copy_(T(hb2.b_eq))
        prob.cons_var.copy_(T(hb2.cons_var, torch.int32)); prob.cons_a.copy_(T(hb2.cons_a)); prob.cons_b.copy_(T(hb2.cons_b))
        out.fill_(0.0)
        graph.replay()
        torch.cuda.synchronize()
        _, ref_t = lu_references(hb2, rhs2, range(0, B, 4))
        assert torch.all(status == 0)
        assert rel_inf_rows(out.cpu().numpy()[::4], ref_t).max() < TOL64


@pytest.mark.parametrize("shape,level", [((32, 16, 40, 64), "G"), ((128, 14, 64, 256), "J")], ids=["n32k16-G", "n128-J"])
def test_first_fused_kkt_solve_allocates_nothing(shape, level):
    n, k, m, m_r = shape
    B = 96
    hb = host_batch(n, k, m, m_r, B, stream=49)
    prob = device_problem(hb, level)
    ps = prob.as_struct()
    v, rhs = T(hb.vars), T(np.random.default_rng(49).normal(size=hb.vars.shape))
    out = torch.empty_like(v)
    with Plan(prob, B) as warm, Plan(prob, B) as plan:
        assert L.lib().mo_plan_kkt_solve_kernel(plan, C.byref(ps)).decode() == expected_kernel(n, level)
        # what the HIP runtime reserves on its own account (module load, kernel code) happens on ANOTHER plan of the same shape first
        _, st = kkt_solve_on(warm, ps, v, rhs, L.MO_KKT_TRANSPOSE, out=out)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        _, st = kkt_solve_on(plan, ps, v, rhs, L.MO_KKT_TRANSPOSE, out=out)                 # the FIRST launch of this plan
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] >= free0 - (1 << 20), (free0, torch.cuda.mem_get_info()[0])
        assert torch.all(st == 0) and torch.all(torch.isfinite(out))


# ---- 8. autograd end to end at n = 64 ---------------------------------------------------------------------------------------------------------------
PARAMS = dict(initial_mu=1.0, sigma=0.1, termination_kkt_tol=1e-9, termination_complementarity_tol=1e-9, max_iterations=40)
E2E_SEED, E2E_B = 2025, 24


def e2e_problems():
    """n = 64, k = 4, m = 16: J ~ U(-1, 1) / sqrt(m_r) with m_r = 128 (G = J^T J + 1e-2 I), r ~ 4 N(0, 1) so that the unconstrained optimum
    leaves the boxes, A_eq ~ U(-1, 1), b_eq ~ U(-0.1, 0.1), single-variable rows on 16 distinct variables with a = +-1, b ~ U(0.1, 1)."""
    rng = np.random.default_rng(E2E_SEED)
    n, k, m, m_r, B = 64, 4, 16, 128, E2E_B
    J = rng.uniform(-1, 1, (B, m_r, n)) / np.sqrt(m_r)
    r = 4 * rng.normal(size=(B, m_r))
    lam = np.full(B, 1e-2)
    A = rng.uniform(-1, 1, (B, k, n))
    b_eq = rng.uniform(-0.1, 0.1, (B, k))
    var = np.stack([rng.permutation(n)[:m] for _ in range(B)]).astype(np.int32)
    a = rng.choice([-1.0, 1.0], (B, m))
    b = rng.uniform(0.1, 1.0, (B, m))
    gx = rng.normal(size=(B, n))
    G = np.einsum("bqi,bqj->bij", J, J) + lam[:, None, None] * np.eye(n)
    c = np.einsum("bqi,bq->bi", J, r)
    return dict(n=n, k=k, m=m, m_r=m_r, J=J, r=r, lam=lam, A=A, b_eq=b_eq, var=var, a=a, b=b, gx=gx, G=G, c=c)


def test_autograd_at_n64_reaches_the_fused_kernel_and_matches_lu():
    """Device gradients against tests/diff_reference.py evaluated AT THE DEVICE'S OWN v (LU on the full K), for (G, c) and for (J, r, lam)
    input.  Bound max(TOL64, 10 D), the rule of tests/test_gpu_diff.py::test_autograd_with_active_inequalities: D is measured on the CPU
    without the code under test -- at the ORACLE's Solve output of the same problems, the largest rel-inf between u from LU on the full
    matrix and u from the reduced system in numpy; the factor 10 covers an unpivoted LDL^T against a pivoted LU.  No problem is excused;
    at least half of the problems must have an active row (s < 1e-6).  A problem whose forward fails still gets zero gradients."""
    P = e2e_problems()
    n, k, m, B = P["n"], P["k"], P["m"], E2E_B
    g_full = np.concatenate([P["gx"], np.zeros((B, 2 * m + k))], axis=1)
    D_cpu = 0.0
    for p in range(B):
        o = orc.Solver(orc.QP(G=np.tril(P["G"][p]), c=P["c"][p], A_eq=P["A"][p], b_eq=P["b_eq"][p], cons_var=P["var"][p], cons_a=P["a"][p], cons_b=P["b"][p]))
        o.solve(**PARAMS)
        _, u_lu = oracle_kkt_solves(o, n, k, m, g_full[p], g_full[p])
        u_red = R.transposed_through_reduced(P["G"][p], P["A"][p], P["var"][p], P["a"][p], np.array(o.variables), g_full[p])
        D_cpu = max(D_cpu, float(rel_inf_rows(u_red[None], u_lu[None])[0]))
    bound = max(TOL64, 10 * D_cpu)
    worst, active = {}, 0
    for level in ("G", "J"):
        names = ("G", "c", "A", "b_eq", "a", "b") if level == "G" else ("J", "r", "lam", "A", "b_eq", "a", "b")
        leaves = {key: T(P[key]).requires_grad_(True) for key in names}
        cost = dict(G=leaves["G"], c=leaves["c"]) if level == "G" else dict(J=leaves["J"], r=leaves["r"], lam=leaves["lam"])
        x, s, y, z, status = D.solve_qp(A_eq=leaves["A"], b_eq=leaves["b_eq"], cons_var=T(P["var"], torch.int32), cons_a=leaves["a"], cons_b=leaves["b"],
                                        params=Q.Params(**PARAMS), return_all=True, return_status=True, **cost)
        assert torch.all(status == 0)
        node_problem = Q.BatchedQP(n=n, k=k, m=m, A_eq=T(P["A"].transpose(0, 2, 1)), b_eq=T(P["b_eq"]), cons_var=T(P["var"], torch.int32), cons_a=T(P["a"]),
                                   cons_b=T(P["b"]), **({"G": T(P["G"]), "c": T(P["c"])} if level == "G" else {"J": T(P["J"]), "r": T(P["r"]), "lam": 1e-2}))
        assert D.kkt_solve_kernel(node_problem, B) == expected_kernel(n, level)
        (x * T(P["gx"])).sum().backward()
        assert torch.all(D.adjoint_status(x) == 0)
        v = torch.cat([x, s, y, z], dim=1).detach().cpu().numpy()
        if level == "G":
            active = int(np.sum(np.min(v[:, n:n + m], axis=1) < 1e-6))
        for p in range(B):
            Kp = R.kkt_matrix(P["G"][p], P["A"][p], P["var"][p], P["a"][p], v[p])
            gr = R.gradients(n, k, m, P["var"][p], v[p], R.solve_transposed(Kp, g_full[p]), J=P["J"][p], r=P["r"][p])
            ref = dict(G=gr["G"], c=gr["c"], J=gr["J"], r=gr["r"], lam=gr["lam"], A=gr["A_eq"], b_eq=gr["b_eq"], a=gr["cons_a"], b=gr["cons_b"])
            for key in names:
                got = leaves[key].grad[p].cpu().numpy().reshape(-1)
                want = np.atleast_1d(ref[key]).reshape(-1)
                err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
                worst[(level, key)] = max(worst.get((level, key), 0.0), err)
    print(f"n = 64 autograd: D = {D_cpu:.3e} (seed {E2E_SEED}, {B} problems), bound {bound:.3e}, {active} of {B} problems with an active row, worst rel-inf {worst}")
    assert 2 * active >= B, (active, B)
    assert max(worst.values()) < bound, (worst, bound)
    # one failing problem inside the batch: zero gradient rows for it, the others to the bit what they are without it
    out = []
    for broken in (False, True):
        var = P["var"].copy()
        if broken:
            var[5, 3] = n + 1
        leaves = [T(P[key]).requires_grad_(True) for key in ("G", "c", "A", "b_eq", "a", "b")]
        x, status = D.solve_qp(G=leaves[0], c=leaves[1], A_eq=leaves[2], b_eq=leaves[3], cons_var=T(var, torch.int32), cons_a=leaves[4], cons_b=leaves[5],
                               params=Q.Params(**PARAMS), return_status=True)
        x.backward(torch.ones_like(x))
        out.append(([t.grad.clone() for t in leaves], status.cpu().numpy(), D.adjoint_status(x).cpu().numpy()))
    (g_ok, st_ok, adj_ok), (g_bad, st_bad, adj_bad) = out
    others = [p for p in range(B) if p != 5]
    assert np.all(st_ok == 0) and np.all(adj_ok == 0)
    assert st_bad[5] == L.MO_STATUS_BAD_INDEX and adj_bad[5] != 0 and np.all(st_bad[others] == 0) and np.all(adj_bad[others] == 0)
    for t_ok, t_bad in zip(g_ok, g_bad):
        assert torch.all(t_bad[5] == 0) and torch.all(torch.isfinite(t_bad))
        assert torch.equal(t_bad[others], t_ok[others]) and torch.any(t_ok[5] != 0)


# ---- 9. one full-size launch ---------------------------------------------------------------------------------------------------------------------------
def test_full_size_transposed_launch():
    n, k, m, m_r, B = 64, 8, 32, 128, 65536
    prob, v, _ = synth.make_batch_torch(n, k, m, m_r, B, dev(), torch.float64)
    gen = torch.Generator(device=dev()); gen.manual_seed(50)
    g = torch.randn(B, prob.V, generator=gen, device=dev(), dtype=torch.float64)
    assert D.kkt_solve_kernel(prob, B) == "fused_rhs_mfma_f64_n64"
    u, status = D.kkt_solve(prob, v, g, transpose=True)
    assert torch.all(status == 0)
    idx = torch.arange(0, B, 256, device=dev())
    h = {key: getattr(prob, key)[idx].cpu().numpy() for key in ("J", "A_eq", "cons_var", "cons_a")}
    vs, gs, us = v[idx].cpu().numpy(), g[idx].cpu().numpy(), u[idx].cpu().numpy()
    ref = np.zeros_like(us)
    for i in range(len(idx)):
        G = h["J"][i].T @ h["J"][i] + prob.lam * np.eye(n)
        ref[i] = R.solve_transposed(R.kkt_matrix(G, h["A_eq"][i].T, h["cons_var"][i], h["cons_a"][i], vs[i]), gs[i])
    err = rel_inf_rows(us, ref)
    print(f"full-size transposed launch: {len(idx)} sampled problems, max rel-inf vs LU {err.max():.3e}")
    assert len(idx) == 256 and err.max() < TOL64
