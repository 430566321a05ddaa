"""Every QP entry point of the C ABI with the problem data somewhere else in memory (run with -m gpu on an MI355X).

tests/layout_cases.py holds the cases and the layouts; tests/test_layout_dispatch_cpu.py proves on the CPU that the packed, the same-stream
scattered and the shared layout of a call select the same template instantiation (it prints the instantiations: the fused fp64 units main,
gather, ny2, ny34, mc4 and tiny, the fp32 unit, the generic kernel LDS-resident and LARGE).  Every test here does, on ONE plan:

 1. the packed call, against the reference of that call at the tolerance its existing packed test uses (named in the test's docstring);
 2. the scattered call: every output the same BITS as the packed call's -- the same instantiation on the same numbers, no atomics in the
    arithmetic; with the J stream moved (fp64: gather stream, fp32: generic kernel) the reference's tolerance and rtol = 1e-12 against
    packed where the existing J-layout test asserts it;
 3. canaries: no input changed, and no element outside an output's own elements touched -- the elements in front of every base, the pads
    between rows, the columns of G_out beyond n, the guard behind the last row;
 4. the shared layout (every input stride 0) against the packed call on the replicated batch, bit for bit (step and Solve);
 5. once per kernel family, every output documented "may be NULL" as NULL: the remaining outputs keep their bits.
The store sites of those outputs were read first: every one is behind a test of its pointer in kkt_fused.hip, kkt_fused_tiny.hip,
kkt_fused_f32.hip and kkt_generic.hip."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from mini_opt_amd import _lib as L
from mini_opt_amd import qp as Q
from oracle import oracle as orc
from tests import layout_cases as LC
from tests import sens_fixtures as SF

pytestmark = pytest.mark.gpu
B = LC.B
DEV = "cuda:0"
NULL_FAMILIES = [("tiny", "J"), ("diag4", "J"), ("f32-64", "J"), ("gen-f64", "J")]   # one-tile, fused fp64 step + Solve, fused fp32, generic
J_ITEMS = [(cid, level) for cid, level in LC.ITEMS if level == "J"]
IDS = lambda items: ["%s-%s" % it for it in items]


def rel_inf_rows(got, ref):
    return np.max(np.abs(got - ref), axis=1) / np.max(np.abs(ref), axis=1)


def is_f32(case):
    return case.dtype == "f32"


@contextlib.contextmanager
def Plan(case, level, k=None, m=None, force_generic=False):
    """The handle of a plan of this test's own for a case of tests/layout_cases.py."""
    n, k0, m0, m_r = case.shape
    flags = (L.MO_PLAN_FORCE_GENERIC if case.force_generic or force_generic else 0) | (L.MO_PLAN_NO_TINY if case.no_tiny else 0)
    with SF.Plan(n, k0 if k is None else k, m0 if m is None else m, m_r if level == "J" else 0, L.MO_F32 if is_f32(case) else L.MO_F64, B, flags) as plan:
        yield plan.h


def ptr(buf):
    return None if buf is None else buf.ptr


def collect(env, tag, **bufs):
    """Synchronise, check the canaries of the call, return the data elements of its outputs."""
    torch.cuda.synchronize()
    env.check(tag)
    if env.variant in ("scattered", "moved"):                   # the outputs with a stride of their own: an odd number of elements into their allocation
        for name, buf in bufs.items():
            assert buf is None or buf.lay_name is None or buf.address() % 16 == buf.buf.element_size(), (tag, name)
    return {name: buf.get().clone() for name, buf in bufs.items() if buf is not None}


# ---- the calls: each allocates its outputs in the layout of `env`, passes NULL for the names in `null` ------------------------------------------
def newton_step(plan, env, flags=0, null=()):
    lay = env.lay
    delta = env.out("delta")
    alpha = None if "alpha" in null else env.out("alpha", 2)
    status = None if "status" in null else env.out("status", 1, torch.int32)
    L.check(L.lib().mo_newton_step(plan, C.byref(env.prob), B, env.inputs["vars"].ptr, lay["vars"].stride, env.inputs["mu"].ptr, lay["mu"].stride, 0.995,
                                   flags, delta.ptr, lay["delta"].stride, ptr(alpha), ptr(status), Q._stream()))
    return collect(env, "mo_newton_step", delta=delta, alpha=alpha, status=status)


def kkt_residual(plan, env, null=()):
    lay = env.lay
    r_out = env.out("r_out")
    kkt = None if "kkt_out" in null else env.out("kkt_out", 4)
    L.check(L.lib().mo_kkt_residual(plan, C.byref(env.prob), B, env.inputs["vars"].ptr, lay["vars"].stride, env.inputs["mu"].ptr, lay["mu"].stride, 0,
                                    r_out.ptr, lay["r_out"].stride, ptr(kkt), Q._stream()))
    return collect(env, "mo_kkt_residual", r_out=r_out, kkt_out=kkt)


def iterate(plan, env, data, strategy, null=()):
    lay = env.lay
    state = env.state(data["vars"])
    delta = None if "delta" in null else env.out("delta")
    ip = None if "ip_out" in null else env.out("ip_out", 6)
    status = env.out("status", 1, torch.int32)
    L.check(L.lib().mo_iterate(plan, C.byref(env.prob), B, state.ptr, lay["vars"].stride, env.inputs["mu"].ptr, lay["mu"].stride, strategy, ptr(delta),
                               lay["delta"].stride, ptr(ip), status.ptr, Q._stream()))
    return collect(env, "mo_iterate", vars=state, delta=delta, ip_out=ip, status=status)


def solve_params(case, strategy):
    """As test_fused_kernels_take_every_layout_of_J (fp32: the tolerances of test_fused_f32_solve_iterate_residual)."""
    k = case.shape[1]
    kw = dict(initial_mu=1.0, sigma=0.1, termination_kkt_tol=1e-8, max_iterations=12)
    if is_f32(case):
        kw = dict(initial_mu=1.0, sigma=0.1, termination_kkt_tol=2e-3, termination_complementarity_tol=1e-3, max_iterations=14)
    return Q.Params(barrier_strategy=strategy, initial_guess_method=Q.SOLVE_EQUALITY_CONSTRAINED if k else Q.NAIVE, **kw)


def qp_solve(plan, env, data, strategy, null=()):
    lay = env.lay
    params = solve_params(env.case, strategy)
    sp = params.as_struct()
    state = env.state(data["vars"])
    term, nit, status = (env.out(name, 1, torch.int32) for name in ("termination", "num_iterations", "status"))
    its = None if "iterations" in null else env.out("iterations", params.max_iterations * L.MO_ITER_RECORD)
    lag = None if "lagrange" in null else env.out("lagrange", 2)
    L.check(L.lib().mo_qp_solve(plan, C.byref(env.prob), B, C.byref(sp), state.ptr, lay["vars"].stride, term.ptr, nit.ptr, ptr(its), ptr(lag), status.ptr,
                                Q._stream()))
    return collect(env, "mo_qp_solve", vars=state, termination=term, num_iterations=nit, iterations=its, lagrange=lag, status=status)


def linearize(plan, env, null=()):
    lay = env.lay
    G, c = env.out("G_out"), env.out("c_out")
    half = None if "half_sq_out" in null else env.out("half_sq_out", 1)
    L.check(L.lib().mo_linearize(plan, C.byref(env.prob), B, G.ptr, lay["G_out"].stride, lay["G_out"].ld, c.ptr, lay["c_out"].stride, ptr(half), Q._stream()))
    return collect(env, "mo_linearize", G_out=G, c_out=c, half_sq_out=half)


# ---- what the layouts of a call must give ---------------------------------------------------------------------------------------------------------
def assert_same_bits(got, want, tag):
    assert got.keys() == want.keys(), tag
    for name in want:
        assert LC.same_bits(got[name], want[name]), (tag, name, "differs from the packed call's bits",
                                                     int((got[name] != want[name]).sum()), "of", got[name].numel(), "elements")


def assert_alignments(env):
    """The bases of the scattered layout: an odd number of elements into their allocation (J: 16-byte aligned when its stream stays)."""
    e = LC.elem(env.case)
    for name, rem in env.alignments().items():
        if name == "J":
            assert rem == (e if env.variant == "moved" else 0), (name, rem)
        elif name == "r" and env.lay["r"].offset == 4:
            assert rem == 0
        else:
            assert rem == (4 if name == "cons_var" else e), (name, rem)


def reported_kernel(plan, env, query):
    return getattr(L.lib(), query)(plan, C.byref(env.prob)).decode()


def run_layouts(case, level, call, check_packed, check_moved=None, shared=False, plan_kw=None, moved_rtol=True, env_kw=None, query=None):
    """Steps 1 .. 4 of the module docstring for one call(plan, env, data) -> outputs.  query: the plan's kernel query for this call
    (mo_plan_step_kernel / mo_plan_solve_kernel): the same name in the packed, the scattered and the shared layout."""
    data = LC.case_data(case.id)
    with Plan(case, level, **(plan_kw or {})) as plan:
        packed = LC.Env(case, level, "packed", data, DEV)
        if query:
            name = reported_kernel(plan, packed, query)
            assert (name == "generic") == (case.key is None or (is_f32(case) and level == "G" and query == "mo_plan_step_kernel")), (case.id, level, name)
            others = [LC.Env(case, level, "scattered", data, DEV)] + ([LC.Env(case, level, "shared", LC.case_data(case.id, shared=True), DEV)] if shared else [])
            assert all(reported_kernel(plan, env, query) == name for env in others), (case.id, level, name)
            if case.moved and level == "J" and is_f32(case):
                assert reported_kernel(plan, LC.Env(case, level, "moved", data, DEV), query) == "generic"
        out_p = call(plan, packed, data)
        check_packed(out_p, data)
        env = LC.Env(case, level, "scattered", data, DEV, **(env_kw or {}))
        assert_alignments(env)
        out_s = call(plan, env, data)
        assert_same_bits(out_s, out_p, (case.id, level, "scattered"))
        if case.moved and level == "J":
            env = LC.Env(case, level, "moved", data, DEV)
            assert_alignments(env)
            out_m = call(plan, env, data)
            (check_moved or check_packed)(out_m, data)
            if moved_rtol and not is_f32(case):       # the gather stream feeds the matrix cores the same operands in the same order
                for name in out_p:
                    np.testing.assert_allclose(out_m[name].cpu().numpy(), out_p[name].cpu().numpy(), rtol=1e-12, atol=1e-13, equal_nan=True, err_msg=name)
        if shared:
            rep = LC.case_data(case.id, shared=True)
            env_r = LC.Env(case, level, "packed", rep, DEV, wrong_lambda=False)
            env_r.prob.lambda_vec, env_r.prob.lambda_stride = None, 0            # one scalar lambda, as the shared layout
            want = call(plan, env_r, rep)
            got = call(plan, LC.Env(case, level, "shared", rep, DEV), rep)
            assert_same_bits(got, want, (case.id, level, "shared"))


# ---- references ---------------------------------------------------------------------------------------------------------------------------------------
def oracle_qp(data, p):
    k, m = data["b"].shape[1], data["cv"].shape[1]
    return orc.QP(G=np.tril(data["G"][p]), c=data["c"][p], A_eq=data["A"][p].T if k else None, b_eq=data["b"][p] if k else None,
                  cons_var=data["cv"][p], cons_a=data["ca"][p], cons_b=data["cb"][p])


@functools.lru_cache(maxsize=None)
def oracle_step(cid, no_ineq=False):
    """oracle.batched_newton_step on the case's (fp32-rounded, for fp32) inputs, G = J^T J + lambda_p I formed in float64."""
    case, data = LC.BY_ID[cid], LC.case_data(cid)
    n, k, m, _ = case.shape
    Gl = np.tril(data["G"]).transpose(0, 2, 1).copy()
    if no_ineq:                                                 # the problem without its inequalities, state [x | y]
        v = np.concatenate([data["vars"][:, :n], data["vars"][:, n + m:n + m + k]], axis=1)
        ref, alpha, status, _ = orc.batched_newton_step(n, k, 0, G=Gl, c=data["c"], A_eq=data["A"] if k else None, b_eq=data["b"] if k else None, vars_=v, mu=data["mu"])
    else:
        ref, alpha, status, _ = orc.batched_newton_step(n, k, m, G=Gl, c=data["c"], A_eq=data["A"] if k else None, b_eq=data["b"] if k else None,
                                                        cons_var=data["cv"], cons_a=data["ca"], cons_b=data["cb"], vars_=data["vars"], mu=data["mu"])
    assert np.all(status == 0)
    return ref, alpha, status


@functools.lru_cache(maxsize=None)
def oracle_residual(cid):
    data = LC.case_data(cid)
    r, kkt = [], []
    for p in range(B):
        o = orc.Solver(oracle_qp(data, p))
        o.variables[:] = data["vars"][p]
        o.evaluate_kkt(True)
        e = o.compute_errors(float(data["mu"][p]))
        r.append(np.array(o.r)); kkt.append([e.r_dual, e.r_comp, e.r_primal_eq, e.r_primal_ineq])
    return np.array(r), np.array(kkt)


def check_step(case):
    tol, atol = (2e-3, 5e-3) if is_f32(case) else (1e-10, 1e-9)

    def check(out, data):
        ref, ref_alpha, ref_status = oracle_step(case.id)
        err = rel_inf_rows(out["delta"].double().cpu().numpy(), ref).max()
        print("%s step: max rel-inf vs oracle %.3e" % (case.id, err))
        assert np.array_equal(out["status"].cpu().numpy().ravel(), ref_status)
        assert err < tol, err
        np.testing.assert_allclose(out["alpha"].double().cpu().numpy(), ref_alpha, rtol=0, atol=atol)
    return check


# ---- 1. mo_newton_step: every case ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,level", LC.ITEMS, ids=IDS(LC.ITEMS))
def test_newton_step_in_every_layout(cid, level):
    """Packed: delta within 1e-10 rel-inf of oracle.batched_newton_step, status equal, alpha within 1e-9 -- the bound of
    test_gpu_fused_diag.py::test_step_against_oracle and test_gpu_parity.py::test_batch_vs_oracle (fused, one-tile and generic fp64 alike);
    fp32: 2e-3 and 5e-3 on fp32-rounded inputs (test_gpu_parity.py::test_fused_f32_shapes, ::test_batch_vs_oracle).  Moved stream: the
    same, and rtol = 1e-12 against packed in fp64 (test_fused_kernels_take_every_layout_of_J)."""
    case = LC.BY_ID[cid]
    run_layouts(case, level, lambda plan, env, data: newton_step(plan, env), check_step(case), shared=True, query="mo_plan_step_kernel")


def test_newton_step_without_inequalities_in_every_layout():
    """MO_STEP_NO_INEQUALITIES on the 32 grid: dx, dy of the problem without its inequalities within 1e-10 of the oracle on that problem,
    ds = dz = 0, alpha = 1 (test_gpu_parity.py::test_fused_f32_shapes does the same in fp32)."""
    case = LC.BY_ID["n32"]
    n, k, m, _ = case.shape

    def check(out, data):
        ref, _, _ = oracle_step(case.id, True)
        d = out["delta"].cpu().numpy()
        assert np.all(out["status"].cpu().numpy() == 0) and np.all(out["alpha"].cpu().numpy() == 1.0)
        assert np.all(d[:, n:n + m] == 0) and np.all(d[:, n + m + k:] == 0)
        assert rel_inf_rows(np.concatenate([d[:, :n], d[:, n + m:n + m + k]], axis=1), ref).max() < 1e-10
    run_layouts(case, "J", lambda plan, env, data: newton_step(plan, env, L.MO_STEP_NO_INEQUALITIES), check, shared=True)


# ---- 2. mo_kkt_residual: every case ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,level", LC.ITEMS, ids=IDS(LC.ITEMS))
def test_kkt_residual_in_every_layout(cid, level):
    """Packed: r_out within 1e-11 max(1, |r|_max) of oracle.Solver.evaluate_kkt per problem (fp32: 2e-4), the bound of
    test_gpu_parity.py::test_sizes_beyond_every_lds_resident_kernel; the four norms against compute_errors at rtol = 1e-6, atol = 1e-9, the
    bound test_gpu_parity.py::test_full_solve_kats holds the recorded norms to (fp32: rtol 2e-3, atol 2e-4 scale, as
    ::test_fused_f32_solve_iterate_residual)."""
    case = LC.BY_ID[cid]

    def check(out, data):
        ref_r, ref_kkt = oracle_residual(case.id)
        scale = max(1.0, np.abs(ref_r).max())
        np.testing.assert_allclose(out["r_out"].double().cpu().numpy(), ref_r, rtol=0, atol=(2e-4 if is_f32(case) else 1e-11) * scale)
        rtol, atol = (2e-3, 2e-4 * scale) if is_f32(case) else (1e-6, 1e-9)
        np.testing.assert_allclose(out["kkt_out"].double().cpu().numpy(), ref_kkt, rtol=rtol, atol=atol)
    run_layouts(case, level, lambda plan, env, data: kkt_residual(plan, env), check)


# ---- 3. mo_iterate and mo_qp_solve: against the generic kernel, as the existing layout test ---------------------------------------------------------------------
def against_generic(case, level, call):
    """check(out, data): `out` against the same call on a MO_PLAN_FORCE_GENERIC plan in the packed layout -- the state after Iterate at
    rtol = 1e-8, atol = 1e-10 (test_gpu_parity.py::test_fused_odd_n_with_stacked_jacobian; fp32: 5e-3 rel-inf,
    ::test_fused_f32_solve_iterate_residual); the optimum of Solve at rtol = 1e-6, atol = 1e-8 (fp32: 5e-3 max(1, |x|_max)) on the problems
    both kernels end SATISFIED_KKT_TOL in the same number of iterations (the same tests).  The reference of these two calls is the existing
    suite; here they anchor the bit comparison."""
    n = case.shape[0]
    cache = {}

    def check(out, data):
        assert torch.all(out["status"] == 0), out["status"]
        if case.key is None:
            return                                              # the generic kernel itself
        if "ref" not in cache:
            with Plan(case, level, force_generic=True) as generic:
                cache["ref"] = call(generic, LC.Env(case, level, "packed", data, DEV), data)
        ref = cache["ref"]
        got_v, ref_v = out["vars"].double().cpu().numpy(), ref["vars"].double().cpu().numpy()
        if "termination" not in out:
            if is_f32(case):
                assert rel_inf_rows(got_v, ref_v).max() < 5e-3
            else:
                np.testing.assert_allclose(got_v, ref_v, rtol=1e-8, atol=1e-10)
            return
        same = ((out["termination"] == Q.SATISFIED_KKT_TOL) & (ref["termination"] == Q.SATISFIED_KKT_TOL) &
                (out["num_iterations"] == ref["num_iterations"])).cpu().numpy().ravel()
        print("%s-%s Solve: %d of %d problems converge alike on the fused and the generic kernel" % (case.id, level, same.sum(), B))
        if is_f32(case):
            assert np.max(np.abs(got_v[same][:, :n] - ref_v[same][:, :n]), initial=0.0) <= 5e-3 * max(1.0, np.abs(ref_v[:, :n]).max())
        else:
            np.testing.assert_allclose(got_v[same][:, :n], ref_v[same][:, :n], rtol=1e-6, atol=1e-8)
    return check


@pytest.mark.parametrize("strategy", [Q.COMPLEMENTARITY, Q.PREDICTOR_CORRECTOR], ids=["complementarity", "predictor-corrector"])
@pytest.mark.parametrize("cid,level", LC.ITEMS, ids=IDS(LC.ITEMS))
def test_iterate_in_every_layout(cid, level, strategy):
    case = LC.BY_ID[cid]
    call = lambda plan, env, data: iterate(plan, env, data, strategy)
    run_layouts(case, level, call, against_generic(case, level, call))


@pytest.mark.parametrize("strategy", [Q.COMPLEMENTARITY, Q.PREDICTOR_CORRECTOR], ids=["complementarity", "predictor-corrector"])
@pytest.mark.parametrize("cid,level", LC.ITEMS, ids=IDS(LC.ITEMS))
def test_qp_solve_in_every_layout(cid, level, strategy):
    """COMPLEMENTARITY reaches the two lean Solve kernels (pck = 0: cases ny2 and mc2), PREDICTOR_CORRECTOR the ones that carry the second
    solve.  Moved stream: termination and iteration counts equal to packed, the rest at rtol = 1e-12, as
    test_fused_kernels_take_every_layout_of_J."""
    case = LC.BY_ID[cid]
    call = lambda plan, env, data: qp_solve(plan, env, data, strategy)
    run_layouts(case, level, call, against_generic(case, level, call), shared=True, query="mo_plan_solve_kernel")


# ---- 4. mo_linearize ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,level", J_ITEMS, ids=IDS(J_ITEMS))
def test_linearize_in_every_layout(cid, level):
    """Packed: lower G = J^T J + lambda_p I and c = J^T r within 1e-12 m_r of the float64 numpy products, strict upper exactly 0, 0.5 |r|^2 at
    rtol = 1e-13 (test_gpu_parity.py::test_fused_linearize_takes_every_layout_of_J); fp32: 2e-6 |G|_max, 2e-6 m_r, rtol 2e-6
    (::test_fused_f32_linearize).  fp32 keeps r 16-byte aligned with a stride divisible by 4 in the scattered layout (fused_f32_supported asks
    it); the misaligned r is the second moved-stream case below."""
    case = LC.BY_ID[cid]
    n, _, _, m_r = case.shape

    def check(out, data):
        Gn = out["G_out"].double().cpu().numpy().reshape(B, n, n).transpose(0, 2, 1)          # [b, row, col]
        ref = data["G"]
        f32 = is_f32(case)
        assert np.all(np.triu(Gn, 1) == 0.0)
        np.testing.assert_allclose(np.tril(Gn), np.tril(ref), rtol=0, atol=2e-6 * np.abs(ref).max() if f32 else 1e-12 * m_r)
        np.testing.assert_allclose(out["c_out"].double().cpu().numpy(), data["c"], rtol=0, atol=(2e-6 if f32 else 1e-12) * m_r)
        np.testing.assert_allclose(out["half_sq_out"].double().cpu().numpy().ravel(), 0.5 * np.einsum("bq,bq->b", data["r"], data["r"]), rtol=2e-6 if f32 else 1e-13)
    run_layouts(case, level, lambda plan, env, data: linearize(plan, env), check, plan_kw=dict(k=0, m=0), moved_rtol=False, env_kw=dict(r_aligned=is_f32(case)))
    if is_f32(case):                                            # r 4 bytes off a 16-byte boundary: the generic kernel
        data = LC.case_data(cid)
        with Plan(case, level, k=0, m=0) as plan:
            check(linearize(plan, LC.Env(case, level, "scattered", data, DEV)), data)


# ---- 5. outputs that may be NULL ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,level", NULL_FAMILIES, ids=IDS(NULL_FAMILIES))
def test_optional_outputs_as_null(cid, level):
    """alpha and status of mo_newton_step, kkt_out of mo_kkt_residual, delta and ip_out of mo_iterate, iterations and lagrange of mo_qp_solve,
    half_sq_out of mo_linearize: passed as NULL in the scattered layout, the remaining outputs keep the bits of the full call."""
    case = LC.BY_ID[cid]
    data = LC.case_data(cid)
    PC = Q.PREDICTOR_CORRECTOR
    calls = [(lambda plan, env, null=(): newton_step(plan, env, null=null), ("alpha", "status"), {}),
             (lambda plan, env, null=(): kkt_residual(plan, env, null=null), ("kkt_out",), {}),
             (lambda plan, env, null=(): iterate(plan, env, data, PC, null=null), ("delta", "ip_out"), {}),
             (lambda plan, env, null=(): qp_solve(plan, env, data, PC, null=null), ("iterations", "lagrange"), {}),
             (lambda plan, env, null=(): linearize(plan, env, null=null), ("half_sq_out",), dict(k=0, m=0))]
    for call, null, plan_kw in calls:
        with Plan(case, level, **plan_kw) as plan:
            env = LC.Env(case, level, "scattered", data, DEV, r_aligned=is_f32(case) and bool(plan_kw))
            full = call(plan, env)
            lean = call(plan, env, null=null)
            assert set(full) - set(lean) == set(null)
            assert_same_bits(lean, {name: t for name, t in full.items() if name not in null}, (cid, "NULL", null))


# ---- 6. the small entry points around the QP --------------------------------------------------------------------------------------------------------------------
SMALL = ["n32", "gen-f32"]     # n = 20, k = 3, m = 10, m_r = 26 in fp64 and in fp32 (these calls have one kernel each: the plan's kernel family plays no part)


def small_env(case, variant, data):
    env = LC.Env(case, "J", variant, data, DEV)
    rng = np.random.default_rng(77)
    x = rng.uniform(-1, 1, (B, case.shape[0]))
    if is_f32(case):
        x = x.astype(np.float32).astype(np.float64)
    env._input("x", x)
    return env, x


@pytest.mark.parametrize("cid", SMALL)
def test_fill_qp_in_every_layout(cid):
    """mo_fill_qp with x_stride, cons_b_stride and G_ld of the scattered layout.  Packed against numpy at the bounds of
    test_gpu_nls.py::test_fill_qp_errors_and_derivative_vs_numpy (fp32: ::test_fp32_variants_of_the_support_entry_points)."""
    case, data = LC.BY_ID[cid], LC.case_data(cid)
    n, k, m, m_r = case.shape
    f32 = is_f32(case)
    got = {}
    with Plan(case, "J") as plan:
        for variant in ("packed", "scattered"):
            env, x = small_env(case, variant, data)
            lay = env.lay
            G, c, cb, err, status = env.out("G_out"), env.out("c_out"), env.out("cons_b_out"), env.out("errors", 2), env.out("status", 1, torch.int32)
            L.check(L.lib().mo_fill_qp(plan, C.byref(env.prob), B, env.inputs["x"].ptr, lay["x"].stride, G.ptr, lay["G_out"].stride, lay["G_out"].ld, c.ptr,
                                       lay["c_out"].stride, cb.ptr, lay["cons_b_out"].stride, err.ptr, status.ptr, Q._stream()))
            got[variant] = collect(env, "mo_fill_qp", G_out=G, c_out=c, cons_b_out=cb, errors=err, status=status)
    out = got["packed"]
    assert torch.all(out["status"] == 0)
    Gn = out["G_out"].double().cpu().numpy().reshape(B, n, n).transpose(0, 2, 1)
    tol = lambda t64, t32: t32 if f32 else t64
    np.testing.assert_allclose(np.tril(Gn), np.tril(data["G"]), rtol=tol(1e-12, 1e-5), atol=tol(1e-12, 1e-5))
    np.testing.assert_allclose(out["c_out"].double().cpu().numpy(), data["c"], rtol=tol(1e-12, 1e-4), atol=tol(1e-12, 1e-4))
    np.testing.assert_allclose(out["cons_b_out"].double().cpu().numpy(), data["ca"] * np.take_along_axis(x, data["cv"].astype(np.int64), 1) + data["cb"],
                               rtol=tol(1e-14, 1e-6), atol=tol(1e-14, 1e-6))
    np.testing.assert_allclose(out["errors"].double().cpu().numpy(), np.stack([0.5 * np.sum(data["r"] ** 2, 1), np.sum(np.abs(data["b"]), 1)], 1), rtol=tol(1e-13, 1e-5))
    assert_same_bits(got["scattered"], out, (cid, "mo_fill_qp"))


@pytest.mark.parametrize("level", ["J", "G"])
@pytest.mark.parametrize("cid", SMALL)
def test_qp_cost_derivative_in_every_layout(cid, level):
    """mo_qp_cost_derivative with dx_stride and the problem's scattered G_ld / A_ld / J.  Packed: {c^T dx, sum sign(b) (A dx)} at rtol = 1e-11,
    atol = 1e-12 and dx^T G dx at rtol = 1e-11 (test_gpu_nls.py::test_fill_qp_errors_and_derivative_vs_numpy; fp32: 1e-4,
    ::test_fp32_variants_of_the_support_entry_points)."""
    case, data = LC.BY_ID[cid], LC.case_data(cid)
    f32 = is_f32(case)
    got = {}
    with Plan(case, level, m=0) as plan:
        for variant in ("packed", "scattered"):
            env = LC.Env(case, level, variant, data, DEV)
            rng = np.random.default_rng(78)
            dx = rng.uniform(-1, 1, (B, case.shape[0]))
            dx = dx.astype(np.float32).astype(np.float64) if f32 else dx
            env._input("x", dx)
            deriv, quad = env.out("deriv", 2), env.out("quad", 1)
            L.check(L.lib().mo_qp_cost_derivative(plan, C.byref(env.prob), B, env.inputs["x"].ptr, env.lay["x"].stride, deriv.ptr, quad.ptr, Q._stream()))
            got[variant] = collect(env, "mo_qp_cost_derivative", deriv=deriv, quad=quad)
    A = data["A"].transpose(0, 2, 1)                            # [b, row, col]
    dref = np.stack([np.einsum("bi,bi->b", data["c"], dx), np.einsum("bk,bk->b", np.sign(data["b"]), np.einsum("bkn,bn->bk", A, dx))], 1)
    qref = np.einsum("bi,bij,bj->b", dx, data["G"], dx)
    np.testing.assert_allclose(got["packed"]["deriv"].double().cpu().numpy(), dref, rtol=1e-4 if f32 else 1e-11, atol=1e-4 if f32 else 1e-12)
    np.testing.assert_allclose(got["packed"]["quad"].double().cpu().numpy().ravel(), qref, rtol=1e-4 if f32 else 1e-11)
    assert_same_bits(got["scattered"], got["packed"], (cid, level, "mo_qp_cost_derivative"))


@pytest.mark.parametrize("cid", SMALL)
def test_nonlinear_errors_in_every_layout(cid):
    """mo_nonlinear_errors with r_stride and r_eq_stride: {0.5 |r|^2, |r_eq|_1} at rtol = 1e-13 (fp32: 1e-5), the bound mo_fill_qp's
    errors_out has in test_gpu_nls.py (the same two sums)."""
    case, data = LC.BY_ID[cid], LC.case_data(cid)
    got = {}
    with Plan(case, "J") as plan:
        for variant in ("packed", "scattered"):
            env = LC.Env(case, "J", variant, data, DEV)
            out = env.out("errors", 2)
            L.check(L.lib().mo_nonlinear_errors(plan, env.inputs["r"].ptr, env.lay["r"].stride, env.inputs["b"].ptr, env.lay["b"].stride, B, out.ptr, Q._stream()))
            got[variant] = collect(env, "mo_nonlinear_errors", errors=out)
    ref = np.stack([0.5 * np.sum(data["r"] ** 2, 1), np.sum(np.abs(data["b"]), 1)], 1)
    np.testing.assert_allclose(got["packed"]["errors"].double().cpu().numpy(), ref, rtol=1e-5 if is_f32(case) else 1e-13)
    assert_same_bits(got["scattered"], got["packed"], (cid, "mo_nonlinear_errors"))


@pytest.mark.parametrize("level", ["J", "G"])
@pytest.mark.parametrize("cid", SMALL)
def test_nullspace_solve_in_every_layout(cid, level):
    """mo_nullspace_solve with x_stride, G_ld and A_ld of the scattered layout.  Packed against the KKT system of the equality-constrained QP
    solved in numpy, rtol = 1e-9, atol = 1e-11, and A x + b = 0 to 1e-11 (test_gpu_nls.py::test_null_space_solver; fp32: rtol 2e-3, atol 2e-4,
    ::test_fp32_variants_of_the_support_entry_points)."""
    case, data = LC.BY_ID[cid], LC.case_data(cid)
    n, k, _, _ = case.shape
    f32 = is_f32(case)
    got = {}
    with Plan(case, level, m=0) as plan:
        for variant in ("packed", "scattered"):
            env = LC.Env(case, level, variant, data, DEV)
            x, term = env.out("x_out"), env.out("termination", 1, torch.int32)
            L.check(L.lib().mo_nullspace_solve(plan, C.byref(env.prob), B, x.ptr, env.lay["x_out"].stride, term.ptr, Q._stream()))
            got[variant] = collect(env, "mo_nullspace_solve", x_out=x, termination=term)
    xs = got["packed"]["x_out"].double().cpu().numpy()
    assert torch.all(got["packed"]["termination"] == 0)
    for p in range(B):
        A = data["A"][p].T
        K = np.block([[data["G"][p], A.T], [A, np.zeros((k, k))]])
        xr = np.linalg.solve(K, -np.concatenate([data["c"][p], data["b"][p]]))[:n]
        np.testing.assert_allclose(xs[p], xr, rtol=2e-3 if f32 else 1e-9, atol=2e-4 if f32 else 1e-11)
        if not f32:
            np.testing.assert_allclose(A @ xs[p] + data["b"][p], 0, atol=1e-11)
    assert_same_bits(got["scattered"], got["packed"], (cid, level, "mo_nullspace_solve"))


@pytest.mark.parametrize("n", [17, 150])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_eigenvalue_stats_in_every_layout(dtype, n):
    """mo_qp_eigenvalue_stats of (G, c) input with G_ld = n + 3 and a padded G_stride, the matrix in LDS (n = 17) and in the plan's global
    workspace (n = 150).  Packed against numpy.linalg.eigvalsh at 1e-10 relative to max(|spectrum|, 1)
    (test_gpu_eig.py::test_eigenvalue_stats_of_indefinite_hessians_any_size; fp32: rtol 2e-6, atol 1e-6, ::test_eigenvalue_stats_fp32_plan)."""
    case = LC.Case("eig%d" % n, dtype, "G", (n, 0, 0, 0), None, "eig", False, False, False, 0)
    rng = np.random.default_rng(n)
    S = rng.uniform(-1, 1, (B, n, n)); S = S + S.transpose(0, 2, 1) + np.diag(rng.uniform(-2, 2, n))
    if dtype == "f32":
        S = S.astype(np.float32).astype(np.float64)
    garbage = S.copy()                                           # [b, col, row]: the strict upper triangle (row < col) must not be read
    il = np.tril_indices(n, -1)
    garbage[:, il[0], il[1]] = 1e30
    data = dict(G=garbage, c=np.zeros((B, n)), mu=np.zeros(B), vars=np.zeros((B, n)))
    got = {}
    with Plan(case, "G") as plan:
        for variant in ("packed", "scattered"):
            env = LC.Env(case, "G", variant, data, DEV)
            out = env.out("eig", 3)
            L.check(L.lib().mo_qp_eigenvalue_stats(plan, C.byref(env.prob), B, out.ptr, Q._stream()))
            got[variant] = collect(env, "mo_qp_eigenvalue_stats", eig=out)
    w = np.linalg.eigvalsh(S)
    ref = np.stack([w.min(axis=1), w.max(axis=1), np.abs(w).min(axis=1)], axis=1)
    g = got["packed"]["eig"].double().cpu().numpy()
    if dtype == "f32":
        np.testing.assert_allclose(g, ref, rtol=2e-6, atol=1e-6)
    else:
        assert np.max(np.abs(g - ref) / np.maximum(np.abs(ref).max(axis=1, keepdims=True), 1.0)) < 1e-10
    assert_same_bits(got["scattered"], got["packed"], (n, dtype, "mo_qp_eigenvalue_stats"))
