"""The SQP outer loop beyond 32 variables, where mo_nls_solve runs its state machine on one wavefront per problem instead of one thread, and
the support kernels (mo_fill_qp / mo_nonlinear_errors / mo_qp_cost_derivative) at a shape where every 64-lane loop takes a second trip.
The problems are tests/nls_wide_problems.py; tests/test_nls_wide_oracle_cpu.py shows with the oracle alone that they reach the branches
named here and that the strict ones leave the device no excuse to differ."""
import numpy as np
import pytest
import torch

from mini_opt_amd import nls as NLS
from mini_opt_amd import qp as Q
from oracle import nls_oracle as N
from tests import nls_problems as P
from tests import nls_wide_problems as W
from tests.test_gpu_nls import T, check_records, knife_edge_rule, params_pair, run_both

pytestmark = pytest.mark.gpu


# ---- a. support kernels where every loop wraps ---------------------------------------------------------------------------------------
def sum_bound(L, S, dtype):
    """Bound on |computed - exact| for an output that accumulates L terms whose absolute values sum to S.

    Summing L floating-point terms in ANY order, with or without fma, errs by at most gamma_L * sum |terms| with gamma_L = L eps / (1 - L eps)
    (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  The outputs here are two-level sums (a dot product per row, then a
    sum over rows, the inner one squared for dx^T G dx): the errors of the levels add, and squaring doubles the inner one to first order.
    4 L eps S covers both levels and the second-order terms, with L the count of ALL products that enter the output and S the same expression
    with every product replaced by its absolute value.  A dropped or doubled element moves the output by about 0.1 S / L."""
    return 4.0 * L * float(np.finfo(dtype).eps) * S


def _support_inputs(np_dtype):
    rng = np.random.default_rng(71)
    B, n, k, m, m_r = 9, 70, 66, 70, 130
    f = lambda a_: a_.astype(np_dtype).astype(np.float64)             # the values the device sees
    d = dict(B=B, n=n, k=k, m=m, m_r=m_r)
    d["J"] = f(rng.uniform(-1, 1, (B, m_r, n))); d["r"] = f(rng.uniform(-1, 1, (B, m_r)))
    d["A"] = f(rng.uniform(-1, 1, (B, k, n))); b = f(rng.uniform(-1, 1, (B, k)))
    b[:, 65] = 0.0; b[2, 3] = 0.0                                       # sign(0) = 0 (nonlinear.cc:440-450), in either trip of the lane loop
    d["b"] = b
    d["cv"] = rng.integers(0, n, (B, m)).astype(np.int32); d["ca"] = rng.choice([-1.0, 1.0, 2.0], (B, m)); d["cb"] = f(rng.uniform(-1, 1, (B, m)))
    d["x"] = f(rng.uniform(-2, 2, (B, n))); d["dx"] = f(rng.uniform(-1, 1, (B, n)))
    lam = f(rng.uniform(0, 0.5, B)); lam[::3] = 0.0
    d["lam"] = lam
    return d


def _close(got, ref, bound, what):
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    assert np.all(err <= bound), (what, float(np.max(err / np.maximum(bound, 1e-300))))


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
def test_support_kernels_where_every_lane_loop_wraps(dt):
    """(n, k, m, m_r) = (70, 66, 70, 130): i += 64 takes a second trip over the constraints, the residual rows, the equality rows and the
    variables, the column-major walk of J reaches its second and third 64-row chunk; inputs differ from problem to problem.  Reference: the
    same sums in numpy long double on the values the device sees; tolerance: sum_bound, derived from the length of each sum."""
    np_dt = np.float64 if dt == torch.float64 else np.float32
    d = _support_inputs(np_dt)
    B, n, k, m, m_r = d["B"], d["n"], d["k"], d["m"], d["m_r"]
    ld = np.longdouble
    J, r, A, b, x, dx, lam = (d[key].astype(ld) for key in ("J", "r", "A", "b", "x", "dx", "lam"))
    common = dict(n=n, k=k, A_eq=T(d["A"].transpose(0, 2, 1), dt), b_eq=T(d["b"], dt))
    cons = dict(m=m, cons_var=T(d["cv"], torch.int32), cons_a=T(d["ca"], dt), cons_b=T(d["cb"], dt))
    prob = Q.BatchedQP(J=T(d["J"], dt), r=T(d["r"], dt), lam_vec=T(d["lam"], dt), **common, **cons)

    # LinearizeAndFillQP's tail: shifted constraints, both error sums, status
    _, _, cbs, err, status = NLS.fill_qp(prob, T(d["x"], dt))
    assert torch.all(status == 0)
    xv = np.take_along_axis(d["x"], d["cv"], 1)
    _close(cbs.cpu().numpy(), d["ca"] * xv + d["cb"], sum_bound(2, np.abs(d["ca"] * xv) + np.abs(d["cb"]), np_dt), "shifted constraints")
    f_ref, eq_ref = 0.5 * (r * r).sum(1), np.abs(b).sum(1)
    _close(err.cpu().numpy()[:, 0], f_ref, sum_bound(m_r, f_ref, np_dt), "0.5 |r|^2 of fill_qp")
    _close(err.cpu().numpy()[:, 1], eq_ref, sum_bound(k, eq_ref, np_dt), "|b_eq|_1 of fill_qp")
    # a bad constraint index in the second trip of one problem's lane loop
    cv2 = d["cv"].copy(); cv2[4, 65] = n
    prob.cons_var = T(cv2, torch.int32)
    _, _, cbs2, _, st2 = NLS.fill_qp(prob, T(d["x"], dt))
    st2, cbs2 = st2.cpu().numpy(), cbs2.cpu().numpy().astype(np.float64)
    assert st2[4] == 4 and np.all(np.delete(st2, 4) == 0)
    assert np.isnan(cbs2[4, 65]) and np.isnan(cbs2).sum() == 1
    keep = np.ones((B, m), bool); keep[4, 65] = False
    assert np.array_equal(cbs2[keep], cbs.cpu().numpy().astype(np.float64)[keep])

    # EvaluateNonlinearErrors
    e = NLS.nonlinear_errors(NLS._Plan(n, k, 0, m_r, dt, torch.device("cuda:0"), B), T(d["r"], dt), T(d["b"], dt)).cpu().numpy()
    _close(e[:, 0], f_ref, sum_bound(m_r, f_ref, np_dt), "0.5 |r|^2")
    _close(e[:, 1], eq_ref, sum_bound(k, eq_ref, np_dt), "|r_eq|_1")

    # ComputeQPCostDerivative (+ dx^T G dx)
    Jdx_abs = (np.abs(J) * np.abs(dx)[:, None, :]).sum(2)                                        # sum_i |J_qi dx_i|
    Jdx = (J * dx[:, None, :]).sum(2)
    df_ref, df_S = (r * Jdx).sum(1), (np.abs(r) * Jdx_abs).sum(1)
    Adx, Adx_abs = (A * dx[:, None, :]).sum(2), (np.abs(A) * np.abs(dx)[:, None, :]).sum(2)
    deq_ref, deq_S = (np.sign(b) * Adx).sum(1), (np.abs(np.sign(b)) * Adx_abs).sum(1)
    quad_ref = (Jdx * Jdx).sum(1) + lam * (dx * dx).sum(1)
    quad_S = (Jdx_abs * Jdx_abs).sum(1) + lam * (dx * dx).sum(1)
    J_col = np.ascontiguousarray(d["J"].transpose(0, 2, 1))                                      # [B, n, m_r]: tensor row i is column i of J
    for label, pj in (("row-major J", Q.BatchedQP(J=T(d["J"], dt), r=T(d["r"], dt), lam_vec=T(d["lam"], dt), **common)),
                      ("column-major J", Q.BatchedQP(J=T(J_col, dt), J_layout="col", r=T(d["r"], dt), lam_vec=T(d["lam"], dt), **common))):
        d1, q1 = NLS.qp_cost_derivative(pj, T(d["dx"], dt))
        d1, q1 = d1.cpu().numpy(), q1.cpu().numpy()
        _close(d1[:, 0], df_ref, sum_bound(m_r * n, df_S, np_dt), f"d_f, {label}")
        _close(d1[:, 1], deq_ref, sum_bound(k * n, deq_S, np_dt), f"d_equality, {label}")
        _close(q1, quad_ref, sum_bound(m_r * n + n, quad_S, np_dt), f"dx^T G dx, {label}")
    # (G, c) level: the lower triangle of G is read, its strict upper triangle holds garbage.  G and c are inputs here, rounded to the plan's type
    f = lambda a_: a_.astype(np_dt).astype(np.float64)
    G = f(np.einsum("bqi,bqj->bij", d["J"], d["J"]) + d["lam"][:, None, None] * np.eye(n)); G = np.tril(G) + np.tril(G, -1).transpose(0, 2, 1)
    c = f(np.einsum("bqi,bq->bi", d["J"], d["r"]))
    garbage = np.tril(np.full((n, n), 1.0e30), -1)                     # tensor [col][i] = G(i, col): i < col is G's strict upper triangle
    G_mem = np.triu(G.transpose(0, 2, 1)) + garbage
    d2, q2 = NLS.qp_cost_derivative(Q.BatchedQP(G=T(G_mem, dt), c=T(c, dt), **common), T(d["dx"], dt))
    d2, q2 = d2.cpu().numpy(), q2.cpu().numpy()
    Gl, cl = G.astype(ld), c.astype(ld)
    _close(d2[:, 0], (cl * dx).sum(1), sum_bound(n, (np.abs(cl) * np.abs(dx)).sum(1), np_dt), "c^T dx")
    _close(d2[:, 1], deq_ref, sum_bound(k * n, deq_S, np_dt), "d_equality, (G, c) level")
    outer = dx[:, :, None] * dx[:, None, :]
    _close(q2, (Gl * outer).sum((1, 2)), sum_bound(n * n, (np.abs(Gl) * np.abs(outer)).sum((1, 2)), np_dt), "dx^T sym(G) dx")


# ---- b. strict cases: the device reproduces the oracle's run of every start --------------------------------------------------------------
def _device_branches(case, out):
    rec = out.iterations.cpu().numpy(); term = out.termination_state.cpu().numpy(); nit = out.num_iterations.cpu().numpy()
    got = set()
    for p in range(len(term)):
        got |= W.branches_of_device_run(case, term[p], nit[p], rec[p])
    return got


def _assert_strict(case, out, x, term, nit, rx, rterm, rnit, logs):
    print(case.name, "device", list(zip(term.tolist(), nit.tolist())), "oracle", list(zip(rterm.tolist(), rnit.tolist())),
          "max |x - x_oracle|", float(np.nanmax(np.abs(x - rx))))
    assert np.array_equal(term, rterm) and np.array_equal(nit, rnit), (case.name, term, rterm, nit, rnit)
    assert torch.all(out.status == 0)
    for p in range(len(x)):
        check_records(out, logs, p)
    np.testing.assert_allclose(x, rx, rtol=0, atol=1e-6)
    missing = [c for c in case.claims if c not in _device_branches(case, out)]          # on the device's own records
    assert not missing, (case.name, missing)


@pytest.mark.parametrize("n", W.SIZES)
@pytest.mark.parametrize("kind", W.STRICT_KINDS)
def test_strict_case_matches_the_oracle_problem_by_problem(kind, n):
    """Termination, iteration count, status, every NLSIteration record and the final variables of every start; and the device's own records
    show the branch the case is there for.  n = 24 is the control on the thread path, 33 the first size on the wave path, at 72 the lane
    loops wrap (and the QP runs on the fused Solve kernel's 96-grid with the per-problem lambda vector and the skip of terminated problems)."""
    case = W.strict_case(kind, n)
    op, dp = params_pair(**case.params)
    guesses = case.guesses()
    out, x, term, nit, rx, rterm, rnit, logs = run_both(case.oracle_problem(), case.device_problem(), op, dp, guesses)
    _assert_strict(case, out, x, term, nit, rx, rterm, rnit, logs)
    if kind == "log":                                                  # no failed search may move the variables
        assert np.array_equal(x, guesses) and np.all(out.iterations.cpu().numpy()[:, :, 7] == NLS.STEP_FAILURE_NON_FINITE_COST)
        lam = out.iterations.cpu().numpy()[:, :, 1]
        assert np.all(lam == case.params.get("lambda_initial", 0.0))


# ---- c. equality-constrained families: not strict ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [W.FIRST_WAVE, W.WRAPPING])
@pytest.mark.parametrize("boxed", [False, True])
def test_sphere_with_product_pairs_on_the_wave_path(boxed, n):
    """Sphere cost and four product equalities through the null-space path (m = 0) and, with a box on eight variables, through the
    interior-point path: oracle/margins.py classes the QPs of this family as knife-edge, so the runs are held to knife_edge_rule with the cap
    the suite uses for the family at n = 32.  What depends on no decision -- lambda and both errors of iteration 0, sums of at most 72 terms of
    the same inputs -- is asserted for every problem at 1e-12, whatever the later decisions do."""
    case = W.sphere_case(n, boxed)
    k = case.equality_rows
    dprob = NLS.Problem(n, NLS.DeviceFamily(NLS.SPHERE, n), cost_rows=n, equality=NLS.DeviceFamily(NLS.PRODUCT_PAIRS, k, params=T(np.array(W.PRODUCTS))),
                        equality_rows=k, inequality_constraints=list(case.constraints))
    op, dp = params_pair(**case.params)
    guesses = case.guesses()
    out, x, term, nit, rx, rterm, rnit, logs = run_both(case.oracle_problem(), dprob, op, dp, guesses)
    assert out.null_space_path == (not boxed)
    rec = out.iterations.cpu().numpy()
    for p in range(len(guesses)):
        lg = logs[p][0]
        np.testing.assert_allclose(rec[p, 0, 1:4], [lg.lam, lg.errors_pre.f, lg.errors_pre.equality], rtol=1e-12, atol=0)
    same = knife_edge_rule(case.name, case.oracle_problem(), op, guesses, term, nit, rterm, rnit, max_fraction=0.05)
    print(case.name, "disagreements with the oracle:", int((~same).sum()), "of", len(same))
    np.testing.assert_allclose(x[same], rx[same], atol=1e-6)


@pytest.mark.parametrize("n", W.SIZES)
def test_rank_deficient_cost_ends_qp_indefinite_on_the_null_space_path(n):
    """Two cost rows and one product equality: without damping the reduced Hessian is singular and every problem ends QP_INDEFINITE with no
    iteration recorded (nonlinear.cc:103-105); with lambda_initial = 0.01 the same problems run to FIRST_ORDER like the oracle's."""
    case = W.deficient_case(n, False)
    op, dp = params_pair(**case.params)
    out, x, term, nit, rx, rterm, rnit, logs = run_both(case.oracle_problem(), case.device_problem(), op, dp, case.guesses())
    assert out.null_space_path
    assert np.all(term == NLS.QP_INDEFINITE) and np.all(nit == 0) and np.all(rterm == N.QP_INDEFINITE) and np.all(rnit == 0)
    assert np.array_equal(x, case.guesses())
    damped = W.deficient_case(n, True)
    op, dp = params_pair(**damped.params)
    out, x, term, nit, rx, rterm, rnit, logs = run_both(damped.oracle_problem(), damped.device_problem(), op, dp, damped.guesses())
    assert np.all(rterm == N.SATISFIED_FIRST_ORDER_TOL)
    same = knife_edge_rule(damped.name, damped.oracle_problem(), op, damped.guesses(), term, nit, rterm, rnit, max_fraction=0.05)
    np.testing.assert_allclose(x[same], rx[same], atol=1e-6)


# ---- d. retractions and callbacks on the wave path (n = 72) -----------------------------------------------------------------------------
def _solve(case, guesses, retraction=None, exit_callback=None, params=None):
    nls = NLS.ConstrainedNonlinearLeastSquares(case.device_problem(), batch=len(guesses), retraction=retraction)
    if exit_callback is not None:
        nls.SetUserExitCallback(exit_callback)
    out = nls.Solve(NLS.Params(**(params or case.params)), T(guesses))
    return (out, out.termination_state.cpu().numpy(), out.num_iterations.cpu().numpy(), nls.variables().cpu().numpy().copy(),
            out.iterations.cpu().numpy().copy())


def test_wrap_pi_retraction_on_the_wave_path():
    """retract_candidate<64> with WRAP_PI over both trips of its lane loop, against the oracle under the reference's ModPi retraction."""
    case = W.wrap_pi_case()
    guesses = case.guesses()
    out, term, nit, x, rec = _solve(case, guesses, retraction=NLS.WRAP_PI)
    rterm, rnit, rx, logs = [], [], [], []
    for g in guesses:
        o = N.ConstrainedNonlinearLeastSquares(case.oracle_problem(), retraction=P.mod_pi_retraction_np)
        t, lg = o.solve(N.Params(**case.params), g)
        rterm.append(t); rnit.append(len(lg)); rx.append(o.variables.copy()); logs.append(lg)
    assert np.array_equal(term, rterm) and np.array_equal(nit, rnit), (term, rterm, nit, rnit)
    for p in range(len(guesses)):
        check_records(out, logs, p)
    np.testing.assert_allclose(x, np.array(rx), rtol=0, atol=1e-6)
    assert np.all(np.abs(x) <= np.pi)
    # and the wrap did something: the Euclidean run from the same starts ends elsewhere
    _, _, _, x_plain, _ = _solve(case, guesses)
    assert np.abs(x_plain - x).max() > 1e-3


def test_callback_retraction_reproduces_the_builtin_on_the_wave_path():
    """MO_RETRACT_CALLBACK: begin_search copies dx into the caller's step buffer over both trips of the lane loop, lane 0 hands alpha over; a
    callback that computes x + alpha dx itself (one fused multiply-add per element, as the kernel does) gives the built-in run bit for bit."""
    case = W.strict_case("rosenbrock armijo", W.WRAPPING)
    guesses = case.guesses()
    _, term_a, nit_a, x_a, rec_a = _solve(case, guesses)
    _, term_b, nit_b, x_b, rec_b = _solve(case, guesses, retraction=lambda x, dx, alpha: torch.addcmul(x, dx, alpha[:, None]))
    assert np.array_equal(term_a, term_b) and np.array_equal(nit_a, nit_b)
    print("callback retraction: max |x - x_builtin|", float(np.abs(x_a - x_b).max()))
    assert np.array_equal(x_a, x_b)
    assert np.array_equal(rec_a, rec_b, equal_nan=True)


def test_user_exit_callback_on_the_wave_path():
    """Stopping the odd-numbered problems after the iteration with index 1 ends them with USER_CALLBACK after two iterations; the
    even-numbered ones are bit-identical to a run without the callback."""
    case = W.strict_case("rosenbrock poly", W.WRAPPING)
    guesses = case.guesses()
    B = len(guesses)
    odd = torch.arange(B, device="cuda:0") % 2 == 1
    _, term, nit, x, rec = _solve(case, guesses, exit_callback=lambda iteration, outputs: ~odd if iteration >= 1 else True)
    _, term0, nit0, x0, rec0 = _solve(case, guesses)
    assert np.all(nit0 > 2)
    assert np.all(term[1::2] == NLS.USER_CALLBACK) and np.all(nit[1::2] == 2)
    assert np.array_equal(term[0::2], term0[0::2]) and np.array_equal(nit[0::2], nit0[0::2])
    assert np.array_equal(x[0::2], x0[0::2]) and np.array_equal(rec[0::2], rec0[0::2], equal_nan=True)
    assert np.array_equal(rec[1::2, :2], rec0[1::2, :2], equal_nan=True) and np.all(np.isnan(rec[1::2, 2:]))


def test_nan_start_is_isolated_on_the_wave_path():
    """One NaN start in a batch of 13 ends that problem with QP_FAILURE and its QP status; the other twelve end exactly as without it."""
    case = W.strict_case("rosenbrock poly", W.WRAPPING)
    guesses = case.guesses()
    assert len(guesses) == 13
    bad = guesses.copy(); bad[6, 40] = np.nan
    out, term, nit, x, rec = _solve(case, bad)
    _, term0, nit0, x0, rec0 = _solve(case, guesses)
    good = [p for p in range(13) if p != 6]
    st = out.status.cpu().numpy()
    assert term[6] == NLS.QP_FAILURE and st[6] != 0 and np.all(st[good] == 0)
    assert np.array_equal(term[good], term0[good]) and np.array_equal(nit[good], nit0[good])
    assert np.array_equal(x[good], x0[good]) and np.array_equal(rec[good], rec0[good], equal_nan=True)


# ---- e. related checks at these sizes ------------------------------------------------------------------------------------------------
def test_device_rosenbrock_family_at_72_variables_is_exactly_the_torch_definition():
    """MO_RESIDUAL_ROSENBROCK with 142 rows against the torch definition, r and the dense J (zeros included).  The inputs are multiples of
    2^-10 in [-3, 3): x^2, x_{i+1} - x_i^2 and the factors 10 and -20 are then exact in fp64, so the two sides agree to the last bit whether
    or not either of them fuses a multiply with an add."""
    rng = np.random.default_rng(13)
    n, B = W.WRAPPING, 13
    x = T(rng.integers(-3072, 3072, (B, n)) / 1024.0)
    r, J = NLS.DeviceFamily(NLS.ROSENBROCK, 2 * (n - 1))(x, True)
    r0, J0 = W.rosenbrock_torch(n)(x, True)
    assert torch.equal(r, r0) and torch.equal(J, J0)
    rn, Jn = W.rosenbrock_np(n)(x[5].cpu().numpy(), True)            # and the torch definition is the oracle's
    assert np.array_equal(r0[5].cpu().numpy(), rn) and np.array_equal(J0[5].cpu().numpy(), Jn)


def test_qp_eigenvalues_of_every_iteration_at_40_variables():
    """Params::log_qp_eigenvalues where the 256-thread eigen kernel and its skip of terminated problems do real work: n = 40, lambda changing
    from iteration to iteration, problems ending with MAX_LAMBDA at different iterations.  Every active iteration's {min, max, abs_min} is
    within 1e-10 |G| of eigvalsh(J^T J + lambda I) built from the oracle's linearisation and lambda of that iteration; NaN follows."""
    case = W.rosenbrock_case(40, "ls0")
    guesses = case.guesses()
    nls = NLS.ConstrainedNonlinearLeastSquares(case.device_problem(), batch=len(guesses))
    out = nls.Solve(NLS.Params(log_qp_eigenvalues=True, **case.params), T(guesses))
    eig = out.qp_eigenvalues.cpu().numpy()
    term, nit = out.termination_state.cpu().numpy(), out.num_iterations.cpu().numpy()
    assert eig.shape == (case.params["max_iterations"], len(guesses), 3)
    assert len(set(nit.tolist())) > 1 and nit.max() < case.params["max_iterations"]
    for p, g in enumerate(guesses):
        Js = []

        def cost(x, want_J):
            r, J = case.cost_np(x, want_J)
            if want_J:
                Js.append(J)
            return r, J
        t, logs = N.ConstrainedNonlinearLeastSquares(N.Problem(case.n, cost)).solve(N.Params(**case.params), g)
        assert (t, len(logs)) == (term[p], nit[p])
        for i, lg in enumerate(logs):
            w = np.linalg.eigvalsh(Js[i].T @ Js[i] + lg.lam * np.eye(case.n))
            np.testing.assert_allclose(eig[i, p], [w.min(), w.max(), np.abs(w).min()], rtol=0, atol=1e-10 * np.abs(w).max(),
                                       err_msg=f"problem {p} iteration {i}")
        assert np.all(np.isnan(eig[nit[p]:, p]))


def test_residual_block_input_at_72_variables_matches_the_dense_run():
    """mo_nls_solve_blocks on the wave path: the 142 rows as Residuals on (i,) and (i, i + 1) give the termination states and iteration
    counts of the dense stack."""
    case = W.strict_case("rosenbrock poly", W.WRAPPING)
    params = dict(case.params, max_iterations=12)
    guesses = case.guesses()
    prob = NLS.Problem.FromResiduals(case.n, W.rosenbrock_residual_blocks(case.n))
    blk = NLS.ConstrainedNonlinearLeastSquares(prob, batch=len(guesses), residual_blocks=True)
    ob = blk.Solve(NLS.Params(**params), T(guesses))
    _, term, nit, x, _ = _solve(case, guesses, params=params)
    assert np.array_equal(ob.termination_state.cpu().numpy(), term) and np.array_equal(ob.num_iterations.cpu().numpy(), nit)
    np.testing.assert_allclose(blk.variables().cpu().numpy(), x, rtol=0, atol=1e-6)
