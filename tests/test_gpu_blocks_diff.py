"""GPU tests of the differentiable solve for residual-block input (run with -m gpu on an MI355X): mo_qp_gradients_blocks and
mo_qp_gradients_eq_blocks against the numpy restatement (tests/blocks_diff_reference.py) at caller-supplied state, against the dense
J-level path of mo_qp_gradients, through the C ABI (strides, NULL members, determinism, no allocation), and solve_qp(layout=...) end to end.

Per-element bound of the kernels, derived and not fitted: |dev - ref| <= (2 R_b P_b + 8) u A, u the unit round-off of the dtype and A the
same formula evaluated on absolute values.  An entry is a sum of at most P_b + 1 rounded products (t or w), times one factor, plus one such
term and the partner corrections: fewer than P_b + 8 roundings relative to A, so the bound has a factor >= 2 in hand for every R_b."""
import ctypes as C

import numpy as np
import pytest
import torch

from mini_opt_amd import _lib as L
from mini_opt_amd import diff as D
from mini_opt_amd import qp as Q
from oracle import oracle as orc
from tests import blocks_diff_reference as BR
from tests import diff_reference as R
from tests.sens_fixtures import DEV, LAM, N7_COST, PARAMS, UNIT, T, autograd_layout, bound_factor, oracle_kkt_solves, random_layout, rel_inf_rows

pytestmark = pytest.mark.gpu


def draw(rng, blocks, B, n, V, dt, shared=False):
    """Packed J [B or 1, values], r [B or 1, rows], vars [B, V], u [B, V]: float64 arrays holding values of the dtype."""
    values, rows = sum(R_ * len(idx) for idx, R_ in blocks), sum(R_ for _, R_ in blocks)
    arrs = [rng.uniform(-1, 1, (1 if shared else B, values)), rng.uniform(-1, 1, (1 if shared else B, rows)), rng.normal(size=(B, V)),
            rng.normal(size=(B, V))]
    if dt == torch.float32:
        arrs = [a.astype(np.float32).astype(np.float64) for a in arrs]
    return arrs


def check_cost_problem(n, blocks, Jp, rp, v, u, got, dt, tag):
    """One problem's device outputs (dict of float64 numpy rows) against the restatement, element by element."""
    Js, rs = BR.unpack(Jp, blocks), BR.split_rows(rp, blocks)
    dJ, dr, dlam = BR.gradients_blocks(blocks, Js, rs, v[:n], u[:n])
    aJ, ar, alam = BR.gradients_blocks(blocks, Js, rs, v[:n], u[:n], absolute=True)
    fv, fr = bound_factor(blocks)
    un = UNIT[dt]
    if "J_blocks" in got:
        err, tol = np.abs(got["J_blocks"] - BR.pack(dJ)), fv * un * BR.pack(aJ)
        assert np.all(err <= tol), (tag, "dJ", float(np.max(err / np.maximum(tol, 1e-300))))
    if "r" in got:
        err, tol = np.abs(got["r"] - np.concatenate(dr)), fr * un * np.concatenate(ar)
        assert np.all(err <= tol), (tag, "dr", float(np.max(err / np.maximum(tol, 1e-300))))
    if "lam" in got:
        assert abs(got["lam"] - dlam) <= (n + 8) * un * alam, (tag, "dlam")


def run_cost_case(rng, n, blocks, B, dt, k=0, m=0, shared=False, check=None, tag=""):
    lay = Q.ResidualLayout(n, blocks, dtype=dt)
    V = n + 2 * m + k
    Jp, rp, v, u = draw(rng, blocks, B, n, V, dt, shared)
    out = D.qp_gradients_blocks(lay, T(Jp, dt), T(rp, dt), T(v, dt), T(u, dt), k=k, m=m)
    assert set(out) == {"J_blocks", "r", "lam"}
    assert out["J_blocks"].shape == (B, lay.values) and out["r"].shape == (B, lay.rows) and out["lam"].shape == (B,)
    host = {key: t.double().cpu().numpy() for key, t in out.items()}
    for p in (sorted({0, 1, B // 2, B - 2, B - 1} & set(range(B))) if check is None else check):
        check_cost_problem(n, blocks, Jp[0 if shared else p], rp[0 if shared else p], v[p], u[p], {key: a[p] for key, a in host.items()}, dt,
                           (tag, n, B, p))
    return lay, (Jp, rp, v, u), out


DTYPES = pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])


# ---- 3. the kernel against the restatement at caller-supplied state -----------------------------------------------------------------------
@DTYPES
def test_blocks_grad_single_value(dt):
    """(a) n = 3, one block ((1,), 1), batch 1."""
    run_cost_case(np.random.default_rng(301), 3, [((1,), 1)], 1, dt, tag="single")


@DTYPES
def test_blocks_grad_repeated_indices_n7(dt):
    """(b) the n = 7 layout of the CPU test ((3, 0, 5, 3) and (2, 2) repeat a variable), batch 5; the state carries k = 2, m = 3 blocks the
    cost kernel must ignore."""
    run_cost_case(np.random.default_rng(302), 7, N7_COST, 5, dt, k=2, m=3, tag="n7")


@DTYPES
@pytest.mark.parametrize("n", [8, 64, 128])
def test_blocks_grad_random_layouts(n, dt):
    """(c) random layouts with repeated variables, more packed values than one pass of the workgroup."""
    rng = np.random.default_rng(310 + n)
    blocks = random_layout(rng, n, count=max(6, min(60, n)), repeats=True)
    assert any(len(set(idx)) < len(idx) for idx, _ in blocks)
    run_cost_case(rng, n, blocks, 37, dt, tag="random")


@DTYPES
def test_blocks_grad_unstaged_instantiation(dt):
    """(d) one block whose packed values and residual exceed the 48 KiB stage budget of the block kernels: the instantiation that reads the
    values from global memory.  fp64: 80 x 77 at n = 80 ((6160 + 80) x 8 B = 49 920 B); fp32: 112 x 110 at n = 112 (49 728 B)."""
    R_, P = (80, 77) if dt == torch.float64 else (112, 110)
    n = R_
    assert (R_ * P + R_) * (8 if dt == torch.float64 else 4) > 48 * 1024
    rng = np.random.default_rng(320)
    run_cost_case(rng, n, [(tuple(int(i) for i in rng.permutation(n)[:P]), R_)], 3, dt, tag="unstaged")


@DTYPES
def test_blocks_grad_workgroups_loop_over_problems(dt):
    """(e) n = 8 with batch = 8 x CU count + 3: every workgroup takes a second problem and re-uses its stage."""
    rng = np.random.default_rng(330)
    B = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 3
    blocks = random_layout(rng, 8, count=6, repeats=True)
    run_cost_case(rng, 8, blocks, B, dt, check=[0, 1, B // 2, B - 4, B - 3, B - 2, B - 1], tag="loop")


# ---- 4. agreement with the dense J-level path ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [12, 64])
def test_blocks_grad_matches_dense_path(n):
    rng = np.random.default_rng(340 + n)
    blocks = random_layout(rng, n, count=3 * n // 2)          # distinct indices inside every block
    B = 9
    lay, (Jp, rp, v, u), out = run_cost_case(rng, n, blocks, B, torch.float64, tag="dense")
    Jd = np.zeros((B, lay.rows, n))
    row = 0
    for (idx, R_), J in zip(blocks, zip(*[BR.unpack(Jp[p], blocks) for p in range(B)])):
        Jd[:, row:row + R_, list(idx)] = np.stack(J)
        row += R_
    dense = D.qp_gradients(Q.BatchedQP(n=n, J=T(Jd), r=T(rp), lam=0.1), T(v), T(u), want=("J", "r", "lam"))
    dJd = dense["J"].cpu().numpy()
    fv, fr = bound_factor(blocks)
    un = UNIT[torch.float64]
    for p in range(B):
        Js, rs = BR.unpack(Jp[p], blocks), BR.split_rows(rp[p], blocks)
        aJ, ar, alam = BR.gradients_blocks(blocks, Js, rs, v[p, :n], u[p, :n], absolute=True)
        gathered, row = [], 0
        for idx, R_ in blocks:
            gathered.append(dJd[p, row:row + R_][:, list(idx)])
            row += R_
        assert np.all(np.abs(out["J_blocks"][p].cpu().numpy() - BR.pack(gathered)) <= fv * un * BR.pack(aJ)), (n, p)
        assert np.all(np.abs((out["r"][p] - dense["r"][p]).cpu().numpy()) <= fr * un * np.concatenate(ar)), (n, p)
        assert abs(float(out["lam"][p] - dense["lam"][p])) <= (n + 8) * un * alam, (n, p)


# ---- 5. strides, NULL members, determinism, no allocation ----------------------------------------------------------------------------------
def test_blocks_grad_strides_null_members_and_determinism():
    n, B, k, m = 7, 5, 2, 3
    V = n + 2 * m + k
    rng = np.random.default_rng(350)
    lay = Q.ResidualLayout(n, N7_COST)
    Jp, rp, v, u = draw(rng, N7_COST, B, n, V, torch.float64, shared=True)          # J_stride = r_stride = 0: one instance for the batch
    J_d, r_d, v_d, u_d = T(Jp), T(rp), T(v), T(u)
    plan = D._plan_of(n, k, m, 0, torch.float64, torch.device(DEV), B)
    SENT = -777.25
    pad = 5
    bufs = lambda: {"J": torch.full((B, lay.values + pad), SENT, dtype=torch.float64, device=DEV),
                    "r": torch.full((B, lay.rows + 3), SENT, dtype=torch.float64, device=DEV),
                    "lam": torch.full((B, 2), SENT, dtype=torch.float64, device=DEV)}

    def launch(buf, members):
        g = L.BlockGrads()
        if "J" in members:
            g.dJ_blocks, g.dJ_stride = buf["J"].data_ptr(), lay.values + pad
        if "r" in members:
            g.dr, g.dr_stride = buf["r"].data_ptr(), lay.rows + 3
        if "lam" in members:
            g.dlambda, g.dlambda_stride = buf["lam"].data_ptr(), 2
        L.check(L.lib().mo_qp_gradients_blocks(plan, lay.h, Q._ptr(J_d), 0, Q._ptr(r_d), 0, B, Q._ptr(v_d), V, Q._ptr(u_d), V, C.byref(g),
                                               Q._stream()))
        torch.cuda.synchronize()

    one = bufs()
    launch(one, ("lam",))                                    # NULL dJ_blocks and dr: neither computed nor written
    assert torch.all(one["J"] == SENT) and torch.all(one["r"] == SENT) and torch.all(one["lam"][:, 1] == SENT)
    a, b = bufs(), bufs()
    launch(a, ("J", "r", "lam"))
    launch(b, ("J", "r", "lam"))
    assert all(torch.equal(a[key], b[key]) for key in a)     # two launches, the same bits
    assert torch.equal(a["lam"][:, 0], one["lam"][:, 0])
    assert torch.all(a["J"][:, lay.values:] == SENT) and torch.all(a["r"][:, lay.rows:] == SENT) and torch.all(a["lam"][:, 1] == SENT)
    host = {"J_blocks": a["J"][:, :lay.values].cpu().numpy(), "r": a["r"][:, :lay.rows].cpu().numpy(), "lam": a["lam"][:, 0].cpu().numpy()}
    for p in range(B):                                       # shared blocks, per-problem outputs
        check_cost_problem(n, N7_COST, Jp[0], rp[0], v[p], u[p], {key: t[p] for key, t in host.items()}, torch.float64, ("strides", p))
    assert not np.array_equal(host["J_blocks"][0], host["J_blocks"][1])
    only_r = bufs()
    launch(only_r, ("r",))
    assert torch.all(only_r["J"] == SENT) and torch.all(only_r["lam"] == SENT) and torch.equal(only_r["r"], a["r"])
    # the documented refusals, with a real plan
    other = D._plan_of(n + 1, 0, 0, 0, torch.float64, torch.device(DEV), B)
    g = L.BlockGrads()
    assert L.lib().mo_qp_gradients_blocks(other, lay.h, Q._ptr(J_d), 0, Q._ptr(r_d), 0, B, Q._ptr(v_d), V, Q._ptr(u_d), V, C.byref(g), None) == -2
    assert L.lib().mo_qp_gradients_eq_blocks(plan, lay.h, B, Q._ptr(v_d), V, Q._ptr(u_d), V, None, 0, None, 0, None) == -2   # 16 rows, k = 2


def test_first_block_gradients_allocate_nothing():
    n, B = 64, 96
    rng = np.random.default_rng(360)
    blocks = [(tuple(int(i) for i in rng.permutation(n)[:4]), 2) for _ in range(96)]
    eq_blocks = [((0, 5, 9), 1), ((7, 3), 2)]
    k = 3
    V = n + k
    Jp, rp, v, u = draw(rng, blocks, B, n, V, torch.float64)
    J_d, r_d, v_d, u_d = T(Jp), T(rp), T(v), T(u)
    lays = [Q.ResidualLayout(n, blocks) for _ in range(2)]
    eqs = [Q.ResidualLayout(n, eq_blocks) for _ in range(2)]
    desc = L.PlanDesc(n, k, 0, 0, L.MO_F64, 0, L.EXTRA_PLAN_FLAGS, 0, B)
    plans = [C.c_void_p(), C.c_void_p()]
    for pl in plans:
        L.check(L.lib().mo_plan_create(C.byref(desc), C.byref(pl)))
    dJ = torch.empty(B, lays[0].values, dtype=torch.float64, device=DEV)
    dr = torch.empty(B, lays[0].rows, dtype=torch.float64, device=DEV)
    dl = torch.empty(B, dtype=torch.float64, device=DEV)
    dJe = torch.empty(B, eqs[0].values, dtype=torch.float64, device=DEV)
    dre = torch.empty(B, k, dtype=torch.float64, device=DEV)
    g = L.BlockGrads()
    g.dJ_blocks, g.dJ_stride, g.dr, g.dr_stride, g.dlambda, g.dlambda_stride = dJ.data_ptr(), lays[0].values, dr.data_ptr(), lays[0].rows, dl.data_ptr(), 1

    def both(i):
        L.check(L.lib().mo_qp_gradients_blocks(plans[i], lays[i].h, Q._ptr(J_d), lays[i].values, Q._ptr(r_d), lays[i].rows, B, Q._ptr(v_d), V,
                                               Q._ptr(u_d), V, C.byref(g), Q._stream()))
        L.check(L.lib().mo_qp_gradients_eq_blocks(plans[i], eqs[i].h, B, Q._ptr(v_d), V, Q._ptr(u_d), V, Q._ptr(dJe), eqs[i].values, Q._ptr(dre), k,
                                                  Q._stream()))
        torch.cuda.synchronize()

    try:
        both(0)                                             # module load and kernel code happen on the twin first
        free0 = torch.cuda.mem_get_info()[0]
        both(1)                                             # the FIRST launches on this plan and these layouts
        assert torch.cuda.mem_get_info()[0] >= free0 - (1 << 20), (free0, torch.cuda.mem_get_info()[0])
        assert torch.all(torch.isfinite(dJ)) and torch.all(torch.isfinite(dJe))
    finally:
        for pl in plans:
            L.lib().mo_plan_destroy(pl)


# ---- 6. equality blocks ----------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_eq_blocks_grad_against_restatement_and_dense_dA(dt):
    n, k, m, B = 9, 3, 2, 7
    eq_blocks = [((0, 4, 0), 1), ((2, 6, 8, 2), 2)]          # in both, the first local column loses its variable to the last
    V = n + 2 * m + k
    rng = np.random.default_rng(370)
    lay = Q.ResidualLayout(n, eq_blocks, dtype=dt)
    assert lay.rows == k
    _, _, v, u = draw(rng, eq_blocks, B, n, V, dt)
    out = D.qp_gradients_eq_blocks(lay, T(v, dt), T(u, dt), m=m)
    assert set(out) == {"J_eq_blocks", "r_eq"} and out["J_eq_blocks"].shape == (B, lay.values)
    again = D.qp_gradients_eq_blocks(lay, T(v, dt), T(u, dt), m=m)
    assert all(torch.equal(out[key], again[key]) for key in out)
    only = D.qp_gradients_eq_blocks(lay, T(v, dt), T(u, dt), m=m, want=("r_eq",))
    assert set(only) == {"r_eq"} and torch.equal(only["r_eq"], out["r_eq"])
    got, got_r = out["J_eq_blocks"].double().cpu().numpy(), out["r_eq"].double().cpu().numpy()
    losers = np.array([True, False, False] + [True, True] + [False] * 6)     # ((0, 4, 0), 1): value 0; ((2, 6, 8, 2), 2): values 0, 1
    assert np.all(got[:, losers] == 0.0) and np.all(got[:, ~losers] != 0.0)
    # the dense dA_eq of mo_qp_gradients at the same state, gathered at the winning columns
    G = np.tile(np.eye(n), (B, 1, 1))
    prob = Q.BatchedQP(n=n, k=k, m=m, G=T(G, dt), c=T(np.zeros((B, n)), dt), A_eq=T(np.zeros((B, n, k)), dt), b_eq=T(np.zeros((B, k)), dt),
                       cons_var=T(np.zeros((1, m)), torch.int32), cons_a=T(np.ones((1, m)), dt), cons_b=T(np.ones((1, m)), dt))
    dA = D.qp_gradients(prob, T(v, dt), T(u, dt), want=("A_eq",))["A_eq"].double().cpu().numpy()        # [B, n, k]
    un = UNIT[dt]
    for p in range(B):
        x, y, ux, uy = v[p, :n], v[p, n + m:n + m + k], u[p, :n], u[p, n + m:n + m + k]
        dJ, dr_eq = BR.gradients_eq_blocks(eq_blocks, x, ux, y, uy)
        aJ, _ = BR.gradients_eq_blocks(eq_blocks, x, ux, y, uy, absolute=True)
        assert np.all(np.abs(got[p] - BR.pack(dJ)) <= 4 * un * BR.pack(aJ)), p
        assert np.array_equal(got_r[p], dr_eq)
        gathered, row = [], 0
        for idx, R_ in eq_blocks:
            blk = dA[p][list(idx), row:row + R_].T.copy()                        # R x P
            for a_, g_ in enumerate(idx):
                if g_ in idx[a_ + 1:]:
                    blk[:, a_] = 0.0
            gathered.append(blk)
            row += R_
        assert np.all(np.abs(got[p] - BR.pack(gathered)) <= 4 * un * BR.pack(aJ)), p


# ---- 7. autograd end to end ------------------------------------------------------------------------------------------------------------------
def oracle_u_pair(G, c, A, b_eq, var, a, b, g):
    """u at the ORACLE's Solve output, by LU on its full system and from the reduced system in numpy (the D of test_gpu_diff.py)."""
    n, k, m = len(c), len(b_eq), len(var)
    o = orc.Solver(orc.QP(G=np.tril(G), c=c, A_eq=A if k else None, b_eq=b_eq if k else None, cons_var=var, cons_a=a, cons_b=b))
    o.solve(**PARAMS)
    vo = np.array(o.variables)
    _, u_lu = oracle_kkt_solves(o, n, k, m, g, g)
    return u_lu, R.transposed_through_reduced(G, A, var, a, vo, g)


@pytest.mark.parametrize("case", ["unconstrained", "equalities", "bounds"])
@pytest.mark.parametrize("n", [8, 64])
def test_autograd_through_residual_blocks(n, case):
    """solve_qp(layout=...) against the restatement evaluated AT THE DEVICE'S OWN v: K from the restated linearisation, u by LU, the block
    formulas.  Bound max(1e-10, 10 D), D as in test_autograd_with_active_inequalities (measured on the CPU at the oracle's optimum of the same
    problems; printed).  lambda = 0.1 makes G positive definite by construction.  No problem is left out."""
    rng = np.random.default_rng(700 + n + len(case))
    B = 6
    blocks = autograd_layout(n, rng)
    lay = Q.ResidualLayout(n, blocks)
    eq_blocks = [(tuple(int(i) for i in rng.permutation(n)[:3]), 1), ((1, 6, 1), 2)] if case == "equalities" else []
    k = sum(R_ for _, R_ in eq_blocks)
    m = 4 if case == "bounds" else 0
    V = n + 2 * m + k
    Jp, rp = rng.uniform(-1, 1, (B, lay.values)), rng.uniform(-1, 1, (B, lay.rows))
    leaves = dict(J_blocks=T(Jp).requires_grad_(True), r=T(rp).requires_grad_(True),
                  lam=torch.full((B,), LAM, dtype=torch.float64, device=DEV, requires_grad=True))
    kw = {}
    Jeq = req = None
    var, a, b = np.zeros((B, 0), np.int32), np.zeros((B, 0)), np.zeros((B, 0))
    if k:
        eq_lay = Q.ResidualLayout(n, eq_blocks)
        Jeq, req = rng.uniform(-1, 1, (B, eq_lay.values)), rng.uniform(-0.5, 0.5, (B, k))
        leaves.update(J_eq_blocks=T(Jeq).requires_grad_(True), r_eq=T(req).requires_grad_(True))
        kw.update(eq_layout=eq_lay, J_eq_blocks=leaves["J_eq_blocks"], r_eq=leaves["r_eq"])
    if m:
        var = np.stack([rng.permutation(n)[:m] for _ in range(B)]).astype(np.int32)
        a, b = rng.choice([-1.0, 1.0], (B, m)), rng.uniform(5.0, 6.0, (B, m))       # loose: |x| stays far below 5
        leaves.update(cons_a=T(a).requires_grad_(True), cons_b=T(b).requires_grad_(True))
        kw.update(cons_var=T(var, torch.int32), cons_a=leaves["cons_a"], cons_b=leaves["cons_b"])
    x, s, y, z, status = D.solve_qp(layout=lay, J_blocks=leaves["J_blocks"], r=leaves["r"], lam=leaves["lam"], params=Q.Params(**PARAMS),
                                    return_all=True, return_status=True, **kw)
    assert torch.all(status == 0)
    gx = rng.normal(size=(B, n))
    loss = (x * T(gx)).sum() + (y * y).sum()
    loss.backward(retain_graph=True)
    assert torch.all(D.adjoint_status(x) == 0)
    first = {key: t.grad.clone() for key, t in leaves.items()}
    for t in leaves.values():
        t.grad = None
    loss.backward()
    assert all(torch.equal(first[key], t.grad) for key, t in leaves.items())          # a second backward repeats the first, bitwise
    v = torch.cat([x, s, y, z], dim=1).detach().cpu().numpy()
    g_full = np.concatenate([gx, np.zeros((B, m)), 2 * v[:, n + m:n + m + k], np.zeros((B, m))], axis=1)
    D_cpu, worst = 0.0, {}
    for p in range(B):
        Js, rs = BR.unpack(Jp[p], blocks), BR.split_rows(rp[p], blocks)
        G_low, c = BR.linearize(n, blocks, Js, rs, LAM)
        G = BR.symmetric(G_low)
        A = BR.jacobian(n, eq_blocks, BR.unpack(Jeq[p], eq_blocks)) if k else np.zeros((0, n))
        b_eq = req[p] if k else np.zeros(0)
        u_lu, u_red = oracle_u_pair(G, c, A, b_eq, var[p], a[p], b[p], g_full[p])
        D_cpu = max(D_cpu, float(rel_inf_rows(u_red[None], u_lu[None])[0]))
        u = R.solve_transposed(R.kkt_matrix(G, A, var[p], a[p], v[p]), g_full[p])
        xs, _, ys, zs = R.split(v[p], n, k, m)
        ux, _, uy, uz = R.split(u, n, k, m)
        dJ, dr, dlam = BR.gradients_blocks(blocks, Js, rs, xs, ux)
        ref = dict(J_blocks=BR.pack(dJ), r=np.concatenate(dr), lam=np.array([dlam]))
        if k:
            dJe, dre = BR.gradients_eq_blocks(eq_blocks, xs, ux, ys, uy)
            ref.update(J_eq_blocks=BR.pack(dJe), r_eq=dre)
            assert first["J_eq_blocks"][p, eq_lay.values - 6].item() == 0.0            # ((1, 6, 1), 2): its first column loses variable 1
        if m:
            ref.update(cons_a=zs * ux[var[p]] - uz * xs[var[p]], cons_b=-uz)
        for key, want in ref.items():
            err = float(np.max(np.abs(first[key][p].cpu().numpy().reshape(-1) - want)) / np.max(np.abs(want)))
            worst[key] = max(worst.get(key, 0.0), err)
    bound = max(1e-10, 10 * D_cpu)
    print(f"blocks autograd n = {n} {case}: D = {D_cpu:.3e}, bound {bound:.3e}, worst rel-inf per input {worst}")
    assert max(worst.values()) < bound, (worst, bound)
    if n == 64:   # the backward's plan runs the fused right-hand-side twin
        Gd, cd, _ = Q.linearize_blocks(lay, T(Jp), T(rp), lam=LAM)
        prob = Q.BatchedQP(n=n, k=k, m=m, G=Gd, c=cd, A_eq=None if not k else T(np.zeros((B, n, k))), b_eq=None if not k else T(req),
                           cons_var=kw.get("cons_var"), cons_a=None if not m else T(a), cons_b=None if not m else T(b))
        assert D.kkt_solve_kernel(prob, B).startswith("fused_rhs"), D.kkt_solve_kernel(prob, B)


def test_autograd_blocks_only_requested_inputs_and_exclusive_forms():
    n, B = 8, 4
    rng = np.random.default_rng(720)
    blocks = autograd_layout(n, rng)
    lay = Q.ResidualLayout(n, blocks)
    eq_blocks = [((0, 4, 7), 1)]
    eq_lay = Q.ResidualLayout(n, eq_blocks)
    Jb, r = T(rng.uniform(-1, 1, (B, lay.values))), T(rng.uniform(-1, 1, (B, lay.rows))).requires_grad_(True)
    Je, re_ = T(rng.uniform(-1, 1, (B, eq_lay.values))).requires_grad_(True), T(rng.uniform(-0.5, 0.5, (B, 1)))
    x = D.solve_qp(layout=lay, J_blocks=Jb, r=r, lam=LAM, eq_layout=eq_lay, J_eq_blocks=Je, r_eq=re_, params=Q.Params(**PARAMS))
    x.sum().backward()
    assert Jb.grad is None and re_.grad is None and r.grad is not None and Je.grad is not None
    assert torch.all(torch.isfinite(r.grad)) and torch.any(r.grad != 0) and torch.any(Je.grad != 0)
    G = T(np.tile(np.eye(n), (B, 1, 1)))
    with pytest.raises(ValueError):
        D.solve_qp(G=G, c=T(np.zeros((B, n))), layout=lay, J_blocks=Jb, r=r)
    with pytest.raises(ValueError):
        D.solve_qp(J=T(np.zeros((B, lay.rows, n))), layout=lay, J_blocks=Jb, r=r)
    with pytest.raises(ValueError):
        D.solve_qp(layout=lay, J_blocks=Jb, r=r, A_eq=T(np.zeros((B, 1, n))), b_eq=re_)
