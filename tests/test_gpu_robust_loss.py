"""Robust loss functions for residual-block costs on the device: mo_residual_loss_eval against the long-double reference, the fused
mo_linearize_blocks_robust bit for bit against the two-launch route, mo_nls_solve_blocks_robust against the wrapped oracle on the strict
starts, and the Python surface (tests/robust_loss_reference.py has the reference, the problems and the starts)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from mini_opt_amd import _lib as L
from mini_opt_amd import nls as NLS
from mini_opt_amd import qp as Q
from oracle import nls_oracle as N
from tests import robust_loss_reference as R
from tests.test_gpu_nls import check_records

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float64, torch.float32]
NP = {torch.float64: np.float64, torch.float32: np.float32}


def T(a, dt=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=DEV).contiguous()


# ---- the layout of (a): n = 9, 40 blocks, R cycling through {1, 2, 3, 7} and the kind through all five (every pair occurs, twice); the
# scales have exact squares in both dtypes (the kernel's a^2 is then the reference's): 1.25 for the first 20 blocks (a^2 in [1, 2): an even
# ulp exponent in fp64), 1.5 for the rest (a^2 in [2, 4): an even ulp exponent in fp32).  Block 5 names a variable twice.
N_A = 9
ROWS_A = [(1, 2, 3, 7)[b % 4] for b in range(40)]
LOSSES_A = [(b % 5, 1.25 if b < 20 else 1.5) for b in range(40)]


def blocks_a():
    rng = np.random.default_rng(11)
    out = []
    for b, Rb in enumerate(ROWS_A):
        idx = [int(i) for i in rng.permutation(N_A)[:1 + b % 3]]
        if b == 5:
            idx = [idx[0], 4 if idx[0] != 4 else 3, idx[0]]
        out.append((tuple(idx), Rb))
    return out


BLOCKS_A = blocks_a()
OFF_A = R.block_offsets(ROWS_A)


def four_squares(M):
    """Integers k1 <= k2 <= k3 <= k4 with sum k^2 = M (Lagrange), by search from the top."""
    k1 = math.isqrt(M)
    while True:
        M1 = M - k1 * k1
        k2 = math.isqrt(M1)
        for _ in range(64):
            if k2 < 0:
                break
            M2 = M1 - k2 * k2
            for k3 in range(math.isqrt(M2), -1, -1):
                M3 = M2 - k3 * k3
                k4 = math.isqrt(M3)
                if k4 * k4 == M3:
                    return sorted([k1, k2, k3, k4])
                if 2 * k3 * k3 < M2:
                    break
            k2 -= 1
        k1 -= 1


def rows_at(target, bits):
    """Four values whose squares sum EXACTLY, in order, to the double / float `target`: integers times 2^-m with M = target 2^2m < 2^bits,
    so every square and every partial sum is an integer below 2^bits -- exact in the kernel's dtype."""
    e = math.floor(math.log2(target))
    two_m = bits - 1 - e
    assert two_m % 2 == 0, "the ulp exponent of the target must be even"
    M = int(target * 2.0 ** two_m)
    assert M * 2.0 ** -two_m == target
    return [k * 2.0 ** -(two_m // 2) for k in four_squares(M)]


@functools.lru_cache(maxsize=None)
def data_a(f32):
    """r [1007, rows] (float64 values representable in the dtype), with the special rows of the issue in the first problems."""
    npdt = np.float32 if f32 else np.float64
    rng = np.random.default_rng(21 + f32)
    B = 1007
    r = np.empty((B, OFF_A[-1]))
    for b, ((kind, a), Rb) in enumerate(zip(LOSSES_A, ROWS_A)):
        v = rng.normal(size=(B, Rb)) * a * rng.uniform(0.2, 2.0, (B, 1)) / math.sqrt(Rb)
        if kind == R.TUKEY:
            # rho' of TUKEY has the condition number 2 t / (1 - t), unbounded at the cutoff: a fixed-eps bound on its weight needs s itself
            # exact, so these blocks' rows lie on a grid of 1/16 (|r| <= 4: every square and partial sum is exact in fp32 already)
            v = np.clip(np.round(v * 16), -64, 64) / 16
        r[:, OFF_A[b]:OFF_A[b + 1]] = v
    r = r.astype(npdt).astype(np.float64)
    r[0] = 0.0                                                        # s = 0 everywhere
    a_joint = 1.5 if f32 else 1.25                                    # the scale whose a^2 has an even ulp exponent in this dtype
    bits = 24 if f32 else 53
    for b, ((kind, a), Rb) in enumerate(zip(LOSSES_A, ROWS_A)):
        if Rb == 7 and a == a_joint:                                  # s at the two neighbours of a^2, one block of every kind
            a2 = npdt(a * a)
            for p, side in ((1, npdt(0)), (2, npdt(np.inf))):
                r[p, OFF_A[b]:OFF_A[b + 1]] = [0.0, 0.0, 0.0] + rows_at(float(np.nextafter(a2, side)), bits)
        r[3, OFF_A[b]:OFF_A[b + 1]] = npdt(a * 1.0e6 / math.sqrt(Rb))  # s / a^2 = 1e12
        if kind == R.TUKEY:
            r[4, OFF_A[b]:OFF_A[b + 1]] = 2.0 * a / math.sqrt(Rb) * 1.01  # beyond the cutoff
    r[5, OFF_A[6] + 1] = np.nan                                       # a NaN in block 6 (R = 3) of problem 5
    return r.astype(npdt).astype(np.float64)


def run_eval(lay, loss, r_np, dt, r_pad=0, w_pad=0, want_w=True, want_f=True):
    """mo_residual_loss_eval through ctypes with padded strides; the guards beyond each row must come back untouched."""
    B, rows = r_np.shape
    r = torch.full((B, rows + r_pad), 7.0, dtype=dt, device=DEV)
    r[:, :rows] = T(r_np, dt)
    w = torch.full((B, rows + w_pad), -3.0, dtype=dt, device=DEV) if want_w else None
    f = torch.full((B + 2,), -5.0, dtype=dt, device=DEV) if want_f else None
    L.check(L.lib().mo_residual_loss_eval(lay._plan, lay.h, loss.h, Q._ptr(r), rows + r_pad, B, Q._ptr(w), rows + w_pad, Q._ptr(f), Q._stream()))
    torch.cuda.synchronize()
    if want_w:
        assert torch.all(w[:, rows:] == -3.0)
    if want_f:
        assert torch.all(f[B:] == -5.0)
    return (w[:, :rows].cpu().numpy() if want_w else None), (f[:B].cpu().numpy() if want_f else None)


@functools.lru_cache(maxsize=None)
def layout_a(dt):
    lay = Q.ResidualLayout(N_A, BLOCKS_A, dtype=dt, device=DEV)
    return lay, Q.ResidualLoss(lay, LOSSES_A)


# ------------------------------------------------------------------ a. mo_residual_loss_eval against the long-double reference
@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
def test_loss_eval_against_the_long_double_reference(dt):
    f32 = dt == torch.float32
    npdt = NP[dt]
    eps = float(np.finfo(npdt).eps)
    lay, loss = layout_a(dt)
    r = data_a(f32)
    w_ref, f_ref, absf_ref = R.loss_eval(ROWS_A, LOSSES_A, r)
    # the special rows are what they claim to be
    s = lambda p, b: np.sum(r[p, OFF_A[b]:OFF_A[b + 1]].astype(np.longdouble) ** 2)
    joints = [b for b in range(40) if ROWS_A[b] == 7 and LOSSES_A[b][1] == (1.5 if f32 else 1.25)]
    assert sorted(LOSSES_A[b][0] for b in joints) == list(R.KINDS)
    for b in joints:
        a2 = npdt(LOSSES_A[b][1] ** 2)
        assert s(1, b) == np.nextafter(a2, npdt(0)) and s(2, b) == np.nextafter(a2, npdt(np.inf))
    w, f = run_eval(lay, loss, r, dt, r_pad=3, w_pad=5)
    # a NaN touches its block's weights and its problem's rho, nothing else
    nanrows = np.zeros_like(r, bool)
    nanrows[5, OFF_A[6]:OFF_A[7]] = True
    assert np.all(np.isnan(w[nanrows])) and not np.any(np.isnan(w[~nanrows]))
    assert np.isnan(f[5]) and not np.any(np.isnan(np.delete(f, 5)))
    ok = ~nanrows
    # weights within 16 eps relative (exact zeros exactly)
    zero = (w_ref == 0) & ok
    assert np.all(w[zero] == 0)
    for b, (kind, a) in enumerate(LOSSES_A):
        if kind == R.TUKEY:
            assert np.all(w[3:5, OFF_A[b]:OFF_A[b + 1]] == 0)          # beyond the cutoff: exactly 0
        if kind == R.HUBER:
            assert np.all(w[0, OFF_A[b]:OFF_A[b + 1]] == 1)            # s = 0: no a / sqrt(0)
    assert np.all(f[0:1] == 0)
    nz = ok & ~zero
    wr = np.abs(w[nz].astype(np.longdouble) - w_ref[nz]) / np.abs(w_ref[nz]) / eps
    fin = ~np.isnan(f_ref)
    bound = (len(ROWS_A) + max(ROWS_A) + 16) * eps * absf_ref[fin]
    fr = np.abs(f[fin].astype(np.longdouble) - f_ref[fin]) / np.where(bound > 0, bound, 1)
    print(f"loss eval {dt}: worst weight error {float(wr.max()):.2f} eps (bound 16), worst rho error {float(fr.max()):.3f} of its bound")
    assert wr.max() <= 16
    assert fr.max() <= 1
    # two launches, the same bits; either output NULL; batch 1
    w2, f2 = run_eval(lay, loss, r, dt, r_pad=0, w_pad=0)
    assert np.array_equal(w, w2, equal_nan=True) and np.array_equal(f, f2, equal_nan=True)
    w3, none = run_eval(lay, loss, r, dt, want_f=False)
    none2, f3 = run_eval(lay, loss, r, dt, want_w=False)
    assert none is None and none2 is None
    assert np.array_equal(w, w3, equal_nan=True) and np.array_equal(f, f3, equal_nan=True)
    for p in (2, 7):
        w1, f1 = run_eval(lay, loss, r[p:p + 1], dt, r_pad=1, w_pad=2)
        assert np.array_equal(w1[0], w[p]) and f1[0] == f[p]
    wq, fq = Q.loss_weights(lay, loss, T(r, dt))
    assert np.array_equal(wq.cpu().numpy(), w, equal_nan=True) and np.array_equal(fq.cpu().numpy(), f, equal_nan=True)


# ------------------------------------------------------------------ b. the fused linearise, bit for bit
def two_launch(lay, loss, Jb, r, **kw):
    w, f = Q.loss_weights(lay, loss, r)
    G, c, _ = Q.linearize_blocks(lay, Jb, r, weights=w, **kw)
    return G, c, f, w


def same(a, b):
    return (a is None and b is None) or torch.equal(a, b)


@functools.lru_cache(maxsize=None)
def big_layout(dt):
    """One block with P = n, R = n + 3 at the first n whose (values + 2 rows) elements exceed 48 KiB: the layout that does not stage."""
    n = 110 if dt == torch.float32 else 77
    assert (n * (n + 3) + 2 * (n + 3)) * (4 if dt == torch.float32 else 8) > 48 * 1024
    lay = Q.ResidualLayout(n, [(tuple(range(n)), n + 3)], dtype=dt, device=DEV)
    return lay, Q.ResidualLoss(lay, [(R.CAUCHY, 2.0)])


@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("B", [1, 300])
def test_fused_robust_linearize_has_the_bits_of_the_two_launch_route(dt, B):
    f32 = dt == torch.float32
    lay, loss = layout_a(dt)
    rng = np.random.default_rng(31 + B + f32)
    r = T(data_a(f32)[6:6 + B] if B == 1 else data_a(f32)[:B], dt)
    r = torch.nan_to_num(r, nan=0.25)
    Jb = T(rng.uniform(-1, 1, (B, lay.values)), dt)
    lam_vec = T(rng.uniform(0.0, 0.5, B) * (rng.random(B) < 0.7), dt)
    variants = [dict(), dict(want_G=False), dict(lam=0.125), dict(lam_vec=lam_vec)]
    for kw in variants:
        G, c, f, w = Q.linearize_blocks(lay, Jb, r, loss=loss, return_weights=True, **kw)
        G2, c2, f2, w2 = two_launch(lay, loss, Jb, r, **kw)
        assert same(G, G2) and same(c, c2) and same(f, f2) and same(w, w2), kw
        G3, c3, f3 = Q.linearize_blocks(lay, Jb, r, loss=loss, **kw)              # weights_out NULL
        assert same(G, G3) and same(c, c3) and same(f, f3), kw
    # J_stride = 0: one instance of the blocks for the batch
    G, c, f, w = Q.linearize_blocks(lay, Jb[:1], r, loss=loss, return_weights=True)
    G2, c2, f2, w2 = two_launch(lay, loss, Jb[:1], r)
    assert same(G, G2) and same(c, c2) and same(f, f2) and same(w, w2)
    # block 5 names a variable twice: its pair lands once, on the diagonal -- and the weighted sibling is the yardstick there too
    assert len(set(BLOCKS_A[5][0])) < len(BLOCKS_A[5][0])


@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
def test_robust_linearize_of_a_layout_that_does_not_stage(dt):
    lay, loss = big_layout(dt)
    rng = np.random.default_rng(41)
    B = 3
    Jb = T(rng.uniform(-1, 1, (B, lay.values)), dt)
    r = T(rng.uniform(-1, 1, (B, lay.rows)), dt)
    G, c, f, w = Q.linearize_blocks(lay, Jb, r, loss=loss, return_weights=True)
    G2, c2, f2, w2 = two_launch(lay, loss, Jb, r)
    assert same(G, G2) and same(c, c2) and same(f, f2) and same(w, w2)
    w_ref, f_ref, _ = R.loss_eval([lay.rows], [(R.CAUCHY, 2.0)], r.cpu().numpy())
    # (s sums R rounded squares in order and CAUCHY's rho' has a condition number <= 1 in s: R eps for s, 16 for the rest)
    np.testing.assert_allclose(w.cpu().numpy(), w_ref.astype(float), rtol=(lay.rows + 16) * float(np.finfo(NP[dt]).eps))
    # without weights_out: refused before any launch, nothing written
    n = lay.n
    Gg = torch.full((B, n, n), -2.0, dtype=dt, device=DEV)
    cg = torch.full((B, n), -2.0, dtype=dt, device=DEV)
    fg = torch.full((B,), -2.0, dtype=dt, device=DEV)
    rc = L.lib().mo_linearize_blocks_robust(lay._plan, lay.h, Q._ptr(Jb), lay.values, Q._ptr(r), lay.rows, 0.0, None, 0, B, Q._ptr(Gg), n * n, n,
                                            Q._ptr(cg), n, Q._ptr(fg), loss.h, None, 0, Q._stream())
    torch.cuda.synchronize()
    assert rc == -3 and b"weights_out" in L.lib().mo_last_error()      # MO_ERR_UNSUPPORTED
    assert torch.all(Gg == -2.0) and torch.all(cg == -2.0) and torch.all(fg == -2.0)


@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
def test_all_trivial_table_gives_the_bits_of_linearize_blocks(dt):
    lay, _ = layout_a(dt)
    trivial = Q.ResidualLoss(lay, [(R.TRIVIAL, 0.0)] * 40)             # a TRIVIAL block's scale is ignored
    rng = np.random.default_rng(51)
    Jb, r = T(rng.uniform(-1, 1, (17, lay.values)), dt), T(rng.uniform(-1, 1, (17, lay.rows)), dt)
    G, c, f, w = Q.linearize_blocks(lay, Jb, r, lam=0.25, loss=trivial, return_weights=True)
    G2, c2, f2 = Q.linearize_blocks(lay, Jb, r, lam=0.25)
    assert same(G, G2) and same(c, c2) and same(f, f2) and torch.all(w == 1)


def test_tukey_rejected_block_with_nan_jacobian_contributes_nothing():
    dt = torch.float64
    lay, loss = layout_a(dt)
    b = 4                                                              # kind 4 = TUKEY, R = 1
    assert LOSSES_A[b][0] == R.TUKEY
    rng = np.random.default_rng(61)
    B = 5
    shapes = lay.shapes
    Js = [rng.uniform(-1, 1, (B, Rb, Pb)) for Rb, Pb in shapes]
    r = np.nan_to_num(data_a(False)[10:10 + B].copy(), nan=0.5)
    r[:, OFF_A[b]:OFF_A[b + 1]] = 3.0 * LOSSES_A[b][1]
    Jn = [J.copy() for J in Js]
    Jn[b][:] = np.nan
    G, c, f, w = Q.linearize_blocks(lay, Q.pack_blocks([T(J) for J in Jn]), T(r), loss=loss, return_weights=True)
    assert torch.all(w[:, OFF_A[b]:OFF_A[b + 1]] == 0)
    assert bool(torch.isfinite(G).all()) and bool(torch.isfinite(c).all())
    keep = [i for i in range(40) if i != b]
    lay2 = Q.ResidualLayout(N_A, [BLOCKS_A[i] for i in keep], dtype=dt, device=DEV)
    loss2 = Q.ResidualLoss(lay2, [LOSSES_A[i] for i in keep])
    r2 = np.concatenate([r[:, OFF_A[i]:OFF_A[i + 1]] for i in keep], axis=1)
    G2, c2, f2 = Q.linearize_blocks(lay2, Q.pack_blocks([T(Js[i]) for i in keep]), T(r2), loss=loss2)
    assert torch.all(G == G2) and torch.all(c == c2)
    np.testing.assert_allclose((f - f2).cpu().numpy(), LOSSES_A[b][1] ** 2 / 6, rtol=1e-12)   # the rejected block's 0.5 rho = a^2 / 6


# ------------------------------------------------------------------ c. the loop against the wrapped oracle, on the strict starts
@pytest.mark.parametrize("case", R.strict_cases(), ids=lambda c: c.name)
def test_robust_nls_loop_matches_the_wrapped_oracle_on_every_strict_start(case):
    B = len(case.starts)
    nls = NLS.ConstrainedNonlinearLeastSquares(case.device_problem(NLS, DEV), batch=B, residual_blocks=True)
    out = nls.Solve(NLS.Params(**case.params), T(case.starts))
    x = nls.variables().cpu().numpy()
    term, nit = out.termination_state.cpu().numpy(), out.num_iterations.cpu().numpy()
    assert out.null_space_path == (case.name == "sphere_soft_l1")
    ref_logs = []
    for p in range(B):
        o = N.ConstrainedNonlinearLeastSquares(case.oracle_problem(p))
        rterm, logs = o.solve(N.Params(**case.params), case.starts[p])
        ref_logs.append(logs)
        assert (int(term[p]), int(nit[p])) == (rterm, len(logs)), (case.name, p, (term[p], nit[p]), (rterm, len(logs)))
        np.testing.assert_allclose(x[p], o.variables, rtol=0, atol=1e-6, err_msg=f"{case.name} start {p}")
    for p in range(B):
        check_records(out, ref_logs, p)
    # EvaluateNonlinearErrors reports the robust f; LossWeights are qp.loss_weights at the solution
    err = nls.EvaluateNonlinearErrors(nls.variables()).cpu().numpy()
    r_sol, _ = case.device_problem(NLS, DEV).cost(nls.variables(), False)
    _, f_ref, _ = R.loss_eval(case.rows, case.losses, r_sol.cpu().numpy())
    np.testing.assert_allclose(err[:, 0], f_ref.astype(float), rtol=1e-12, atol=1e-300)
    lay = Q.ResidualLayout(case.n, case.blocks, device=DEV)
    w, _ = Q.loss_weights(lay, Q.ResidualLoss(lay, case.losses), r_sol.contiguous())
    assert torch.equal(nls.LossWeights(), w)


# ------------------------------------------------------------------ d. the Python surface
def test_no_loss_anywhere_is_the_solver_of_before_bit_for_bit():
    """loss=None residuals go through mo_nls_solve_blocks as before; the same problem under an all-TRIVIAL table goes through
    mo_nls_solve_blocks_robust, which is then mo_nls_solve_blocks: the same variables, terminations and iteration counts."""
    case = R.rosen_case(R.STRICT_SEEDS["rosenbrock_huber"])
    B = len(case.starts)
    prm = NLS.Params(**case.params)
    a = NLS.ConstrainedNonlinearLeastSquares(case.device_problem(NLS, DEV, with_loss=False), batch=B, residual_blocks=True)
    assert a._cost_loss is None
    oa = a.Solve(prm, T(case.starts))
    b = NLS.ConstrainedNonlinearLeastSquares(case.device_problem(NLS, DEV, with_loss=False), batch=B, residual_blocks=True)
    b._cost_loss = Q.create_loss(b._cost_layout, [(R.TRIVIAL, 1.0)] * len(case.blocks))
    ob = b.Solve(prm, T(case.starts))
    assert torch.equal(a.variables(), b.variables())
    assert torch.equal(oa.termination_state, ob.termination_state) and torch.equal(oa.num_iterations, ob.num_iterations)
    assert torch.equal(torch.nan_to_num(oa.iterations), torch.nan_to_num(ob.iterations))
    assert torch.all(a.LossWeights() == 1)
    # and the robust run differs from it: the loss is active at these starts
    c = NLS.ConstrainedNonlinearLeastSquares(case.device_problem(NLS, DEV), batch=B, residual_blocks=True)
    oc = c.Solve(prm, T(case.starts))
    assert not torch.equal(torch.nan_to_num(oa.iterations), torch.nan_to_num(oc.iterations))


def test_loss_argument_errors():
    case = R.sphere_case([1, 3])
    with pytest.raises(L.MiniOptError, match="residual_blocks=True"):
        NLS.ConstrainedNonlinearLeastSquares(case.device_problem(NLS, DEV), batch=2)
    fn = case.block_fns_torch(DEV)[0]
    eq = case.eq_fns_torch(DEV)[0]
    bad = NLS.Problem.FromResiduals(6, [NLS.MakeResidual((0, 1), fn, 2)], [NLS.MakeResidual((0, 1), eq, 1, loss=NLS.Huber(1.0))])
    with pytest.raises(L.MiniOptError, match="equality"):
        NLS.ConstrainedNonlinearLeastSquares(bad, batch=2, residual_blocks=True)
    lay = Q.ResidualLayout(4, [((0, 1), 2), ((2, 3), 1), ((1, 2), 3)], device=DEV)
    for losses, word in (([(R.HUBER, 1.0), (R.CAUCHY, 0.0), (R.TRIVIAL, 1.0)], "block 1"),
                         ([(R.HUBER, 1.0), (R.CAUCHY, 1.0), (R.TUKEY, float("inf"))], "block 2"),
                         ([(R.HUBER, float("nan")), (R.CAUCHY, 1.0), (R.TUKEY, 1.0)], "block 0"),
                         ([(R.HUBER, 1.0), (R.CAUCHY, 1.0), (7, 1.0)], "block 2"),
                         ([(R.HUBER, -1.0), (R.CAUCHY, 1.0), (R.TUKEY, 1.0)], "block 0")):
        with pytest.raises(L.MiniOptError, match=word) as e:
            Q.ResidualLoss(lay, losses)
        assert e.value.code == -1                                      # MO_ERR_INVALID_ARGUMENT
    with pytest.raises(L.MiniOptError):
        NLS.ConstrainedNonlinearLeastSquares(NLS.Problem.FromResiduals(6, [NLS.MakeResidual((0, 1), fn, 2, loss=NLS.Tukey(0.0))]), batch=2,
                                             residual_blocks=True)
    other = Q.ResidualLayout(4, [((0, 1), 2), ((2, 3), 2)], device=DEV)
    loss = Q.ResidualLoss(lay, [(R.HUBER, 1.0)] * 3)
    with pytest.raises(L.MiniOptError, match="loss table built for"):
        Q.loss_weights(other, loss, torch.zeros(1, 4, dtype=torch.float64, device=DEV))
