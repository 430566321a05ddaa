"""GPU tests of the per-row weights of residual-block costs (run with -m gpu on an MI355X): mo_linearize_blocks_weighted,
mo_qp_gradients_blocks_weighted and mo_qp_tangent_rhs_blocks_weighted against their unweighted siblings (bit identity without weights and with
all-ones weights; exact equivalence with the call on (sqrt(w) J, sqrt(w) r) for weights that are powers of four), against the numpy
restatement (tests/weighted_blocks_reference.py), with zero weights over NaN rows, through the C ABI (strides, guards, NULL members, no
allocation) and through solve_qp(layout=..., weights=...) in reverse and forward mode.

Bounds.  dweights: |dev - ref| <= (2 R_b P_b + 8) u A per stacked row, the per-row factor of sens_fixtures.bound_factor and the rule of
test_gpu_blocks_diff.py: an entry is the product of two sums of at most P_b + 1 rounded products, negated, plus the pair corrections --
fewer than 2 P_b + 8 roundings relative to A, the restatement on absolute values.  rho along wdot: |dev - ref| <= (c_i + 4) u A per variable,
c_i = blocks_tangent_reference.term_counts (the per-element count of test_gpu_blocks_tangent.py: twice the roundings a term can pass
through, plus 8); the weighted kernel rounds a term twice more than its sibling (w t, and wdot t with its sum), doubled: + 4."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

from mini_opt_amd import _lib as L
from mini_opt_amd import diff as D
from mini_opt_amd import qp as Q
from oracle import oracle as orc
from tests import blocks_tangent_reference as BT
from tests import diff_reference as R
from tests import tangent_reference as TR
from tests import weighted_blocks_reference as WR
from tests.sens_fixtures import DEV, LAM, N7_COST, PARAMS, UNIT, Guarded, T, autograd_layout, bound_factor, cus, oracle_kkt_solves, random_layout, rel_inf_rows

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
SHAPES = ["n7", "n33", "n64"]


def shape(name):
    if name == "n7":
        return 7, N7_COST
    if name == "n33":
        return 33, random_layout(np.random.default_rng(33), 33, 14, repeats=True)
    rng = np.random.default_rng(64)
    return 64, [(tuple(int(i) for i in rng.permutation(64)[:4]), 2) for _ in range(96)]


def rnd(a, dt):
    return a.astype(np.float32).astype(np.float64) if dt == torch.float32 else a


class Data:
    """One batch: host arrays (float64 holding values of the dtype) and device tensors.  J, r, weights [B, ...]; v, u [B, n]; tangents."""

    def __init__(self, rng, n, blocks, B, dt, weights="pow4"):
        self.n, self.blocks, self.B, self.dt = n, blocks, B, dt
        self.lay = Q.ResidualLayout(n, blocks, dtype=dt)
        vals, rows = self.lay.values, self.lay.rows
        self.J, self.r = rnd(rng.uniform(-1, 1, (B, vals)), dt), rnd(rng.uniform(-1, 1, (B, rows)), dt)
        self.v, self.u = rnd(rng.normal(size=(B, n)), dt), rnd(rng.normal(size=(B, n)), dt)
        if weights == "pow4":
            self.w = rng.choice([0.25, 1.0, 4.0], (B, rows))
        elif weights == "ones":
            self.w = np.ones((B, rows))
        else:                                   # general weights in [0, 2], one row in eight exactly 0
            self.w = rnd(rng.uniform(0, 2, (B, rows)), dt) * (rng.random((B, rows)) >= 0.125)
        self.t = dict(J_blocks=rnd(rng.normal(size=(B, vals)), dt), r=rnd(rng.normal(size=(B, rows)), dt), lam=rnd(rng.normal(size=B), dt),
                      weights=rnd(rng.normal(size=(B, rows)), dt))
        # per packed value its stacked row: the row map of the packing
        self.row_of = np.concatenate([off + np.tile(np.arange(R_), len(idx)) for (idx, R_), off in
                                      zip(blocks, np.cumsum([0] + [R_ for _, R_ in blocks[:-1]]))])

    def dev(self, a):
        return T(a, self.dt)


# ---- the three entry points, raw (weights None -> NULL) --------------------------------------------------------------------------------------
def stride(t, B):
    return 0 if t is None or (int(t.shape[0]) == 1 and B > 1) else int(t.shape[1])


def c_linearize(lay, J, r, w, B, lam=LAM, want_G=True):
    n = lay.n
    G = torch.empty(B, n, n, dtype=lay.dtype, device=DEV) if want_G else None
    c, f = torch.empty(B, n, dtype=lay.dtype, device=DEV), torch.empty(B, dtype=lay.dtype, device=DEV)
    L.check(L.lib().mo_linearize_blocks_weighted(lay._plan, lay.h, Q._ptr(J), stride(J, B), Q._ptr(r), stride(r, B), Q._ptr(w), stride(w, B), lam,
                                                 None, 0, B, Q._ptr(G), n * n, n, Q._ptr(c), n, Q._ptr(f), Q._stream()))
    return G, c, f


def c_gradients(lay, J, r, w, v, u, want=("J_blocks", "r", "lam", "weights"), k=0, m=0):
    B, V = int(v.shape[0]), int(v.shape[1])
    g = L.BlockWeightedGrads()
    out = {}
    for nm, (ptr, st, width) in dict(J_blocks=("dJ_blocks", "dJ_stride", lay.values), r=("dr", "dr_stride", lay.rows),
                                     lam=("dlambda", "dlambda_stride", 1), weights=("dweights", "dweights_stride", lay.rows)).items():
        if nm in want:
            out[nm] = torch.empty(B, width, dtype=lay.dtype, device=DEV)
            setattr(g, ptr, out[nm].data_ptr())
            setattr(g, st, width)
    plan = D._plan_of(lay.n, k, m, 0, lay.dtype, torch.device(DEV), B)
    L.check(L.lib().mo_qp_gradients_blocks_weighted(plan, lay.h, Q._ptr(J), stride(J, B), Q._ptr(r), stride(r, B), Q._ptr(w), stride(w, B), B,
                                                    Q._ptr(v), V, Q._ptr(u), V, C.byref(g), Q._stream()))
    return out


def c_tangent(lay, J, r, w, v, tang, k=0, m=0):
    B, V = int(v.shape[0]), int(v.shape[1])
    t = L.BlockWeightedTangents()
    for nm, (ptr, st) in dict(J_blocks=("dJ_blocks", "dJ_stride"), r=("dr", "dr_stride"), lam=("dlambda", "dlambda_stride"),
                              weights=("dweights", "dweights_stride")).items():
        if nm in tang:
            setattr(t, ptr, tang[nm].data_ptr())
            setattr(t, st, 1 if tang[nm].dim() == 1 else stride(tang[nm], B))
    rho = torch.empty_like(v)
    plan = D._plan_of(lay.n, k, m, 0, lay.dtype, torch.device(DEV), B)
    L.check(L.lib().mo_qp_tangent_rhs_blocks_weighted(plan, lay.h, Q._ptr(J), stride(J, B), Q._ptr(r), stride(r, B), Q._ptr(w), stride(w, B), None,
                                                      None, 0, B, Q._ptr(v), V, C.byref(t), Q._ptr(rho), V, Q._stream()))
    return rho


# ---- 1. bit identity with the siblings ---------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", ["n7", "n33"])
def test_weighted_calls_without_weights_and_with_ones_are_their_siblings(name, dt):
    n, blocks = shape(name)
    d = Data(np.random.default_rng(5100 + n), n, blocks, 37, dt, weights="ones")
    J, r, v, u = d.dev(d.J), d.dev(d.r), d.dev(d.v), d.dev(d.u)
    tang = {key: d.dev(d.t[key]) for key in ("J_blocks", "r", "lam")}
    G0, c0, f0 = Q.linearize_blocks(d.lay, J, r, lam=LAM)
    g0 = D.qp_gradients_blocks(d.lay, J, r, v, u)
    rho0 = D.qp_tangent_rhs_blocks(d.lay, J, r, v, tang)
    for w in (None, d.dev(d.w)):
        G, c, f = c_linearize(d.lay, J, r, w, d.B)
        assert torch.equal(G, G0) and torch.equal(c, c0) and torch.equal(f, f0)
        _, c_only, f_only = c_linearize(d.lay, J, r, w, d.B, want_G=False)
        assert torch.equal(c_only, c0) and torch.equal(f_only, f0)
        g = c_gradients(d.lay, J, r, w, v, u, want=("J_blocks", "r", "lam"))
        assert torch.equal(g["J_blocks"], g0["J_blocks"]) and torch.equal(g["r"], g0["r"]) and torch.equal(g["lam"][:, 0], g0["lam"])
        assert torch.equal(c_tangent(d.lay, J, r, w, v, tang), rho0)


# ---- 2. exact equivalence with pre-scaling -----------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", SHAPES)
def test_weights_that_are_powers_of_four_equal_the_prescaled_call(name, dt):
    """sqrt(w) in {1/2, 1, 2}: scaling by it commutes with every rounding, so the weighted calls must give the bits of the unweighted calls on
    (sqrt(w) J, sqrt(w) r) -- and sqrt(w) times their dJ_blocks and dr."""
    n, blocks = shape(name)
    d = Data(np.random.default_rng(5200 + n), n, blocks, 37, dt, weights="pow4")
    sq = np.sqrt(d.w)
    J, r, w, v, u = d.dev(d.J), d.dev(d.r), d.dev(d.w), d.dev(d.v), d.dev(d.u)
    sJ, sr = d.dev(d.J * sq[:, d.row_of]), d.dev(d.r * sq)
    G, c, f = Q.linearize_blocks(d.lay, J, r, lam=LAM, weights=w)
    G0, c0, f0 = Q.linearize_blocks(d.lay, sJ, sr, lam=LAM)
    assert torch.equal(G, G0) and torch.equal(c, c0) and torch.equal(f, f0)
    g = D.qp_gradients_blocks_weighted(d.lay, J, r, w, v, u, want=("J_blocks", "r", "lam"))
    g0 = D.qp_gradients_blocks(d.lay, sJ, sr, v, u)
    assert torch.equal(g["J_blocks"], d.dev(sq[:, d.row_of]) * g0["J_blocks"]) and torch.equal(g["r"], d.dev(sq) * g0["r"])
    assert torch.equal(g["lam"], g0["lam"])
    for keys in (("J_blocks", "r", "lam"), ("J_blocks",), ("r",)):
        tang = {key: d.dev(d.t[key]) for key in keys}
        scaled = {key: d.dev(d.t[key] * (sq[:, d.row_of] if key == "J_blocks" else sq if key == "r" else 1.0)) for key in keys}
        assert torch.equal(D.qp_tangent_rhs_blocks_weighted(d.lay, J, r, w, v, tang), D.qp_tangent_rhs_blocks(d.lay, sJ, sr, v, scaled)), keys


# ---- 3. dweights, and rho along wdot, against the restatement --------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", SHAPES)
def test_dweights_and_rho_along_wdot_against_the_restatement(name, dt):
    n, blocks = shape(name)
    B = 9
    d = Data(np.random.default_rng(5300 + n), n, blocks, B, dt, weights="general")
    d.w[:, 1] = 0.0                             # every problem has a row whose weight is exactly 0
    J, r, w, v, u = d.dev(d.J), d.dev(d.r), d.dev(d.w), d.dev(d.v), d.dev(d.u)
    got = {key: t.double().cpu().numpy() for key, t in D.qp_gradients_blocks_weighted(d.lay, J, r, w, v, u).items()}
    only = D.qp_gradients_blocks_weighted(d.lay, J, r, w, v, u, want=("weights",))
    assert set(only) == {"weights"} and np.array_equal(only["weights"].double().cpu().numpy(), got["weights"])
    rho_w = D.qp_tangent_rhs_blocks_weighted(d.lay, J, r, w, v, {"weights": d.dev(d.t["weights"])}).double().cpu().numpy()
    rho_all = D.qp_tangent_rhs_blocks_weighted(d.lay, J, r, w, v, {key: d.dev(a) for key, a in d.t.items()}).double().cpu().numpy()
    fv, fr = bound_factor(blocks)
    un = UNIT[dt]
    counts = BT.term_counts(n, 0, 0, blocks) + 4.0
    worst = {}

    def hold(key, err, tol):
        worst[key] = max(worst.get(key, 0.0), float(np.max(err / np.maximum(tol, 1e-300))))
        assert np.all(err <= tol), (name, key, worst[key])

    for p in (0, B // 2, B - 1):
        Js, rs, ws = WR.unpack(d.J[p], blocks), WR.split_rows(d.r[p], blocks), WR.split_rows(d.w[p], blocks)
        dJ, dr, dlam, dw = WR.gradients(blocks, Js, rs, ws, d.v[p], d.u[p])
        aJ, ar, alam, aw = WR.gradients(blocks, Js, rs, ws, d.v[p], d.u[p], absolute=True)
        hold("dweights", np.abs(got["weights"][p] - np.concatenate(dw)), fr * un * np.concatenate(aw))
        hold("dJ", np.abs(got["J_blocks"][p] - WR.pack(dJ)), (fv + 2) * un * WR.pack(aJ))       # (one more rounding than the sibling: the weight)
        hold("dr", np.abs(got["r"][p] - np.concatenate(dr)), (fr + 2) * un * np.concatenate(ar))
        assert abs(got["lam"][p] - dlam) <= (n + 8) * un * alam
        zero = d.w[p] == 0
        assert zero.any() and np.all(got["r"][p][zero] == 0.0) and np.all(got["J_blocks"][p][zero[d.row_of]] == 0.0)
        for rho, keys in ((rho_w, ("weights",)), (rho_all, tuple(d.t))):
            tang = {key: (WR.unpack(d.t[key][p], blocks) if key == "J_blocks" else d.t[key][p] if key == "lam" else WR.split_rows(d.t[key][p], blocks))
                    for key in keys}
            ref = WR.tangent_rhs(n, blocks, Js, rs, ws, d.v[p], tang)
            mag = WR.tangent_rhs(n, blocks, Js, rs, ws, d.v[p], tang, absolute=True)
            hold("rho " + "+".join(keys), np.abs(rho[p] - ref), counts * un * mag)
    print(f"weighted {name} {dt}: worst |dev - ref| / bound {worst}")


# ---- 4. zero weights with garbage ----------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", SHAPES)
def test_zero_weights_mask_rows_that_hold_nan(name, dt):
    """A third of the rows of every second problem: w = 0, J and r NaN there.  G, c, half_sq, dJ_blocks and dr are those of the call where the
    rows hold zeros; dJ_blocks and dr at the masked rows are exactly 0; solve_qp returns status OK and a finite x for every problem."""
    n, blocks = shape(name)
    rng = np.random.default_rng(5400 + n)
    B = 12
    d = Data(rng, n, blocks, B, dt, weights="general")
    d.w = np.where(d.w == 0, 1.0, d.w)
    rows = d.lay.rows
    mask = np.zeros((B, rows), bool)
    for p in range(0, B, 2):
        mask[p, rng.permutation(rows)[:max(1, rows // 3)]] = True
    d.w[mask] = 0.0
    vmask = mask[:, d.row_of]
    Jz, rz = np.where(vmask, 0.0, d.J), np.where(mask, 0.0, d.r)
    Jn, rn = np.where(vmask, np.nan, d.J), np.where(mask, np.nan, d.r)
    w, v, u = d.dev(d.w), d.dev(d.v), d.dev(d.u)
    out = {}
    for key, (J, r) in dict(zeros=(d.dev(Jz), d.dev(rz)), nan=(d.dev(Jn), d.dev(rn))).items():
        out[key] = (Q.linearize_blocks(d.lay, J, r, lam=LAM, weights=w), D.qp_gradients_blocks_weighted(d.lay, J, r, w, v, u, want=("J_blocks", "r", "lam")))
    (lin_z, g_z), (lin_n, g_n) = out["zeros"], out["nan"]
    for a, b in zip(lin_z, lin_n):
        assert torch.all(torch.isfinite(b)) and torch.equal(a, b)
    for key in g_z:
        assert torch.all(torch.isfinite(g_n[key])) and torch.equal(g_z[key], g_n[key]), key
    assert torch.all(g_n["J_blocks"][torch.as_tensor(vmask, device=DEV)] == 0) and torch.all(g_n["r"][torch.as_tensor(mask, device=DEV)] == 0)
    x, status = D.solve_qp(layout=d.lay, J_blocks=d.dev(Jn), r=d.dev(rn), lam=LAM, weights=w, params=Q.Params(**PARAMS), return_status=True)
    assert torch.all(status == 0) and torch.all(torch.isfinite(x))
    x0 = D.solve_qp(layout=d.lay, J_blocks=d.dev(Jz), r=d.dev(rz), lam=LAM, weights=w, params=Q.Params(**PARAMS))
    assert torch.equal(x, x0)


# ---- 5. every loop wraps, both instantiations, the second problem of a workgroup ------------------------------------------------------------
def wrap_layouts(dt):
    """(n, blocks): more than 256 stacked rows and more than 256 x 4 packed values (staged); one block beyond the 48 KiB stage budget, the
    construction of test_blocks_grad_unstaged_instantiation with n = 128 (unstaged)."""
    rng = np.random.default_rng(5500)
    big = [(tuple(int(i) for i in rng.permutation(40)[:4]), 3) for _ in range(90)] + [((7, 2, 7), 2)]
    assert sum(R_ for _, R_ in big) > 256 and sum(R_ * len(idx) for idx, R_ in big) > 1024
    R_, P = (80, 77) if dt == torch.float64 else (112, 110)
    assert (R_ * P + 2 * R_) * (8 if dt == torch.float64 else 4) > 48 * 1024
    return [("staged", 40, big), ("unstaged", 128, [(tuple(int(i) for i in rng.permutation(128)[:P]), R_)])]


@DTYPES
@pytest.mark.parametrize("which", [0, 1], ids=["staged", "unstaged"])
def test_weighted_loops_wrap_and_the_second_problem_of_a_workgroup(which, dt):
    """batch = grid + 19 with the grid at its largest (8 workgroups per CU; a smaller grid only gives every workgroup more problems), problem
    p + grid a copy of problem p: the copies are taken by a workgroup that has already run a problem and must give the same bits.  The values
    are pinned by the exact equivalence with the pre-scaled unweighted calls (weights powers of four) and dweights by its restatement."""
    tag, n, blocks = wrap_layouts(dt)[which]
    grid, extra = 8 * cus(), 19
    B = grid + extra
    rng = np.random.default_rng(5510 + which)
    lay = Q.ResidualLayout(n, blocks, dtype=dt)
    gen = torch.Generator(device=DEV).manual_seed(5520 + which)
    U = lambda *s: torch.rand(*s, generator=gen, dtype=dt, device=DEV) * 2 - 1
    J, r, v, u = U(B, lay.values), U(B, lay.rows), U(B, n), U(B, n)
    w = torch.tensor([0.25, 1.0, 4.0], dtype=dt, device=DEV)[torch.randint(0, 3, (B, lay.rows), generator=gen, device=DEV)]
    dJt, drt, dwt = U(B, lay.values), U(B, lay.rows), U(B, lay.rows)
    for t in (J, r, v, u, w, dJt, drt, dwt):
        t[grid:] = t[:extra]
    row_of = torch.as_tensor(np.concatenate([off + np.tile(np.arange(R_), len(idx)) for (idx, R_), off in
                                             zip(blocks, np.cumsum([0] + [R_ for _, R_ in blocks[:-1]]))]), device=DEV)
    sq = torch.sqrt(w)
    sJ, sr = J * sq[:, row_of], r * sq
    G, c, f = Q.linearize_blocks(lay, J, r, lam=LAM, weights=w)
    G0, c0, f0 = Q.linearize_blocks(lay, sJ, sr, lam=LAM)
    assert torch.equal(G, G0) and torch.equal(c, c0) and torch.equal(f, f0)
    g = D.qp_gradients_blocks_weighted(lay, J, r, w, v, u)
    g0 = D.qp_gradients_blocks(lay, sJ, sr, v, u)
    assert torch.equal(g["J_blocks"], sq[:, row_of] * g0["J_blocks"]) and torch.equal(g["r"], sq * g0["r"]) and torch.equal(g["lam"], g0["lam"])
    rho = D.qp_tangent_rhs_blocks_weighted(lay, J, r, w, v, {"J_blocks": dJt, "r": drt})
    assert torch.equal(rho, D.qp_tangent_rhs_blocks(lay, sJ, sr, v, {"J_blocks": dJt * sq[:, row_of], "r": drt * sq}))
    rho_w = D.qp_tangent_rhs_blocks_weighted(lay, J, r, w, v, {"J_blocks": dJt, "r": drt, "weights": dwt})
    for t in (G, c, f, g["J_blocks"], g["r"], g["lam"], g["weights"], rho, rho_w):
        assert torch.equal(t[grid:], t[:extra]), tag
    assert torch.all(torch.isfinite(rho_w)) and not torch.equal(rho_w, rho)
    fr = bound_factor(blocks)[1]
    for p in (0, B - 1):
        h = lambda t: t[p].double().cpu().numpy()
        Js, rs, ws = WR.unpack(h(J), blocks), WR.split_rows(h(r), blocks), WR.split_rows(h(w), blocks)
        if which == 0:
            dw = np.concatenate(WR.gradients(blocks, Js, rs, ws, h(v), h(u))[3])
            aw = np.concatenate(WR.gradients(blocks, Js, rs, ws, h(v), h(u), absolute=True)[3])
        else:   # one block without a repeated variable: dw = -s t in closed form (the restatement's triple loop would take seconds here)
            ii = list(blocks[0][0])
            dw = -(Js[0] @ h(u)[ii]) * (Js[0] @ h(v)[ii] + rs[0])
            aw = (np.abs(Js[0]) @ np.abs(h(u)[ii])) * (np.abs(Js[0]) @ np.abs(h(v)[ii]) + np.abs(rs[0]))
        assert np.all(np.abs(h(g["weights"]) - dw) <= fr * UNIT[dt] * aw), (tag, p)


# ---- 6. strides, guards and NULL members ---------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("shared", [False, True], ids=["per_problem", "stride0"])
def test_weighted_strides_guards_null_members_and_determinism(shared, dt):
    """Every pointer argument at an odd element offset with a stride larger than its tail inside a guarded buffer; shared: J_stride = 0 and
    weights_stride = 0 (one instance each).  The results are those of the contiguous calls; every output member NULL in turn; two launches
    give equal bits; no canary is touched."""
    n, blocks, B, pad = 7, N7_COST, 5, 3
    d = Data(np.random.default_rng(5600), n, blocks, B, dt, weights="general")
    lay = d.lay
    vals, rows = lay.values, lay.rows
    bufs = []

    def put(a, lead=B):
        """[lead, width] host array -> (pointer, stride) of a strided copy at an odd offset inside a Guarded buffer."""
        a = np.atleast_2d(a)[:lead]
        width = a.shape[1]
        g = Guarded(lead * (width + pad), dt, off=1)
        g.view.view(lead, width + pad)[:, :width] = T(a, dt)
        bufs.append(g)
        return g.view.data_ptr(), (0 if lead == 1 else width + pad)

    def out(width):
        g = Guarded(B * (width + pad), dt, off=1)
        bufs.append(g)
        return g

    S = 1 if shared else B
    Jp, Js_ = put(d.J, S)
    rp, rs_ = put(d.r)
    wp, ws_ = put(d.w, S)
    vp, vs_ = put(d.v)
    up, us_ = put(d.u)
    tang = {key: put(d.t[key].reshape(B, -1)) for key in d.t}
    J, r, w, v, u = d.dev(d.J[:S]), d.dev(d.r), d.dev(d.w[:S]), d.dev(d.v), d.dev(d.u)
    ref_lin = Q.linearize_blocks(lay, J, r, lam=LAM, weights=w)
    ref_g = D.qp_gradients_blocks_weighted(lay, J, r, w, v, u)
    ref_rho = D.qp_tangent_rhs_blocks_weighted(lay, J, r, w, v, {key: d.dev(a) for key, a in d.t.items()})
    lib, stream = L.lib(), Q._stream()
    plan = D._plan_of(n, 0, 0, 0, dt, torch.device(DEV), B)
    rowsview = lambda g, width: g.view.view(B, width + pad)[:, :width]

    def lin(want_G=True, want_f=True):
        Gb, cb, fb = out(n * n), out(n), Guarded(B, dt, off=1)
        bufs.append(fb)
        L.check(lib.mo_linearize_blocks_weighted(lay._plan, lay.h, Jp, Js_, rp, rs_, wp, ws_, LAM, None, 0, B, Gb.view.data_ptr() if want_G else None,
                                                 n * n + pad, n, cb.view.data_ptr(), n + pad, fb.view.data_ptr() if want_f else None, stream))
        torch.cuda.synchronize()
        return rowsview(Gb, n * n).reshape(B, n, n), rowsview(cb, n), fb.view, Gb, fb

    G1, c1, f1, _, _ = lin()
    G2, c2, f2, _, _ = lin()
    assert torch.equal(G1, G2) and torch.equal(c1, c2) and torch.equal(f1, f2)
    assert torch.equal(G1, ref_lin[0]) and torch.equal(c1, ref_lin[1]) and torch.equal(f1, ref_lin[2])
    _, c3, _, Gb, fb = lin(want_G=False, want_f=False)
    assert torch.equal(c3, c1) and torch.all(Gb.buf == 777.0) and torch.all(fb.buf == 777.0)

    members = dict(J_blocks=("dJ_blocks", "dJ_stride", vals), r=("dr", "dr_stride", rows), lam=("dlambda", "dlambda_stride", 1),
                   weights=("dweights", "dweights_stride", rows))

    def grad(skip=None):
        g, got, held = L.BlockWeightedGrads(), {}, {}
        for nm, (ptr, st, width) in members.items():
            held[nm] = out(width)
            if nm != skip:
                setattr(g, ptr, held[nm].view.data_ptr())
                setattr(g, st, width + pad)
                got[nm] = rowsview(held[nm], width)
        L.check(lib.mo_qp_gradients_blocks_weighted(plan, lay.h, Jp, Js_, rp, rs_, wp, ws_, B, vp, vs_, up, us_, C.byref(g), stream))
        torch.cuda.synchronize()
        if skip:
            assert torch.all(held[skip].buf == 777.0), skip
        return got

    first = grad()
    for skip in (None, *members):
        got = grad(skip)
        for nm, t in got.items():
            assert torch.equal(t, first[nm]) and torch.equal(t.reshape(B, -1), ref_g[nm].reshape(B, -1)), (skip, nm)

    def tangent(skip=None):
        t = L.BlockWeightedTangents()
        for nm, (ptr, st) in dict(J_blocks=("dJ_blocks", "dJ_stride"), r=("dr", "dr_stride"), lam=("dlambda", "dlambda_stride"),
                                  weights=("dweights", "dweights_stride")).items():
            if nm != skip:
                setattr(t, ptr, tang[nm][0])
                setattr(t, st, tang[nm][1])
        rb = out(n)
        L.check(lib.mo_qp_tangent_rhs_blocks_weighted(plan, lay.h, Jp, Js_, rp, rs_, wp, ws_, None, None, 0, B, vp, vs_, C.byref(t),
                                                      rb.view.data_ptr(), n + pad, stream))
        torch.cuda.synchronize()
        return rowsview(rb, n)

    assert torch.equal(tangent(), ref_rho) and torch.equal(tangent(), tangent())
    for skip in d.t:                                         # a NULL member is a zero tangent
        rest = {key: d.dev(a) for key, a in d.t.items() if key != skip}
        assert torch.equal(tangent(skip), D.qp_tangent_rhs_blocks_weighted(lay, J, r, w, v, rest)), skip
    assert all(g.intact() for g in bufs)
    # the documented refusals, with a real plan: dweights without weights, and the LDS rule before any launch
    g = L.BlockWeightedGrads()
    g.dweights, g.dweights_stride = first["weights"].data_ptr(), rows + pad
    assert lib.mo_qp_gradients_blocks_weighted(plan, lay.h, Jp, Js_, rp, rs_, None, 0, B, vp, vs_, up, us_, C.byref(g), stream) == -1
    assert b"weights" in lib.mo_last_error()


def test_weighted_lds_rules_refuse_before_any_launch():
    """fp64, n = 8: 2 n + 3 rows values within 63 KiB <=> rows <= 2682 (the sibling's 2 n + 2 rows: 4024); 2 n + 3 rows within 64 KiB for the
    tangent <=> rows <= 2725.  One layout between the rules: the siblings accept what the weighted calls refuse."""
    n, B = 8, 2
    rows = 2800
    lay = Q.ResidualLayout(n, [((i % n,), 7) for i in range(rows // 7)])
    assert lay.rows == rows
    rng = np.random.default_rng(5700)
    J, r, w, v, u = (T(rng.uniform(-1, 1, (B, width))) for width in (lay.values, rows, rows, n, n))
    assert set(D.qp_gradients_blocks(lay, J, r, v, u)) == {"J_blocks", "r", "lam"}
    with pytest.raises(L.MiniOptError) as e:
        D.qp_gradients_blocks_weighted(lay, J, r, w, v, u)
    assert e.value.code == -3 and "63 KiB" in str(e.value)
    assert D.qp_tangent_rhs_blocks(lay, J, r, v, {"r": r}).shape == (B, n)
    with pytest.raises(L.MiniOptError) as e:
        D.qp_tangent_rhs_blocks_weighted(lay, J, r, w, v, {"r": r})
    assert e.value.code == -3 and "64 KiB" in str(e.value)
    G, c, f = Q.linearize_blocks(lay, J, r, lam=LAM, weights=w)        # no rule for the linearise: it reads from global memory
    assert torch.all(torch.isfinite(G)) and torch.all(torch.isfinite(c))


# ---- 7. the first call allocates nothing ---------------------------------------------------------------------------------------------------------
def test_first_weighted_calls_allocate_nothing():
    n, B = 64, 96
    _, blocks = shape("n64")
    d = Data(np.random.default_rng(5800), n, blocks, B, torch.float64, weights="general")
    J, r, w, v, u = d.dev(d.J), d.dev(d.r), d.dev(d.w), d.dev(d.v), d.dev(d.u)
    tang = {key: d.dev(a) for key, a in d.t.items()}
    lays = [d.lay, Q.ResidualLayout(n, blocks)]
    desc = L.PlanDesc(n, 0, 0, 0, L.MO_F64, 0, L.EXTRA_PLAN_FLAGS, 0, B)
    plans = [C.c_void_p(), C.c_void_p()]
    for pl in plans:
        L.check(L.lib().mo_plan_create(C.byref(desc), C.byref(pl)))
    G, c, f = torch.empty(B, n, n, dtype=torch.float64, device=DEV), torch.empty(B, n, dtype=torch.float64, device=DEV), torch.empty(B, dtype=torch.float64, device=DEV)
    outs = dict(dJ_blocks=torch.empty_like(J), dr=torch.empty_like(r), dlambda=torch.empty(B, dtype=torch.float64, device=DEV), dweights=torch.empty_like(r))
    g, t = L.BlockWeightedGrads(), L.BlockWeightedTangents()
    for (nm, o), st in zip(outs.items(), ("dJ_stride", "dr_stride", "dlambda_stride", "dweights_stride")):
        setattr(g, nm, o.data_ptr())
        setattr(g, st, o[0].numel())
    for nm, st, key in (("dJ_blocks", "dJ_stride", "J_blocks"), ("dr", "dr_stride", "r"), ("dlambda", "dlambda_stride", "lam"), ("dweights", "dweights_stride", "weights")):
        setattr(t, nm, tang[key].data_ptr())
        setattr(t, st, tang[key][0].numel())
    rho = torch.empty_like(v)
    lib, s = L.lib(), Q._stream()

    def all_three(i):
        lay = lays[i]
        L.check(lib.mo_linearize_blocks_weighted(lay._plan, lay.h, Q._ptr(J), lay.values, Q._ptr(r), lay.rows, Q._ptr(w), lay.rows, LAM, None, 0, B,
                                                 Q._ptr(G), n * n, n, Q._ptr(c), n, Q._ptr(f), s))
        L.check(lib.mo_qp_gradients_blocks_weighted(plans[i], lay.h, Q._ptr(J), lay.values, Q._ptr(r), lay.rows, Q._ptr(w), lay.rows, B, Q._ptr(v), n,
                                                    Q._ptr(u), n, C.byref(g), s))
        L.check(lib.mo_qp_tangent_rhs_blocks_weighted(plans[i], lay.h, Q._ptr(J), lay.values, Q._ptr(r), lay.rows, Q._ptr(w), lay.rows, None, None, 0, B,
                                                      Q._ptr(v), n, C.byref(t), Q._ptr(rho), n, s))
        torch.cuda.synchronize()

    try:
        all_three(0)                                        # module load and kernel code happen on the twin first
        free0 = torch.cuda.mem_get_info()[0]
        all_three(1)                                        # the FIRST launches on this plan and this layout
        assert torch.cuda.mem_get_info()[0] >= free0 - (1 << 20), (free0, torch.cuda.mem_get_info()[0])
        assert all(torch.all(torch.isfinite(o)) for o in (G, c, f, rho, *outs.values()))
    finally:
        for pl in plans:
            L.lib().mo_plan_destroy(pl)


# ---- 8. autograd end to end ------------------------------------------------------------------------------------------------------------------------
class Problem:
    def __init__(self, n, case, rng, B):
        self.n, self.B, self.case = n, B, case
        self.blocks = autograd_layout(n, rng)
        self.lay = Q.ResidualLayout(n, self.blocks)
        self.eq_blocks = [(tuple(int(i) for i in rng.permutation(n)[:3]), 1), ((1, 6, 1), 2)] if case == "equalities" else []
        self.k = sum(R_ for _, R_ in self.eq_blocks)
        self.m = 4 if case == "bounds" else 0
        self.V = n + 2 * self.m + self.k
        self.eq_lay = Q.ResidualLayout(n, self.eq_blocks) if self.k else None
        self.J, self.r = rng.uniform(-1, 1, (B, self.lay.values)), rng.uniform(-1, 1, (B, self.lay.rows))
        self.w = rng.uniform(0.5, 2.0, (B, self.lay.rows))
        self.Jeq = rng.uniform(-1, 1, (B, self.eq_lay.values)) if self.k else np.zeros((B, 0))
        self.req = rng.uniform(-0.5, 0.5, (B, self.k))
        self.var = np.stack([rng.permutation(n)[:self.m] for _ in range(B)]).astype(np.int32)
        self.a, self.b = rng.choice([-1.0, 1.0], (B, self.m)), rng.uniform(5.0, 6.0, (B, self.m))       # loose: |x| stays far below 5
        self.t = dict(J_blocks=rng.normal(size=self.J.shape), r=rng.normal(size=self.r.shape), weights=rng.normal(size=self.w.shape))

    def solve(self, J=None, w=None, grad=("J_blocks", "r", "lam", "weights"), dual=(), var=None):
        """solve_qp on the problem's data (J, w: replacements, e.g. [1, ...]); returns (leaves, (x, s, y, z, status))."""
        B = self.B
        leaves = dict(J_blocks=T(self.J if J is None else J), r=T(self.r), lam=torch.full((B,), LAM, dtype=torch.float64, device=DEV),
                      weights=T(self.w if w is None else w))
        for key in grad:
            leaves[key].requires_grad_(True)
        inp = dict(leaves)
        for key in dual:
            tv = self.t[key]
            inp[key] = fwAD.make_dual(leaves[key], T(tv[:leaves[key].shape[0]]))
        kw = {}
        if self.k:
            kw.update(eq_layout=self.eq_lay, J_eq_blocks=T(self.Jeq), r_eq=T(self.req))
        if self.m:
            kw.update(cons_var=T(self.var if var is None else var, torch.int32), cons_a=T(self.a), cons_b=T(self.b))
        res = D.solve_qp(layout=self.lay, J_blocks=inp["J_blocks"], r=inp["r"], lam=inp["lam"], weights=inp["weights"], params=Q.Params(**PARAMS),
                         return_all=True, return_status=True, **kw)
        return leaves, res

    def qp(self, p):
        """(sym G, c, A, b_eq, Js, rs, ws) of problem p from the restatement."""
        Js, rs, ws = WR.unpack(self.J[p], self.blocks), WR.split_rows(self.r[p], self.blocks), WR.split_rows(self.w[p], self.blocks)
        G_low, c, _ = WR.linearize(self.n, self.blocks, Js, rs, ws, LAM)
        A = WR_jacobian(self.n, self.eq_blocks, self.Jeq[p]) if self.k else np.zeros((0, self.n))
        return WR.symmetric(G_low), c, A, self.req[p], Js, rs, ws


def WR_jacobian(n, eq_blocks, Jeq):
    from tests.blocks_diff_reference import jacobian
    return jacobian(n, eq_blocks, WR.unpack(Jeq, eq_blocks))


def oracle_state(pr, p, G, c, A, b_eq):
    k = pr.k
    o = orc.Solver(orc.QP(G=np.tril(G), c=c, A_eq=A if k else None, b_eq=b_eq if k else None, cons_var=pr.var[p], cons_a=pr.a[p], cons_b=pr.b[p]))
    o.solve(**PARAMS)
    return o, np.array(o.variables)


@pytest.mark.parametrize("case", ["unconstrained", "equalities", "bounds"])
@pytest.mark.parametrize("n", [8, 64])
def test_autograd_through_weighted_residual_blocks(n, case):
    """solve_qp(layout=..., weights=...) against the restatement evaluated AT THE DEVICE'S OWN v: K from the restated weighted linearisation,
    u by LU, the pair-by-pair gradients.  Bound max(1e-10, 10 D) of test_autograd_through_residual_blocks, D measured on the CPU the same way:
    the largest rel-inf between u from LU on the oracle's full system and u through the reduced system, at the oracle's optimum."""
    rng = np.random.default_rng(5900 + n + len(case))
    B = 6
    pr = Problem(n, case, rng, B)
    k, m = pr.k, pr.m
    leaves, (x, s, y, z, status) = pr.solve()
    assert torch.all(status == 0)
    assert D.adjoint_status(x) is None
    gx = rng.normal(size=(B, n))
    loss = (x * T(gx)).sum() + (y * y).sum()
    loss.backward(retain_graph=True)
    assert torch.all(D.adjoint_status(x) == 0)
    first = {key: t.grad.clone() for key, t in leaves.items()}
    for t in leaves.values():
        t.grad = None
    loss.backward()
    assert all(torch.equal(first[key], t.grad) for key, t in leaves.items())          # a second backward repeats the first, bitwise
    assert first["weights"].shape == (B, pr.lay.rows) and first["J_blocks"].shape == (B, pr.lay.values)
    v = torch.cat([x, s, y, z], dim=1).detach().cpu().numpy()
    g_full = np.concatenate([gx, np.zeros((B, m)), 2 * v[:, n + m:n + m + k], np.zeros((B, m))], axis=1)
    D_cpu, worst = 0.0, {}
    for p in range(B):
        G, c, A, b_eq, Js, rs, ws = pr.qp(p)
        o, vo = oracle_state(pr, p, G, c, A, b_eq)
        _, u_lu = oracle_kkt_solves(o, n, k, m, g_full[p], g_full[p])
        u_red = R.transposed_through_reduced(G, A, pr.var[p], pr.a[p], vo, g_full[p])
        D_cpu = max(D_cpu, float(rel_inf_rows(u_red[None], u_lu[None])[0]))
        u = R.solve_transposed(R.kkt_matrix(G, A, pr.var[p], pr.a[p], v[p]), g_full[p])
        dJ, dr, dlam, dw = WR.gradients(pr.blocks, Js, rs, ws, v[p, :n], u[:n])
        for key, want in dict(J_blocks=WR.pack(dJ), r=np.concatenate(dr), lam=np.array([dlam]), weights=np.concatenate(dw)).items():
            err = float(np.max(np.abs(first[key][p].cpu().numpy().reshape(-1) - want)) / np.max(np.abs(want)))
            worst[key] = max(worst.get(key, 0.0), err)
    bound = max(1e-10, 10 * D_cpu)
    print(f"weighted blocks autograd n = {n} {case}: D = {D_cpu:.3e}, bound {bound:.3e}, worst rel-inf per input {worst}")
    assert max(worst.values()) < bound, (worst, bound)

    # J_blocks given once, weights per problem: the one instance is read in place
    J1 = pr.J[:1]
    lv_exp, res_exp = pr.solve(J=np.repeat(J1, B, axis=0))             # the caller expands
    (res_exp[0] * T(gx)).sum().backward()
    lv_one, res_one = pr.solve(J=J1)
    assert torch.equal(res_one[0], res_exp[0])
    (res_one[0] * T(gx)).sum().backward()
    assert torch.equal(lv_one["weights"].grad, lv_exp["weights"].grad) and torch.equal(lv_one["r"].grad, lv_exp["r"].grad)
    assert lv_one["J_blocks"].grad.shape == (1, pr.lay.values) and torch.equal(lv_one["J_blocks"].grad, lv_exp["J_blocks"].grad.sum(0, keepdim=True))
    # only weights asks for a gradient: nothing else gets one
    lv_w, res_w = pr.solve(J=J1, grad=("weights",))
    (res_w[0] * T(gx)).sum().backward()
    assert torch.equal(lv_w["weights"].grad, lv_exp["weights"].grad) and lv_w["J_blocks"].grad is None and lv_w["r"].grad is None
    # weights given once
    lv_w1, res_w1 = pr.solve(w=pr.w[:1])
    lv_wB, res_wB = pr.solve(w=np.repeat(pr.w[:1], B, axis=0))
    assert torch.equal(res_w1[0], res_wB[0])
    (res_w1[0] * T(gx)).sum().backward()
    (res_wB[0] * T(gx)).sum().backward()
    assert lv_w1["weights"].grad.shape == (1, pr.lay.rows) and torch.equal(lv_w1["weights"].grad, lv_wB["weights"].grad.sum(0, keepdim=True))
    assert torch.equal(lv_w1["J_blocks"].grad, lv_wB["J_blocks"].grad)


def test_weighted_failing_problem_contributes_zero_to_every_summed_gradient():
    """One problem whose forward fails on purpose (a constraint index outside [0, n): MO_STATUS_BAD_INDEX) inside a healthy batch, with
    J_blocks and weights given once: the summed gradients are the sums over the healthy problems, to the bit those of the batch without it."""
    n, B = 8, 6
    pr = Problem(n, "bounds", np.random.default_rng(5950), B)
    gx = T(np.random.default_rng(5951).normal(size=(B, n)))
    var = pr.var.copy()
    var[3, 1] = n + 1
    lv, res = pr.solve(J=pr.J[:1], w=pr.w[:1], var=var)
    assert res[4][3].item() == L.MO_STATUS_BAD_INDEX and torch.all(res[4][[0, 1, 2, 4, 5]] == 0)
    (res[0] * gx).sum().backward()
    assert all(torch.all(torch.isfinite(t.grad)) for t in lv.values())
    assert torch.all(lv["r"].grad[3] == 0) and torch.all(lv["lam"].grad[3] == 0) and torch.any(lv["r"].grad[2] != 0)
    # the same batch with per-problem copies: the healthy problems' gradients, summed by hand
    lv_full, res_full = pr.solve(J=np.repeat(pr.J[:1], B, axis=0), w=np.repeat(pr.w[:1], B, axis=0), var=var)
    (res_full[0] * gx).sum().backward()
    assert torch.all(lv_full["J_blocks"].grad[3] == 0) and torch.all(lv_full["weights"].grad[3] == 0)
    assert torch.equal(lv["J_blocks"].grad, lv_full["J_blocks"].grad.sum(0, keepdim=True))
    assert torch.equal(lv["weights"].grad, lv_full["weights"].grad.sum(0, keepdim=True))


# ---- 9. forward mode -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["unconstrained", "equalities", "bounds"])
@pytest.mark.parametrize("n", [8, 64])
def test_forward_ad_through_weighted_residual_blocks(n, case):
    """forward_ad with a dual `weights` (alone, and together with dual J_blocks and r): g . vdot = sum <.grad, direction> against the backward
    of the same call, by Hoelder on the bound max(1e-10, 10 D) of test_forward_ad_through_residual_blocks -- D measured on the CPU at the
    oracle's optimum, the largest rel-inf between vdot from LU on the full K and vdot through the reduced system, for the restatement's rho."""
    rng = np.random.default_rng(6000 + n + len(case))
    B = 6
    pr = Problem(n, case, rng, B)
    k, m = pr.k, pr.m
    g = rng.normal(size=(B, pr.V))
    g[:, n:n + m] = 0.0
    g[:, n + m + k:] = 0.0
    lv, res = pr.solve()
    (torch.cat(res[:4], dim=1) * T(g)).sum().backward()
    D_cpu = 0.0
    for p in range(B):
        G, c, A, b_eq, Js, rs, ws = pr.qp(p)
        _, vo = oracle_state(pr, p, G, c, A, b_eq)
        tang = dict(J_blocks=WR.unpack(pr.t["J_blocks"][p], pr.blocks), r=WR.split_rows(pr.t["r"][p], pr.blocks),
                    weights=WR.split_rows(pr.t["weights"][p], pr.blocks))
        rho = np.zeros(pr.V)
        rho[:n] = WR.tangent_rhs(n, pr.blocks, Js, rs, ws, vo[:n], tang)
        lu, red = TR.vdot(G, A, pr.var[p], pr.a[p], vo, rho), TR.vdot_reduced(G, A, pr.var[p], pr.a[p], vo, rho)
        D_cpu = max(D_cpu, float(rel_inf_rows(red[None], lu[None])[0]))
    bound = max(1e-10, 10 * D_cpu)
    for dual in (("weights",), ("weights", "J_blocks", "r")):
        with fwAD.dual_level():
            _, rd = pr.solve(grad=(), dual=dual)
            assert torch.all(rd[4] == 0)
            st = D.tangent_status(rd[0])
            assert st is not None and st.shape == (B,) and st.dtype == torch.int32 and torch.all(st == 0)
            vdot = torch.cat([fwAD.unpack_dual(t).tangent for t in rd[:4]], dim=1).cpu().numpy()
        lhs = np.sum(g * vdot, axis=1)
        rhs = np.zeros(B)
        hold = np.sum(np.abs(g), axis=1) * np.max(np.abs(vdot), axis=1)
        for key in dual:
            gr, td = lv[key].grad.cpu().numpy().reshape(B, -1), pr.t[key].reshape(B, -1)
            rhs += np.sum(gr * td, axis=1)
            hold += np.max(np.abs(gr), axis=1) * np.sum(np.abs(td), axis=1)
        print(f"weighted forward_ad n = {n} {case} {dual}: D = {D_cpu:.3e}, max |g . vdot - sum <grad, tangent>| / Hoelder = {np.max(np.abs(lhs - rhs) / hold):.3e}")
        assert np.any(vdot != 0) and np.all(np.abs(lhs - rhs) <= bound * hold), (dual, lhs, rhs)


# ---- 10. the unweighted calls are untouched -----------------------------------------------------------------------------------------------------
def test_unweighted_solve_qp_builds_the_unweighted_node():
    n, B = 8, 4
    rng = np.random.default_rng(6100)
    blocks = autograd_layout(n, rng)
    lay = Q.ResidualLayout(n, blocks)
    Jb, r = T(rng.uniform(-1, 1, (B, lay.values))).requires_grad_(True), T(rng.uniform(-1, 1, (B, lay.rows)))
    w = T(rng.uniform(0.5, 2, (B, lay.rows)))

    def node(x):
        seen, todo = set(), [x.grad_fn]
        while todo:
            f = todo.pop()
            if f is None or f in seen:
                continue
            seen.add(f)
            if "QPSolve" in type(f).__name__:
                return type(f).__name__
            todo.extend(fn for fn, _ in f.next_functions)
        return None

    assert node(D.solve_qp(layout=lay, J_blocks=Jb, r=r, lam=LAM, params=Q.Params(**PARAMS))) == "QPSolveBlocksFunctionBackward"
    assert node(D.solve_qp(layout=lay, J_blocks=Jb, r=r, lam=LAM, weights=w, params=Q.Params(**PARAMS))) == "QPSolveWeightedBlocksFunctionBackward"
    assert tuple(D._BLOCK) == ("J_blocks", "r", "lam", "J_eq_blocks", "r_eq", "cons_a", "cons_b")
    assert D.QPSolveBlocksFunction.NAMES == tuple(D._BLOCK) and D.BLOCK_TANGENTS == tuple(D._BLOCK) and D.BLOCK_GRADIENTS == tuple(D._BLOCK)[:5]
    with pytest.raises(ValueError):
        D.solve_qp(G=T(np.tile(np.eye(n), (B, 1, 1))), c=T(np.zeros((B, n))), weights=w)
