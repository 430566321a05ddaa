"""GPU tests of forward mode for residual-block input (run with -m gpu on an MI355X): mo_qp_tangent_rhs_blocks against the pair-by-pair numpy
restatement (tests/blocks_tangent_reference.py) at caller-supplied state, against the dense mo_qp_tangent_rhs on the (G, c) problem, against
the merged block gradients through the transpose identity, through the C ABI (strides, NULL members, determinism, refusals, no allocation),
and torch.autograd.forward_ad through solve_qp(layout=...).

Per-element bound of the kernel, derived and not fitted: |dev - ref| <= c u A with u the unit round-off of the dtype, A the sum of the
magnitudes of the element's terms (blocks_tangent_reference.rho(absolute=True)) and c the term count of the layout
(blocks_tangent_reference.term_counts: twice the roundings any term can pass through, plus 8)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

from mini_opt_amd import _lib as L
from mini_opt_amd import diff as D
from mini_opt_amd import qp as Q
from oracle import oracle as orc
from tests import blocks_diff_reference as BR
from tests import blocks_tangent_reference as BT
from tests import diff_reference as R
from tests import tangent_reference as TR
from tests.sens_fixtures import DEV, LAM, N7_COST, PARAMS, UNIT, T, autograd_layout, bound_factor, random_layout, rel_inf_rows

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
N7_EQ = [((0, 4, 0), 1), ((2, 6, 1), 1)]          # the first local column of block 0 loses variable 0 to the last
KEYS = ("J_blocks", "r", "lam", "J_eq_blocks", "r_eq", "cons_a", "cons_b")
REF_KEY = dict(J_blocks="J_blocks", r="r", lam="lam", J_eq_blocks="J_eq_blocks", r_eq="r_eq", cons_a="a", cons_b="b")


class Case:
    """One batch on the host (float64 arrays holding values of the dtype) with its layouts on the device."""

    def __init__(self, rng, n, blocks, B, dt, eq_blocks=(), m=0, var=None, shared=False):
        self.n, self.blocks, self.eq_blocks, self.B, self.dt, self.m = n, list(blocks), list(eq_blocks), B, dt, m
        self.k = sum(R_ for _, R_ in self.eq_blocks)
        self.V = n + 2 * m + self.k
        self.lay = Q.ResidualLayout(n, self.blocks, dtype=dt)
        self.eq_lay = Q.ResidualLayout(n, self.eq_blocks, dtype=dt) if self.eq_blocks else None
        S = 1 if shared else B
        eqv = self.eq_lay.values if self.eq_lay else 0
        rnd = lambda a: a.astype(np.float32).astype(np.float64) if dt == torch.float32 else a
        self.J, self.r = rnd(rng.uniform(-1, 1, (S, self.lay.values))), rnd(rng.uniform(-1, 1, (S, self.lay.rows)))
        self.v = rnd(rng.normal(size=(B, self.V)))
        self.var = (np.stack([rng.integers(0, n, m) for _ in range(B)]) if var is None else np.tile(np.asarray(var), (B, 1))).astype(np.int32)
        self.t = dict(J_blocks=rnd(rng.normal(size=(S, self.lay.values))), r=rnd(rng.normal(size=(S, self.lay.rows))), lam=rnd(rng.normal(size=S)),
                      J_eq_blocks=rnd(rng.normal(size=(S, eqv))), r_eq=rnd(rng.normal(size=(S, self.k))),
                      cons_a=rnd(rng.normal(size=(S, m))), cons_b=rnd(rng.normal(size=(S, m))))

    def keys(self, keys=KEYS):
        return [key for key in keys if not ((key in ("J_eq_blocks", "r_eq") and not self.k) or (key in ("cons_a", "cons_b") and not self.m))]

    def device(self, keys=KEYS):
        """rho [B, V] through the Python front end for the tangent members named."""
        tang = {key: T(self.t[key], self.dt) for key in self.keys(keys)}
        return D.qp_tangent_rhs_blocks(self.lay, T(self.J, self.dt), T(self.r, self.dt), T(self.v, self.dt), tang, k=self.k, m=self.m,
                                       eq_layout=self.eq_lay, cons_var=T(self.var, torch.int32) if self.m else None)

    def ref_tangents(self, p, keys):
        s = lambda a: a[0 if a.shape[0] == 1 else p]
        out = {}
        for key in self.keys(keys):
            val = s(self.t[key])
            if key == "J_blocks":
                val = BR.unpack(val, self.blocks)
            elif key == "r":
                val = BR.split_rows(val, self.blocks)
            elif key == "J_eq_blocks":
                val = BR.unpack(val, self.eq_blocks)
            out[REF_KEY[key]] = val
        return out

    def reference(self, p, keys=KEYS, absolute=False):
        s = lambda a: a[0 if a.shape[0] == 1 else p]
        return BT.rho(self.n, self.k, self.m, self.blocks, BR.unpack(s(self.J), self.blocks), BR.split_rows(s(self.r), self.blocks), self.v[p],
                      self.ref_tangents(p, keys), eq_blocks=self.eq_blocks, var=self.var[p], absolute=absolute)

    def counts(self, p):
        return BT.term_counts(self.n, self.k, self.m, self.blocks, self.eq_blocks, self.var[p])

    def check(self, got, keys=KEYS, problems=None, tag=""):
        got = got.double().cpu().numpy()
        assert got.shape == (self.B, self.V)
        worst = 0.0
        for p in (sorted({0, 1, self.B // 2, self.B - 2, self.B - 1} & set(range(self.B))) if problems is None else problems):
            ref, mag = self.reference(p, keys), self.reference(p, keys, absolute=True)
            assert np.array_equal(np.isnan(got[p]), np.isnan(ref)), (tag, p)
            ok = ~np.isnan(ref)
            err, tol = np.abs(got[p] - ref)[ok], (self.counts(p) * UNIT[self.dt] * mag)[ok]
            worst = max(worst, float(np.max(err / np.maximum(tol, 1e-300))))
            assert np.all(err <= tol), (tag, self.n, p, worst, np.argmax(err / np.maximum(tol, 1e-300)))
        print(f"{tag} n = {self.n} B = {self.B} {self.dt}: worst |dev - ref| / bound = {worst:.3e}")


# ---- 1. the kernel against the restatement at caller-supplied state -----------------------------------------------------------------------
@DTYPES
def test_blocks_tangent_single_value(dt):
    """n = 1, one 1 x 1 block, batch 1."""
    case = Case(np.random.default_rng(801), 1, [((0,), 1)], 1, dt)
    case.check(case.device(), tag="single")


@DTYPES
def test_blocks_tangent_repeated_indices_n7(dt):
    """The n = 7 layout of the block backward tests ((3, 0, 5, 3) and (2, 2) repeat a variable; variables repeat across blocks), k = 2 with an
    equality column that loses its global column and whose tangent entries are NaN, m = 3 with two rows on variable 2, batch 5: each
    tangent member alone, then all together."""
    case = Case(np.random.default_rng(802), 7, N7_COST, 5, dt, eq_blocks=N7_EQ, m=3, var=(2, 2, 5))
    case.t["J_eq_blocks"][:, 0] = np.nan                      # block ((0, 4, 0), 1): packed value 0 is the losing column
    for key in KEYS:
        got = case.device((key,))
        assert torch.all(torch.isfinite(got)), key
        case.check(got, (key,), tag=f"n7 {key} alone")
    got = case.device()
    assert torch.all(torch.isfinite(got))
    case.check(got, tag="n7 all")


@DTYPES
@pytest.mark.parametrize("repeats", [False, True], ids=["distinct", "repeats"])
@pytest.mark.parametrize("n", [8, 64, 128, 300])
def test_blocks_tangent_random_layouts(n, repeats, dt):
    """Random layouts (out-of-order indices, with and without a repeated variable inside a block), random equality blocks and constraint
    rows, batch 3.  Phase 3 gives a variable sixteen lanes at n = 8, four at 64, two at 128 and one at 300, where the workgroup also needs a
    second pass over the variables."""
    rng = np.random.default_rng(810 + n + int(repeats))
    blocks = random_layout(rng, n, count=max(6, min(60, n)), repeats=repeats)
    assert any(len(set(idx)) < len(idx) for idx, _ in blocks) == repeats
    eq_blocks = random_layout(rng, n, count=3, repeats=repeats)
    case = Case(rng, n, blocks, 3, dt, eq_blocks=eq_blocks, m=5)
    case.check(case.device(), tag="random")


@DTYPES
def test_blocks_tangent_unstaged_instantiation(dt):
    """n = 128, 130 blocks of 8 x 12: (values + rows) = 13 520 values exceed the 48 KiB stage budget in both dtypes (and the staged
    instantiation needs twice that: values and tangents), so J_blocks, dJ_blocks, r and dr are read from global memory.  Batch 2."""
    n, B = 128, 2
    rng = np.random.default_rng(820)
    blocks = [(tuple(int(i) for i in rng.permutation(n)[:12]), 8) for _ in range(130)]
    case = Case(rng, n, blocks, B, dt, eq_blocks=[((5, 9, 5), 2)], m=2)
    assert (case.lay.values + case.lay.rows) * (8 if dt == torch.float64 else 4) > 48 * 1024
    case.check(case.device(), tag="unstaged")


@DTYPES
def test_blocks_tangent_workgroups_loop_over_problems(dt):
    """n = 8 with batch = 2 x grid + 3 (grid = eight workgroups per CU): every workgroup takes a second problem, three take a third, and all
    re-use their LDS; the second and third problems of a workgroup are among the ones checked."""
    rng = np.random.default_rng(830)
    grid = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    B = 2 * grid + 3
    blocks = random_layout(rng, 8, count=6, repeats=True)
    case = Case(rng, 8, blocks, B, dt, eq_blocks=[((1, 6, 1), 2)], m=2)
    case.check(case.device(), problems=[0, 1, grid - 1, grid, grid + 1, B // 2, 2 * grid - 1, 2 * grid, 2 * grid + 1, 2 * grid + 2], tag="loop")


# ---- 2. agreement with the dense path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("repeats", [False, True], ids=["distinct", "repeats"])
@pytest.mark.parametrize("n", [12, 64])
def test_blocks_tangent_matches_dense_path(n, repeats):
    """lambda = 0.  dG = G(J + dJ) - G(J) - G(dJ) and dc = c(J + dJ, r + dr) - c(J, r) - c(dJ, dr) by mo_linearize_blocks (exact polarisation of a
    quadratic map), dA_eq = mo_jacobian_blocks(dJ_eq); mo_qp_tangent_rhs on the (G, c) problem against the block call, fp64.
    Bound per element: the block kernel's own c u A, plus the dense side: the polarisation cancels, so its error is that of the three
    linearisations, each cell a sum of at most N_cell rounded products, carried through a sum of n + k + m + 2 further terms:
    (2 (N_cell + n + k + m) + 8) u (sym(|G|(|J + dJ|) + |G|(|J|) + |G|(|dJ|)) |x| + the same for c + A), |.| the linearisation of absolute
    values, A the block call's magnitudes for the terms that do not come from the polarisation."""
    rng = np.random.default_rng(840 + n + int(repeats))
    blocks = random_layout(rng, n, count=3 * n // 2, repeats=repeats)
    eq_blocks = random_layout(rng, n, count=2, repeats=repeats)
    dt, B = torch.float64, 4
    case = Case(rng, n, blocks, B, dt, eq_blocks=eq_blocks, m=3)
    case.t["lam"][:] = 0.0
    keys = [key for key in KEYS if key != "lam"]
    got = case.device(keys)
    case.check(got, keys, tag="dense (block side)")
    lay, eq_lay, k, m = case.lay, case.eq_lay, case.k, case.m
    lin = lambda J, r: Q.linearize_blocks(lay, T(J), T(r), lam=0.0)[:2]
    (G2, c2), (G1, c1), (G0, c0) = lin(case.J + case.t["J_blocks"], case.r + case.t["r"]), lin(case.J, case.r), lin(case.t["J_blocks"], case.t["r"])
    dG, dc = G2 - G1 - G0, c2 - c1 - c0
    dA, _ = Q.jacobian_blocks(eq_lay, T(case.t["J_eq_blocks"]), T(case.t["r_eq"]))
    A0, _ = Q.jacobian_blocks(eq_lay, T(np.zeros_like(case.t["J_eq_blocks"])), T(case.t["r_eq"]))
    prob = Q.BatchedQP(n=n, k=k, m=m, G=G1, c=c1, A_eq=A0, b_eq=T(case.t["r_eq"]), cons_var=T(case.var, torch.int32),
                       cons_a=T(np.ones((B, m))), cons_b=T(np.ones((B, m))))
    dense = D.qp_tangent_rhs(prob, T(case.v), {"G": dG, "c": dc, "A_eq": dA, "b_eq": T(case.t["r_eq"]), "cons_a": T(case.t["cons_a"]),
                                               "cons_b": T(case.t["cons_b"])}).cpu().numpy()
    got = got.cpu().numpy()
    ones = BR.linearize(n, blocks, [np.ones((R_, len(idx))) for idx, R_ in blocks], [np.ones(R_) for _, R_ in blocks])
    n_cell = max(float(np.max(ones[0])), float(np.max(ones[1])))
    un = UNIT[dt]
    for p in range(B):
        mag, cnt = case.reference(p, keys, absolute=True), case.counts(p)
        x = np.abs(case.v[p, :n])
        lin_mag = np.zeros(n)
        for J, r in ((case.J[p] + case.t["J_blocks"][p], case.r[p] + case.t["r"][p]), (case.J[p], case.r[p]), (case.t["J_blocks"][p], case.t["r"][p])):
            Ga, ca = BR.linearize(n, blocks, BR.unpack(np.abs(J), blocks), BR.split_rows(np.abs(r), blocks))
            lin_mag += BR.symmetric(Ga) @ x + ca
        extra = np.concatenate([lin_mag, np.zeros(m), np.zeros(k), np.zeros(m)])
        tol = cnt * un * mag + (2 * (n_cell + n + k + m) + 8) * un * (mag + extra)
        err = np.abs(got[p] - dense[p])
        assert np.all(err <= tol), (n, p, float(np.max(err / np.maximum(tol, 1e-300))))
        assert np.all(dense[p, n:n + m] == 0) and np.all(got[p, n:n + m] == 0)


# ---- 3. the transpose identity on the device -------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("n", [7, 64])
def test_blocks_tangent_transpose_identity_on_the_device(n, dt):
    """For random (vars, u):  u . rho = -sum <qp_gradients_blocks / qp_gradients_eq_blocks / qp_gradients(cons_a, cons_b), tangents>.  Both
    sides are held to their own derived bounds against their restatements, so the two dot products (taken in float64 on the host) differ
    by at most  u_dt (c_max |u| . A_rho + sum_members f_max A_grad . |tangent|),  A the magnitudes of the two restatements, c_max the
    largest term count and f_max the largest bound factor of the gradient tests; the host's own sums add 2^-53 (V + values) of the same
    magnitudes, covered by the + V + values in the factors."""
    rng = np.random.default_rng(850 + n)
    blocks = N7_COST if n == 7 else random_layout(rng, n, count=60, repeats=True)
    eq_blocks = N7_EQ if n == 7 else random_layout(rng, n, count=3, repeats=True)
    B, m = 4, 3
    case = Case(rng, n, blocks, B, dt, eq_blocks=eq_blocks, m=m)
    k, V = case.k, case.V
    u = rng.normal(size=(B, V))
    if dt == torch.float32:
        u = u.astype(np.float32).astype(np.float64)
    v_d, u_d = T(case.v, dt), T(u, dt)
    rho = case.device().double().cpu().numpy()
    cost = D.qp_gradients_blocks(case.lay, T(case.J, dt), T(case.r, dt), v_d, u_d, k=k, m=m)
    eq = D.qp_gradients_eq_blocks(case.eq_lay, v_d, u_d, m=m)
    prob = Q.BatchedQP(n=n, k=k, m=m, G=T(np.tile(np.eye(n), (B, 1, 1)), dt), c=T(np.zeros((B, n)), dt), A_eq=T(np.zeros((B, n, k)), dt),
                       b_eq=T(np.zeros((B, k)), dt), cons_var=T(case.var, torch.int32), cons_a=T(np.ones((B, m)), dt), cons_b=T(np.ones((B, m)), dt))
    cons = D.qp_gradients(prob, v_d, u_d, want=("cons_a", "cons_b"))
    grads = dict(cost, **eq, **cons)
    assert set(grads) == set(KEYS)
    fv, fr = bound_factor(blocks)
    f_max = max(float(fv.max()), float(fr.max()), n + 8.0) + V + case.lay.values
    un = UNIT[dt]
    for p in range(B):
        lhs = float(u[p] @ rho[p])
        rhs = -sum(float(grads[key][p].double().cpu().numpy().reshape(-1) @ np.atleast_1d(case.t[key][p]).reshape(-1)) for key in KEYS)
        x, _, y, z = R.split(case.v[p], n, k, m)
        ux, _, uy, uz = R.split(u[p], n, k, m)
        aJ, ar, alam = BR.gradients_blocks(blocks, BR.unpack(case.J[p], blocks), BR.split_rows(case.r[p], blocks), x, ux, absolute=True)
        aJe, are = BR.gradients_eq_blocks(eq_blocks, x, ux, y, uy, absolute=True)
        a_grad = dict(J_blocks=BR.pack(aJ), r=np.concatenate(ar), lam=np.array([alam]), J_eq_blocks=BR.pack(aJe), r_eq=are,
                      cons_a=np.abs(z * ux[case.var[p]]) + np.abs(uz * x[case.var[p]]), cons_b=np.abs(uz))
        bound = (float(case.counts(p).max()) + V) * float(np.abs(u[p]) @ case.reference(p, absolute=True))
        bound += f_max * sum(float(a_grad[key] @ np.abs(np.atleast_1d(case.t[key][p]).reshape(-1))) for key in KEYS)
        print(f"transpose identity n = {n} {dt} problem {p}: u . rho = {lhs:.12e}, -sum <grad, tangent> = {rhs:.12e}, |diff| / bound = {abs(lhs - rhs) / (un * bound):.3e}")
        assert abs(lhs - rhs) <= un * bound, (n, p, lhs, rhs)


# ---- 4. the C ABI: strides, NULL members, determinism, bad indices, refusals, no allocation -------------------------------------------------
SENT = -777.25


class Raw:
    """mo_qp_tangent_rhs_blocks through ctypes with padded strides: vars and rho [B, V + pad], sentinels in the padding."""

    def __init__(self, case, pad=3):
        self.case, self.pad = case, pad
        c = case
        self.plan = D._plan_of(c.n, c.k, c.m, 0, c.dt, torch.device(DEV), c.B)
        self.J, self.r = T(c.J, c.dt), T(c.r, c.dt)
        self.vars = torch.full((c.B, c.V + pad), float("nan"), dtype=c.dt, device=DEV)     # NaN beyond V: never read
        self.vars[:, :c.V] = T(c.v, c.dt)
        self.var = T(c.var, torch.int32) if c.m else None
        self.tang = {key: T(c.t[key], c.dt) for key in KEYS}
        self.keep = []

    def members(self, keys, override=None):
        c, t = self.case, L.BlockTangents()
        src = dict(self.tang, **(override or {}))
        stride = lambda x, per: 0 if (x.shape[0] == 1 and c.B != 1) else per
        for key in keys:
            x = src[key]
            self.keep.append(x)
            if key == "J_blocks":
                t.dJ_blocks, t.dJ_stride = x.data_ptr(), stride(x, c.lay.values)
            elif key == "r":
                t.dr, t.dr_stride = x.data_ptr(), stride(x, c.lay.rows)
            elif key == "lam":
                t.dlambda, t.dlambda_stride = x.data_ptr(), stride(x, 1)
            elif key == "J_eq_blocks":
                t.dJ_eq_blocks, t.dJ_eq_stride = x.data_ptr(), stride(x, c.eq_lay.values)
            elif key == "r_eq":
                t.dr_eq, t.dr_eq_stride = x.data_ptr(), stride(x, c.k)
            elif key == "cons_a":
                t.dcons_a, t.dcons_stride = x.data_ptr(), stride(x, c.m)
            elif key == "cons_b":
                t.dcons_b, t.dcons_stride = x.data_ptr(), stride(x, c.m)
        return t

    def call(self, t, J=True, r=True, plan=None, lay=None, eq_lay="own", r_tensor=None):
        c = self.case
        rho = torch.full((c.B, c.V + self.pad), SENT, dtype=c.dt, device=DEV)
        js = 0 if (self.J.shape[0] == 1 and c.B != 1) else c.lay.values
        rs = 0 if (self.r.shape[0] == 1 and c.B != 1) else c.lay.rows
        r_t = self.r if r_tensor is None else r_tensor
        eq = (c.eq_lay.h if c.eq_lay else None) if isinstance(eq_lay, str) else eq_lay
        rc = L.lib().mo_qp_tangent_rhs_blocks(self.plan if plan is None else plan, (c.lay if lay is None else lay).h, Q._ptr(self.J) if J else None, js,
                                              Q._ptr(r_t) if r else None, rs, eq, Q._ptr(self.var), c.m, c.B, Q._ptr(self.vars), c.V + self.pad,
                                              C.byref(t), Q._ptr(rho), c.V + self.pad, Q._stream())
        torch.cuda.synchronize()
        return rc, rho


@DTYPES
@pytest.mark.parametrize("shared", [False, True], ids=["per-problem", "shared"])
def test_blocks_tangent_strides_null_members_and_determinism(shared, dt):
    """vars_stride and rho_stride beyond V (NaN behind vars, sentinels behind rho left untouched); shared: J_blocks, r and every tangent with
    stride 0.  Every member NULL in turn; dJ_blocks alone equals dJ_blocks with a dr of zeros, to the bit; dr alone does not read r (r is
    NaN there).  Two launches give the same bits."""
    rng = np.random.default_rng(860 + int(shared))
    case = Case(rng, 7, N7_COST, 5, dt, eq_blocks=N7_EQ, m=3, var=(2, 2, 5), shared=shared)
    raw = Raw(case)
    V = case.V
    rc, a = raw.call(raw.members(KEYS))
    rc2, b = raw.call(raw.members(KEYS))
    assert rc == 0 and rc2 == 0 and torch.equal(a, b)                       # two launches, the same bits
    assert torch.all(a[:, V:] == SENT) and torch.all(torch.isfinite(a[:, :V]))
    case.check(a[:, :V], tag="strides all")
    if shared:
        assert not torch.equal(a[0, :V], a[1, :V])                           # shared data, per-problem state
    for leave in KEYS:                                                       # every member NULL in turn
        keys = [key for key in KEYS if key != leave]
        rc, got = raw.call(raw.members(keys))
        assert rc == 0 and torch.all(got[:, V:] == SENT)
        case.check(got[:, :V], keys, tag=f"without {leave}")
    rc, none = raw.call(raw.members(()), J=False, r=False)                    # no tangent at all: rho = 0, the blocks are not needed
    assert rc == 0 and torch.all(none[:, :V] == 0) and torch.all(none[:, V:] == SENT)
    rc, only_dJ = raw.call(raw.members(("J_blocks",)))
    rc2, with_zero_dr = raw.call(raw.members(("J_blocks", "r"), override={"r": torch.zeros_like(raw.tang["r"])}))
    assert rc == 0 and rc2 == 0 and torch.equal(only_dJ, with_zero_dr)
    case.check(only_dJ[:, :V], ("J_blocks",), tag="dJ_blocks alone")
    rc, only_dr = raw.call(raw.members(("r",)), r_tensor=torch.full_like(raw.r, float("nan")))   # r is read only against dJ_blocks
    assert rc == 0 and torch.all(torch.isfinite(only_dr[:, :V]))
    case.check(only_dr[:, :V], ("r",), tag="dr alone")


@DTYPES
def test_blocks_tangent_bad_cons_var(dt):
    """A constraint index outside [0, n): the rho_pi entry of that row is NaN, every other element is finite and what it is without the row's
    dcons_a -- the dense kernel's v = -1 rule.  No fault: the index is never used."""
    rng = np.random.default_rng(870)
    case = Case(rng, 7, N7_COST, 4, dt, eq_blocks=N7_EQ, m=3, var=(2, 2, 5))
    case.var[1, 1] = 7
    case.var[2, 0] = -3
    got = case.device()
    nan = torch.isnan(got).cpu().numpy()
    want = np.zeros_like(nan)
    want[1, case.n + case.m + case.k + 1] = want[2, case.n + case.m + case.k + 0] = True
    assert np.array_equal(nan, want)
    case.check(got, problems=range(4), tag="bad cons_var")


def test_blocks_tangent_error_codes_and_lds_refusal():
    """Every error code of the header with real plans and layouts.  The LDS refusal: n = 8, one block ((0,), R) with the smallest R whose
    vectors (2 n + 2 R values) exceed 64 KiB is MO_ERR_UNSUPPORTED with its own message and rho keeps its sentinels; R - 1 runs."""
    rng = np.random.default_rng(880)
    case = Case(rng, 7, N7_COST, 3, torch.float64, eq_blocks=N7_EQ, m=3, var=(2, 2, 5))
    raw = Raw(case)
    INVALID, DIMENSION, UNSUPPORTED = -1, -2, -3
    untouched = lambda res: res[1].eq(SENT).all().item()
    for keys, kw, word in ((("J_blocks",), dict(J=False), b"J_blocks"), (("r",), dict(r=False), b"J_blocks"),
                           (("J_eq_blocks",), dict(eq_lay=None), b"eq_layout"), (("r_eq",), dict(eq_lay=None), b"eq_layout")):
        res = raw.call(raw.members(keys), **kw)
        assert res[0] == INVALID and word in L.lib().mo_last_error() and untouched(res), (res[0], L.lib().mo_last_error())
    var, raw.var = raw.var, None
    res = raw.call(raw.members(("cons_a",)))
    assert res[0] == INVALID and b"cons_var" in L.lib().mo_last_error() and untouched(res)
    assert raw.call(raw.members(("cons_b",)))[0] == 0                         # dcons_b alone needs no cons_var
    raw.var = var
    t = raw.members(KEYS)
    lib = L.lib().mo_qp_tangent_rhs_blocks
    args = lambda **kw: [kw.get("plan", raw.plan), kw.get("lay", case.lay.h), Q._ptr(raw.J), case.lay.values, Q._ptr(raw.r), case.lay.rows,
                         case.eq_lay.h, Q._ptr(raw.var), case.m, 3, kw.get("vars", Q._ptr(raw.vars)), case.V + raw.pad, kw.get("t", C.byref(t)),
                         kw.get("rho", Q._ptr(raw.vars)), case.V + raw.pad, None]
    for kw in (dict(lay=None), dict(t=None), dict(vars=None), dict(rho=None)):
        assert lib(*args(**kw)) == INVALID, kw
    assert lib(*args(plan=None)) == INVALID and b"plan is NULL" in L.lib().mo_last_error()
    other_n = D._plan_of(8, case.k, case.m, 0, torch.float64, torch.device(DEV), 3)
    res = raw.call(t, plan=other_n)
    assert res[0] == DIMENSION and b"n = 7" in L.lib().mo_last_error() and untouched(res)          # the layout's n differs from the plan's
    other_k = D._plan_of(7, case.k + 1, case.m, 0, torch.float64, torch.device(DEV), 3)
    res = raw.call(t, plan=other_k)
    assert res[0] == DIMENSION and b"eq_layout" in L.lib().mo_last_error() and untouched(res)      # eq_layout's rows differ from the plan's k
    eq8 = Q.ResidualLayout(8, [((0, 1), 2)])
    res = raw.call(t, eq_lay=eq8.h)
    assert res[0] == DIMENSION and untouched(res)                                                    # eq_layout's n differs from the plan's
    # with k = 0 the equality members and eq_layout, with m = 0 the inequality members are ignored
    # (the members and cons_var point at a NaN buffer too short for any of them: they are not read)
    plain = Case(rng, 7, N7_COST, 3, torch.float64)
    praw = Raw(plain)
    poison = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
    tj = praw.members(("J_blocks", "r", "lam"))
    tj.dJ_eq_blocks = tj.dr_eq = tj.dcons_a = tj.dcons_b = poison.data_ptr()
    praw.var = poison
    rc, got = praw.call(tj, eq_lay=case.eq_lay.h)
    assert rc == 0, L.lib().mo_last_error()
    plain.check(got[:, :plain.V], ("J_blocks", "r", "lam"), tag="k = m = 0")
    # the LDS refusal
    n = 8
    lds = lambda rows: (2 * n + 2 * rows) * 8
    rows = next(q for q in range(1, 1 << 16) if lds(q) > 64 * 1024)
    for R_, refused in ((rows, True), (rows - 1, False)):
        big = Case(rng, n, [((0,), R_)], 1, torch.float64)
        braw = Raw(big)
        rc, rho = braw.call(braw.members(("J_blocks", "r", "lam")))
        if refused:
            msg = L.lib().mo_last_error()
            assert rc == UNSUPPORTED and f"{R_} residual rows".encode() in msg and b"block tangent" in msg, (rc, msg)
            assert torch.all(rho == SENT)
        else:
            assert rc == 0 and torch.all(rho[:, big.V:] == SENT)
            big.check(rho[:, :big.V], ("J_blocks", "r", "lam"), tag="largest that fits")


def test_first_block_tangent_allocates_nothing():
    n, B, k = 64, 96, 3
    rng = np.random.default_rng(890)
    blocks = [(tuple(int(i) for i in rng.permutation(n)[:4]), 2) for _ in range(96)]
    eq_blocks = [((0, 5, 9), 1), ((7, 3), 2)]
    case = Case(rng, n, blocks, B, torch.float64, eq_blocks=eq_blocks)
    V = case.V
    J_d, r_d, v_d = T(case.J), T(case.r), T(case.v)
    tang = {key: T(case.t[key]) for key in case.keys()}
    lays = [case.lay, Q.ResidualLayout(n, blocks)]
    eqs = [case.eq_lay, Q.ResidualLayout(n, eq_blocks)]
    desc = L.PlanDesc(n, k, 0, 0, L.MO_F64, 0, L.EXTRA_PLAN_FLAGS, 0, B)
    plans = [C.c_void_p(), C.c_void_p()]
    for pl in plans:
        L.check(L.lib().mo_plan_create(C.byref(desc), C.byref(pl)))
    rho = torch.empty(B, V, dtype=torch.float64, device=DEV)
    t = L.BlockTangents()
    t.dJ_blocks, t.dJ_stride, t.dr, t.dr_stride = tang["J_blocks"].data_ptr(), lays[0].values, tang["r"].data_ptr(), lays[0].rows
    t.dlambda, t.dlambda_stride = tang["lam"].data_ptr(), 1
    t.dJ_eq_blocks, t.dJ_eq_stride, t.dr_eq, t.dr_eq_stride = tang["J_eq_blocks"].data_ptr(), eqs[0].values, tang["r_eq"].data_ptr(), k

    def launch(i):
        L.check(L.lib().mo_qp_tangent_rhs_blocks(plans[i], lays[i].h, Q._ptr(J_d), lays[i].values, Q._ptr(r_d), lays[i].rows, eqs[i].h, None, 0, B,
                                                 Q._ptr(v_d), V, C.byref(t), Q._ptr(rho), V, Q._stream()))
        torch.cuda.synchronize()

    try:
        launch(0)                                           # module load and kernel code happen on the twin first
        free0 = torch.cuda.mem_get_info()[0]
        launch(1)                                           # the FIRST launch on this plan and these layouts
        assert torch.cuda.mem_get_info()[0] >= free0 - (1 << 20), (free0, torch.cuda.mem_get_info()[0])
        case.check(rho, tag="first launch")
    finally:
        for pl in plans:
            L.lib().mo_plan_destroy(pl)


# ---- 5. torch.autograd.forward_ad through solve_qp(layout=...) --------------------------------------------------------------------------------
def autograd_problem(n, case, rng, B):
    blocks = autograd_layout(n, rng)
    eq_blocks = [(tuple(int(i) for i in rng.permutation(n)[:3]), 1), ((1, 6, 1), 2)] if case == "equalities" else []
    m = 4 if case == "bounds" else 0
    c = Case(rng, n, blocks, B, torch.float64, eq_blocks=eq_blocks, m=m)
    c.J, c.r = rng.uniform(-1, 1, c.J.shape), rng.uniform(-1, 1, c.r.shape)
    c.Jeq, c.req = rng.uniform(-1, 1, (B, c.eq_lay.values if c.k else 0)), rng.uniform(-0.5, 0.5, (B, c.k))
    c.var = np.stack([rng.permutation(n)[:m] for _ in range(B)]).astype(np.int32)
    c.a, c.b = rng.choice([-1.0, 1.0], (B, m)), rng.uniform(5.0, 6.0, (B, m))       # loose: |x| stays far below 5
    return c


def solve_blocks(c, dual, requires_grad=False, var=None):
    """solve_qp(layout=...) on the case's data: dual=True wraps every floating-point input in a dual tensor carrying the case's tangents."""
    prim = dict(J_blocks=T(c.J), r=T(c.r), lam=torch.full((c.B,), LAM, dtype=torch.float64, device=DEV))
    if c.k:
        prim.update(J_eq_blocks=T(c.Jeq), r_eq=T(c.req))
    if c.m:
        prim.update(cons_a=T(c.a), cons_b=T(c.b))
    if requires_grad:
        for t in prim.values():
            t.requires_grad_(True)
    inp = {key: fwAD.make_dual(t, T(c.t[key])) for key, t in prim.items()} if dual else dict(prim)
    kw = {}
    if c.k:
        kw.update(eq_layout=c.eq_lay, J_eq_blocks=inp["J_eq_blocks"], r_eq=inp["r_eq"])
    if c.m:
        kw.update(cons_var=T(c.var if var is None else var, torch.int32), cons_a=inp["cons_a"], cons_b=inp["cons_b"])
    res = D.solve_qp(layout=c.lay, J_blocks=inp["J_blocks"], r=inp["r"], lam=inp["lam"], params=Q.Params(**PARAMS), return_all=True,
                     return_status=True, **kw)
    return prim, res


@pytest.mark.parametrize("case", ["unconstrained", "equalities", "bounds"])
@pytest.mark.parametrize("n", [8, 64])
def test_forward_ad_through_residual_blocks(n, case):
    """The tangent of [x | s | y | z] through solve_qp(layout=...) along a direction in every packed input at once, against
    tangent_reference.vdot (LU on the full K of the restated linearisation) fed with the block restatement's rho, both AT THE DEVICE'S OWN v.
    Bound max(1e-10, 10 D) as test_autograd_through_residual_blocks derives it: D is measured on the CPU, without the code under test, at the
    ORACLE's Solve output of the same problems -- the largest rel-inf between vdot from LU on the full K and vdot from the reduced system
    the kernels factorise (the conditioning of K at the returned point times the unit round-off); printed by every run.  Then, in the same
    run, g . vdot against sum <.grad, tangent> of .backward() for a random g on x and y, by Hoelder on the same bound."""
    rng = np.random.default_rng(900 + n + len(case))
    B = 6
    c = autograd_problem(n, case, rng, B)
    k, m = c.k, c.m
    with fwAD.dual_level():
        _, res = solve_blocks(c, dual=True)
        assert torch.all(res[4] == 0)
        st = D.tangent_status(res[0])
        assert st is not None and st.shape == (B,) and st.dtype == torch.int32 and torch.all(st == 0)
        v = torch.cat([fwAD.unpack_dual(t).primal for t in res[:4]], dim=1).cpu().numpy()
        vdot = torch.cat([fwAD.unpack_dual(t).tangent for t in res[:4]], dim=1).cpu().numpy()
    c.v = v
    D_cpu, worst = 0.0, 0.0
    for p in range(B):
        Js, rs = BR.unpack(c.J[p], c.blocks), BR.split_rows(c.r[p], c.blocks)
        G = BR.symmetric(BR.linearize(n, c.blocks, Js, rs, LAM)[0])
        cc = BR.linearize(n, c.blocks, Js, rs, LAM)[1]
        A = BR.jacobian(n, c.eq_blocks, BR.unpack(c.Jeq[p], c.eq_blocks)) if k else np.zeros((0, n))
        tang = c.ref_tangents(p, KEYS)
        rho_at = lambda vv: BT.rho(n, k, m, c.blocks, Js, rs, vv, tang, eq_blocks=c.eq_blocks, var=c.var[p])
        o = orc.Solver(orc.QP(G=np.tril(G), c=cc, A_eq=A if k else None, b_eq=c.req[p] if k else None, cons_var=c.var[p], cons_a=c.a[p], cons_b=c.b[p]))
        o.solve(**PARAMS)
        vo = np.array(o.variables)
        lu, red = TR.vdot(G, A, c.var[p], c.a[p], vo, rho_at(vo)), TR.vdot_reduced(G, A, c.var[p], c.a[p], vo, rho_at(vo))
        D_cpu = max(D_cpu, float(rel_inf_rows(red[None], lu[None])[0]))
        ref = TR.vdot(G, A, c.var[p], c.a[p], v[p], rho_at(v[p]))
        worst = max(worst, float(rel_inf_rows(vdot[p][None], ref[None])[0]))
    bound = max(1e-10, 10 * D_cpu)
    print(f"blocks forward_ad n = {n} {case}: D = {D_cpu:.3e}, bound {bound:.3e}, worst rel-inf of vdot {worst:.3e}")
    assert worst < bound, (worst, bound)
    # the backward of the same problems
    prim, res = solve_blocks(c, dual=False, requires_grad=True)
    g = rng.normal(size=(B, c.V))
    g[:, n:n + m] = 0.0
    g[:, n + m + k:] = 0.0
    vfull = torch.cat(res[:4], dim=1)
    (vfull * T(g)).sum().backward()
    lhs = np.sum(g * vdot, axis=1)
    rhs = np.zeros(B)
    hold = np.sum(np.abs(g), axis=1) * np.max(np.abs(vdot), axis=1)
    for key, t in prim.items():
        gr, td = t.grad.cpu().numpy().reshape(B, -1), c.t[key].reshape(B, -1)
        rhs += np.sum(gr * td, axis=1)
        hold += np.max(np.abs(gr), axis=1) * np.sum(np.abs(td), axis=1)
    print(f"blocks forward_ad n = {n} {case}: max |g . vdot - sum <grad, tangent>| / Hoelder = {np.max(np.abs(lhs - rhs) / hold):.3e}")
    assert np.all(np.abs(lhs - rhs) <= bound * hold), (lhs, rhs)


def test_forward_ad_blocks_failing_problem_gets_a_zero_tangent():
    """One problem whose forward fails on purpose (a constraint index outside [0, n): MO_STATUS_BAD_INDEX) inside a healthy batch: its
    tangent rows are zero, its neighbours are to the bit what they are without it, and tangent_status tells which problem it was.  A
    tangent on lam counts only where lam > 0: with lam = 0 the lam direction changes nothing."""
    n, B = 8, 6
    rng = np.random.default_rng(910)
    c = autograd_problem(n, "bounds", rng, B)
    out = []
    for broken in (False, True):
        var = c.var.copy()
        if broken:
            var[3, 1] = n + 1
        with fwAD.dual_level():
            _, res = solve_blocks(c, dual=True, var=var)
            vdot = torch.cat([fwAD.unpack_dual(t).tangent for t in res[:4]], dim=1).clone()
            out.append((vdot, res[4].cpu().numpy(), D.tangent_status(res[0]).cpu().numpy()))
    (t_ok, st_ok, ts_ok), (t_bad, st_bad, ts_bad) = out
    assert np.all(st_ok == 0) and np.all(ts_ok == 0)
    assert st_bad[3] == L.MO_STATUS_BAD_INDEX and ts_bad[3] != 0, (st_bad, ts_bad)
    others = [0, 1, 2, 4, 5]
    assert np.all(st_bad[others] == 0) and np.all(ts_bad[others] == 0)
    assert torch.all(t_bad[3] == 0) and torch.all(torch.isfinite(t_bad))
    assert torch.equal(t_bad[others], t_ok[others]) and torch.any(t_ok[3] != 0)
    # lam = 0 is not added (nonlinear.cc:187-189), so its tangent is masked as its gradient is
    lay = c.lay
    Jb, r = T(c.J), T(c.r)
    zero = torch.zeros(B, dtype=torch.float64, device=DEV)
    with fwAD.dual_level():
        x1 = D.solve_qp(layout=lay, J_blocks=fwAD.make_dual(Jb, T(c.t["J_blocks"])), r=r, lam=fwAD.make_dual(zero, T(c.t["lam"])), params=Q.Params(**PARAMS))
        x2 = D.solve_qp(layout=lay, J_blocks=fwAD.make_dual(Jb, T(c.t["J_blocks"])), r=r, lam=0.0, params=Q.Params(**PARAMS))
        assert torch.equal(fwAD.unpack_dual(x1).tangent, fwAD.unpack_dual(x2).tangent)
