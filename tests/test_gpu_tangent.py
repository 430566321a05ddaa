"""GPU tests of the forward-mode sensitivities of a QP solve (run with -m gpu on an MI355X): mo_qp_tangent_rhs against the numpy restatement
(tests/tangent_reference.py), qp_jvp against LU on the full K, the adjoint identity against mo_qp_gradients on the device, and
torch.autograd.forward_ad through solve_qp.  Bounds: TOL64 / TOL32 of tests/test_gpu_diff.py, as rel-inf per problem."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

from mini_opt_amd import _lib as L
from mini_opt_amd import diff as D
from mini_opt_amd import qp as Q
from tests import diff_reference as R
from tests import tangent_reference as TR
from tests.sens_fixtures import ACTIVE_SEED, PARAMS, T, active_set_problems, dev, device_problem, host_batch, padded, rel_inf_rows

pytestmark = pytest.mark.gpu
TOL64 = 1e-10
TOL32 = 2e-3
# (n, k, m, m_r): nothing but the cost, odd everything | odd m, a box (two rows on one variable) | fp32 tail of a 4-vector | odd n beyond one
# tile, a box on every variable | aligned 16-byte path, the solve runs the fused RHS twin | the solve runs the LARGE path
SHAPES = [(5, 0, 0, 7), (8, 2, 5, 12), (7, 3, 4, 9), (33, 3, 66, 35), (64, 8, 32, 128), (96, 40, 20, 128)]
SID = lambda s: f"n{s[0]}k{s[1]}m{s[2]}r{s[3]}"
DTYPES = [torch.float64, torch.float32]
DID = lambda dt: "f64" if dt == torch.float64 else "f32"


def directions(hb, seed, f32=False, shared=False):
    """One direction in every member, mathematical orientation ("A" [B, k, n], "G" [B, n, n] NOT symmetric); shared: one for the batch."""
    rng = np.random.default_rng(seed)
    B = 1 if shared else hb.vars.shape[0]
    n, k, m, m_r = hb.n, hb.k, hb.m, hb.J.shape[1]
    d = dict(G=rng.normal(size=(B, n, n)), c=rng.normal(size=(B, n)), J=rng.normal(size=(B, m_r, n)), r=rng.normal(size=(B, m_r)),
             lam=rng.normal(size=B), A=rng.normal(size=(B, k, n)), b_eq=rng.normal(size=(B, k)), a=rng.normal(size=(B, m)),
             b=rng.normal(size=(B, m)))
    if f32:
        d = {key: val.astype(np.float32).astype(np.float64) for key, val in d.items()}
    return d


def level_keys(hb, level):
    keys = ["G", "c"] if level == "G" else ["J", "r", "lam"]
    return keys + (["A", "b_eq"] if hb.k else []) + (["a", "b"] if hb.m else [])


NAMES = dict(G="G", c="c", J="J", r="r", lam="lam", A="A_eq", b_eq="b_eq", a="cons_a", b="cons_b")   # reference key -> GRADIENTS key


def device_tangents(d, keys, dt, J_layout="row", dJ_ld=None):
    """The dict qp_tangent_rhs takes, in BatchedQP's layouts."""
    out = {}
    for key in keys:
        val = d[key]
        if key in ("G", "A"):
            val = val.transpose(0, 2, 1)            # memory = column-major
        elif key == "J":
            val = padded(val.transpose(0, 2, 1), dJ_ld or val.shape[1]) if J_layout == "col" else padded(val, dJ_ld or val.shape[2])
        out[NAMES[key]] = T(val, dt)
    return out


def reference_rho(hb, d, keys, level):
    B = hb.vars.shape[0]
    pick = lambda val, p: val[p if val.shape[0] > 1 else 0]
    return np.stack([TR.rho(hb.n, hb.k, hb.m, hb.cons_var[p], hb.vars[p], {key: pick(d[key], p) for key in keys},
                            J=hb.J[p] if level == "J" else None, r=hb.r[p] if level == "J" else None) for p in range(B)])


def reference_vdot(hb, rho):
    n, k = hb.n, hb.k
    return np.stack([TR.vdot(hb.G[p], hb.A_eq[p].T if k else np.zeros((0, n)), hb.cons_var[p], hb.cons_a[p], hb.vars[p], rho[p])
                     for p in range(rho.shape[0])])


def blocks(hb):
    n, k, m = hb.n, hb.k, hb.m
    return dict(d=slice(0, n), comp=slice(n, n + m), pe=slice(n + m, n + m + k), pi=slice(n + m + k, n + 2 * m + k))


def check_rho(got, ref, hb, tol, tag):
    for name, sl in blocks(hb).items():
        if sl.start == sl.stop:
            continue
        if name == "comp":
            assert np.all(got[:, sl] == 0), (tag, name)
            continue
        err = rel_inf_rows(got[:, sl], ref[:, sl]).max()
        assert err < tol, (tag, name, err)


# ---- 1. rho against the numpy restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DID)
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_rho_against_the_numpy_restatement(shape, dt):
    n, k, m, m_r = shape
    f32 = dt == torch.float32
    tol = TOL32 if f32 else TOL64
    B = 6
    hb = host_batch(n, k, m, m_r, B, stream=51, f32=f32)
    d = directions(hb, 21, f32)
    v = T(hb.vars, dt)
    keys = level_keys(hb, "G")
    got = D.qp_tangent_rhs(device_problem(hb, "G", dt), v, device_tangents(d, keys, dt))
    check_rho(got.double().cpu().numpy(), reference_rho(hb, d, keys, "G"), hb, tol, "G-level")
    # J-level: both layouts, packed and with padded leading dimensions; the paddings of J and of its tangent differ
    keys = level_keys(hb, "J")
    ref = reference_rho(hb, d, keys, "J")
    for layout, ld, dld in (("row", None, None), ("row", n + 3, n + 4), ("row", n + 4, None), ("col", None, None), ("col", m_r + 5, m_r + 4),
                            ("col", None, m_r + 1)):
        prob = device_problem(hb, "J", dt, J_layout=layout, J_ld=ld)
        got = D.qp_tangent_rhs(prob, v, device_tangents(d, keys, dt, J_layout=layout, dJ_ld=dld))
        check_rho(got.double().cpu().numpy(), ref, hb, tol, (layout, ld, dld))


# ---- the C ABI with padded members ---------------------------------------------------------------------------------------------------------
class Raw:
    """mo_qp_tangent_rhs through ctypes with padded leading dimensions and strides for every member and for rho."""
    CANARY = -777.25

    def __init__(self, hb, level, dt=torch.float64, J_layout="row"):
        self.hb, self.level, self.dt, self.J_layout = hb, level, dt, J_layout
        self.prob = device_problem(hb, level, dt, J_layout=J_layout)
        self.B = hb.vars.shape[0]
        self.plan = D.plan_for(self.prob, self.B)
        self.ps = self.prob.as_struct()
        self.v = T(hb.vars, dt)
        self.V = hb.vars.shape[1]
        self.keep = []

    def matrix(self, a, ld, extra, fill):
        """[B, vectors, length] -> [B, vectors * ld + extra] with `fill` in every padding element."""
        B, vectors, _ = a.shape
        flat = np.full((B, vectors * ld + extra), fill)
        flat[:, :vectors * ld] = padded(a, ld, fill).reshape(B, -1)
        t = T(flat, self.dt)
        self.keep.append(t)
        return t, (0 if B == 1 and self.B > 1 else vectors * ld + extra)

    def vector(self, a, extra):
        a = a.reshape(a.shape[0], -1)
        B, length = a.shape
        flat = np.full((B, length + extra), np.nan)
        flat[:, :length] = a
        t = T(flat, self.dt)
        self.keep.append(t)
        return t, (0 if B == 1 and self.B > 1 else length + extra)

    def members(self, d, keys, pad=1, fill=np.nan, poison_upper=False):
        """An mo_qp_tangents over padded buffers: every leading dimension `pad` beyond the matrix, every stride beyond its member."""
        hb, t = self.hb, L.QPTangents()
        n, k, m_r = hb.n, hb.k, hb.J.shape[1]
        for key in keys:
            val = d[key]
            if key == "G":
                g = val.transpose(0, 2, 1).copy()                         # [B, column, row]
                if poison_upper:
                    g[:, np.triu(np.ones((n, n), dtype=bool), 1).T] = np.nan   # row < column
                buf, t.dG_stride = self.matrix(g, n + pad, 3 * pad, fill)
                t.dG, t.dG_ld = buf.data_ptr(), n + pad
            elif key == "A":
                buf, t.dA_stride = self.matrix(val.transpose(0, 2, 1), k + pad, 5 * pad, fill)
                t.dA_eq, t.dA_ld = buf.data_ptr(), k + pad
            elif key == "J":
                if self.J_layout == "col":
                    buf, t.dJ_stride = self.matrix(val.transpose(0, 2, 1), m_r + pad, 2 * pad, fill)
                    t.dJ_ld = m_r + pad
                else:
                    buf, t.dJ_stride = self.matrix(val, n + pad, 2 * pad, fill)
                    t.dJ_ld = n + pad
                t.dJ = buf.data_ptr()
            elif key in ("a", "b"):
                continue
            else:
                buf, stride = self.vector(val, pad)
                setattr(t, {"c": "dc", "b_eq": "db_eq", "r": "dr", "lam": "dlambda"}[key], buf.data_ptr())
                setattr(t, {"c": "dc_stride", "b_eq": "db_stride", "r": "dr_stride", "lam": "dlambda_stride"}[key], stride)
        for key, field in (("a", "dcons_a"), ("b", "dcons_b")):           # the two share one stride
            if key in keys:
                buf, t.dcons_stride = self.vector(d[key], pad)
                setattr(t, field, buf.data_ptr())
        return t

    def call(self, t, rho_pad=3):
        rho = torch.full((self.B, self.V + rho_pad), self.CANARY, dtype=self.dt, device=dev())
        rc = L.lib().mo_qp_tangent_rhs(self.plan, C.byref(self.ps), self.B, Q._ptr(self.v), self.V, C.byref(t), Q._ptr(rho), self.V + rho_pad,
                                       Q._stream())
        torch.cuda.synchronize()
        return rc, rho

    def launch(self, t, rho_pad=3):
        rc, rho = self.call(t, rho_pad)
        L.check(rc)
        assert torch.all(rho[:, self.V:] == self.CANARY)                  # nothing beyond V
        return rho[:, :self.V].contiguous()


# ---- 2. poison -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DID)
@pytest.mark.parametrize("shape", [(8, 2, 5, 12), (7, 3, 4, 9), (33, 3, 66, 35), (64, 8, 32, 128)], ids=SID)
def test_poison_in_the_upper_triangle_and_the_padding_never_reaches_rho(shape, dt):
    """NaN in the strict upper triangle of dG and in every padding row or column of dJ, dA_eq and dG (and between the problems): rho is
    finite and to the bit what the same buffers give with zeros there.  The padding of 4 keeps the 16-byte path on the aligned shapes."""
    n, k, m, m_r = shape
    f32 = dt == torch.float32
    hb = host_batch(n, k, m, m_r, 6, stream=52, f32=f32)
    d = directions(hb, 22, f32)
    for level, layout in (("G", "row"), ("J", "row"), ("J", "col")):
        raw = Raw(hb, level, dt, J_layout=layout)
        keys = level_keys(hb, level)
        for pad in (4, 1):
            clean = raw.launch(raw.members(d, keys, pad=pad, fill=0.0, poison_upper=False))
            dirty = raw.launch(raw.members(d, keys, pad=pad, fill=np.nan, poison_upper=True))
            assert torch.all(torch.isfinite(dirty)), (level, layout, pad)
            assert torch.equal(clean, dirty), (level, layout, pad)
            check_rho(dirty.double().cpu().numpy(), reference_rho(hb, d, keys, level), hb, TOL32 if f32 else TOL64, (level, layout, pad))


# ---- 3. through the C ABI ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level,layout", [("G", "row"), ("J", "row"), ("J", "col")], ids=["G", "Jrow", "Jcol"])
def test_c_abi_strides_shared_directions_null_members(level, layout):
    n, k, m, m_r, B = 8, 2, 5, 12, 7
    hb = host_batch(n, k, m, m_r, B, stream=53)
    raw = Raw(hb, level, J_layout=layout)
    keys = level_keys(hb, level)
    d = directions(hb, 23)
    # padded strides for every member and for rho (launch() checks the canary beyond V); two launches give the same bits
    t = raw.members(d, keys, pad=3)
    rho = raw.launch(t)
    check_rho(rho.cpu().numpy(), reference_rho(hb, d, keys, level), hb, TOL64, "all members")
    assert torch.equal(rho, raw.launch(t))
    # stride 0 = one direction shared by the batch: to the bit the expanded copy
    ds = directions(hb, 24, shared=True)
    de = {key: np.repeat(val, B, axis=0) for key, val in ds.items()}
    assert all(getattr(raw.members(ds, keys), f) == 0 for f in ("dc_stride" if level == "G" else "dr_stride", "dA_stride", "dcons_stride"))
    assert torch.equal(raw.launch(raw.members(ds, keys)), raw.launch(raw.members(de, keys)))
    # all members NULL: exactly zero
    assert torch.all(raw.launch(L.QPTangents()) == 0)
    # each single member alone
    for key in keys:
        got = raw.launch(raw.members(d, [key], pad=2)).cpu().numpy()
        ref = reference_rho(hb, d, [key], level)
        scale = np.max(np.abs(ref), axis=1)
        assert np.all(scale > 0) and np.all(np.max(np.abs(got - ref), axis=1) <= TOL64 * scale), key
        for name, sl in blocks(hb).items():               # a block no member feeds is exactly zero
            if not np.any(ref[:, sl]):
                assert np.all(got[:, sl] == 0), (key, name)
    # the documented refusals, with a real plan
    other = ["J"] if level == "G" else ["G"]
    rc, rho = raw.call(raw.members(d, other))
    assert rc == -1 and torch.all(rho == Raw.CANARY)
    for field, low in (("dG_ld", n - 1), ("dA_ld", k - 1), ("dJ_ld", (n if layout == "row" else m_r) - 1)):
        t = raw.members(d, keys)
        if (field == "dG_ld") != (level == "G") and field != "dA_ld":
            continue
        setattr(t, field, low)
        rc, rho = raw.call(t)
        assert rc == -2 and field.encode() in L.lib().mo_last_error() and torch.all(rho == Raw.CANARY), field


# ---- 4. qp_jvp against LU on the full K --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level,dt", [("J", torch.float64), ("G", torch.float64), ("J", torch.float32)], ids=["J-f64", "G-f64", "J-f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_qp_jvp_against_lu_on_the_full_kkt_matrix(shape, level, dt):
    n, k, m, m_r = shape
    f32 = dt == torch.float32
    B = 12
    hb = host_batch(n, k, m, m_r, B, stream=54, f32=f32)
    d = directions(hb, 25, f32)
    keys = level_keys(hb, level)
    prob = device_problem(hb, level, dt)
    if not f32 and shape == (64, 8, 32, 128):
        assert D.kkt_solve_kernel(prob, B).startswith("fused_rhs_"), D.kkt_solve_kernel(prob, B)
    if shape == (96, 40, 20, 128):
        assert D.kkt_solve_kernel(prob, B) == "generic"
    vdot, status = D.qp_jvp(prob, T(hb.vars, dt), device_tangents(d, keys, dt))
    assert torch.all(status == 0)
    ref = reference_vdot(hb, reference_rho(hb, d, keys, level))
    err = rel_inf_rows(vdot.double().cpu().numpy(), ref)
    print(f"qp_jvp vs LU {shape} {level} {DID(dt)}: kernel {D.kkt_solve_kernel(prob, B)}, max rel-inf {err.max():.3e}")
    assert err.max() < (TOL32 if f32 else TOL64)


# ---- 5. the adjoint identity on the device -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", ["J", "G"])
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_device_adjoint_identity(shape, level):
    """g . qp_jvp(thetadot) against sum <qp_gradients(kkt_solve(g, transpose=True)), thetadot>.  Bound: TOL64 (|g|_1 |vdot|_inf +
    sum_theta |grad_theta|_inf |thetadot|_1) -- Hoelder on the rel-inf bounds the two sides are already held to."""
    n, k, m, m_r = shape
    B = 8
    hb = host_batch(n, k, m, m_r, B, stream=55)
    d = directions(hb, 26)
    d["G"] = 0.5 * (d["G"] + d["G"].transpose(0, 2, 1))      # the gradient is the one for a symmetric G
    keys = level_keys(hb, level)
    prob = device_problem(hb, level)
    v = T(hb.vars)
    g = np.random.default_rng(27).normal(size=hb.vars.shape)
    tang = device_tangents(d, keys, torch.float64)
    vdot, st = D.qp_jvp(prob, v, tang)
    u, st_u = D.kkt_solve(prob, v, T(g), transpose=True)
    assert torch.all(st == 0) and torch.all(st_u == 0)
    grads = D.qp_gradients(prob, v, u)
    assert set(grads) == set(tang)
    vd = vdot.cpu().numpy()
    lhs = np.sum(g * vd, axis=1)
    rhs = np.zeros(B)
    bound = np.sum(np.abs(g), axis=1) * np.max(np.abs(vd), axis=1)
    for key in tang:
        gr, td = grads[key].cpu().numpy().reshape(B, -1), tang[key].cpu().numpy().reshape(B, -1)
        rhs += np.sum(gr * td, axis=1)
        bound += np.max(np.abs(gr), axis=1) * np.sum(np.abs(td), axis=1)
    print(f"adjoint identity {shape} {level}: max |lhs - rhs| / bound = {np.max(np.abs(lhs - rhs) / bound):.3e} (of TOL64 = {TOL64})")
    assert np.all(np.abs(lhs - rhs) <= TOL64 * bound), (lhs, rhs)


# ---- 6. torch.autograd.forward_ad through solve_qp -----------------------------------------------------------------------------------------
def params():
    return Q.Params(**PARAMS)


def test_forward_ad_unconstrained_against_torch_linalg_solve():
    """(a) m = 0, k = 0, G = M M^T / n + I: the tangent of x along (Mdot, cdot) through solve_qp against forward AD through
    torch.linalg.solve(G, -c), TOL64."""
    n, B = 8, 16
    gen = torch.Generator(device="cpu").manual_seed(15)
    rnd = lambda *s: (torch.rand(*s, generator=gen, dtype=torch.float64) * 2 - 1).to(dev())
    M0, c0, dM, dc = rnd(B, n, n), rnd(B, n), rnd(B, n, n), rnd(B, n)
    out = []
    for which in ("device", "torch"):
        with fwAD.dual_level():
            M, c = fwAD.make_dual(M0, dM), fwAD.make_dual(c0, dc)
            G = M @ M.transpose(1, 2) / n + torch.eye(n, dtype=torch.float64, device=dev())
            x = D.solve_qp(G=G, c=c, params=params()) if which == "device" else torch.linalg.solve(G, -c.unsqueeze(-1)).squeeze(-1)
            if which == "device":
                assert torch.all(D.tangent_status(x) == 0)
            px, tx = fwAD.unpack_dual(x)
            out.append((px.clone(), tx.clone()))
    for i, tag in ((0, "x"), (1, "xdot")):
        err = rel_inf_rows(out[0][i].cpu().numpy(), out[1][i].cpu().numpy())
        print(f"forward_ad unconstrained {tag}: {err.max():.3e}")
        assert err.max() < TOL64, tag


def test_forward_ad_equality_only_against_the_dense_kkt_solve_in_torch():
    """(b) (12, 3, 0): the tangent of x along a direction in M (G = M M^T / n + I), c, A_eq, b_eq against forward AD through the dense KKT
    solve [[G, A^T], [A, 0]] [x; nu] = [-c; -b_eq] in torch, TOL64."""
    n, k, B = 12, 3, 16
    gen = torch.Generator(device="cpu").manual_seed(16)
    rnd = lambda *s: (torch.rand(*s, generator=gen, dtype=torch.float64) * 2 - 1).to(dev())
    prim = [rnd(B, n, n), rnd(B, n), rnd(B, k, n), rnd(B, k)]
    tang = [rnd(B, n, n), rnd(B, n), rnd(B, k, n), rnd(B, k)]
    out = []
    for which in ("device", "torch"):
        with fwAD.dual_level():
            M, c, A, b = (fwAD.make_dual(p, t) for p, t in zip(prim, tang))
            G = M @ M.transpose(1, 2) / n + torch.eye(n, dtype=torch.float64, device=dev())
            if which == "device":
                x = D.solve_qp(G=G, c=c, A_eq=A, b_eq=b, params=params())
            else:
                Kd = torch.cat([torch.cat([G, A.transpose(1, 2)], dim=2), torch.cat([A, torch.zeros(B, k, k, dtype=torch.float64, device=dev())], dim=2)], dim=1)
                x = torch.linalg.solve(Kd, -torch.cat([c, b], dim=1).unsqueeze(-1)).squeeze(-1)[:, :n]
            px, tx = fwAD.unpack_dual(x)
            out.append((px.clone(), tx.clone()))
    for i, tag in ((0, "x"), (1, "xdot")):
        err = rel_inf_rows(out[0][i].cpu().numpy(), out[1][i].cpu().numpy())
        print(f"forward_ad equality-only {tag}: {err.max():.3e}")
        assert err.max() < TOL64, tag


def test_forward_ad_with_active_inequalities():
    """(c) The device tangent of the whole [x | s | y | z] against tests/tangent_reference.py evaluated AT THE DEVICE'S OWN v (LU on the full
    K), on the active-set problems of test_gpu_diff.py (seed 2024, 25 problems for each m = 1 ... 8), along one seeded direction in G (not
    symmetric: solve_qp passes 1/2 (Gdot + Gdot^T)), c, a and b at once.

    The bound is max(TOL64, 10 D).  D is measured on the CPU without the code under test and printed by every run: at the ORACLE's Solve
    output of the same problems, the largest rel-inf between vdot from LU on the full K and vdot from the reduced system
    H = G + C^T S^-1 Z C in numpy; the factor 10 covers an unpivoted LDL^T against a pivoted LU, as in test_gpu_diff.py.  No problem is
    excused; at least half of the problems must have an active row (s < 1e-6).  Measured: D = 2.6e-5 (a direction that moves a and b
    makes rho_pi non-zero, and at a slack of 1e-11 the two factorisations agree no better), 150 of 200 problems with an active row, the
    device's worst rel-inf of vdot 1.4e-5."""
    from oracle import oracle as orc
    groups = active_set_problems()
    n = 8
    rng = np.random.default_rng(28)
    D_cpu, active, total, worst = 0.0, 0, 0, 0.0
    for grp in groups:
        m, cnt = grp["m"], grp["G"].shape[0]
        d = dict(G=rng.normal(size=(cnt, n, n)), c=rng.normal(size=(cnt, n)), a=rng.normal(size=(cnt, m)), b=rng.normal(size=(cnt, m)))
        dsym = dict(d, G=0.5 * (d["G"] + d["G"].transpose(0, 2, 1)))
        none = np.zeros((0, n))
        # the CPU measurement of D at the oracle's optimum
        for p in range(cnt):
            o = orc.Solver(orc.QP(G=np.tril(grp["G"][p]), c=grp["c"][p], cons_var=grp["var"][p], cons_a=grp["a"][p], cons_b=grp["b"][p]))
            o.solve(**PARAMS)
            vo = np.array(o.variables)
            rho = TR.rho(n, 0, m, grp["var"][p], vo, {key: val[p] for key, val in dsym.items()})
            lu = TR.vdot(grp["G"][p], none, grp["var"][p], grp["a"][p], vo, rho)
            red = TR.vdot_reduced(grp["G"][p], none, grp["var"][p], grp["a"][p], vo, rho)
            D_cpu = max(D_cpu, float(rel_inf_rows(red[None], lu[None])[0]))
        # the device
        with fwAD.dual_level():
            G, c, a, b = (fwAD.make_dual(T(grp[key]), T(d[key])) for key in ("G", "c", "a", "b"))
            res = D.solve_qp(G=G, c=c, cons_var=T(grp["var"], torch.int32), cons_a=a, cons_b=b, params=params(), return_all=True,
                             return_status=True)
            assert torch.all(res[4] == 0) and torch.all(D.tangent_status(res[0]) == 0)
            v = torch.cat([fwAD.unpack_dual(t).primal for t in res[:4]], dim=1).cpu().numpy()
            vdot = torch.cat([fwAD.unpack_dual(t).tangent for t in res[:4]], dim=1).cpu().numpy()
        active += int(np.sum(np.min(v[:, n:n + m], axis=1) < 1e-6)); total += cnt
        ref = np.stack([TR.vdot(grp["G"][p], none, grp["var"][p], grp["a"][p], v[p],
                                TR.rho(n, 0, m, grp["var"][p], v[p], {key: val[p] for key, val in dsym.items()})) for p in range(cnt)])
        worst = max(worst, float(rel_inf_rows(vdot, ref).max()))
    bound = max(TOL64, 10 * D_cpu)
    print(f"active-set forward_ad: D = {D_cpu:.3e} (seed {ACTIVE_SEED}, {total} problems), bound {bound:.3e}, "
          f"{active} of {total} problems with an active row, worst rel-inf of vdot {worst:.3e}")
    assert 2 * active >= total, (active, total)
    assert worst < bound, (worst, bound)


def test_forward_ad_failing_problem_gets_a_zero_tangent():
    """(d) One problem whose forward fails (a constraint index outside [0, n): MO_STATUS_BAD_INDEX) inside a healthy batch: its tangent rows
    are zero, the others are to the bit what they are without it, and tangent_status tells which problem it was."""
    n, m, B = 8, 2, 6
    rng = np.random.default_rng(29)
    U = rng.uniform(-1, 1, (B, n, n))
    G = np.einsum("bik,bjk->bij", U, U) / n + np.eye(n)
    c = rng.normal(size=(B, n))
    a = np.tile(np.array([[1.0, -1.0]]), (B, 1))
    b = np.tile(np.array([[0.2, 2.0]]), (B, 1))            # -0.2 <= x_0 <= 2
    tang = [rng.normal(size=t.shape) for t in (G, c, a, b)]
    out = []
    for broken in (False, True):
        var = np.zeros((B, m), dtype=np.int32)
        if broken:
            var[3, 1] = n + 1
        with fwAD.dual_level():
            duals = [fwAD.make_dual(T(p), T(t)) for p, t in zip((G, c, a, b), tang)]
            res = D.solve_qp(G=duals[0], c=duals[1], cons_var=T(var, torch.int32), cons_a=duals[2], cons_b=duals[3], params=params(),
                             return_all=True, return_status=True)
            vdot = torch.cat([fwAD.unpack_dual(t).tangent for t in res[:4]], dim=1).clone()
            out.append((vdot, res[4].cpu().numpy(), D.tangent_status(res[0]).cpu().numpy()))
    (t_ok, st_ok, ts_ok), (t_bad, st_bad, ts_bad) = out
    assert np.all(st_ok == 0) and np.all(ts_ok == 0)
    assert st_bad[3] == L.MO_STATUS_BAD_INDEX and ts_bad[3] != 0, (st_bad, ts_bad)
    others = [0, 1, 2, 4, 5]
    assert np.all(st_bad[others] == 0) and np.all(ts_bad[others] == 0)
    assert torch.all(t_bad[3] == 0) and torch.all(torch.isfinite(t_bad))
    assert torch.equal(t_bad[others], t_ok[others]) and torch.any(t_ok[3] != 0)


def test_forward_ad_j_level_with_duals_on_j_and_lam_only():
    """(e) J-level input, dual tensors for J and lam only (every other input plain): the tangent of [x | s | y | z] against the numpy
    restatement at the device's v, TOL64."""
    n, k, m, m_r, B = 8, 2, 5, 12, 8
    hb = host_batch(n, k, m, m_r, B, stream=56)
    rng = np.random.default_rng(30)
    dJ, dlam = rng.normal(size=hb.J.shape), rng.normal(size=B)
    with fwAD.dual_level():
        J = fwAD.make_dual(T(hb.J), T(dJ))
        lam = fwAD.make_dual(torch.full((B,), 1e-3, dtype=torch.float64, device=dev()), T(dlam))
        res = D.solve_qp(J=J, r=T(hb.r), lam=lam, A_eq=T(hb.A_eq.transpose(0, 2, 1)), b_eq=T(hb.b_eq), cons_var=T(hb.cons_var, torch.int32),
                         cons_a=T(hb.cons_a), cons_b=T(hb.cons_b), params=params(), return_all=True)
        assert torch.all(D.tangent_status(res[0]) == 0)
        v = torch.cat([fwAD.unpack_dual(t).primal for t in res], dim=1).cpu().numpy()
        vdot = torch.cat([fwAD.unpack_dual(t).tangent for t in res], dim=1).cpu().numpy()
    for p in range(B):
        Gp = hb.J[p].T @ hb.J[p] + 1e-3 * np.eye(n)
        rho = TR.rho(n, k, m, hb.cons_var[p], v[p], dict(J=dJ[p], lam=dlam[p]), J=hb.J[p], r=hb.r[p])
        ref = TR.vdot(Gp, hb.A_eq[p].T, hb.cons_var[p], hb.cons_a[p], v[p], rho)
        err = np.max(np.abs(vdot[p] - ref)) / np.max(np.abs(ref))
        print(f"J-level forward_ad, problem {p}: vdot {err:.3e}")
        assert err < TOL64


# ---- 7. nothing is allocated on the launch path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 8, 32, 128), (96, 40, 20, 128)], ids=["cfg3", "large"])
def test_first_tangent_launch_and_solve_allocate_nothing(shape):
    n, k, m, m_r = shape
    B = 24
    hb = host_batch(n, k, m, m_r, B, stream=57)
    d = directions(hb, 31)
    # what the HIP runtime reserves on its own account (module load, kernel code) happens on ANOTHER plan and shape-twin first
    prob = device_problem(hb, "J")
    tang = device_tangents(d, level_keys(hb, "J"), torch.float64)
    v = T(hb.vars)
    desc = L.PlanDesc(n, k, m, m_r, L.MO_F64, 0, L.EXTRA_PLAN_FLAGS, 0, B)
    plans = [C.c_void_p(), C.c_void_p()]
    for pl in plans:
        L.check(L.lib().mo_plan_create(C.byref(desc), C.byref(pl)))
    ps = prob.as_struct()
    V = hb.vars.shape[1]
    rho, out = torch.empty_like(v), torch.empty_like(v)
    status = torch.empty(B, dtype=torch.int32, device=dev())
    t = L.QPTangents()
    t.dJ, t.dJ_stride, t.dJ_ld = tang["J"].data_ptr(), m_r * n, n
    t.dr, t.dr_stride, t.dlambda, t.dlambda_stride = tang["r"].data_ptr(), m_r, tang["lam"].data_ptr(), 1
    t.dA_eq, t.dA_stride, t.dA_ld, t.db_eq, t.db_stride = tang["A_eq"].data_ptr(), n * k, k, tang["b_eq"].data_ptr(), k
    t.dcons_a, t.dcons_b, t.dcons_stride = tang["cons_a"].data_ptr(), tang["cons_b"].data_ptr(), m

    def both(plan):
        L.check(L.lib().mo_qp_tangent_rhs(plan, C.byref(ps), B, Q._ptr(v), V, C.byref(t), Q._ptr(rho), V, Q._stream()))
        L.check(L.lib().mo_kkt_solve(plan, C.byref(ps), B, Q._ptr(v), V, Q._ptr(rho), V, 0, Q._ptr(out), V, Q._ptr(status), Q._stream()))
        torch.cuda.synchronize()

    try:
        both(plans[0])
        free0 = torch.cuda.mem_get_info()[0]
        both(plans[1])                                      # the FIRST launches of this plan
        assert torch.cuda.mem_get_info()[0] >= free0 - (1 << 20), (free0, torch.cuda.mem_get_info()[0])
        assert torch.all(status == 0) and torch.all(torch.isfinite(out))
        ref = reference_vdot(hb, reference_rho(hb, d, level_keys(hb, "J"), "J"))
        assert rel_inf_rows(out.cpu().numpy(), ref).max() < TOL64
    finally:
        for pl in plans:
            L.lib().mo_plan_destroy(pl)


# ---- 8. the LDS budget ---------------------------------------------------------------------------------------------------------------------------
def tangent_lds_bytes(n, k, m, m_r, elem):
    """The header's statement: 2 n + 2 k + m + 2 m_r values, each block padded to 16 bytes, m 32-bit indices and 4 KiB of partial sums."""
    pad = lambda x: -(-x * elem // 16) * 16
    return 2 * pad(n) + 2 * pad(k) + pad(m) + 2 * pad(m_r) + 4 * m + 4096


def test_lds_refusal_names_the_shape_and_launches_nothing():
    """n = 8, k = m = 0, fp64, batch 1: the smallest m_r whose vectors exceed 64 KiB is refused with MO_ERR_UNSUPPORTED and a message that
    names the shape, and rho keeps its canary; the m_r one below runs and matches the reference."""
    n = 8
    m_r = next(q for q in range(1, 1 << 16) if tangent_lds_bytes(n, 0, 0, q, 8) > 64 * 1024)
    assert tangent_lds_bytes(n, 0, 0, m_r - 1, 8) <= 64 * 1024
    for rows, refused in ((m_r, True), (m_r - 1, False)):
        hb = host_batch(n, 0, 0, rows, 1, stream=58)
        d = directions(hb, 32)
        raw = Raw(hb, "J")
        rc, rho = raw.call(raw.members(d, ["J", "r", "lam"], pad=0), rho_pad=2)
        if refused:
            assert rc == -3 and f"m_r = {rows}".encode() in L.lib().mo_last_error(), (rc, L.lib().mo_last_error())
            assert torch.all(rho == Raw.CANARY)
            # without dJ and dr no residual row is kept: the same plan takes the call
            assert raw.call(raw.members(d, ["lam"], pad=0))[0] == 0
        else:
            assert rc == 0 and torch.all(rho[:, raw.V:] == Raw.CANARY)
            ref = reference_rho(hb, d, ["J", "r", "lam"], "J")
            assert rel_inf_rows(rho[:, :raw.V].cpu().numpy(), ref).max() < TOL64
