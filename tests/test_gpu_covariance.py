"""mo_qp_covariance (csrc/qp_covariance.hip) through the C ABI, against the long-double truth of tests/covariance_reference.py at the bound
    |C - C_truth|_max / |C_truth|_max <= 8 max(E_case, 8 eps)
(E_case: the worst error of the plain-numpy restatement in the plan's dtype over the case's batch), and its exactness properties bit for bit.
Every output buffer is prefilled with a NaN whose payload the kernel never writes (PREFILL): a word that still holds it was not written,
and no word outside the payload may lose it."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from mini_opt_amd import _lib as L
from mini_opt_amd import qp as Q
from tests import covariance_reference as CR
from tests.sens_fixtures import Plan
from tests.test_gpu_second_problem import batch_for, cus, draw_failures, pick_sample

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TDT = {"f64": torch.float64, "f32": torch.float32}
IDT = {"f64": torch.int64, "f32": torch.int32}
PREFILL = {"f64": 0x7FF8DEAD0000BEEF, "f32": 0x7FC0BEEF}
OK, NONFINITE, BAD_INDEX, NOT_PD = CR.OK, CR.NONFINITE, CR.BAD_INDEX, CR.NOT_POSITIVE_DEFINITE


def prefilled(shape, dtype):
    return torch.full(shape, PREFILL[dtype], dtype=IDT[dtype], device=DEV).view(TDT[dtype])


def bits(t, dtype):
    return t.view(IDT[dtype])


def untouched(t, dtype):
    return bits(t, dtype) == PREFILL[dtype]


def same_bits(a, b):
    as_int = torch.int64 if a.dtype == torch.float64 else torch.int32                     # (a view of equal element size takes any strides)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(as_int), b.view(as_int))


class Out:
    """cov [B, q, q] / var [B, q] (None if not asked for) as written, status [B] numpy, rc, and whether every padding word kept its prefill."""


def run(G, A, dtype, sel=None, scale=None, scale_stride=1, want_cov=True, want_var=True, pad=False, shared_G=False, shared_A=False,
        upper=None, batch=None):
    """One call.  G [B, n, n] (its lower triangle is handed over; `upper`: the value written over the strict upper triangle, default the
    mirror), A [B, k, n] or None, numpy holding values of `dtype`.  pad: G_ld = n + 3, A_ld = k + 2, cov_ld = q + 5 and every stride beyond
    its payload, the input padding NaN."""
    tdt = TDT[dtype]
    n = G.shape[1]
    k = 0 if A is None else A.shape[1]
    B = int(batch if batch is not None else max(G.shape[0], 0 if A is None else A.shape[0]))
    q = n if sel is None else len(sel)
    g_ld, a_ld, cov_ld = (n + 3, k + 2, q + 5) if pad else (n, k, q)
    g_stride, a_stride = g_ld * n + (7 if pad else 0), a_ld * n + (3 if pad else 0)
    cov_stride, var_stride = cov_ld * q + (9 if pad else 0), q + (4 if pad else 0)
    Gm = np.tril(G) + np.tril(G, -1).transpose(0, 2, 1)
    if upper is not None:
        iu = np.triu_indices(n, 1)
        Gm = Gm.copy(); Gm[:, iu[0], iu[1]] = upper
    g_host = np.full((G.shape[0], g_stride), np.nan)
    g_host[:, :g_ld * n].reshape(-1, n, g_ld)[:, :, :n] = Gm.transpose(0, 2, 1)          # column l of G = row l of the buffer
    g_dev = torch.as_tensor(g_host, dtype=tdt, device=DEV)
    prob = L.Problem()
    prob.G, prob.G_stride, prob.G_ld = Q._ptr(g_dev), (0 if shared_G else g_stride), g_ld
    a_dev = None
    if k:
        a_host = np.full((A.shape[0], a_stride), np.nan)
        a_host[:, :a_ld * n].reshape(-1, n, a_ld)[:, :, :k] = A.transpose(0, 2, 1)       # column i of A_eq (k entries) = row i of the buffer
        a_dev = torch.as_tensor(a_host, dtype=tdt, device=DEV)
        prob.A_eq, prob.A_stride, prob.A_ld = Q._ptr(a_dev), (0 if shared_A else a_stride), a_ld
    sel_dev = None if sel is None else torch.as_tensor(np.asarray(sel, dtype=np.int32), device=DEV)
    scale_dev = None if scale is None else torch.as_tensor(np.asarray(scale, dtype=np.float64).reshape(-1), dtype=tdt, device=DEV)
    cov = prefilled((B, cov_stride), dtype) if want_cov else None
    var = prefilled((B, var_stride), dtype) if want_var else None
    status = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    out = Out()
    with Plan(n, k, 0, 0, tdt, B) as plan:
        out.rc = L.lib().mo_qp_covariance(plan.h, C.byref(prob), B, Q._ptr(sel_dev), q, Q._ptr(scale_dev), scale_stride if scale is not None else 0,
                                          Q._ptr(cov), cov_stride, cov_ld, Q._ptr(var), var_stride, Q._ptr(status), Q._stream())
        out.msg = L.lib().mo_last_error().decode()
        torch.cuda.synchronize()
    out.status = status.cpu().numpy()
    out.padding_kept = True
    out.cov = out.var = None
    if want_cov:
        body = cov[:, :cov_ld * q].reshape(B, q, cov_ld)
        out.cov = body[:, :, :q].transpose(1, 2).contiguous()                             # [B, i, j]
        out.padding_kept &= bool(untouched(body[:, :, q:], dtype).all()) and bool(untouched(cov[:, cov_ld * q:], dtype).all())
        out.raw_cov = cov
    if want_var:
        out.var = var[:, :q].contiguous()
        out.padding_kept &= bool(untouched(var[:, q:], dtype).all())
        out.raw_var = var
    return out


def written(out, dtype):
    """No payload word still holds the prefill."""
    return all(not bool(untouched(t, dtype).any()) for t in (out.cov, out.var) if t is not None)


def check_against_truth(name, out, Ct, bound, dtype, rows=None):
    cov = out.cov.cpu().numpy()
    worst = 0.0
    for p in (range(cov.shape[0]) if rows is None else rows):
        if not Ct[p].any():
            assert not cov[p].any() and not np.signbit(cov[p]).any(), (name, p)           # exactly +0
            continue
        worst = max(worst, CR.error(cov[p], Ct[p]))
    print(f"covariance {name}: device error {worst / CR.EPS[dtype]:.2f} eps, bound {bound / CR.EPS[dtype]:.2f} eps")
    assert worst <= bound, (name, worst / CR.EPS[dtype], bound / CR.EPS[dtype])


# ---- 1 - 5: the case table --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CR.names())
def test_case_against_the_truth(name):
    case = CR.by_name(name)
    out = run(case.G, case.A, case.dtype)
    assert out.rc == 0, out.msg
    assert np.all(out.status == OK), out.status
    assert written(out, case.dtype) and out.padding_kept
    assert same_bits(out.cov, out.cov.transpose(1, 2).contiguous())                       # symmetric to the bit
    assert same_bits(out.var, torch.diagonal(out.cov, dim1=1, dim2=2).contiguous())       # the diagonal's bits
    check_against_truth(name, out, CR.reference(name), CR.bound(name), case.dtype)


def test_beyond_the_capacity_rule_is_unsupported_and_writes_nothing():
    n, k = CR.CAPACITY_N + 1, CR.CAPACITY_K
    rng = np.random.default_rng(7)
    out = run(np.eye(n)[None].repeat(2, 0), rng.uniform(-1, 1, (2, k, n)), "f64")
    assert out.rc == -3 and "LDS" in out.msg, (out.rc, out.msg)
    assert bool(untouched(out.raw_cov, "f64").all()) and bool(untouched(out.raw_var, "f64").all()) and np.all(out.status == -1)


# ---- 6: not positive definite -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def indefinite_batch():
    """n = 9, k = 2, B = 5: G = Q diag(d) Q^T; problems 1 and 3 have d_4 = -0.5 on a direction (column 4 of Q) inside null(A) = the span of
    the columns 2 .. 8 of Q.  A_fix adds that direction as a third equality row."""
    rng = np.random.default_rng(61)
    B, n, k = 5, 9, 2
    G = np.empty((B, n, n)); A = np.empty((B, k, n)); A_fix = np.empty((B, k + 1, n))
    for p in range(B):
        Qm = np.linalg.qr(rng.standard_normal((n, n)))[0]
        d = rng.uniform(0.5, 2.0, n)
        if p in (1, 3):
            d[4] = -0.5
        M = (Qm * d[None, :]) @ Qm.T
        G[p] = (M + M.T) / 2
        A[p] = Qm[:, :k].T
        A_fix[p] = Qm[:, [0, 1, 4]].T
    return G, A, A_fix


def test_not_positive_definite():
    G, A, A_fix = indefinite_batch()
    bad = np.array([False, True, False, True, False])
    out = run(G, A, "f64")
    assert out.rc == 0 and written(out, "f64")
    assert np.array_equal(out.status, np.where(bad, NOT_PD, OK)), out.status
    badt = torch.as_tensor(bad, device=DEV)
    assert bool(torch.isnan(out.cov[badt]).all()) and bool(torch.isnan(out.var[badt]).all())
    assert bool(torch.isfinite(out.cov[~badt]).all())
    for p in np.flatnonzero(~bad):                                                        # the neighbours give the bits they give alone
        alone = run(G[p:p + 1], A[p:p + 1], "f64")
        assert same_bits(alone.cov[0], out.cov[p]) and same_bits(alone.var[0], out.var[p]), p
    fixed = run(G, A_fix, "f64")                                                          # the direction removed by an equality row
    assert np.all(fixed.status == OK), fixed.status
    Ct = np.stack([CR.truth(G[p], A_fix[p]) for p in range(G.shape[0])])
    E = max(CR.error(CR.restatement(G[p], A_fix[p], "f64"), Ct[p]) for p in range(G.shape[0]))
    check_against_truth("indefinite_fixed", fixed, Ct, CR.FACTOR * max(E, CR.FLOOR * CR.EPS["f64"]), "f64")


# ---- 7: non-finite input ----------------------------------------------------------------------------------------------------------------
def test_non_finite_input():
    case = CR.by_name("eq_n7_k3_f64")
    clean = run(case.G, case.A, "f64")
    G, A = case.G.copy(), case.A.copy()
    G[0, 4, 2] = G[0, 2, 4] = np.nan                 # lower triangle of G
    G[2, 6, 6] = np.inf
    A[3, 1, 5] = np.nan
    A[4, 2, 0] = -np.inf
    out = run(G, A, "f64")
    bad = np.array([True, False, True, True, True])
    assert np.array_equal(out.status, np.where(bad, NONFINITE, OK)), out.status
    badt = torch.as_tensor(bad, device=DEV)
    assert written(out, "f64") and bool(torch.isnan(out.cov[badt]).all()) and bool(torch.isnan(out.var[badt]).all())
    assert same_bits(out.cov[1], clean.cov[1]) and same_bits(out.var[1], clean.var[1])
    up = run(case.G, case.A, "f64", upper=np.nan)    # NaN all over the strict upper triangle: never read
    assert np.all(up.status == OK) and same_bits(up.cov, clean.cov) and same_bits(up.var, clean.var)
    sc = run(case.G, case.A, "f64", scale=[1.0, np.nan, 2.0, np.inf, 0.5])               # the scale is an entry that is read
    assert np.array_equal(sc.status, [OK, NONFINITE, OK, NONFINITE, OK]), sc.status


# ---- 8: selection -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sel", [("eq_n7_k3_f64", (5, 0, 3, 5)), ("eq_n33_k5_f64", None), ("k0_n33_f64", None), ("eq_n33_k5_f32", None)])
def test_selection(name, sel):
    case = CR.by_name(name)
    if sel is None:
        sel = tuple(int(i) for i in np.random.default_rng(81).permutation(case.n)[:case.n // 2])   # a permuted half
    full = run(case.G, case.A, case.dtype)
    idx = torch.as_tensor(sel, device=DEV)
    want = full.cov.index_select(1, idx).index_select(2, idx)
    got = run(case.G, case.A, case.dtype, sel=sel, pad=True)
    assert got.rc == 0 and np.all(got.status == OK) and got.padding_kept and written(got, case.dtype)
    assert same_bits(got.cov, want)
    assert same_bits(got.var, torch.diagonal(want, dim1=1, dim2=2).contiguous())
    alone = run(case.G, case.A, case.dtype, sel=sel, want_cov=False)                      # var_out alone: the diagonal's bits
    assert alone.rc == 0 and np.all(alone.status == OK) and same_bits(alone.var, got.var)
    for bad in (case.n, -1):
        s = list(sel); s[1] = bad
        out = run(case.G, case.A, case.dtype, sel=s)
        assert out.rc == 0 and np.all(out.status == BAD_INDEX), (bad, out.status)
        assert written(out, case.dtype) and bool(torch.isnan(out.cov).all()) and bool(torch.isnan(out.var).all())


# ---- 9: strides and guards ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["eq_n7_k3_f64", "eq_n33_k5_f32", "k0_n17_f64", "eq_n64_k8_f64"])
def test_strides_and_guards(name):
    case = CR.by_name(name)
    packed = run(case.G, case.A, case.dtype)
    padded = run(case.G, case.A, case.dtype, pad=True)                                    # (the input padding is NaN: reading it shows as status 3)
    assert padded.rc == 0 and np.all(padded.status == OK) and padded.padding_kept and written(padded, case.dtype)
    assert same_bits(padded.cov, packed.cov) and same_bits(padded.var, packed.var)
    B = 4                                                                                 # one instance for the batch
    shared = run(case.G[2:3], None if case.A is None else case.A[2:3], case.dtype, shared_G=True, shared_A=True, batch=B, pad=True)
    assert np.all(shared.status == OK) and shared.padding_kept
    for p in range(B):
        assert same_bits(shared.cov[p], packed.cov[2]) and same_bits(shared.var[p], packed.var[2]), p
    mixed = run(case.G, None if case.A is None else case.A[2:3], case.dtype, shared_A=True)   # G per problem, A shared
    one = run(case.G[:1], None if case.A is None else case.A[2:3], case.dtype)
    assert same_bits(mixed.cov[0], one.cov[0])
    s = np.array([0.5, 2.0, 4.0, 0.25, 8.0])
    per = run(case.G, case.A, case.dtype, scale=s, scale_stride=1)
    once = run(case.G, case.A, case.dtype, scale=s[1:2], scale_stride=0)
    want = packed.cov * torch.as_tensor(s, dtype=packed.cov.dtype, device=DEV)[:, None, None]
    assert same_bits(per.cov, want) and same_bits(once.cov, packed.cov * 2.0)


# ---- 10: exactness ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k0_n17_f64", "k0_n65_f32", "eq_n33_k5_f64", "eq_n64_k8_f32", "deficient_n7_k3_f64", "singular_G_n12_mr9_k4_f64"])
def test_exactness_properties(name):
    case = CR.by_name(name)
    a = run(case.G, case.A, case.dtype)
    b = run(case.G, case.A, case.dtype)
    assert np.all(a.status == OK)
    assert same_bits(a.cov, a.cov.transpose(1, 2).contiguous())                           # symmetric to the bit
    assert same_bits(a.cov, b.cov) and same_bits(a.var, b.var)                            # two launches
    four = run(4.0 * case.G, case.A, case.dtype)                                          # 4 G -> C / 4
    assert same_bits(four.cov, a.cov * 0.25) and same_bits(four.var, a.var * 0.25)
    eighth = run(case.G, case.A, case.dtype, scale=[0.125], scale_stride=0)               # scale = 2^-3
    assert same_bits(eighth.cov, a.cov * 0.125) and same_bits(eighth.var, a.var * 0.125)
    diag = run(case.G, case.A, case.dtype, want_cov=False)                                # var_out alone
    assert same_bits(diag.var, a.var)


# ---- 11: a workgroup's second problem -----------------------------------------------------------------------------------------------------
SECOND_KINDS = ("neg_G", "neg_diag", "nan_G", "inf_A", "nan_scale")


@functools.lru_cache(maxsize=None)
def second_host(cu):
    n, k, seed = 8, 2, 1101
    cap = CR.workgroups_per_cu(n, k, n, 8)
    B = batch_for(cap, cu)
    rng = np.random.default_rng(seed)
    J = rng.uniform(-1, 1, (B, 2 * n, n))
    G = np.einsum("bqi,bqj->bij", J, J)
    A = rng.uniform(-1, 1, (B, k, n))
    scale = 2.0 ** rng.integers(-3, 4, B).astype(np.float64)
    kind = draw_failures(B, SECOND_KINDS, seed)
    names = np.array(["healthy"] + list(SECOND_KINDS))[kind + 1]
    G[names == "neg_G"] *= -1.0
    for p in np.flatnonzero(names == "neg_diag"):
        G[p, np.arange(n), np.arange(n)] -= 1e3
    G[names == "nan_G", 3, 1] = np.nan; G[names == "nan_G", 1, 3] = np.nan
    A[names == "inf_A", 1, 2] = np.inf
    scale[names == "nan_scale"] = np.nan
    for p in np.flatnonzero(names == "healthy")[::5]:                                    # a zero row: the early exit of the pivot loop, still a success
        A[p, p % k, :] = 0.0
    want = np.where(names == "healthy", OK, np.where((names == "neg_G") | (names == "neg_diag"), NOT_PD, NONFINITE))
    return dict(n=n, k=k, cap=cap, seed=seed, B=B, G=G, A=A, scale=scale, healthy=names == "healthy", want=want)


def test_second_problem_of_a_workgroup():
    cu = cus()
    d = second_host(cu)
    out = run(d["G"], d["A"], "f64", scale=d["scale"])
    assert out.rc == 0 and written(out, "f64")                                            # no output stays unwritten
    assert np.array_equal(out.status, d["want"])
    h = torch.as_tensor(d["healthy"], device=DEV)
    assert bool(torch.isfinite(out.cov[h]).all()) and bool(torch.isnan(out.cov[~h]).all()) and bool(torch.isnan(out.var[~h]).all())
    sample = pick_sample(d["B"], d["cap"] * cu, d["healthy"], ~d["healthy"], d["seed"])
    alone = run(d["G"][sample], d["A"][sample], "f64", scale=d["scale"][sample])         # one problem per workgroup on a fresh plan
    rows = torch.as_tensor(sample, device=DEV)
    assert same_bits(alone.cov, out.cov.index_select(0, rows)) and same_bits(alone.var, out.var.index_select(0, rows))
    assert np.array_equal(alone.status, out.status[sample])
    # ... and they are right: TOL64 = 1e-10 of tests/test_gpu_second_problem.py (the case table above holds the kernel to the tight bound;
    # here G = J^T J of a 16 x 8 uniform J restricted to a 6-dimensional null space, condition below 1e4, so 1e4 n eps is below 1e-10)
    for p in sample[d["healthy"][sample]][:16]:
        Ct = CR.truth(d["G"][p], d["A"][p][np.abs(d["A"][p]).sum(axis=1) > 0]) * d["scale"][p]
        assert CR.error(out.cov[p].cpu().numpy(), Ct) <= 1e-10, p


# ---- 12: qp.covariance --------------------------------------------------------------------------------------------------------------------
def test_python_surface():
    import mini_opt_amd
    case = CR.by_name("eq_n7_k3_f64")
    ref = run(case.G, case.A, "f64")
    Gd = torch.as_tensor(np.tril(case.G).transpose(0, 2, 1).copy(), dtype=torch.float64, device=DEV)
    Ad = torch.as_tensor(case.A.transpose(0, 2, 1).copy(), dtype=torch.float64, device=DEV)
    res = mini_opt_amd.covariance(Gd, Ad)
    assert res.var is None and tuple(res.cov.shape) == (5, 7, 7) and res.status.dtype == torch.int32 and bool((res.status == 0).all())
    assert same_bits(res.cov.transpose(1, 2).contiguous(), ref.cov)                       # (cov[b] is column-major: symmetric, so the same bits)
    res = Q.covariance(Gd, Ad, full=False, diag=True)
    assert res.cov is None and tuple(res.var.shape) == (5, 7) and same_bits(res.var, ref.var)
    res = Q.covariance(Gd, Ad, select=(5, 0, 3, 5), scale=0.5, diag=True)
    idx = torch.as_tensor((5, 0, 3, 5), device=DEV)
    want = ref.cov.index_select(1, idx).index_select(2, idx) * 0.5
    assert tuple(res.cov.shape) == (5, 4, 4) and same_bits(res.cov, want) and same_bits(res.var, torch.diagonal(want, dim1=1, dim2=2).contiguous())
    one = Q.covariance(Gd[2:3], Ad, scale=torch.full((5,), 2.0, dtype=torch.float64, device=DEV))   # [1, n, n] against [B, n, k]
    alone = run(case.G[2:3].repeat(5, 0), case.A, "f64", scale=[2.0], scale_stride=0)
    assert tuple(one.cov.shape) == (5, 7, 7) and same_bits(one.cov, alone.cov)
    k0 = Q.covariance(Gd.to(torch.float32))
    assert k0.cov.dtype == torch.float32 and bool((k0.status == 0).all())
    with pytest.raises(ValueError):
        Q.covariance(Gd, Ad, full=False, diag=False)
    with pytest.raises(ValueError):
        Q.covariance(Gd, Ad[:3])
