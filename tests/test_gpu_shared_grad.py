"""GPU tests of the batch-reduced gradients (run with -m gpu on an MI355X): mo_qp_gradients_shared against the float64 sums of
tests/shared_grad_reference.py, and solve_qp with inputs given once for the batch (leading dimension 1, never expanded).

The bound is derived: every output is a sum of B (dJ: B + n) products, so an element whose exact value is sum a_p b_p may be off by
2 (B + n + 8) UNIT[dtype] sum |a_p| |b_p| (shared_grad_reference.bound); the reference is numpy float64 on the inputs as the device holds
them (fp32 inputs promoted)."""
import ctypes as C

import numpy as np
import pytest
import torch

from mini_opt_amd import _lib as L
from mini_opt_amd import diff as D
from mini_opt_amd import qp as Q
from tests import shared_grad_reference as S
from tests.sens_fixtures import CANARY, PARAMS, UNIT, Guarded, T, cus, dev, expand, host_batch, ragged_batch

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
NPDT = {F64: np.float64, F32: np.float32}
SHAPES = [(7, 3, 4, 9), (16, 0, 0, 4), (33, 17, 6, 35), (64, 8, 32, 128), (128, 16, 64, 256)]   # (n, k, m, m_r)
J_KEYS, G_KEYS = ("J", "r", "lam"), ("G", "c")


def row_keys(k, m):
    return (("A_eq", "b_eq") if k else ()) + (("cons_a", "cons_b") if m else ())


def data(shape, B, dt, seed, integer=False, r_shared=False):
    """vars, u [B, V], var [m], J [m_r, n], r [B or 1, m_r] in the values the device will hold (float64 arrays of dt-representable numbers)."""
    n, k, m, m_r = shape
    rng = np.random.default_rng(seed)
    draw = (lambda *s: rng.integers(-2, 3, s).astype(np.float64)) if integer else (lambda *s: rng.normal(size=s).astype(NPDT[dt]).astype(np.float64))
    Vn = n + 2 * m + k
    return dict(V=draw(B, Vn), U=draw(B, Vn), var=rng.integers(0, n, m).astype(np.int32), J=draw(m_r, n), R=draw(1 if r_shared else B, m_r))


def problem(shape, d, dt, level, J_layout="row", J_pad=0):
    """A BatchedQP whose every input is ONE instance (leading dimension 1) but r; only J, r and cons_var are read by the gradients."""
    n, k, m, m_r = shape
    kw = dict(n=n, k=k, m=m)
    if k:
        kw.update(A_eq=torch.zeros(1, n, k, dtype=dt, device=dev()), b_eq=torch.zeros(1, k, dtype=dt, device=dev()))
    if m:
        kw.update(cons_var=T(d["var"][None], torch.int32), cons_a=torch.ones(1, m, dtype=dt, device=dev()), cons_b=torch.ones(1, m, dtype=dt, device=dev()))
    if level == "G":
        return Q.BatchedQP(G=torch.eye(n, dtype=dt, device=dev())[None].contiguous(), c=torch.zeros(1, n, dtype=dt, device=dev()), **kw)
    if J_layout == "col":
        Jt = np.zeros((1, n, m_r + J_pad)); Jt[0, :, :m_r] = d["J"].T
        return Q.BatchedQP(J=T(Jt, dt), r=T(d["R"], dt), J_layout="col", J_rows=m_r, **kw)
    Jt = np.zeros((1, m_r, n + J_pad)); Jt[0, :, :n] = d["J"]
    return Q.BatchedQP(J=T(Jt, dt), r=T(d["R"], dt), **kw)


def to_math(prob, key, t):
    """A [1, ...] device output in the orientation of shared_grad_reference (A_eq k x n, J m_r x n), float64."""
    a = t[0].double().cpu().numpy()
    if key == "A_eq":
        return a.T
    if key == "J":
        return a[:, :prob.m_r].T if prob.J_layout == "col" else a[:, :prob.n]
    return a


def shared(prob, d, dt, want, ok_fwd=None, ok_adj=None):
    sf = None if ok_fwd is None else T(np.where(ok_fwd, 0, 2), torch.int32)
    sa = None if ok_adj is None else T(np.where(ok_adj, 0, 2), torch.int32)
    out = D.qp_gradients_shared(prob, T(d["V"], dt), T(d["U"], dt), want, status_fwd=sf, status_adj=sa)
    torch.cuda.synchronize()
    return {key: to_math(prob, key, t) for key, t in out.items()}


def reference(shape, d, ok=None, level="J"):
    n, k, m, _ = shape
    ok = np.ones(len(d["V"]), dtype=bool) if ok is None else ok
    return S.direct(n, k, m, d["var"], d["V"], d["U"], ok, J=d["J"] if level == "J" else None, R=d["R"] if level == "J" else None)


def check_bound(got, val, mag, B, n, dt, keys, what=""):
    tol = S.bound(B, n, UNIT[dt], mag)
    for key in keys:
        err = np.abs(got[key] - val[key])
        ratio = float(np.max(err / np.maximum(tol[key], np.finfo(np.float64).tiny)))
        print(f"{what}{key}: max error / bound = {ratio:.3e}")
        assert np.all(np.isfinite(got[key])) and np.all(err <= tol[key]), (what, key, float(err.max()), ratio)


# ---- 1. the fragment maps, exactly --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("J_layout", ["row", "col"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"n{s[0]}k{s[1]}m{s[2]}r{s[3]}" for s in SHAPES])
def test_integer_data_gives_the_integer_result(shape, J_layout, dt):
    """Integers in {-2, ..., 2} in vars, u, J and r, B = 256: every intermediate is below 2^19, so every output is exact in both dtypes
    and must EQUAL the float64 result -- a wrong operand lane, C/D row map, tile offset or transpose cannot hide in a tolerance."""
    n, k, m, m_r = shape
    B = 256
    for r_shared in (False, True):
        d = data(shape, B, dt, 100 + n, integer=True, r_shared=r_shared)
        val, _ = reference(shape, d)
        got = shared(problem(shape, d, dt, "J", J_layout), d, dt, J_KEYS + row_keys(k, m))
        got.update(shared(problem(shape, d, dt, "G"), d, dt, G_KEYS))
        for key in J_KEYS + G_KEYS + row_keys(k, m):
            assert got[key].shape == np.shape(val[key]) and np.array_equal(got[key], val[key]), (key, r_shared)


# ---- 2. random data within the derived bound ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("which", ["1", "3", "5", "ragged", "4096"])
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]], ids=["n33", "n64"])
def test_random_data_against_the_float64_sum(shape, which, dt):
    """B = 1 and 3 (less than one MFMA step), 5 (a ragged second step), 4 chunks + 1 and 4096 (many chunks): within the bound of the float64
    sum, and within the same bound of the float64 host sum of mo_qp_gradients' per-problem outputs."""
    n, k, m, m_r = shape
    B = ragged_batch(S.chunks) if which == "ragged" else int(which)
    if which == "ragged":
        assert S.chunks(B, cus()) > 1 and S.chunk_len(B, cus()) % 4 != 0
    d = data(shape, B, dt, 7 * n + B)
    for level, keys in (("J", J_KEYS + row_keys(k, m)), ("G", G_KEYS)):
        prob = problem(shape, d, dt, level)
        val, mag = reference(shape, d, level=level)
        got = shared(prob, d, dt, keys)
        check_bound(got, val, mag, B, n, dt, keys, f"B={B} vs float64: ")
        each = D.qp_gradients(prob, T(d["V"], dt), T(d["U"], dt), keys)
        summed = {key: to_math(prob, key, torch.as_tensor(t.cpu().numpy().astype(np.float64).sum(0, keepdims=True))) for key, t in each.items()}
        check_bound(got, summed, mag, B, n, dt, keys, f"B={B} vs per-problem sum: ")


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_each_member_alone(dt):
    """Every output asked for alone, all other members NULL: the bound, and the bits of the call that asks for all of them."""
    shape = SHAPES[2]
    n, k, m, m_r = shape
    B = 37
    d = data(shape, B, dt, 5150)
    for level, keys in (("J", J_KEYS + row_keys(k, m)), ("G", G_KEYS)):
        prob = problem(shape, d, dt, level)
        val, mag = reference(shape, d, level=level)
        every = shared(prob, d, dt, keys)
        for key in keys:
            alone = shared(prob, d, dt, (key,))
            assert set(alone) == {key}
            check_bound(alone, val, mag, B, n, dt, (key,), "alone: ")
            assert np.array_equal(alone[key], every[key]), key


# ---- 3. masking ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_masked_problems_contribute_nothing(dt):
    """Every fifth problem carries status 2 in status_fwd or in status_adj (alternating) and a row of NaN in u.  One chunk before and
    after (B = 30 -> 24): the result is finite and equals, to the bit, the call on the batch with those problems removed.  Many chunks
    (B = 4096, the boundaries move): within the bound.  Every problem masked: exact zeros."""
    shape = SHAPES[2]
    n, k, m, m_r = shape
    keys = J_KEYS + row_keys(k, m)
    for B in (30, 4096):
        d = data(shape, B, dt, 900 + B)
        bad = np.arange(B) % 5 == 3
        ok_fwd = ~(bad & (np.arange(B) % 10 == 3))
        ok_adj = ~(bad & (np.arange(B) % 10 == 8))
        assert np.array_equal(ok_fwd & ok_adj, ~bad)
        d["U"][bad] = np.nan
        kept = dict(d, V=d["V"][~bad], U=d["U"][~bad], R=d["R"][~bad])
        for level, keys in (("J", J_KEYS + row_keys(k, m)), ("G", G_KEYS)):
            got = shared(problem(shape, d, dt, level), d, dt, keys, ok_fwd, ok_adj)
            val, mag = reference(shape, d, ok=~bad, level=level)
            check_bound(got, val, mag, B, n, dt, keys, f"masked B={B}: ")
            if B == 30:
                assert S.chunks(B, cus()) == 1 and S.chunks(int((~bad).sum()), cus()) == 1
                without = shared(problem(shape, kept, dt, level), kept, dt, keys)
                for key in keys:
                    assert np.array_equal(got[key], without[key]), key
    keys = J_KEYS + row_keys(k, m)
    got = shared(problem(shape, d, dt, "J"), d, dt, keys, np.zeros(B, dtype=bool), None)
    for key in keys:
        assert np.all(got[key] == 0), key


def test_empty_batch_writes_zeros():
    shape = SHAPES[0]
    n, k, m, m_r = shape
    d = data(shape, 0, F64, 1)
    d["R"] = np.zeros((1, m_r))
    got = shared(problem(shape, d, F64, "J"), d, F64, J_KEYS + row_keys(k, m))
    for key, a in got.items():
        assert np.all(a == 0), key


# ---- 4. layout: strides, leading dimensions, misaligned bases, canaries ----------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("J_layout", ["row", "col"])
@pytest.mark.parametrize("off", [1, 0], ids=["misaligned", "aligned"])
def test_strides_leading_dimensions_and_canaries(J_layout, dt, off):
    """vars_stride = u_stride = V + 3; dG_ld, dA_ld, dJ_ld padded by 3 with bases off 16 bytes (scalar stores), or to whole 16-byte pieces
    with aligned bases (16-byte stores); a canary
    in the padding, behind every output and behind the workspace; two launches give the same bits; dG is symmetric to the bit."""
    shape = SHAPES[2]
    n, k, m, m_r = shape
    B, Vn = 70, n + 2 * m + k
    ld_of = lambda width: width + 3 if off else (width + 3) // 4 * 4 + 4     # aligned: whole 16-byte pieces in both dtypes
    d = data(shape, B, dt, 31337)
    stride = Vn + 3
    wide = lambda a: T(np.concatenate([a, np.full((B, 3), np.nan)], axis=1), dt)
    v, u = wide(d["V"]), wide(d["U"])
    runs = []
    for level, keys in (("J", J_KEYS + row_keys(k, m)), ("G", G_KEYS)):
        prob = problem(shape, d, dt, level, J_layout, J_pad=5)
        ps = prob.as_struct()
        plan = D.plan_for(prob, B)
        val, mag = reference(shape, d, level=level)
        for launch in range(2):
            g = L.QPGrads()
            bufs = {}
            new = lambda key, count: bufs.setdefault(key, Guarded(count, dt, off)).view
            jr, jc = (n, m_r) if J_layout == "col" else (m_r, n)     # dJ: jr lines of jc contiguous values
            if level == "G":
                g.dG, g.dG_ld = Q._ptr(new("G", n * ld_of(n))), ld_of(n)
                g.dc = Q._ptr(new("c", n))
            else:
                g.dJ, g.dJ_ld = Q._ptr(new("J", jr * ld_of(jc))), ld_of(jc)
                g.dJ_layout = L.MO_COL_MAJOR if J_layout == "col" else L.MO_ROW_MAJOR
                g.dr, g.dlambda = Q._ptr(new("r", m_r)), Q._ptr(new("lam", 1))
                g.dA_eq, g.dA_ld = Q._ptr(new("A_eq", n * ld_of(k))), ld_of(k)
                g.db_eq, g.dcons_a, g.dcons_b = Q._ptr(new("b_eq", k)), Q._ptr(new("cons_a", m)), Q._ptr(new("cons_b", m))
            nbytes = C.c_int64()
            L.check(L.lib().mo_qp_gradients_shared_workspace(plan, C.byref(ps), B, C.byref(g), C.byref(nbytes)))
            work = torch.full((int(nbytes.value) + 64,), 99, dtype=torch.uint8, device=dev())
            L.check(L.lib().mo_qp_gradients_shared(plan, C.byref(ps), B, Q._ptr(v), stride, Q._ptr(u), stride, None, None, C.byref(g),
                                                   Q._ptr(work), int(nbytes.value), Q._stream()))
            torch.cuda.synchronize()
            assert bool(torch.all(work[int(nbytes.value):] == 99)), "workspace overrun"
            got = {}
            for key, b in bufs.items():
                assert b.intact(), key
                a = b.view.double().cpu().numpy()
                if key in ("G", "A_eq", "J"):
                    lines, width = {"G": (n, n), "A_eq": (n, k), "J": (jr, jc)}[key]
                    a = a.reshape(lines, ld_of(width))
                    assert np.all(a[:, width:] == CANARY), key       # the padding of every line is not written
                    a = a[:, :width]
                    a = a.T if key == "A_eq" or (key == "J" and J_layout == "col") else a
                got[key] = a[0] if key == "lam" else a
            check_bound(got, val, mag, B, n, dt, keys, "layout: ")
            runs.append(got)
        first, second = runs[-2], runs[-1]
        for key in keys:
            assert np.array_equal(first[key], second[key]), key
        if level == "G":
            assert np.array_equal(first["G"], first["G"].T)


# ---- 5. refusals, with a real plan -----------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_and_write_nothing():
    shape = SHAPES[0]
    n, k, m, m_r = shape
    B, dt = 40, F64
    d = data(shape, B, dt, 12)
    v, u = T(d["V"], dt), T(d["U"], dt)
    Vn = n + 2 * m + k
    lib = L.lib()
    prob = problem(shape, d, dt, "J")
    plan = D.plan_for(prob, B)
    out = Guarded(m_r * n, dt, 0)
    vec = Guarded(m, dt, 0)
    work = torch.empty(1 << 20, dtype=torch.uint8, device=dev())

    def call(ps, g, nbytes=1 << 20, base=0, refused=True):
        rc = lib.mo_qp_gradients_shared(plan, C.byref(ps), B, Q._ptr(v), Vn, Q._ptr(u), Vn, None, None, C.byref(g),
                                        C.c_void_p(work.data_ptr() + base), nbytes, Q._stream())
        torch.cuda.synchronize()
        assert not refused or (bool(torch.all(out.buf == CANARY)) and bool(torch.all(vec.buf == CANARY))), "a refused call wrote"
        return rc, lib.mo_last_error().decode()

    def grads(**kw):
        g = L.QPGrads()
        for key, val in kw.items():
            setattr(g, key, val)
        return g

    dJ = dict(dJ=Q._ptr(out.view), dJ_ld=n, dJ_layout=L.MO_ROW_MAJOR)
    ps = prob.as_struct()
    ps.J_stride = m_r * n
    rc, msg = call(ps, grads(**dJ))
    assert rc == -1 and "J_stride" in msg, (rc, msg)
    rc, msg = call(ps, grads(dr=Q._ptr(vec.view)))
    assert rc == -1 and "J_stride" in msg, (rc, msg)
    ps = prob.as_struct()
    ps.cons_stride = m
    for member in ("dcons_a", "dcons_b"):
        rc, msg = call(ps, grads(**{member: Q._ptr(vec.view)}))
        assert rc == -1 and "cons_stride" in msg, (rc, msg)
    rc, msg = call(prob.as_struct(), grads(dG=Q._ptr(out.view), dG_ld=n))                    # dG with J-level input
    assert rc == -1 and "dG" in msg, (rc, msg)
    probG = problem(shape, d, dt, "G")
    rc, msg = call(probG.as_struct(), grads(**dJ))                                            # dJ with (G, c) input
    assert rc == -1 and "dJ" in msg, (rc, msg)
    g = grads(**dJ)
    need = C.c_int64()
    L.check(lib.mo_qp_gradients_shared_workspace(plan, C.byref(prob.as_struct()), B, C.byref(g), C.byref(need)))
    assert 0 < need.value < (1 << 20)
    rc, msg = call(prob.as_struct(), g, nbytes=need.value - 1)                                # one byte short
    assert rc == -1 and "workspace" in msg and str(need.value) in msg, (rc, msg)
    rc, msg = call(prob.as_struct(), g, base=8)                                               # not 16-byte aligned
    assert rc == -1 and "aligned" in msg, (rc, msg)
    rc, msg = call(prob.as_struct(), g, nbytes=need.value, refused=False)                                    # ... and the exact size is taken
    assert rc == 0, msg
    assert not bool(torch.all(out.view == CANARY))


def test_no_allocation_on_the_launch_path():
    """hipMemGetInfo is flat across the FIRST call on a plan (module load and kernel code happen on a twin plan of the same shape first)."""
    shape = SHAPES[3]
    n, k, m, m_r = shape
    B, dt = 300, F64
    d = data(shape, B, dt, 13)
    prob = problem(shape, d, dt, "J")
    ps = prob.as_struct()
    v, u = T(d["V"], dt), T(d["U"], dt)
    Vn = n + 2 * m + k
    dJ = torch.empty(m_r, n, dtype=dt, device=dev())
    g = L.QPGrads()
    g.dJ, g.dJ_ld, g.dJ_layout = Q._ptr(dJ), n, L.MO_ROW_MAJOR
    plans = []
    for _ in range(2):
        desc = L.PlanDesc(n, k, m, m_r, L.MO_F64, 0, L.EXTRA_PLAN_FLAGS, 0, B)
        plan = C.c_void_p()
        L.check(L.lib().mo_plan_create(C.byref(desc), C.byref(plan)))
        plans.append(plan)
    need = C.c_int64()
    L.check(L.lib().mo_qp_gradients_shared_workspace(plans[1], C.byref(ps), B, C.byref(g), C.byref(need)))
    work = torch.empty(int(need.value), dtype=torch.uint8, device=dev())

    def run(plan):
        L.check(L.lib().mo_qp_gradients_shared(plan, C.byref(ps), B, Q._ptr(v), Vn, Q._ptr(u), Vn, None, None, C.byref(g), Q._ptr(work),
                                               int(need.value), Q._stream()))
        torch.cuda.synchronize()

    try:
        run(plans[0])
        free0 = torch.cuda.mem_get_info()[0]
        run(plans[1])                                      # the FIRST launches of this plan
        assert torch.cuda.mem_get_info()[0] >= free0 - (1 << 20), (free0, torch.cuda.mem_get_info()[0])
        assert torch.all(torch.isfinite(dJ))
    finally:
        for pl in plans:
            L.lib().mo_plan_destroy(pl)


# ---- 6. solve_qp end to end ------------------------------------------------------------------------------------------------------------------
def adjoint_of(n, k, m, kw, x, s, y, z, status, J_level):
    """(V, U, ok) on the host for the loss x.sum(): the state solve_qp returned and the adjoint mo_kkt_solve gives for g = [1 | 0 | 0 | 0]."""
    v = torch.cat([x, s, y, z], dim=1).detach().contiguous()
    g = torch.zeros_like(v)
    g[:, :n] = 1
    det = {key: (t.detach() if isinstance(t, torch.Tensor) else t) for key, t in kw.items()}
    if "A_eq" in det:
        det["A_eq"] = det["A_eq"].transpose(1, 2).contiguous()
    if J_level and isinstance(det.get("lam"), torch.Tensor):
        det["lam_vec"] = det.pop("lam")
    prob = Q.BatchedQP(n=n, k=k, m=m, **det)
    u, adj = D.kkt_solve(prob, v, g, transpose=True)
    ok = ((status == 0) & (adj == 0)).cpu().numpy()
    return v.double().cpu().numpy(), u.double().cpu().numpy(), ok


def test_solve_qp_shared_G_end_to_end():
    """B = 4096, n = 64, fp64: G [1, n, n], box rows given once, c per problem, one problem whose c is not finite (its forward fails).
    x is bit-equal to the call with G expanded by the caller; G.grad is [1, n, n], finite, within the bound of the expanded call's
    G.grad.sum(0); the backward's peak allocation stays below 32 MiB (the expanded call has to hold the 128 MiB [B, n, n] gradient)."""
    n, m, B = 64, 32, 4096
    rng = np.random.default_rng(64)
    Uu = rng.uniform(-1, 1, (n, n))
    G1 = T((Uu @ Uu.T / n + np.eye(n))[None])
    c = rng.normal(size=(B, n))
    c[7, 5] = np.nan
    c = T(c)
    var = T(np.r_[0:16, 0:16][None], torch.int32)
    a = T(np.r_[np.ones(16), -np.ones(16)][None])
    b = T(np.full((1, m), 0.5))                                # -0.5 <= x_i <= 0.5 for i < 16
    prm = Q.Params(**PARAMS)
    Gs = G1.clone().requires_grad_(True)
    cs = c.clone().requires_grad_(True)
    x, s, y, z, status = D.solve_qp(G=Gs, c=cs, cons_var=var, cons_a=a, cons_b=b, params=prm, return_all=True, return_status=True)
    assert int(status[7]) != 0 and int((status != 0).sum()) == 1
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    x.sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"backward peak allocation: {rise / 2**20:.1f} MiB")
    assert rise < 32 * 2**20, rise
    assert tuple(Gs.grad.shape) == (1, n, n) and bool(torch.all(torch.isfinite(Gs.grad)))
    assert torch.equal(Gs.grad[0], Gs.grad[0].T)
    Ge = expand(G1, B).requires_grad_(True)
    ce = c.clone().requires_grad_(True)
    xe = D.solve_qp(G=Ge, c=ce, cons_var=var, cons_a=a, cons_b=b, params=prm)
    assert torch.equal(x, xe)
    xe.sum().backward()
    assert torch.equal(cs.grad, ce.grad)
    V, U, ok = adjoint_of(n, 0, m, dict(G=G1, c=c, cons_var=var, cons_a=a, cons_b=b), x, s, y, z, status, False)
    assert not ok[7] and ok.sum() == B - 1
    val, mag = S.direct(n, 0, m, var[0].cpu().numpy(), V, U, ok)
    tol = S.bound(B, n, UNIT[F64], mag)["G"]
    got = Gs.grad[0].cpu().numpy()
    for what, ref in (("expanded sum", Ge.grad.sum(0).cpu().numpy()), ("float64 reference", val["G"])):
        err = np.abs(got - ref)
        print(f"G.grad vs {what}: max error / bound = {np.max(err / tol):.3e}")
        assert np.all(err <= tol), (what, float(err.max()))


def small_case(dt, seed=41):
    n, k, m, m_r, B = 64, 8, 32, 128, 64
    hb = host_batch(n, k, m, m_r, B, stream=seed, f32=dt == F32)
    kw = dict(A_eq=T(hb.A_eq.transpose(0, 2, 1), dt), b_eq=T(hb.b_eq, dt), cons_var=T(hb.cons_var, torch.int32), cons_a=T(hb.cons_a, dt),
              cons_b=T(hb.cons_b, dt))
    return (n, k, m, m_r, B), hb, kw


def run_pair(dims, kw, shared_names, dt, J_level):
    """solve_qp with the inputs `shared_names` given once and then expanded by the caller: x to the bit, every shared gradient [1, ...],
    finite and within the bound of the expanded call's gradient summed over the batch (and of the float64 reference)."""
    n, k, m, m_r, B = dims
    prm = Q.Params(**PARAMS)
    res = []
    for expanded in (False, True):
        args = {}
        for key, t in kw.items():
            if isinstance(t, torch.Tensor) and t.is_floating_point():
                t = expand(t, B) if expanded and key in shared_names else t.detach().clone()
                t.requires_grad_(key in shared_names)
            args[key] = t
        x, s, y, z, status = D.solve_qp(params=prm, return_all=True, return_status=True, **args)
        x.sum().backward()
        res.append((args, x, s, y, z, status))
    (args, x, s, y, z, status), (args_e, xe, *_rest) = res
    assert torch.equal(x, xe)
    V, U, ok = adjoint_of(n, k, m, kw, x, s, y, z, status, J_level)
    var = kw["cons_var"][0].cpu().numpy()
    Jm = kw["J"][0].double().cpu().numpy() if J_level else None
    Rm = kw["r"].double().cpu().numpy() if J_level else None
    val, mag = S.direct(n, k, m, var, V, U, ok, J=Jm, R=Rm)
    tol = S.bound(B, n, UNIT[dt], mag)
    key_of = {"G": "G", "J": "J", "r": "r", "lam": "lam", "A_eq": "A_eq"}
    for name in shared_names:
        gs, ge = args[name].grad, args_e[name].grad
        assert gs is not None and int(gs.shape[0]) == 1 and tuple(gs.shape[1:]) == tuple(ge.shape[1:]) and bool(torch.all(torch.isfinite(gs)))
        got = gs[0].double().cpu().numpy()
        for what, ref in (("expanded sum", ge.double().sum(0).cpu().numpy()), ("float64 reference", val[key_of[name]])):
            err = np.abs(got - ref)
            t = np.broadcast_to(tol[key_of[name]], err.shape)
            print(f"{name}.grad vs {what}: max error / bound = {np.max(err / np.maximum(t, 1e-300)):.3e}")
            assert np.all(err <= t), (name, what, float(err.max()))


@pytest.mark.parametrize("r_shared", [False, True], ids=["r_per_problem", "r_shared"])
def test_solve_qp_shared_J(r_shared):
    dims, hb, kw = small_case(F64)
    kw.update(J=T(hb.J[:1]), r=T(hb.r[:1] if r_shared else hb.r), lam=T(np.array([1e-3])))
    run_pair(dims, kw, ("J", "lam") + (("r",) if r_shared else ()), F64, True)


def test_solve_qp_shared_r_with_a_J_per_problem_falls_back_to_the_summed_per_problem_result():
    dims, hb, kw = small_case(F64)
    n, k, m, m_r, B = dims
    prm = Q.Params(**PARAMS)
    r1 = T(hb.r[:1]).requires_grad_(True)
    re = expand(r1, B).requires_grad_(True)
    x = D.solve_qp(J=T(hb.J), r=r1, lam=1e-3, params=prm, **kw)
    x.sum().backward()
    xe = D.solve_qp(J=T(hb.J), r=re, lam=1e-3, params=prm, **kw)
    xe.sum().backward()
    assert torch.equal(x, xe) and tuple(r1.grad.shape) == (1, m_r)
    assert torch.equal(r1.grad[0], re.grad.sum(0))


def test_solve_qp_shared_A_eq():
    dims, hb, kw = small_case(F64)
    n, k, m, m_r, B = dims
    kw.update(G=T(hb.G), c=T(hb.c), A_eq=T(hb.A_eq.transpose(0, 2, 1)[:1]))
    run_pair(dims, kw, ("A_eq",), F64, False)


def test_solve_qp_shared_G_fp32():
    dims, hb, kw = small_case(F32)
    kw.update(G=T(hb.G[:1], F32), c=T(hb.c, F32))
    run_pair(dims, kw, ("G",), F32, False)


def test_forward_mode_with_a_shared_dual_G():
    """torch.autograd.forward_ad: a dual [1, n, n] G (never expanded) gives the tangent of the call with G and its tangent expanded by the
    caller, to the bit."""
    import torch.autograd.forward_ad as fwAD
    dims, hb, kw = small_case(F64)
    n, k, m, m_r, B = dims
    G1, c = T(hb.G[:1]), T(hb.c)
    rng = np.random.default_rng(3)
    dG = rng.normal(size=(1, n, n))
    dG = T(dG + dG.transpose(0, 2, 1))
    prm = Q.Params(**PARAMS)
    tangents = []
    for expanded in (False, True):
        with fwAD.dual_level():
            Gd = fwAD.make_dual(expand(G1, B) if expanded else G1, expand(dG, B) if expanded else dG)
            x = D.solve_qp(G=Gd, c=c, params=prm, **kw)
            primal, tangent = fwAD.unpack_dual(x)
            assert tangent is not None and bool(torch.all(torch.isfinite(tangent)))
            tangents.append((primal.clone(), tangent.clone()))
    assert torch.equal(tangents[0][0], tangents[1][0]) and torch.equal(tangents[0][1], tangents[1][1])
    assert bool(torch.any(tangents[0][1] != 0))
