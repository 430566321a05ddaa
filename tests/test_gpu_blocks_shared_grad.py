"""GPU tests of the batch-reduced block gradients (run with -m gpu on an MI355X): mo_qp_gradients_blocks_shared against the float64 sums of
tests/blocks_shared_grad_reference.py, mo_linearize_blocks without G_out, and solve_qp(layout=...) with inputs given once for the batch
(leading dimension 1, never expanded).

The bound is derived: an output element is formed from at most 3 P_b + 1 totals (P_b terms M[i][j] + M[j][i], one Q, the partner term),
each a sum of B rounded products, so an element whose exact value is sum a b may be off by 2 (B + 3 P_max + 8) UNIT[dtype] sum |a| |b|
(blocks_shared_grad_reference.bound); the reference is numpy float64 on the inputs as the device holds them (fp32 inputs promoted)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from mini_opt_amd import _lib as L
from mini_opt_amd import diff as D
from mini_opt_amd import qp as Q
from tests import blocks_shared_grad_reference as BS
from tests import shared_grad_reference as S
from tests.sens_fixtures import (CANARY, LAM, N7_COST, PARAMS, UNIT, Guarded, T, autograd_layout, cus, dev, expand, ragged_batch,
                                 random_layout)

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
NPDT = {F64: np.float64, F32: np.float32}
DTYPES = pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
N7_EQ = [((0, 4, 0), 1), ((2, 6), 2)]     # the eq layout repeats an index inside a block: local column 0 LOSES variable 0
COST_KEYS, EQ_KEYS = ("J_blocks", "lam"), ("J_eq_blocks", "r_eq")


class Case:
    """A cost layout, an eq layout and m inequality rows (which only widen the state): "n7" N7_COST with N7_EQ; "n33" a random layout with
    repeats, where M crosses tile borders; "n64" 96 blocks of 2 x 4."""
    _made = {}

    def __init__(self, name, dt):
        rng = np.random.default_rng({"n7": 71, "n33": 331, "n64": 641}[name])
        if name == "n7":
            self.n, self.cost, self.eq, self.m = 7, N7_COST, N7_EQ, 3
        elif name == "n33":
            self.n, self.cost, self.eq, self.m = 33, random_layout(rng, 33, 14, repeats=True), [((5, 20, 5, 32), 2), ((16, 0, 31), 1)], 2
            assert any(len(set(idx)) < len(idx) for idx, _ in self.cost)
        else:
            self.n, self.cost, self.eq, self.m = 64, autograd_layout(64, rng), [((1, 6, 1), 2), ((63, 17, 40), 1)], 0
            assert len(self.cost) == 96 and all(R_ == 2 and len(idx) == 4 for idx, R_ in self.cost)
        self.k = sum(R_ for _, R_ in self.eq)
        self.V = self.n + 2 * self.m + self.k
        self.lay = Q.ResidualLayout(self.n, self.cost, dtype=dt)
        self.eq_lay = Q.ResidualLayout(self.n, self.eq, dtype=dt)
        self.pmax = BS.p_max(self.cost, self.eq)

    @classmethod
    def get(cls, name, dt):
        if (name, dt) not in cls._made:
            cls._made[(name, dt)] = cls(name, dt)
        return cls._made[(name, dt)]


def data(c, B, dt, seed, integer=False, r_shared=False):
    """vars, u [B, V], ONE J [values], r [B or 1, rows] in the values the device will hold (float64 arrays of dt-representable numbers)."""
    rng = np.random.default_rng(seed)
    draw = (lambda *s: rng.integers(-2, 3, s).astype(np.float64)) if integer else (lambda *s: rng.normal(size=s).astype(NPDT[dt]).astype(np.float64))
    return dict(V=draw(B, c.V), U=draw(B, c.V), J=draw(c.lay.values), R=draw(1 if r_shared else B, c.lay.rows))


def keys_of(r_shared):
    return COST_KEYS + (("r",) if r_shared else ()) + EQ_KEYS


def status_words(ok):
    return None if ok is None else T(np.where(ok, 0, 2), torch.int32)


def shared(c, d, dt, want, ok_fwd=None, ok_adj=None):
    out = D.qp_gradients_blocks_shared(c.lay, T(d["J"][None], dt), T(d["R"], dt), T(d["V"], dt), T(d["U"], dt), m=c.m, want=want,
                                       eq_layout=c.eq_lay, status_fwd=status_words(ok_fwd), status_adj=status_words(ok_adj))
    torch.cuda.synchronize()
    for key, t in out.items():
        assert int(t.shape[0]) == 1, key
    return {key: (t.double().cpu().numpy().reshape(-1)[0] if key == "lam" else t[0].double().cpu().numpy()) for key, t in out.items()}


def reference(c, d, ok=None):
    """(value, magnitude): the float64 direct sum over the counted problems and the same sum of absolute values."""
    ok = np.ones(len(d["V"]), dtype=bool) if ok is None else ok
    f = BS.direct if len(d["V"]) <= 64 else BS.direct_batched
    args = (c.n, c.k, c.m, c.cost, c.eq, d["J"], d["R"], d["V"], d["U"], ok)
    return f(*args), f(*args, absolute=True)


def check_bound(got, val, mag, B, c, dt, keys, what=""):
    tol = BS.bound(B, c.pmax, UNIT[dt], mag)
    for key in keys:
        err = np.abs(got[key] - val[key])
        ratio = float(np.max(err / np.maximum(tol[key], np.finfo(np.float64).tiny)))
        print(f"{what}{key}: max error / bound = {ratio:.3e}")
        assert np.all(np.isfinite(got[key])) and np.all(err <= tol[key]), (what, key, float(np.max(err)), ratio)


# ---- 1. the gathers, exactly ---------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", ["n7", "n33", "n64"])
def test_integer_data_gives_the_integer_result(name, dt):
    """Integers in {-2, ..., 2} in vars, u, J_blocks and r, B = 256: every intermediate is below 2^19 for P_b <= 8, so every output is exact
    in both dtypes and must EQUAL the float64 result -- a wrong schedule entry, tile offset, partner list or winner cannot hide in a
    tolerance."""
    c = Case.get(name, dt)
    B = 256
    for r_shared in (False, True):
        d = data(c, B, dt, 100 + c.n, integer=True, r_shared=r_shared)
        val, _ = reference(c, d)
        got = shared(c, d, dt, keys_of(r_shared))
        for key in keys_of(r_shared):
            assert np.shape(got[key]) == np.shape(val[key]) and np.array_equal(got[key], val[key]), (key, r_shared)


# ---- 2. random data within the derived bound -----------------------------------------------------------------------------------------------
def per_problem_sum(c, d, dt, keys):
    """The float64 host sum of mo_qp_gradients_blocks' and mo_qp_gradients_eq_blocks' per-problem outputs."""
    v, u = T(d["V"], dt), T(d["U"], dt)
    cost = [key for key in keys if key in ("J_blocks", "r", "lam")]
    each = D.qp_gradients_blocks(c.lay, T(d["J"][None], dt), T(d["R"], dt), v, u, k=c.k, m=c.m, want=cost)
    each.update(D.qp_gradients_eq_blocks(c.eq_lay, v, u, m=c.m, want=[key for key in keys if key in EQ_KEYS]))
    return {key: t.cpu().numpy().astype(np.float64).sum(0) for key, t in each.items()}


@DTYPES
@pytest.mark.parametrize("which", ["1", "3", "5", "ragged", "4096"])
@pytest.mark.parametrize("name", ["n33", "n64"])
def test_random_data_against_the_float64_sum(name, which, dt):
    """B = 1 and 3 (less than one MFMA step), 5 (a ragged second step), 4 chunks + 1 and 4096 (many chunks), r per problem and shared: within
    the bound of the float64 direct sum, and within the same bound of the float64 host sum of the per-problem kernels' outputs."""
    c = Case.get(name, dt)
    B = ragged_batch(BS.chunks) if which == "ragged" else int(which)
    if which == "ragged":
        assert BS.chunks(B, cus()) > 1 and BS.chunk_len(B, cus()) % 4 != 0
    for r_shared in (False, True):
        if B == 1 and r_shared:
            continue   # (one problem: r [1, rows] IS the per-problem r)
        d = data(c, B, dt, 7 * c.n + B, r_shared=r_shared)
        keys = keys_of(r_shared)
        val, mag = reference(c, d)
        got = shared(c, d, dt, keys)
        check_bound(got, val, mag, B, c, dt, keys, f"B={B} vs float64: ")
        check_bound(got, per_problem_sum(c, d, dt, keys), mag, B, c, dt, keys, f"B={B} vs per-problem sum: ")


@DTYPES
def test_each_member_alone_and_two_launches(dt):
    """Every output asked for alone, all other members NULL: the bound, and the bits of the call that asks for all of them; a second launch
    of that call repeats its bits."""
    c = Case.get("n33", dt)
    B = 37
    for r_shared in (False, True):
        d = data(c, B, dt, 5150, r_shared=r_shared)
        keys = keys_of(r_shared)
        val, mag = reference(c, d)
        every, again = shared(c, d, dt, keys), shared(c, d, dt, keys)
        for key in keys:
            assert np.array_equal(every[key], again[key]), key
            alone = shared(c, d, dt, (key,))
            assert set(alone) == {key}
            check_bound(alone, val, mag, B, c, dt, (key,), "alone: ")
            assert np.array_equal(alone[key], every[key]), key


# ---- 3. masking ----------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_masked_problems_contribute_nothing(dt):
    """Every fifth problem carries status 2 in status_fwd or in status_adj (alternating) and a row of NaN in u.  One chunk before and
    after (B = 30 -> 24): the result is finite and equals, to the bit, the call on the batch with those problems removed.  Many chunks
    (B = 4096, the boundaries move): within the bound.  Every problem masked: exact zeros."""
    c = Case.get("n33", dt)
    keys = keys_of(False)
    for B in (30, 4096):
        d = data(c, B, dt, 900 + B)
        bad = np.arange(B) % 5 == 3
        ok_fwd = ~(bad & (np.arange(B) % 10 == 3))
        ok_adj = ~(bad & (np.arange(B) % 10 == 8))
        assert np.array_equal(ok_fwd & ok_adj, ~bad)
        d["U"][bad] = np.nan
        d["R"][bad[:len(d["R"])]] = np.nan
        got = shared(c, d, dt, keys, ok_fwd, ok_adj)
        val, mag = reference(c, d, ok=~bad)
        check_bound(got, val, mag, B, c, dt, keys, f"masked B={B}: ")
        if B == 30:
            assert BS.chunks(B, cus()) == 1 and BS.chunks(int((~bad).sum()), cus()) == 1
            kept = dict(d, V=d["V"][~bad], U=d["U"][~bad], R=d["R"][~bad])
            without = shared(c, kept, dt, keys)
            for key in keys:
                assert np.array_equal(got[key], without[key]), key
    got = shared(c, d, dt, keys, np.zeros(B, dtype=bool), None)
    for key in keys:
        assert np.all(got[key] == 0), key


def test_empty_batch_writes_zeros():
    c = Case.get("n7", F64)
    for r_shared in (False, True):
        d = data(c, 0, F64, 1)
        d["R"] = np.zeros((1 if r_shared else 0, c.lay.rows))
        d["J"] = np.ones(c.lay.values)
        want = keys_of(r_shared)
        if not r_shared:   # (an r per problem of an empty batch has no row to point at: the packed values are asked for with the one r)
            want = ("lam",) + EQ_KEYS
        got = shared(c, d, F64, want)
        for key, a in got.items():
            assert np.all(a == 0), key


def test_empty_batch_with_an_r_per_problem_writes_zeros():
    """batch = 0 with r_stride != 0 and dJ_blocks asked for: the packed Q totals are summed over zero chunks.  r, vars and u point at one
    row that no kernel may read (NaN); J_blocks is all ones.  Exact zeros, nothing beyond the outputs touched."""
    dt = F64
    c = Case.get("n7", dt)
    nan_row = lambda size: torch.full((1, size), float("nan"), dtype=dt, device=dev())
    v, u, r = nan_row(c.V), nan_row(c.V), nan_row(c.lay.rows)
    J = torch.ones(1, c.lay.values, dtype=dt, device=dev())
    plan = D._plan_of(c.n, c.k, c.m, 0, dt, dev(), 1)
    bufs = {"dJ_blocks": Guarded(c.lay.values, dt), "dlambda": Guarded(1, dt), "dJ_eq_blocks": Guarded(c.eq_lay.values, dt), "dr_eq": Guarded(c.k, dt)}
    g = L.BlockSharedGrads()
    for member, b in bufs.items():
        setattr(g, member, b.view.data_ptr())
    nbytes = C.c_int64()
    L.check(L.lib().mo_qp_gradients_blocks_shared_workspace(plan, c.lay.h, c.eq_lay.h, c.lay.rows, 0, C.byref(g), C.byref(nbytes)))
    work = torch.full((int(nbytes.value) + 64,), 99, dtype=torch.uint8, device=dev())
    rc, msg = raw_call(c, plan, 0, v, u, c.V, J, r, c.lay.rows, g, work, int(nbytes.value))
    assert rc == 0, msg
    assert bool(torch.all(work[int(nbytes.value):] == 99)), "workspace overrun"
    for member, b in bufs.items():
        assert b.intact() and bool(torch.all(b.view == 0)), member


# ---- 4. layout: strides, misaligned bases, canaries -------------------------------------------------------------------------------------------
def raw_call(c, plan, B, v, u, stride, J, r, r_stride, g, work, nbytes, base=0):
    rc = L.lib().mo_qp_gradients_blocks_shared(plan, c.lay.h, Q._ptr(J), Q._ptr(r), r_stride, c.eq_lay.h, B, Q._ptr(v), stride, Q._ptr(u), stride,
                                               None, None, C.byref(g), C.c_void_p(work.data_ptr() + base), nbytes, Q._stream())
    torch.cuda.synchronize()
    return rc, L.lib().mo_last_error().decode()


@DTYPES
@pytest.mark.parametrize("r_shared", [False, True], ids=["r_per_problem", "r_shared"])
@pytest.mark.parametrize("off", [1, 0], ids=["misaligned", "aligned"])
def test_strides_and_canaries(off, r_shared, dt):
    """vars_stride = u_stride = V + 3 (NaN in the gap); every output inside a canary-filled buffer at a base off 16 bytes, or aligned; a
    canary behind the workspace.  Nothing beyond the outputs is touched, the results are within the bound, two launches give the same bits."""
    c = Case.get("n33", dt)
    B = 70
    d = data(c, B, dt, 31337, r_shared=r_shared)
    stride = c.V + 3
    wide = lambda a: T(np.concatenate([a, np.full((B, 3), np.nan)], axis=1), dt)
    v, u = wide(d["V"]), wide(d["U"])
    J, r = T(d["J"][None], dt), T(d["R"], dt)
    plan = D._plan_of(c.n, c.k, c.m, 0, dt, dev(), B)
    keys = keys_of(r_shared)
    val, mag = reference(c, d)
    sizes = {"J_blocks": c.lay.values, "r": c.lay.rows, "lam": 1, "J_eq_blocks": c.eq_lay.values, "r_eq": c.k}
    member = {"J_blocks": "dJ_blocks", "r": "dr", "lam": "dlambda", "J_eq_blocks": "dJ_eq_blocks", "r_eq": "dr_eq"}
    runs = []
    for launch in range(2):
        g = L.BlockSharedGrads()
        bufs = {key: Guarded(sizes[key], dt, off) for key in keys}
        for key in keys:
            setattr(g, member[key], bufs[key].view.data_ptr())
        nbytes = C.c_int64()
        r_stride = 0 if r_shared else c.lay.rows
        L.check(L.lib().mo_qp_gradients_blocks_shared_workspace(plan, c.lay.h, c.eq_lay.h, r_stride, B, C.byref(g), C.byref(nbytes)))
        work = torch.full((int(nbytes.value) + 64,), 99, dtype=torch.uint8, device=dev())
        rc, msg = raw_call(c, plan, B, v, u, stride, J, r, r_stride, g, work, int(nbytes.value))
        assert rc == 0, msg
        assert bool(torch.all(work[int(nbytes.value):] == 99)), "workspace overrun"
        got = {}
        for key, b in bufs.items():
            assert b.intact(), key
            a = b.view.double().cpu().numpy()
            got[key] = a[0] if key == "lam" else a
        check_bound(got, val, mag, B, c, dt, keys, "layout: ")
        runs.append(got)
    for key in keys:
        assert np.array_equal(runs[0][key], runs[1][key]), key


# ---- 5. refusals, with a real plan -------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_and_write_nothing():
    dt, B = F64, 40
    c = Case.get("n7", dt)
    d = data(c, B, dt, 12)
    v, u, J, r = T(d["V"], dt), T(d["U"], dt), T(d["J"][None], dt), T(d["R"], dt)
    lib = L.lib()
    plan = D._plan_of(c.n, c.k, c.m, 0, dt, dev(), B)
    out = Guarded(c.lay.values, dt, 0)
    vec = Guarded(c.lay.rows, dt, 0)
    work = torch.empty(1 << 20, dtype=torch.uint8, device=dev())
    rows = c.lay.rows

    def call(g, plan=plan, cost=c.lay.h, eq=c.eq_lay.h, J=J, r=r, r_stride=rows, nbytes=1 << 20, base=0, stride=c.V, refused=True):
        rc = lib.mo_qp_gradients_blocks_shared(plan, cost, Q._ptr(J), Q._ptr(r), r_stride, eq, B, Q._ptr(v), stride, Q._ptr(u), stride, None, None,
                                               C.byref(g), C.c_void_p(work.data_ptr() + base), nbytes, Q._stream())
        torch.cuda.synchronize()
        assert not refused or (bool(torch.all(out.buf == CANARY)) and bool(torch.all(vec.buf == CANARY))), "a refused call wrote"
        return rc, lib.mo_last_error().decode()

    def grads(**kw):
        g = L.BlockSharedGrads()
        for key, val in kw.items():
            setattr(g, key, val.data_ptr())
        return g

    dJ = grads(dJ_blocks=out.view)
    rc, msg = call(grads(dr=vec.view))                                     # dr with an r per problem
    assert rc == -1 and "r_stride" in msg, (rc, msg)
    rc, msg = call(dJ, J=None)                                             # dJ_blocks without J_blocks
    assert rc == -1 and "J_blocks" in msg, (rc, msg)
    rc, msg = call(grads(dr=vec.view), r=None, r_stride=0)                 # dr without r
    assert rc == -1 and "J_blocks / r" in msg, (rc, msg)
    for member in ("dJ_eq_blocks", "dr_eq"):
        rc, msg = call(grads(**{member: out.view}), eq=None)               # an eq member without eq_layout
        assert rc == -1 and "eq_layout" in msg, (rc, msg)
    other = Q.ResidualLayout(c.n + 1, [((0, c.n), 2)], dtype=dt)           # a layout of another n
    rc, msg = call(dJ, cost=other.h)
    assert rc == -2 and "n = " in msg, (rc, msg)
    rc, msg = call(grads(dJ_eq_blocks=out.view), eq=c.lay.h)               # an eq layout whose rows are not the plan's k
    assert rc == -2 and "rows" in msg, (rc, msg)
    rc, msg = call(dJ, stride=c.V - 1)
    assert rc == -2 and "stride" in msg, (rc, msg)
    need = C.c_int64()
    L.check(lib.mo_qp_gradients_blocks_shared_workspace(plan, c.lay.h, c.eq_lay.h, rows, B, C.byref(dJ), C.byref(need)))
    assert 0 < need.value < (1 << 20)
    rc, msg = call(dJ, nbytes=need.value - 1)                              # one byte short
    assert rc == -1 and "workspace" in msg and str(need.value) in msg, (rc, msg)
    rc, msg = call(dJ, base=8)                                             # not 16-byte aligned
    assert rc == -1 and "aligned" in msg, (rc, msg)
    big = Q.ResidualLayout(c.n, [((0, 1), 8200)], dtype=dt)                # (n + 8200) x 8 B of r and u_x per problem: beyond 64 KiB
    rbig = torch.zeros(B, 8200, dtype=dt, device=dev())
    Jbig = torch.zeros(1, big.values, dtype=dt, device=dev())
    rc, msg = call(dJ, cost=big.h, J=Jbig, r=rbig, r_stride=8200)
    assert rc == -3 and "LDS" in msg, (rc, msg)
    rc, msg = call(dJ, nbytes=need.value, refused=False)                   # ... and the exact size is taken
    assert rc == 0, msg
    assert not bool(torch.all(out.view == CANARY))


def test_the_lds_rule_at_its_edge():
    """dJ_blocks with an r per problem, fp64, n = 7: blocks_q_kernel stages the (n + rows) values of one problem beside 64 bytes of flags in
    64 KiB of LDS, so n + rows = 8184 is the largest shape it takes and 8185 the first it refuses.  The largest one runs (B = 3, one problem
    staged at a time) and is within the bound of the float64 sum; the next one is refused by
    the call and by the workspace query alike, with MO_ERR_UNSUPPORTED and nothing written."""
    dt, B, n = F64, 3, 7
    edge = (64 * 1024 - 64) // 8 - n
    plan = D._plan_of(n, 0, 0, 0, dt, dev(), B)
    for rows, fits in ((edge, True), (edge + 1, False)):
        c = Case.__new__(Case)
        c.n, c.cost, c.eq, c.m, c.k, c.V = n, [((2, 5), rows)], None, 0, 0, n
        c.lay, c.eq_lay, c.pmax = Q.ResidualLayout(n, c.cost, dtype=dt), None, 2
        d = data(c, B, dt, 8184)
        v, u, J, r = T(d["V"], dt), T(d["U"], dt), T(d["J"][None], dt), T(d["R"], dt)
        out = Guarded(c.lay.values, dt, 0)
        g = L.BlockSharedGrads()
        g.dJ_blocks = out.view.data_ptr()
        need = C.c_int64(-1)
        rc = L.lib().mo_qp_gradients_blocks_shared_workspace(plan, c.lay.h, None, rows, B, C.byref(g), C.byref(need))
        if not fits:
            assert rc == -3 and b"LDS" in L.lib().mo_last_error() and need.value == -1, (rc, L.lib().mo_last_error())
        else:
            assert rc == 0 and need.value > 0, (rc, L.lib().mo_last_error())
        work = torch.empty(max(int(need.value), 16), dtype=torch.uint8, device=dev())
        rc = L.lib().mo_qp_gradients_blocks_shared(plan, c.lay.h, Q._ptr(J), Q._ptr(r), rows, None, B, Q._ptr(v), c.V, Q._ptr(u), c.V, None, None,
                                                   C.byref(g), C.c_void_p(work.data_ptr()), int(work.numel()), Q._stream())
        msg = L.lib().mo_last_error().decode()
        torch.cuda.synchronize()
        if not fits:
            assert rc == -3 and "LDS" in msg, (rc, msg)
            assert bool(torch.all(out.buf == CANARY)), "a refused call wrote"
            continue
        assert rc == 0, msg
        assert out.intact()
        val, mag = reference(c, d)
        check_bound({"J_blocks": out.view.double().cpu().numpy()}, val, mag, B, c, dt, ("J_blocks",), f"rows={rows}: ")


def test_dense_linearize_still_needs_G_out():
    """Only mo_linearize_blocks forms c without G: the dense mo_linearize refuses a NULL G_out, names it, and writes nothing."""
    dt, B, n, m_r = F64, 3, 7, 9
    rng = np.random.default_rng(9)
    q = Q.BatchedQP(n=n, J=T(rng.normal(size=(B, m_r, n)), dt), r=T(rng.normal(size=(B, m_r)), dt), lam=LAM)
    prob = q.as_struct()
    plan = D._plan_of(n, 0, 0, m_r, dt, dev(), B)
    cc = Guarded(B * n, dt, 0)
    rc = L.lib().mo_linearize(plan, C.byref(prob), B, None, n * n, n, cc.view.data_ptr(), n, None, Q._stream())
    msg = L.lib().mo_last_error().decode()
    torch.cuda.synchronize()
    assert rc == -1 and "G_out" in msg, (rc, msg)
    assert bool(torch.all(cc.buf == CANARY)), "a refused call wrote"


def test_no_allocation_on_the_launch_path():
    """hipMemGetInfo is flat across the FIRST call on a plan (module load and kernel code happen on a twin plan of the same shape first)."""
    dt, B = F64, 300
    c = Case.get("n64", dt)
    d = data(c, B, dt, 13)
    v, u, J, r = T(d["V"], dt), T(d["U"], dt), T(d["J"][None], dt), T(d["R"], dt)
    outs = {key: torch.empty(size, dtype=dt, device=dev()) for key, size in (("dJ_blocks", c.lay.values), ("dlambda", 1), ("dJ_eq_blocks", c.eq_lay.values), ("dr_eq", c.k))}
    g = L.BlockSharedGrads()
    for key, t in outs.items():
        setattr(g, key, t.data_ptr())
    plans = []
    for _ in range(2):
        desc = L.PlanDesc(c.n, c.k, c.m, 0, L.MO_F64, 0, L.EXTRA_PLAN_FLAGS, 0, B)
        plan = C.c_void_p()
        L.check(L.lib().mo_plan_create(C.byref(desc), C.byref(plan)))
        plans.append(plan)
    need = C.c_int64()
    L.check(L.lib().mo_qp_gradients_blocks_shared_workspace(plans[1], c.lay.h, c.eq_lay.h, c.lay.rows, B, C.byref(g), C.byref(need)))
    work = torch.empty(int(need.value), dtype=torch.uint8, device=dev())
    try:
        rc, msg = raw_call(c, plans[0], B, v, u, c.V, J, r, c.lay.rows, g, work, int(need.value))
        assert rc == 0, msg
        free0 = torch.cuda.mem_get_info()[0]
        rc, msg = raw_call(c, plans[1], B, v, u, c.V, J, r, c.lay.rows, g, work, int(need.value))     # the FIRST launches of this plan
        assert rc == 0, msg
        assert torch.cuda.mem_get_info()[0] >= free0 - (1 << 20), (free0, torch.cuda.mem_get_info()[0])
        assert all(bool(torch.all(torch.isfinite(t))) for t in outs.values())
    finally:
        for pl in plans:
            L.lib().mo_plan_destroy(pl)


# ---- 6. mo_linearize_blocks without G_out -------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", ["n7", "n64"])
def test_linearize_blocks_without_G_gives_the_bits_of_the_full_call(name, dt):
    c = Case.get(name, dt)
    B = 19
    rng = np.random.default_rng(66)
    for shared_J in (False, True):
        J, r = T(rng.normal(size=(1 if shared_J else B, c.lay.values)), dt), T(rng.normal(size=(B, c.lay.rows)), dt)
        G, cf, ff = Q.linearize_blocks(c.lay, J, r, lam=LAM)
        none, cc, fc = Q.linearize_blocks(c.lay, J, r, lam=LAM, want_G=False)
        torch.cuda.synchronize()
        assert none is None and torch.equal(cc, cf) and torch.equal(fc, ff) and bool(torch.all(torch.isfinite(G)))


# ---- 7. solve_qp end to end ----------------------------------------------------------------------------------------------------------------------
def bits_equal(a, b):
    """torch.equal on the bit patterns: a failed problem's row may hold NaN, which must be the same NaN."""
    as_int = torch.int64 if a.dtype == F64 else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))


def state_and_adjoint(c_lay, eq_lay, kw, x, s, y, z, status, lam):
    """(V, U, ok) on the host for the loss x.sum(): the state solve_qp returned and the adjoint mo_kkt_solve gives for g = [1 | 0 | 0 | 0] on
    the (G, c) problem of the blocks -- ONE G where J_blocks is given once, c from the call that forms no G."""
    n = c_lay.n
    v = torch.cat([x, s, y, z], dim=1).detach().contiguous()
    g = torch.zeros_like(v)
    g[:, :n] = 1
    J, r = kw["J_blocks"].detach(), kw["r"].detach()
    lam_t = torch.full((1,), float(lam), dtype=v.dtype, device=v.device)
    if int(J.shape[0]) == 1:
        G, _, _ = Q.linearize_blocks(c_lay, J, r[:1], lam_vec=lam_t)
        _, cc, _ = Q.linearize_blocks(c_lay, J, r, lam_vec=lam_t, want_G=False)
    else:
        G, cc, _ = Q.linearize_blocks(c_lay, J, r, lam_vec=lam_t)
    k = 0 if eq_lay is None else eq_lay.rows
    A = None
    if k:
        A, _ = Q.jacobian_blocks(eq_lay, kw["J_eq_blocks"].detach(), kw["r_eq"].detach()[:int(kw["J_eq_blocks"].shape[0])])
    m = int(kw["cons_a"].shape[1]) if "cons_a" in kw else 0
    prob = Q.BatchedQP(n=n, k=k, m=m, G=G, c=cc, A_eq=A, b_eq=kw["r_eq"].detach() if k else None, cons_var=kw.get("cons_var"),
                       cons_a=kw["cons_a"].detach() if m else None, cons_b=kw["cons_b"].detach() if m else None)
    u, adj = D.kkt_solve(prob, v, g, transpose=True)
    ok = ((status == 0) & (adj == 0)).cpu().numpy()
    return v.double().cpu().numpy(), u.double().cpu().numpy(), ok


def test_solve_qp_shared_J_blocks_end_to_end():
    """B = 4096, n = 64, fp64, 96 blocks of 2 x 4, lam = LAM, box rows given once, J_blocks [1, values], r per problem, one problem whose r
    is not finite (its forward fails).  x is bit-equal to the call with J_blocks expanded by the caller; J_blocks.grad is [1, values],
    finite, within the bound of the expanded call's gradient summed in float64 and of the float64 direct sum; the peak allocation over
    forward + backward of the shared call stays below B n n 8 bytes -- one expanded G, which the expanded call necessarily exceeds."""
    n, m, B = 64, 32, 4096
    c = Case.get("n64", F64)
    rng = np.random.default_rng(6464)
    J1 = T(rng.uniform(-1, 1, (1, c.lay.values)))
    r = rng.uniform(-1, 1, (B, c.lay.rows))
    r[7, 5] = np.nan
    r = T(r)
    var = T(np.r_[0:16, 0:16][None], torch.int32)
    a = T(np.r_[np.ones(16), -np.ones(16)][None])
    b = T(np.full((1, m), 0.5))                                # -0.5 <= x_i <= 0.5 for i < 16
    prm = Q.Params(**PARAMS)
    cap = B * n * n * 8
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    Js = J1.clone().requires_grad_(True)
    x, s, y, z, status = D.solve_qp(layout=c.lay, J_blocks=Js, r=r, lam=LAM, cons_var=var, cons_a=a, cons_b=b, params=prm, return_all=True,
                                    return_status=True)
    x.sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"shared call, forward + backward: peak allocation {peak / 2**20:.1f} MiB (one expanded G: {cap / 2**20:.0f} MiB)")
    assert peak < cap, (peak, cap)
    assert int(status[7]) != 0 and int((status != 0).sum()) == 1
    assert tuple(Js.grad.shape) == (1, c.lay.values) and bool(torch.all(torch.isfinite(Js.grad)))
    torch.cuda.reset_peak_memory_stats()
    Je = expand(J1, B).requires_grad_(True)
    xe = D.solve_qp(layout=c.lay, J_blocks=Je, r=r, lam=LAM, cons_var=var, cons_a=a, cons_b=b, params=prm)
    xe.sum().backward()
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() > cap             # what the shared call saves
    assert bits_equal(x, xe)
    assert bool(torch.all(Je.grad[7] == 0))                    # the failed problem contributes exactly nothing
    V, U, ok = state_and_adjoint(c.lay, None, dict(J_blocks=J1, r=r, cons_var=var, cons_a=a, cons_b=b), x, s, y, z, status, LAM)
    assert not ok[7] and ok.sum() == B - 1
    args = (n, 0, m, c.cost, None, J1[0].cpu().numpy(), r.cpu().numpy(), V, U, ok)
    val, mag = BS.direct_batched(*args), BS.direct_batched(*args, absolute=True)
    tol = BS.bound(B, BS.p_max(c.cost), UNIT[F64], mag)["J_blocks"]
    got = Js.grad[0].cpu().numpy()
    for what, ref in (("expanded sum", Je.grad.double().sum(0).cpu().numpy()), ("float64 direct sum", val["J_blocks"])):
        err = np.abs(got - ref)
        print(f"J_blocks.grad vs {what}: max error / bound = {np.max(err / tol):.3e}")
        assert np.all(err <= tol), (what, float(err.max()))


def small_inputs(name, dt, B=33, seed=5):
    """Every input of the block form per problem, well conditioned (lam = LAM), loose box rows: float tensors of `dt`."""
    c = Case.get(name, dt)
    rng = np.random.default_rng(seed + c.n)
    m = 4
    kw = dict(J_blocks=T(rng.uniform(-1, 1, (B, c.lay.values)), dt), r=T(rng.uniform(-1, 1, (B, c.lay.rows)), dt),
              lam=T(np.full(B, LAM), dt), J_eq_blocks=T(rng.uniform(-1, 1, (B, c.eq_lay.values)), dt), r_eq=T(rng.uniform(-0.5, 0.5, (B, c.k)), dt),
              cons_var=T(np.stack([rng.permutation(c.n)[:m] for _ in range(B)]), torch.int32), cons_a=T(rng.choice([-1.0, 1.0], (B, m)), dt),
              cons_b=T(rng.uniform(5.0, 6.0, (B, m)), dt))
    return c, kw


def run_pair(c, kw, once, dt, B):
    """solve_qp(layout=...) with the inputs `once` given once ([1, ...]) and then expanded by the caller: x to the bit; every gradient of
    an input given once is [1, ...], finite and within the bound of the expanded call's gradient summed in float64."""
    prm = Q.Params(**PARAMS)
    res = []
    for expanded in (False, True):
        args = {}
        for key, t in kw.items():
            t = t[:1] if key in once else t
            if t.is_floating_point():
                t = expand(t, B) if expanded and key in once else t.detach().clone()
                t.requires_grad_(key in once)
            elif expanded and key in once:
                t = expand(t, B)
            args[key] = t
        x, s, y, z, status = D.solve_qp(layout=c.lay, eq_layout=c.eq_lay, params=prm, return_all=True, return_status=True, **args)
        good = (status == 0).view(-1, 1)      # (an fp32 solve may fail a problem: it is left out of the loss, and gets zero gradients)
        zero = torch.zeros((), dtype=dt, device=x.device)
        (torch.where(good, x, zero).sum() + (torch.where(good, y, zero) ** 2).sum()).backward()
        res.append((args, x, s, y, z, status))
    (args, x, s, y, z, status), (args_e, xe, _s, _y, _z, status_e) = res
    assert bits_equal(x, xe) and torch.equal(status, status_e)
    # the magnitude of the bound: the adjoint of the loss at the device's own state, from the expanded call's per-problem gradients' inputs
    v = torch.cat([x, s, y, z], dim=1).detach()
    m = int(kw["cons_a"].shape[1])
    g = torch.zeros_like(v)
    g[:, :c.n] = 1
    g[:, c.n + m:c.n + m + c.k] = 2 * y.detach()
    full = {key: (expand(t[:1], B) if key in once else t).detach() for key, t in kw.items()}
    G, cc, _ = Q.linearize_blocks(c.lay, full["J_blocks"], full["r"], lam_vec=full["lam"])
    A, _ = Q.jacobian_blocks(c.eq_lay, full["J_eq_blocks"], full["r_eq"])
    prob = Q.BatchedQP(n=c.n, k=c.k, m=m, G=G, c=cc, A_eq=A, b_eq=full["r_eq"], cons_var=full["cons_var"], cons_a=full["cons_a"], cons_b=full["cons_b"])
    g = torch.where((status == 0).view(-1, 1), g, torch.zeros((), dtype=dt, device=g.device))
    u, adj = D.kkt_solve(prob, v.contiguous(), g, transpose=True)
    ok = ((status == 0) & (adj == 0)).cpu().numpy()
    assert ok.sum() >= B // 2
    Vh, Uh = v.double().cpu().numpy(), u.double().cpu().numpy()
    Jh = kw["J_blocks"][0].double().cpu().numpy()
    Rh = (kw["r"][:1] if "r" in once else kw["r"]).double().cpu().numpy()
    mag = BS.direct(c.n, c.k, m, c.cost, c.eq, Jh, Rh, Vh, Uh, ok, absolute=True)   # (J_blocks / r / lam: read only where J_blocks is given once)
    _, mag_cons = S.direct(c.n, c.k, m, kw["cons_var"][0].cpu().numpy(), Vh, Uh, ok)
    for name in once:
        if not args[name].is_floating_point():
            continue
        gs, ge = args[name].grad, args_e[name].grad
        assert gs is not None and int(gs.shape[0]) == 1 and tuple(gs.shape[1:]) == tuple(ge.shape[1:]) and bool(torch.all(torch.isfinite(gs))), name
        got, ref = gs[0].double().cpu().numpy(), ge.double().sum(0).cpu().numpy()
        assert np.any(ref != 0), name
        if name in mag:
            tol = np.broadcast_to(BS.bound(B, c.pmax, UNIT[dt], mag)[name], got.shape)
        else:   # cons_a, cons_b: the dense form's reduced launch and its bound
            tol = S.bound(B, c.n, UNIT[dt], mag_cons)[name]
        err = np.abs(got - ref)
        print(f"{name}.grad vs expanded sum: max error / bound = {np.max(err / np.maximum(tol, 1e-300)):.3e}")
        assert np.all(err <= tol), (name, float(err.max()))


ONCE = {"J_eq_per_problem_r_eq": ("J_eq_blocks",), "J_eq_and_r_eq": ("J_eq_blocks", "r_eq"), "r_and_J": ("J_blocks", "r", "lam"),
        "lam_per_problem": ("J_blocks",), "constraints": ("cons_var", "cons_a", "cons_b"), "all_but_r_eq": ("J_blocks", "r", "lam", "J_eq_blocks", "cons_var", "cons_a", "cons_b")}


@DTYPES
@pytest.mark.parametrize("which", list(ONCE))
@pytest.mark.parametrize("name", ["n7", "n33"])
def test_solve_qp_blocks_given_once(name, which, dt):
    B = 33
    c, kw = small_inputs(name, dt, B)
    run_pair(c, kw, ONCE[which], dt, B)


@DTYPES
def test_solve_qp_shared_r_with_J_blocks_per_problem_falls_back_to_the_summed_per_problem_result(dt):
    B = 33
    c, kw = small_inputs("n7", dt, B)
    prm = Q.Params(**PARAMS)
    r1 = kw["r"][:1].clone().requires_grad_(True)
    re_ = expand(r1, B).requires_grad_(True)
    rest = {key: t for key, t in kw.items() if key != "r"}
    x = D.solve_qp(layout=c.lay, eq_layout=c.eq_lay, r=r1, params=prm, **rest)
    x.sum().backward()
    xe = D.solve_qp(layout=c.lay, eq_layout=c.eq_lay, r=re_, params=prm, **rest)
    xe.sum().backward()
    assert bits_equal(x, xe) and tuple(r1.grad.shape) == (1, c.lay.rows)
    assert torch.equal(r1.grad[0], re_.grad.sum(0))


@DTYPES
@pytest.mark.parametrize("name", ["n7", "n33"])
def test_forward_mode_with_a_shared_dual_J_blocks(name, dt):
    """torch.autograd.forward_ad: a dual [1, values] J_blocks (never expanded) gives the tangent of the call with J_blocks and its tangent
    expanded by the caller, to the bit."""
    import torch.autograd.forward_ad as fwAD
    B = 33
    c, kw = small_inputs(name, dt, B)
    J1 = kw["J_blocks"][:1].contiguous()
    dJ = T(np.random.default_rng(3).normal(size=(1, c.lay.values)), dt)
    rest = {key: t for key, t in kw.items() if key not in ("J_blocks", "lam")}
    prm = Q.Params(**PARAMS)
    tangents = []
    for expanded in (False, True):
        with fwAD.dual_level():
            Jd = fwAD.make_dual(expand(J1, B) if expanded else J1, expand(dJ, B) if expanded else dJ)
            x = D.solve_qp(layout=c.lay, eq_layout=c.eq_lay, J_blocks=Jd, lam=LAM, params=prm, **rest)
            primal, tangent = fwAD.unpack_dual(x)
            assert tangent is not None and bool(torch.all(torch.isfinite(tangent)))
            tangents.append((primal.clone(), tangent.clone()))
    assert bits_equal(tangents[0][0], tangents[1][0]) and bits_equal(tangents[0][1], tangents[1][1])
    assert bool(torch.any(tangents[0][1] != 0))
