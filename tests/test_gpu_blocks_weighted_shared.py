"""GPU tests of the batch-reduced block gradients under per-row weights (run with -m gpu on an MI355X): mo_qp_gradients_blocks_weighted_shared
against the float64 sums of tests/blocks_weighted_shared_reference.py and against the host sum of mo_qp_gradients_blocks_weighted's
per-problem outputs, and solve_qp(layout=..., weights=..., reduce_in_kernel=True).

The bound is derived by counting roundings (blocks_weighted_shared_reference.bound): an element whose exact value is a sum of terms may be
off by 1.01 (2 B + 4 P_max + 8) UNIT[dtype] sum |terms|; the reference is numpy float64 on the inputs as the device holds them (fp32
inputs promoted)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from mini_opt_amd import _lib as L
from mini_opt_amd import diff as D
from mini_opt_amd import qp as Q
from tests import blocks_weighted_shared_reference as WS
from tests.sens_fixtures import CANARY, LAM, N7_COST, PARAMS, UNIT, Guarded, T, autograd_layout, cus, dev, expand, random_layout

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
NPDT = {F64: np.float64, F32: np.float32}
DTYPES = pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
SHARING = [(False, False), (True, False), (False, True), (True, True)]      # (r given once, weights given once)
MEMBER = {"J_blocks": "dJ_blocks", "r": "dr", "lam": "dlambda", "weights": "dweights"}
PER_GROUP = 2048   # packed values one workgroup of the partial kernel owns


class Case:
    """A cost layout and m inequality rows (which only widen the state): "n7" N7_COST, which names a variable twice in two blocks; "n33" a
    random layout with repeats; "n64" 96 blocks of 2 x 4; "big" n = 40, more packed values than one workgroup owns; "wide" blocks of 9 to
    12 columns, one of them with a repeat."""
    _made = {}

    def __init__(self, name, dt):
        rng = np.random.default_rng({"n7": 72, "n33": 332, "n64": 642, "big": 402, "wide": 202}[name])
        if name == "n7":
            self.n, self.cost, self.m = 7, N7_COST, 3
        elif name == "n33":
            self.n, self.cost, self.m = 33, random_layout(rng, 33, 14, repeats=True), 2
            assert any(len(set(idx)) < len(idx) for idx, _ in self.cost)
        elif name == "n64":
            self.n, self.cost, self.m = 64, autograd_layout(64, rng), 0
        elif name == "big":
            self.n, self.cost, self.m = 40, [(tuple(int(i) for i in rng.permutation(40)[:6]), 5) for _ in range(75)] + [((3, 9, 3), 4)], 1
        else:
            self.n, self.m = 20, 0
            self.cost = [(tuple(int(i) for i in rng.permutation(20)[:P]), R_) for P, R_ in ((9, 2), (12, 3), (11, 1))]
            self.cost.append(((4, 0, 7, 19, 4, 2, 11, 13, 5, 8), 2))
        self.k, self.V = 0, self.n + 2 * self.m
        self.lay = Q.ResidualLayout(self.n, self.cost, dtype=dt)
        self.pmax = WS.p_max(self.cost)

    @classmethod
    def get(cls, name, dt):
        if (name, dt) not in cls._made:
            cls._made[(name, dt)] = cls(name, dt)
        return cls._made[(name, dt)]


def data(c, B, dt, seed, integer=False, r_shared=False, w_shared=False):
    """vars, u [B, V], ONE J [values], r and weights [B or 1, rows] in the values the device will hold (float64 arrays of dt-representable
    numbers).  Integer data: weights in {0, ..., 3}, everything else in {-2, ..., 2}."""
    rng = np.random.default_rng(seed)
    draw = (lambda *s: rng.integers(-2, 3, s).astype(np.float64)) if integer else (lambda *s: rng.normal(size=s).astype(NPDT[dt]).astype(np.float64))
    wB = 1 if w_shared else B
    Wt = rng.integers(0, 4, (wB, c.lay.rows)).astype(np.float64) if integer else rng.uniform(0.25, 2.0, (wB, c.lay.rows)).astype(NPDT[dt]).astype(np.float64)
    return dict(V=draw(B, c.V), U=draw(B, c.V), J=draw(c.lay.values), R=draw(1 if r_shared else B, c.lay.rows), Wt=Wt)


def keys_of(r_shared, w_shared):
    return ("J_blocks", "lam") + (("r",) if r_shared else ()) + (("weights",) if w_shared else ())


def status_words(ok):
    return None if ok is None else T(np.where(ok, 0, 2), torch.int32)


def host(out):
    return {key: (t.double().cpu().numpy().reshape(-1)[0] if key == "lam" else t[0].double().cpu().numpy()) for key, t in out.items()}


def shared(c, d, dt, want, ok_fwd=None, ok_adj=None):
    out = D.qp_gradients_blocks_weighted_shared(c.lay, T(d["J"][None], dt), T(d["R"], dt), T(d["Wt"], dt), T(d["V"], dt), T(d["U"], dt), m=c.m,
                                                want=want, status_fwd=status_words(ok_fwd), status_adj=status_words(ok_adj))
    torch.cuda.synchronize()
    for key, t in out.items():
        assert int(t.shape[0]) == 1, key
    return host(out)


def reference(c, d, ok=None):
    """(value, magnitude): the float64 direct sum over the counted problems and the same sum of absolute values."""
    ok = np.ones(len(d["V"]), dtype=bool) if ok is None else ok
    args = (c.n, c.cost, d["J"], d["R"], d["Wt"], d["V"], d["U"], ok)
    return WS.direct(*args), WS.direct(*args, absolute=True)


def check_bound(got, val, mag, B, c, dt, keys, what=""):
    tol = WS.bound(B, c.pmax, UNIT[dt], mag)
    for key in keys:
        err = np.abs(got[key] - val[key])
        ratio = float(np.max(err / np.maximum(tol[key], np.finfo(np.float64).tiny)))
        print(f"{what}{key}: max error / bound = {ratio:.3e}")
        assert np.all(np.isfinite(got[key])) and np.all(err <= tol[key]), (what, key, float(np.max(err)), ratio)


def per_problem_sum(c, d, dt, keys):
    """The float64 host sum of mo_qp_gradients_blocks_weighted's per-problem outputs."""
    each = D.qp_gradients_blocks_weighted(c.lay, T(d["J"][None], dt), T(d["R"], dt), T(d["Wt"], dt), T(d["V"], dt), T(d["U"], dt), m=c.m, want=keys)
    return {key: (float(t.double().sum()) if key == "lam" else t.double().sum(0).cpu().numpy()) for key, t in each.items()}


# ---- 1. the gathers, exactly ---------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", ["n7", "n33", "n64"])
def test_integer_data_gives_the_integer_result(name, dt):
    """Integers in vars, u, J_blocks, r and the weights (zeros among them), B = 256: every intermediate is below 2^22 for P_b <= 8, so
    every output is exact in both dtypes and must EQUAL the float64 result -- a wrong schedule entry, partner list or pair list cannot hide
    in a tolerance."""
    c = Case.get(name, dt)
    B = 256
    for r_shared, w_shared in SHARING:
        d = data(c, B, dt, 100 + c.n, integer=True, r_shared=r_shared, w_shared=w_shared)
        keys = keys_of(r_shared, w_shared)
        val, _ = reference(c, d)
        got = shared(c, d, dt, keys)
        for key in keys:
            assert np.shape(got[key]) == np.shape(val[key]) and np.array_equal(got[key], val[key]), (key, r_shared, w_shared)


# ---- 2. random data within the derived bound -----------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("B", [1, 5, 33, 37, 4096 + 17])
@pytest.mark.parametrize("name", ["n33", "n64"])
def test_random_data_against_the_float64_sum(name, B, dt):
    """B = 1, 5 (one partial stage), 33 (a chunk boundary: 32 + 1), 37 (two chunks, the stages of both partial) and 4096 + 17 (many chunks,
    a short last one), all four sharing combinations of r and the weights: within the bound of the float64 direct sum, and within the same
    bound of the float64 host sum of the per-problem kernel's outputs."""
    c = Case.get(name, dt)
    if B == 33:
        assert WS.chunks(B, cus()) == 2
    for r_shared, w_shared in SHARING:
        d = data(c, B, dt, 7 * c.n + B, r_shared=r_shared, w_shared=w_shared)
        keys = keys_of(r_shared, w_shared)
        val, mag = reference(c, d)
        got = shared(c, d, dt, keys)
        what = f"B={B} r{'1' if r_shared else 'B'} w{'1' if w_shared else 'B'} "
        check_bound(got, val, mag, B, c, dt, keys, what + "vs float64: ")
        check_bound(got, per_problem_sum(c, d, dt, keys), mag, B, c, dt, keys, what + "vs per-problem sum: ")


# ---- 3., 4. more values than a workgroup owns; blocks of more than eight columns -------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", ["big", "wide"])
def test_many_values_and_wide_blocks(name, dt):
    c = Case.get(name, dt)
    if name == "big":
        assert c.lay.values > PER_GROUP and c.lay.values % PER_GROUP != 0      # two value-groups per chunk, the second one partial
    else:
        assert c.pmax > 8
    B = 70
    for integer in (True, False):
        d = data(c, B, dt, 11 + c.n, integer=integer, r_shared=True, w_shared=True)
        keys = keys_of(True, True)
        val, mag = reference(c, d)
        got = shared(c, d, dt, keys)
        if integer:
            for key in keys:
                assert np.array_equal(got[key], val[key]), key
        else:
            check_bound(got, val, mag, B, c, dt, keys, f"{name}: ")


# ---- 5. each member alone ------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", ["n7", "n33"])
def test_each_member_alone_and_two_launches(name, dt):
    """Every output asked for alone, all other members NULL: the bound, and the bits of the call that asks for all of them; a second launch
    of that call repeats its bits."""
    c = Case.get(name, dt)
    B = 37
    d = data(c, B, dt, 5151, r_shared=True, w_shared=True)
    keys = keys_of(True, True)
    val, mag = reference(c, d)
    every, again = shared(c, d, dt, keys), shared(c, d, dt, keys)
    for key in keys:
        assert np.array_equal(every[key], again[key]), key
        alone = shared(c, d, dt, (key,))
        assert set(alone) == {key}
        check_bound(alone, val, mag, B, c, dt, (key,), "alone: ")
        assert np.array_equal(alone[key], every[key]), key


# ---- 6. masked problems and zero weights ---------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", ["n7", "n33"])
def test_masked_problems_and_zero_weights_contribute_nothing(name, dt):
    """Every fifth problem, the first and the last of the batch and the first of the second stage carry status 2 in status_fwd or in
    status_adj (alternating) and NaN in their rows of vars, u, r and the weights; among the counting problems one weight in seven is
    exactly 0 and r holds NaN there.  One chunk (B = 30): finite, within the bound, and to the bit the call on the batch with the masked
    problems removed.  Many chunks (B = 4096 + 17): within the bound.  Every problem masked: exact zeros."""
    c = Case.get(name, dt)
    keys = keys_of(False, False)
    for B in (30, 4096 + 17):
        d = data(c, B, dt, 900 + B)
        bad = np.arange(B) % 5 == 3
        bad[[0, 16, B - 1]] = True
        flip = np.arange(B) % 2 == 0
        ok_fwd, ok_adj = ~(bad & flip), ~(bad & ~flip)
        assert np.array_equal(ok_fwd & ok_adj, ~bad)
        zero = np.random.default_rng(B).random(d["Wt"].shape) < 1.0 / 7
        d["Wt"][zero] = 0.0
        d["R"][zero] = np.nan
        for key in ("V", "U", "R", "Wt"):
            d[key][bad] = np.nan
        got = shared(c, d, dt, keys, ok_fwd, ok_adj)
        val, mag = reference(c, d, ok=~bad)
        check_bound(got, val, mag, B, c, dt, keys, f"masked B={B}: ")
        if B == 30:
            assert WS.chunks(B, cus()) == 1
            kept = {key: (a if key == "J" else a[~bad]) for key, a in d.items()}
            without = shared(c, kept, dt, keys)
            for key in keys:
                assert np.array_equal(got[key], without[key]), key
    got = shared(c, d, dt, keys, np.zeros(B, dtype=bool), None)
    for key in keys:
        assert np.all(got[key] == 0), key


# ---- 7. the empty batch --------------------------------------------------------------------------------------------------------------------
def raw_call(c, plan, B, v, u, stride, J, r, r_stride, w, w_stride, g, work, nbytes, base=0):
    rc = L.lib().mo_qp_gradients_blocks_weighted_shared(plan, c.lay.h, Q._ptr(J), Q._ptr(r), r_stride, Q._ptr(w), w_stride, B, Q._ptr(v), stride,
                                                        Q._ptr(u), stride, None, None, C.byref(g), C.c_void_p(work.data_ptr() + base), nbytes,
                                                        Q._stream())
    torch.cuda.synchronize()
    return rc, L.lib().mo_last_error().decode()


def test_empty_batch_writes_zeros():
    """batch = 0 through the front end (r and the weights given once, every member) and through the C ABI with r and weights per problem:
    r, the weights, vars and u point at one row that no kernel may read (NaN).  Exact zeros, nothing beyond the outputs touched."""
    dt = F64
    c = Case.get("n7", dt)
    d = data(c, 0, dt, 1, r_shared=True, w_shared=True)
    got = shared(c, d, dt, keys_of(True, True))
    for key, a in got.items():
        assert np.all(a == 0), key
    nan_row = lambda size: torch.full((1, size), float("nan"), dtype=dt, device=dev())
    v, u, r, w = nan_row(c.V), nan_row(c.V), nan_row(c.lay.rows), nan_row(c.lay.rows)
    J = torch.ones(1, c.lay.values, dtype=dt, device=dev())
    plan = D._plan_of(c.n, c.k, c.m, 0, dt, dev(), 1)
    bufs = {"dJ_blocks": Guarded(c.lay.values, dt), "dlambda": Guarded(1, dt)}
    g = L.BlockWeightedSharedGrads()
    for member, b in bufs.items():
        setattr(g, member, b.view.data_ptr())
    nbytes = C.c_int64()
    L.check(L.lib().mo_qp_gradients_blocks_weighted_shared_workspace(plan, c.lay.h, c.lay.rows, c.lay.rows, 0, C.byref(g), C.byref(nbytes)))
    work = torch.full((int(nbytes.value) + 64,), 99, dtype=torch.uint8, device=dev())
    rc, msg = raw_call(c, plan, 0, v, u, c.V, J, r, c.lay.rows, w, c.lay.rows, g, work, int(nbytes.value))
    assert rc == 0, msg
    assert bool(torch.all(work[int(nbytes.value):] == 99)), "workspace overrun"
    for member, b in bufs.items():
        assert b.intact() and bool(torch.all(b.view == 0)), member


# ---- 8. strides, misaligned bases, canaries -------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("r_shared,w_shared", SHARING, ids=["r_w_per_problem", "r_once", "w_once", "r_w_once"])
@pytest.mark.parametrize("off", [1, 0], ids=["misaligned", "aligned"])
def test_strides_and_canaries(off, r_shared, w_shared, dt):
    """vars_stride = u_stride = V + 3, r_stride = rows + 2, weights_stride = rows + 5 (NaN in every gap); every output inside a
    canary-filled buffer at a base off 16 bytes, or aligned; a canary behind the workspace.  Nothing beyond the outputs is touched, the
    results are within the bound, two launches give the same bits."""
    c = Case.get("n33", dt)
    B = 70
    d = data(c, B, dt, 31338, r_shared=r_shared, w_shared=w_shared)
    wide = lambda a, extra: T(np.concatenate([a, np.full((len(a), extra), np.nan)], axis=1), dt)
    v, u = wide(d["V"], 3), wide(d["U"], 3)
    J, r, w = T(d["J"][None], dt), wide(d["R"], 2), wide(d["Wt"], 5)
    r_stride, w_stride = (0 if r_shared else c.lay.rows + 2), (0 if w_shared else c.lay.rows + 5)
    plan = D._plan_of(c.n, c.k, c.m, 0, dt, dev(), B)
    keys = keys_of(r_shared, w_shared)
    val, mag = reference(c, d)
    sizes = {"J_blocks": c.lay.values, "r": c.lay.rows, "lam": 1, "weights": c.lay.rows}
    runs = []
    for launch in range(2):
        g = L.BlockWeightedSharedGrads()
        bufs = {key: Guarded(sizes[key], dt, off) for key in keys}
        for key in keys:
            setattr(g, MEMBER[key], bufs[key].view.data_ptr())
        nbytes = C.c_int64()
        L.check(L.lib().mo_qp_gradients_blocks_weighted_shared_workspace(plan, c.lay.h, r_stride, w_stride, B, C.byref(g), C.byref(nbytes)))
        work = torch.full((int(nbytes.value) + 64,), 99, dtype=torch.uint8, device=dev())
        rc, msg = raw_call(c, plan, B, v, u, c.V + 3, J, r, r_stride, w, w_stride, g, work, int(nbytes.value))
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


# ---- 9. refusals, with a real plan ----------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_and_write_nothing():
    dt, B = F64, 40
    c = Case.get("n7", dt)
    d = data(c, B, dt, 12)
    v, u, J, r, w = T(d["V"], dt), T(d["U"], dt), T(d["J"][None], dt), T(d["R"], dt), T(d["Wt"], dt)
    lib = L.lib()
    plan = D._plan_of(c.n, c.k, c.m, 0, dt, dev(), B)
    out = Guarded(c.lay.values, dt, 0)
    vec = Guarded(c.lay.rows, dt, 0)
    work = torch.empty(1 << 20, dtype=torch.uint8, device=dev())
    rows = c.lay.rows

    def call(g, plan=plan, cost=c.lay.h, J=J, r=r, w=w, r_stride=rows, w_stride=rows, nbytes=1 << 20, base=0, stride=c.V, refused=True):
        ref = None if g is None else C.byref(g)
        rc = lib.mo_qp_gradients_blocks_weighted_shared(plan, cost, Q._ptr(J), Q._ptr(r), r_stride, Q._ptr(w), w_stride, B, Q._ptr(v), stride,
                                                        Q._ptr(u), stride, None, None, ref, C.c_void_p(work.data_ptr() + base), nbytes, Q._stream())
        torch.cuda.synchronize()
        assert not refused or (bool(torch.all(out.buf == CANARY)) and bool(torch.all(vec.buf == CANARY))), "a refused call wrote"
        return rc, lib.mo_last_error().decode()

    def grads(**kw):
        g = L.BlockWeightedSharedGrads()
        for key, val in kw.items():
            setattr(g, key, val.data_ptr())
        return g

    dJ = grads(dJ_blocks=out.view)
    rc, msg = call(dJ, cost=None)
    assert rc == -1 and "cost_layout" in msg, (rc, msg)
    rc, msg = call(None)
    assert rc == -1 and "out" in msg, (rc, msg)
    rc, msg = call(dJ, J=None)
    assert rc == -1 and "J_blocks" in msg, (rc, msg)
    rc, msg = call(dJ, r=None)
    assert rc == -1 and "J_blocks / r" in msg, (rc, msg)
    rc, msg = call(dJ, w=None)
    assert rc == -1 and "weights" in msg, (rc, msg)
    rc, msg = call(grads(dr=vec.view))                                     # dr with an r per problem
    assert rc == -1 and "r_stride" in msg, (rc, msg)
    rc, msg = call(grads(dweights=vec.view))                               # dweights with weights per problem
    assert rc == -1 and "weights_stride" in msg, (rc, msg)
    other = Q.ResidualLayout(c.n + 1, [((0, c.n), 2)], dtype=dt)           # a layout of another n
    rc, msg = call(dJ, cost=other.h)
    assert rc == -2 and "n = " in msg, (rc, msg)
    rc, msg = call(dJ, stride=c.V - 1)
    assert rc == -2 and "stride" in msg, (rc, msg)
    need = C.c_int64()
    L.check(lib.mo_qp_gradients_blocks_weighted_shared_workspace(plan, c.lay.h, rows, rows, B, C.byref(dJ), C.byref(need)))
    assert 0 < need.value < (1 << 20)
    rc, msg = call(dJ, nbytes=need.value - 1)                              # one byte short
    assert rc == -1 and "workspace" in msg and str(need.value) in msg, (rc, msg)
    rc, msg = call(dJ, base=8)                                             # not 16-byte aligned
    assert rc == -1 and "aligned" in msg, (rc, msg)
    big = Q.ResidualLayout(c.n, [((0, 1), 4100)], dtype=dt)                # (2 n + 2 x 4100) x 8 B per staged problem: beyond 64 KiB
    rbig = torch.zeros(B, 4100, dtype=dt, device=dev())
    Jbig = torch.zeros(1, big.values, dtype=dt, device=dev())
    rc, msg = call(dJ, cost=big.h, J=Jbig, r=rbig, w=rbig, r_stride=4100, w_stride=4100)
    assert rc == -3 and "LDS" in msg, (rc, msg)
    rc, msg = call(dJ, nbytes=need.value, refused=False)                   # ... and the exact size is taken
    assert rc == 0, msg
    assert not bool(torch.all(out.view == CANARY))
    with pytest.raises(ValueError, match="r \\[1, rows\\]"):
        D.qp_gradients_blocks_weighted_shared(c.lay, J, r, w, v, u, m=c.m, want=("r",))
    with pytest.raises(ValueError, match="weights \\[1, rows\\]"):
        D.qp_gradients_blocks_weighted_shared(c.lay, J, r, w, v, u, m=c.m, want=("weights",))


# ---- 10. the LDS rule at its edge -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("member", ["dJ_blocks", "dweights"])
def test_the_lds_rule_at_its_edge(member):
    """fp64, n = 7: one staged problem is 2 n + 2 rows values (rows more with dweights: s t) beside 64 bytes of flags in 64 KiB of LDS, so
    rows = 4085 (2723 with dweights) is the largest shape the launch takes and the next one the first it refuses.  The largest one runs
    (B = 3, one problem staged at a time, four value-groups per chunk) and is within the bound of the float64 sum; the next one is refused
    by the call and by the workspace query alike, with MO_ERR_UNSUPPORTED and nothing written."""
    dt, B, n = F64, 3, 7
    per_row = 3 if member == "dweights" else 2
    edge = ((64 * 1024 - 64) // 8 - 2 * n) // per_row
    assert edge == (2723 if member == "dweights" else 4085)
    plan = D._plan_of(n, 0, 0, 0, dt, dev(), B)
    key = "weights" if member == "dweights" else "J_blocks"
    for rows, fits in ((edge, True), (edge + 1, False)):
        c = Case.__new__(Case)
        c.n, c.cost, c.m, c.k, c.V = n, [((2, 5), rows)], 0, 0, n
        c.lay, c.pmax = Q.ResidualLayout(n, c.cost, dtype=dt), 2
        d = data(c, B, dt, 8184, w_shared=member == "dweights")
        v, u, J, r, w = T(d["V"], dt), T(d["U"], dt), T(d["J"][None], dt), T(d["R"], dt), T(d["Wt"], dt)
        w_stride = 0 if member == "dweights" else rows
        out = Guarded(rows if member == "dweights" else c.lay.values, dt, 0)
        g = L.BlockWeightedSharedGrads()
        setattr(g, member, out.view.data_ptr())
        need = C.c_int64(-1)
        rc = L.lib().mo_qp_gradients_blocks_weighted_shared_workspace(plan, c.lay.h, rows, w_stride, B, C.byref(g), C.byref(need))
        if not fits:
            assert rc == -3 and b"LDS" in L.lib().mo_last_error() and need.value == -1, (rc, L.lib().mo_last_error())
        else:
            assert rc == 0 and need.value > 0, (rc, L.lib().mo_last_error())
        work = torch.empty(max(int(need.value), 16), dtype=torch.uint8, device=dev())
        rc, msg = raw_call(c, plan, B, v, u, c.V, J, r, rows, w, w_stride, g, work, int(work.numel()))
        if not fits:
            assert rc == -3 and "LDS" in msg, (rc, msg)
            assert bool(torch.all(out.buf == CANARY)), "a refused call wrote"
            continue
        assert rc == 0, msg
        assert out.intact()
        val, mag = reference(c, d)
        check_bound({key: out.view.double().cpu().numpy()}, val, mag, B, c, dt, (key,), f"rows={rows}: ")


# ---- 11. no allocation on the launch path ---------------------------------------------------------------------------------------------------
def test_no_allocation_on_the_launch_path():
    """hipMemGetInfo is flat across the FIRST call on a plan (module load and kernel code happen on a twin plan of the same shape first)."""
    dt, B = F64, 300
    c = Case.get("n64", dt)
    d = data(c, B, dt, 13)
    v, u, J, r, w = T(d["V"], dt), T(d["U"], dt), T(d["J"][None], dt), T(d["R"], dt), T(d["Wt"], dt)
    outs = {key: torch.empty(size, dtype=dt, device=dev()) for key, size in (("dJ_blocks", c.lay.values), ("dlambda", 1))}
    g = L.BlockWeightedSharedGrads()
    for key, t in outs.items():
        setattr(g, key, t.data_ptr())
    plans = []
    for _ in range(2):
        desc = L.PlanDesc(c.n, c.k, c.m, 0, L.MO_F64, 0, L.EXTRA_PLAN_FLAGS, 0, B)
        plan = C.c_void_p()
        L.check(L.lib().mo_plan_create(C.byref(desc), C.byref(plan)))
        plans.append(plan)
    rows = c.lay.rows
    need = C.c_int64()
    L.check(L.lib().mo_qp_gradients_blocks_weighted_shared_workspace(plans[1], c.lay.h, rows, rows, B, C.byref(g), C.byref(need)))
    work = torch.empty(int(need.value), dtype=torch.uint8, device=dev())
    try:
        rc, msg = raw_call(c, plans[0], B, v, u, c.V, J, r, rows, w, rows, g, work, int(need.value))
        assert rc == 0, msg
        free0 = torch.cuda.mem_get_info()[0]
        rc, msg = raw_call(c, plans[1], B, v, u, c.V, J, r, rows, w, rows, g, work, int(need.value))     # the FIRST launches of this plan
        assert rc == 0, msg
        assert torch.cuda.mem_get_info()[0] >= free0 - (1 << 20), (free0, torch.cuda.mem_get_info()[0])
        assert all(bool(torch.all(torch.isfinite(t))) for t in outs.values())
    finally:
        for pl in plans:
            L.lib().mo_plan_destroy(pl)


# ---- 12. solve_qp end to end: bits and bound ------------------------------------------------------------------------------------------------
def bits_equal(a, b):
    """torch.equal on the bit patterns: a failed problem's row may hold NaN, which must be the same NaN."""
    as_int = torch.int64 if a.dtype == F64 else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))


def small_inputs(name, dt, B=33, seed=5):
    """ONE J_blocks, r and weights per problem, well conditioned (lam = LAM), four loose box rows per problem."""
    c = Case.get(name, dt)
    rng = np.random.default_rng(seed + c.n)
    m = 4
    kw = dict(J_blocks=T(rng.uniform(-1, 1, (1, c.lay.values)), dt), r=T(rng.uniform(-1, 1, (B, c.lay.rows)), dt),
              weights=T(rng.uniform(0.25, 2.0, (B, c.lay.rows)), dt),
              cons_var=T(np.stack([rng.permutation(c.n)[:m] for _ in range(B)]), torch.int32), cons_a=T(rng.choice([-1.0, 1.0], (B, m)), dt),
              cons_b=T(rng.uniform(5.0, 6.0, (B, m)), dt))
    return c, kw, m


def run_solve(c, kw, leaves, dt, lam_count=1, **flags):
    """solve_qp on fresh leaves of the float inputs named in `leaves` and of lam [lam_count]; the loss is the sum of x over the problems
    that solved.  Returns (leaves, x, s, y, z, status)."""
    args = {key: (t.detach().clone().requires_grad_(key in leaves) if t.is_floating_point() else t) for key, t in kw.items()}
    lam = T(np.full(lam_count, LAM), dt).requires_grad_(True)
    x, s, y, z, status = D.solve_qp(layout=c.lay, lam=lam, params=Q.Params(**PARAMS), return_all=True, return_status=True, **args, **flags)
    good = (status == 0).view(-1, 1)
    torch.where(good, x, torch.zeros((), dtype=dt, device=x.device)).sum().backward()
    args["lam"] = lam
    return args, x, s, y, z, status


def check_end_to_end(c, kw, m, once, dt, B, fails=()):
    """reduce_in_kernel=True against the default route and against the call with every input expanded by the caller."""
    kw = {key: (t[:1].contiguous() if key in once else t) for key, t in kw.items()}
    leaves = ("J_blocks", "r", "weights")
    red, x, s, y, z, status = run_solve(c, kw, leaves, dt, reduce_in_kernel=True)
    dfl, xd, _, _, _, status_d = run_solve(c, kw, leaves, dt)
    exp, xe, _, _, _, status_e = run_solve(c, {key: (expand(t, B) if t.is_floating_point() else t) for key, t in kw.items()}, leaves, dt,
                                           lam_count=B)
    assert bits_equal(x, xd) and bits_equal(x, xe) and torch.equal(status, status_d) and torch.equal(status, status_e)
    for p in fails:
        assert int(status[p]) != 0
    assert int((status != 0).sum()) == len(fails) or dt == F32
    per_problem = [key for key in ("r", "weights") if key not in once]
    for key in per_problem:      # the members given per problem: the per-problem launch without dJ_blocks gives the default route's bits
        assert tuple(red[key].grad.shape) == (B, c.lay.rows) and bits_equal(red[key].grad, dfl[key].grad), key
        for p in fails:
            assert bool(torch.all(red[key].grad[p] == 0)), key
    # the bound's magnitude from the device's own state and adjoint
    v = torch.cat([x, s, y, z], dim=1).detach().contiguous()
    g = torch.zeros_like(v)
    g[:, :c.n] = 1
    g = torch.where((status == 0).view(-1, 1), g, torch.zeros((), dtype=dt, device=g.device))
    full = {key: expand(t, B) for key, t in kw.items()}
    G, cc, _ = Q.linearize_blocks(c.lay, kw["J_blocks"], full["r"], lam_vec=T(np.full(B, LAM), dt), batch=B, weights=full["weights"])
    prob = Q.BatchedQP(n=c.n, k=0, m=m, G=G, c=cc, cons_var=full["cons_var"], cons_a=full["cons_a"], cons_b=full["cons_b"])
    u, adj = D.kkt_solve(prob, v, g, transpose=True)
    ok = ((status == 0) & (adj == 0)).cpu().numpy()
    assert ok.sum() >= B // 2 and not any(ok[p] for p in fails)
    hostf = lambda t: t.double().cpu().numpy()
    mag = WS.direct(c.n, c.cost, hostf(kw["J_blocks"][0]), hostf(kw["r"]), hostf(kw["weights"]), hostf(v), hostf(u), ok, absolute=True)
    tol = WS.bound(B, c.pmax, UNIT[dt], mag)
    for key in ("J_blocks", "lam") + tuple(once):
        gs, ge = red[key].grad, exp[key].grad
        assert gs is not None and int(gs.shape[0]) == 1 and int(ge.shape[0]) == B and bool(torch.all(torch.isfinite(gs))), key
        got, ref = hostf(gs).reshape(-1), hostf(ge).reshape(B, -1).sum(0)
        assert np.any(ref != 0), key
        err = np.abs(got - ref)
        bound = np.broadcast_to(np.asarray(tol[key]), got.shape)
        print(f"{key}.grad vs expanded sum: max error / bound = {np.max(err / np.maximum(bound, 1e-300)):.3e}")
        assert np.all(err <= bound), (key, float(err.max()))


@DTYPES
@pytest.mark.parametrize("once", [(), ("weights",), ("r",)], ids=["r_w_per_problem", "w_once", "r_once"])
@pytest.mark.parametrize("name", ["n7", "n33"])
def test_solve_qp_reduce_in_kernel_end_to_end(name, once, dt):
    """J_blocks [1, values], weights [B, rows], r [B, rows] at B = 33 (then weights [1, rows], then r [1, rows]): x to the bit the default
    call's and the expanded call's; r.grad and weights.grad per problem to the bit the default route's; J_blocks.grad, lam.grad and the
    gradients of what is given once are [1, ...], finite and within the bound of the expanded call's gradients summed in float64."""
    B = 33
    c, kw, m = small_inputs(name, dt, B)
    check_end_to_end(c, kw, m, once, dt, B)


def test_solve_qp_reduce_in_kernel_failing_problem_contributes_nothing():
    """One problem whose forward fails on purpose (a constraint index outside [0, n): MO_STATUS_BAD_INDEX) inside a healthy batch."""
    dt, B = F64, 33
    c, kw, m = small_inputs("n7", dt, B)
    var = kw["cons_var"].clone()
    var[17, 1] = c.n + 1
    kw["cons_var"] = var
    check_end_to_end(c, kw, m, (), dt, B, fails=(17,))


def test_reduce_in_kernel_changes_nothing_with_J_blocks_per_problem():
    dt, B = F64, 9
    c, kw, m = small_inputs("n7", dt, B)
    kw["J_blocks"] = expand(kw["J_blocks"], B)
    a, xa, *_ = run_solve(c, kw, ("J_blocks", "r", "weights"), dt, reduce_in_kernel=True)
    b, xb, *_ = run_solve(c, kw, ("J_blocks", "r", "weights"), dt)
    assert bits_equal(xa, xb)
    for key in ("J_blocks", "r", "weights", "lam"):
        assert bits_equal(a[key].grad, b[key].grad), key


# ---- 13. solve_qp end to end: memory ---------------------------------------------------------------------------------------------------------
def test_solve_qp_reduce_in_kernel_forms_no_per_problem_packed_gradient():
    """B = 4096, n = 64, 96 blocks of 2 x 4 (values = 768 >> V), only J_blocks asks for a gradient: over the backward the peak allocation
    rises by less than B x values x 8 bytes with the flag, and by at least that on the default route, which writes the [B, values]
    gradient."""
    dt, B = F64, 4096
    c = Case.get("n64", dt)
    rng = np.random.default_rng(6465)
    J1 = T(rng.uniform(-1, 1, (1, c.lay.values)))
    r, w = T(rng.uniform(-1, 1, (B, c.lay.rows))), T(rng.uniform(0.25, 2.0, (B, c.lay.rows)))
    packed = B * c.lay.values * 8
    rise = {}
    for flag in (True, False):
        Js = J1.clone().requires_grad_(True)
        x = D.solve_qp(layout=c.lay, J_blocks=Js, r=r, lam=LAM, weights=w, params=Q.Params(**PARAMS), reduce_in_kernel=flag)
        loss = x.sum()
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss.backward()
        torch.cuda.synchronize()
        rise[flag] = torch.cuda.max_memory_allocated() - before
        assert tuple(Js.grad.shape) == (1, c.lay.values) and bool(torch.all(torch.isfinite(Js.grad)))
    print(f"backward, rise of the peak allocation: reduce_in_kernel {rise[True] / 2**20:.1f} MiB, default {rise[False] / 2**20:.1f} MiB "
          f"(one [B, values] gradient: {packed / 2**20:.1f} MiB)")
    assert rise[True] < packed <= rise[False], (rise, packed)
