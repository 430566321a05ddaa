"""The problem hand-out of the fused kernels (the queue_* functions of csrc/mo_fused_device.h) in every kernel that uses it.

The full-size tests reach guided chunks above one problem only in the fp64 step, the fp64 Solve and the fp32 step kernel; both linearize
kernels and the fp32 Solve / Iterate kernel otherwise only ever see chunks of one.  Here NewtonStep, Iterate and linearize run in both
precisions on the smallest shapes that reach each fused kernel (fp64: n = 16, the 32 grid, one variable past the one-tile kernel; fp32:
n = 64; k = m = 0, m_r = 4, packed row-major J), at batches 1, 5 and 40 009.  At 40 009 the first guided chunk is
40 009 >> floor(log2(256 CUs x 4 WPS x 4)) = 4 problems at three waves per SIMD and 2 at four.  Every call runs once with tickets forced
and once with static rounds forced: no output sentinel may be left, the two schemes must agree bit for bit, and 64 sampled problems must
equal, bit for bit, the same problems run as a batch of their own (a problem's result does not depend on who hands it out)."""
import ctypes as C
import functools

import pytest
import torch

from mini_opt_amd import _lib as L
from mini_opt_amd import qp as Q

pytestmark = pytest.mark.gpu

N = {torch.float64: 16, torch.float32: 64}
M_R, LAM, MU, BIG = 4, 0.5, 0.1, 40009
SCHEMES = (L.MO_PLAN_TICKETS_ALWAYS, L.MO_PLAN_STATIC_ROUNDS_ALWAYS)


@functools.lru_cache(maxsize=None)
def _data(dtype):
    """(J, r, x) of BIG problems, every problem with data of its own; the smaller batches are its first problems."""
    gen = torch.Generator(device="cuda:0").manual_seed(20260 + N[dtype])
    mk = lambda *shape: torch.randn(*shape, generator=gen, device="cuda:0", dtype=dtype)
    return mk(BIG, M_R, N[dtype]), mk(BIG, M_R), mk(BIG, N[dtype])


def _solver(J, r, x):
    solver = Q.QPInteriorPointSolver(Q.BatchedQP(n=int(J.shape[2]), J=J, r=r, lam=LAM))
    solver.SetVariables(x)
    solver.delta_.fill_(float("nan"))
    solver.status_.fill_(-1)
    return solver


def _newton_step(J, r, x):
    solver = _solver(J, r, x)
    assert solver.step_kernel().startswith("fused")
    delta, alpha, status = solver.NewtonStep(MU)
    return {"delta": delta, "status": status, "alpha": alpha}


def _iterate(J, r, x):
    solver = _solver(J, r, x)
    assert solver.solve_kernel().startswith("fused")
    ip, status = solver.Iterate(MU)
    return {"delta": solver.delta_, "status": status, "variables": solver.variables(), "ip": ip}


def _linearize(J, r, x):
    B, n = int(J.shape[0]), int(J.shape[2])
    qp = Q.BatchedQP(n=n, J=J, r=r, lam=LAM)
    # The C ABI has no name query for the linearisation: this shows only that the shape is one the fused kernels serve (packed J, m_r = 4,
    # n = 16 / 64: fused_supported / fused_f32_supported take MODE_LINEARIZE for it), not which kernel mo_linearize launched.
    assert Q.QPInteriorPointSolver(qp).step_kernel().startswith("fused")
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=J.dtype, device=J.device)
    G, c, f = nan(B, n, n), nan(B, n), nan(B)
    desc = L.PlanDesc(n, 0, 0, M_R, Q._DT[J.dtype], J.device.index or 0, L.EXTRA_PLAN_FLAGS, 0, B)
    plan = C.c_void_p()
    L.check(L.lib().mo_plan_create(C.byref(desc), C.byref(plan)))
    try:
        prob = qp.as_struct()
        L.check(L.lib().mo_linearize(plan, C.byref(prob), B, Q._ptr(G), n * n, n, Q._ptr(c), n, Q._ptr(f), Q._stream()))
    finally:
        L.lib().mo_plan_destroy(plan)
    return {"G": G, "c": c, "half_sq": f}


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("batch", [1, 5, BIG])
@pytest.mark.parametrize("call", [_newton_step, _iterate, _linearize], ids=["NewtonStep", "Iterate", "linearize"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_every_problem_once_under_both_schemes(dtype, call, batch, monkeypatch):
    inputs = [t[:batch] for t in _data(dtype)]
    outs = []
    for flag in SCHEMES:
        monkeypatch.setattr(L, "EXTRA_PLAN_FLAGS", flag)
        out = call(*inputs)
        torch.cuda.synchronize()
        for name in ("delta", "G", "c", "half_sq"):   # pre-filled with NaN
            if name in out:
                assert not bool(torch.isnan(out[name]).any()), (flag, name)
        if "status" in out:                           # pre-filled with -1
            assert bool((out["status"] == 0).all()), flag
        outs.append(out)
    for name in outs[0]:
        assert _same_bits(outs[0][name], outs[1][name]), name
    # the sampled problems as a batch of their own (default scheme): first, last and seeded random ones
    if batch > 64:
        mid = torch.randperm(batch - 2, generator=torch.Generator().manual_seed(batch))[:62] + 1
        idx = torch.cat([torch.tensor([0, batch - 1]), mid]).to(inputs[0].device)
    else:
        idx = torch.arange(batch, device=inputs[0].device)
    monkeypatch.setattr(L, "EXTRA_PLAN_FLAGS", 0)
    ref = call(*[t.index_select(0, idx) for t in inputs])
    for name in ref:
        assert _same_bits(outs[0][name].index_select(0, idx), ref[name]), name
