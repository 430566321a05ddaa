"""Differentiable batched QP: `.backward()` through QPInteriorPointSolver::Solve.

    kkt_solve       mo_kkt_solve     the KKT system of a state for the caller's right-hand side (direct or transposed)
    qp_gradients    mo_qp_gradients  gradients of a loss with respect to the QP's data from the state v and the adjoint u = K^-T g
    qp_gradients_shared    mo_qp_gradients_shared  the same gradients SUMMED over the batch, for data the whole batch shares
    qp_gradients_blocks, qp_gradients_eq_blocks    the same for residual-block input: gradients of the PACKED local Jacobians
    qp_gradients_blocks_shared    mo_qp_gradients_blocks_shared  those gradients SUMMED over the batch, for blocks the whole batch shares
    qp_tangent_rhs  mo_qp_tangent_rhs  forward mode: rho = F_theta thetadot from the state v and a direction in the QP's data
    qp_jvp          qp_tangent_rhs + kkt_solve: the directional derivative vdot of the whole solution [x | s | y | z]
    qp_tangent_rhs_blocks, qp_jvp_blocks    the same for residual-block input: rho from the PACKED tangents of the blocks
    solve_qp        the user-facing call: forward = Solve (the kernels of qp.QPInteriorPointSolver, fused where the shape allows),
                    backward = ONE transposed KKT solve + ONE gradient launch for exactly the inputs that require a gradient
                    (+ ONE batch-reduced launch for the inputs given once for the batch, leading dimension 1),
                    jvp (torch.autograd.forward_ad) = ONE tangent launch + ONE KKT solve, for all three input forms

The mathematics is in include/mini_opt_hip.h (above mo_kkt_solve) and DESIGN.md section 4.8.  All arithmetic happens in the HIP library;
torch owns memory, streams and the autograd graph.  Plans are created once per (shape, dtype, device, batch) and cached.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, Optional

import torch

from . import _lib as L
from .qp import _DT, BatchedQP, Params, ResidualLayout, _ptr, _stream, jacobian_blocks, linearize_blocks

_PLANS: Dict[tuple, C.c_void_p] = {}
GRADIENTS = ("G", "c", "J", "r", "lam", "A_eq", "b_eq", "cons_a", "cons_b")


def plan_for(problem: BatchedQP, batch: int) -> C.c_void_p:
    """The cached plan of (shape, dtype, device, batch); created on first use, kept until clear_plan_cache()."""
    return _plan_of(problem.n, problem.k, problem.m, problem.m_r, problem.dtype, problem.device, batch)


def _plan_of(n: int, k: int, m: int, m_r: int, dtype, dev, batch: int) -> C.c_void_p:
    key = (n, k, m, m_r, dtype, dev.index or 0, int(batch))
    plan = _PLANS.get(key)
    if plan is None:
        desc = L.PlanDesc(n, k, m, m_r, _DT[dtype], dev.index or 0, L.EXTRA_PLAN_FLAGS, 0, int(batch))
        plan = C.c_void_p()
        L.check(L.lib().mo_plan_create(C.byref(desc), C.byref(plan)))
        _PLANS[key] = plan
    return plan


def clear_plan_cache() -> None:
    for plan in _PLANS.values():
        L.lib().mo_plan_destroy(plan)
    _PLANS.clear()


def _check_state(t: torch.Tensor, name: str, V: int, like) -> int:
    """The one check of a [B, V] state-sized tensor (vars, rhs, u); `like` carries the dtype and device (a BatchedQP or a ResidualLayout)."""
    if t.dim() != 2 or int(t.shape[1]) != V or not t.is_contiguous() or t.dtype != like.dtype or t.device != like.device:
        raise ValueError(f"{name}: expected a contiguous [B, {V}] {like.dtype} tensor on {like.device}, got {tuple(t.shape)} {t.dtype}")
    return int(t.shape[0])


def _check_state_pair(vars: torch.Tensor, other: torch.Tensor, name: str, V: int, like) -> int:
    B = _check_state(vars, "vars", V, like)
    if _check_state(other, name, V, like) != B:
        raise ValueError(f"vars and {name} must have the same batch")
    return B


def _take(x: Optional[torch.Tensor], name: str, tail, B: int, dtype, device, keep: list):
    """(pointer, problem stride) of an input [B or 1, *tail]; stride 0 -- one direction or value shared by the batch -- iff the leading
    dimension is 1 and B is not.  `keep` holds the tensor until the launch."""
    if (x is None or x.dim() != 1 + len(tail) or tuple(int(d) for d in x.shape[1:]) != tuple(tail) or int(x.shape[0]) not in (1, B)
            or not x.is_contiguous() or x.dtype != dtype or x.device != device):
        got = "None" if x is None else f"{tuple(x.shape)} {x.dtype}"
        raise ValueError(f"{name}: expected a contiguous [{B} or 1, {', '.join(map(str, tail))}] {dtype} tensor on {device}, got {got}")
    keep.append(x)
    per = 1
    for d in tail:
        per *= int(d)
    return _ptr(x), (0 if int(x.shape[0]) == 1 and B != 1 else per)


def _check_names(names, kind: str, allowed, no_rows=(), other_level=()) -> None:
    """The names of a `want` list or a tangent dict (kind: "gradient" or "tangent"): known, of rows the problem has, of its input level."""
    for w in names:
        if w not in allowed:
            raise ValueError(f"unknown {kind} {w!r}: one of {allowed}")
        if w in no_rows:
            raise ValueError(f"{kind} {w!r} of a problem without such rows")
        if w in other_level:
            raise ValueError(f"{kind} {w!r} does not belong to this problem's input level ((J, r, lam) or (G, c))")


def _check_dense_names(problem: BatchedQP, names, kind: str) -> None:
    no_rows = (("A_eq", "b_eq") if problem.k == 0 else ()) + (("cons_a", "cons_b") if problem.m == 0 else ())
    _check_names(names, kind, GRADIENTS, no_rows, ("G",) if problem.J is not None else ("J", "r", "lam"))


def kkt_solve(problem: BatchedQP, vars: torch.Tensor, rhs: torch.Tensor, transpose: bool = False, include_inequalities: bool = True):
    """mo_kkt_solve: factorise the KKT matrix K of every problem at `vars` [B, V] (s > 0 required) and solve for `rhs` [B, V].
    transpose=False: out = delta with K delta = -rhs (SolveForUpdate with r_ := rhs, mu = 0); transpose=True: out = u with K^T u = rhs.
    Returns (out [B, V], status [B] int32 MO_STATUS_*); out is NaN for problems whose status is not OK."""
    B = _check_state_pair(vars, rhs, "rhs", problem.V, problem)
    out = torch.empty_like(vars)
    status = torch.empty(B, dtype=torch.int32, device=vars.device)
    flags = (L.MO_KKT_TRANSPOSE if transpose else 0) | (0 if include_inequalities else L.MO_STEP_NO_INEQUALITIES)
    prob = problem.as_struct()
    L.check(L.lib().mo_kkt_solve(plan_for(problem, B), C.byref(prob), B, _ptr(vars), problem.V, _ptr(rhs), problem.V, flags,
                                 _ptr(out), problem.V, _ptr(status), _stream()))
    return out, status


def kkt_solve_kernel(problem: BatchedQP, batch: int) -> str:
    """mo_plan_kkt_solve_kernel: the kernel kkt_solve (and the backward of solve_qp) launches for this problem's shape and layout on the cached
    plan of `batch` problems: "generic", or the fused step kernel's right-hand-side twin ("fused_rhs_mfma_f64_n64", "fused_rhs_qp_f64_n32", ...)."""
    prob = problem.as_struct()
    return L.lib().mo_plan_kkt_solve_kernel(plan_for(problem, int(batch)), C.byref(prob)).decode()


def qp_gradients(problem: BatchedQP, vars: torch.Tensor, u: torch.Tensor, want: Optional[Iterable[str]] = None) -> Dict[str, torch.Tensor]:
    """mo_qp_gradients: the gradients named in `want` (default: every one the problem's input level has) from the state `vars` [B, V] and
    the adjoint `u` [B, V] = kkt_solve(..., transpose=True) of g = dl/dv.  Keys and layouts follow BatchedQP:
      "c" [B, n]    "G" [B, n, n] (symmetric)    "A_eq" [B, n, k]    "b_eq" [B, k]    "cons_a", "cons_b" [B, m]
      "J" (the shape and layout of problem.J)    "r" [B, m_r]    "lam" [B]
    "G" is the gradient with respect to a symmetric G; "G" with J-level input and "J" / "r" / "lam" with (G, c) input raise."""
    B = _check_state_pair(vars, u, "u", problem.V, problem)
    n, k, m = problem.n, problem.k, problem.m
    j_level = problem.J is not None
    if want is None:
        want = (("J", "r", "lam") if j_level else ("G", "c")) + (("A_eq", "b_eq") if k else ()) + (("cons_a", "cons_b") if m else ())
    want = tuple(want)
    _check_dense_names(problem, want, "gradient")
    dt, dev = problem.dtype, problem.device
    new = lambda *shape: torch.empty(*shape, dtype=dt, device=dev)
    out: Dict[str, torch.Tensor] = {}
    g = L.QPGrads()
    if "G" in want:
        out["G"] = new(B, n, n)
        g.dG, g.dG_stride, g.dG_ld = _ptr(out["G"]), n * n, n
    if "c" in want:
        out["c"] = new(B, n)
        g.dc, g.dc_stride = _ptr(out["c"]), n
    if "A_eq" in want:
        out["A_eq"] = new(B, n, k)
        g.dA_eq, g.dA_stride, g.dA_ld = _ptr(out["A_eq"]), n * k, k
    if "b_eq" in want:
        out["b_eq"] = new(B, k)
        g.db_eq, g.db_stride = _ptr(out["b_eq"]), k
    if "cons_a" in want or "cons_b" in want:
        g.dcons_stride = m
        if "cons_a" in want:
            out["cons_a"] = new(B, m)
            g.dcons_a = _ptr(out["cons_a"])
        if "cons_b" in want:
            out["cons_b"] = new(B, m)
            g.dcons_b = _ptr(out["cons_b"])
    if "J" in want:
        rows, ld = int(problem.J.shape[1]), int(problem.J.shape[2])
        padded = ld > (problem.m_r if problem.J_layout == "col" else n)   # (the padding beyond the matrix is not written: define it)
        out["J"] = torch.zeros(B, rows, ld, dtype=dt, device=dev) if padded else new(B, rows, ld)
        g.dJ, g.dJ_stride, g.dJ_ld = _ptr(out["J"]), rows * ld, ld
        g.dJ_layout = L.MO_COL_MAJOR if problem.J_layout == "col" else L.MO_ROW_MAJOR
    if "r" in want:
        out["r"] = new(B, problem.m_r)
        g.dr, g.dr_stride = _ptr(out["r"]), problem.m_r
    if "lam" in want:
        out["lam"] = new(B)
        g.dlambda, g.dlambda_stride = _ptr(out["lam"]), 1
    prob = problem.as_struct()
    L.check(L.lib().mo_qp_gradients(plan_for(problem, B), C.byref(prob), B, _ptr(vars), problem.V, _ptr(u), problem.V, C.byref(g), _stream()))
    return out


def qp_gradients_shared(problem: BatchedQP, vars: torch.Tensor, u: torch.Tensor, want: Iterable[str], status_fwd: Optional[torch.Tensor] = None,
                        status_adj: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """mo_qp_gradients_shared: the gradients named in `want`, SUMMED over the batch, for data the whole batch shares.  Keys and layouts are
    those of qp_gradients with a leading dimension of 1: "G" [1, n, n], "c" [1, n], "A_eq" [1, n, k], "J" [1, rows, ld], "lam" [1], ...
    status_fwd / status_adj: [B] int32 status words; a problem counts iff every given word is MO_STATUS_OK (its rows of `vars` / `u` may
    then hold anything, NaN included).  "J" and "r" need problem.J with a leading dimension of 1, "cons_a" / "cons_b" a constraint set with
    one.  No [B, ...] matrix is formed: the workspace (chunk partials, from torch's allocator) is a few tiles per CU."""
    B = _check_state_pair(vars, u, "u", problem.V, problem)
    n, k, m = problem.n, problem.k, problem.m
    want = tuple(want)
    _check_dense_names(problem, want, "gradient")
    dt, dev = problem.dtype, problem.device
    _check_status(status_fwd, "status_fwd", B, dev)
    _check_status(status_adj, "status_adj", B, dev)
    new = lambda *shape: torch.empty(1, *shape, dtype=dt, device=dev)
    out: Dict[str, torch.Tensor] = {}
    g = L.QPGrads()
    if "G" in want:
        out["G"] = new(n, n)
        g.dG, g.dG_ld = _ptr(out["G"]), n
    if "c" in want:
        out["c"] = new(n)
        g.dc = _ptr(out["c"])
    if "A_eq" in want:
        out["A_eq"] = new(n, k)
        g.dA_eq, g.dA_ld = _ptr(out["A_eq"]), k
    if "b_eq" in want:
        out["b_eq"] = new(k)
        g.db_eq = _ptr(out["b_eq"])
    if "cons_a" in want:
        out["cons_a"] = new(m)
        g.dcons_a = _ptr(out["cons_a"])
    if "cons_b" in want:
        out["cons_b"] = new(m)
        g.dcons_b = _ptr(out["cons_b"])
    if "J" in want:
        rows, ld = int(problem.J.shape[1]), int(problem.J.shape[2])
        padded = ld > (problem.m_r if problem.J_layout == "col" else n)   # (the padding beyond the matrix is not written: define it)
        out["J"] = torch.zeros(1, rows, ld, dtype=dt, device=dev) if padded else new(rows, ld)
        g.dJ, g.dJ_ld = _ptr(out["J"]), ld
        g.dJ_layout = L.MO_COL_MAJOR if problem.J_layout == "col" else L.MO_ROW_MAJOR
    if "r" in want:
        out["r"] = new(problem.m_r)
        g.dr = _ptr(out["r"])
    if "lam" in want:
        out["lam"] = new()
        g.dlambda = _ptr(out["lam"])
    prob = problem.as_struct()
    plan = plan_for(problem, B)
    nbytes = C.c_int64()
    L.check(L.lib().mo_qp_gradients_shared_workspace(plan, C.byref(prob), B, C.byref(g), C.byref(nbytes)))
    work = torch.empty(max(int(nbytes.value), 16), dtype=torch.uint8, device=dev)
    L.check(L.lib().mo_qp_gradients_shared(plan, C.byref(prob), B, _ptr(vars), problem.V, _ptr(u), problem.V, _ptr(status_fwd), _ptr(status_adj),
                                           C.byref(g), _ptr(work), int(work.numel()), _stream()))
    return out


def qp_tangent_rhs(problem: BatchedQP, vars: torch.Tensor, tangents: Dict[str, torch.Tensor]) -> torch.Tensor:
    """mo_qp_tangent_rhs: rho [B, V] = F_theta thetadot at the state `vars` [B, V] for the direction `tangents` in the problem's data, the
    right-hand side of the forward-mode system K vdot = -rho.  `tangents` maps the keys of GRADIENTS to tensors in BatchedQP's layouts (the
    layouts qp_gradients returns): "c" [B, n], "G" [B, n, n] (LOWER triangle read as a symmetric matrix, the rest ignored), "A_eq" [B, n, k],
    "b_eq" [B, k], "cons_a", "cons_b" [B, m], "J" in the layout of problem.J (its own leading dimension allowed), "r" [B, m_r], "lam" [B].
    A missing key is a zero tangent; a leading dimension of 1 is one direction shared by the batch."""
    B = _check_state(vars, "vars", problem.V, problem)
    n, k, m = problem.n, problem.k, problem.m
    t = L.QPTangents()
    keep = []
    take = lambda name, tail: _take(tangents[name], f"tangent {name!r}", tail, B, problem.dtype, problem.device, keep)
    _check_dense_names(problem, tangents, "tangent")
    if "G" in tangents:
        t.dG, t.dG_stride = take("G", (n, n))
        t.dG_ld = n
    if "c" in tangents:
        t.dc, t.dc_stride = take("c", (n,))
    if "A_eq" in tangents:
        t.dA_eq, t.dA_stride = take("A_eq", (n, k))
        t.dA_ld = k
    if "b_eq" in tangents:
        t.db_eq, t.db_stride = take("b_eq", (k,))
    if "cons_a" in tangents:
        t.dcons_a, t.dcons_stride = take("cons_a", (m,))
    if "cons_b" in tangents:
        t.dcons_b, stride_b = take("cons_b", (m,))
        if "cons_a" in tangents and stride_b != t.dcons_stride:
            raise ValueError("tangents 'cons_a' and 'cons_b' share one stride: give both per problem or both shared")
        t.dcons_stride = stride_b
    if "J" in tangents:
        rows = int(problem.J.shape[1])
        ld = int(tangents["J"].shape[-1]) if tangents["J"].dim() == 3 else 0
        if ld < (problem.m_r if problem.J_layout == "col" else n):
            raise ValueError(f"tangent 'J': leading dimension {ld} below the layout's minimum")
        t.dJ, t.dJ_stride = take("J", (rows, ld))
        t.dJ_ld = ld
    if "r" in tangents:
        t.dr, t.dr_stride = take("r", (problem.m_r,))
    if "lam" in tangents:
        t.dlambda, t.dlambda_stride = take("lam", ())
    rho = torch.empty_like(vars)
    prob = problem.as_struct()
    L.check(L.lib().mo_qp_tangent_rhs(plan_for(problem, B), C.byref(prob), B, _ptr(vars), problem.V, C.byref(t), _ptr(rho), problem.V, _stream()))
    return rho


def qp_jvp(problem: BatchedQP, vars: torch.Tensor, tangents: Dict[str, torch.Tensor]):
    """The directional derivative vdot [B, V] = (dv* / dtheta) thetadot of the solution [x | s | y | z] at `vars` along `tangents` (see
    qp_tangent_rhs): one tangent launch and one KKT solve, K vdot = -rho.  Returns (vdot, status [B] int32 MO_STATUS_*); vdot is NaN for
    problems whose status is not OK."""
    return kkt_solve(problem, vars, qp_tangent_rhs(problem, vars, tangents), transpose=False)


_PENDING_TANGENT_STATUS: Optional[torch.Tensor] = None   # from a Function's jvp to solve_qp, which hangs it on the tensors it returns


def _masked(t: Optional[torch.Tensor], ok: torch.Tensor) -> Optional[torch.Tensor]:
    """The zero-masking rule: a problem whose forward status or adjoint / tangent-solve status is not MO_STATUS_OK gets ZERO."""
    if t is None:
        return None
    return torch.where(ok.view(-1, *([1] * (t.dim() - 1))), t, torch.zeros((), dtype=t.dtype, device=t.device))


def _solve_forward(ctx, problem: BatchedQP, B: int, params: Params):
    """The forward of both Functions: mo_qp_solve from a zero state; what backward and jvp need goes on ctx."""
    dev = problem.device
    v = torch.zeros(B, problem.V, dtype=problem.dtype, device=dev)
    term = torch.empty(B, dtype=torch.int32, device=dev)
    nit = torch.empty(B, dtype=torch.int32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    prob, sp = problem.as_struct(), params.as_struct()
    L.check(L.lib().mo_qp_solve(plan_for(problem, B), C.byref(prob), B, C.byref(sp), _ptr(v), problem.V, _ptr(term), _ptr(nit), None, None,
                                _ptr(status), _stream()))
    ctx.problem, ctx.v, ctx.status = problem, v, status
    ctx.adjoint_status = None
    ctx.tangent_status = None
    ctx.termination_state, ctx.num_iterations = term, nit
    ctx.mark_non_differentiable(status)
    ctx.set_materialize_grads(False)   # jvp: an input without a tangent arrives as None, not as a tensor of zeros to be read
    return v.clone(), status


def _adjoint(ctx, g):
    """The backward of both Functions begins here: K(v)^T u = g once; returns (problem, v, u, ok [B]: forward and adjoint status OK)."""
    problem, v = ctx.problem, ctx.v
    if g is None:
        g = torch.zeros_like(v)
    u, adj = kkt_solve(problem, v, g.contiguous(), transpose=True)
    ctx.adjoint_status = adj
    return problem, v, u, (ctx.status == L.MO_STATUS_OK) & (adj == L.MO_STATUS_OK)


def _given(names, tangents) -> Dict[str, torch.Tensor]:
    return {nm: t.detach().contiguous() for nm, t in zip(names, tangents) if t is not None}


def _jvp_result(ctx, vdot, st):
    """The jvp of both Functions ends here: the solve's status words are kept and handed to solve_qp, failed problems get a zero tangent."""
    global _PENDING_TANGENT_STATUS
    ctx.tangent_status = _PENDING_TANGENT_STATUS = st
    return _masked(vdot, (ctx.status == L.MO_STATUS_OK) & (st == L.MO_STATUS_OK)), None


class QPSolveFunction(torch.autograd.Function):
    """v*(theta) = QPInteriorPointSolver::Solve with the adjoint of the KKT conditions as its backward.

    forward(G, c, J, r, lam, A_eq, b_eq, cons_a, cons_b, cons_var, params) -> (v [B, V] = [x | s | y | z], status [B]); tensors in BatchedQP's
    layouts, contiguous, each with a leading dimension of B or of 1 (given once for the batch: read with stride 0, never expanded; the
    constraint triple all three or none); `lam` a [B] or [1] tensor or None.  The backward solves K(v)^T u = g once and launches
    mo_qp_gradients once, for the per-problem inputs whose needs_input_grad is set, and mo_qp_gradients_shared once, for the shared ones:
    their gradients are summed over the batch by the kernel and arrive as [1, ...].  A problem whose forward status or adjoint status is not MO_STATUS_OK gets ZERO gradients: one
    infeasible problem must not poison the reduction over a batch with NaN.  The adjoint's status words stay on the node
    (`adjoint_status`, None before the first backward)."""

    @staticmethod
    def forward(ctx, G, c, J, r, lam, A_eq, b_eq, cons_a, cons_b, cons_var, params):
        det = lambda t: None if t is None else t.detach()
        ref = J if J is not None else G
        n = int(ref.shape[2])
        k = 0 if A_eq is None else int(A_eq.shape[2])
        m = 0 if cons_a is None else int(cons_a.shape[1])
        problem = BatchedQP(n=n, k=k, m=m, J=det(J), r=det(r), lam=0.0, lam_vec=det(lam), G=det(G), c=det(c), A_eq=det(A_eq), b_eq=det(b_eq),
                            cons_var=cons_var, cons_a=det(cons_a), cons_b=det(cons_b))
        inputs = (G, c, J, r, lam, A_eq, b_eq, cons_a, cons_b)
        B = max(int(t.shape[0]) for t in inputs if t is not None)
        ctx.shared = frozenset(nm for nm, t in zip(GRADIENTS, inputs) if t is not None and int(t.shape[0]) == 1 and B > 1)
        return _solve_forward(ctx, problem, B, params)

    @staticmethod
    def backward(ctx, g, _g_status):
        problem, v, u, ok = _adjoint(ctx, g)
        want = [nm for nm, need in zip(GRADIENTS, ctx.needs_input_grad[:9]) if need]
        # summed by the kernel: what the batch shares -- but "r" given once against a J per problem, which mo_qp_gradients_shared refuses
        # (dr = -J s_u needs one J): that one is formed per problem and summed here
        summed = [nm for nm in want if nm in ctx.shared and not (nm == "r" and "J" not in ctx.shared)]
        each = [nm for nm in want if nm not in summed]
        grads = {nm: _masked(t, ok) for nm, t in qp_gradients(problem, v, u, each).items()} if each else {}
        for nm in each:
            if nm in ctx.shared:
                grads[nm] = grads[nm].sum(0, keepdim=True)
        if summed:
            grads.update(qp_gradients_shared(problem, v, u, summed, status_fwd=ctx.status, status_adj=ctx.adjoint_status))
        return (*[grads.get(nm) for nm in GRADIENTS], None, None)

    @staticmethod
    def jvp(ctx, dG, dc, dJ, dr, dlam, dA_eq, db_eq, dcons_a, dcons_b, _dcons_var, _dparams):
        """torch.autograd.forward_ad: vdot = (dv* / dtheta) thetadot at the saved state, ONE tangent launch + ONE KKT solve.  The G tangent is
        passed as 1/2 (Gdot + Gdot^T), so the JVP is the exact transpose of the backward for any Gdot.  A problem whose forward status or
        tangent-solve status is not MO_STATUS_OK gets a ZERO tangent (the backward's rule); the solve's status words are kept
        (`tangent_status`)."""
        if dG is not None:
            dG = 0.5 * (dG + dG.transpose(1, 2))
        tangents = _given(GRADIENTS, (dG, dc, dJ, dr, dlam, dA_eq, db_eq, dcons_a, dcons_b))
        return _jvp_result(ctx, *qp_jvp(ctx.problem, ctx.v, tangents))


def tangent_status(t: torch.Tensor) -> Optional[torch.Tensor]:
    """The [B] status words of the tangent solve behind a tensor solve_qp returned under torch.autograd.forward_ad (None if the call
    carried no tangent)."""
    while t is not None:
        st = getattr(t, "_mo_tangent_status", None)
        if st is not None:
            return st
        t = t._base
    return None


def qp_gradients_blocks(layout: ResidualLayout, J_blocks: torch.Tensor, r: torch.Tensor, vars: torch.Tensor, u: torch.Tensor, k: int = 0,
                        m: int = 0, want: Iterable[str] = ("J_blocks", "r", "lam")) -> Dict[str, torch.Tensor]:
    """mo_qp_gradients_blocks: gradients of a loss with respect to the packed cost blocks of `layout` (the inputs of linearize_blocks) from the
    state `vars` [B, V] and the adjoint `u` [B, V] of the (G, c) problem they were linearised into; k, m: that problem's equality and
    inequality rows (V = n + 2 m + k).  J_blocks [B or 1, values], r [B or 1, rows] (1: shared by the batch; the outputs are per problem).
    Returns the ones named in `want`: "J_blocks" [B, values] (the packing of J_blocks), "r" [B, rows], "lam" [B]."""
    want = tuple(want)
    _check_names(want, "gradient", ("J_blocks", "r", "lam"))
    B = _check_state_pair(vars, u, "u", layout.n + 2 * int(m) + int(k), layout)
    keep = []
    J_ptr, J_stride = _take(J_blocks, "J_blocks", (layout.values,), B, layout.dtype, layout.device, keep)
    r_ptr, r_stride = _take(r, "r", (layout.rows,), B, layout.dtype, layout.device, keep)
    new = lambda *shape: torch.empty(*shape, dtype=layout.dtype, device=layout.device)
    out: Dict[str, torch.Tensor] = {}
    g = L.BlockGrads()
    if "J_blocks" in want:
        out["J_blocks"] = new(B, layout.values)
        g.dJ_blocks, g.dJ_stride = _ptr(out["J_blocks"]), layout.values
    if "r" in want:
        out["r"] = new(B, layout.rows)
        g.dr, g.dr_stride = _ptr(out["r"]), layout.rows
    if "lam" in want:
        out["lam"] = new(B)
        g.dlambda, g.dlambda_stride = _ptr(out["lam"]), 1
    plan = _plan_of(layout.n, int(k), int(m), 0, layout.dtype, layout.device, B)
    L.check(L.lib().mo_qp_gradients_blocks(plan, layout.h, J_ptr, J_stride, r_ptr, r_stride, B, _ptr(vars), int(vars.shape[1]), _ptr(u),
                                           int(u.shape[1]), C.byref(g), _stream()))
    return out


def qp_gradients_eq_blocks(eq_layout: ResidualLayout, vars: torch.Tensor, u: torch.Tensor, m: int = 0,
                           want: Iterable[str] = ("J_eq_blocks", "r_eq")) -> Dict[str, torch.Tensor]:
    """mo_qp_gradients_eq_blocks: gradients with respect to the packed equality blocks of `eq_layout` (the inputs of jacobian_blocks; k = its
    rows) from `vars`, `u` [B, n + 2 m + k]: "J_eq_blocks" [B, values] (exactly 0 for a column that loses its global column), "r_eq" [B, k]."""
    want = tuple(want)
    _check_names(want, "gradient", ("J_eq_blocks", "r_eq"))
    k = eq_layout.rows
    B = _check_state_pair(vars, u, "u", eq_layout.n + 2 * int(m) + k, eq_layout)
    out: Dict[str, torch.Tensor] = {}
    if "J_eq_blocks" in want:
        out["J_eq_blocks"] = torch.empty(B, eq_layout.values, dtype=eq_layout.dtype, device=eq_layout.device)
    if "r_eq" in want:
        out["r_eq"] = torch.empty(B, k, dtype=eq_layout.dtype, device=eq_layout.device)
    plan = _plan_of(eq_layout.n, k, int(m), 0, eq_layout.dtype, eq_layout.device, B)
    L.check(L.lib().mo_qp_gradients_eq_blocks(plan, eq_layout.h, B, _ptr(vars), int(vars.shape[1]), _ptr(u), int(u.shape[1]),
                                              _ptr(out.get("J_eq_blocks")), eq_layout.values, _ptr(out.get("r_eq")), k, _stream()))
    return out


def _check_status(st: Optional[torch.Tensor], name: str, B: int, dev) -> None:
    if st is not None and (st.dtype != torch.int32 or tuple(st.shape) != (B,) or not st.is_contiguous() or st.device != dev):
        raise ValueError(f"{name}: expected a contiguous [{B}] int32 tensor on {dev}")


BLOCK_GRADIENTS = ("J_blocks", "r", "lam", "J_eq_blocks", "r_eq")


def qp_gradients_blocks_shared(layout: ResidualLayout, J_blocks: Optional[torch.Tensor], r: Optional[torch.Tensor], vars: torch.Tensor,
                               u: torch.Tensor, k: int = 0, m: int = 0, want: Iterable[str] = ("J_blocks", "lam"),
                               eq_layout: Optional[ResidualLayout] = None, status_fwd: Optional[torch.Tensor] = None,
                               status_adj: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """mo_qp_gradients_blocks_shared: the gradients of qp_gradients_blocks / qp_gradients_eq_blocks named in `want`, SUMMED over the batch,
    for packed blocks the whole batch shares: "J_blocks" [1, values], "r" [1, rows], "lam" [1], "J_eq_blocks" [1, eq_layout.values],
    "r_eq" [1, k].  J_blocks [1, values] and r [B or 1, rows] are needed (and read) only with "J_blocks" / "r"; "r" needs r [1, rows].
    k, m: the (G, c) problem's equality and inequality rows (k = eq_layout.rows when an eq_layout is given).  status_fwd / status_adj: [B]
    int32 status words; a problem counts iff every given word is MO_STATUS_OK (its rows of `vars` / `u` / `r` may then hold anything).
    No [B, values] gradient is formed: the workspace (chunk partials, from torch's allocator) is a few tiles and packed values per CU."""
    want = tuple(want)
    if eq_layout is not None:
        if eq_layout.n != layout.n or eq_layout.dtype != layout.dtype or eq_layout.device != layout.device:
            raise ValueError("eq_layout must share n, dtype and device with layout")
        k = eq_layout.rows
    k, m = int(k), int(m)
    _check_names(want, "gradient", BLOCK_GRADIENTS, ("J_eq_blocks", "r_eq") if eq_layout is None or k == 0 else ())
    V = layout.n + 2 * m + k
    B = _check_state_pair(vars, u, "u", V, layout)
    dt, dev = layout.dtype, layout.device
    _check_status(status_fwd, "status_fwd", B, dev)
    _check_status(status_adj, "status_adj", B, dev)
    keep = []
    J_ptr = r_ptr = None
    r_stride = 0
    if "J_blocks" in want or "r" in want:
        J_ptr, _ = _take(J_blocks, "J_blocks", (layout.values,), 1, dt, dev, keep)          # ONE instance
        r_ptr, r_stride = _take(r, "r", (layout.rows,), B, dt, dev, keep)
        if "r" in want and int(r.shape[0]) != 1:
            raise ValueError("gradient 'r' summed over the batch needs r [1, rows]")
    new = lambda *shape: torch.empty(1, *shape, dtype=dt, device=dev)
    out: Dict[str, torch.Tensor] = {}
    g = L.BlockSharedGrads()
    if "J_blocks" in want:
        out["J_blocks"] = new(layout.values)
        g.dJ_blocks = _ptr(out["J_blocks"])
    if "r" in want:
        out["r"] = new(layout.rows)
        g.dr = _ptr(out["r"])
    if "lam" in want:
        out["lam"] = new()
        g.dlambda = _ptr(out["lam"])
    if "J_eq_blocks" in want:
        out["J_eq_blocks"] = new(eq_layout.values)
        g.dJ_eq_blocks = _ptr(out["J_eq_blocks"])
    if "r_eq" in want:
        out["r_eq"] = new(k)
        g.dr_eq = _ptr(out["r_eq"])
    plan = _plan_of(layout.n, k, m, 0, dt, dev, B)
    eq_h = None if eq_layout is None else eq_layout.h
    nbytes = C.c_int64()
    L.check(L.lib().mo_qp_gradients_blocks_shared_workspace(plan, layout.h, eq_h, r_stride, B, C.byref(g), C.byref(nbytes)))
    work = torch.empty(max(int(nbytes.value), 16), dtype=torch.uint8, device=dev)
    L.check(L.lib().mo_qp_gradients_blocks_shared(plan, layout.h, J_ptr, r_ptr, r_stride, eq_h, B, _ptr(vars), V, _ptr(u), V, _ptr(status_fwd),
                                                  _ptr(status_adj), C.byref(g), _ptr(work), int(work.numel()), _stream()))
    return out


BLOCK_TANGENTS = ("J_blocks", "r", "lam", "J_eq_blocks", "r_eq", "cons_a", "cons_b")


def qp_tangent_rhs_blocks(layout: ResidualLayout, J_blocks: Optional[torch.Tensor], r: Optional[torch.Tensor], vars: torch.Tensor,
                          tangents: Dict[str, torch.Tensor], k: int = 0, m: int = 0, eq_layout: Optional[ResidualLayout] = None,
                          cons_var: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mo_qp_tangent_rhs_blocks: rho [B, V] = F_theta thetadot at the state `vars` [B, V] of the (G, c) problem the blocks were linearised
    into, for a direction in the PACKED block data; no n x n or rows x n matrix is formed.  `tangents` maps "J_blocks" [B, layout.values],
    "r" [B, layout.rows], "lam" [B], "J_eq_blocks" [B, eq_layout.values], "r_eq" [B, k], "cons_a", "cons_b" [B, m] to tensors; a missing key
    is a zero tangent, a leading dimension of 1 is one direction shared by the batch.  J_blocks [B or 1, values] and r [B or 1, rows] are
    needed (and read) only with the "J_blocks" / "r" tangents.  k, m: the problem's equality and inequality rows (k = eq_layout.rows when an
    eq_layout is given); cons_var int32 [B or 1, m] with "cons_a"."""
    if eq_layout is not None:
        if eq_layout.n != layout.n or eq_layout.dtype != layout.dtype or eq_layout.device != layout.device:
            raise ValueError("eq_layout must share n, dtype and device with layout")
        k = eq_layout.rows
    n, k, m = layout.n, int(k), int(m)
    V = n + 2 * m + k
    dt, dev = layout.dtype, layout.device
    B = _check_state(vars, "vars", V, layout)
    no_rows = (("J_eq_blocks", "r_eq") if k == 0 or eq_layout is None else ()) + (("cons_a", "cons_b") if m == 0 else ())
    _check_names(tangents, "tangent", BLOCK_TANGENTS, no_rows)
    keep = []
    take = lambda x, name, tail, dtype=dt: _take(x, name, tail, B, dtype, dev, keep)
    t = L.BlockTangents()
    J_ptr = r_ptr = None
    J_stride = r_stride = 0
    if "J_blocks" in tangents or "r" in tangents:
        J_ptr, J_stride = take(J_blocks, "J_blocks", (layout.values,))
        r_ptr, r_stride = take(r, "r", (layout.rows,))
    if "J_blocks" in tangents:
        t.dJ_blocks, t.dJ_stride = take(tangents["J_blocks"], "tangent 'J_blocks'", (layout.values,))
    if "r" in tangents:
        t.dr, t.dr_stride = take(tangents["r"], "tangent 'r'", (layout.rows,))
    if "lam" in tangents:
        t.dlambda, t.dlambda_stride = take(tangents["lam"], "tangent 'lam'", ())
    if "J_eq_blocks" in tangents:
        t.dJ_eq_blocks, t.dJ_eq_stride = take(tangents["J_eq_blocks"], "tangent 'J_eq_blocks'", (eq_layout.values,))
    if "r_eq" in tangents:
        t.dr_eq, t.dr_eq_stride = take(tangents["r_eq"], "tangent 'r_eq'", (k,))
    if "cons_a" in tangents:
        t.dcons_a, t.dcons_stride = take(tangents["cons_a"], "tangent 'cons_a'", (m,))
    if "cons_b" in tangents:
        t.dcons_b, stride_b = take(tangents["cons_b"], "tangent 'cons_b'", (m,))
        if "cons_a" in tangents and stride_b != t.dcons_stride:
            raise ValueError("tangents 'cons_a' and 'cons_b' share one stride: give both per problem or both shared")
        t.dcons_stride = stride_b
    cv_ptr, cv_stride = None, 0
    if m and cons_var is not None:
        cv_ptr, cv_stride = take(cons_var, "cons_var", (m,), torch.int32)
    elif "cons_a" in tangents:
        raise ValueError("tangent 'cons_a' needs cons_var")
    rho = torch.empty_like(vars)
    plan = _plan_of(n, k, m, 0, dt, dev, B)
    L.check(L.lib().mo_qp_tangent_rhs_blocks(plan, layout.h, J_ptr, J_stride, r_ptr, r_stride, None if eq_layout is None else eq_layout.h,
                                             cv_ptr, cv_stride, B, _ptr(vars), V, C.byref(t), _ptr(rho), V, _stream()))
    return rho


def qp_jvp_blocks(problem: BatchedQP, layout: ResidualLayout, J_blocks: torch.Tensor, r: torch.Tensor, vars: torch.Tensor,
                  tangents: Dict[str, torch.Tensor], eq_layout: Optional[ResidualLayout] = None):
    """The directional derivative vdot [B, V] of the solution of the (G, c) problem `problem` that linearize_blocks / jacobian_blocks built
    from the blocks, along `tangents` in the packed block data (see qp_tangent_rhs_blocks): one tangent launch and one KKT solve on
    `problem`, K vdot = -rho.  Returns (vdot, status [B] int32 MO_STATUS_*); vdot is NaN for problems whose status is not OK."""
    if problem.n != layout.n or (eq_layout is not None and eq_layout.rows != problem.k):
        raise ValueError("problem does not belong to these layouts (n / k differ)")
    rho = qp_tangent_rhs_blocks(layout, J_blocks, r, vars, tangents, k=problem.k, m=problem.m, eq_layout=eq_layout, cons_var=problem.cons_var)
    return kkt_solve(problem, vars, rho, transpose=False)


class QPSolveBlocksFunction(torch.autograd.Function):
    """QPSolveFunction for residual-block input.  forward(J_blocks, r, lam, J_eq_blocks, r_eq, cons_a, cons_b, cons_var, layout, eq_layout,
    params) -> (v, status): linearize_blocks gives (G, c), jacobian_blocks gives A_eq (b_eq = r_eq), mo_qp_solve runs on the (G, c) problem --
    the sequence of mo_nls_solve_blocks.  Every tensor has a leading dimension of B or of 1 (given once for the batch: read with stride 0,
    never expanded; the constraint triple all three or none).  With J_blocks AND lam given once, G is formed ONCE, [1, n, n], and c by the
    c-only linearize; a J_eq_blocks given once gives A_eq [1, n, k].  The backward solves K(v)^T u = g once on that problem (the fused
    right-hand-side twin where kkt_solve_kernel says so); inputs per problem go to mo_qp_gradients_blocks, mo_qp_gradients_eq_blocks and
    mo_qp_gradients (cons_a / cons_b), inputs given once to ONE mo_qp_gradients_blocks_shared launch (and mo_qp_gradients_shared for
    cons_a / cons_b): their gradients are summed over the batch by the kernels and arrive as [1, ...].  No n x n or m_r x n gradient is
    formed.  lam's gradient counts only where lam was added (lam > 0).  Zero gradients for problems whose forward or adjoint status is not
    OK, as QPSolveFunction."""

    NAMES = ("J_blocks", "r", "lam", "J_eq_blocks", "r_eq", "cons_a", "cons_b")

    @staticmethod
    def forward(ctx, J_blocks, r, lam, J_eq_blocks, r_eq, cons_a, cons_b, cons_var, layout, eq_layout, params):
        det = lambda t: None if t is None else t.detach()
        J_blocks, r, lam, J_eq_blocks, r_eq, cons_a, cons_b = (det(t) for t in (J_blocks, r, lam, J_eq_blocks, r_eq, cons_a, cons_b))
        inputs = (J_blocks, r, lam, J_eq_blocks, r_eq, cons_a, cons_b)
        B = max(int(t.shape[0]) for t in inputs if t is not None)
        once = lambda t: int(t.shape[0]) == 1 and B > 1
        ctx.shared = frozenset(nm for nm, t in zip(QPSolveBlocksFunction.NAMES, inputs) if t is not None and once(t))
        if once(J_blocks) and once(lam):   # one G for the batch: a batch-1 linearize; c from the call that forms no G
            G, _, _ = linearize_blocks(layout, J_blocks, r[:1], lam_vec=lam)
            _, c, _ = linearize_blocks(layout, J_blocks, r, lam_vec=lam, want_G=False)
        else:
            G, c, _ = linearize_blocks(layout, J_blocks, r, lam_vec=lam, batch=B)
        n = layout.n
        k = 0 if eq_layout is None else eq_layout.rows
        m = 0 if cons_a is None else int(cons_a.shape[1])
        A_eq = None
        if eq_layout is not None:   # [B or 1, n, k]: memory = k x n column-major, BatchedQP's layout (r_eq is not read: no |r|_1 is kept)
            A_eq, _ = jacobian_blocks(eq_layout, J_eq_blocks, r_eq[:1] if once(J_eq_blocks) else r_eq)
        problem = BatchedQP(n=n, k=k, m=m, G=G, c=c, A_eq=A_eq, b_eq=r_eq if k else None, cons_var=cons_var, cons_a=cons_a, cons_b=cons_b)
        ctx.layout, ctx.eq_layout, ctx.J_blocks, ctx.r, ctx.lam = layout, eq_layout, J_blocks, r, lam
        return _solve_forward(ctx, problem, B, params)

    @staticmethod
    def backward(ctx, g, _g_status):
        problem, v, u, ok = _adjoint(ctx, g)
        names = QPSolveBlocksFunction.NAMES
        want = [nm for nm, nd in zip(names, ctx.needs_input_grad[:7]) if nd]
        # summed by the kernels: what the batch shares -- but "r" given once against J_blocks per problem, which the reduced launch refuses
        # (dr = -sum s_u J_b needs one J_blocks): that one is formed per problem and summed here
        summed = [nm for nm in want if nm in ctx.shared and not (nm == "r" and "J_blocks" not in ctx.shared)]
        each = [nm for nm in want if nm not in summed]
        grads: Dict[str, torch.Tensor] = {}
        sel = lambda group, among: [nm for nm in group if nm in among]
        cost, eq, cons = sel(each, ("J_blocks", "r", "lam")), sel(each, ("J_eq_blocks", "r_eq")), sel(each, ("cons_a", "cons_b"))
        if cost:
            grads.update(qp_gradients_blocks(ctx.layout, ctx.J_blocks, ctx.r, v, u, k=problem.k, m=problem.m, want=cost))
        if eq:
            grads.update(qp_gradients_eq_blocks(ctx.eq_layout, v, u, m=problem.m, want=eq))
        if cons:
            grads.update(qp_gradients(problem, v, u, cons))
        if "lam" in grads:
            grads["lam"] = torch.where(ctx.lam > 0, grads["lam"], torch.zeros((), dtype=v.dtype, device=v.device))
        grads = {nm: _masked(t, ok) for nm, t in grads.items()}
        for nm in each:
            if nm in ctx.shared:
                grads[nm] = grads[nm].sum(0, keepdim=True)
        blocks, cons = sel(summed, BLOCK_GRADIENTS), sel(summed, ("cons_a", "cons_b"))
        if blocks:
            red = qp_gradients_blocks_shared(ctx.layout, ctx.J_blocks, ctx.r, v, u, k=problem.k, m=problem.m, want=blocks, eq_layout=ctx.eq_layout,
                                             status_fwd=ctx.status, status_adj=ctx.adjoint_status)
            if "lam" in red:
                red["lam"] = torch.where(ctx.lam > 0, red["lam"], torch.zeros((), dtype=v.dtype, device=v.device))
            grads.update(red)
        if cons:
            grads.update(qp_gradients_shared(problem, v, u, cons, status_fwd=ctx.status, status_adj=ctx.adjoint_status))
        return (*[grads.get(nm) for nm in names], None, None, None, None)

    @staticmethod
    def jvp(ctx, dJ_blocks, dr, dlam, dJ_eq_blocks, dr_eq, dcons_a, dcons_b, _dcons_var, _dlayout, _deq_layout, _dparams):
        """torch.autograd.forward_ad: vdot at the saved state from the packed tangents, ONE mo_qp_tangent_rhs_blocks launch + ONE KKT solve on
        the (G, c) problem the forward built.  lam's tangent counts only where lam was added (lam > 0), as its gradient does.  A problem whose
        forward status or tangent-solve status is not MO_STATUS_OK gets a ZERO tangent (the backward's rule); the solve's status words are
        kept (`tangent_status`)."""
        if dlam is not None:
            dlam = torch.where(ctx.lam > 0, dlam, torch.zeros((), dtype=ctx.v.dtype, device=ctx.v.device))
        tangents = _given(BLOCK_TANGENTS, (dJ_blocks, dr, dlam, dJ_eq_blocks, dr_eq, dcons_a, dcons_b))
        return _jvp_result(ctx, *qp_jvp_blocks(ctx.problem, ctx.layout, ctx.J_blocks, ctx.r, ctx.v, tangents, eq_layout=ctx.eq_layout))


def adjoint_status(t: torch.Tensor) -> Optional[torch.Tensor]:
    """The [B] status words of the adjoint solve behind a tensor solve_qp returned (None before the first backward)."""
    seen, todo = set(), [t.grad_fn]
    while todo:
        node = todo.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        if hasattr(node, "adjoint_status"):
            return node.adjoint_status
        todo.extend(fn for fn, _ in node.next_functions)
    return None


def _check_cons(cons_var, cons_a, cons_b) -> None:
    if (cons_var is None) != (cons_a is None) or (cons_a is None) != (cons_b is None):
        raise ValueError("cons_var, cons_a and cons_b come together")
    if cons_var is not None and cons_var.dtype != torch.int32:
        raise ValueError("cons_var must be int32")


def _full(t: Optional[torch.Tensor], B: int) -> Optional[torch.Tensor]:
    """An input of solve_qp with its leading dimension of 1 broadcast over the batch, contiguous."""
    return None if t is None else (t.expand(B, *t.shape[1:]) if t.shape[0] != B else t).contiguous()


def _result(v: torch.Tensor, status: torch.Tensor, n: int, m: int, k: int, return_all: bool, return_status: bool):
    """What solve_qp returns from v = [x | s | y | z]: x or all four slices, the status if asked for, a single result bare."""
    global _PENDING_TANGENT_STATUS
    x = v[:, :n]
    res = (x, v[:, n:n + m], v[:, n + m:n + m + k], v[:, n + m + k:]) if return_all else (x,)
    if _PENDING_TANGENT_STATUS is not None:   # the call ran under forward_ad: tangent_status() finds the words on what it returns
        for t in (v, *res):
            t._mo_tangent_status = _PENDING_TANGENT_STATUS
        _PENDING_TANGENT_STATUS = None
    if return_status:
        res = res + (status,)
    return res[0] if len(res) == 1 else res


def solve_qp(G=None, c=None, J=None, r=None, lam=0.0, A_eq=None, b_eq=None, cons_var=None, cons_a=None, cons_b=None,
             params: Optional[Params] = None, return_all: bool = False, return_status: bool = False, layout: Optional[ResidualLayout] = None,
             J_blocks=None, eq_layout: Optional[ResidualLayout] = None, J_eq_blocks=None, r_eq=None):
    """Solve a batch of QPs   min 1/2 x^T G x + c^T x   s.t.  A_eq x + b_eq = 0,  cons_a[i] x[cons_var[i]] + cons_b[i] >= 0   on the GPU and
    keep the result on the autograd graph.  Give EITHER (G [B, n, n] SYMMETRIC, c [B, n]) OR the least-squares form (J [B, m_r, n], r [B, m_r],
    lam: float or [B] tensor; G = J^T J + lam I, c = J^T r, lam added where > 0).  A_eq [B, k, n] (rows = constraints), b_eq [B, k];
    cons_var int32 [B, m] (never differentiable), cons_a, cons_b [B, m]; a leading dimension of 1 is ONE instance for the whole batch (a
    learned layer's parameters): it is read with stride 0, never copied B times, and its gradient arrives summed over the batch, [1, ...],
    from one batch-reduced launch (mo_qp_gradients_shared).  The constraint triple is shared only if all three have a leading dimension
    of 1.  The residual-block form below follows the same rule: J_blocks, r, lam, J_eq_blocks, r_eq and the constraint triple given once are
    read with stride 0 (J_blocks and lam given once: ONE G for the batch), and their gradients arrive summed, [1, ...], from one
    batch-reduced launch (mo_qp_gradients_blocks_shared).
    OR the residual-block form (the reference's own cost model): layout = a qp.ResidualLayout, J_blocks [B, layout.values] the packed local
    Jacobians, r [B, layout.rows], lam as above; equalities, if any, as eq_layout, J_eq_blocks [B, eq_layout.values], r_eq [B, k] (A_eq = the
    stacked UpdateJacobian, b_eq = r_eq) instead of A_eq / b_eq.  Its gradients arrive in the packed layouts and are computed from the
    blocks alone (QPSolveBlocksFunction).  The three forms are mutually exclusive.
    Returns x [B, n] (return_all: x, s, y, z), and with return_status also the [B] int32 forward status (MO_STATUS_*).

    Gradients: every floating-point input that requires_grad receives one, nothing else is computed.  G's gradient is the one with respect
    to a symmetric G, -1/2 (u_x x^T + x u_x^T).  Problems whose forward or adjoint status is not OK receive zero gradients (see
    QPSolveFunction); adjoint_status(x) returns the adjoint's status words after a backward.  The derivative is that of the KKT conditions
    at the returned point: it is as accurate as the solve (termination_kkt_tol), and at an active inequality the slack sits at the
    interior-point floor, so K is ill-conditioned there by construction."""
    params = params if params is not None else Params()
    if layout is not None or J_blocks is not None or eq_layout is not None or J_eq_blocks is not None or r_eq is not None:
        if G is not None or c is not None or J is not None or A_eq is not None or b_eq is not None:
            raise ValueError("layout= (residual-block input) excludes G, c, J, A_eq and b_eq: the three input forms are mutually exclusive")
        return _solve_qp_blocks(layout, J_blocks, r, lam, eq_layout, J_eq_blocks, r_eq, cons_var, cons_a, cons_b, params, return_all, return_status)
    if (J is None) == (G is None):
        raise ValueError("give either (G, c) or (J, r)")
    ref = J if J is not None else G
    if ref.dim() != 3:
        raise ValueError("G / J must be [B, rows, n]")
    B = max(int(t.shape[0]) for t in (G, c, J, r, A_eq, b_eq, cons_a, cons_b) if t is not None)
    if isinstance(lam, torch.Tensor):
        B = max(B, int(lam.numel()))
    full = lambda t: _full(t, B)
    one = lambda t: None if t is None else (t.contiguous() if int(t.shape[0]) == 1 else _full(t, B))   # given once: passed through
    lam_t = None
    if isinstance(lam, torch.Tensor):
        if J is None:
            raise ValueError("lam belongs to the (J, r) form")
        lam_t = one(lam.reshape(-1))
    elif float(lam) != 0.0:
        if J is None:
            raise ValueError("lam belongs to the (J, r) form")
        lam_t = torch.full((B,), float(lam), dtype=ref.dtype, device=ref.device)
    _check_cons(cons_var, cons_a, cons_b)
    A_t = None if A_eq is None else one(A_eq).transpose(1, 2).contiguous()   # BatchedQP's layout: memory = k x n column-major
    cons = one if cons_var is not None and all(int(t.shape[0]) == 1 for t in (cons_var, cons_a, cons_b)) else full
    v, status = QPSolveFunction.apply(one(G), one(c), one(J), one(r), lam_t, A_t, one(b_eq), cons(cons_a), cons(cons_b),
                                      cons(cons_var), params)
    k = 0 if A_eq is None else int(A_eq.shape[1])
    m = 0 if cons_a is None else int(cons_a.shape[1])
    return _result(v, status, int(ref.shape[2]), m, k, return_all, return_status)


def _solve_qp_blocks(layout, J_blocks, r, lam, eq_layout, J_eq_blocks, r_eq, cons_var, cons_a, cons_b, params, return_all, return_status):
    if layout is None or J_blocks is None or r is None:
        raise ValueError("the residual-block form needs layout, J_blocks and r")
    if (eq_layout is None) != (J_eq_blocks is None) or (eq_layout is None) != (r_eq is None):
        raise ValueError("eq_layout, J_eq_blocks and r_eq come together")
    if eq_layout is not None and (eq_layout.n != layout.n or eq_layout.dtype != layout.dtype or eq_layout.device != layout.device):
        raise ValueError("eq_layout must share n, dtype and device with layout")
    _check_cons(cons_var, cons_a, cons_b)
    tensors = [t for t in (J_blocks, r, J_eq_blocks, r_eq, cons_a, cons_b) if t is not None]
    if isinstance(lam, torch.Tensor):
        lam = lam.reshape(-1)
        tensors.append(lam)
    B = max(int(t.shape[0]) for t in tensors)
    full = lambda t: _full(t, B)
    one = lambda t: None if t is None else (t.contiguous() if int(t.shape[0]) == 1 else _full(t, B))   # given once: passed through
    lam_t = one(lam) if isinstance(lam, torch.Tensor) else torch.full((1,), float(lam), dtype=layout.dtype, device=layout.device)
    cons = one if cons_var is not None and all(int(t.shape[0]) == 1 for t in (cons_var, cons_a, cons_b)) else full
    v, status = QPSolveBlocksFunction.apply(one(J_blocks), one(r), lam_t, one(J_eq_blocks), one(r_eq), cons(cons_a), cons(cons_b),
                                            cons(cons_var), layout, eq_layout, params)
    k = 0 if eq_layout is None else eq_layout.rows
    m = 0 if cons_a is None else int(cons_a.shape[1])
    return _result(v, status, layout.n, m, k, return_all, return_status)
