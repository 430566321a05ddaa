"""Differentiable batched QP: `.backward()` through QPInteriorPointSolver::Solve.

    kkt_solve       mo_kkt_solve     the KKT system of a state for the caller's right-hand side (direct or transposed)
    qp_gradients    mo_qp_gradients  gradients of a loss with respect to the QP's data from the state v and the adjoint u = K^-T g
    qp_gradients_shared    mo_qp_gradients_shared  the same gradients SUMMED over the batch, for data the whole batch shares
    qp_gradients_blocks, qp_gradients_eq_blocks    the same for residual-block input: gradients of the PACKED local Jacobians
    qp_gradients_blocks_shared    mo_qp_gradients_blocks_shared  those gradients SUMMED over the batch, for blocks the whole batch shares
    qp_tangent_rhs  mo_qp_tangent_rhs  forward mode: rho = F_theta thetadot from the state v and a direction in the QP's data
    qp_jvp          qp_tangent_rhs + kkt_solve: the directional derivative vdot of the whole solution [x | s | y | z]
    qp_tangent_rhs_blocks, qp_jvp_blocks    the same for residual-block input: rho from the PACKED tangents of the blocks
    qp_gradients_blocks_weighted, qp_tangent_rhs_blocks_weighted, qp_jvp_blocks_weighted    the block calls for a cost with one weight per
                    stacked residual row, 1/2 sum_i w_i (J x + r)_i^2: the weights' own gradient and tangent beside the blocks'
    qp_gradients_blocks_weighted_shared    mo_qp_gradients_blocks_weighted_shared  the weighted block gradients SUMMED over the batch, for ONE
                    instance of the blocks under weights and residuals per problem
    solve_qp        the user-facing call: forward = Solve (the kernels of qp.QPInteriorPointSolver, fused where the shape allows),
                    backward = ONE transposed KKT solve + ONE gradient launch for exactly the inputs that require a gradient
                    (+ ONE batch-reduced launch for the inputs given once for the batch, leading dimension 1),
                    jvp (torch.autograd.forward_ad) = ONE tangent launch + ONE KKT solve, for all three input forms

The mathematics is in include/mini_opt_hip.h (above mo_kkt_solve) and DESIGN.md section 4.8.  All arithmetic happens in the HIP library;
torch owns memory, streams and the autograd graph.  Plans are created once per (shape, dtype, device, batch) and cached.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Iterable, NamedTuple, Optional

import torch

from . import _lib as L
from .qp import _DT, BatchedQP, Params, ResidualLayout, _ptr, _stream, jacobian_blocks, linearize_blocks

_PLANS: Dict[tuple, C.c_void_p] = {}

# The members of mo_qp_grads / mo_qp_tangents (dense) and of mo_block_grads / mo_block_shared_grads / mo_block_tangents (blocks):
# name -> (pointer field, stride field, leading-dimension field or None, tail shape as a function of the problem).  The stride of a member is
# the product of its tail, its leading dimension the last entry; cons_a and cons_b share one stride field.  A struct without a member's
# stride field (mo_block_shared_grads: one instance per member) is filled with strided=False.  The order is that of the Functions' inputs.
_DENSE = {
    "G": ("dG", "dG_stride", "dG_ld", lambda p: (p.n, p.n)),
    "c": ("dc", "dc_stride", None, lambda p: (p.n,)),
    "J": ("dJ", "dJ_stride", "dJ_ld", lambda p: (int(p.J.shape[1]), int(p.J.shape[2]))),   # problem.J's rows and leading dimension
    "r": ("dr", "dr_stride", None, lambda p: (p.m_r,)),
    "lam": ("dlambda", "dlambda_stride", None, lambda p: ()),
    "A_eq": ("dA_eq", "dA_stride", "dA_ld", lambda p: (p.n, p.k)),
    "b_eq": ("db_eq", "db_stride", None, lambda p: (p.k,)),
    "cons_a": ("dcons_a", "dcons_stride", None, lambda p: (p.m,)),
    "cons_b": ("dcons_b", "dcons_stride", None, lambda p: (p.m,)),
}
_BLOCK = {   # the problem: a _Blocks
    "J_blocks": ("dJ_blocks", "dJ_stride", None, lambda s: (s.layout.values,)),
    "r": ("dr", "dr_stride", None, lambda s: (s.layout.rows,)),
    "lam": ("dlambda", "dlambda_stride", None, lambda s: ()),
    "J_eq_blocks": ("dJ_eq_blocks", "dJ_eq_stride", None, lambda s: (s.eq_layout.values,)),
    "r_eq": ("dr_eq", "dr_eq_stride", None, lambda s: (s.k,)),
    "cons_a": ("dcons_a", "dcons_stride", None, lambda s: (s.m,)),
    "cons_b": ("dcons_b", "dcons_stride", None, lambda s: (s.m,)),
}
GRADIENTS = tuple(_DENSE)
BLOCK_TANGENTS = tuple(_BLOCK)
BLOCK_GRADIENTS = BLOCK_TANGENTS[:5]    # (the constraint members of a block problem go through the dense entry points)
_DENSE_J, _DENSE_EQ = GRADIENTS[2:5], GRADIENTS[5:7]    # the J-level cost members (G alone belongs to the other level); the equality members
_BLOCK_COST, _BLOCK_EQ, _CONS = BLOCK_TANGENTS[:3], BLOCK_TANGENTS[3:5], BLOCK_TANGENTS[5:]
# the weighted block cost (mo_block_weighted_grads / mo_block_weighted_tangents): the members of _BLOCK and, behind them, the per-row weights
_WEIGHTED = {**_BLOCK, "weights": ("dweights", "dweights_stride", None, lambda s: (s.layout.rows,))}
WEIGHTED_TANGENTS = tuple(_WEIGHTED)
_WEIGHTED_COST = _BLOCK_COST + WEIGHTED_TANGENTS[-1:]


class _Blocks(NamedTuple):
    """What the tails of _BLOCK are functions of; dtype and device are the cost layout's (the equality layout's without one)."""
    layout: Optional[ResidualLayout]
    eq_layout: Optional[ResidualLayout]
    k: int
    m: int

    @property
    def dtype(self):
        return (self.eq_layout if self.layout is None else self.layout).dtype

    @property
    def device(self):
        return (self.eq_layout if self.layout is None else self.layout).device


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
    no_rows = (_DENSE_EQ if problem.k == 0 else ()) + (_CONS if problem.m == 0 else ())
    _check_names(names, kind, GRADIENTS, no_rows, GRADIENTS[:1] if problem.J is not None else _DENSE_J)


def _check_status(st: Optional[torch.Tensor], name: str, B: int, dev) -> None:
    if st is not None and (st.dtype != torch.int32 or tuple(st.shape) != (B,) or not st.is_contiguous() or st.device != dev):
        raise ValueError(f"{name}: expected a contiguous [{B}] int32 tensor on {dev}")


def _outputs(struct, table, problem, want, lead: int, strided: bool = True, zeroed=()):
    """The outputs named in `want` as new [lead, *tail] tensors (lead: B, or 1 for a gradient summed over the batch) and `struct` with their
    pointers, leading dimensions and -- strided -- problem strides.  Names in `zeroed` are zero-filled.  Returns (tensors, struct)."""
    out: Dict[str, torch.Tensor] = {}
    for nm in want:
        ptr, stride, ld, tail = table[nm]
        tail = tail(problem)
        out[nm] = (torch.zeros if nm in zeroed else torch.empty)(lead, *tail, dtype=problem.dtype, device=problem.device)
        if struct is None:
            continue
        setattr(struct, ptr, _ptr(out[nm]))
        if strided:
            setattr(struct, stride, math.prod(tail))
        if ld:
            setattr(struct, ld, tail[-1])
    return out, struct


def _dense_outputs(problem: BatchedQP, want, lead: int, strided: bool):
    """_outputs for mo_qp_grads.  dJ is in problem.J's layout with its leading dimension; the padding beyond the matrix is not written by
    the kernels, so a padded dJ is defined here: zero."""
    g = L.QPGrads()
    col = problem.J_layout == "col"
    if "J" in want:
        g.dJ_layout = L.MO_COL_MAJOR if col else L.MO_ROW_MAJOR
    padded = "J" in want and int(problem.J.shape[2]) > (problem.m_r if col else problem.n)
    return _outputs(g, _DENSE, problem, want, lead, strided, zeroed=("J",) if padded else ())


def _inputs(struct, table, problem, tangents: Dict[str, torch.Tensor], B: int, keep: list, tails=None) -> None:
    """The tangents of a dict into `struct` through _take: pointers, leading dimensions, strides (0: one direction for the batch).  Two members
    behind one stride field (cons_a, cons_b) must agree on it.  `tails`: the tails that are not the table's."""
    strides: Dict[str, int] = {}
    for nm, x in tangents.items():
        ptr, stride, ld, tail = table[nm]
        tail = (tails or {}).get(nm) or tail(problem)
        p, s = _take(x, f"tangent {nm!r}", tail, B, problem.dtype, problem.device, keep)
        if strides.setdefault(stride, s) != s:
            raise ValueError("tangents 'cons_a' and 'cons_b' share one stride: give both per problem or both shared")
        setattr(struct, ptr, p)
        setattr(struct, stride, s)
        if ld:
            setattr(struct, ld, tail[-1])


def _eq_rows(layout: ResidualLayout, eq_layout: Optional[ResidualLayout], k: int) -> int:
    """The equality rows of a block problem: eq_layout's, which must fit `layout`; the caller's k without one."""
    if eq_layout is None:
        return int(k)
    if eq_layout.n != layout.n or eq_layout.dtype != layout.dtype or eq_layout.device != layout.device:
        raise ValueError("eq_layout must share n, dtype and device with layout")
    return eq_layout.rows


def _reduced_launch(dev, query, launch) -> None:
    """A batch-reduced launch: query(bytes*) names its workspace (chunk partials), torch's allocator gives it, launch(workspace, bytes,
    stream) runs on it."""
    nbytes = C.c_int64()
    L.check(query(C.byref(nbytes)))
    work = torch.empty(max(int(nbytes.value), 16), dtype=torch.uint8, device=dev)
    L.check(launch(_ptr(work), int(work.numel()), _stream()))


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
    if want is None:
        want = ((_DENSE_J if problem.J is not None else GRADIENTS[:2]) + (_DENSE_EQ if problem.k else ()) + (_CONS if problem.m else ()))
    want = tuple(want)
    _check_dense_names(problem, want, "gradient")
    out, g = _dense_outputs(problem, want, B, strided=True)
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
    want = tuple(want)
    _check_dense_names(problem, want, "gradient")
    _check_status(status_fwd, "status_fwd", B, problem.device)
    _check_status(status_adj, "status_adj", B, problem.device)
    out, g = _dense_outputs(problem, want, 1, strided=False)
    prob, plan, lib = problem.as_struct(), plan_for(problem, B), L.lib()
    _reduced_launch(problem.device, lambda nbytes: lib.mo_qp_gradients_shared_workspace(plan, C.byref(prob), B, C.byref(g), nbytes),
                    lambda work, nbytes, stream: lib.mo_qp_gradients_shared(plan, C.byref(prob), B, _ptr(vars), problem.V, _ptr(u), problem.V,
                                                                            _ptr(status_fwd), _ptr(status_adj), C.byref(g), work, nbytes, stream))
    return out


def qp_tangent_rhs(problem: BatchedQP, vars: torch.Tensor, tangents: Dict[str, torch.Tensor]) -> torch.Tensor:
    """mo_qp_tangent_rhs: rho [B, V] = F_theta thetadot at the state `vars` [B, V] for the direction `tangents` in the problem's data, the
    right-hand side of the forward-mode system K vdot = -rho.  `tangents` maps the keys of GRADIENTS to tensors in BatchedQP's layouts (the
    layouts qp_gradients returns): "c" [B, n], "G" [B, n, n] (LOWER triangle read as a symmetric matrix, the rest ignored), "A_eq" [B, n, k],
    "b_eq" [B, k], "cons_a", "cons_b" [B, m], "J" in the layout of problem.J (its own leading dimension allowed), "r" [B, m_r], "lam" [B].
    A missing key is a zero tangent; a leading dimension of 1 is one direction shared by the batch."""
    B = _check_state(vars, "vars", problem.V, problem)
    _check_dense_names(problem, tangents, "tangent")
    tails = {}
    if "J" in tangents:   # (its own leading dimension allowed)
        ld = int(tangents["J"].shape[-1]) if tangents["J"].dim() == 3 else 0
        if ld < (problem.m_r if problem.J_layout == "col" else problem.n):
            raise ValueError(f"tangent 'J': leading dimension {ld} below the layout's minimum")
        tails["J"] = (int(problem.J.shape[1]), ld)
    t = L.QPTangents()
    keep = []
    _inputs(t, _DENSE, problem, tangents, B, keep, tails)
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


def _partition(want, shared, r_key: str, J_key: str):
    """(each, summed): the names of `want` computed per problem and the ones a batch-reduced launch sums.  Summed by the kernels: what the
    batch shares (`shared`) -- but r given once against a J / J_blocks per problem, which the reduced launches refuse (dr = -J s_u needs one
    J): that one is formed per problem and summed by _per_problem."""
    summed = [nm for nm in want if nm in shared and not (nm == r_key and J_key not in shared)]
    return [nm for nm in want if nm not in summed], summed


def _per_problem(grads: Dict[str, torch.Tensor], ok: torch.Tensor, shared) -> Dict[str, torch.Tensor]:
    """What follows the per-problem launches of a backward: the zero-masking rule, then the sum over the batch for the names in `shared`."""
    grads = {nm: _masked(t, ok) for nm, t in grads.items()}
    for nm in grads:
        if nm in shared:
            grads[nm] = grads[nm].sum(0, keepdim=True)
    return grads


def _where_lam_added(lam: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """lam's gradient or tangent counts only where lam was added (lam > 0)."""
    return torch.where(lam > 0, t, torch.zeros((), dtype=t.dtype, device=t.device))


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
        each, summed = _partition(want, ctx.shared, "r", "J")
        grads = _per_problem(qp_gradients(problem, v, u, each), ok, ctx.shared) if each else {}
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


def _reads_blocks(names) -> bool:
    """Whether a launch reads the cost blocks: only the J_blocks and r members do."""
    return any(nm in names for nm in _BLOCK_COST[:2])


def _take_cost_blocks(s: _Blocks, J_blocks, r, B: int, keep: list, J_lead: Optional[int] = None):
    """(J pointer, J stride, r pointer, r stride) of the packed cost blocks a launch reads, J_blocks [J_lead or B or 1, values] and
    r [B or 1, rows], through _take."""
    J_name, r_name = _BLOCK_COST[:2]
    return (*_take(J_blocks, J_name, _BLOCK[J_name][3](s), J_lead or B, s.dtype, s.device, keep),
            *_take(r, r_name, _BLOCK[r_name][3](s), B, s.dtype, s.device, keep))


def qp_gradients_blocks(layout: ResidualLayout, J_blocks: torch.Tensor, r: torch.Tensor, vars: torch.Tensor, u: torch.Tensor, k: int = 0,
                        m: int = 0, want: Iterable[str] = ("J_blocks", "r", "lam")) -> Dict[str, torch.Tensor]:
    """mo_qp_gradients_blocks: gradients of a loss with respect to the packed cost blocks of `layout` (the inputs of linearize_blocks) from the
    state `vars` [B, V] and the adjoint `u` [B, V] of the (G, c) problem they were linearised into; k, m: that problem's equality and
    inequality rows (V = n + 2 m + k).  J_blocks [B or 1, values], r [B or 1, rows] (1: shared by the batch; the outputs are per problem).
    Returns the ones named in `want`: "J_blocks" [B, values] (the packing of J_blocks), "r" [B, rows], "lam" [B]."""
    want = tuple(want)
    _check_names(want, "gradient", _BLOCK_COST)
    k, m = int(k), int(m)
    B = _check_state_pair(vars, u, "u", layout.n + 2 * m + k, layout)
    blocks = _Blocks(layout, None, k, m)
    keep = []
    J_ptr, J_stride, r_ptr, r_stride = _take_cost_blocks(blocks, J_blocks, r, B, keep)
    out, g = _outputs(L.BlockGrads(), _BLOCK, blocks, want, B)
    plan = _plan_of(layout.n, k, m, 0, layout.dtype, layout.device, B)
    L.check(L.lib().mo_qp_gradients_blocks(plan, layout.h, J_ptr, J_stride, r_ptr, r_stride, B, _ptr(vars), int(vars.shape[1]), _ptr(u),
                                           int(u.shape[1]), C.byref(g), _stream()))
    return out


def qp_gradients_eq_blocks(eq_layout: ResidualLayout, vars: torch.Tensor, u: torch.Tensor, m: int = 0,
                           want: Iterable[str] = ("J_eq_blocks", "r_eq")) -> Dict[str, torch.Tensor]:
    """mo_qp_gradients_eq_blocks: gradients with respect to the packed equality blocks of `eq_layout` (the inputs of jacobian_blocks; k = its
    rows) from `vars`, `u` [B, n + 2 m + k]: "J_eq_blocks" [B, values] (exactly 0 for a column that loses its global column), "r_eq" [B, k]."""
    want = tuple(want)
    _check_names(want, "gradient", _BLOCK_EQ)
    k = eq_layout.rows
    B = _check_state_pair(vars, u, "u", eq_layout.n + 2 * int(m) + k, eq_layout)
    out, _ = _outputs(None, _BLOCK, _Blocks(None, eq_layout, k, int(m)), want, B)   # (no struct: the entry point takes the two pointers)
    dJ_eq, dr_eq = (_ptr(out.get(nm)) for nm in _BLOCK_EQ)
    plan = _plan_of(eq_layout.n, k, int(m), 0, eq_layout.dtype, eq_layout.device, B)
    L.check(L.lib().mo_qp_gradients_eq_blocks(plan, eq_layout.h, B, _ptr(vars), int(vars.shape[1]), _ptr(u), int(u.shape[1]),
                                              dJ_eq, eq_layout.values, dr_eq, k, _stream()))
    return out


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
    k, m = _eq_rows(layout, eq_layout, k), int(m)
    _check_names(want, "gradient", BLOCK_GRADIENTS, _BLOCK_EQ if eq_layout is None or k == 0 else ())
    V = layout.n + 2 * m + k
    B = _check_state_pair(vars, u, "u", V, layout)
    _check_status(status_fwd, "status_fwd", B, layout.device)
    _check_status(status_adj, "status_adj", B, layout.device)
    blocks = _Blocks(layout, eq_layout, k, m)
    keep = []
    J_ptr = r_ptr = None
    r_stride = 0
    if _reads_blocks(want):
        J_ptr, _, r_ptr, r_stride = _take_cost_blocks(blocks, J_blocks, r, B, keep, J_lead=1)          # ONE instance of J_blocks
        if "r" in want and int(r.shape[0]) != 1:
            raise ValueError("gradient 'r' summed over the batch needs r [1, rows]")
    out, g = _outputs(L.BlockSharedGrads(), _BLOCK, blocks, want, 1, strided=False)
    plan, lib = _plan_of(layout.n, k, m, 0, layout.dtype, layout.device, B), L.lib()
    eq_h = None if eq_layout is None else eq_layout.h
    _reduced_launch(layout.device, lambda nbytes: lib.mo_qp_gradients_blocks_shared_workspace(plan, layout.h, eq_h, r_stride, B, C.byref(g), nbytes),
                    lambda work, nbytes, stream: lib.mo_qp_gradients_blocks_shared(plan, layout.h, J_ptr, r_ptr, r_stride, eq_h, B, _ptr(vars), V,
                                                                                   _ptr(u), V, _ptr(status_fwd), _ptr(status_adj), C.byref(g),
                                                                                   work, nbytes, stream))
    return out


def qp_tangent_rhs_blocks(layout: ResidualLayout, J_blocks: Optional[torch.Tensor], r: Optional[torch.Tensor], vars: torch.Tensor,
                          tangents: Dict[str, torch.Tensor], k: int = 0, m: int = 0, eq_layout: Optional[ResidualLayout] = None,
                          cons_var: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mo_qp_tangent_rhs_blocks: rho [B, V] = F_theta thetadot at the state `vars` [B, V] of the (G, c) problem the blocks were linearised
    into, for a direction in the PACKED block data; no n x n or rows x n matrix is formed.  `tangents` maps "J_blocks" [B, layout.values],
    "r" [B, layout.rows], "lam" [B], "J_eq_blocks" [B, eq_layout.values], "r_eq" [B, k], "cons_a", "cons_b" [B, m] to tensors; a missing key
    is a zero tangent, a leading dimension of 1 is one direction shared by the batch.  J_blocks [B or 1, values] and r [B or 1, rows] are
    needed (and read) only with the "J_blocks" / "r" tangents.  k, m: the problem's equality and inequality rows (k = eq_layout.rows when an
    eq_layout is given); cons_var int32 [B or 1, m] with "cons_a"."""
    n, k, m = layout.n, _eq_rows(layout, eq_layout, k), int(m)
    V = n + 2 * m + k
    B = _check_state(vars, "vars", V, layout)
    no_rows = (_BLOCK_EQ if k == 0 or eq_layout is None else ()) + (_CONS if m == 0 else ())
    _check_names(tangents, "tangent", BLOCK_TANGENTS, no_rows)
    blocks = _Blocks(layout, eq_layout, k, m)
    keep = []
    J_ptr = r_ptr = None
    J_stride = r_stride = 0
    if _reads_blocks(tangents):
        J_ptr, J_stride, r_ptr, r_stride = _take_cost_blocks(blocks, J_blocks, r, B, keep)
    t = L.BlockTangents()
    _inputs(t, _BLOCK, blocks, tangents, B, keep)
    cv_ptr, cv_stride = None, 0
    if m and cons_var is not None:
        cv_ptr, cv_stride = _take(cons_var, "cons_var", (m,), B, torch.int32, layout.device, keep)
    elif "cons_a" in tangents:
        raise ValueError("tangent 'cons_a' needs cons_var")
    rho = torch.empty_like(vars)
    plan = _plan_of(n, k, m, 0, layout.dtype, layout.device, B)
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


def _take_weights(s: _Blocks, weights, B: int, keep: list):
    return _take(weights, "weights", _WEIGHTED["weights"][3](s), B, s.dtype, s.device, keep)


def qp_gradients_blocks_weighted(layout: ResidualLayout, J_blocks: torch.Tensor, r: torch.Tensor, weights: torch.Tensor, vars: torch.Tensor,
                                 u: torch.Tensor, k: int = 0, m: int = 0,
                                 want: Iterable[str] = ("J_blocks", "r", "lam", "weights")) -> Dict[str, torch.Tensor]:
    """mo_qp_gradients_blocks_weighted: qp_gradients_blocks for the cost 1/2 sum_i w_i (J x + r)_i^2, weights [B or 1, rows] (1: one
    instance, read with stride 0).  Returns the ones named in `want`: "J_blocks" [B, values] and "r" [B, rows] (exactly 0 at a row whose
    weight is exactly 0, whatever its data hold), "lam" [B], "weights" [B, rows].  J_blocks [1, values] with weights [B, rows] reads the one
    instance in place; a `want` without "J_blocks" forms no [B, values] tensor."""
    want = tuple(want)
    _check_names(want, "gradient", _WEIGHTED_COST)
    k, m = int(k), int(m)
    B = _check_state_pair(vars, u, "u", layout.n + 2 * m + k, layout)
    blocks = _Blocks(layout, None, k, m)
    keep = []
    J_ptr, J_stride, r_ptr, r_stride = _take_cost_blocks(blocks, J_blocks, r, B, keep)
    w_ptr, w_stride = _take_weights(blocks, weights, B, keep)
    out, g = _outputs(L.BlockWeightedGrads(), _WEIGHTED, blocks, want, B)
    plan = _plan_of(layout.n, k, m, 0, layout.dtype, layout.device, B)
    L.check(L.lib().mo_qp_gradients_blocks_weighted(plan, layout.h, J_ptr, J_stride, r_ptr, r_stride, w_ptr, w_stride, B, _ptr(vars),
                                                    int(vars.shape[1]), _ptr(u), int(u.shape[1]), C.byref(g), _stream()))
    return out


def qp_gradients_blocks_weighted_shared(layout: ResidualLayout, J_blocks: torch.Tensor, r: torch.Tensor, weights: torch.Tensor,
                                        vars: torch.Tensor, u: torch.Tensor, k: int = 0, m: int = 0,
                                        want: Iterable[str] = ("J_blocks", "lam"), status_fwd: Optional[torch.Tensor] = None,
                                        status_adj: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """mo_qp_gradients_blocks_weighted_shared: the gradients of qp_gradients_blocks_weighted named in `want`, SUMMED over the batch, for ONE
    instance of the packed blocks: "J_blocks" [1, values], "r" [1, rows], "lam" [1], "weights" [1, rows].  J_blocks [1, values],
    r [B or 1, rows], weights [B or 1, rows]; "r" needs r [1, rows], "weights" needs weights [1, rows].  k, m: the (G, c) problem's equality
    and inequality rows.  status_fwd / status_adj: [B] int32 status words; a problem counts iff every given word is MO_STATUS_OK (its rows
    of `vars` / `u` / `r` / `weights` may then hold anything).  A row whose weight is exactly 0 in a problem contributes exactly nothing
    to "J_blocks" and "r" from that problem, whatever its r holds.  No [B, values] gradient is formed: the workspace (chunk partials, from
    torch's allocator) is a few packed vectors per CU."""
    want = tuple(want)
    _check_names(want, "gradient", _WEIGHTED_COST)
    k, m = int(k), int(m)
    V = layout.n + 2 * m + k
    B = _check_state_pair(vars, u, "u", V, layout)
    _check_status(status_fwd, "status_fwd", B, layout.device)
    _check_status(status_adj, "status_adj", B, layout.device)
    blocks = _Blocks(layout, None, k, m)
    keep = []
    J_ptr, _, r_ptr, r_stride = _take_cost_blocks(blocks, J_blocks, r, B, keep, J_lead=1)          # ONE instance of J_blocks
    w_ptr, w_stride = _take_weights(blocks, weights, B, keep)
    if "r" in want:
        if int(r.shape[0]) != 1:
            raise ValueError("gradient 'r' summed over the batch needs r [1, rows]")
        r_stride = 0      # (also for a batch of one, where _take reports the row's length)
    if "weights" in want:
        if int(weights.shape[0]) != 1:
            raise ValueError("gradient 'weights' summed over the batch needs weights [1, rows]")
        w_stride = 0
    out, g = _outputs(L.BlockWeightedSharedGrads(), _WEIGHTED, blocks, want, 1, strided=False)
    plan, lib = _plan_of(layout.n, k, m, 0, layout.dtype, layout.device, B), L.lib()
    _reduced_launch(layout.device,
                    lambda nbytes: lib.mo_qp_gradients_blocks_weighted_shared_workspace(plan, layout.h, r_stride, w_stride, B, C.byref(g), nbytes),
                    lambda work, nbytes, stream: lib.mo_qp_gradients_blocks_weighted_shared(plan, layout.h, J_ptr, r_ptr, r_stride, w_ptr, w_stride,
                                                                                            B, _ptr(vars), V, _ptr(u), V, _ptr(status_fwd),
                                                                                            _ptr(status_adj), C.byref(g), work, nbytes, stream))
    return out


def qp_tangent_rhs_blocks_weighted(layout: ResidualLayout, J_blocks: torch.Tensor, r: torch.Tensor, weights: torch.Tensor, vars: torch.Tensor,
                                   tangents: Dict[str, torch.Tensor], k: int = 0, m: int = 0, eq_layout: Optional[ResidualLayout] = None,
                                   cons_var: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mo_qp_tangent_rhs_blocks_weighted: qp_tangent_rhs_blocks for the weighted cost; `tangents` may also hold "weights" [B or 1, rows], the
    direction in the weights.  J_blocks, r and weights [B or 1, ...] are always given."""
    n, k, m = layout.n, _eq_rows(layout, eq_layout, k), int(m)
    V = n + 2 * m + k
    B = _check_state(vars, "vars", V, layout)
    no_rows = (_BLOCK_EQ if k == 0 or eq_layout is None else ()) + (_CONS if m == 0 else ())
    _check_names(tangents, "tangent", WEIGHTED_TANGENTS, no_rows)
    blocks = _Blocks(layout, eq_layout, k, m)
    keep = []
    J_ptr, J_stride, r_ptr, r_stride = _take_cost_blocks(blocks, J_blocks, r, B, keep)
    w_ptr, w_stride = _take_weights(blocks, weights, B, keep)
    t = L.BlockWeightedTangents()
    _inputs(t, _WEIGHTED, blocks, tangents, B, keep)
    cv_ptr, cv_stride = None, 0
    if m and cons_var is not None:
        cv_ptr, cv_stride = _take(cons_var, "cons_var", (m,), B, torch.int32, layout.device, keep)
    elif "cons_a" in tangents:
        raise ValueError("tangent 'cons_a' needs cons_var")
    rho = torch.empty_like(vars)
    plan = _plan_of(n, k, m, 0, layout.dtype, layout.device, B)
    L.check(L.lib().mo_qp_tangent_rhs_blocks_weighted(plan, layout.h, J_ptr, J_stride, r_ptr, r_stride, w_ptr, w_stride,
                                                      None if eq_layout is None else eq_layout.h, cv_ptr, cv_stride, B, _ptr(vars), V,
                                                      C.byref(t), _ptr(rho), V, _stream()))
    return rho


def qp_jvp_blocks_weighted(problem: BatchedQP, layout: ResidualLayout, J_blocks: torch.Tensor, r: torch.Tensor, weights: torch.Tensor,
                           vars: torch.Tensor, tangents: Dict[str, torch.Tensor], eq_layout: Optional[ResidualLayout] = None):
    """qp_jvp_blocks for the weighted cost: one weighted tangent launch and one KKT solve on `problem`, the (G, c) problem
    linearize_blocks(..., weights=weights) / jacobian_blocks built.  Returns (vdot, status)."""
    if problem.n != layout.n or (eq_layout is not None and eq_layout.rows != problem.k):
        raise ValueError("problem does not belong to these layouts (n / k differ)")
    rho = qp_tangent_rhs_blocks_weighted(layout, J_blocks, r, weights, vars, tangents, k=problem.k, m=problem.m, eq_layout=eq_layout,
                                         cons_var=problem.cons_var)
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

    NAMES = BLOCK_TANGENTS

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
        each, summed = _partition(want, ctx.shared, "r", "J_blocks")
        grads: Dict[str, torch.Tensor] = {}
        sel = lambda group, among: [nm for nm in group if nm in among]
        cost, eq, cons = sel(each, _BLOCK_COST), sel(each, _BLOCK_EQ), sel(each, _CONS)
        if cost:
            grads.update(qp_gradients_blocks(ctx.layout, ctx.J_blocks, ctx.r, v, u, k=problem.k, m=problem.m, want=cost))
        if eq:
            grads.update(qp_gradients_eq_blocks(ctx.eq_layout, v, u, m=problem.m, want=eq))
        if cons:
            grads.update(qp_gradients(problem, v, u, cons))
        grads = _per_problem(grads, ok, ctx.shared)
        blocks, cons = sel(summed, BLOCK_GRADIENTS), sel(summed, _CONS)
        if blocks:
            grads.update(qp_gradients_blocks_shared(ctx.layout, ctx.J_blocks, ctx.r, v, u, k=problem.k, m=problem.m, want=blocks,
                                                    eq_layout=ctx.eq_layout, status_fwd=ctx.status, status_adj=ctx.adjoint_status))
        if cons:
            grads.update(qp_gradients_shared(problem, v, u, cons, status_fwd=ctx.status, status_adj=ctx.adjoint_status))
        if "lam" in grads:   # (per problem or summed; zeroing commutes with the mask: lam per problem is never summed here)
            grads["lam"] = _where_lam_added(ctx.lam, grads["lam"])
        return (*[grads.get(nm) for nm in names], None, None, None, None)

    @staticmethod
    def jvp(ctx, dJ_blocks, dr, dlam, dJ_eq_blocks, dr_eq, dcons_a, dcons_b, _dcons_var, _dlayout, _deq_layout, _dparams):
        """torch.autograd.forward_ad: vdot at the saved state from the packed tangents, ONE mo_qp_tangent_rhs_blocks launch + ONE KKT solve on
        the (G, c) problem the forward built.  lam's tangent counts only where lam was added (lam > 0), as its gradient does.  A problem whose
        forward status or tangent-solve status is not MO_STATUS_OK gets a ZERO tangent (the backward's rule); the solve's status words are
        kept (`tangent_status`)."""
        if dlam is not None:
            dlam = _where_lam_added(ctx.lam, dlam)
        tangents = _given(BLOCK_TANGENTS, (dJ_blocks, dr, dlam, dJ_eq_blocks, dr_eq, dcons_a, dcons_b))
        return _jvp_result(ctx, *qp_jvp_blocks(ctx.problem, ctx.layout, ctx.J_blocks, ctx.r, ctx.v, tangents, eq_layout=ctx.eq_layout))


class QPSolveWeightedBlocksFunction(torch.autograd.Function):
    """QPSolveBlocksFunction for the weighted cost 1/2 sum_i w_i (J x + r)_i^2 + 1/2 lam |x|^2.  forward(J_blocks, r, lam, J_eq_blocks, r_eq,
    cons_a, cons_b, weights, cons_var, layout, eq_layout, params) -> (v, status); weights [B or 1, layout.rows].  Any input given once is read
    with stride 0 in the forward: J_blocks [1, values] with weights [B, rows] forms G per problem from the ONE instance of J_blocks.  The
    gradients of the cost members -- J_blocks, r, lam, weights -- come from ONE mo_qp_gradients_blocks_weighted launch per problem; those of
    inputs given once are summed over the batch afterwards ([1, ...]).  With reduce_in_kernel (the last, optional argument of forward) and
    J_blocks given once, the cost members given once come from ONE mo_qp_gradients_blocks_weighted_shared launch instead and only the
    members given per problem go through the per-problem launch, which then forms no [B, values] tensor; the default keeps the bits of
    the per-problem route's sum.  A backward that does not ask for J_blocks' gradient forms no [B, values] tensor.  The equality and
    constraint members go the ways of QPSolveBlocksFunction; so do lam's rule (its gradient and tangent count only where lam > 0) and the
    zero gradients and tangents of problems whose forward, adjoint or tangent status is not OK."""

    NAMES = WEIGHTED_TANGENTS

    @staticmethod
    def forward(ctx, J_blocks, r, lam, J_eq_blocks, r_eq, cons_a, cons_b, weights, cons_var, layout, eq_layout, params, reduce_in_kernel=False):
        ctx.reduce_in_kernel = bool(reduce_in_kernel)
        det = lambda t: None if t is None else t.detach()
        J_blocks, r, lam, J_eq_blocks, r_eq, cons_a, cons_b, weights = (det(t) for t in (J_blocks, r, lam, J_eq_blocks, r_eq, cons_a, cons_b,
                                                                                          weights))
        inputs = (J_blocks, r, lam, J_eq_blocks, r_eq, cons_a, cons_b, weights)
        B = max(int(t.shape[0]) for t in inputs if t is not None)
        once = lambda t: int(t.shape[0]) == 1 and B > 1
        ctx.shared = frozenset(nm for nm, t in zip(QPSolveWeightedBlocksFunction.NAMES, inputs) if t is not None and once(t))
        if once(J_blocks) and once(lam) and once(weights):   # one G for the batch, as QPSolveBlocksFunction
            G, _, _ = linearize_blocks(layout, J_blocks, r[:1], lam_vec=lam, weights=weights)
            _, c, _ = linearize_blocks(layout, J_blocks, r, lam_vec=lam, want_G=False, weights=weights)
        else:
            G, c, _ = linearize_blocks(layout, J_blocks, r, lam_vec=lam, batch=B, weights=weights)
        k = 0 if eq_layout is None else eq_layout.rows
        m = 0 if cons_a is None else int(cons_a.shape[1])
        A_eq = None
        if eq_layout is not None:
            A_eq, _ = jacobian_blocks(eq_layout, J_eq_blocks, r_eq[:1] if once(J_eq_blocks) else r_eq)
        problem = BatchedQP(n=layout.n, k=k, m=m, G=G, c=c, A_eq=A_eq, b_eq=r_eq if k else None, cons_var=cons_var, cons_a=cons_a, cons_b=cons_b)
        ctx.layout, ctx.eq_layout, ctx.J_blocks, ctx.r, ctx.lam, ctx.weights = layout, eq_layout, J_blocks, r, lam, weights
        return _solve_forward(ctx, problem, B, params)

    @staticmethod
    def backward(ctx, g, _g_status):
        problem, v, u, ok = _adjoint(ctx, g)
        names = QPSolveWeightedBlocksFunction.NAMES
        want = [nm for nm, nd in zip(names, ctx.needs_input_grad[:8]) if nd]
        sel = lambda group, among: [nm for nm in group if nm in among]
        cost = sel(want, _WEIGHTED_COST)                     # per problem by default: shared ones are summed by _per_problem
        reduced = [nm for nm in cost if nm in ctx.shared] if ctx.reduce_in_kernel and "J_blocks" in ctx.shared else []
        cost = [nm for nm in cost if nm not in reduced]      # (reduce_in_kernel: what is left has a leading dimension of B; no dJ_blocks)
        each, summed = _partition(sel(want, _BLOCK_EQ + _CONS), ctx.shared, "r", "J_blocks")
        grads: Dict[str, torch.Tensor] = {}
        if cost:
            grads.update(qp_gradients_blocks_weighted(ctx.layout, ctx.J_blocks, ctx.r, ctx.weights, v, u, k=problem.k, m=problem.m, want=cost))
        eq, cons = sel(each, _BLOCK_EQ), sel(each, _CONS)
        if eq:
            grads.update(qp_gradients_eq_blocks(ctx.eq_layout, v, u, m=problem.m, want=eq))
        if cons:
            grads.update(qp_gradients(problem, v, u, cons))
        grads = _per_problem(grads, ok, ctx.shared)
        if reduced:
            grads.update(qp_gradients_blocks_weighted_shared(ctx.layout, ctx.J_blocks, ctx.r, ctx.weights, v, u, k=problem.k, m=problem.m,
                                                             want=reduced, status_fwd=ctx.status, status_adj=ctx.adjoint_status))
        eq, cons = sel(summed, _BLOCK_EQ), sel(summed, _CONS)
        if eq:
            grads.update(qp_gradients_blocks_shared(ctx.layout, None, None, v, u, k=problem.k, m=problem.m, want=eq, eq_layout=ctx.eq_layout,
                                                    status_fwd=ctx.status, status_adj=ctx.adjoint_status))
        if cons:
            grads.update(qp_gradients_shared(problem, v, u, cons, status_fwd=ctx.status, status_adj=ctx.adjoint_status))
        if "lam" in grads:
            grads["lam"] = _where_lam_added(ctx.lam, grads["lam"])
        return (*[grads.get(nm) for nm in names], None, None, None, None, None)

    @staticmethod
    def jvp(ctx, dJ_blocks, dr, dlam, dJ_eq_blocks, dr_eq, dcons_a, dcons_b, dweights, _dcons_var, _dlayout, _deq_layout, _dparams,
            _dreduce=None):
        """torch.autograd.forward_ad: ONE mo_qp_tangent_rhs_blocks_weighted launch + ONE KKT solve; a dual `weights` is the tangent wdot."""
        if dlam is not None:
            dlam = _where_lam_added(ctx.lam, dlam)
        tangents = _given(WEIGHTED_TANGENTS, (dJ_blocks, dr, dlam, dJ_eq_blocks, dr_eq, dcons_a, dcons_b, dweights))
        return _jvp_result(ctx, *qp_jvp_blocks_weighted(ctx.problem, ctx.layout, ctx.J_blocks, ctx.r, ctx.weights, ctx.v, tangents,
                                                        eq_layout=ctx.eq_layout))


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


def _pass_through(data, lam, cons_var, cons_a, cons_b):
    """solve_qp's rule for its inputs.  B is the largest leading dimension among `data`, cons_a, cons_b and a tensor `lam` (flattened).  An
    input with a leading dimension of 1 -- given once for the batch -- stays [1, ...], contiguous; any other is expanded to B, contiguous.
    The constraint triple is shared only if all three are given once, else all three are expanded.  Returns (B, data, lam, (cons_a, cons_b,
    cons_var)); None stays None and a `lam` that is no tensor is returned as it came."""
    _check_cons(cons_var, cons_a, cons_b)
    if isinstance(lam, torch.Tensor):
        lam = lam.reshape(-1)
    B = max(int(t.shape[0]) for t in (*data, cons_a, cons_b, lam) if isinstance(t, torch.Tensor))
    one = lambda t: t.contiguous() if int(t.shape[0]) == 1 else _full(t, B)
    cons = one if cons_var is not None and all(int(t.shape[0]) == 1 for t in (cons_var, cons_a, cons_b)) else (lambda t: _full(t, B))
    opt = lambda f, t: f(t) if isinstance(t, torch.Tensor) else t
    return B, [opt(one, t) for t in data], opt(one, lam), [opt(cons, t) for t in (cons_a, cons_b, cons_var)]


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
             J_blocks=None, eq_layout: Optional[ResidualLayout] = None, J_eq_blocks=None, r_eq=None, weights=None,
             reduce_in_kernel: bool = False):
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
    weights [B or 1, layout.rows] (residual-block form only): one weight per stacked residual row, the cost 1/2 sum_i w_i (J x + r)_i^2 +
    1/2 lam |x|^2 -- confidences per measurement, or a 0 / 1 mask: a row whose weight is exactly 0 contributes exactly nothing, its J values
    and r may be NaN, and its entries of J_blocks.grad and r.grad are exactly 0.  weights.grad arrives as [B, rows] ([1, rows] for a weight
    given once); forward_ad takes a dual `weights`.  Under weights every input given once is still read with stride 0; by default the
    gradients of J_blocks, r, lam and weights given once are formed per problem and summed afterwards (QPSolveWeightedBlocksFunction).
    reduce_in_kernel=True (only with `weights`): with J_blocks given once, the cost members given once -- J_blocks, lam, r, weights -- come
    from ONE batch-reduced launch (mo_qp_gradients_blocks_weighted_shared) and no [B, values] gradient is formed; r [B, rows] and
    weights [B, rows] come from one per-problem launch that does not ask for J_blocks' gradient.  The summed gradients then agree with the
    default route's within rounding, not bit for bit (another order of the sums), which is why the flag is opt-in: the default route
    keeps the bits it has.  Forward values and jvp are untouched; with J_blocks per problem the flag changes nothing.  Without `weights`
    the call is exactly the unweighted one, whatever the flag.
    Returns x [B, n] (return_all: x, s, y, z), and with return_status also the [B] int32 forward status (MO_STATUS_*).

    Gradients: every floating-point input that requires_grad receives one, nothing else is computed.  G's gradient is the one with respect
    to a symmetric G, -1/2 (u_x x^T + x u_x^T).  Problems whose forward or adjoint status is not OK receive zero gradients (see
    QPSolveFunction); adjoint_status(x) returns the adjoint's status words after a backward.  The derivative is that of the KKT conditions
    at the returned point: it is as accurate as the solve (termination_kkt_tol), and at an active inequality the slack sits at the
    interior-point floor, so K is ill-conditioned there by construction."""
    params = params if params is not None else Params()
    if layout is not None or J_blocks is not None or eq_layout is not None or J_eq_blocks is not None or r_eq is not None or weights is not None:
        if G is not None or c is not None or J is not None or A_eq is not None or b_eq is not None:
            raise ValueError("layout= (residual-block input) excludes G, c, J, A_eq and b_eq: the three input forms are mutually exclusive")
        return _solve_qp_blocks(layout, J_blocks, r, lam, eq_layout, J_eq_blocks, r_eq, cons_var, cons_a, cons_b, params, return_all, return_status,
                                weights, reduce_in_kernel)
    if (J is None) == (G is None):
        raise ValueError("give either (G, c) or (J, r)")
    ref = J if J is not None else G
    if ref.dim() != 3:
        raise ValueError("G / J must be [B, rows, n]")
    if J is None and (isinstance(lam, torch.Tensor) or float(lam) != 0.0):
        raise ValueError("lam belongs to the (J, r) form")
    B, (G_t, c_t, J_t, r_t, A_t, b_t), lam_t, cons = _pass_through((G, c, J, r, A_eq, b_eq), lam, cons_var, cons_a, cons_b)
    if not isinstance(lam_t, torch.Tensor):
        lam_t = None if float(lam) == 0.0 else torch.full((B,), float(lam), dtype=ref.dtype, device=ref.device)
    if A_t is not None:
        A_t = A_t.transpose(1, 2).contiguous()   # BatchedQP's layout: memory = k x n column-major
    v, status = QPSolveFunction.apply(G_t, c_t, J_t, r_t, lam_t, A_t, b_t, *cons, params)
    k = 0 if A_eq is None else int(A_eq.shape[1])
    m = 0 if cons_a is None else int(cons_a.shape[1])
    return _result(v, status, int(ref.shape[2]), m, k, return_all, return_status)


def _solve_qp_blocks(layout, J_blocks, r, lam, eq_layout, J_eq_blocks, r_eq, cons_var, cons_a, cons_b, params, return_all, return_status,
                     weights=None, reduce_in_kernel=False):
    if layout is None or J_blocks is None or r is None:
        raise ValueError("the residual-block form needs layout, J_blocks and r")
    if (eq_layout is None) != (J_eq_blocks is None) or (eq_layout is None) != (r_eq is None):
        raise ValueError("eq_layout, J_eq_blocks and r_eq come together")
    k = _eq_rows(layout, eq_layout, 0)
    _, (J_t, r_t, J_eq_t, r_eq_t, w_t), lam_t, cons = _pass_through((J_blocks, r, J_eq_blocks, r_eq, weights), lam, cons_var, cons_a, cons_b)
    if not isinstance(lam_t, torch.Tensor):
        lam_t = torch.full((1,), float(lam), dtype=layout.dtype, device=layout.device)
    if w_t is not None:
        cons_a_t, cons_b_t, cons_var_t = cons
        v, status = QPSolveWeightedBlocksFunction.apply(J_t, r_t, lam_t, J_eq_t, r_eq_t, cons_a_t, cons_b_t, w_t, cons_var_t, layout, eq_layout,
                                                        params, bool(reduce_in_kernel))
    else:
        v, status = QPSolveBlocksFunction.apply(J_t, r_t, lam_t, J_eq_t, r_eq_t, *cons, layout, eq_layout, params)
    m = 0 if cons_a is None else int(cons_a.shape[1])
    return _result(v, status, layout.n, m, k, return_all, return_status)
