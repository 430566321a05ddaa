"""The differentiable QP's launches, per launch, event-timed, in one process: mo_kkt_solve (direct and transposed,
J-level and (G, c) input) on the plan's own kernel -- the fused step kernel's right-hand-side twin where the shape is covered -- and on a
MO_PLAN_FORCE_GENERIC plan, mo_qp_gradients (dc only; dG + dc; the J-level set dJ + dr + dlambda), the forward mo_qp_solve, and the two
yardsticks of mo_kkt_solve: mo_newton_step on the plan's own kernel and on the generic one.  Prints one JSON line per shape.

  cfg3  n = 64, k = 8, m = 32, m_r = 128 (BASELINE configs[2])        ref8  n = 8, k = 2, m = 4, m_r = 16 (the reference's own size)
  n128  n = 128, k = 14, m = 64, m_r = 256 (the 128 tile grid)

mo_kkt_solve does strictly less than the Newton step of the same kernel family (no residual, no alpha) and reads one more V-vector:
kkt_over_step (generic pair) and kkt_over_fused_step (the plan's own pair) are expected at or below 1.1.  backward = the transposed solve +
the gradient launch of the input level; backward_over_forward is that over the ten-iteration forward Solve.  mo_qp_gradients is data movement: achieved bytes/s against its algorithmic bytes (the vectors and matrices it must
read and write once).

  blocksA  n = 64, 96 residual blocks of 2 x 4        blocksC  n = 128, 200 residual blocks of 3 x 6        
Residual-block input: mo_qp_gradients_blocks (dJ_blocks + dr + dlambda) against its yardstick in the same run, mo_qp_gradients (dJ + dr +
dlambda) on the dense scattered stack of the same problems; the forward mo_linearize_blocks; solve_qp(layout=...) forward and backward as
the user calls them (autograd and Python included).  The block launch moves 2 (values + rows) + 2 n elements per problem, the dense one
2 m_r n.

  shared_cfg3  n = 64, m = 32 box rows, (G, c) input, ONE G for the batch        shared_n128  n = 128, m = 64, m_r = 256, ONE J for the batch
Data the batch shares: mo_qp_gradients_shared (dG, or dJ + dlambda) against the route without it, mo_qp_gradients
per problem + a sum over the batch; solve_qp's forward with the shared input given once against the same input expanded by the caller;
the whole backward of both.  Both routes in one process, alternating, best of the rounds, every timing around a synchronise.  The
reduced launch reads 2 n (+ m_r for r) elements per problem; the per-problem route writes and reads back n^2 (m_r n) per problem."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from mini_opt_amd import _lib as L  # noqa: E402
from mini_opt_amd import diff as D  # noqa: E402
from mini_opt_amd import qp as Q  # noqa: E402
from mini_opt_amd import synth  # noqa: E402

SHAPES = {"cfg3": (64, 8, 32, 128), "ref8": (8, 2, 4, 16), "n128": (128, 14, 64, 256)}
BLOCK_SHAPES = {"blocksA": (64, 96, 2, 4), "blocksC": (128, 200, 3, 6)}   # n, blocks, R, P
HBM = 8.0e12


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3 / reps


def run(shape, dtype, batch, reps, warmup, rounds):
    n, k, m, m_r = SHAPES[shape]
    dev = torch.device("cuda:0")
    elem = 8 if dtype == torch.float64 else 4
    qp, v, mu = synth.make_batch_torch(n, k, m, m_r, batch, dev, dtype)
    V = qp.V
    lib = L.lib()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    s = Q._stream()

    def plan_of(flags):
        desc = L.PlanDesc(n, k, m, m_r, Q._DT[dtype], 0, flags, 0, batch)
        plan = C.c_void_p()
        L.check(lib.mo_plan_create(C.byref(desc), C.byref(plan)))
        return plan

    plan, plan_generic = plan_of(0), plan_of(L.MO_PLAN_FORCE_GENERIC)
    pj = qp.as_struct()
    # the (G, c) twin of the same problems
    G = torch.empty(batch, n, n, dtype=dtype, device=dev)
    c = torch.empty(batch, n, dtype=dtype, device=dev)
    L.check(lib.mo_linearize(plan, C.byref(pj), batch, P(G), n * n, n, P(c), n, None, s))
    qg = Q.BatchedQP(n=n, k=k, m=m, G=G, c=c, A_eq=qp.A_eq, b_eq=qp.b_eq, cons_var=qp.cons_var, cons_a=qp.cons_a, cons_b=qp.cons_b)
    pg = qg.as_struct()
    rhs = torch.randn(batch, V, dtype=dtype, device=dev)
    out = torch.empty_like(rhs)
    u = torch.empty_like(rhs)
    delta = torch.empty_like(rhs)
    alpha = torch.empty(batch, 2, dtype=dtype, device=dev)
    status = torch.empty(batch, dtype=torch.int32, device=dev)
    dG = torch.empty(batch, n, n, dtype=dtype, device=dev)
    dc = torch.empty(batch, n, dtype=dtype, device=dev)
    dJ = torch.empty(batch, m_r, n, dtype=dtype, device=dev)
    dr = torch.empty(batch, m_r, dtype=dtype, device=dev)
    dlam = torch.empty(batch, dtype=dtype, device=dev)
    g_c, g_G, g_J = L.QPGrads(), L.QPGrads(), L.QPGrads()
    g_c.dc, g_c.dc_stride = dc.data_ptr(), n
    g_G.dc, g_G.dc_stride, g_G.dG, g_G.dG_stride, g_G.dG_ld = dc.data_ptr(), n, dG.data_ptr(), n * n, n
    g_J.dJ, g_J.dJ_stride, g_J.dJ_ld, g_J.dJ_layout = dJ.data_ptr(), m_r * n, n, L.MO_ROW_MAJOR
    g_J.dr, g_J.dr_stride, g_J.dlambda, g_J.dlambda_stride = dr.data_ptr(), m_r, dlam.data_ptr(), 1
    prm = Q.Params(max_iterations=10)
    solver = Q.QPInteriorPointSolver(qp)
    solver_qp_level = Q.QPInteriorPointSolver(qg)
    kkt = lambda pl, ps, flags, dst: (lambda: L.check(lib.mo_kkt_solve(pl, C.byref(ps), batch, P(v), V, P(rhs), V, flags, P(dst), V, P(status), s)))  # noqa: E731
    step = lambda pl, ps: (lambda: L.check(lib.mo_newton_step(pl, C.byref(ps), batch, P(v), V, P(mu), 1, 0.995, 0, P(delta), V, P(alpha), P(status), s)))  # noqa: E731

    calls = {
        "kkt_solve": kkt(plan, pj, 0, out),
        "kkt_solve_transposed": kkt(plan, pj, L.MO_KKT_TRANSPOSE, u),
        "kkt_solve_generic": kkt(plan_generic, pj, 0, out),
        "kkt_solve_transposed_generic": kkt(plan_generic, pj, L.MO_KKT_TRANSPOSE, out),
        "newton_step_generic": step(plan_generic, pj),
        "newton_step_plan_default": step(plan, pj),
        "kkt_solve_qp_level": kkt(plan, pg, 0, out),
        "kkt_solve_transposed_qp_level": kkt(plan, pg, L.MO_KKT_TRANSPOSE, out),
        "newton_step_plan_default_qp_level": step(plan, pg),
        "gradients_c": lambda: L.check(lib.mo_qp_gradients(plan, C.byref(pg), batch, P(v), V, P(u), V, C.byref(g_c), s)),
        "gradients_G": lambda: L.check(lib.mo_qp_gradients(plan, C.byref(pg), batch, P(v), V, P(u), V, C.byref(g_G), s)),
        "gradients_J": lambda: L.check(lib.mo_qp_gradients(plan, C.byref(pj), batch, P(v), V, P(u), V, C.byref(g_J), s)),
        "forward_solve": lambda: solver.Solve(prm, record_iterations=False),
        "forward_solve_qp_level": lambda: solver_qp_level.Solve(prm, record_iterations=False),
    }
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    best = {key: float("inf") for key in calls}
    for _ in range(rounds):  # alternating rounds, best of
        for key, fn in calls.items():
            best[key] = min(best[key], timed(fn, reps if not key.startswith("forward_solve") else max(1, reps // 4)))
    algo = {"gradients_c": elem * 2 * n, "gradients_G": elem * (2 * n + n * n + n),
            "gradients_J": elem * (m_r * n + m_r + 2 * n + m_r * n + m_r + 1)}
    res = {"shape": shape, "n": n, "k": k, "m": m, "m_r": m_r, "dtype": str(dtype).split(".")[-1], "batch": batch,
           "step_kernel_plan_default": lib.mo_plan_step_kernel(plan, C.byref(pj)).decode(), "solve_kernel": solver.solve_kernel(),
           "kkt_solve_kernel": lib.mo_plan_kkt_solve_kernel(plan, C.byref(pj)).decode(),
           "kkt_solve_kernel_qp_level": lib.mo_plan_kkt_solve_kernel(plan, C.byref(pg)).decode()}
    res.update({key + "_s": t for key, t in best.items()})
    # the generic pair (the yardstick of the first version of mo_kkt_solve), then the plan's own pair
    res["kkt_over_step"] = best["kkt_solve_generic"] / best["newton_step_generic"]
    res["kkt_transposed_over_step"] = best["kkt_solve_transposed_generic"] / best["newton_step_generic"]
    res["kkt_over_fused_step"] = best["kkt_solve"] / best["newton_step_plan_default"]
    res["kkt_transposed_over_fused_step"] = best["kkt_solve_transposed"] / best["newton_step_plan_default"]
    res["kkt_over_fused_step_qp_level"] = best["kkt_solve_qp_level"] / best["newton_step_plan_default_qp_level"]
    res["kkt_transposed_over_fused_step_qp_level"] = best["kkt_solve_transposed_qp_level"] / best["newton_step_plan_default_qp_level"]
    res["backward_s"] = best["kkt_solve_transposed"] + best["gradients_J"]
    res["backward_over_forward"] = res["backward_s"] / best["forward_solve"]
    res["backward_generic_s"] = best["kkt_solve_transposed_generic"] + best["gradients_J"]
    res["backward_generic_over_forward"] = res["backward_generic_s"] / best["forward_solve"]
    res["backward_qp_level_s"] = best["kkt_solve_transposed_qp_level"] + best["gradients_G"]
    res["backward_over_forward_qp_level"] = res["backward_qp_level_s"] / best["forward_solve_qp_level"]
    for key, b in algo.items():
        res[key + "_bytes_per_problem"] = b
        res[key + "_TBps"] = b * batch / best[key] / 1e12
        res[key + "_frac_8TBps"] = b * batch / best[key] / HBM
    for pl in (plan, plan_generic):
        lib.mo_plan_destroy(pl)
    return res


def run_blocks(shape, dtype, batch, reps, warmup, rounds):
    import numpy as np
    n, count, R, Pn = BLOCK_SHAPES[shape]
    dev = torch.device("cuda:0")
    elem = 8 if dtype == torch.float64 else 4
    rng = np.random.default_rng(47)
    blocks = [(tuple(int(i) for i in rng.permutation(n)[:Pn]), R) for _ in range(count)]      # distinct variables: the dense stack can express it
    lay = Q.ResidualLayout(n, blocks, dtype=dtype)
    values, rows = lay.values, lay.rows
    gen = torch.Generator(device=dev).manual_seed(48)
    Jb = torch.rand(batch, values, dtype=dtype, device=dev, generator=gen) * 2 - 1
    r = torch.rand(batch, rows, dtype=dtype, device=dev, generator=gen) * 2 - 1
    v = torch.randn(batch, n, dtype=dtype, device=dev, generator=gen)
    u = torch.randn(batch, n, dtype=dtype, device=dev, generator=gen)
    Jd = torch.zeros(batch, rows, n, dtype=dtype, device=dev)
    for b, (idx, _) in enumerate(blocks):
        Jd[:, b * R:(b + 1) * R, list(idx)] = Jb[:, b * R * Pn:(b + 1) * R * Pn].reshape(batch, Pn, R).transpose(1, 2)
    lib = L.lib()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    s = Q._stream()
    plan_g = D._plan_of(n, 0, 0, 0, dtype, dev, batch)                 # the plan of the (G, c) solve: what the block gradients run on
    dense = Q.BatchedQP(n=n, J=Jd, r=r, lam=0.1)
    plan_d = D.plan_for(dense, batch)
    pd = dense.as_struct()
    dJb, dr, dlam = torch.empty_like(Jb), torch.empty_like(r), torch.empty(batch, dtype=dtype, device=dev)
    dJd = torch.empty_like(Jd)
    gb = L.BlockGrads()
    gb.dJ_blocks, gb.dJ_stride, gb.dr, gb.dr_stride, gb.dlambda, gb.dlambda_stride = dJb.data_ptr(), values, dr.data_ptr(), rows, dlam.data_ptr(), 1
    gd = L.QPGrads()
    gd.dJ, gd.dJ_stride, gd.dJ_ld, gd.dJ_layout = dJd.data_ptr(), rows * n, n, L.MO_ROW_MAJOR
    gd.dr, gd.dr_stride, gd.dlambda, gd.dlambda_stride = dr.data_ptr(), rows, dlam.data_ptr(), 1
    prm = Q.Params(max_iterations=10)
    Jb_leaf, r_leaf = Jb.clone().requires_grad_(True), r.clone().requires_grad_(True)
    gx = torch.randn(batch, n, dtype=dtype, device=dev, generator=gen)
    graph = {}

    def forward():
        graph["x"], graph["status"] = D.solve_qp(layout=lay, J_blocks=Jb_leaf, r=r_leaf, lam=0.1, params=prm, return_status=True)

    def backward():
        Jb_leaf.grad = r_leaf.grad = None
        graph["x"].backward(gx, retain_graph=True)

    calls = {
        "gradients_blocks": lambda: L.check(lib.mo_qp_gradients_blocks(plan_g, lay.h, P(Jb), values, P(r), rows, batch, P(v), n, P(u), n, C.byref(gb), s)),
        "gradients_J_dense": lambda: L.check(lib.mo_qp_gradients(plan_d, C.byref(pd), batch, P(v), n, P(u), n, C.byref(gd), s)),
        "linearize_blocks": lambda: Q.linearize_blocks(lay, Jb, r, lam=0.1),
        "solve_qp_blocks_forward": forward,
        "solve_qp_blocks_backward": backward,
    }
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    best = {key: float("inf") for key in calls}
    for _ in range(rounds):  # alternating rounds, best of
        for key, fn in calls.items():
            best[key] = min(best[key], timed(fn, reps if not key.startswith("solve_qp") else max(1, reps // 4)))
    x = graph["x"]
    qg = Q.BatchedQP(n=n, G=torch.empty(1, n, n, dtype=dtype, device=dev), c=torch.empty(1, n, dtype=dtype, device=dev))
    res = {"shape": shape, "n": n, "blocks": count, "R": R, "P": Pn, "values": values, "rows": rows, "dtype": str(dtype).split(".")[-1],
           "batch": batch, "kkt_solve_kernel": D.kkt_solve_kernel(qg, batch),
           "forward_status_ok": bool(torch.all(graph["status"] == 0)),
           "adjoint_status_ok": bool(torch.all(D.adjoint_status(x) == 0))}
    res.update({key + "_s": t for key, t in best.items()})
    res["blocks_over_dense"] = best["gradients_blocks"] / best["gradients_J_dense"]
    res["backward_over_forward"] = best["solve_qp_blocks_backward"] / best["solve_qp_blocks_forward"]
    algo = {"gradients_blocks": elem * (2 * (values + rows) + 2 * n + 1), "gradients_J_dense": elem * (2 * rows * n + 2 * rows + 2 * n + 1)}
    for key, b in algo.items():
        res[key + "_bytes_per_problem"] = b
        res[key + "_TBps"] = b * batch / best[key] / 1e12
        res[key + "_frac_8TBps"] = b * batch / best[key] / HBM
    return res


SHARED_SHAPES = {"shared_cfg3": (64, 32, 0), "shared_n128": (128, 64, 256)}   # n, m box rows, m_r (0: (G, c) input)


def wall(fn, reps):
    torch.cuda.synchronize()
    import time
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def run_shared(shape, dtype, batch, reps, warmup, rounds):
    n, m, m_r = SHARED_SHAPES[shape]
    dev = torch.device("cuda:0")
    elem = 8 if dtype == torch.float64 else 4
    gen = torch.Generator(device=dev).manual_seed(49)
    rnd = lambda *shape_: torch.rand(*shape_, dtype=dtype, device=dev, generator=gen) * 2 - 1   # noqa: E731
    half = m // 2
    var = torch.arange(half, dtype=torch.int32, device=dev).repeat(2)[None].contiguous()
    a = torch.cat([torch.ones(half, dtype=dtype, device=dev), -torch.ones(half, dtype=dtype, device=dev)])[None].contiguous()
    b = torch.full((1, m), 0.5, dtype=dtype, device=dev)                      # -0.5 <= x_i <= 0.5 for i < m / 2
    cons = dict(cons_var=var, cons_a=a, cons_b=b)
    if m_r:
        one = dict(J=rnd(1, m_r, n))
        per = dict(r=rnd(batch, m_r))
        extra = dict(lam=1e-3)
        name, members = "J", ("J", "lam")
    else:
        U = rnd(n, n)
        one = dict(G=(U @ U.T / n + torch.eye(n, dtype=dtype, device=dev))[None].contiguous())
        per = dict(c=rnd(batch, n))
        extra = {}
        name, members = "G", ("G",)
    prm = Q.Params(max_iterations=10)
    V = n + 2 * m
    v = torch.randn(batch, V, dtype=dtype, device=dev, generator=gen)
    u = torch.randn(batch, V, dtype=dtype, device=dev, generator=gen)
    prob = Q.BatchedQP(n=n, m=m, lam=extra.get("lam", 0.0), **one, **per, **cons)
    graphs = {}

    def forward(key, expanded):
        leaf = (one[name].expand(batch, *one[name].shape[1:]).contiguous() if expanded else one[name].clone()).requires_grad_(True)

        def fn():
            graphs[key] = (leaf, D.solve_qp(**{name: leaf}, **per, **extra, **cons, params=prm))
        return fn

    def backward(key):
        def fn():
            leaf, x = graphs[key]
            leaf.grad = None
            x.backward(torch.ones_like(x), retain_graph=True)
        return fn

    calls = {
        "gradients_shared": lambda: D.qp_gradients_shared(prob, v, u, members),
        "gradients_per_problem_then_sum": lambda: {key: t.sum(0, keepdim=True) for key, t in D.qp_gradients(prob, v, u, members).items()},
        "solve_qp_forward_shared": forward("shared", False),
        "solve_qp_forward_expanded": forward("expanded", True),
        "solve_qp_backward_shared": backward("shared"),
        "solve_qp_backward_expanded": backward("expanded"),
    }
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    best = {key: float("inf") for key in calls}
    for _ in range(rounds):  # alternating rounds, best of
        for key, fn in calls.items():
            best[key] = min(best[key], wall(fn, reps if key.startswith("gradients") else 1))
    mat = (m_r if m_r else n) * n
    res = {"shape": shape, "n": n, "m": m, "m_r": m_r, "dtype": str(dtype).split(".")[-1], "batch": batch,
           "chunks": S_chunks(batch, torch.cuda.get_device_properties(dev).multi_processor_count),
           "forward_bit_equal": bool(torch.equal(graphs["shared"][1], graphs["expanded"][1]))}
    res.update({key + "_s": t for key, t in best.items()})
    res["shared_speedup_gradients"] = best["gradients_per_problem_then_sum"] / best["gradients_shared"]
    res["shared_speedup_forward"] = best["solve_qp_forward_expanded"] / best["solve_qp_forward_shared"]
    res["shared_speedup_backward"] = best["solve_qp_backward_expanded"] / best["solve_qp_backward_shared"]
    res["gradients_shared_bytes"] = elem * (batch * (2 * n + m_r) + mat)                       # x, u_x (and r) of every problem in, one matrix out
    res["gradients_per_problem_then_sum_bytes"] = elem * (batch * (2 * n + 2 * mat) + (mat if m_r else 0) + mat)   # ... + the matrix per problem out and in again
    for key in ("gradients_shared", "gradients_per_problem_then_sum"):
        res[key + "_TBps"] = res[key + "_bytes"] / best[key] / 1e12
    return res


BLOCK_SHARED_SHAPES = {"blocks_shared_n64": (64, 96, 2, 4, 32), "blocks_shared_n128": (128, 200, 3, 6, 64)}   # n, blocks, R, P, m box rows


def run_blocks_shared(shape, dtype, batch, reps, warmup, rounds):
    """J_blocks given once, r per problem: the reduced launch against mo_qp_gradients_blocks + sum(0), and solve_qp(layout=...) forward and
    backward against the call with J_blocks expanded by the caller.  Both routes in one process, alternating, best of `rounds`."""
    import numpy as np
    n, count, R, Pn, m = BLOCK_SHARED_SHAPES[shape]
    dev = torch.device("cuda:0")
    elem = 8 if dtype == torch.float64 else 4
    rng = np.random.default_rng(50)
    blocks = [(tuple(int(i) for i in rng.permutation(n)[:Pn]), R) for _ in range(count)]
    lay = Q.ResidualLayout(n, blocks, dtype=dtype)
    values, rows = lay.values, lay.rows
    gen = torch.Generator(device=dev).manual_seed(50)
    rnd = lambda *shape_: torch.rand(*shape_, dtype=dtype, device=dev, generator=gen) * 2 - 1   # noqa: E731
    J1, r = rnd(1, values), rnd(batch, rows)
    half = m // 2
    var = torch.arange(half, dtype=torch.int32, device=dev).repeat(2)[None].contiguous()
    a = torch.cat([torch.ones(half, dtype=dtype, device=dev), -torch.ones(half, dtype=dtype, device=dev)])[None].contiguous()
    b = torch.full((1, m), 0.5, dtype=dtype, device=dev)
    cons = dict(cons_var=var, cons_a=a, cons_b=b)
    prm = Q.Params(max_iterations=10)
    V = n + 2 * m
    v = torch.randn(batch, V, dtype=dtype, device=dev, generator=gen)
    u = torch.randn(batch, V, dtype=dtype, device=dev, generator=gen)
    members = ("J_blocks", "lam")
    graphs = {}

    def forward(key, expanded):
        leaf = (J1.expand(batch, values).contiguous() if expanded else J1.clone()).requires_grad_(True)

        def fn():
            graphs[key] = (leaf, D.solve_qp(layout=lay, J_blocks=leaf, r=r, lam=0.1, params=prm, **cons))
        return fn

    def backward(key):
        def fn():
            leaf, x = graphs[key]
            leaf.grad = None
            x.backward(torch.ones_like(x), retain_graph=True)
        return fn

    calls = {
        "gradients_blocks_shared": lambda: D.qp_gradients_blocks_shared(lay, J1, r, v, u, m=m, want=members),
        "gradients_blocks_then_sum": lambda: {key: t.sum(0, keepdim=True) for key, t in D.qp_gradients_blocks(lay, J1, r, v, u, m=m, want=members).items()},
        "solve_qp_forward_shared": forward("shared", False),
        "solve_qp_forward_expanded": forward("expanded", True),
        "solve_qp_backward_shared": backward("shared"),
        "solve_qp_backward_expanded": backward("expanded"),
    }
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    best = {key: float("inf") for key in calls}
    for _ in range(rounds):  # alternating rounds, best of
        for key, fn in calls.items():
            best[key] = min(best[key], wall(fn, reps if key.startswith("gradients") else 1))
    res = {"shape": shape, "n": n, "blocks": count, "R": R, "P": Pn, "values": values, "rows": rows, "m": m, "dtype": str(dtype).split(".")[-1],
           "batch": batch, "chunks": S_chunks(batch, torch.cuda.get_device_properties(dev).multi_processor_count),
           "forward_bit_equal": bool(torch.equal(graphs["shared"][1], graphs["expanded"][1]))}
    res.update({key + "_s": t for key, t in best.items()})
    res["shared_speedup_gradients"] = best["gradients_blocks_then_sum"] / best["gradients_blocks_shared"]
    res["shared_speedup_forward"] = best["solve_qp_forward_expanded"] / best["solve_qp_forward_shared"]
    res["shared_speedup_backward"] = best["solve_qp_backward_expanded"] / best["solve_qp_backward_shared"]
    res["gradients_blocks_shared_bytes"] = elem * (batch * (2 * n + rows) + 2 * values)           # x, u_x and r of every problem in, one packed gradient out
    res["gradients_blocks_then_sum_bytes"] = elem * (batch * (2 * n + rows + 2 * values) + 2 * values)   # ... + the packed gradient per problem out and in again
    for key in ("gradients_blocks_shared", "gradients_blocks_then_sum"):
        res[key + "_TBps"] = res[key + "_bytes"] / best[key] / 1e12
    return res


def S_chunks(batch, cus):
    c = max(1, min(cus, (batch + 31) // 32))
    length = max(1, -(-batch // c))
    return -(-batch // length)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg3,ref8")
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L.build()
    lines = []
    for sh in a.shapes.split(","):
        res = (run_blocks if sh in BLOCK_SHAPES else run_shared if sh in SHARED_SHAPES else run_blocks_shared if sh in BLOCK_SHARED_SHAPES else run)(sh, torch.float64 if a.dtype == "f64" else torch.float32, a.batch, a.reps, a.warmup, a.rounds)
        print(json.dumps(res), flush=True)
        lines.append(res)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for res in lines:
                fh.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
