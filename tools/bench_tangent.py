"""The forward-mode launches of the differentiable QP ("Forward mode"), per launch, event-timed, in one process:
mo_qp_tangent_rhs (dc only; dG + dc; the J-level set dJ + dr + dlambda), the whole JVP (mo_qp_tangent_rhs + mo_kkt_solve, flags = 0) and, IN
THE SAME RUN, their yardsticks: mo_qp_gradients with the matching members and the backward (transposed mo_kkt_solve + mo_qp_gradients).
Prints one JSON line per shape.

  cfg3  n = 64, k = 8, m = 32, m_r = 128 (BASELINE configs[2])        ref8  n = 8, k = 2, m = 4, m_r = 16 (the reference's own size)

Both kernels are data movement.  Algorithmic bytes per problem (what must cross the memory interface once), in elements:
  tangent_J    reads J, dJ (2 m_r n), r, dr (2 m_r), dlambda (1), x, y, z of the state (n + k + m), cons_var (m 32-bit); writes rho (V)
  gradients_J  reads J (m_r n), r (m_r), x and u_x (2 n); writes dJ (m_r n), dr (m_r), dlambda (1)
so the J-level tangent moves the bytes of gradients_J (2 m_r n dominate both): tangent_J_over_gradients_J is the figure to read, against the
spread of a second identical run.  The tangent kernel reads J and dJ TWICE (row products, then column products); the second pass is
expected to come from the cache hierarchy, and the achieved bytes/s are stated against the algorithmic bytes, not the issued ones."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from mini_opt_amd import _lib as L  # noqa: E402
from mini_opt_amd import qp as Q  # noqa: E402
from mini_opt_amd import synth  # noqa: E402

SHAPES = {"cfg3": (64, 8, 32, 128), "ref8": (8, 2, 4, 16)}
HBM = 8.0e12


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3 / reps


def run(shape, dtype, batch, reps, warmup, rounds, only=None):
    n, k, m, m_r = SHAPES[shape]
    dev = torch.device("cuda:0")
    elem = 8 if dtype == torch.float64 else 4
    qp, v, _ = synth.make_batch_torch(n, k, m, m_r, batch, dev, dtype)
    V = qp.V
    lib = L.lib()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    s = Q._stream()
    desc = L.PlanDesc(n, k, m, m_r, Q._DT[dtype], 0, 0, 0, batch)
    plan = C.c_void_p()
    L.check(lib.mo_plan_create(C.byref(desc), C.byref(plan)))
    pj = qp.as_struct()
    # the (G, c) twin of the same problems
    G = torch.empty(batch, n, n, dtype=dtype, device=dev)
    c = torch.empty(batch, n, dtype=dtype, device=dev)
    L.check(lib.mo_linearize(plan, C.byref(pj), batch, P(G), n * n, n, P(c), n, None, s))
    qg = Q.BatchedQP(n=n, k=k, m=m, G=G, c=c, A_eq=qp.A_eq, b_eq=qp.b_eq, cons_var=qp.cons_var, cons_a=qp.cons_a, cons_b=qp.cons_b)
    pg = qg.as_struct()
    new = lambda *shape_: torch.randn(*shape_, dtype=dtype, device=dev)  # noqa: E731
    g = new(batch, V)
    rho, vdot, u = torch.empty_like(g), torch.empty_like(g), torch.empty_like(g)
    status = torch.empty(batch, dtype=torch.int32, device=dev)
    # tangents (inputs of the tangent kernel) and gradients (outputs of the gradient kernel)
    tG, tc, tJ, tr, tlam = new(batch, n, n), new(batch, n), new(batch, m_r, n), new(batch, m_r), new(batch)
    dG, dc, dJ, dr, dlam = (torch.empty_like(t) for t in (tG, tc, tJ, tr, tlam))
    t_c, t_G, t_J = L.QPTangents(), L.QPTangents(), L.QPTangents()
    t_c.dc, t_c.dc_stride = tc.data_ptr(), n
    t_G.dc, t_G.dc_stride, t_G.dG, t_G.dG_stride, t_G.dG_ld = tc.data_ptr(), n, tG.data_ptr(), n * n, n
    t_J.dJ, t_J.dJ_stride, t_J.dJ_ld = tJ.data_ptr(), m_r * n, n
    t_J.dr, t_J.dr_stride, t_J.dlambda, t_J.dlambda_stride = tr.data_ptr(), m_r, tlam.data_ptr(), 1
    g_c, g_G, g_J = L.QPGrads(), L.QPGrads(), L.QPGrads()
    g_c.dc, g_c.dc_stride = dc.data_ptr(), n
    g_G.dc, g_G.dc_stride, g_G.dG, g_G.dG_stride, g_G.dG_ld = dc.data_ptr(), n, dG.data_ptr(), n * n, n
    g_J.dJ, g_J.dJ_stride, g_J.dJ_ld, g_J.dJ_layout = dJ.data_ptr(), m_r * n, n, L.MO_ROW_MAJOR
    g_J.dr, g_J.dr_stride, g_J.dlambda, g_J.dlambda_stride = dr.data_ptr(), m_r, dlam.data_ptr(), 1
    tangent = lambda ps, t: (lambda: L.check(lib.mo_qp_tangent_rhs(plan, C.byref(ps), batch, P(v), V, C.byref(t), P(rho), V, s)))  # noqa: E731
    grads = lambda ps, gr: (lambda: L.check(lib.mo_qp_gradients(plan, C.byref(ps), batch, P(v), V, P(u), V, C.byref(gr), s)))  # noqa: E731
    kkt = lambda ps, flags, rhs, dst: (lambda: L.check(lib.mo_kkt_solve(plan, C.byref(ps), batch, P(v), V, P(rhs), V, flags, P(dst), V, P(status), s)))  # noqa: E731
    kkt(pj, L.MO_KKT_TRANSPOSE, g, u)()   # a real adjoint for the gradient launches

    def jvp():
        tangent(pj, t_J)()
        kkt(pj, 0, rho, vdot)()

    def backward():
        kkt(pj, L.MO_KKT_TRANSPOSE, g, u)()
        grads(pj, g_J)()

    calls = {
        "tangent_c": tangent(pg, t_c), "gradients_c": grads(pg, g_c),
        "tangent_G": tangent(pg, t_G), "gradients_G": grads(pg, g_G),
        "tangent_J": tangent(pj, t_J), "gradients_J": grads(pj, g_J),
        "kkt_solve": kkt(pj, 0, rho, vdot), "kkt_solve_transposed": kkt(pj, L.MO_KKT_TRANSPOSE, g, u),
        "jvp": jvp, "backward": backward,
    }
    if only:   # a profiler's view: the named launches alone
        calls = {key: fn for key, fn in calls.items() if key in only}
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    best = {key: float("inf") for key in calls}
    for _ in range(rounds):  # alternating rounds, best of
        for key, fn in calls.items():
            best[key] = min(best[key], timed(fn, reps))
    state = n + k + m
    algo = {"tangent_c": elem * (n + state + V) + 4 * m, "gradients_c": elem * 2 * n,
            "tangent_G": elem * (n * n + n + state + V) + 4 * m, "gradients_G": elem * (2 * n + n * n + n),
            "tangent_J": elem * (2 * m_r * n + 2 * m_r + 1 + state + V) + 4 * m,
            "gradients_J": elem * (m_r * n + m_r + 2 * n + m_r * n + m_r + 1)}
    res = {"shape": shape, "n": n, "k": k, "m": m, "m_r": m_r, "dtype": str(dtype).split(".")[-1], "batch": batch,
           "kkt_solve_kernel": lib.mo_plan_kkt_solve_kernel(plan, C.byref(pj)).decode(), "status_ok": bool(torch.all(status == 0))}
    res.update({key + "_s": t for key, t in best.items()})
    for lvl in ("c", "G", "J"):
        if "tangent_" + lvl in best and "gradients_" + lvl in best:
            res[f"tangent_{lvl}_over_gradients_{lvl}"] = best["tangent_" + lvl] / best["gradients_" + lvl]
    if "jvp" in best and "backward" in best:
        res["jvp_over_backward"] = best["jvp"] / best["backward"]
    for key, b in algo.items():
        if key not in best:
            continue
        res[key + "_bytes_per_problem"] = b
        res[key + "_TBps"] = b * batch / best[key] / 1e12
        res[key + "_frac_8TBps"] = b * batch / best[key] / HBM
    lib.mo_plan_destroy(plan)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg3,ref8")
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", default=None, help="comma-separated subset of the launches (for a profiler): tangent_J,gradients_J,...")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L.build()
    lines = []
    for sh in a.shapes.split(","):
        res = run(sh, torch.float64 if a.dtype == "f64" else torch.float32, a.batch, a.reps, a.warmup, a.rounds,
                  only=a.calls.split(",") if a.calls else None)
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
