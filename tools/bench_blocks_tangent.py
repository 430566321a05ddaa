"""Forward mode for residual-block input ("Forward mode, block input"), per launch, event-timed, in one process and
in the same interleaved rounds:
  tangent_blocks     mo_qp_tangent_rhs_blocks with dJ_blocks + dr + dlambda
  gradients_blocks   (a) mo_qp_gradients_blocks on the same data (dJ_blocks, dr, dlambda)
  tangent_dense      (b) the dense mo_qp_tangent_rhs (dJ + dr + dlambda) on the blocks scattered into the m_r x n row-major stack
  jvp_blocks         mo_qp_tangent_rhs_blocks + mo_kkt_solve (flags = 0) on the (G, c) problem
  backward_blocks    transposed mo_kkt_solve + mo_qp_gradients_blocks
Writes one JSON line per shape and the ratios; --out names the text file (profiles/blocks_tangent_bench.txt).

  A  n = 64, 96 blocks of R = 2, P = 4          C  n = 128, 200 blocks of R = 3, P = 6          (the README's two block shapes)

Algorithmic bytes per problem (what must cross the memory interface once), in elements, nnz = sum R_b P_b, m_r = sum R_b:
  tangent_blocks    reads J_blocks, dJ_blocks (2 nnz), r, dr (2 m_r), dlambda (1), x (n); writes rho (n)
  gradients_blocks  reads J_blocks (nnz), r (m_r), x, u_x (2 n); writes dJ_blocks (nnz), dr (m_r), dlambda (1)
  tangent_dense     reads J, dJ (2 m_r n), r, dr (2 m_r), dlambda (1), x (n); writes rho (n)
The schedule of the layout is shared by the batch and read from L2; it is not counted."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from mini_opt_amd import _lib as L  # noqa: E402
from mini_opt_amd import qp as Q  # noqa: E402

SHAPES = {"A": (64, 96, 2, 4), "C": (128, 200, 3, 6)}
HBM = 8.0e12


def layout_for(shape, seed=0):
    n, nb, R, P = SHAPES[shape]
    g = torch.Generator().manual_seed(seed)
    return n, [(tuple(torch.randperm(n, generator=g)[:P].tolist()), R) for _ in range(nb)]


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3 / reps


def run(shape, dtype, batch, reps, warmup, rounds):
    n, blocks = layout_for(shape)
    lay = Q.ResidualLayout(n, blocks, dtype=dtype)
    dev = lay.device
    m_r, nnz = lay.rows, lay.values
    elem = 8 if dtype == torch.float64 else 4
    lib = L.lib()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    s = Q._stream()
    rnd = lambda *shape_: torch.rand(*shape_, dtype=dtype, device=dev) * 2 - 1  # noqa: E731
    Jp, r, dJp, dr, dlam = rnd(batch, nnz), rnd(batch, m_r), rnd(batch, nnz), rnd(batch, m_r), rnd(batch)
    # the dense stack of the same blocks and of their tangents: every packed value's (row, column) in the m_r x n row-major matrix
    rows, cols, row = [], [], 0
    for idx, R in blocks:
        for j in idx:
            for q in range(R):
                rows.append(row + q)
                cols.append(j)
        row += R
    dst = torch.tensor(rows, device=dev) * n + torch.tensor(cols, device=dev)

    def scatter(packed):
        d = torch.zeros(batch, m_r * n, dtype=dtype, device=dev)
        d[:, dst] = packed
        return d.view(batch, m_r, n)

    Jd, dJd = scatter(Jp), scatter(dJp)
    lam = 0.1
    G, c, _ = Q.linearize_blocks(lay, Jp, r, lam=lam)
    qg = Q.BatchedQP(n=n, G=G, c=c)
    qj = Q.BatchedQP(n=n, J=Jd, r=r, lam=lam)
    pg, pj = qg.as_struct(), qj.as_struct()
    V = n
    plan_g, plan_j = C.c_void_p(), C.c_void_p()
    desc = L.PlanDesc(n, 0, 0, 0, Q._DT[dtype], 0, 0, 0, batch)
    L.check(lib.mo_plan_create(C.byref(desc), C.byref(plan_g)))
    desc = L.PlanDesc(n, 0, 0, m_r, Q._DT[dtype], 0, 0, 0, batch)
    L.check(lib.mo_plan_create(C.byref(desc), C.byref(plan_j)))
    # a real state: the solution of the (G, c) problems, x = -G^-1 c through the KKT solve at x = 0
    v = torch.zeros(batch, V, dtype=dtype, device=dev)
    status = torch.empty(batch, dtype=torch.int32, device=dev)
    kkt = lambda flags, rhs, out: (lambda: L.check(lib.mo_kkt_solve(plan_g, C.byref(pg), batch, P(v), V, P(rhs), V, flags, P(out), V, P(status), s)))  # noqa: E731
    x0 = torch.empty_like(v)
    kkt(0, c, x0)()
    torch.cuda.synchronize()
    v.copy_(x0)
    g = torch.randn(batch, V, dtype=dtype, device=dev)
    rho, rho_d, vdot, u = (torch.empty_like(v) for _ in range(4))
    oJ, orr, olam = torch.empty_like(Jp), torch.empty_like(r), torch.empty_like(dlam)
    tb = L.BlockTangents()
    tb.dJ_blocks, tb.dJ_stride, tb.dr, tb.dr_stride, tb.dlambda, tb.dlambda_stride = dJp.data_ptr(), nnz, dr.data_ptr(), m_r, dlam.data_ptr(), 1
    td = L.QPTangents()
    td.dJ, td.dJ_stride, td.dJ_ld, td.dr, td.dr_stride, td.dlambda, td.dlambda_stride = dJd.data_ptr(), m_r * n, n, dr.data_ptr(), m_r, dlam.data_ptr(), 1
    gb = L.BlockGrads()
    gb.dJ_blocks, gb.dJ_stride, gb.dr, gb.dr_stride, gb.dlambda, gb.dlambda_stride = oJ.data_ptr(), nnz, orr.data_ptr(), m_r, olam.data_ptr(), 1
    tangent_blocks = lambda: L.check(lib.mo_qp_tangent_rhs_blocks(plan_g, lay.h, P(Jp), nnz, P(r), m_r, None, None, 0, batch, P(v), V, C.byref(tb),  # noqa: E731
                                                                  P(rho), V, s))
    gradients_blocks = lambda: L.check(lib.mo_qp_gradients_blocks(plan_g, lay.h, P(Jp), nnz, P(r), m_r, batch, P(v), V, P(u), V, C.byref(gb), s))  # noqa: E731
    tangent_dense = lambda: L.check(lib.mo_qp_tangent_rhs(plan_j, C.byref(pj), batch, P(v), V, C.byref(td), P(rho_d), V, s))  # noqa: E731
    kkt(L.MO_KKT_TRANSPOSE, g, u)()   # a real adjoint for the gradient launches

    def jvp_blocks():
        tangent_blocks()
        kkt(0, rho, vdot)()

    def backward_blocks():
        kkt(L.MO_KKT_TRANSPOSE, g, u)()
        gradients_blocks()

    calls = {"tangent_blocks": tangent_blocks, "gradients_blocks": gradients_blocks, "tangent_dense": tangent_dense, "jvp_blocks": jvp_blocks,
             "backward_blocks": backward_blocks}
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    agree = float(((rho - rho_d).abs().amax(dim=1) / rho_d.abs().amax(dim=1)).max())   # the block and the dense launch computed the same rho
    times = {key: [] for key in calls}
    for _ in range(rounds):  # interleaved rounds
        for key, fn in calls.items():
            times[key].append(timed(fn, reps))
    best = {key: min(ts) for key, ts in times.items()}
    algo = {"tangent_blocks": elem * (2 * nnz + 2 * m_r + 1 + n + n), "gradients_blocks": elem * (2 * nnz + 2 * m_r + 2 * n + 1),
            "tangent_dense": elem * (2 * m_r * n + 2 * m_r + 1 + n + n)}
    res = {"shape": shape, "n": n, "blocks": len(blocks), "nnz": nnz, "m_r": m_r, "dtype": str(dtype).split(".")[-1], "batch": batch,
           "reps": reps, "rounds": rounds, "kkt_solve_kernel": lib.mo_plan_kkt_solve_kernel(plan_g, C.byref(pg)).decode(),
           "status_ok": bool(torch.all(status == 0)), "rho_blocks_vs_dense_rel_inf": agree}
    for key in calls:
        res[key + "_s"] = best[key]
        res[key + "_spread"] = max(times[key]) / best[key]
    res["tangent_blocks_over_gradients_blocks"] = best["tangent_blocks"] / best["gradients_blocks"]
    res["tangent_blocks_over_tangent_dense"] = best["tangent_blocks"] / best["tangent_dense"]
    res["jvp_blocks_over_backward_blocks"] = best["jvp_blocks"] / best["backward_blocks"]
    for key, b in algo.items():
        res[key + "_bytes_per_problem"] = b
        res[key + "_TBps"] = b * batch / best[key] / 1e12
        res[key + "_frac_8TBps"] = b * batch / best[key] / HBM
    lib.mo_plan_destroy(plan_g)
    lib.mo_plan_destroy(plan_j)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="A,C")
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for sh in a.shapes.split(","):
        res = run(sh, torch.float64 if a.dtype == "f64" else torch.float32, a.batch, a.reps, a.warmup, a.rounds)
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
