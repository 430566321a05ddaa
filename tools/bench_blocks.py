"""Residual-block input against the dense stack: mo_linearize_blocks vs mo_linearize on the equivalent dense J, and
blocks -> (G, c) -> mo_qp_solve vs the J-level mo_qp_solve, in one process, alternating.  Prints one JSON line per (shape, dtype).

  A  n = 64,  96 blocks of R = 2, P = 4      B  n = 12, 10 blocks of R = 2, P = 3 (qp_test.cc:529)      C  n = 128, 200 blocks of R = 3, P = 6

Algorithmic bytes of the blocks linearisation per problem: elem x (nnz + m_r + n^2 + n + 1) (packed J and r in, G, c, 0.5 |r|^2 out); the
schedule (read from L2 by every workgroup) is reported once.  Kernel-only times: run under rocprofv3 --kernel-trace --stats."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from mini_opt_amd import _lib as L  # noqa: E402
from mini_opt_amd import qp as Q  # noqa: E402

SHAPES = {"A": (64, 96, 2, 4), "B": (12, 10, 2, 3), "C": (128, 200, 3, 6)}
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


def run(shape, dtype, batch, reps, warmup, e2e):
    n, blocks = layout_for(shape)
    lay = Q.ResidualLayout(n, blocks, dtype=dtype)
    dev = lay.device
    m_r, nnz = lay.rows, lay.values
    elem = 8 if dtype == torch.float64 else 4
    Jp = torch.rand(batch, nnz, dtype=dtype, device=dev) * 2 - 1
    r = torch.rand(batch, m_r, dtype=dtype, device=dev) * 2 - 1
    # the equivalent dense stack: every packed value's (row, column) in the m_r x n row-major J
    rows, cols, row = [], [], 0
    for idx, R in blocks:
        for a, j in enumerate(idx):
            for q in range(R):
                rows.append(row + q)
                cols.append(j)
        row += R
    dst = torch.tensor(rows, device=dev) * n + torch.tensor(cols, device=dev)
    Jd = torch.zeros(batch, m_r * n, dtype=dtype, device=dev)
    Jd[:, dst] = Jp
    Jd = Jd.view(batch, m_r, n)
    G = torch.empty(batch, n, n, dtype=dtype, device=dev)
    c = torch.empty(batch, n, dtype=dtype, device=dev)
    f = torch.empty(batch, dtype=dtype, device=dev)
    lib = L.lib()
    desc = L.PlanDesc(n, 0, 0, m_r, Q._DT[dtype], dev.index or 0, 0, 0, batch)
    plan = C.c_void_p()
    L.check(lib.mo_plan_create(C.byref(desc), C.byref(plan)))
    prob = Q.BatchedQP(n=n, J=Jd, r=r, lam=1e-3).as_struct()
    s = Q._stream()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def blk():
        L.check(lib.mo_linearize_blocks(plan, lay.h, P(Jp), nnz, P(r), m_r, 1e-3, None, 0, batch, P(G), n * n, n, P(c), n, P(f), s))

    def dense():
        L.check(lib.mo_linearize(plan, C.byref(prob), batch, P(G), n * n, n, P(c), n, P(f), s))

    for _ in range(warmup):
        blk(); dense()
    tb, td = [], []
    for _ in range(5):  # alternating rounds
        tb.append(timed(blk, reps)); td.append(timed(dense, reps))
    tb, td = min(tb), min(td)
    bytes_blk = elem * (nnz + m_r + n * n + n + 1)
    bytes_dense = elem * (m_r * n + m_r + n * n + n + 1)
    out = {"shape": shape, "dtype": str(dtype).split(".")[-1], "batch": batch, "n": n, "m_r": m_r, "nnz": nnz,
           "blocks_s": tb, "dense_s": td, "speedup": td / tb,
           "blocks_problems_per_s": batch / tb, "dense_problems_per_s": batch / td,
           "bytes_per_problem_blocks": bytes_blk, "bytes_per_problem_dense": bytes_dense,
           "blocks_TBps": bytes_blk * batch / tb / 1e12, "blocks_frac_8TBps": bytes_blk * batch / tb / HBM,
           "dense_TBps": bytes_dense * batch / td / 1e12,
           "schedule_bytes": 4 * (n * n + 1 + n + 1 + m_r + len(blocks) * n) + 16 * (sum(len(i) * (len(i) + 1) // 2 for i, _ in blocks)
                                                                                      + sum(len(i) for i, _ in blocks))}
    if e2e:
        prm = Q.Params(max_iterations=10)
        sg = Q.QPInteriorPointSolver(Q.BatchedQP(n=n, G=G, c=c))
        sj = Q.QPInteriorPointSolver(Q.BatchedQP(n=n, J=Jd, r=r, lam=1e-3))

        def e2e_blk():
            blk()
            sg.Solve(prm, record_iterations=False)

        def e2e_dense():
            sj.Solve(prm, record_iterations=False)

        e2e_blk(); e2e_dense()
        tb2, td2 = [], []
        for _ in range(3):
            tb2.append(timed(e2e_blk, max(1, reps // 4))); td2.append(timed(e2e_dense, max(1, reps // 4)))
        out.update({"e2e_blocks_qp_s": min(tb2), "e2e_dense_qp_s": min(td2), "e2e_speedup": min(td2) / min(tb2),
                    "e2e_solve_kernel_G": sg.solve_kernel(), "e2e_solve_kernel_J": sj.solve_kernel()})
    lib.mo_plan_destroy(plan)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="A,B,C")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L.build()
    lines = []
    for sh in a.shapes.split(","):
        for dt in a.dtypes.split(","):
            res = run(sh, torch.float64 if dt == "f64" else torch.float32, a.batch, a.reps, a.warmup, not a.no_e2e)
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
