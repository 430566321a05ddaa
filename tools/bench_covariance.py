"""Parameter covariance (mo_qp_covariance), event-timed per launch, the variants alternating in one process, the
median of --samples launches after --warmup.  Per shape (fp64):
  cov_full_1 / cov_full_2   mo_qp_covariance with the full q x q output, two separate series whose relative gap is the noise margin
  cov_var                   mo_qp_covariance with var_out only
  (a) kkt_solve_loop        the route the project offered before: diff.kkt_solve once per unit right-hand side, n launches (n factorisations)
                            with a positive definite G; --loop-samples rounds (each round is n launches)
  (b) torch                 k = 0: torch.linalg.cholesky + torch.cholesky_inverse; k > 0: torch.linalg.inv of the (n + k) x (n + k) KKT matrix
                            (recorded as an error string if torch cannot run it on this machine)
and the HBM floor: read the lower triangle, write C = about 2 B n^2 8 bytes at 8 TB/s.
Writes one JSON line per shape; --out names the text file (profiles/covariance_bench.txt).

  A  B = 65 536, n = 64, k = 0        B  B = 65 536, n = 64, k = 8        C  B = 16 384, n = 128, k = 0"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from mini_opt_amd import _lib as L  # noqa: E402
from mini_opt_amd import diff as D  # noqa: E402
from mini_opt_amd import qp as Q  # noqa: E402

SHAPES = {"A": (65536, 64, 0), "B": (65536, 64, 8), "C": (16384, 128, 0)}
HBM_BYTES_PER_SECOND = 8.0e12


def sample(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3


def medians(calls, samples, warmup):
    """{name: median seconds}: every variant once per round, `samples` rounds."""
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {key: [] for key in calls}
    for _ in range(samples):
        for key, fn in calls.items():
            times[key].append(sample(fn))
    return {key: statistics.median(ts) for key, ts in times.items()}


def run_shape(shape, batch, samples, warmup, loop_samples):
    B, n, k = SHAPES[shape]
    B = batch or B
    dev, dt = torch.device("cuda:0"), torch.float64
    g = torch.Generator(device="cpu").manual_seed(11)
    chunk = 4096
    G = torch.empty(B, n, n, dtype=dt, device=dev)
    for lo in range(0, B, chunk):                                    # G = J^T J of a 2n x n J: positive definite, symmetric to the bit
        J = torch.randn(min(chunk, B - lo), 2 * n, n, generator=g, dtype=dt).to(dev)
        G[lo:lo + J.shape[0]] = J.transpose(1, 2) @ J
    G = ((G + G.transpose(1, 2)) * 0.5).contiguous()
    A = (torch.rand(B, n, k, generator=g, dtype=dt) * 2 - 1).to(dev) if k else None   # BatchedQP.A_eq: k x n column-major
    cov = torch.empty(B, n, n, dtype=dt, device=dev)
    var = torch.empty(B, n, dtype=dt, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    lib, s = L.lib(), Q._stream()
    desc = L.PlanDesc(n, k, 0, 0, L.MO_F64, 0, 0, 0, B)
    plan = C.c_void_p()
    L.check(lib.mo_plan_create(C.byref(desc), C.byref(plan)))
    prob = L.Problem()
    prob.G, prob.G_stride, prob.G_ld = G.data_ptr(), n * n, n
    if k:
        prob.A_eq, prob.A_stride, prob.A_ld = A.data_ptr(), n * k, k
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def cov_full():
        L.check(lib.mo_qp_covariance(plan, C.byref(prob), B, None, n, None, 0, P(cov), n * n, n, None, 0, P(status), s))

    def cov_var():
        L.check(lib.mo_qp_covariance(plan, C.byref(prob), B, None, n, None, 0, None, 0, 0, P(var), n, P(status), s))

    med = medians({"cov_full_1": cov_full, "cov_var": cov_var, "cov_full_2": cov_full}, samples, warmup)
    assert bool((status == 0).all())
    reference = cov.clone()

    # (a) n unit right-hand sides through mo_kkt_solve: column j of the KKT inverse's top-left block per launch
    V = n + k
    qp = Q.BatchedQP(n=n, k=k, G=G, c=torch.zeros(B, n, dtype=dt, device=dev), A_eq=A, b_eq=torch.zeros(B, k, dtype=dt, device=dev) if k else None)
    state = torch.zeros(B, V, dtype=dt, device=dev)
    rhs = torch.zeros(B, V, dtype=dt, device=dev)
    cols = torch.empty(B, n, n, dtype=dt, device=dev)

    def kkt_loop():
        for j in range(n):
            rhs.zero_()
            rhs[:, j] = -1.0                                         # K delta = -rhs
            out, _ = D.kkt_solve(qp, state, rhs)
            cols[:, j, :] = out[:, :n]
    med.update(medians({"kkt_solve_loop": kkt_loop}, loop_samples, 1))
    loop_err = float(((cols - reference).abs().amax(dim=(1, 2)) / reference.abs().amax(dim=(1, 2))).max())

    # (b) torch's own batched routines
    torch_err = None
    try:
        if k == 0:
            def torch_route():
                return torch.cholesky_inverse(torch.linalg.cholesky(G))
        else:
            K = torch.zeros(B, V, V, dtype=dt, device=dev)
            K[:, :n, :n] = G
            K[:, n:, :n] = A.transpose(1, 2)
            K[:, :n, n:] = A

            def torch_route():
                return torch.linalg.inv(K)[:, :n, :n]
        got = torch_route()
        torch.cuda.synchronize()
        torch_err = float(((got - reference).abs().amax(dim=(1, 2)) / reference.abs().amax(dim=(1, 2))).max())
        del got
        med.update(medians({"torch": torch_route}, max(3, samples // 3), 1))
    except Exception as e:  # noqa: BLE001 -- "if it runs on the machine": the failure is the result
        med["torch"] = None
        torch_err = f"{type(e).__name__}: {e}"[:200]
    lib.mo_plan_destroy(plan)

    t1, t2 = med["cov_full_1"], med["cov_full_2"]
    full = 0.5 * (t1 + t2)
    noise = abs(t1 - t2) / min(t1, t2)
    floor = 2.0 * B * n * n * 8 / HBM_BYTES_PER_SECOND
    ratio = lambda t: None if t is None else round(t / full, 3)  # noqa: E731
    return dict(shape=shape, batch=B, n=n, k=k, dtype="float64", samples=samples, warmup=warmup, loop_samples=loop_samples,
                seconds={key: (None if v is None else round(v, 9)) for key, v in med.items()}, noise_margin=round(noise, 4),
                hbm_floor_seconds=round(floor, 9), floor_over_cov_full=round(floor / full, 4), floor_over_cov_var=round(floor * 0.5 / med["cov_var"], 4),
                cov_var_over_cov_full=round(med["cov_var"] / full, 4), kkt_solve_loop_over_cov_full=ratio(med["kkt_solve_loop"]),
                torch_over_cov_full=ratio(med["torch"]), kkt_solve_loop_max_rel_difference=loop_err, torch_max_rel_difference=torch_err,
                cov_beats_kkt_solve_loop=bool(full * (1 + noise) < med["kkt_solve_loop"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=0, help="override the shapes' batch sizes")
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-samples", type=int, default=3)
    ap.add_argument("--shapes", default="A,B,C")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for shape in args.shapes.split(","):
        lines.append(json.dumps(run_shape(shape, args.batch, args.samples, args.warmup, args.loop_samples)))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
        if args.out:                                                 # (rewritten after every shape: a run cut short keeps what it measured)
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
