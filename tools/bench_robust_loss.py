"""Robust loss functions for residual-block costs, event-timed per launch, the variants alternating in one
process, the median of --samples launches after --warmup:
  (a) linearise    mo_linearize_blocks; mo_linearize_blocks_weighted with given weights; the two-launch robust route
                   (mo_residual_loss_eval + mo_linearize_blocks_weighted) as two separate series, two_launch_1 and two_launch_2, whose
                   relative gap is the noise margin; the fused mo_linearize_blocks_robust.
  (b) end to end   the outlier fit y = a exp(b t) (12 blocks of 1 x 2, 3 gross outliers per data set) through
                   ConstrainedNonlinearLeastSquares(residual_blocks=True) with a Huber loss (mo_nls_solve_blocks_robust) against the same
                   data without a loss (mo_nls_solve_blocks): wall time per Solve.  No threshold.
Writes one JSON line per shape and part; --out names the text file (profiles/robust_loss_bench.txt).

  A  n = 64, 96 blocks of R = 2, P = 4          C  n = 128, 200 blocks of R = 3, P = 6          (the shapes of profiles/blocks_weighted_bench.txt)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from mini_opt_amd import _lib as L  # noqa: E402
from mini_opt_amd import nls as NLS  # noqa: E402
from mini_opt_amd import qp as Q  # noqa: E402

SHAPES = {"A": (64, 96, 2, 4), "C": (128, 200, 3, 6)}


def layout_for(shape, seed=0):
    n, nb, R, P = SHAPES[shape]
    g = torch.Generator().manual_seed(seed)
    return n, [(tuple(torch.randperm(n, generator=g)[:P].tolist()), R) for _ in range(nb)]


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


def run_linearize(shape, dtype, batch, samples, warmup):
    n, blocks = layout_for(shape)
    dev = torch.device("cuda:0")
    lay = Q.ResidualLayout(n, blocks, dtype=dtype, device=dev)
    kinds = (Q.HUBER, Q.SOFT_L1, Q.CAUCHY, Q.TUKEY)
    loss = Q.ResidualLoss(lay, [(kinds[b % 4], 1.0) for b in range(len(blocks))])
    rows, vals = lay.rows, lay.values
    rnd = lambda *shape_: torch.rand(*shape_, dtype=dtype, device=dev) * 2 - 1  # noqa: E731
    J, r, wg = rnd(batch, vals), rnd(batch, rows), rnd(batch, rows) + 1.5
    G, c, f = torch.empty(batch, n, n, dtype=dtype, device=dev), torch.empty(batch, n, dtype=dtype, device=dev), torch.empty(batch, dtype=dtype, device=dev)
    w = torch.empty(batch, rows, dtype=dtype, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    s, lib = Q._stream(), L.lib()

    def plain():
        L.check(lib.mo_linearize_blocks(lay._plan, lay.h, P(J), vals, P(r), rows, 0.0, None, 0, batch, P(G), n * n, n, P(c), n, P(f), s))

    def weighted():
        L.check(lib.mo_linearize_blocks_weighted(lay._plan, lay.h, P(J), vals, P(r), rows, P(wg), rows, 0.0, None, 0, batch, P(G), n * n, n,
                                                 P(c), n, P(f), s))

    def two_launch():
        L.check(lib.mo_residual_loss_eval(lay._plan, lay.h, loss.h, P(r), rows, batch, P(w), rows, P(f), s))
        L.check(lib.mo_linearize_blocks_weighted(lay._plan, lay.h, P(J), vals, P(r), rows, P(w), rows, 0.0, None, 0, batch, P(G), n * n, n,
                                                 P(c), n, None, s))

    def fused():
        L.check(lib.mo_linearize_blocks_robust(lay._plan, lay.h, P(J), vals, P(r), rows, 0.0, None, 0, batch, P(G), n * n, n, P(c), n, P(f),
                                               loss.h, None, 0, s))

    def loss_only():
        L.check(lib.mo_residual_loss_eval(lay._plan, lay.h, loss.h, P(r), rows, batch, P(w), rows, P(f), s))

    med = medians({"linearize_blocks": plain, "weighted": weighted, "two_launch_1": two_launch, "fused_robust": fused, "two_launch_2": two_launch,
                   "loss_eval": loss_only}, samples, warmup)
    t1, t2 = med["two_launch_1"], med["two_launch_2"]
    noise = abs(t1 - t2) / min(t1, t2)
    two = 0.5 * (t1 + t2)
    return dict(part="linearize", shape=shape, n=n, blocks=len(blocks), values=vals, rows=rows, dtype=str(dtype).split(".")[-1], batch=batch,
                samples=samples, warmup=warmup, seconds={k: round(v, 9) for k, v in med.items()}, noise_margin=round(noise, 4),
                fused_over_two_launch=round(med["fused_robust"] / two, 4), fused_over_weighted=round(med["fused_robust"] / med["weighted"], 4),
                fused_no_slower_than_two_launch_beyond_noise=bool(med["fused_robust"] <= two * (1 + noise)))


def run_fit(batch, repeats):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    t = torch.linspace(0.0, 2.0, 12, dtype=torch.float64)
    a = 1.0 + torch.rand(batch, 1, generator=g, dtype=torch.float64)
    b = -1.0 + 0.7 * torch.rand(batch, 1, generator=g, dtype=torch.float64)
    y = a * torch.exp(b * t) + 0.01 * torch.randn(batch, 12, generator=g, dtype=torch.float64)
    for j in range(3):   # three gross outliers per data set
        col = torch.randint(0, 12, (batch,), generator=g)
        y[torch.arange(batch), col] += (1.0 + torch.rand(batch, generator=g, dtype=torch.float64)) * (2 * torch.randint(0, 2, (batch,), generator=g) - 1)
    Y = y.to(dev)

    def make(i):
        ti = float(t[i])

        def fn(x, want_J):
            e = torch.exp(x[:, 1] * ti)
            return (x[:, 0] * e - Y[:, i]).unsqueeze(1), (torch.stack([e, x[:, 0] * ti * e], dim=1).unsqueeze(1) if want_J else None)
        return fn
    x0 = torch.tensor([[1.0, 0.0]], dtype=torch.float64, device=dev).expand(batch, 2).contiguous()
    out = {}
    for name, loss in (("plain", None), ("huber", NLS.Huber(0.05))):
        prob = NLS.Problem.FromResiduals(2, [NLS.MakeResidual((0, 1), make(i), 1, loss=loss) for i in range(12)])
        solver = NLS.ConstrainedNonlinearLeastSquares(prob, batch=batch, device=dev, residual_blocks=True)
        ts = []
        for _ in range(repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            o = solver.Solve(NLS.Params(), x0)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        err = (solver.variables().cpu() - torch.cat([a, b], dim=1)).abs().max(dim=1).values
        out[name] = dict(seconds_per_solve=round(statistics.median(ts[1:]), 6), mean_outer_iterations=round(float(o.num_iterations.double().mean()), 3),
                         median_distance_from_true_parameters=round(float(err.median()), 5))
    return dict(part="outlier_fit_end_to_end", batch=batch, repeats=repeats, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="A,C")
    ap.add_argument("--fit-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [json.dumps(run_linearize(shape, torch.float64, args.batch, args.samples, args.warmup)) for shape in args.shapes.split(",")]
    lines.append(json.dumps(run_fit(args.batch, args.fit_repeats)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
