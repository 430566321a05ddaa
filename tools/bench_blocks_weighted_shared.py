"""Batch-reduced block gradients under per-row weights, event-timed per launch, variants alternating in one
process, the median of --samples launches after --warmup.  J_blocks given once, weights and r per problem:
  (a) launch       mo_qp_gradients_blocks_weighted_shared (dJ_blocks + dlambda, [1, ...]) against the route it replaces:
                   mo_qp_gradients_blocks_weighted writing [B, values] and [B], the zero mask, sum(0).  The replaced route is timed as two
                   independent series (buffers of their own) with the reduced launch in between; their relative gap is the noise margin.
  (b) end to end   solve_qp forward + backward with J_blocks [1, values] requiring grad, with and without reduce_in_kernel: times and
                   torch.cuda.max_memory_allocated
Writes one JSON line per shape and part; --out names the text file.

  A  n = 64, 96 blocks of R = 2, P = 4          C  n = 128, 200 blocks of R = 3, P = 6          (the README's two block shapes)"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from mini_opt_amd import _lib as L  # noqa: E402
from mini_opt_amd import diff as D  # noqa: E402
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


def run(shape, dtype, batch, samples, warmup):
    n, blocks = layout_for(shape)
    dev = torch.device("cuda:0")
    lay = Q.ResidualLayout(n, blocks, dtype=dtype)
    rows, vals, elem = lay.rows, lay.values, torch.empty((), dtype=dtype).element_size()
    rnd = lambda *shape_: torch.rand(*shape_, dtype=dtype, device=dev) * 2 - 1  # noqa: E731
    J1, r, w, v, u = rnd(1, vals), rnd(batch, rows), rnd(batch, rows) + 1.5, rnd(batch, n), rnd(batch, n)
    status = torch.zeros(batch, dtype=torch.int32, device=dev)
    ok = status == 0
    base = dict(shape=shape, n=n, blocks=len(blocks), values=vals, rows=rows, dtype=str(dtype).split(".")[-1], batch=batch, samples=samples, warmup=warmup)
    out = []
    want = ("J_blocks", "lam")
    results = {}

    def reduced():
        results["reduced"] = D.qp_gradients_blocks_weighted_shared(lay, J1, r, w, v, u, want=want, status_fwd=status, status_adj=status)

    def replaced(series):
        def fn():
            each = D.qp_gradients_blocks_weighted(lay, J1, r, w, v, u, want=want)
            results[series] = {key: D._masked(t, ok).sum(0, keepdim=True) for key, t in each.items()}
        return fn

    med = medians({"replaced_1": replaced("replaced_1"), "reduced": reduced, "replaced_2": replaced("replaced_2")}, samples, warmup)
    p1, p2, t = med["replaced_1"], med["replaced_2"], med["reduced"]
    margin = abs(p1 - p2) / min(p1, p2)
    inputs = batch * (2 * n + 2 * rows) * elem + vals * elem
    res = dict(base, part="a_launch", replaced_1_s=p1, replaced_2_s=p2, reduced_s=t, noise_margin=margin,
               replaced_over_reduced=min(p1, p2) / t, reduced_wins_by_more_than_the_margin=bool(t * (1.0 + margin) < min(p1, p2)),
               reduced_algorithmic_bytes=inputs + (vals + 1) * elem,
               # the per-problem launch writes [B, values] and [B]; the mask reads and writes them; sum(0) reads them
               replaced_algorithmic_bytes=inputs + 4 * batch * (vals + 1) * elem + (vals + 1) * elem)
    a, b = results["reduced"]["J_blocks"], results["replaced_1"]["J_blocks"]
    res["J_blocks_rel_inf_between_routes"] = float((a - b).abs().max() / b.abs().max())
    out.append(res)
    results.clear()
    v = u = a = b = None
    torch.cuda.empty_cache()

    # (b) end to end: one J for the batch, per-problem weights and r, only J_blocks' gradient
    g = rnd(batch, n)

    def route(flag):
        def fn():
            Js = J1.detach().clone().requires_grad_(True)
            x = D.solve_qp(layout=lay, J_blocks=Js, r=r, lam=0.1, weights=w, reduce_in_kernel=flag)
            (x * g).sum().backward()
            return Js.grad
        return fn

    res = dict(base, part="b_end_to_end")
    grads = {}
    for name, fn in (("reduce_in_kernel", route(True)), ("default", route(False))):
        for _ in range(max(1, warmup)):
            grads[name] = fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        floor = torch.cuda.memory_allocated()
        ts = [sample(fn) for _ in range(max(10, samples // 2))]
        res[name + "_s"] = statistics.median(ts)
        res[name + "_max_memory_allocated"] = torch.cuda.max_memory_allocated()
        res[name + "_memory_allocated_before"] = floor
    ga, gb = grads["reduce_in_kernel"], grads["default"]
    res["grad_rel_inf_between_routes"] = float((ga - gb).abs().max() / gb.abs().max())
    res["default_over_reduced_time"] = res["default_s"] / res["reduce_in_kernel_s"]
    res["default_over_reduced_peak_memory"] = res["default_max_memory_allocated"] / res["reduce_in_kernel_max_memory_allocated"]
    out.append(res)
    D.clear_plan_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="A,C")
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L.lib()
    lines = []
    for sh in a.shapes.split(","):
        for res in run(sh, torch.float64 if a.dtype == "f64" else torch.float32, a.batch, a.samples, a.warmup):
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
