"""Per-row weights for residual-block costs, event-timed per launch, variants alternating in one process, the
median of --samples launches after --warmup:
  (a) regression   mo_linearize_blocks, mo_qp_gradients_blocks, mo_qp_tangent_rhs_blocks of a PARENT build of the library (--parent PATH,
                   loaded beside this tree's) timed as two separate series, parent_1 and parent_2, with this tree's in between.  The two
                   series are two loads of the parent (the file and a copy of it: code objects, plans and layouts of their own), so their
                   gap holds what placement costs as well as what time does.  The relative gap between the parent's two series is the noise
                   margin; this tree's time must lie within it of the parent's.
  (b) weighted     the three weighted launches with per-problem J_blocks and with J_blocks given once (stride 0)
  (c) end to end   solve_qp forward + backward with J_blocks [1, values], weights [B, rows], only weights requiring grad, against the
                   caller-side route (expand J, scale J and r by sqrt(w) in torch, unweighted solve_qp): times and torch.cuda.max_memory_allocated
Writes one JSON line per shape and part; --out names the text file (profiles/blocks_weighted_bench.txt).

  A  n = 64, 96 blocks of R = 2, P = 4          C  n = 128, 200 blocks of R = 3, P = 6          (the README's two block shapes)"""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from mini_opt_amd import _lib as L  # noqa: E402
from mini_opt_amd import diff as D  # noqa: E402
from mini_opt_amd import qp as Q  # noqa: E402

SHAPES = {"A": (64, 96, 2, 4), "C": (128, 200, 3, 6)}
TRIO = ("mo_linearize_blocks", "mo_qp_gradients_blocks", "mo_qp_tangent_rhs_blocks")
SETUP = ("mo_plan_create", "mo_plan_destroy", "mo_residual_layout_create", "mo_residual_layout_destroy", "mo_last_error")


def layout_for(shape, seed=0):
    n, nb, R, P = SHAPES[shape]
    g = torch.Generator().manual_seed(seed)
    return n, [(tuple(torch.randperm(n, generator=g)[:P].tolist()), R) for _ in range(nb)]


def open_other(path):
    """Another build of the library beside this tree's: only the calls the regression part needs, with this tree's prototypes (they are
    the parent's: nothing that exists changed signature)."""
    lib, ref = C.CDLL(path), L.lib()
    for name in TRIO + SETUP:
        fn, proto = getattr(lib, name), getattr(ref, name)
        fn.argtypes, fn.restype = proto.argtypes, proto.restype
    return lib


class Handles:
    """The plans and the layout of one library for one shape: the layout's plan (m_r = rows: linearize) and the (G, c) plan."""

    def __init__(self, lib, n, blocks, dtype, batch):
        self.lib = lib
        rows = sum(R for _, R in blocks)
        self.plan_l, self.plan_g, self.lay = C.c_void_p(), C.c_void_p(), C.c_void_p()
        for plan, m_r, mb in ((self.plan_l, rows, 0), (self.plan_g, 0, batch)):
            desc = L.PlanDesc(n, 0, 0, m_r, Q._DT[dtype], 0, 0, 0, mb)
            self.check(lib.mo_plan_create(C.byref(desc), C.byref(plan)))
        rr = (C.c_int32 * len(blocks))(*[R for _, R in blocks])
        pp = (C.c_int32 * len(blocks))(*[len(idx) for idx, _ in blocks])
        flat = [i for idx, _ in blocks for i in idx]
        self.check(lib.mo_residual_layout_create(self.plan_l, len(blocks), rr, pp, (C.c_int32 * len(flat))(*flat), C.byref(self.lay)))

    def check(self, rc):
        if rc != 0:
            raise RuntimeError(self.lib.mo_last_error().decode())

    def close(self):
        self.lib.mo_residual_layout_destroy(self.lay)
        self.lib.mo_plan_destroy(self.plan_l)
        self.lib.mo_plan_destroy(self.plan_g)


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


def run(shape, dtype, batch, samples, warmup, parent):
    n, blocks = layout_for(shape)
    dev = torch.device("cuda:0")
    rows, vals = sum(R for _, R in blocks), sum(R * len(idx) for idx, R in blocks)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    s = Q._stream()
    rnd = lambda *shape_: torch.rand(*shape_, dtype=dtype, device=dev) * 2 - 1  # noqa: E731
    J, r, w, v, u = rnd(batch, vals), rnd(batch, rows), rnd(batch, rows) + 1.5, rnd(batch, n), rnd(batch, n)
    dJ, dr, dlam, dw = rnd(batch, vals), rnd(batch, rows), rnd(batch), rnd(batch, rows)
    G, c, f = torch.empty(batch, n, n, dtype=dtype, device=dev), torch.empty(batch, n, dtype=dtype, device=dev), torch.empty(batch, dtype=dtype, device=dev)
    oJ, orr, olam, ow, rho = torch.empty_like(J), torch.empty_like(r), torch.empty_like(dlam), torch.empty_like(r), torch.empty_like(v)
    base = dict(shape=shape, n=n, blocks=len(blocks), values=vals, rows=rows, dtype=str(dtype).split(".")[-1], batch=batch, samples=samples, warmup=warmup)
    out = []

    def trio(h, weighted=False, J_stride=vals):
        """The three launches on the handles `h`; weighted: the weighted entry points of this tree's library."""
        lib = h.lib
        gb = (L.BlockWeightedGrads if weighted else L.BlockGrads)()
        gb.dJ_blocks, gb.dJ_stride, gb.dr, gb.dr_stride, gb.dlambda, gb.dlambda_stride = oJ.data_ptr(), vals, orr.data_ptr(), rows, olam.data_ptr(), 1
        tb = (L.BlockWeightedTangents if weighted else L.BlockTangents)()
        tb.dJ_blocks, tb.dJ_stride, tb.dr, tb.dr_stride, tb.dlambda, tb.dlambda_stride = dJ.data_ptr(), vals, dr.data_ptr(), rows, dlam.data_ptr(), 1
        if weighted:
            gb.dweights, gb.dweights_stride, tb.dweights, tb.dweights_stride = ow.data_ptr(), rows, dw.data_ptr(), rows
            return {"linearize": lambda: h.check(lib.mo_linearize_blocks_weighted(h.plan_l, h.lay, P(J), J_stride, P(r), rows, P(w), rows, 0.1, None, 0, batch,
                                                                                  P(G), n * n, n, P(c), n, P(f), s)),
                    "gradients": lambda: h.check(lib.mo_qp_gradients_blocks_weighted(h.plan_g, h.lay, P(J), J_stride, P(r), rows, P(w), rows, batch, P(v), n,
                                                                                     P(u), n, C.byref(gb), s)),
                    "tangent": lambda: h.check(lib.mo_qp_tangent_rhs_blocks_weighted(h.plan_g, h.lay, P(J), J_stride, P(r), rows, P(w), rows, None, None, 0,
                                                                                     batch, P(v), n, C.byref(tb), P(rho), n, s))}
        return {"linearize": lambda: h.check(lib.mo_linearize_blocks(h.plan_l, h.lay, P(J), vals, P(r), rows, 0.1, None, 0, batch, P(G), n * n, n, P(c), n,
                                                                     P(f), s)),
                "gradients": lambda: h.check(lib.mo_qp_gradients_blocks(h.plan_g, h.lay, P(J), vals, P(r), rows, batch, P(v), n, P(u), n, C.byref(gb), s)),
                "tangent": lambda: h.check(lib.mo_qp_tangent_rhs_blocks(h.plan_g, h.lay, P(J), vals, P(r), rows, None, None, 0, batch, P(v), n, C.byref(tb),
                                                                        P(rho), n, s))}

    here = Handles(L.lib(), n, blocks, dtype, batch)
    if parent:
        twin = os.path.join(tempfile.mkdtemp(), "libminiopt_hip_parent_twin.so")   # a second load of the parent: dlopen keys on the file
        shutil.copy(parent, twin)
        old, old2 = Handles(open_other(parent), n, blocks, dtype, batch), Handles(open_other(twin), n, blocks, dtype, batch)
        calls = {}
        for series, h in (("parent_1", old), ("this", here), ("parent_2", old2)):
            calls.update({f"{series}.{key}": fn for key, fn in trio(h).items()})
        med = medians(calls, samples, warmup)
        res = dict(base, part="a_regression")
        for key in ("linearize", "gradients", "tangent"):
            p1, p2, t = med[f"parent_1.{key}"], med[f"parent_2.{key}"], med[f"this.{key}"]
            margin = abs(p1 - p2) / min(p1, p2)
            gap = t / min(p1, p2) - 1.0
            res.update({f"{key}_parent_1_s": p1, f"{key}_parent_2_s": p2, f"{key}_this_s": t, f"{key}_noise_margin": margin,
                        f"{key}_this_over_parent_minus_1": gap, f"{key}_within_margin": bool(t <= max(p1, p2) * (1.0 + margin))})
        out.append(res)
        old.close()
        old2.close()
    calls = {f"unweighted.{key}": fn for key, fn in trio(here).items()}
    calls.update({f"weighted.{key}": fn for key, fn in trio(here, weighted=True).items()})
    calls.update({f"weighted_J_once.{key}": fn for key, fn in trio(here, weighted=True, J_stride=0).items()})
    med = medians(calls, samples, warmup)
    out.append(dict(base, part="b_weighted", **{key.replace(".", "_") + "_s": t for key, t in med.items()}))
    here.close()
    J1 = J[:1].clone()
    del calls
    G = c = f = oJ = orr = olam = ow = rho = dJ = dr = dlam = dw = J = v = u = None   # (c) starts from r, w and one instance of J
    torch.cuda.empty_cache()

    # (c) end to end: one J for the batch, per-problem weights, only the weights' gradient
    lay = Q.ResidualLayout(n, blocks, dtype=dtype)
    row_of = torch.cat([off + torch.arange(R, device=dev).repeat(len(idx)) for (idx, R), off in
                        zip(blocks, torch.tensor([0] + [R for _, R in blocks[:-1]]).cumsum(0).tolist())])
    g = rnd(batch, n)

    def weighted_route():
        ww = w.detach().requires_grad_(True)
        x = D.solve_qp(layout=lay, J_blocks=J1, r=r, lam=0.1, weights=ww)
        (x * g).sum().backward()
        return ww.grad

    def caller_route():
        ww = w.detach().requires_grad_(True)
        sq = ww.sqrt()
        x = D.solve_qp(layout=lay, J_blocks=J1.expand(batch, -1) * sq[:, row_of], r=r * sq, lam=0.1)
        (x * g).sum().backward()
        return ww.grad

    res = dict(base, part="c_end_to_end")
    grads = {}
    for name, fn in (("weighted", weighted_route), ("caller_sqrt_w", caller_route)):
        for _ in range(max(1, warmup)):
            grads[name] = fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        floor = torch.cuda.memory_allocated()
        ts = [sample(fn) for _ in range(max(10, samples // 2))]
        res[name + "_s"] = statistics.median(ts)
        res[name + "_max_memory_allocated"] = torch.cuda.max_memory_allocated()
        res[name + "_memory_allocated_before"] = floor
    ga, gb_ = grads["weighted"], grads["caller_sqrt_w"]
    res["grad_rel_inf_between_routes"] = float(((ga - gb_).abs().amax(dim=1) / gb_.abs().amax(dim=1)).max())
    res["caller_over_weighted_time"] = res["caller_sqrt_w_s"] / res["weighted_s"]
    res["caller_over_weighted_peak_memory"] = res["caller_sqrt_w_max_memory_allocated"] / res["weighted_max_memory_allocated"]
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
    ap.add_argument("--parent", default=None, help="a build of the library at the parent commit (libminiopt_hip.so): part (a)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for sh in a.shapes.split(","):
        for res in run(sh, torch.float64 if a.dtype == "f64" else torch.float32, a.batch, a.samples, a.warmup, a.parent):
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
