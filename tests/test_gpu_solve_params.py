"""Every Solve kernel against every Solve parameter, on the device (run with -m gpu on an MI355X): mo_qp_solve on every case of
tests/solve_param_cases.py -- one per Solve instantiation: the one-tile kernel, the fp64 template on each grid, stream, y-tile and slot count
incl. the lean ones, the fp32 kernels, the generic kernel LDS-resident and LARGE -- in all 18 cells initial_guess_method x barrier_strategy x
initialize_mu_with_complementarity (initial_mu = 0.05, sigma = 0.3), as a short run (3 iterations) and a full run, plus the cell in which
termination_complementarity_tol alone decides.  The referee is the oracle's Solve with its decision margins (oracle/margins.py); fp32 cases:
the fp64 oracle on the fp32-rounded inputs.

 unconditional   status 0; kkt_initial of iteration 0 (the guess and the initial mu); ip.mu of iteration 0 (not under PREDICTOR_CORRECTOR, whose
                 ip.mu is the corrector's); lagrange = NaN, NaN when k = 0
 clear prefix    the iterations before the oracle's first knife-edge decision: the device ran them, and all 14 record entries agree
                 (NaN-equal).  Whole run clear: termination and iteration count exact, the state, lagrange = {min y, |y|_inf}
 disagreements   a termination or count that differs from the oracle's must sit on a knife edge (margins.Disagreements)
 m = 0           mu from the state is 0, and the flag changes no bit of the outputs but the ip.mu records

Tolerances: fp64 records rtol 1e-6, atol 1e-9 + 1e-12 x the run's largest kkt_initial (test_gpu_parity.py::test_fused_solve_vs_oracle), state
rtol 1e-7 / atol 1e-9; fp32 records rtol / atol 5e-3 (test_fused_f32_solve_iterate_residual), x within 5e-3 |x|_inf.
tests/test_solve_params_oracle_cpu.py asserts how long the clear prefix is and that most full runs are clear throughout."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from mini_opt_amd import _lib as L
from mini_opt_amd import qp as Q
from oracle import margins as M
from tests import solve_param_cases as SP

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def T(a, dt):
    return torch.as_tensor(np.array(a, order="C"), dtype=dt, device=DEV).contiguous()


@functools.lru_cache(maxsize=None)
def solver_of(cid):
    """The case's problems on the device (packed layout) and a solver on them; the plan's Solve kernel is the one the case names."""
    case, d = SP.BY_ID[cid], SP.problems(cid)
    n, k, m, m_r = case.shape
    dt = torch.float64 if case.dtype == "f64" else torch.float32
    common = dict(A_eq=T(d["A"], dt) if k else None, b_eq=T(d["b"], dt) if k else None, cons_var=T(d["cv"], torch.int32) if m else None,
                  cons_a=T(d["ca"], dt) if m else None, cons_b=T(d["cb"], dt) if m else None)
    if SP.level_of(case) == "J":
        J = np.full((SP.B, m_r, n + case.J_extra), 7.7); J[:, :, :n] = d["J"]                    # (columns beyond n: never read)
        prob = Q.BatchedQP(n=n, k=k, m=m, J=T(J, dt), r=T(d["r"], dt), lam=d["lam"], **common)
    else:
        prob = Q.BatchedQP(n=n, k=k, m=m, G=T(np.tril(d["G"]).transpose(0, 2, 1), dt), c=T(d["c"], dt), **common)
    s = Q.QPInteriorPointSolver(prob, force_generic=case.force_generic, no_tiny=case.no_tiny)
    assert s.solve_kernel() == SP.kernel_name(cid), (cid, s.solve_kernel(), SP.kernel_name(cid))
    return s, dt


def solve(cid, kw):
    """mo_qp_solve from the case's user state; lagrange is always passed (the Python wrapper passes NULL when k = 0)."""
    s, dt = solver_of(cid)
    V = s.p_.V
    state = T(SP.problems(cid)["vars"], dt)
    term = torch.full((SP.B,), -7, dtype=torch.int32, device=DEV)
    nit = torch.full((SP.B,), -7, dtype=torch.int32, device=DEV)
    status = torch.full((SP.B,), -7, dtype=torch.int32, device=DEV)
    its = torch.full((SP.B, kw["max_iterations"], L.MO_ITER_RECORD), float("nan"), dtype=dt, device=DEV)
    lag = torch.full((SP.B, 2), 7.0, dtype=dt, device=DEV)
    sp = Q.Params(**kw).as_struct()
    L.check(L.lib().mo_qp_solve(s._plan, C.byref(s._prob), SP.B, C.byref(sp), Q._ptr(state), V, Q._ptr(term), Q._ptr(nit), Q._ptr(its), Q._ptr(lag),
                                Q._ptr(status), Q._stream()))
    torch.cuda.synchronize()
    return dict(term=term.cpu().numpy(), nit=nit.cpu().numpy(), status=status.cpu().numpy(), rec=its.double().cpu().numpy(),
                vars=state.double().cpu().numpy(), lag=lag.double().cpu().numpy(), raw=(state.cpu(), its.cpu(), lag.cpu()))


def close(got, want, rtol, atol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore"):
        return bool(np.all(both_nan | (np.abs(got - want) <= atol + rtol * np.abs(want))))


def check_cell(cid, cell, kind, out, refs, fails, stats, dis):
    case = SP.BY_ID[cid]
    n, k, m, m_r = case.shape
    f32 = case.dtype == "f32"
    tag = "%s %s %s" % (cid, kind, SP.cell_id(cell))
    bad = lambda p, what, *vals: fails.append("%s p%d: %s %s" % (tag, p, what, " ".join(str(v) for v in vals)))
    pc = cell != SP.COMP_CELL and cell.strategy == SP.PREDICTOR_CORRECTOR
    for p, ref in enumerate(refs):
        if out["status"][p] != 0:
            bad(p, "status", out["status"][p])
            continue
        rec, nit, term = out["rec"][p], int(out["nit"][p]), int(out["term"][p])
        if f32:
            rtol, atol = 5e-3, 5e-3
        else:
            rtol, atol = 1e-6, 1e-9 + 1e-12 * float(np.max(ref.records[:, :4]))
        # unconditional
        if not close(rec[0, :4], ref.records[0, :4], rtol, atol):
            bad(p, "kkt_initial of iteration 0", rec[0, :4], ref.records[0, :4])
        if not pc and not close(rec[0, 8], ref.records[0, 8], rtol, atol):
            bad(p, "ip.mu of iteration 0", rec[0, 8], ref.records[0, 8])
        if k == 0 and not np.all(np.isnan(out["lag"][p])):
            bad(p, "lagrange with k = 0", out["lag"][p])
        # the clear prefix
        edge = SP.first_edge(cid, ref.margins)
        n_clear = ref.nit if edge is None else min(edge, ref.nit)
        stats["prefix"] += n_clear; stats["runs"] += 1; stats["clear"] += edge is None
        if nit < n_clear:
            bad(p, "the device stopped inside the oracle's clear prefix", (term, nit), "oracle", (ref.term, ref.nit), "first edge", edge)
        for i in range(min(n_clear, nit)):
            if not close(rec[i], ref.records[i], rtol, atol):
                bad(p, "record of iteration %d (first edge %s)" % (i, edge), rec[i], ref.records[i])
                break
        agrees = (term, nit) == (ref.term, ref.nit)
        if edge is None:
            if not agrees:
                bad(p, "(termination, iterations) of a run that is clear throughout", (term, nit), "oracle", (ref.term, ref.nit))
            else:
                v = out["vars"][p]
                if f32:
                    if np.max(np.abs(v[:n] - ref.vars[:n])) > 5e-3 * np.max(np.abs(ref.vars[:n])):
                        bad(p, "x", np.max(np.abs(v[:n] - ref.vars[:n])), np.max(np.abs(ref.vars[:n])))
                elif not close(v, ref.vars, 1e-7, 1e-9):
                    bad(p, "state", np.max(np.abs(v - ref.vars)))
                if k:
                    y = ref.vars[n + m:n + m + k]
                    if not close(out["lag"][p], [y.min(), np.abs(y).max()], 5e-3 if f32 else 1e-7, 5e-3 if f32 else 1e-9):
                        bad(p, "lagrange", out["lag"][p], [y.min(), np.abs(y).max()])
        try:
            dis.check("%s p%d device %s oracle %s" % (tag, p, (term, nit), (ref.term, ref.nit)), agrees, SP.edge_margins(cid, ref.margins))
        except AssertionError as e:
            fails.append(str(e))


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))


def run_kind(cid, kind):
    refs = SP.referee(cid, kind)
    m = SP.BY_ID[cid].shape[2]
    fails, stats, dis = [], dict(prefix=0, runs=0, clear=0), M.Disagreements("%s %s" % (cid, kind))
    outs = {}
    for cell, cell_refs in refs.items():
        out = outs[cell] = solve(cid, SP.params(cid, cell, kind))
        if kind == "short":                                     # every problem ends (MAX_ITERATIONS, 3)
            for p in range(SP.B):
                if out["status"][p] == 0 and (int(out["term"][p]), int(out["nit"][p])) != (SP.MAX_ITERATIONS, 3):
                    fails.append("%s short %s p%d: ends (%d, %d)" % (cid, SP.cell_id(cell), p, out["term"][p], out["nit"][p]))
        check_cell(cid, cell, kind, out, cell_refs, fails, stats, dis)
    if m == 0:   # no inequalities: mu from the state is 0, and the reference never uses mu -- the flag changes the ip.mu records only
        for g in SP.GUESSES:
            for s in SP.STRATEGIES:
                on, off = outs[SP.Cell(g, s, 1)], outs[SP.Cell(g, s, 0)]
                nit = on["nit"]
                if not all(np.all(on["rec"][p, :nit[p], 8] == 0.0) for p in range(SP.B)):
                    fails.append("%s %s guess %d strategy %d: mu from the state is not 0 with m = 0" % (cid, kind, g, s))
                keep = [c for c in range(L.MO_ITER_RECORD) if c != 8]
                same = (np.array_equal(on["term"], off["term"]) and np.array_equal(nit, off["nit"]) and same_bits(on["raw"][0], off["raw"][0])
                        and same_bits(on["raw"][2], off["raw"][2]) and same_bits(on["raw"][1][:, :, keep], off["raw"][1][:, :, keep]))
                if not same:
                    fails.append("%s %s guess %d strategy %d: the mu flag changes bits of a Solve without inequalities" % (cid, kind, g, s))
    print("\n%s %s: %d runs, %d clear throughout, clear prefix %d iterations in all; %s" % (cid, kind, stats["runs"], stats["clear"], stats["prefix"],
                                                                                          dis.report() if dis.items else "no disagreement"))
    for line in fails:
        print("  FAIL " + line)
    assert not fails, "%d failures, the first: %s" % (len(fails), "\n".join(fails[:6]))


@pytest.mark.parametrize("cid", SP.IDS)
def test_short_runs(cid):
    """All 18 cells, max_iterations = 3."""
    run_kind(cid, "short")


@pytest.mark.parametrize("cid", SP.IDS)
def test_full_runs(cid):
    """All 18 cells to termination_kkt_tol, and the cell in which termination_complementarity_tol decides."""
    run_kind(cid, "full")
