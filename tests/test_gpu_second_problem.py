"""The second (and third) problem a workgroup of a PERSISTENT kernel takes.

Every kernel outside the fused family launches min(batch, cap x CUs) workgroups and walks the batch with
`for (p = blockIdx.x; p < batch; p += gridDim.x)`, keeping its LDS workspace -- on the LARGE path and in the eigenvalue kernel beyond the LDS
also a slot of the plan's global H_work -- from one problem to the next.  Here every such kernel gets a batch of B = 3 x cap x CUs + 3
problems (cap = the launcher's per-CU ceiling: the real grid can only be smaller, so every workgroup takes at least three problems), every
problem with data of its own, a seeded third of them failing in one of the ways the project reports per problem (s = 0, s < 0, constraint
index outside [0, n), NaN in J / G, duplicated equality row; for the null-space solver a negated G, a large negative diagonal entry, a NaN
and a zero equality row, which is the early exit of its pivot loop).  Outputs are pre-filled with NaN, status words with -1.

  1. nothing is left unwritten, a healthy problem reports 0 and finite outputs, a failing one the status of its kind (NaN outputs where
     include/mini_opt_hip.h says so);
  2. 64 problems that can never be a workgroup's first (index >= cap x CUs; B - 1; at least 16 healthy ones whose predecessor in the
     workgroup, index - cap x CUs, fails) give THE SAME BITS when run as a batch of their own on a fresh plan (one problem per workgroup);
  3. the results meet the oracle at the project's bounds (TOL64 = 1e-10 rel-inf on directions, TOL32 = 2e-3 in fp32, 1e-9 on alpha,
     1e-11 on G, the null-space / eigenvalue / gradient / block bounds of their own tests).  On EVERY healthy problem: NewtonStep,
     linearize, eig, qp_grad (batched or vectorised oracles), and residual / Iterate / kkt_solve of the LARGE cases.  On a seeded SAMPLE of
     the healthy problems, because the oracle is a Python loop per problem: 2048 for residual / Iterate / kkt_solve of the LDS-resident
     cases, 512 for the null-space solver and the block kernels, 128 for the (termination, iterations) of Solve, with no disagreement
     excused (the seeds were checked against the oracle alone: status 0 on every healthy problem, no sampled Solve with a decision on a
     knife edge or a numerically singular KKT matrix);
  4. (LARGE and eig beyond the LDS) a second launch on the same plan gives the same bits, and so does the sample after a launch in which the
     failing problems were replaced by healthy data: the workspace a launch leaves behind does not show;
  5. (LARGE) a plan made for the full batch and launched on its first CUs + 3 problems gives the bits of the full launch.

The eigenvalue kernel beyond the LDS keeps only its vectors in LDS, so its natural grid is 8 workgroups per CU like the LDS-resident one; its
case makes the plan for max_batch = CUs, which bounds the H_work slots, and launch_qp_eig clamps the grid to them: CUs workgroups, cap 1.

Not compared bit for bit: the `ip` record of a problem whose status is not OK (mo_iterate leaves it undefined there).  A duplicated equality
row makes a Schur pivot that is zero up to rounding: the kernel may report OK, FACTORIZATION_FAILED or NONFINITE (test_status_words does not
pin it either); such a problem counts as neither healthy nor failing, but takes part in 1 (written, NaN iff not OK) and 2.
The fp32 cases hold NewtonStep and linearize to the fp64 oracle on fp32-rounded inputs (the bounds of test_batch_vs_oracle and
test_synthetic_fixture); the other modes of the fp32 LARGE case are covered by 1, 2, 4 only.
mo_linearize has cases of its own: its system has k = m = 0, so the kernel and the cap follow from n alone (LARGE from n = 72 on).
The calls go to the C ABI with the argument lists of their Python mirrors, because the mirrors allocate most outputs themselves: that is what
lets every output be pre-filled, a plan be launched twice, and a prefix of a batch be launched on the plan of the whole batch."""
import copy
import ctypes as C
import functools
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from mini_opt_amd import _lib as L
from mini_opt_amd import diff as D
from mini_opt_amd import qp as Q
from oracle import nls_oracle as N
from oracle import oracle as orc
from tests import blocks_diff_reference as BR
from tests import diff_reference as R
from tests.sens_fixtures import UNIT, Plan, device_problem, host_batch, oracle_kkt_solves, oracle_solver, random_layout
from tests.test_gpu_parity import TOL32, TOL64, T, rel_inf_rows, solves_agree_or_knife_edge
from tests.test_gpu_residual_blocks import bound_terms, oracle_hessian, oracle_jacobian, pack_np
from tests.test_gpu_residual_blocks import draw as draw_blocks

pytestmark = pytest.mark.gpu
NAN = float("nan")
F64, F32 = torch.float64, torch.float32
ORACLE_SAMPLE = 2048       # healthy problems held to an oracle that is a Python loop per problem (every healthy problem of a LARGE batch)
SOLVE_SAMPLE = 128         # ... to the replay of the whole Solve with its decision margins (oracle/margins.py), which is slow
SOLVE_KW = dict(initial_mu=1.0, sigma=0.1, termination_kkt_tol=1e-9, max_iterations=8)
OK, SLACK, FACTOR, NONFINITE, BAD_INDEX = (L.MO_STATUS_OK, L.MO_STATUS_NONPOSITIVE_SLACK, L.MO_STATUS_FACTORIZATION_FAILED,
                                           L.MO_STATUS_NONFINITE, L.MO_STATUS_BAD_INDEX)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def batch_for(cap, cu):
    return 3 * cap * cu + 3


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def assert_same_bits(full, ref, rows=None, skip_rows=None, tag=""):
    """Every output of `ref` equals, bit for bit, the rows `rows` of the same output of `full`; `skip_rows`: {name: bool mask over ref's rows}
    of rows that are not compared."""
    assert set(full) == set(ref)
    for name in ref:
        a = full[name] if rows is None else full[name].index_select(0, rows)
        b = ref[name]
        if skip_rows and name in skip_rows:
            keep = torch.as_tensor(~skip_rows[name], device=a.device)
            a, b = a[keep], b[keep]
        assert _same_bits(a, b), (tag, name)


def draw_failures(B, kinds, seed):
    """kind[p] = -1 (healthy) or the index into `kinds` of the failure of problem p: a seeded random third fails, cycling through the kinds."""
    rng = np.random.default_rng(seed)
    kind = np.full(B, -1, dtype=np.int64)
    if kinds:
        bad = np.flatnonzero(rng.random(B) < 1.0 / 3.0)
        kind[bad] = np.arange(len(bad)) % len(kinds)
    return kind


def pick_sample(B, first, healthy, failing, seed):
    """64 problems that are never a workgroup's first (index >= first = cap x CUs): B - 1, at least 16 healthy ones whose predecessor
    `first` problems earlier fails (wherever the real grid is first / j, that predecessor ran in the same workgroup), seeded random others."""
    rng = np.random.default_rng(seed)
    cand = np.arange(first, B - 1)
    after_failure = cand[healthy[cand] & failing[cand - first]]
    chosen = {B - 1}
    if failing.any():
        assert len(after_failure) >= 16, len(after_failure)
        chosen.update(int(p) for p in rng.permutation(after_failure)[:24])
    for p in rng.permutation(cand):
        if len(chosen) == 64:
            break
        chosen.add(int(p))
    return np.array(sorted(chosen))


def oracle_sample(healthy, seed, count=512):
    idx = np.flatnonzero(healthy)
    return np.sort(np.random.default_rng(seed).permutation(idx)[:count])


def full(shape, dt, value=NAN):
    return torch.full(shape, value, dtype=dt, device="cuda:0")


# =====================================================================================================================================
# the three generic families: kkt_generic_kernel LDS-resident on 64 and on 256 threads, and LARGE
# =====================================================================================================================================
@dataclass(frozen=True)
class Case:
    n: int
    k: int
    m: int
    m_r: int
    level: str      # "J": (J, r, lambda) input, "G": (G, c) input
    dt: torch.dtype
    cap: int        # the launcher's workgroups per CU: 32 (64 threads), 8 (256 threads), 2 (LARGE)
    stream: int     # the seed of synth.make_batch and of the failures, checked on the CPU: the oracle reports OK on every healthy problem

    @property
    def large(self):
        return self.cap == 2


CASES = {
    "g64_cfg1_J": Case(8, 2, 4, 16, "J", F64, 32, 101),
    "g64_cfg1_G": Case(8, 2, 4, 16, "G", F64, 32, 112),
    "g256_n44_J": Case(44, 6, 8, 48, "J", F64, 8, 103),
    "large_cfg3_J": Case(64, 8, 32, 128, "J", F64, 2, 104),
    "large_n67_J": Case(67, 9, 5, 70, "J", F64, 2, 105),
    "large_n67_G": Case(67, 9, 5, 70, "G", F64, 2, 106),
    "large_n67_J_f32": Case(67, 9, 5, 70, "J", F32, 2, 107),
}
KINDS = ("s_zero", "s_neg", "bad_index", "nan", "dup_row")
MODES = ("residual", "step", "iterate_c", "iterate_pc", "solve", "kkt_solve", "kkt_solve_T")   # (mo_linearize: its own cases below)


@functools.lru_cache(maxsize=None)
def case_host(name, cu):
    """(hb, hb_clean, kind, rhs): the host batch with its failures, the same batch without them, the failure kinds, a right-hand side."""
    cs = CASES[name]
    B = batch_for(cs.cap, cu)
    f32 = cs.dt == F32
    clean = host_batch(cs.n, cs.k, cs.m, cs.m_r, B, stream=cs.stream, f32=f32)
    hb = copy.deepcopy(clean)
    kind = draw_failures(B, KINDS, cs.stream)
    n = cs.n
    for p in np.flatnonzero(kind >= 0):
        kd = KINDS[kind[p]]
        if kd == "s_zero":
            hb.vars[p, n] = 0.0
        elif kd == "s_neg":
            hb.vars[p, n + 1] = -1.0
        elif kd == "bad_index":
            hb.cons_var[p, 0] = n + 3
        elif kd == "nan":
            hb.J[p, 0, 0] = np.nan
            hb.G[p, 0, 0] = np.nan
        else:
            hb.A_eq[p, :, 1] = hb.A_eq[p, :, 0]
    rhs = np.random.default_rng(cs.stream).normal(size=hb.vars.shape)
    if f32:
        rhs = rhs.astype(np.float32).astype(np.float64)
    return hb, clean, kind, rhs


def expected_status(kind, mode):
    """Per problem the set of status words the call may report, and the mask of healthy problems (exactly {OK})."""
    names = np.array(["healthy"] + list(KINDS))[kind + 1]
    table = {"healthy": {OK}, "s_zero": {SLACK}, "s_neg": {SLACK}, "bad_index": {BAD_INDEX}, "nan": {FACTOR, NONFINITE},
             "dup_row": {OK, FACTOR, NONFINITE}}
    if mode == "solve":   # the NAIVE initial guess replaces the caller's state: its slacks do not matter
        table = dict(table, s_zero={OK}, s_neg={OK})
    allowed = [table[nm] for nm in names]
    healthy = np.array([a == {OK} for a in allowed])
    failing = np.array([OK not in a for a in allowed])
    return allowed, healthy, failing


def upload(cs, hb, rhs):
    prob = device_problem(hb, cs.level, cs.dt)
    return prob, T(hb.vars, cs.dt), T(hb.mu, cs.dt), T(rhs, cs.dt)


def take(prob, idx):
    """The problems `idx` (device index tensor) of a BatchedQP as a batch of their own."""
    sel = lambda t: None if t is None else t.index_select(0, idx).contiguous()
    return Q.BatchedQP(n=prob.n, k=prob.k, m=prob.m, J=sel(prob.J), r=sel(prob.r), lam=prob.lam, G=sel(prob.G), c=sel(prob.c), A_eq=sel(prob.A_eq),
                       b_eq=sel(prob.b_eq), cons_var=sel(prob.cons_var), cons_a=sel(prob.cons_a), cons_b=sel(prob.cons_b))


class Runner:
    """One solver (= one plan) on one batch, every mode of the generic kernel on that plan.  The kernel name is asserted; every call goes to the
    C ABI with the argument list of its mirror in mini_opt_amd/qp.py and diff.py, because the mirrors allocate most outputs themselves (zeros
    or uninitialised): here EVERY output is pre-filled, floating point with NaN, integers with -1."""

    def __init__(self, prob, vars_d, mu_d, rhs_d):
        self.prob, self.vars, self.mu, self.rhs = prob, vars_d, mu_d, rhs_d
        self.B = int(vars_d.shape[0])
        self.s = Q.QPInteriorPointSolver(prob, batch=self.B, force_generic=True)
        assert self.s.step_kernel() == "generic" and self.s.solve_kernel() == "generic"

    def close(self):
        self.s._destroy()

    def run(self, mode, batch=None):
        """batch: launch only the first `batch` problems, on the plan of the whole batch."""
        lib, prob = L.lib(), self.prob
        B = self.B if batch is None else batch
        dt, V = prob.dtype, prob.V
        plan, ps, ptr, stream = self.s._plan, C.byref(self.s._prob), Q._ptr, Q._stream()
        vars_, mu, rhs = self.vars[:B].clone(), self.mu[:B], self.rhs[:B]
        new = lambda *shape: full(shape, dt)
        ints = lambda: full((B,), torch.int32, -1)
        status = ints()
        if mode == "residual":
            out = {"r": new(B, V), "kkt": new(B, L.MO_KKT_RECORD)}
            L.check(lib.mo_kkt_residual(plan, ps, B, ptr(vars_), V, ptr(mu), 1, 0, ptr(out["r"]), V, ptr(out["kkt"]), stream))
        elif mode == "step":
            out = {"delta": new(B, V), "alpha": new(B, 2), "status": status}
            L.check(lib.mo_newton_step(plan, ps, B, ptr(vars_), V, ptr(mu), 1, 0.995, 0, ptr(out["delta"]), V, ptr(out["alpha"]), ptr(status), stream))
        elif mode in ("iterate_c", "iterate_pc"):
            out = {"delta": new(B, V), "variables": vars_, "ip": new(B, L.MO_IP_RECORD), "status": status}
            L.check(lib.mo_iterate(plan, ps, B, ptr(vars_), V, ptr(mu), 1, Q.COMPLEMENTARITY if mode == "iterate_c" else Q.PREDICTOR_CORRECTOR,
                                   ptr(out["delta"]), V, ptr(out["ip"]), ptr(status), stream))
        elif mode == "solve":
            sp = Q.Params(**SOLVE_KW).as_struct()
            out = {"variables": vars_, "termination": ints(), "num_iterations": ints(), "iterations": new(B, SOLVE_KW["max_iterations"], L.MO_ITER_RECORD),
                   "lagrange": new(B, 2), "status": status}
            L.check(lib.mo_qp_solve(plan, ps, B, C.byref(sp), ptr(vars_), V, ptr(out["termination"]), ptr(out["num_iterations"]),
                                    ptr(out["iterations"]), ptr(out["lagrange"]), ptr(status), stream))
        else:
            # D.kkt_solve, on the plan D.kkt_solve itself would take (its cache is keyed without flags: the caller has set L.EXTRA_PLAN_FLAGS
            # to the force-generic flag and cleared the cache)
            assert D.kkt_solve_kernel(prob, B) == "generic"
            out = {"out": new(B, V), "status": status}
            pq = prob.as_struct()
            L.check(lib.mo_kkt_solve(D.plan_for(prob, B), C.byref(pq), B, ptr(vars_), V, ptr(rhs), V, L.MO_KKT_TRANSPOSE if mode == "kkt_solve_T" else 0,
                                     ptr(out["out"]), V, ptr(status), stream))
        torch.cuda.synchronize()
        return out


def modes_of(cs):
    return list(MODES)


def check_written(cs, mode, out, kind):
    """Assertion 1."""
    allowed, healthy, failing = expected_status(kind, mode)
    host = {name: t.double().cpu().numpy() if t.is_floating_point() else t.cpu().numpy() for name, t in out.items()}
    if mode == "residual":
        assert np.all(np.isfinite(host["r"][healthy])) and np.all(np.isfinite(host["kkt"][healthy]))
        return healthy, failing
    st = host["status"]
    assert not np.any(st == -1), f"{int(np.sum(st == -1))} status words were never written"
    wrong = [int(p) for p in range(len(st)) if int(st[p]) not in allowed[p]]
    assert not wrong, (mode, wrong[:8], [int(st[p]) for p in wrong[:8]], [int(kind[p]) for p in wrong[:8]])
    ok = st == OK
    main = "out" if mode.startswith("kkt_solve") else "variables" if mode == "solve" else "delta"
    assert np.all(np.isfinite(host[main][ok])), mode
    if mode != "solve":          # delta / out are NaN-filled for problems whose status is not OK
        assert np.all(np.isnan(host[main][~ok])), mode
    if mode == "step":
        assert np.all(np.isfinite(host["alpha"][ok])) and np.all(np.isnan(host["alpha"][~ok]))
    if mode.startswith("iterate"):
        assert np.all(np.isfinite(host["variables"][ok]))
        assert np.all(np.isfinite(host["ip"][ok][:, :3]))
    if mode == "solve":
        assert np.all(host["num_iterations"][ok] >= 1) and np.all(host["num_iterations"] >= 0)
        assert np.all(np.isin(host["termination"], (Q.SATISFIED_KKT_TOL, Q.MAX_ITERATIONS)))
        assert np.all(np.isfinite(host["lagrange"][ok]))
        first_record = host["iterations"][ok][:, 0]
        assert np.all(np.isfinite(first_record[:, :11]))                 # kkt_initial, kkt_final, mu, alpha.primal, alpha.dual
    return healthy, failing


def make_oracle_qp(hb, p):
    return orc.QP(G=np.tril(hb.G[p]), c=hb.c[p], A_eq=hb.A_eq[p].T if hb.k else None, b_eq=hb.b_eq[p] if hb.k else None,
                  cons_var=hb.cons_var[p], cons_a=hb.cons_a[p], cons_b=hb.cons_b[p])


def check_oracle(cs, mode, out, hb, rhs, healthy, tag):
    """Assertion 3."""
    f32 = cs.dt == F32
    if f32 and mode != "step":
        return
    host = {name: t.double().cpu().numpy() if t.is_floating_point() else t.cpu().numpy() for name, t in out.items()}
    n, k, m = cs.n, cs.k, cs.m
    if mode == "step":
        cost = dict(J=hb.J, r=hb.r, lam=hb.lam) if cs.level == "J" else dict(G=np.tril(hb.G).transpose(0, 2, 1).copy(), c=hb.c)
        ref, ref_alpha, ref_status, _ = orc.batched_newton_step(n, k, m, A_eq=hb.A_eq, b_eq=hb.b_eq, cons_var=np.clip(hb.cons_var, 0, n - 1),
                                                                cons_a=hb.cons_a, cons_b=hb.cons_b, vars_=hb.vars, mu=hb.mu, **cost)
        assert np.all(ref_status[healthy] == 0)
        err = rel_inf_rows(host["delta"][healthy], ref[healthy])
        print(f"{tag}: step vs oracle on {int(healthy.sum())} problems: max rel-inf {err.max():.3e}")
        assert err.max() < (TOL32 if f32 else TOL64), err.max()
        np.testing.assert_allclose(host["alpha"][healthy], ref_alpha[healthy], rtol=0, atol=5e-3 if f32 else 1e-9)
        return
    sample = oracle_sample(healthy, cs.stream + 1, SOLVE_SAMPLE if mode == "solve" else ORACLE_SAMPLE)
    if mode == "solve":
        agree = solves_agree_or_knife_edge(tag, lambda i: make_oracle_qp(hb, sample[i]), SOLVE_KW,
                                           {"generic": (host["termination"][sample], host["num_iterations"][sample])})
        assert agree.all(), (tag, sample[~agree])
        return
    for p in sample:
        o = oracle_solver(hb, p, hb.vars[p])
        if mode == "residual":
            o.evaluate_kkt(True)
            scale = max(1.0, np.abs(o.r).max())
            np.testing.assert_allclose(host["r"][p], o.r, rtol=0, atol=1e-11 * scale)
            e = o.compute_errors(float(hb.mu[p]))
            np.testing.assert_allclose(host["kkt"][p], [e.r_dual, e.r_comp, e.r_primal_eq, e.r_primal_ineq], rtol=1e-6, atol=1e-9)
        elif mode.startswith("iterate"):
            st, ip = o.iterate(float(hb.mu[p]), orc.COMPLEMENTARITY if mode == "iterate_c" else orc.PREDICTOR_CORRECTOR)
            assert st == 0
            assert np.max(np.abs(host["variables"][p] - o.variables)) / np.max(np.abs(o.variables)) < TOL64, (tag, p)
            exp = [ip.mu, ip.alpha_primal, ip.alpha_dual, ip.alpha_probe_primal, ip.alpha_probe_dual, ip.mu_affine]
            np.testing.assert_allclose(host["ip"][p], exp, rtol=1e-8, atol=1e-12, equal_nan=True)
        else:
            ref_d, ref_t = oracle_kkt_solves(o, n, k, m, rhs[p], rhs[p])
            ref = ref_t if mode == "kkt_solve_T" else ref_d
            assert np.max(np.abs(host["out"][p] - ref)) / np.max(np.abs(ref)) < TOL64, (tag, p)


def ip_skip(out):
    """The rows of `ip` that are not compared bit for bit: problems whose status is not OK (their record is undefined)."""
    return {"ip": (out["status"] != OK).cpu().numpy()} if "ip" in out else None


@pytest.fixture
def force_generic_kkt_plans(monkeypatch):
    """D.kkt_solve takes its plan from a cache keyed without flags: the force-generic flag goes in through L.EXTRA_PLAN_FLAGS, and the cache is
    emptied before and after."""
    D.clear_plan_cache()
    monkeypatch.setattr(L, "EXTRA_PLAN_FLAGS", L.EXTRA_PLAN_FLAGS | L.MO_PLAN_FORCE_GENERIC)
    yield
    D.clear_plan_cache()


def sub_runner(big, rows):
    """The problems `rows` of a Runner's batch on a solver and plans of their own."""
    idx = torch.as_tensor(rows, device="cuda:0")
    return Runner(take(big.prob, idx), *(t.index_select(0, idx).contiguous() for t in (big.vars, big.mu, big.rhs)))


CASE_MODES = [(name, mode) for name, cs in CASES.items() for mode in modes_of(cs)]


@pytest.mark.parametrize("name,mode", CASE_MODES, ids=[f"{name}-{mode}" for name, mode in CASE_MODES])
def test_generic_kernel_second_problem(name, mode, force_generic_kkt_plans):
    cs = CASES[name]
    cu = cus()
    hb, clean, kind, rhs = case_host(name, cu)
    B, first = hb.batch, cs.cap * cu
    assert B == batch_for(cs.cap, cu)
    tag = (name, mode)
    big = Runner(*upload(cs, hb, rhs))
    try:
        out = big.run(mode)
        healthy, failing = check_written(cs, mode, out, kind)                              # 1
        sample = pick_sample(B, first, healthy, failing, cs.stream)
        small = sub_runner(big, sample)                                                    # 2: a fresh solver, fresh plans
        try:
            ref = small.run(mode)
        finally:
            small.close()
        assert_same_bits(out, ref, rows=torch.as_tensor(sample, device="cuda:0"), skip_rows=ip_skip(ref), tag=tag)
        check_oracle(cs, mode, out, hb, rhs, healthy, tag)                                 # 3
        if cs.large:
            again = big.run(mode)                                                          # 4: the same plan, a second launch
            assert_same_bits(out, again, skip_rows=ip_skip(out), tag=tag + ("second launch",))
        if cs.large and mode == "step":                                                    # 5: a prefix on the plan of the whole batch
            pre = big.run(mode, batch=cu + 3)
            head = lambda o: {nm: t[:cu + 3] for nm, t in o.items()}
            assert_same_bits(head(out), head(pre), tag=tag + ("prefix",))
    finally:
        big.close()


@pytest.mark.parametrize("name", [name for name, cs in CASES.items() if cs.large])
def test_large_workspace_after_a_launch_with_failures(name, force_generic_kkt_plans):
    """4, second half: every mode is launched on the batch with its failures; then the failing problems are replaced by healthy data IN PLACE
    (same tensors, same solver, same plans: the workspace holds the half-factored matrices and NaNs of the launch before) and launched
    again.  The whole batch is healthy now, and the sampled problems whose data did not change give the bits of a batch of their own on
    fresh plans."""
    cs = CASES[name]
    cu = cus()
    hb, clean, kind, rhs = case_host(name, cu)
    B, first = hb.batch, cs.cap * cu
    big = Runner(*upload(cs, hb, rhs))
    try:
        for mode in modes_of(cs):
            big.run(mode)
        prob_c, vars_c, _, _ = upload(cs, clean, rhs)
        for fld in ("J", "r", "G", "c", "A_eq", "b_eq", "cons_var", "cons_a", "cons_b"):
            if getattr(big.prob, fld) is not None:
                getattr(big.prob, fld).copy_(getattr(prob_c, fld))
        big.vars.copy_(vars_c)
        keep = pick_sample(B, first, kind < 0, kind >= 0, cs.stream + 2)
        keep = keep[kind[keep] < 0]
        assert len(keep) >= 16
        small = sub_runner(big, keep)
        try:
            for mode in modes_of(cs):
                tag = (name, mode, "healed")
                healed = big.run(mode)
                if "status" in healed:
                    assert bool((healed["status"] == OK).all()), tag
                assert_same_bits(healed, small.run(mode), rows=torch.as_tensor(keep, device="cuda:0"), tag=tag)
        finally:
            small.close()
    finally:
        big.close()


# =====================================================================================================================================
# mo_linearize on the generic kernel.  Its system has k = m = 0, so the kernel it reaches follows from n alone: 64 threads up to n = 48
# (cap 32), 256 threads LDS-resident up to n = 71 (cap 8), LARGE -- G assembled in the workgroup's H_work slot, which load_qp does not
# zero, and read back from there -- from n = 72 on (cap 2).
# =====================================================================================================================================
LIN_CASES = {"lin64_n8": (8, 16, F64, 32, 151), "lin256_n67": (67, 70, F64, 8, 152), "lin256_n67_f32": (67, 70, F32, 8, 153),
             "large_n76": (76, 80, F64, 2, 154), "large_n76_f32": (76, 80, F32, 2, 155)}
LIN_LAM = float(np.float32(1e-3))


@functools.lru_cache(maxsize=None)
def lin_host(name, cu):
    n, m_r, dt, cap, seed = LIN_CASES[name]
    B = batch_for(cap, cu)
    rng = np.random.default_rng(seed)
    J = rng.uniform(-1, 1, (B, m_r, n)); r = rng.uniform(-1, 1, (B, m_r))
    if dt == F32:
        J, r = J.astype(np.float32).astype(np.float64), r.astype(np.float32).astype(np.float64)
    kind = draw_failures(B, ("nan",), seed)          # the one per-problem failure of a call without status: a NaN in J stays that problem's
    J[kind >= 0, 0, 0] = np.nan
    return dict(n=n, m_r=m_r, dt=dt, cap=cap, seed=seed, B=B, J=J, r=r, healthy=kind < 0)


def lin_run(plan, d, J_d, r_d):
    """Q.linearize(force_generic=True) with pre-filled outputs, on the caller's plan."""
    n, dt, B = d["n"], d["dt"], int(J_d.shape[0])
    out = {"G": full((B, n, n), dt), "c": full((B, n), dt), "half_sq": full((B,), dt)}
    ps = Q.BatchedQP(n=n, J=J_d, r=r_d, lam=LIN_LAM).as_struct()
    L.check(L.lib().mo_linearize(plan.h, C.byref(ps), B, Q._ptr(out["G"]), n * n, n, Q._ptr(out["c"]), n, Q._ptr(out["half_sq"]), Q._stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(LIN_CASES))
def test_linearize_kernel_second_problem(name):
    cu = cus()
    d = lin_host(name, cu)
    n, m_r, dt, B, healthy = d["n"], d["m_r"], d["dt"], d["B"], d["healthy"]
    f32 = dt == F32
    J_d, r_d = T(d["J"], dt), T(d["r"], dt)
    sample = pick_sample(B, d["cap"] * cu, healthy, ~healthy, d["seed"])
    idx = torch.as_tensor(sample, device="cuda:0")
    with Plan(n, 0, 0, m_r, dt, B, L.MO_PLAN_FORCE_GENERIC) as plan:
        out = lin_run(plan, d, J_d, r_d)
        host = {key: t.double().cpu().numpy() for key, t in out.items()}
        for key in host:                                                                                   # 1
            assert np.all(np.isfinite(host[key][healthy])), key
        with Plan(n, 0, 0, m_r, dt, len(sample), L.MO_PLAN_FORCE_GENERIC) as fresh:                        # 2
            assert_same_bits(out, lin_run(fresh, d, J_d.index_select(0, idx).contiguous(), r_d.index_select(0, idx).contiguous()), rows=idx, tag=name)
        Jh, rh = d["J"][healthy], d["r"][healthy]                                                          # 3: the whole batch
        got = host["G"][healthy].transpose(0, 2, 1)                          # column-major G -> [row, col]
        np.testing.assert_allclose(np.tril(got), np.tril(np.matmul(Jh.transpose(0, 2, 1), Jh) + LIN_LAM * np.eye(n)), rtol=1e-5 if f32 else 0,
                                   atol=1e-5 if f32 else 1e-11)
        assert np.all(np.triu(got, 1) == 0)                                  # strict upper exactly 0 (residual_test.cc:130-134)
        np.testing.assert_allclose(host["c"][healthy], np.einsum("bqi,bq->bi", Jh, rh), rtol=1e-4 if f32 else 1e-12, atol=1e-4 if f32 else 1e-12)
        np.testing.assert_allclose(host["half_sq"][healthy], 0.5 * np.sum(rh ** 2, axis=1), rtol=1e-5 if f32 else 1e-13)
        if d["cap"] == 2:                                                                                  # 4: the H_work slots outlive the launch
            assert_same_bits(out, lin_run(plan, d, J_d, r_d), tag=(name, "second launch"))
            lin_run(plan, d, J_d.flip(0).contiguous(), r_d.flip(0).contiguous())      # other problems, NaN ones too, in every slot
            assert_same_bits(out, lin_run(plan, d, J_d, r_d), tag=(name, "after other data"))
            clean = J_d.clone()
            clean[:, 0, 0] = torch.nan_to_num(clean[:, 0, 0], nan=0.25)               # the failing problems healed
            keep = torch.as_tensor(sample[healthy[sample]], device="cuda:0")
            healed = lin_run(plan, d, clean, r_d)
            assert bool(torch.isfinite(healed["G"]).all())
            assert_same_bits(out, {key: t.index_select(0, keep) for key, t in healed.items()}, rows=keep, tag=(name, "healed"))


# =====================================================================================================================================
# nullspace_kernel
# =====================================================================================================================================
NULL_CASES = {"n12_k3_G": (12, 3, 20, "G", 32, 201), "n50_k7_G": (50, 7, 60, "G", 8, 202), "n12_k3_J": (12, 3, 16, "J", 32, 203)}
NULL_KINDS = {"G": ("neg_G", "neg_diag", "nan", "zero_row"), "J": ("nan", "zero_row")}
NULL_LAM = 0.05


@functools.lru_cache(maxsize=None)
def nullspace_host(name, cu):
    n, k, m_r, level, cap, seed = NULL_CASES[name]
    B = batch_for(cap, cu)
    rng = np.random.default_rng(seed)
    J = rng.uniform(-1, 1, (B, m_r, n)); r = rng.uniform(-1, 1, (B, m_r))
    A = rng.uniform(-1, 1, (B, k, n)); b = rng.uniform(-1, 1, (B, k))
    kinds = NULL_KINDS[level]
    kind = draw_failures(B, kinds, seed)
    names = np.array(["healthy"] + list(kinds))[kind + 1]
    J[names == "nan", 0, 0] = np.nan
    G = np.einsum("bqi,bqj->bij", J, J) + (NULL_LAM if level == "J" else 0.0) * np.eye(n)
    c = np.einsum("bqi,bq->bi", J, r)
    G[names == "neg_G"] *= -1.0                      # negative definite
    G[names == "neg_diag", 0, 0] -= 1e3              # indefinite with a large negative direction
    for p in np.flatnonzero(names == "zero_row"):    # a zero equality row: rank k - 1, the pivot loop ends early; consistent, so still a success
        A[p, p % k, :] = 0.0; b[p, p % k] = 0.0
    c[names == "nan"] = 0.0                          # (J^T r of a J with a NaN; G-level input takes a finite c)
    healthy = (names == "healthy") | (names == "zero_row")
    return dict(n=n, k=k, m_r=m_r, level=level, cap=cap, seed=seed, B=B, J=J, r=r, G=G, c=c, A=A, b=b, healthy=healthy, failing=~healthy)


def nullspace_run(d, idx=None):
    sel = (lambda a: a) if idx is None else (lambda a: a[idx])
    A_d, b_d = T(sel(d["A"]).transpose(0, 2, 1)), T(sel(d["b"]))
    if d["level"] == "J":
        prob = Q.BatchedQP(n=d["n"], k=d["k"], J=T(sel(d["J"])), r=T(sel(d["r"])), lam=NULL_LAM, A_eq=A_d, b_eq=b_d)
    else:
        prob = Q.BatchedQP(n=d["n"], k=d["k"], G=T(np.tril(sel(d["G"])).transpose(0, 2, 1)), c=T(sel(d["c"])), A_eq=A_d, b_eq=b_d)
    B = int(A_d.shape[0])
    x, term = full((B, d["n"]), F64), full((B,), torch.int32, -1)
    with Plan(d["n"], d["k"], 0, prob.m_r, F64, B) as plan:          # QPNullSpaceSolver.Solve with pre-filled outputs
        ps = prob.as_struct()
        L.check(L.lib().mo_nullspace_solve(plan.h, C.byref(ps), B, Q._ptr(x), d["n"], Q._ptr(term), Q._stream()))
        torch.cuda.synchronize()
    return {"x": x, "termination": term}


@pytest.mark.parametrize("name", list(NULL_CASES))
def test_nullspace_kernel_second_problem(name):
    cu = cus()
    d = nullspace_host(name, cu)
    B, healthy, failing = d["B"], d["healthy"], d["failing"]
    out = nullspace_run(d)
    term, x = out["termination"].cpu().numpy(), out["x"].cpu().numpy()
    assert np.all(term[healthy] == Q.QPNullSpaceSolver.SUCCESS) and np.all(term[failing] == Q.QPNullSpaceSolver.NOT_POSITIVE_DEFINITE)   # 1
    assert np.all(np.isfinite(x[healthy])) and np.all(np.isnan(x[failing]))
    sample = pick_sample(B, d["cap"] * cu, healthy, failing, d["seed"])                                                                   # 2
    assert_same_bits(out, nullspace_run(d, sample), rows=torch.as_tensor(sample, device="cuda:0"), tag=name)
    res = np.einsum("bkn,bn->bk", d["A"][healthy], x[healthy]) + d["b"][healthy]                                                          # 3
    np.testing.assert_allclose(res, 0, atol=1e-11)
    for p in oracle_sample(healthy, d["seed"] + 1):
        ok, xr = N.null_space_solve(N.QPData(np.tril(d["G"][p]), d["c"][p], d["A"][p], d["b"][p], []))
        assert ok, p
        np.testing.assert_allclose(x[p], xr, rtol=1e-9, atol=1e-11)


# =====================================================================================================================================
# qp_eig_kernel: matrix in LDS, and (n = 150, as tests/test_gpu_eig.py) in the plan's H_work (cap 1: the grid is clamped to CUs slots)
# =====================================================================================================================================
EIG_CASES = {"n8_J_lds": (8, "J", 8, 301), "n17_G_lds": (17, "G", 8, 302), "n150_G_hwork": (150, "G", 1, 303)}


def eig_stats(w):
    return np.stack([w.min(axis=1), w.max(axis=1), np.abs(w).min(axis=1)], axis=1)


@functools.lru_cache(maxsize=None)
def eig_host(name, cu):
    n, level, cap, seed = EIG_CASES[name]
    B = batch_for(cap, cu)
    rng = np.random.default_rng(seed)
    if level == "J":
        J = rng.uniform(-1, 1, (B, 12, n)); r = rng.uniform(-1, 1, (B, 12))
        ref = eig_stats(np.linalg.eigvalsh(np.einsum("bri,brj->bij", J, J) + 1e-3 * np.eye(n)))
        return dict(n=n, B=B, cap=cap, seed=seed, J=J, r=r, ref=ref, scale=np.abs(ref).max(axis=1, keepdims=True))
    S = rng.uniform(-1, 1, (B, n, n)); S = S + S.transpose(0, 2, 1) + np.diag(rng.uniform(-2, 2, n))   # indefinite
    ref = eig_stats(np.linalg.eigvalsh(S))
    garbage = S.copy()                                   # tensor [b, col, row]: the strict upper triangle of G must not be read
    il = np.tril_indices(n, -1)
    garbage[:, il[0], il[1]] = 1e30
    return dict(n=n, B=B, cap=cap, seed=seed, G=garbage, ref=ref, scale=np.maximum(np.abs(ref).max(axis=1, keepdims=True), 1.0))


def eig_problem(d, idx=None):
    sel = (lambda a: a) if idx is None else (lambda a: a[idx])
    if "J" in d:
        return Q.BatchedQP(n=d["n"], J=T(sel(d["J"])), r=T(sel(d["r"])), lam=1e-3)
    G = T(sel(d["G"]))
    return Q.BatchedQP(n=d["n"], G=G, c=torch.zeros(G.shape[0], d["n"], dtype=F64, device="cuda:0"))


def eig_run(plan, prob):
    """Q.eigenvalue_stats with a pre-filled output, on the caller's plan."""
    B = int(prob._any().shape[0])
    out = full((B, 3), F64)
    ps = prob.as_struct()
    L.check(L.lib().mo_qp_eigenvalue_stats(plan.h, C.byref(ps), B, Q._ptr(out), Q._stream()))
    torch.cuda.synchronize()
    return {"eig": out}


@pytest.mark.parametrize("name", list(EIG_CASES))
def test_eig_kernel_second_problem(name):
    cu = cus()
    d = eig_host(name, cu)
    n, B = d["n"], d["B"]
    prob = eig_problem(d)
    nobody = np.zeros(B, dtype=bool)
    sample = pick_sample(B, d["cap"] * cu, ~nobody, nobody, d["seed"])
    idx = torch.as_tensor(sample, device="cuda:0")
    # Beyond the LDS only the vectors are LDS-resident, so the natural grid is 8 workgroups per CU there as well, each with a slot of H_work.
    # max_batch bounds the slots a plan allocates (include/mini_opt_hip.h) and launch_qp_eig clamps its grid to them: a plan made for
    # max_batch = CUs runs the batch on CUs workgroups, one slot each, at least three problems per slot.
    with Plan(n, 0, 0, prob.m_r, F64, cu if name.endswith("hwork") else B) as plan:
        out = eig_run(plan, prob)
        got = out["eig"].cpu().numpy()
        assert np.all(np.isfinite(got))                                                                     # 1
        err = np.max(np.abs(got - d["ref"]) / d["scale"])                                                   # 3
        assert err < 1e-10, err
        with Plan(n, 0, 0, prob.m_r, F64, len(sample)) as fresh:                                            # 2
            assert_same_bits(out, eig_run(fresh, eig_problem(d, sample)), rows=idx, tag=name)
        if name.endswith("hwork"):                                                                          # 4
            assert_same_bits(out, eig_run(plan, prob), tag=(name, "second launch"))
            eig_run(plan, eig_problem(d, np.arange(B)[::-1].copy()))      # other matrices in every slot
            assert_same_bits(out, eig_run(plan, prob), tag=(name, "after other data"))


# =====================================================================================================================================
# qp_grad_kernel (dense mo_qp_gradients)
# =====================================================================================================================================
GRAD_SHAPE = (8, 2, 5, 12)      # the shape of test_qp_gradients_strides_and_null_members


@functools.lru_cache(maxsize=None)
def grad_host(cu):
    n, k, m, m_r = GRAD_SHAPE
    B = batch_for(8, cu)
    hb = host_batch(n, k, m, m_r, B, stream=401)
    kind = draw_failures(B, ("bad_index",), 401)
    hb.cons_var[kind >= 0, 0] = n + 3
    u = np.random.default_rng(401).normal(size=hb.vars.shape)
    return hb, kind, u


def grad_run(hb, u, level, idx=None):
    """D.qp_gradients (every gradient of the input level) with pre-filled outputs, on a plan of its own."""
    n, k, m, m_r = GRAD_SHAPE
    if idx is not None:
        hb = type(hb)(n, k, m, m_r, hb.J[idx], hb.r[idx], hb.lam, hb.A_eq[idx], hb.b_eq[idx], hb.cons_var[idx], hb.cons_a[idx], hb.cons_b[idx],
                      hb.vars[idx], hb.mu[idx])
        hb.G = np.einsum("bqi,bqj->bij", hb.J, hb.J) + hb.lam * np.eye(n)
        hb.c = np.einsum("bqi,bq->bi", hb.J, hb.r)
        u = u[idx]
    prob = device_problem(hb, level)
    B, V = hb.batch, hb.vars.shape[1]
    out = {"A_eq": full((B, n, k), F64), "b_eq": full((B, k), F64), "cons_a": full((B, m), F64), "cons_b": full((B, m), F64)}
    g = L.QPGrads()
    g.dA_eq, g.dA_stride, g.dA_ld = Q._ptr(out["A_eq"]), n * k, k
    g.db_eq, g.db_stride = Q._ptr(out["b_eq"]), k
    g.dcons_a, g.dcons_b, g.dcons_stride = Q._ptr(out["cons_a"]), Q._ptr(out["cons_b"]), m
    if level == "G":
        out.update(G=full((B, n, n), F64), c=full((B, n), F64))
        g.dG, g.dG_stride, g.dG_ld = Q._ptr(out["G"]), n * n, n
        g.dc, g.dc_stride = Q._ptr(out["c"]), n
    else:
        out.update(J=full((B, m_r, n), F64), r=full((B, m_r), F64), lam=full((B,), F64))
        g.dJ, g.dJ_stride, g.dJ_ld, g.dJ_layout = Q._ptr(out["J"]), m_r * n, n, L.MO_ROW_MAJOR
        g.dr, g.dr_stride = Q._ptr(out["r"]), m_r
        g.dlambda, g.dlambda_stride = Q._ptr(out["lam"]), 1
    v_d, u_d = T(hb.vars), T(u)
    with Plan(n, k, m, m_r, F64, B) as plan:
        ps = prob.as_struct()
        L.check(L.lib().mo_qp_gradients(plan.h, C.byref(ps), B, Q._ptr(v_d), V, Q._ptr(u_d), V, C.byref(g), Q._stream()))
        torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("level", ["J", "G"])
def test_qp_grad_kernel_second_problem(level):
    n, k, m, m_r = GRAD_SHAPE
    cu = cus()
    hb, kind, u = grad_host(cu)
    B = hb.batch
    out = grad_run(hb, u, level)
    host = {key: t.cpu().numpy().reshape(B, -1) for key, t in out.items()}
    failing = kind >= 0
    # 1: the one documented per-problem outcome is dcons_a = NaN at a constraint whose variable is outside [0, n); all else is finite
    assert np.all(np.isnan(host["cons_a"][failing, 0])) and np.all(np.isfinite(host["cons_a"][~failing]))
    assert np.all(np.isfinite(host["cons_a"][:, 1:]))
    for key in host:
        if key != "cons_a":
            assert np.all(np.isfinite(host[key])), key
    sample = pick_sample(B, 8 * cu, ~failing, failing, 401)                                                  # 2
    assert_same_bits(out, grad_run(hb, u, level, sample), rows=torch.as_tensor(sample, device="cuda:0"), tag=level)
    var = np.clip(hb.cons_var, 0, n - 1)                                                                     # 3: the whole batch
    worst = 0.0
    for p in range(B):
        ref = R.gradients(n, k, m, var[p], hb.vars[p], u[p], J=hb.J[p] if level == "J" else None, r=hb.r[p] if level == "J" else None)
        for key in host:
            want = np.atleast_1d(ref[key]).reshape(-1)
            got = host[key][p]
            if key == "A_eq":
                got = got.reshape(n, k).T.reshape(-1)                # [n, k] memory = k x n column-major
            if key == "cons_a" and failing[p]:
                got, want = got[1:], want[1:]
            worst = max(worst, np.max(np.abs(got - want)) / np.max(np.abs(want)))
    assert worst < TOL64, worst


# =====================================================================================================================================
# blocks_linearize_kernel, blocks_jacobian, blocks_eq_grad: the n = 8 layout of test_blocks_grad_workgroups_loop_over_problems
# =====================================================================================================================================
BLOCKS_N = 8


@functools.lru_cache(maxsize=None)
def blocks_host(cu):
    B = batch_for(8, cu)
    blocks = random_layout(np.random.default_rng(330), BLOCKS_N, count=6, repeats=True)
    rng = np.random.default_rng(501)
    Js, rs = draw_blocks(rng, blocks, B, False)
    rows = sum(R_ for _, R_ in blocks)
    V = BLOCKS_N + rows                                   # the state of the equality gradients: k = rows, m = 0
    return dict(B=B, blocks=blocks, Js=Js, rs=rs, rows=rows, v=rng.normal(size=(B, V)), u=rng.normal(size=(B, V)))


def blocks_run(d, which, idx=None):
    """Q.linearize_blocks / Q.jacobian_blocks / D.qp_gradients_eq_blocks with pre-filled outputs."""
    sel = (lambda a: a) if idx is None else (lambda a: a[idx])
    n, blocks = BLOCKS_N, d["blocks"]
    lay = Q.ResidualLayout(n, blocks)
    Jp, r = T(pack_np([sel(J) for J in d["Js"]])), T(np.concatenate([sel(r_) for r_ in d["rs"]], 1))
    B = int(Jp.shape[0])
    lib = L.lib()
    if which == "linearize":
        out = {"G": full((B, n, n), F64), "c": full((B, n), F64), "half_sq": full((B,), F64)}
        L.check(lib.mo_linearize_blocks(lay._plan, lay.h, Q._ptr(Jp), lay.values, Q._ptr(r), lay.rows, 0.37, None, 0, B, Q._ptr(out["G"]), n * n, n,
                                        Q._ptr(out["c"]), n, Q._ptr(out["half_sq"]), Q._stream()))
    elif which == "jacobian":
        out = {"J": full((B, n, lay.rows), F64), "l1": full((B,), F64)}
        L.check(lib.mo_jacobian_blocks(lay._plan, lay.h, Q._ptr(Jp), lay.values, Q._ptr(r), lay.rows, B, Q._ptr(out["J"]), lay.rows * n, lay.rows,
                                       L.MO_COL_MAJOR, Q._ptr(out["l1"]), Q._stream()))
    else:
        V = n + lay.rows
        v_d, u_d = T(sel(d["v"])), T(sel(d["u"]))
        out = {"J_eq_blocks": full((B, lay.values), F64), "r_eq": full((B, lay.rows), F64)}
        with Plan(n, lay.rows, 0, 0, F64, B) as plan:
            L.check(lib.mo_qp_gradients_eq_blocks(plan.h, lay.h, B, Q._ptr(v_d), V, Q._ptr(u_d), V, Q._ptr(out["J_eq_blocks"]), lay.values,
                                                  Q._ptr(out["r_eq"]), lay.rows, Q._stream()))
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("which", ["linearize", "jacobian", "eq_grad"])
def test_block_kernels_second_problem(which):
    cu = cus()
    d = blocks_host(cu)
    B, blocks, n, rows = d["B"], d["blocks"], BLOCKS_N, d["rows"]
    out = blocks_run(d, which)
    host = {key: t.cpu().numpy() for key, t in out.items()}
    for key in host:
        assert np.all(np.isfinite(host[key])), key                                                           # 1
    nobody = np.zeros(B, dtype=bool)
    sample = pick_sample(B, 8 * cu, ~nobody, nobody, 501)                                                    # 2
    assert_same_bits(out, blocks_run(d, which, sample), rows=torch.as_tensor(sample, device="cuda:0"), tag=which)
    un = UNIT[F64]                                                                                           # 3: the bounds of the kernels' own tests
    R_max = max(R_ for _, R_ in blocks)
    lam = 0.37
    for p in oracle_sample(~nobody, 502):
        if which == "linearize":
            H_ref, b_ref, f_ref = oracle_hessian(n, blocks, d["Js"], d["rs"], p)
            S, Sc, Lh, Lc = bound_terms(n, blocks, d["Js"], d["rs"], p)
            Hd = host["G"][p].T
            assert np.all(np.abs(Hd - (H_ref + lam * np.eye(n))) <= 2 * (R_max + Lh) * un * S + (un * lam) * np.eye(n)), p
            assert np.all(np.abs(host["c"][p] - b_ref) <= 2 * (R_max + Lc) * un * Sc), p
            assert np.all(np.triu(Hd, 1) == 0) and np.all(Hd[(Lh == 0) & ~np.eye(n, dtype=bool)] == 0) and np.all(host["c"][p][Lc == 0] == 0)
            assert abs(host["half_sq"][p] - f_ref) <= 4 * (rows + 2) * un * abs(f_ref) + 1e-300
        elif which == "jacobian":
            ref, bref = oracle_jacobian(n, blocks, d["Js"], d["rs"], p, rows)
            assert np.array_equal(host["J"][p].T, ref), p
            np.testing.assert_allclose(host["l1"][p], np.abs(bref).sum(), rtol=1e-14)
        else:
            x, y, ux, uy = d["v"][p, :n], d["v"][p, n:], d["u"][p, :n], d["u"][p, n:]
            dJ, dr_eq = BR.gradients_eq_blocks(blocks, x, ux, y, uy)
            aJ, _ = BR.gradients_eq_blocks(blocks, x, ux, y, uy, absolute=True)
            assert np.all(np.abs(host["J_eq_blocks"][p] - BR.pack(dJ)) <= 4 * un * BR.pack(aJ)), p
            assert np.array_equal(host["r_eq"][p], dr_eq), p
