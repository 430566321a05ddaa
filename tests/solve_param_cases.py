"""Every Solve kernel against every Solve parameter (test infrastructure, not product code): the cases, the parameter cells and the oracle
referee of tests/test_solve_params_oracle_cpu.py, tests/test_gpu_solve_params.py and the Solve rows of tests/test_layout_dispatch_cpu.py.
Plain numpy; nothing here touches the device.

QPInteriorPointSolver::Solve (qp.cc:100-151: initial guess, initial mu, barrier strategy, termination test, mu update) is written out once per
kernel -- kkt_fused.hip (one template behind the one-y-tile, lean two-slot, ny2, ny3/4, mc4, flat and gather instantiations), kkt_fused_f32.hip,
kkt_fused_tiny.hip, kkt_generic.hip (LDS-resident and LARGE) -- so every one of them runs the whole parameter product here:

  cases   the first input level of every row of tests/layout_cases.py (the smallest shape per Solve instantiation) + k = 0 and m = 0 on the
          one-y-tile 32 grid and on the one-tile kernel
  cells   initial_guess_method {NAIVE, SOLVE_EQUALITY_CONSTRAINED, USER_PROVIDED} x barrier_strategy {COMPLEMENTARITY, FIXED_DECREASE,
          PREDICTOR_CORRECTOR} x initialize_mu_with_complementarity {0, 1}, with initial_mu = 0.05 and sigma = 0.3 (neither 1.0, where
          s.z / M = 1 of the NAIVE / SOLVE_EQUALITY_CONSTRAINED start hides the flag, nor the 0.1 of every other device test)
  runs    short: max_iterations = 3, a termination_kkt_tol nothing reaches (every problem ends MAX_ITERATIONS, 3; m = 0 included, which
                 solves its equality-constrained QP in one step);  full: termination_kkt_tol = 1e-8, max_iterations = 20
  + one cell per case where termination_complementarity_tol alone keeps the loop going (COMP_CELL)

fp32 cases: the fp64 oracle on fp32-rounded inputs.  fp32 arithmetic cannot bring a KKT residual of terms of O(10) below ~1e-5, so their
full run and their complementarity cell use the tolerances of a fp32 Solve (FULL_F32, COMP_F32: the 2e-3 / 1e-3 of
test_gpu_parity.py::test_fused_f32_solve_iterate_residual), and a decision of the oracle counts as clear for them only if its margin is above
1e-3 as well (the same test's rule), not just above the fp64 threshold of its kind."""
import collections
import functools

import numpy as np

from tests import layout_cases as LC

B = 6
NAIVE, SOLVE_EQUALITY_CONSTRAINED, USER_PROVIDED = 0, 1, 2
COMPLEMENTARITY, FIXED_DECREASE, PREDICTOR_CORRECTOR = 0, 1, 2
SATISFIED_KKT_TOL, MAX_ITERATIONS = 0, 1
GUESSES = (NAIVE, SOLVE_EQUALITY_CONSTRAINED, USER_PROVIDED)
STRATEGIES = (COMPLEMENTARITY, FIXED_DECREASE, PREDICTOR_CORRECTOR)
GUESS_NAME = {NAIVE: "naive", SOLVE_EQUALITY_CONSTRAINED: "eq", USER_PROVIDED: "user"}
STRATEGY_NAME = {COMPLEMENTARITY: "comp", FIXED_DECREASE: "fixed", PREDICTOR_CORRECTOR: "pc"}

Cell = collections.namedtuple("Cell", "guess strategy mu_from_state")
CELLS = [Cell(g, s, f) for g in GUESSES for s in STRATEGIES for f in (0, 1)]
COMP_CELL = "complementarity-decides"          # the key of the extra cell in referee()
INITIAL_MU, SIGMA = 0.05, 0.3
SHORT = dict(max_iterations=3, termination_kkt_tol=1e-30)
FULL = dict(max_iterations=20, termination_kkt_tol=1e-8)
FULL_F32 = dict(max_iterations=20, termination_kkt_tol=2e-3, termination_complementarity_tol=1e-3)
# kmax < termination_kkt_tol from an early iteration on, while FIXED_DECREASE still walks mu = 0.05 x 0.3^i down to the complementarity tolerance
COMP = dict(max_iterations=20, termination_kkt_tol=1e-3, termination_complementarity_tol=1e-10)
COMP_F32 = dict(max_iterations=20, termination_kkt_tol=2e-2, termination_complementarity_tol=1e-5)
F32_CLEAR = 1e-3                               # the margin a decision needs before fp32 rounding cannot flip it


def cell_id(cell):
    return cell if cell == COMP_CELL else "%s-%s-%s" % (GUESS_NAME[cell.guess], STRATEGY_NAME[cell.strategy], "mu_state" if cell.mu_from_state else "mu_init")


# ---- the case table ----------------------------------------------------------------------------------------------------------------------
# The rows of tests/layout_cases.py at their first input level, and four rows of the same form for k = 0 and m = 0.
EXTRA = [
    LC._case("n32-k0",  "f64", "J", (20, 0, 10, 26), (LC.FUSED_STEP, 2, 4, 0, 1, LC.JMODE_VECTOR, 1, 1, 0, 0), "main"),
    LC._case("n32-m0",  "f64", "J", (20, 3, 0, 26),  (LC.FUSED_STEP, 2, 4, 0, 1, LC.JMODE_VECTOR, 1, 1, 0, 0), "main"),
    LC._case("tiny-k0", "f64", "J", (8, 0, 4, 16),   (LC.FUSED_TINY, 1, 3, 0, 1, LC.JMODE_VECTOR, 1, 1, 0, 0), "tiny"),
    LC._case("tiny-m0", "f64", "J", (8, 2, 0, 16),   (LC.FUSED_TINY, 1, 3, 0, 1, LC.JMODE_VECTOR, 1, 1, 0, 0), "tiny"),
]
CASES = list(LC.CASES) + EXTRA
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]


def level_of(case):
    return case.levels[0]


# What mo_plan_solve_kernel must report, and the FusedKey of MODE_SOLVE (None: the generic kernel): family, tile grid nt, QP-level input,
# constraint slots mc, J stream, y tiles, lean (an instantiation without the predictor-corrector's second solve exists: pck = 0 unless the
# strategy is PREDICTOR_CORRECTOR), fp32, pad.  Written out by hand from the shapes, not derived from the selector.
SolveKey = collections.namedtuple("SolveKey", "family nt qpl mc jmode ny lean f32 pad")
_V, _F, _G = LC.JMODE_VECTOR, LC.JMODE_FLAT, LC.JMODE_GATHER
_S, _T = LC.FUSED_SOLVE, LC.FUSED_TINY
EXPECTED = {
    #  id          kernel name                      family nt qpl mc jmode ny lean f32 pad
    "tiny":      ("fused_solve_tiny_f64",       SolveKey(_T, 1, 0, 1, _V, 1, 0, 0, 0)),
    "tiny-k0":   ("fused_solve_tiny_f64",       SolveKey(_T, 1, 0, 1, _V, 1, 0, 0, 0)),
    "tiny-m0":   ("fused_solve_tiny_f64",       SolveKey(_T, 1, 0, 1, _V, 1, 0, 0, 0)),
    "n32":       ("fused_solve_mfma_f64_n32",   SolveKey(_S, 2, 0, 1, _V, 1, 0, 0, 0)),
    "n32-k0":    ("fused_solve_mfma_f64_n32",   SolveKey(_S, 2, 0, 1, _V, 1, 0, 0, 0)),
    "n32-m0":    ("fused_solve_mfma_f64_n32",   SolveKey(_S, 2, 0, 1, _V, 1, 0, 0, 0)),
    "flat":      ("fused_solve_mfma_f64_n32",   SolveKey(_S, 2, 0, 1, _F, 1, 0, 0, 0)),
    "gather":    ("fused_solve_mfma_f64_n32",   SolveKey(_S, 2, 0, 1, _G, 1, 0, 0, 0)),
    "diag4":     ("fused_solve_mfma_f64_n64",   SolveKey(_S, 4, 0, 1, _V, 1, 0, 0, 0)),
    "diag4pad":  ("fused_solve_mfma_f64_n64",   SolveKey(_S, 4, 0, 1, _V, 1, 0, 0, 0)),
    "ny2":       ("fused_solve_mfma_f64_n32",   SolveKey(_S, 2, 0, 2, _V, 2, 1, 0, 0)),
    "mc2":       ("fused_solve_mfma_f64_n64",   SolveKey(_S, 4, 0, 2, _V, 1, 1, 0, 0)),
    "mc4":       ("fused_solve_qp_f64_n32",     SolveKey(_S, 2, 1, 4, _V, 1, 0, 0, 0)),
    "ny3":       ("fused_solve_mfma_f64_n64",   SolveKey(_S, 4, 0, 2, _V, 3, 0, 0, 0)),
    "ny4":       ("fused_solve_mfma_f64_n64",   SolveKey(_S, 4, 0, 2, _V, 4, 0, 0, 0)),
    "n96":       ("fused_solve_mfma_f64_n96",   SolveKey(_S, 6, 0, 1, _V, 1, 0, 0, 0)),
    "n128":      ("fused_solve_mfma_f64_n128",  SolveKey(_S, 8, 0, 1, _V, 1, 0, 0, 0)),
    "f32-64":    ("fused_solve_mfma_f32_n64",   SolveKey(_S, 4, 0, 1, _V, 1, 0, 1, 0)),
    "f32-pad":   ("fused_solve_mfma_f32_n64",   SolveKey(_S, 4, 0, 1, _V, 1, 0, 1, 1)),
    "f32-128":   ("fused_solve_mfma_f32_n128",  SolveKey(_S, 8, 0, 1, _V, 1, 0, 1, 1)),
    "gen-f64":   ("generic", None),
    "gen-f32":   ("generic", None),
    "gen-large": ("generic", None),
}
assert set(EXPECTED) == set(IDS)


def kernel_name(case_id):
    return EXPECTED[case_id][0]


# ---- problems ------------------------------------------------------------------------------------------------------------------------------
SEED = 9100
# Seeds chosen so that the conditions of tests/test_solve_params_oracle_cpu.py hold (the first of SEED + index + 100 j, j = 0, 1, ..., that
# keeps the early decisions of the short runs off a knife edge); every other case draws from SEED + its index.
SEED_OF = {"diag4pad": 9205, "f32-64": 12913, "f32-pad": 9514, "f32-128": 9215, "gen-f32": 9217}
# cons_b ~ U(lo, hi): (0.5, 2) unless named here.  ny3 / ny4 leave x only n - k = 7 / 8 free directions; behind the wide boxes the
# PREDICTOR_CORRECTOR of the NAIVE start lands on z + dz = 0 (margins of 0 to 1e-9) at iteration 1 on ny4 with every one of 40 seeds tried, the
# kind of tie SOLVE_EQUALITY_CONSTRAINED starts on when no inequality is active.  With the tighter boxes iterations 0 and 1 are clear.
B_RANGE_OF = {"ny3": (0.1, 1.0), "ny4": (0.1, 1.0)}


@functools.lru_cache(maxsize=None)
def problems(case_id):
    """The B problems of a case as float64 numpy arrays (fp32 cases rounded through float32).  Every inequality holds strictly at x = 0
    (a = +-1, +-2, b in [0.5, 2] or B_RANGE_OF) and b_eq = -A x0 for |x0| <= 0.02, so the NAIVE start (x = 0) is strictly inside with slacks of O(1), far
    from the 1e-9 slack floor, and the equalities are consistent with a point near it.  The user state is drawn as in
    tests/test_gpu_parity.py::_fused_vs_generic_case.  G, A in the memory order of the C ABI ([b, col, row]); lambda 0.5 where J has fewer
    rows than variables, else 1e-3."""
    case = BY_ID[case_id]
    n, k, m, m_r = case.shape
    mr = m_r if level_of(case) == "J" else 2 * n                # (G, c) input: G from a J of its own
    rng = np.random.default_rng(SEED_OF.get(case_id, SEED + IDS.index(case_id)))
    f = (lambda a: a.astype(np.float32).astype(np.float64)) if case.dtype == "f32" else (lambda a: a)
    J = f(rng.uniform(-1, 1, (B, mr, n))); r = f(rng.uniform(-1, 1, (B, mr)))
    A = f(rng.uniform(-1, 1, (B, n, k)))
    x0 = rng.uniform(-0.02, 0.02, (B, n))
    b = f(-np.einsum("bik,bi->bk", A, x0))
    cv = rng.integers(0, n, (B, m)).astype(np.int32); ca = rng.choice([-2.0, -1.0, 1.0, 2.0], (B, m)); cb = f(rng.uniform(*B_RANGE_OF.get(case_id, (0.5, 2.0)), (B, m)))
    x = rng.uniform(-0.1, 0.1, (B, n)); sl = rng.uniform(0.2, 1.5, (B, m)); z = rng.uniform(0.1, 2, (B, m)); y = rng.uniform(-1, 1, (B, k))
    vars_ = f(np.concatenate([x, sl, y, z], axis=1))
    lam = float(f(np.array(0.5 if mr < n else 1e-3)))
    G = np.einsum("bqi,bqj->bij", J, J) + lam * np.eye(n)       # symmetric: [b, col, row] is its column-major memory
    c = np.einsum("bqi,bq->bi", J, r)
    if level_of(case) == "G":
        G, c = f(G), f(c)
    d = dict(J=J, r=r, A=A, b=b, cv=cv, ca=ca, cb=cb, vars=vars_, lam=lam, G=G, c=c)
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def params(case_id, cell, kind):
    """The Solve parameters (names of QPInteriorPointSolver::Params) of one cell in run `kind` (short / full; the COMP_CELL has one run)."""
    f32 = BY_ID[case_id].dtype == "f32"
    if cell == COMP_CELL:
        return dict(initial_mu=INITIAL_MU, sigma=SIGMA, barrier_strategy=FIXED_DECREASE, initial_guess_method=NAIVE,
                    initialize_mu_with_complementarity=0, **(COMP_F32 if f32 else COMP))
    run = SHORT if kind == "short" else FULL_F32 if f32 else FULL
    return dict(initial_mu=INITIAL_MU, sigma=SIGMA, barrier_strategy=cell.strategy, initial_guess_method=cell.guess,
                initialize_mu_with_complementarity=cell.mu_from_state, **run)


# ---- the referee -----------------------------------------------------------------------------------------------------------------------------
# One Solve of the oracle: termination state, iteration count, final variables, the decision margins of oracle/margins.py, the
# QPInteriorPointIteration records [iterations, 14] (kkt_initial[4], kkt_final[4], ip[6]).
Ref = collections.namedtuple("Ref", "term nit vars margins records")


def _record(kkt_initial, kkt_final, ip):
    return [kkt_initial.r_dual, kkt_initial.r_comp, kkt_initial.r_primal_eq, kkt_initial.r_primal_ineq,
            kkt_final.r_dual, kkt_final.r_comp, kkt_final.r_primal_eq, kkt_final.r_primal_ineq,
            ip.mu, ip.alpha_primal, ip.alpha_dual, ip.alpha_probe_primal, ip.alpha_probe_dual, ip.mu_affine]


def oracle_qp(case_id, p):
    from oracle import oracle as orc
    d = problems(case_id)
    k = BY_ID[case_id].shape[1]
    return orc.QP(G=np.tril(d["G"][p]), c=d["c"][p], A_eq=d["A"][p].T if k else None, b_eq=d["b"][p] if k else None,
                  cons_var=d["cv"][p], cons_a=d["ca"][p], cons_b=d["cb"][p])


def solve_once(case_id, p, kw):
    """The oracle's Solve of problem p from the case's user state, replayed with its margins and records."""
    from oracle import margins as M
    records = []
    term, nit, v, marg = M.solve_with_margins(oracle_qp(case_id, p), vars0=problems(case_id)["vars"][p], records=records, **kw)
    assert len(records) == nit
    return Ref(term, nit, v, marg, np.array([_record(*r) for r in records]).reshape(-1, 14))


def oracle_records(case_id, p, kw):
    """[iterations, 14] of orc_solve itself (oracle/kkt_oracle.c), which solve_once's replay must reproduce."""
    from oracle import oracle as orc
    o = orc.Solver(oracle_qp(case_id, p))
    o.variables[:] = problems(case_id)["vars"][p]
    term, its = o.solve(**kw)
    return term, np.array([_record(i.kkt_initial, i.kkt_final, i.ip) for i in its]).reshape(-1, 14)


@functools.lru_cache(maxsize=None)
def referee(case_id, kind):
    """{cell: [Ref of problem 0 .. B-1]} for run `kind` of a case; the full run carries the COMP_CELL as well."""
    cells = CELLS + ([COMP_CELL] if kind == "full" else [])
    return {cell: [solve_once(case_id, p, params(case_id, cell, kind)) for p in range(B)] for cell in cells}


def ratio(case_id, margin):
    """margin / threshold of one logged decision (below 1: a knife edge).  fp32 cases: the threshold is at least F32_CLEAR."""
    thr = margin[3]
    if BY_ID[case_id].dtype == "f32":
        thr = max(thr, F32_CLEAR)
    return margin[2] / thr


def first_edge(case_id, margins):
    """The iteration of the first knife-edge decision of a run (the slack floor of the initial guess counts as iteration 0), None if every
    decision was clear.  The device must follow the oracle's records on the iterations before it."""
    its = [max(m[0], 0) for m in margins if ratio(case_id, m) < 1.0]
    return min(its) if its else None


def clear_prefix_demanded(case_id, cell):
    """How many leading iterations of a short run the oracle must decide clear of every threshold, on every problem (what
    tests/test_solve_params_oracle_cpu.py asserts, so that the clear prefix the GPU test checks in full is never empty there):
    NAIVE / USER_PROVIDED: all three under COMPLEMENTARITY / FIXED_DECREASE, the first two under PREDICTOR_CORRECTOR (whose corrector aims
    at s z = sigma mu with sigma = (mu_affine / mu)^3, so z + dz comes close to 0 by construction as the run proceeds).
    SOLVE_EQUALITY_CONSTRAINED: none (with PREDICTOR_CORRECTOR it starts on a tie: z + dz = 0 exactly on inactive constraints, active ones
    clamped onto the slack floor).  fp32 x PREDICTOR_CORRECTOR: none per problem -- at the 1e-3 a fp32 decision needs, the corrector's
    z + dz is an edge from iteration 0 or 1 on; half the runs of a case must still have iteration 0 clear."""
    if cell.guess == SOLVE_EQUALITY_CONSTRAINED:
        return 0
    if cell.strategy != PREDICTOR_CORRECTOR:
        return 3
    return 0 if BY_ID[case_id].dtype == "f32" else 2


def edge_margins(case_id, margins):
    """The margins as oracle.margins.Disagreements takes them, with the threshold of the case's precision."""
    if BY_ID[case_id].dtype != "f32":
        return margins
    return [(m[0], m[1], m[2], max(m[3], F32_CLEAR)) for m in margins]


def undecided_iterations(ref, kw):
    """Iterations of a run that end with kmax(kkt_final) < termination_kkt_tol and do not end the run: the loop went on, so ComputeMu() >=
    termination_complementarity_tol there -- the second operand of the termination test alone kept it going.  (The iteration that ends a
    SATISFIED_KKT_TOL run is not one of them.)"""
    kmax = ref.records[:, 4:8].max(axis=1)
    last = ref.nit - 1 if ref.term == SATISFIED_KKT_TOL else ref.nit
    return int(np.sum(kmax[:last] < kw["termination_kkt_tol"]))
