"""Conditions on the inputs of tests/test_gpu_solve_params.py, from the oracle alone (no GPU).  The GPU test follows the oracle's records only up
to a problem's first knife-edge decision and accepts a different termination only on a knife edge; these are the caps that stop that rule
from excusing everything: every parameter of a cell changes what the oracle computes, and the clear prefix is long where it is demanded
(tests/solve_param_cases.py::clear_prefix_demanded).  Seeds and constraint margins were chosen so that they hold; they are asserted here."""
import numpy as np
import pytest

from tests import solve_param_cases as SP


@pytest.mark.parametrize("cid", SP.IDS)
def test_short_runs(cid):
    """Every short run ends (MAX_ITERATIONS, 3); the mu flag and the guess each change iteration 0; the demanded prefix is clear."""
    short = SP.referee(cid, "short")
    n, k, m, m_r = SP.BY_ID[cid].shape
    pc_first = []
    for cell, refs in short.items():
        need = SP.clear_prefix_demanded(cid, cell)
        for p, ref in enumerate(refs):
            assert (ref.term, ref.nit) == (SP.MAX_ITERATIONS, 3), (cid, SP.cell_id(cell), p, ref.term, ref.nit)
            edge = SP.first_edge(cid, ref.margins)
            assert edge is None or edge >= need, (cid, SP.cell_id(cell), p, "knife edge at iteration", edge, "clear prefix demanded", need)
            if cell.strategy == SP.PREDICTOR_CORRECTOR and cell.guess != SP.SOLVE_EQUALITY_CONSTRAINED:
                pc_first.append(edge is None or edge > 0)
    assert 2 * sum(pc_first) >= len(pc_first), (cid, "iteration 0 clear in", sum(pc_first), "of", len(pc_first), "NAIVE / USER_PROVIDED predictor-corrector runs")
    for s in SP.STRATEGIES:
        # the flag bites: mu of iteration 0 (ip.mu; under PREDICTOR_CORRECTOR, whose ip.mu is the corrector's, |s o z - mu| of kkt_initial)
        q = 1 if s == SP.PREDICTOR_CORRECTOR else 8
        for g in SP.GUESSES:
            for p in range(SP.B):
                on, off = short[SP.Cell(g, s, 1)][p].records[0], short[SP.Cell(g, s, 0)][p].records[0]
                if m:
                    assert abs(on[q] - off[q]) > 0.01 * abs(off[q]), (cid, g, s, p, on[q], off[q])
                else:   # no inequalities: the reference's ComputeMu() is 0 (qp.cc:509-516) and mu is never used
                    assert on[8] == 0.0 and off[8] == SP.INITIAL_MU, (cid, g, s, p, on[8], off[8])
                    np.testing.assert_array_equal(on[:8], off[:8])
        # the guess bites: pairwise different kkt_initial at iteration 0
        for flag in (0, 1):
            for p in range(SP.B):
                ki = [short[SP.Cell(g, s, flag)][p].records[0, :4] for g in SP.GUESSES]
                for a in range(3):
                    for b in range(a + 1, 3):
                        assert np.max(np.abs(ki[a] - ki[b])) > 1e-3 * max(np.max(np.abs(ki[a])), np.max(np.abs(ki[b]))), (cid, s, flag, p, a, b, ki[a], ki[b])


@pytest.mark.parametrize("cid", [c for c in SP.IDS if SP.BY_ID[c].shape[2] > 0])
def test_complementarity_tolerance_decides(cid):
    """COMP_CELL: on every problem at least two iterations end with kmax < termination_kkt_tol while mu >= termination_complementarity_tol, so
    the second operand of the termination test alone keeps the loop going -- and the run still ends SATISFIED_KKT_TOL, so it is also what
    stops it.  (m = 0: mu = 0, the operand cannot decide.)"""
    kw = SP.params(cid, SP.COMP_CELL, "full")
    for p, ref in enumerate(SP.referee(cid, "full")[SP.COMP_CELL]):
        assert ref.term == SP.SATISFIED_KKT_TOL and ref.nit < kw["max_iterations"], (cid, p, ref.term, ref.nit)
        assert SP.undecided_iterations(ref, kw) >= 2, (cid, p, SP.undecided_iterations(ref, kw))


def test_full_runs_are_mostly_clear(capsys):
    """Full runs under COMPLEMENTARITY / FIXED_DECREASE: at least 3/4 of each cell's problems (all cases pooled) have every decision clear of
    its threshold, so termination, iteration count and optimum are checked exactly there.  The shares per strategy are printed."""
    share = {}
    for cell in SP.CELLS:
        clear = [SP.first_edge(cid, ref.margins) is None for cid in SP.IDS for ref in SP.referee(cid, "full")[cell]]
        share.setdefault(cell.strategy, []).extend(clear)
        if cell.strategy != SP.PREDICTOR_CORRECTOR:
            assert 4 * sum(clear) >= 3 * len(clear), (SP.cell_id(cell), sum(clear), len(clear))
    with capsys.disabled():
        print("\nfull runs with every decision clear: " + ", ".join("%s %d/%d" % (SP.STRATEGY_NAME[s], sum(v), len(v)) for s, v in share.items()))


@pytest.mark.parametrize("cid", ["tiny", "n32", "tiny-m0", "f32-pad"])
def test_replayed_records_are_the_oracles(cid):
    """The records the referee takes from the replay of oracle/margins.py are, bit for bit, those orc_solve writes."""
    for kind in ("short", "full"):
        for cell, refs in SP.referee(cid, kind).items():
            for p, ref in enumerate(refs):
                term, rec = SP.oracle_records(cid, p, SP.params(cid, cell, kind))
                assert term == ref.term and rec.shape == ref.records.shape, (cid, kind, SP.cell_id(cell), p)
                np.testing.assert_array_equal(rec, ref.records)
