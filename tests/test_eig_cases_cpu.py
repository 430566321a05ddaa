"""The exact-spectrum cases of tests/eig_cases.py, checked on the host: symmetric to the bit, exact (rebuilt in fractions.Fraction), and
numpy.linalg.eigvalsh (LAPACK) within the bound the GPU tests use -- which is where that bound's constant comes from: C_BOUND must be
8 x max(r, 1) for r = LAPACK's worst error / (n eps |A|) over all cases (profiles/eig_spectra.txt: r = 0.706, C = 8)."""
import fractions

import numpy as np
import pytest

from tests import eig_cases as E

CASES64 = list(E.all_cases(False))
CASES32 = list(E.all_cases(True))
J_SHAPES = [(8, 5), (8, 12), (33, 20), (33, 40), (64, 48), (64, 70)]


def test_every_case_is_symmetric_to_the_bit_and_has_its_spectrum_listed():
    for c in CASES64 + CASES32:
        assert c.A.shape == (c.n, c.n) and c.A.dtype == np.float64 and len(c.spec) == c.n, c.name
        assert np.array_equal(c.A, c.A.T), c.name
        assert np.all(np.isfinite(c.A)), c.name
        # trace and Frobenius norm of the exact spectrum (loose: this only catches a wrong spectrum list, exactness is tested below)
        assert abs(float(np.trace(c.A)) - float(c.spec.sum())) <= 1e-9 * max(c.scale, 1) * c.n, c.name
        assert abs(float((c.A * c.A).sum()) - float((c.spec * c.spec).sum())) <= 1e-9 * max(c.scale, 1) ** 2 * c.n, c.name
    for c in CASES32:
        assert np.array_equal(c.A.astype(np.float32).astype(np.float64), c.A), c.name


def test_dense_cases_are_dense_where_the_construction_allows():
    """Three levels of 16 from n = 17 on: the Householder loop of the kernel gets real reflections in every column."""
    for c in CASES64:
        fam = c.name.rsplit("_n", 1)[0]
        if fam in ("straddle", "all_positive", "all_negative", "near_zero_negative", "near_zero_positive", "wide_range") and c.n >= 17:
            assert np.count_nonzero(c.A) >= 0.85 * c.n * c.n, (c.name, np.count_nonzero(c.A))


@pytest.mark.parametrize("family", E.FAMILIES)
def test_dense_cases_are_exact(family):
    """Three representative sizes per family, rebuilt reflection by reflection in exact rational arithmetic (and the fp32 form at n = 16)."""
    for n, fp32 in ((3, False), (17, False), (33, False), (16, True)):
        ints, q = E.spectrum(family, n, fp32)
        A = E.dense_case(family, n, fp32).A
        F = E.exact_dense_fraction(ints, q, E.seed_of(family, n, fp32), fp32)
        for i in range(n):
            for j in range(n):
                assert fractions.Fraction(float(A[i, j])) == F[i][j], (family, n, i, j)


def test_big_dense_cases_have_the_exact_similarity_invariants():
    """n = 141 and 150 are too slow for Fraction: Q Q^T = c^(2L) I in integers instead (so A is an exact similarity of diag(spec))."""
    for n in (140, 141, 150):
        for fp32 in (False, True):
            cmax = E.cmax_for(n, fp32)
            Q, sh = E.q_matrix(n, 2 if fp32 else 3, cmax, E.seed_of("straddle", n, fp32))
            assert np.array_equal(Q @ Q.T, (1 << (2 * sh)) * np.eye(n, dtype=np.int64))


@pytest.mark.parametrize("n,m_r", J_SHAPES)
def test_j_cases_are_exact(n, m_r):
    c = E.j_case(n, m_r)
    assert c.J.shape == (m_r, n)
    assert np.array_equal(c.J.astype(np.float32).astype(np.float64), c.J)
    F = [[fractions.Fraction(float(x)) for x in row] for row in c.J]
    G = c.J.T @ c.J                                   # exact in fp64 (every partial sum is on a coarse grid); compare with the rational product
    for i in range(0, n, max(1, n // 8)):
        for j in range(n):
            assert fractions.Fraction(float(G[i, j])) == sum(F[r][i] * F[r][j] for r in range(m_r)), (i, j)
    w = np.linalg.eigvalsh(G + 0.5 * np.eye(n))
    ref = np.sort(c.spec(0.5))
    assert np.max(np.abs(w - ref)) <= E.bound(n, ref.max())
    assert np.array_equal(c.spec(-1.0), c.s2) and np.array_equal(c.spec(float("nan")), c.s2)
    if m_r < n:
        assert np.count_nonzero(c.s2 == 0.0) == n - m_r


def lapack_ratio(c):
    """max error of {min, max, abs_min} and of the whole sorted spectrum, over n eps |A| (n DBL_MIN for the zero matrix)."""
    w = np.linalg.eigvalsh(c.A)
    exact = np.sort(c.spec)
    err = max(float(np.max(np.abs(w - exact))), float(np.max(np.abs(E.stats(w) - c.ref))))
    return err / E.bound(c.n, c.scale, 1.0)


def test_lapack_meets_the_bound_and_fixes_its_constant(capsys):
    worst, per_n = ("", 0.0), {}
    for c in CASES64 + CASES32:
        r = lapack_ratio(c)
        per_n[c.n] = max(per_n.get(c.n, 0.0), r)
        if r > worst[1]:
            worst = (c.name, r)
        assert r <= E.C_BOUND, (c.name, r)                   # eigvalsh is inside the bound of the GPU test on every case
    with capsys.disabled():
        print("\nLAPACK worst error / (n eps |A|): %.3f at %s; per n: %s; C = %g"
              % (worst[1], worst[0], " ".join("%d:%.3f" % kv for kv in sorted(per_n.items())), E.C_BOUND))
    assert E.C_BOUND == 8.0 * max(1.0, worst[1]), worst     # C is 8 x max(measured, 1), not a choice


def test_the_bound_is_far_below_the_old_tolerance():
    assert E.bound(150, 1.0) * 100 <= 1e-10
