"""The null-space case table (tests/nullspace_cases.py) held to itself, without a GPU: the long-double reference is well posed, the oracle's
own error is small enough to referee the kernel, and every case takes the path it was built for."""
import numpy as np
import pytest

from tests import nullspace_cases as NC


def test_the_table_has_every_family_and_shape():
    cs = NC.cases()
    assert {c.family for c in cs} == set("ABCDEFG")
    for fam in "ABCE":                                                   # these families run as fp32 plans as well
        f64 = {c.name[:-4] for c in cs if c.family == fam and c.dtype == "f64" and c.name != NC.CAPACITY_CASE and c.keep is None}
        assert f64 == {c.name[:-4] for c in cs if c.family == fam and c.dtype == "f32"}
    assert all(c.dtype == "f64" for c in cs if c.family in "DFG")
    assert {(c.n, c.k) for c in cs if c.family == "A"} == {(8, 1), (8, 3), (40, 8), (41, 8), (70, 5)}
    assert NC.CAPACITY_K == 24 and NC.by_name(NC.CAPACITY_CASE).k == 24    # 8 (129 (128 + 24) + 640 + 96 + 16) + 32 = 162 912 B <= 163 840 B < k = 25
    for c in cs:
        if c.dtype == "f32":                                             # every fp32 input is an fp32 number
            for a in (c.A, c.b, c.G, c.c, c.J, c.r):
                assert a is None or np.array_equal(a, a.astype(np.float32).astype(np.float64)), c.name
        if c.G is not None:
            assert np.array_equal(c.G, c.G.transpose(0, 2, 1)), c.name
    lam = NC.by_name("G_lambda_vec_n12_k3").lam
    assert np.any(lam == 0) and np.any(lam < 0) and np.any(lam > 0)


@pytest.mark.parametrize("name", NC.names())
def test_reference_is_well_posed(name):
    """The long-double solve satisfies its own KKT system to 64 long-double eps of the system's scale."""
    case = NC.by_name(name)
    x, res = NC.reference(name)
    ok = case.term == NC.SUCCESS
    assert np.all(np.isfinite(x[ok].astype(np.float64))) and np.all(np.isnan(x[~ok].astype(np.float64)))
    assert res.max() <= 64 * NC.EPS_LD, (name, res.max() / NC.EPS_LD)


@pytest.mark.parametrize("name", NC.names())
def test_oracle_error_and_decisions(name):
    case = NC.by_name(name)
    o = NC.oracle_errors(name)
    print(f"{name}: oracle forward error {o.E_case:.2f} eps, constraint backward error {o.BE_case:.3f} eps")
    assert np.array_equal(o.term, case.term), name
    ok = case.term == NC.SUCCESS
    assert np.all(np.isfinite(o.fwd[ok])) and np.all(np.isfinite(o.be[ok]))
    if case.family != "F":                                               # the condition the GPU bound rests on
        assert o.E_case <= NC.ORACLE_FWD_MAX, (name, o.fwd)
    for p in range(case.B):
        diag, rank, P = NC.pivoted_qr(case.A[p])
        want = case.k if case.rank is None else case.rank[p]
        assert rank == want, (name, p)
        # no rank decision on a knife edge, in the PLAN's precision: the pivots that count are RANK_MARGIN above the threshold
        # |R|_max eps min(n, k), the others exactly zero or as far below
        thr = diag.max() * case.eps * min(case.n, case.k)
        assert np.all(diag[:want] >= NC.RANK_MARGIN * thr) and np.all(diag[want:] * NC.RANK_MARGIN <= thr), (name, p, diag, thr)
        if case.dom is None:
            continue
        # Family A: row j is the j-th pivot and its dominant entry d (column j) lands on the diagonal: |R_jj| = d to 2^-20.  |R_jj| is the
        # norm of what is left of the row, up to sqrt(d^2 + |off|^2) = d (1 + |off|^2 / 2 d^2): in fp64 the off-axis entries are 2^-24 of d
        # or less and the term vanishes, in fp32 those of s = 10 add up to n 2^-21 / 3, beyond 2^-20 from n = 8 on -- so it is allowed for.
        assert np.array_equal(P, np.arange(case.k)), (name, p, P)
        for j in np.flatnonzero(np.isfinite(case.dom[p])):
            d = case.dom[p, j]
            off2 = np.sum(case.A[p, j] ** 2) - d * d
            assert abs(case.A[p, j, j]) == d and off2 < 2.0 ** -12 * d * d
            assert abs(diag[j] - d) <= (2.0 ** -20 + off2 / (d * d)) * d, (name, p, j)
            if case.dtype == "f64":
                assert abs(diag[j] - d) <= 2.0 ** -20 * d, (name, p, j)


def test_family_b_exact_entries_are_the_references():
    """-b / a is the reference's x at the constrained index, to the rounding of the long-double solve."""
    for case in (c for c in NC.cases() if c.family == "B"):
        x, _ = NC.reference(case.name)
        assert len(case.exact_idx) == case.B // 2
        for p in range(case.B // 2):                                     # the zero-tail half: the j-th largest row sits on axis j
            got = x[p][case.exact_idx[p]]
            assert np.max(np.abs(got - case.exact_val[p])) <= 64 * NC.EPS_LD * np.max(np.abs(x[p])), (case.name, p)
            order = np.argsort(-np.abs(case.A[p]).max(axis=1))
            assert np.array_equal(case.exact_idx[p][order], np.arange(case.k))
            assert p >= 2 or not np.array_equal(order, np.arange(case.k))   # ... in an order the pivot search has to undo
        for p in range(case.B):                                          # axis rows, powers of two
            nz = case.A[p][case.A[p] != 0]
            assert len(nz) == case.k and np.array_equal(np.log2(np.abs(nz)), np.round(np.log2(np.abs(nz))))


def test_family_c_scaling_is_exact_and_reorders_the_pivots():
    assert NC.C_SPREAD["f64"] == 20
    for case in (c for c in NC.cases() if c.family == "C" and c.A_ref is not None):
        s = case.A[:, :, 0] / case.A_ref[:, :, 0]
        assert np.array_equal(np.log2(s), np.round(np.log2(s))) and np.all(np.log2(s).min(axis=1) == -NC.C_SPREAD[case.dtype])
        assert np.all(np.log2(s).max(axis=1) == NC.C_SPREAD[case.dtype])
        assert np.array_equal(case.A, case.A_ref * s[:, :, None]) and np.array_equal(case.b, case.b_ref * s)
        assert any(not np.array_equal(NC.pivoted_qr(case.A[p])[2], NC.pivoted_qr(case.A_ref[p])[2]) for p in range(case.B))


def test_family_f_margins():
    """The reduced Hessian's smallest eigenvalue is +-2^-20 |G| as built (to rounding), far from the decision's rounding noise."""
    for tag, sgn in (("pos", 1.0), ("neg", -1.0)):
        case = NC.by_name(f"F_margin_{tag}_n10_k3")
        for p in range(case.B):
            Z = np.linalg.svd(case.A[p])[2][case.k:].T
            w = np.linalg.eigvalsh(Z.T @ case.G[p] @ Z)
            assert abs(np.linalg.norm(case.G[p], 2) - 1.0) < 1e-12
            assert abs(w[0] - sgn * 2.0 ** -20) < 1e-12 and w[1] > 0.2
