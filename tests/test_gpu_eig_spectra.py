"""mo_qp_eigenvalue_stats (qp_eig_kernel, csrc/eig_kernels.hip) on matrices whose spectra are known EXACTLY (tests/eig_cases.py): integer
spectra under dyadic Householder similarities, analytic tridiagonals, exact J-level input.  No numerical reference is involved, and the bound is
C n eps |A| with C = 8 from LAPACK's own error on the same matrices (tests/test_eig_cases_cpu.py, profiles/eig_spectra.txt) -- 375 times
below the 1e-10 |G| of tests/test_gpu_eig.py at n = 150, tight enough to see an inaccurate reflection or a wrong neighbour of zero.

  a. {min, max, abs_min} within the bound for every spectrum family and analytic matrix at n = 1 ... 150 (n = 140: the last LDS-resident
     size, n = 141: the first in the plan's workspace), fp64, and on fp32 plans (+ 2^-24 |value| for the one output rounding);
  b. the strict upper triangle of G is never read: 1e30 and NaN there change nothing;
  c. J-level input in four layouts (packed, J_ld = n + 3, column-major with J_ld = m_r + 2, padded J_stride; NaN in every gap) with m_r < n
     and m_r > n, scalar lambda > 0, = 0, < 0 and a lambda_vec that mixes them: within the bound, every layout the bits of the packed one;
  d. 2^s A gives 2^s times the bits of A for s up to +-900 (J: 2^+-260 J), because the kernel scales by an exact power of two;
  e. a NaN or +-inf among the entries read gives three NaNs for that problem and leaves the bits of its neighbours alone; a NaN lambda acts
     as no damping (`if (lambda > 0)`, nonlinear.cc:187-189);
  f. one workgroup walking healthy, NaN, zero, c I, healthy (n = 141 on a plan of max_batch = 1, whose single workspace slot clamps the grid
     to one workgroup; launch_qp_eig does not clamp an LDS-resident grid): the last problem has the bits of running alone.

Every check prints `EIGRATIO <test> <case> <max error / bound>` (pytest -s shows them; the worst per family is in profiles/eig_spectra.txt).
Outputs are pre-filled with a canary, so an unwritten output fails.  The calls go to the C ABI (as tests/test_gpu_second_problem.py::eig_run)
so that layouts, plans and batches can vary."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from mini_opt_amd import _lib as L
from mini_opt_amd import qp as Q
from tests import eig_cases as E
from tests.sens_fixtures import Plan

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
NP = {F64: np.float64, F32: np.float32}
CANARY = 777.0
NAN = float("nan")

# batches of eight and seven per size; the hard ones (2^20 dynamic range, the two near-zero families, the alternating blocks) in the middle
GROUPS = (("c_identity", "straddle", "wide_range", "near_zero_negative", "coupled", "kac", "zero", "all_positive"),
          ("rank_one", "multiplicities", "near_zero_positive", "blocks", "second_difference", "all_negative", "ones_shift"))
assert sorted(GROUPS[0] + GROUPS[1]) == sorted(E.FAMILIES + E.ANALYTIC)


@functools.lru_cache(maxsize=None)
def case(name, n, fp32=False):
    c = E.case(name, n, fp32)
    c.A.setflags(write=False)
    return c


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda:0").contiguous()


def launch(plan, prob, B, dt, keep):
    out = torch.full((B, 3), CANARY, dtype=dt, device="cuda:0")
    L.check(L.lib().mo_qp_eigenvalue_stats(plan.h, C.byref(prob), B, Q._ptr(out), Q._stream()))
    torch.cuda.synchronize()
    del keep
    return out.cpu().numpy()


def run_G(mats, dt=F64, max_batch=None):
    """mats[b][row, col] = G_b(row, col): the tensor is [b, col, row] (column-major memory), n x n packed.  -> [B, 3] numpy in the plan's dtype."""
    mats = np.asarray(mats, dtype=np.float64)
    B, n = mats.shape[0], mats.shape[1]
    G = dev(mats.transpose(0, 2, 1), dt)
    c = torch.zeros(B, n, dtype=dt, device="cuda:0")
    prob = L.Problem()
    prob.G, prob.G_stride, prob.G_ld = Q._ptr(G), n * n, n
    prob.c, prob.c_stride = Q._ptr(c), n
    with Plan(n, 0, 0, 0, dt, max_batch or B) as plan:
        return launch(plan, prob, B, dt, (G, c))


def with_upper(A, fill):
    """G(row, col) = fill for row < col: the triangle that must not be read."""
    G = np.array(A, dtype=np.float64)
    G[np.triu_indices(G.shape[0], 1)] = fill
    return G


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def check(tag, name, got, ref, bnd, fp32=False):
    """|got - ref| <= bnd (+ 2^-24 |ref| for the output rounding of an fp32 plan) on each of {min, max, abs_min}; prints the worst ratio."""
    got = np.asarray(got, dtype=np.float64)
    lim = bnd + (2.0 ** -24 * np.abs(ref) if fp32 else 0.0)
    assert np.all(np.isfinite(got)), (tag, name, got)
    ratio = float(np.max(np.abs(got - ref) / lim))
    print("EIGRATIO %s %s %.4f" % (tag, name, ratio))
    assert ratio <= 1.0, (tag, name, got.tolist(), np.asarray(ref).tolist(), ratio)


# ---------------------------------------------------------------------------------------------------------------------------------------
# a. exact spectra
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [0, 1])
@pytest.mark.parametrize("n", E.SIZES_F64)
def test_exact_spectra_fp64(n, group):
    cases = [case(name, n) for name in GROUPS[group]]
    got = run_G([c.A for c in cases])
    for p, c in enumerate(cases):
        check("a_f64", c.name, got[p], c.ref, c.bound)


@pytest.mark.parametrize("group", [0, 1])
@pytest.mark.parametrize("n", E.SIZES_F32)
def test_exact_spectra_fp32_plan(n, group):
    """fp32-exact inputs, widened on load and computed in fp64: the fp64 bound plus the single rounding of the output."""
    cases = [case(name, n, True) for name in GROUPS[group] if name != "kac"]
    got = run_G([c.A for c in cases], F32)
    assert got.dtype == np.float32
    for p, c in enumerate(cases):
        check("a_f32", c.name, got[p], c.ref, c.bound, fp32=True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# b. the strict upper triangle
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", E.SIZES_F64)
def test_strict_upper_triangle_is_never_read(n):
    cases = [case(name, n) for name in ("straddle", "near_zero_negative", "wide_range", "multiplicities", "second_difference")]
    fills = [None, 1e30, NAN, NAN, -1e30]
    clean = run_G([c.A for c in cases])
    got = run_G([c.A if f is None else with_upper(c.A, f) for c, f in zip(cases, fills)])
    for p, c in enumerate(cases):
        check("b_upper", "%s_fill_%s" % (c.name, fills[p]), got[p], c.ref, c.bound)
    assert same_bits(got, clean)


# ---------------------------------------------------------------------------------------------------------------------------------------
# c. J-level input
# ---------------------------------------------------------------------------------------------------------------------------------------
J_LAYOUTS = ("packed", "row_ld", "col_ld", "stride")


def j_problem(J, layout, dt, lam=0.0, lam_vec=None):
    """(mo_problem, tensors to keep alive) for J [B, m_r, n]; every gap of a padded layout holds NaN."""
    B, m_r, n = J.shape
    prob = L.Problem()
    if layout == "packed":
        buf, stride, ld, lay = J, m_r * n, n, L.MO_ROW_MAJOR
    elif layout == "row_ld":
        buf = np.full((B, m_r, n + 3), NAN); buf[:, :, :n] = J
        stride, ld, lay = m_r * (n + 3), n + 3, L.MO_ROW_MAJOR
    elif layout == "col_ld":
        buf = np.full((B, n, m_r + 2), NAN); buf[:, :, :m_r] = J.transpose(0, 2, 1)
        stride, ld, lay = n * (m_r + 2), m_r + 2, L.MO_COL_MAJOR
    else:
        buf = np.full((B, m_r * n + 5), NAN); buf[:, :m_r * n] = J.reshape(B, m_r * n)
        stride, ld, lay = m_r * n + 5, n, L.MO_ROW_MAJOR
    Jt = dev(buf, dt)
    r = torch.zeros(B, m_r, dtype=dt, device="cuda:0")
    prob.J, prob.J_stride, prob.J_ld, prob.J_layout = Q._ptr(Jt), stride, ld, lay
    prob.r, prob.r_stride = Q._ptr(r), m_r
    prob.lam = float(lam)
    keep = [Jt, r]
    if lam_vec is not None:
        lv = dev(np.asarray(lam_vec, dtype=np.float64), dt)
        prob.lambda_vec, prob.lambda_stride = Q._ptr(lv), 1
        keep.append(lv)
    return prob, keep


def run_J(plan, J, layout, dt, lam=0.0, lam_vec=None):
    prob, keep = j_problem(J, layout, dt, lam, lam_vec)
    return launch(plan, prob, J.shape[0], dt, keep)


@functools.lru_cache(maxsize=None)
def j_batch(n, m_r, B=4):
    cs = [E.j_case(n, m_r, v) for v in range(B)]
    return cs, np.stack([c.J for c in cs])


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,m_rs", [(8, (5, 12)), (33, (20, 40)), (64, (48, 70))])
def test_j_level_input_in_every_layout(n, m_rs, dt):
    fp32 = dt == F32
    for m_r in m_rs:
        cs, J = j_batch(n, m_r)
        B = len(cs)
        lam_modes = {"pos": (0.75, None), "zero": (0.0, None), "neg": (-2.0, None), "vec": (0.125, [0.5, 0.0, -1.0, 0.25])}
        with Plan(n, 0, 0, m_r, dt, B) as plan:
            for mode, (lam, lam_vec) in lam_modes.items():
                got = {lay: run_J(plan, J, lay, dt, lam, lam_vec) for lay in J_LAYOUTS}
                for p, c in enumerate(cs):
                    spec = c.spec(lam_vec[p] if lam_vec else lam)      # lam < 0 acts as 0; lambda_vec overrides lambda
                    # (m_r < n with no damping: a zero cluster of multiplicity n - m_r, abs_min <= the bound)
                    check("c_J_%s" % ("f32" if fp32 else "f64"), "%s_%s" % (c.name, mode), got["packed"][p], E.stats(spec),
                          E.bound(n, float(spec.max())), fp32)
                for lay in J_LAYOUTS[1:]:
                    assert same_bits(got[lay], got["packed"]), (n, m_r, mode, lay)


# ---------------------------------------------------------------------------------------------------------------------------------------
# d. power-of-two scaling
# ---------------------------------------------------------------------------------------------------------------------------------------
SHIFTS = (100, -100, 400, -400, 520, -520, 900, -900)


@pytest.mark.parametrize("n", [16, 141])
def test_power_of_two_scaling_of_G(n):
    """2^s A in the middle of a batch whose other problems stay as they are: 2^s times the bits of s = 0, and within the (scaled) bound."""
    first, c, last = case("straddle", n), case("near_zero_negative", n), case("multiplicities", n)
    base = run_G([first.A, c.A, last.A])
    check("d_scale", c.name + "_s0", base[1], c.ref, c.bound)
    for s in SHIFTS:
        got = run_G([first.A, np.ldexp(c.A, s), last.A])
        check("d_scale", "%s_s%+d" % (c.name, s), np.ldexp(got[1], -s), c.ref, c.bound)
        assert same_bits(got[1], np.ldexp(base[1], s)), (n, s, got[1].tolist(), np.ldexp(base[1], s).tolist())
        assert same_bits(got[[0, 2]], base[[0, 2]]), (n, s)


@pytest.mark.parametrize("m_r", [20, 40])
def test_power_of_two_scaling_of_J(m_r):
    """2^+-260 J: G = J^T J scales by 2^+-520 (lambda = 0; m_r = 20 < n leaves a zero cluster)."""
    n = 33
    cs, J = j_batch(n, m_r)
    with Plan(n, 0, 0, m_r, F64, len(cs)) as plan:
        base = run_J(plan, J, "packed", F64)
        for s in (260, -260):
            Js = J.copy(); Js[1] = np.ldexp(J[1], s)
            got = run_J(plan, Js, "packed", F64)
            spec = cs[1].spec(0.0)
            check("d_scale_J", "%s_s%+d" % (cs[1].name, s), np.ldexp(got[1], -2 * s), E.stats(spec), E.bound(n, float(spec.max())))
            assert same_bits(got[1], np.ldexp(base[1], 2 * s)), (m_r, s, got[1].tolist())
            assert same_bits(got[[0, 2, 3]], base[[0, 2, 3]]), (m_r, s)


# ---------------------------------------------------------------------------------------------------------------------------------------
# e. non-finite input
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 17, 141])
def test_non_finite_entry_gives_nan_for_that_problem_alone(n):
    names = ("straddle", "near_zero_positive", "all_negative", "blocks")
    mats = [case(name, n).A for name in names]
    base = run_G(mats)
    for p, name in enumerate(names):
        check("e_base", case(name, n).name, base[p], case(name, n).ref, case(name, n).bound)
    mid = n // 2
    for bad in (NAN, float("inf"), float("-inf")):
        for (r, c) in ((0, 0), (n - 1, 0), (n - 1, n - 1), (mid + 1, mid)):      # G(row, col), row >= col: the triangle that is read
            G = np.array(mats[1]); G[r, c] = bad                                     # (the mirror entry G(c, r) stays finite: it is not read)
            got = run_G([mats[0], G, mats[2], mats[3]])
            assert np.all(np.isnan(got[1])), (n, bad, r, c, got[1].tolist())
            assert same_bits(got[[0, 2, 3]], base[[0, 2, 3]]), (n, bad, r, c)


def test_non_finite_j_gives_nan_and_nan_lambda_is_no_damping():
    n, m_r = 8, 12
    cs, J = j_batch(n, m_r)
    with Plan(n, 0, 0, m_r, F64, len(cs)) as plan:
        base = run_J(plan, J, "packed", F64, 0.75)
        for (r, c) in ((0, 0), (m_r - 1, n - 1), (5, 3), (m_r - 1, 0)):           # the last one: a NaN in a zero row of J
            for bad in (NAN, float("inf")):
                Jb = J.copy(); Jb[2, r, c] = bad
                got = run_J(plan, Jb, "packed", F64, 0.75)
                assert np.all(np.isnan(got[2])), (r, c, bad, got[2].tolist())
                assert same_bits(got[[0, 1, 3]], base[[0, 1, 3]]), (r, c, bad)
        undamped = run_J(plan, J, "packed", F64, 0.0)
        for p, c in enumerate(cs):
            check("e_J", c.name + "_lam0", undamped[p], E.stats(c.spec(0.0)), E.bound(n, float(c.spec(0.0).max())))
        assert same_bits(run_J(plan, J, "packed", F64, NAN), undamped)
        vec = run_J(plan, J, "packed", F64, 0.75, [0.75, NAN, 0.75, 0.0])
        assert same_bits(vec[[1, 3]], undamped[[1, 3]]) and same_bits(vec[[0, 2]], base[[0, 2]])


# ---------------------------------------------------------------------------------------------------------------------------------------
# f. what a problem leaves behind in LDS
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_nothing_stale_after_a_nan_or_degenerate_predecessor():
    n = 141
    first, last = case("wide_range", n), case("near_zero_negative", n)
    poisoned = np.array(case("straddle", n).A); poisoned[n // 2 + 1, n // 2] = NAN
    zero, ident = case("zero", n), case("c_identity", n)
    got = run_G([first.A, poisoned, zero.A, ident.A, last.A], max_batch=1)        # one workspace slot: one workgroup walks the batch
    alone = run_G([last.A], max_batch=1)
    check("f_walk", first.name, got[0], first.ref, first.bound)
    assert np.all(np.isnan(got[1])), got[1].tolist()
    check("f_walk", zero.name, got[2], zero.ref, zero.bound)
    check("f_walk", ident.name, got[3], ident.ref, ident.bound)
    check("f_walk", last.name, got[4], last.ref, last.bound)
    assert same_bits(got[4:5], alone), (got[4].tolist(), alone.tolist())
