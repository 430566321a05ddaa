"""Matrices whose spectra are known exactly, for the eigenvalue kernel (csrc/eig_kernels.hip, mo_qp_eigenvalue_stats).  Host only: numpy and
the standard library, no torch, no GPU, so the CPU suite imports it (tests/test_eig_cases_cpu.py) as well as tests/test_gpu_eig_spectra.py.

Exact dense matrices.  A = Q diag(spec) Q^T with Q a product of Householder reflections H = I - (2 / c) v v^T whose v has c entries of +-1 (c a
power of two, 2 <= c <= 16) at seeded positions and zeros elsewhere.  The reflections come in LEVELS: one level is a seeded random partition of
the indices into groups of c (the last groups of a level take the smaller powers of two that still fit), one reflection per group.  The
reflections of a level have disjoint supports, so together they are one orthogonal matrix whose entries are multiples of 2 / c <= 1 / 8 ... 1;
L levels of c = 16 give a Q with entries on the grid 8^-L and an A on the grid 2^(q - 6 L) for a spectrum of integers times 2^q, whatever n is,
and |A_ij| <= max |spec|: a few dozen bits, exact in float64 (the fp32 cases use two levels of c <= 8 and integers below 2^16: 24 bits).  Three
levels of 16 connect every index with 4096 others: A is dense from n = 17 on.  The build itself runs in integers (numpy int64: c^L Q and
c^(2L) A), so no rounding can happen on the way; tests/test_eig_cases_cpu.py rebuilds a sample with fractions.Fraction.
For n <= 3 only c = 2 fits, whose reflection is a signed swap: those matrices are permuted diagonals ("ones_shift" below is the dense one).

Exact J-level input.  J = the first m_r rows of diag(s) Q, or all n followed by zero rows: J^T J = Q^T diag(s^2 | 0) Q, and with a dyadic
lambda the spectrum of J^T J + max(lambda, 0) I is {s_i^2 + max(lambda, 0)} and n - m_r times max(lambda, 0).  Every partial sum of a J^T J
entry is bounded by max s^2 and lies on the grid 2^(2q - 6L): the kernel's fp64 fma chain forms G without rounding.

Analytic matrices.  second_difference: tridiag(-1, 2, -1), lambda_j = 2 - 2 cos(j pi / (n + 1)) (reference in numpy.longdouble); kac: zero
diagonal, off-diagonal sqrt(j (n - j)), eigenvalues n - 1 - 2 j (the square roots are rounded, which moves an eigenvalue by at most
eps n / 2: inside every bound used here); blocks: block-diagonal of second-difference blocks and exact dense blocks, so that the reflection
loop alternates between its "already tridiagonal" branch and real reflections; ones_shift: a 1 1^T + b I, spectrum {b (n - 1 times), n a + b},
dense at every n >= 2; coupled: [[T, e I], [e I, T]] with T = tridiag(+1, 2, +1) and e = 2^-20, spectrum lambda_j(T) +- e because the two
Kronecker terms commute: every column of the first half has a POSITIVE sub-diagonal entry that dominates its tail by 2^20, which is where
a Householder vector built with the cancelling sign (v_0 = x_0 - |x|) loses |H x - alpha e_1| ~ 2 eps x_0^2 / |tail|.

THE BOUND.  |computed - exact| <= C n eps |A| for each of {min, max, abs_min}, |A| = max |exact eigenvalue|; for a zero matrix C n DBL_MIN.
C is not chosen: it is 8 x max(r, 1), where r is the worst error / (n eps |A|) of numpy.linalg.eigvalsh (LAPACK) over every case below
(tests/test_eig_cases_cpu.py measures it and asserts r <= C / 8; profiles/eig_spectra.txt records it).  Measured r = 0.706 (ones_shift at n = 17;
0.67 at n = 3, where one ulp of |A| is already a third of n eps |A|; 0.23 or less from n = 33 on), hence C = 8.  The factor 8 is for the kernel's other summation
orders (256-thread reductions, fma).  At n = 150 the bound is 8 x 150 x 2.2e-16 = 2.7e-13 |A|: 375 times below the 1e-10 |G| of
tests/test_gpu_eig.py."""
import fractions
from dataclasses import dataclass

import numpy as np

EPS = float(np.finfo(np.float64).eps)
DBL_MIN = float(np.finfo(np.float64).tiny)
C_BOUND = 8.0

SIZES_F64 = (1, 2, 3, 16, 17, 33, 64, 140, 141, 150)   # 140: the last size whose matrix is LDS resident, 141: the first in the plan's workspace
SIZES_F32 = (16, 64, 141)
FAMILIES = ("straddle", "multiplicities", "c_identity", "zero", "rank_one", "all_positive", "all_negative", "near_zero_negative",
            "near_zero_positive", "wide_range")
ANALYTIC = ("second_difference", "kac", "blocks", "ones_shift", "coupled")


def bound(n, scale, c=C_BOUND):
    """C n eps |A|; C n DBL_MIN for the zero matrix."""
    return c * n * (EPS * scale if scale > 0 else DBL_MIN)


def stats(w):
    w = np.asarray(w)
    return np.array([w.min(), w.max(), np.abs(w).min()])


@dataclass
class Case:
    name: str
    A: np.ndarray          # n x n, symmetric to the bit
    spec: np.ndarray       # the exact eigenvalues (float64, or longdouble for second_difference), any order
    fp32: bool = False     # every entry is exact in float32

    @property
    def n(self):
        return self.A.shape[0]

    @property
    def scale(self):
        return float(np.abs(self.spec).max())

    @property
    def ref(self):
        """{min, max, abs_min} of the exact spectrum, in float64."""
        return stats(self.spec).astype(np.float64)

    @property
    def bound(self):
        return bound(self.n, self.scale)


# ---------------------------------------------------------------------------------------------------------------------------------------
# spectra: integers `ints` and a power of two `q`; the eigenvalues are ints * 2^q
# ---------------------------------------------------------------------------------------------------------------------------------------
def spectrum(family, n, fp32=False):
    a = np.arange(n, dtype=np.int64)
    q = 0
    if family == "straddle":                    # distinct integers on both sides of zero; an exact 0 from n = 3 on
        ints = a - n // 3 if n >= 3 else 2 * a - 1
    elif family == "multiplicities":            # [-3] * 5 + [0] * 4 + [2] * rest, shrunk below n = 15
        k1, k2 = min(5, n // 3), min(4, n // 3)
        ints = np.array([-3] * k1 + [0] * k2 + [2] * (n - k1 - k2), dtype=np.int64)
    elif family == "c_identity":                # zero-width Gershgorin interval
        ints = np.full(n, 3, dtype=np.int64)
    elif family == "zero":
        ints = np.zeros(n, dtype=np.int64)
    elif family == "rank_one":
        ints = np.array([0] * (n - 1) + [5], dtype=np.int64)
    elif family == "all_positive":              # no eigenvalue below zero: the kernel's target 2 is invalid
        ints = a + 1
    elif family == "all_negative":              # none above: target 3 is invalid
        ints = -(a + 1)
    elif family in ("near_zero_negative", "near_zero_positive"):   # {..., -2, -1, 2, 3, ...} and its negative
        nneg = (n + 1) // 2
        ints = np.concatenate([-(np.arange(nneg, dtype=np.int64) + 1), np.arange(n - nneg, dtype=np.int64) + 2])
        if family == "near_zero_positive":
            ints = -ints
    elif family == "wide_range":                # {-W, -1, W, 2, 3, ...} / 1024: |max| / |min| = W = 2^20 (2^16 in fp32)
        W = 1 << (16 if fp32 else 20)
        ints = np.array(([-W, -1, W] + list(range(2, n)))[:n], dtype=np.int64)
        q = -10
    else:
        raise KeyError(family)
    assert len(ints) == n
    return ints, q


# ---------------------------------------------------------------------------------------------------------------------------------------
# reflections
# ---------------------------------------------------------------------------------------------------------------------------------------
def levels_of(n, nlev, cmax, seed):
    """nlev levels; a level is a list of (c, positions, signs): a seeded partition of a permutation of 0 .. n - 1 into groups of cmax, then of
    the smaller powers of two down to 2 (an index left over stays untouched at that level)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nlev):
        perm = rng.permutation(n)
        lvl, at, c = [], 0, cmax
        while c >= 2:
            while n - at >= c:
                lvl.append((c, perm[at:at + c].copy(), rng.choice(np.array([-1, 1], dtype=np.int64), c)))
                at += c
            c //= 2
        out.append(lvl)
    return out


def level_matrix(n, lvl, cmax):
    """cmax x (the orthogonal matrix of one level), in integers: cmax I - (2 cmax / c) v v^T on each group."""
    M = np.zeros((n, n), dtype=np.int64)
    M[np.arange(n), np.arange(n)] = cmax
    for c, pos, sgn in lvl:
        M[np.ix_(pos, pos)] -= (2 * cmax // c) * np.outer(sgn, sgn)
    return M


def q_matrix(n, nlev, cmax, seed):
    """(cmax^nlev Q as int64, nlev log2(cmax)) with Q = H_k ... H_1, the reflections in the order of levels_of."""
    Q = np.zeros((n, n), dtype=np.int64)
    Q[np.arange(n), np.arange(n)] = 1
    for lvl in levels_of(n, nlev, cmax, seed):
        Q = level_matrix(n, lvl, cmax) @ Q
    return Q, nlev * int(np.log2(cmax))


def cmax_for(n, fp32):
    c = 8 if fp32 else 16
    while c > max(n, 1):
        c //= 2
    return c


def exact_dense(ints, q, seed, fp32=False):
    """A = Q diag(ints 2^q) Q^T, built in integers and scaled once by a power of two."""
    n = len(ints)
    cmax = cmax_for(n, fp32)
    if cmax < 2:
        return np.ldexp(np.asarray(ints, dtype=np.float64).reshape(n, n), q)
    Q, sh = q_matrix(n, 2 if fp32 else 3, cmax, seed)
    M = (Q * np.asarray(ints, dtype=np.int64)[None, :]) @ Q.T          # cmax^(2 nlev) A 2^-q; |M| <= 2^(2 sh) max |ints| < 2^53
    assert np.abs(M).max() < (1 << 53)
    return np.ldexp(M.astype(np.float64), q - 2 * sh)


def exact_dense_fraction(ints, q, seed, fp32=False):
    """The same matrix from the definition, H_k ... H_1 diag(spec) H_1 ... H_k one reflection at a time, in fractions.Fraction."""
    F = fractions.Fraction
    n = len(ints)
    A = [[F(0)] * n for _ in range(n)]
    for i in range(n):
        A[i][i] = F(int(ints[i])) * F(2) ** q
    cmax = cmax_for(n, fp32)
    if cmax < 2:
        return A
    for lvl in levels_of(n, 2 if fp32 else 3, cmax, seed):
        for c, pos, sgn in lvl:                     # A <- H A H, H = I - (2 / c) v v^T: only rows / columns `pos` change
            pos, sgn = [int(p) for p in pos], [int(s) for s in sgn]
            for j in range(n):                      # rows: A <- H A
                t = sum(s * A[p][j] for p, s in zip(pos, sgn)) * F(2, c)
                for p, s in zip(pos, sgn):
                    A[p][j] -= s * t
            for i in range(n):                      # columns: A <- A H
                t = sum(s * A[i][p] for p, s in zip(pos, sgn)) * F(2, c)
                for p, s in zip(pos, sgn):
                    A[i][p] -= s * t
    return A


def seed_of(family, n, fp32=False):
    return 1000 * (FAMILIES + ("second_difference", "kac", "blocks", "ones_shift", "J")).index(family) + n + (500000 if fp32 else 0)


def dense_case(family, n, fp32=False):
    ints, q = spectrum(family, n, fp32)
    A = exact_dense(ints, q, seed_of(family, n, fp32), fp32)
    return Case("%s_n%d%s" % (family, n, "_f32" if fp32 else ""), A, np.ldexp(ints.astype(np.float64), q), fp32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# analytic matrices
# ---------------------------------------------------------------------------------------------------------------------------------------
def second_difference(n):
    A = 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    j = np.arange(1, n + 1, dtype=np.longdouble)
    pi = np.arctan(np.longdouble(1)) * 4
    return A, 2 - 2 * np.cos(j * pi / np.longdouble(n + 1))


def kac(n):
    j = np.arange(1, n, dtype=np.float64)
    off = np.sqrt(j * (n - j))
    return np.diag(off, 1) + np.diag(off, -1), (n - 1 - 2 * np.arange(n)).astype(np.float64)


def analytic_case(kind, n, fp32=False):
    if kind == "second_difference":
        A, spec = second_difference(n)
        return Case("second_difference_n%d" % n, A, spec, True)
    if kind == "kac":
        A, spec = kac(n)
        return Case("kac_n%d" % n, A, spec, False)
    if kind == "ones_shift":                        # a = 1 / 4, b = -3: spectrum {-3 (n - 1 times), n / 4 - 3}
        return Case("ones_shift_n%d" % n, np.full((n, n), 0.25) - 3.0 * np.eye(n), np.array([-3.0] * (n - 1) + [n / 4.0 - 3.0]), True)
    if kind == "coupled":                           # [[T, e I], [e I, T]] (+ a 1 x 1 block 2 for odd n), T = tridiag(+1, 2, +1), e = 2^-20
        m, e = n // 2, 2.0 ** -20
        T = 2.0 * np.eye(m) + np.eye(m, k=1) + np.eye(m, k=-1)
        A = 2.0 * np.eye(n)
        A[:m, :m], A[m:2 * m, m:2 * m] = T, T
        A[np.arange(m), m + np.arange(m)] = e
        A[m + np.arange(m), np.arange(m)] = e
        w = second_difference(m)[1]                 # tridiag(+1, 2, +1) = D tridiag(-1, 2, -1) D with D = diag(+-1): the same spectrum
        spec = np.concatenate([w + np.longdouble(e), w - np.longdouble(e), np.full(n - 2 * m, 2.0, dtype=np.longdouble)])
        return Case("coupled_n%d" % n, A, spec, True)
    if kind == "blocks":                            # tridiagonal | dense (| tridiagonal | dense from n = 16 on)
        parts = 4 if n >= 16 else 2
        sizes = [n // parts] * parts
        sizes[-1] += n - sum(sizes)
        A = np.zeros((n, n))
        spec, at = [], 0
        for b, sz in enumerate(sizes):
            if sz == 0:
                continue
            if b % 2 == 0:
                blk, w = second_difference(sz)
            else:
                ints, q = spectrum("straddle", sz, fp32)
                blk, w = exact_dense(ints + 2 * b, q, seed_of("blocks", n, fp32) + b, fp32), (ints + 2 * b).astype(np.float64)
            A[at:at + sz, at:at + sz] = blk
            spec.append(np.asarray(w, dtype=np.longdouble))
            at += sz
        return Case("blocks_n%d%s" % (n, "_f32" if fp32 else ""), A, np.concatenate(spec), True if fp32 else False)
    raise KeyError(kind)


def case(name, n, fp32=False):
    c = dense_case(name, n, fp32) if name in FAMILIES else analytic_case(name, n, fp32)
    if fp32:
        assert c.fp32, name
    return c


F32_ANALYTIC = ("second_difference", "blocks", "ones_shift", "coupled")     # kac's square roots are not fp32 numbers


def all_cases(fp32=False):
    """Every (family | analytic kind) at every size of its precision."""
    for n in (SIZES_F32 if fp32 else SIZES_F64):
        for name in FAMILIES + (F32_ANALYTIC if fp32 else ANALYTIC):
            yield case(name, n, fp32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# J-level input
# ---------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class JCase:
    name: str
    J: np.ndarray          # m_r x n
    s2: np.ndarray         # the n eigenvalues of J^T J (n - m_r zeros when m_r < n)

    @property
    def n(self):
        return self.J.shape[1]

    @property
    def m_r(self):
        return self.J.shape[0]

    def spec(self, lam):
        """Exact spectrum of J^T J + max(lam, 0) I (a NaN lambda acts as 0: `if (lambda > 0)`, nonlinear.cc:187-189)."""
        return self.s2 + (lam if lam > 0 else 0.0)


def j_case(n, m_r, variant=0):
    """s = distinct integers 1 .. (times 1/4); two levels of c <= 8, so every entry of J has at most 5 + 6 bits: exact in float32 too."""
    cmax = cmax_for(n, True)
    Q, sh = q_matrix(n, 2, cmax, seed_of("J", n) + 7919 * variant + m_r)
    s = (np.arange(n, dtype=np.int64) * (3 + variant) % 29) + 1          # integers in 1 .. 29, not sorted
    J = np.ldexp((Q * s[:, None]).astype(np.float64), -2 - sh)           # diag(s / 4) Q
    s2 = (s.astype(np.float64) / 4.0) ** 2
    if m_r <= n:
        J, s2 = J[:m_r], np.concatenate([s2[:m_r], np.zeros(n - m_r)])
    else:
        J = np.concatenate([J, np.zeros((m_r - n, n))])
    return JCase("J_n%d_mr%d_v%d" % (n, m_r, variant), np.ascontiguousarray(J), s2)
