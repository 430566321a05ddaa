"""Edge cases of the null-space QP solver (nullspace_kernel in csrc/kkt_generic.hip, mo_nullspace_solve) and their extended-precision referee.
Host only: numpy, scipy (through oracle.nls_oracle) and the standard library, no torch, no GPU, so the CPU suite imports it
(tests/test_nullspace_cases_cpu.py) as well as tests/test_gpu_nullspace_edges.py.

THE REFERENCE.  The KKT system [[sym(G), A^T], [A, 0]] [x; nu] = [-c; -b] solved in numpy.longdouble by Gaussian elimination with partial
pivoting (kkt_solve).  fp32 cases hold inputs that are already rounded to fp32; J-level cases form G = J^T J + max(lambda, 0) I and c = J^T r
in long double.  Rank-deficient cases (family D) carry `keep`, the rows that are independent BY CONSTRUCTION; the others are dropped before
the reference solve.  Family C is solved from its unscaled rows (`A_ref`, `b_ref`): scaling a row and its b by a power of two changes no x.

THE BOUNDS (tests/test_gpu_nullspace_edges.py).  With eps the unit roundoff of the plan's type (2^-52, 2^-23) and every error in long double:
    forward error      |x - x_ref|_inf / |x_ref|_inf                     <= 8 max(E_case, 8 eps)
    backward error     |A x + b|_2 / (|A|_F |x|_2 + |b|_2)               <= 8 max(BE_case, 1 eps)
E_case / BE_case are the worst errors of oracle.nls_oracle.null_space_solve (LAPACK's pivoted QR and Cholesky, fp64) over the case's batch,
as multiples of 2^-52: a property of the reference, never of the kernel.  An fp32 plan is held to the same multiples of 2^-23, the fp64
oracle run on the fp32-rounded inputs providing them: the error of a backward-stable method scales with the unit roundoff.  The factor 8
covers another, equally stable summation order (wave butterflies against LAPACK's loops).  tests/test_nullspace_cases_cpu.py asserts the
condition the bound rests on: E_case <= 64 eps on every SUCCESS problem of families A - E and G (family F's margin case has a reduced
Hessian of condition 2^20, where the oracle's own error sets the bound).

THE FAMILIES (each case a batch of B <= 16 problems, n <= 128, with a seed of its own; cond(G) <= 100 unless stated).
  A  rows dominated by one entry: row q has +-(1 - q / 2k) at column q and uniform(-1, 1) 2^-s elsewhere, s in {24, 30, 36} (fp32: {10, 13,
     16}), so pivoting leaves the dominant entry on the diagonal and the Householder tail is 2^-s of the pivot: a tail whose square is
     below eps of the pivot's.  Shapes (8, 1), (8, 3), (40, 8) (64 threads, n + k = 48), (41, 8) (256 threads), (70, 5).  "late": row 0 is
     an ordinary row of norm > 2 supported away from columns 1 .. k - 1, so only the columns j >= 1 have the small tail.
  B  rows +-2^e e_i in shuffled order.  In the first half of the batch the j-th largest row sits on axis j: exactly zero tails, every
     column takes the tau = 0 branch with beta = c0 keeping its sign, after pivot swaps (problems 0 and 1 have ascending rows), and x at
     the constrained indices is -b / a EXACTLY (exact_idx, exact_val).  The second half has the rows on random axes: the reflectors are
     signed swaps (c0 = 0, tau = 1) whose rank-one application rounds t_j + w when two of them meet in one entry -- as Eigen's does --,
     so those problems are held to the reference alone.
  C  random full-rank rows scaled (with their b) by 2^e, e spread over -20 .. 20 (fp32: -6 .. 6, see C_SPREAD): a non-trivial pivot order,
     the solution of the unscaled rows.  "negligible_rows": two of four rows are 2^-70 of the others, 2^-20 of the rank threshold but not
     zero: rank 2 with two reflectors BEYOND the rank, which the reduced Hessian has to take in full; the reference drops those rows.
  D  exact rank deficiency, dependent in any arithmetic: axis rows only with a repeated axis (ranks 1 and k - 1), random rows with an
     all-zero row first / in the middle / last (rank k - 1), k = 1 with A = 0 (rank 0).  The pivot loop's early exit at j = 0 and j > 0.
  E  shape edges, random full-rank data: n = k = 1; k = n; k = n - 1; k = 1 at n = 63, 64, 65; (127, 9); (128, 16) given (G, c) and given
     (J, r, lambda) with m_r = 130; (128, 24), the last k the LDS takes at n = 128 in fp64 (CAPACITY_K: (n | 1)(n + k) + 5 n + 4 k + 16
     doubles and 8 flags within 160 KiB).
  F  termination decisions with a margin: G = Q diag(d) Q^T, the rows of A from Q^T, so the reduced Hessian's spectrum is the rest of d.
     Smallest reduced eigenvalue +2^-20 |G| -> SUCCESS, -2^-20 |G| -> NOT_POSITIVE_DEFINITE; G = diag(1, 0, 2), A = e_0 -> a pivot that
     is exactly 0 -> NOT_POSITIVE_DEFINITE.
  G  J-level input: a per-problem lambda with a 0 and a negative entry (lambda > 0 gates the term), and column-major J.
Families A, B, C and E run as fp64 and as fp32 plans, the others as fp64."""
import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np
import scipy.linalg

from oracle import nls_oracle as N

LD = np.longdouble
EPS64 = 2.0 ** -52
EPS32 = 2.0 ** -23
EPS_LD = float(np.finfo(LD).eps)
SUCCESS, NOT_POSITIVE_DEFINITE = 0, 1
FACTOR = 8.0                 # another equally stable summation order
FWD_FLOOR, BE_FLOOR = 8.0, 1.0   # eps: the floors of the two bounds
ORACLE_FWD_MAX = 64.0        # eps: the condition the forward bound rests on (families A - E, G)
LDS_BYTES = 160 * 1024


def capacity_k(n):
    """The largest k whose (G, c) problem the null-space kernel keeps in LDS in fp64, by include/mini_opt_hip.h's rule."""
    k = 0
    while 8 * ((n | 1) * (n + k + 1) + 5 * n + 4 * (k + 1) + 16) + 32 <= LDS_BYTES:
        k += 1
    return k


CAPACITY_N = 128
CAPACITY_K = capacity_k(CAPACITY_N)


@dataclass
class Case:
    name: str
    family: str
    dtype: str                       # "f64" | "f32": the plan's type; every array below already holds values of that type
    seed: int
    A: np.ndarray                    # [B, k, n]
    b: np.ndarray                    # [B, k]
    term: np.ndarray                 # [B] expected termination
    G: Optional[np.ndarray] = None   # [B, n, n] symmetric        (G, c) input
    c: Optional[np.ndarray] = None   # [B, n]
    J: Optional[np.ndarray] = None   # [B, m_r, n]                (J, r, lambda) input
    r: Optional[np.ndarray] = None   # [B, m_r]
    lam: Optional[np.ndarray] = None     # [B]
    J_layout: str = "row"
    keep: Optional[np.ndarray] = None    # [B, k] bool: the rows the solve keeps (family D: the independent ones; C negligible_rows)
    rank: Optional[np.ndarray] = None    # [B] constructed rank (default k)
    dom: Optional[np.ndarray] = None     # [B, k] |dominant entry| expected as |R_jj| (NaN: an ordinary column) (family A)
    exact_idx: Optional[np.ndarray] = None   # [B / 2, k] the constrained index of row q of the first B / 2 problems and
    exact_val: Optional[np.ndarray] = None   # [B / 2, k] its exact x (family B)
    A_ref: Optional[np.ndarray] = None   # the unscaled rows (family C)
    b_ref: Optional[np.ndarray] = None

    @property
    def B(self):
        return self.A.shape[0]

    @property
    def n(self):
        return self.A.shape[2]

    @property
    def k(self):
        return self.A.shape[1]

    @property
    def m_r(self):
        return 0 if self.J is None else self.J.shape[1]

    @property
    def eps(self):
        return EPS64 if self.dtype == "f64" else EPS32

    def hessian(self, p):
        """(sym(G), c) of problem p in long double."""
        if self.J is None:
            return self.G[p].astype(LD), self.c[p].astype(LD)
        J, r = self.J[p].astype(LD), self.r[p].astype(LD)
        G = ld_matmul(J.T, J) + max(float(self.lam[p]), 0.0) * np.eye(self.n, dtype=LD)
        return (G + G.T) / 2, ld_matmul(J.T, r[:, None])[:, 0]


def ld_matmul(a, b):
    return (a[:, :, None] * b[None, :, :]).sum(axis=1)


def kkt_solve(G, c, A, b):
    """[[G, A^T], [A, 0]] [x; nu] = [-c; -b] in long double, Gaussian elimination with partial pivoting.  Returns (x, residual / scale) with
    residual = |K z - rhs|_inf and scale = |K|_inf |z|_inf + |rhs|_inf."""
    n, k = G.shape[0], A.shape[0]
    K = np.zeros((n + k, n + k), dtype=LD)
    K[:n, :n] = G; K[:n, n:] = A.T; K[n:, :n] = A
    rhs = np.concatenate([-c, -b]).astype(LD)
    U, y, P = K.copy(), rhs.copy(), n + k
    for j in range(P):
        piv = j + int(np.argmax(np.abs(U[j:, j])))
        if piv != j:
            U[[j, piv]] = U[[piv, j]]; y[[j, piv]] = y[[piv, j]]
        l = U[j + 1:, j] / U[j, j]
        U[j + 1:, j:] -= l[:, None] * U[j, j:][None, :]
        y[j + 1:] -= l * y[j]
    z = np.zeros(P, dtype=LD)
    for j in range(P - 1, -1, -1):
        z[j] = (y[j] - (U[j, j + 1:] * z[j + 1:]).sum()) / U[j, j]
    res = np.abs((K * z[None, :]).sum(axis=1) - rhs).max()
    scale = np.abs(K).sum(axis=1).max() * np.abs(z).max() + np.abs(rhs).max()
    return z[:n], float(res / scale)


def forward_error(x, x_ref):
    """|x - x_ref|_inf / |x_ref|_inf in long double."""
    x_ref = np.asarray(x_ref, dtype=LD)
    return float(np.abs(np.asarray(x, dtype=LD) - x_ref).max() / np.abs(x_ref).max())


def backward_error(A, b, x):
    """|A x + b|_2 / (|A|_F |x|_2 + |b|_2) in long double (0 for 0 / 0: A = 0 with b = 0)."""
    A, b, x = np.asarray(A, dtype=LD), np.asarray(b, dtype=LD), np.asarray(x, dtype=LD)
    res = np.sqrt((((A * x[None, :]).sum(axis=1) + b) ** 2).sum())
    den = np.sqrt((A ** 2).sum()) * np.sqrt((x ** 2).sum()) + np.sqrt((b ** 2).sum())
    return float(res / den) if den > 0 else float(res)


# ---- builders ---------------------------------------------------------------------------------------------------------------------------
def _round(a, dtype):
    return a if dtype == "f64" else a.astype(np.float32).astype(np.float64)


def _spd(rng, B, n, cond=100.0):
    """Q diag(d) Q^T with d log-spaced over [1, cond], symmetric to the bit."""
    G = np.empty((B, n, n))
    for p in range(B):
        Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
        d = np.logspace(0.0, np.log10(cond), n) if n > 1 else np.array([2.0])
        M = (Q * d[None, :]) @ Q.T
        G[p] = (M + M.T) / 2
    return G


def _gc(rng, B, n, dtype, cond=100.0):
    return _round(_spd(rng, B, n, cond), dtype), _round(rng.uniform(-1, 1, (B, n)), dtype)     # (entrywise rounding keeps G symmetric)


def _ok(B):
    return np.full(B, SUCCESS, dtype=np.int64)


def _family_a(n, k, dtype, seed, late=False):
    rng = np.random.default_rng(seed)
    shifts = (24, 30, 36) if dtype == "f64" else (10, 13, 16)
    B = 12
    G, c = _gc(rng, B, n, dtype)
    A = np.empty((B, k, n)); dom = np.empty((B, k))
    for p in range(B):
        A[p] = rng.uniform(-1, 1, (k, n)) * 2.0 ** -shifts[p % 3]
        for q in range(k):
            dom[p, q] = 1.0 - q / (2.0 * k)
            A[p, q, q] = dom[p, q] * rng.choice([-1.0, 1.0])
        if late:
            A[p, 0, :] = rng.uniform(-1, 1, n); A[p, 0, 1:k] = 0.0; A[p, 0, 0] = 2.0
            dom[p, 0] = np.nan
    name = f"A_{'late_' if late else ''}n{n}_k{k}_{dtype}"
    return Case(name, "A", dtype, seed, _round(A, dtype), _round(rng.uniform(-1, 1, (B, k)), dtype), _ok(B), G=G, c=c, dom=_round(dom, dtype))


def _family_b(n, k, dtype, seed):
    rng = np.random.default_rng(seed)
    B = 8
    G, c = _gc(rng, B, n, dtype)
    A = np.zeros((B, k, n)); b = _round(rng.uniform(-1, 1, (B, k)), dtype)
    idx = np.empty((B, k), dtype=np.int64); val = np.empty((B, k))
    for p in range(B):
        mag = 2.0 ** rng.permutation(np.arange(-8, 9))[:k]           # distinct powers of two: no tie in the pivot search
        axes = rng.permutation(n)[:k]
        if p < B // 2:
            if p < 2:
                mag = np.sort(mag)                                   # ascending rows: the pivot search has to swap
            axes[np.argsort(-mag)] = np.arange(k)                    # the j-th largest row on axis j: tau = 0 in every column
        sign = rng.choice([-1.0, 1.0], k)
        for q in range(k):
            A[p, q, axes[q]] = sign[q] * mag[q]
            idx[p, q] = axes[q]; val[p, q] = -b[p, q] / A[p, q, axes[q]]   # a power of two divides exactly
    exact = np.arange(B) < B // 2
    return Case(f"B_n{n}_k{k}_{dtype}", "B", dtype, seed, A, b, _ok(B), G=G, c=c, exact_idx=idx[exact], exact_val=val[exact])


def _family_c(n, k, dtype, seed):
    rng = np.random.default_rng(seed)
    B = 6
    G, c = _gc(rng, B, n, dtype)
    A0 = _round(rng.uniform(-1, 1, (B, k, n)), dtype); b0 = _round(rng.uniform(-1, 1, (B, k)), dtype)
    e = np.stack([rng.permutation(np.round(np.linspace(-C_SPREAD[dtype], C_SPREAD[dtype], k))) for _ in range(B)])
    s = 2.0 ** e
    return Case(f"C_n{n}_k{k}_{dtype}", "C", dtype, seed, A0 * s[:, :, None], b0 * s, _ok(B), G=G, c=c, A_ref=A0, b_ref=b0)


def _family_c_negligible():
    """Two ordinary rows and two rows that are 2^-70 of them (with their b): NOT zero, so they get reflectors of their own, but 2^-20 of the
    rank threshold |R|_max eps min(n, k), so the rank is 2 by a wide margin and the solve is that of the two ordinary rows."""
    rng = np.random.default_rng(350)
    B, n, k = 6, 10, 4
    G, c = _gc(rng, B, n, "f64")
    A = rng.uniform(-1, 1, (B, k, n)); b = rng.uniform(-1, 1, (B, k)); keep = np.ones((B, k), dtype=bool)
    for p in range(B):
        small = rng.permutation(k)[:2]
        A[p, small] *= 2.0 ** -70; b[p, small] *= 2.0 ** -70; keep[p, small] = False
    return Case("C_negligible_rows_n10_k4", "C", "f64", 350, A, b, _ok(B), G=G, c=c, keep=keep, rank=np.full(B, 2))


def _family_d():
    out = []
    # axis rows only, every row on ONE axis: rank 1, the pivot loop ends at j = 1
    rng = np.random.default_rng(401)
    B, n, k = 4, 8, 3
    G, c = _gc(rng, B, n, "f64")
    A = np.zeros((B, k, n)); b = np.zeros((B, k)); keep = np.zeros((B, k), dtype=bool)
    for p in range(B):
        axis, t = int(rng.integers(0, n)), rng.uniform(-1, 1)
        a = rng.choice([-1.0, 1.0], k) * 2.0 ** rng.permutation(np.arange(-3, 4))[:k]
        A[p, :, axis] = a; b[p] = -a * t; keep[p, 0] = True
    out.append(Case("D_one_axis_n8_k3", "D", "f64", 401, A, b, _ok(B), G=G, c=c, keep=keep, rank=np.full(B, 1)))
    # axis rows on k - 1 axes, one axis twice: rank k - 1
    rng = np.random.default_rng(402)
    B, n, k = 4, 9, 4
    G, c = _gc(rng, B, n, "f64")
    A = np.zeros((B, k, n)); b = np.zeros((B, k)); keep = np.ones((B, k), dtype=bool)
    for p in range(B):
        axes = rng.permutation(n)[:k - 1]
        rows = rng.permutation(k)                                    # rows[0], rows[1] share axes[0]
        a = rng.choice([-1.0, 1.0], k) * 2.0 ** rng.permutation(np.arange(-4, 5))[:k]
        t = rng.uniform(-1, 1, k - 1)
        for i, q in enumerate(rows):
            ax = 0 if i == 0 else i - 1
            A[p, q, axes[ax]] = a[q]; b[p, q] = -a[q] * t[ax]
        keep[p, rows[1]] = False
    out.append(Case("D_repeated_axis_n9_k4", "D", "f64", 402, A, b, _ok(B), G=G, c=c, keep=keep, rank=np.full(B, k - 1)))
    # random rows and an all-zero row at the first, a middle and the last position: rank k - 1
    rng = np.random.default_rng(403)
    B, n, k = 6, 10, 4
    G, c = _gc(rng, B, n, "f64")
    A = rng.uniform(-1, 1, (B, k, n)); b = rng.uniform(-1, 1, (B, k)); keep = np.ones((B, k), dtype=bool)
    for p in range(B):
        q = (0, k // 2, k - 1)[p % 3]
        A[p, q] = 0.0; b[p, q] = 0.0; keep[p, q] = False
    out.append(Case("D_zero_row_n10_k4", "D", "f64", 403, A, b, _ok(B), G=G, c=c, keep=keep, rank=np.full(B, k - 1)))
    # k = 1, A = 0: rank 0, the pivot loop ends at j = 0, x = -G^-1 c
    rng = np.random.default_rng(404)
    B, n, k = 4, 5, 1
    G, c = _gc(rng, B, n, "f64")
    out.append(Case("D_zero_A_n5_k1", "D", "f64", 404, np.zeros((B, k, n)), np.zeros((B, k)), _ok(B), G=G, c=c,
                    keep=np.zeros((B, k), dtype=bool), rank=np.zeros(B, dtype=np.int64)))
    return out


def _family_e(n, k, dtype, seed, m_r=0):
    rng = np.random.default_rng(seed)
    B = 8 if n <= 16 else 4
    A = _round(rng.uniform(-1, 1, (B, k, n)), dtype); b = _round(rng.uniform(-1, 1, (B, k)), dtype)
    if m_r:
        # J^T J of a nearly square uniform J is ill-conditioned by itself: lambda = 2 keeps cond(G) below 100
        return Case(f"E_n{n}_k{k}_J{m_r}_{dtype}", "E", dtype, seed, A, b, _ok(B), J=_round(rng.uniform(-1, 1, (B, m_r, n)), dtype),
                    r=_round(rng.uniform(-1, 1, (B, m_r)), dtype), lam=np.full(B, 2.0))
    G, c = _gc(rng, B, n, dtype)
    return Case(f"E_n{n}_k{k}_{dtype}", "E", dtype, seed, A, b, _ok(B), G=G, c=c)


def _family_f():
    out = []
    n, k, B = 10, 3, 8
    for tag, sgn, seed in (("pos", 1.0, 601), ("neg", -1.0, 602)):
        rng = np.random.default_rng(seed)
        G = np.empty((B, n, n)); A = np.empty((B, k, n))
        for p in range(B):
            Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
            d = np.concatenate([rng.uniform(0.5, 1.0, k), [sgn * 2.0 ** -20, 1.0], rng.uniform(0.25, 1.0, n - k - 2)])   # |G| = 1
            M = (Q * d[None, :]) @ Q.T
            G[p] = (M + M.T) / 2
            A[p] = Q[:, :k].T
        term = _ok(B) if sgn > 0 else np.full(B, NOT_POSITIVE_DEFINITE, dtype=np.int64)
        out.append(Case(f"F_margin_{tag}_n{n}_k{k}", "F", "f64", seed, A, rng.uniform(-1, 1, (B, k)), term, G=G, c=rng.uniform(-1, 1, (B, n))))
    out.append(Case("F_semidefinite_n3_k1", "F", "f64", 603, np.array([[[1.0, 0.0, 0.0]]]), np.array([[-0.5]]),
                    np.array([NOT_POSITIVE_DEFINITE]), G=np.diag([1.0, 0.0, 2.0])[None], c=np.array([[1.0, -4.0, 6.0]])))
    return out


def _family_g():
    out = []
    for tag, seed, layout in (("lambda_vec", 701, "row"), ("colmajor", 702, "col")):
        rng = np.random.default_rng(seed)
        B, n, k, m_r = 6, 12, 3, 20
        lam = np.array([0.0, -0.5, 0.25, 1.0, 0.0, 0.125]) if layout == "row" else np.full(B, 0.25)
        out.append(Case(f"G_{tag}_n{n}_k{k}", "G", "f64", seed, rng.uniform(-1, 1, (B, k, n)), rng.uniform(-1, 1, (B, k)), _ok(B),
                        J=rng.uniform(-1, 1, (B, m_r, n)), r=rng.uniform(-1, 1, (B, m_r)), lam=lam, J_layout=layout))
    return out


A_SHAPES = ((8, 1), (8, 3), (40, 8), (41, 8), (70, 5))
B_SHAPES = ((8, 3), (41, 8))
C_SHAPES = ((12, 5), (60, 10))
# Row scales 2^-e .. 2^e.  The solver's rank rule (Eigen's) drops a row whose |R_jj| is below |R|_max eps min(n, k): a spread of 2^40 is
# 2^12 inside that rule in fp64 and 2^17 BEYOND it in fp32 (eps = 2^-23), where the unit row would sit on the threshold itself.  fp32
# plans take the spread 2^-6 .. 2^6, which leaves every row more than RANK_MARGIN above the fp32 threshold (asserted on the CPU).
C_SPREAD = {"f64": 20, "f32": 6}
RANK_MARGIN = 16.0
E_SHAPES = ((1, 1), (6, 6), (7, 6), (63, 1), (64, 1), (65, 1), (127, 9), (128, 16))
E_SEEDS = {(6, 6, "f64"): 533}   # x = -A^-1 b there: seed 501 draws an A_eq of condition 505 (oracle error 480 eps), 533 stays below 80


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for t, dtype in enumerate(("f64", "f32")):
        out += [_family_a(n, k, dtype, 100 + 20 * t + i) for i, (n, k) in enumerate(A_SHAPES)]
        out.append(_family_a(8, 3, dtype, 110 + 20 * t, late=True))
        out += [_family_b(n, k, dtype, 200 + 20 * t + i) for i, (n, k) in enumerate(B_SHAPES)]
        out += [_family_c(n, k, dtype, 300 + 20 * t + i) for i, (n, k) in enumerate(C_SHAPES)]
        out += [_family_e(n, k, dtype, E_SEEDS.get((n, k, dtype), 500 + 20 * t + i)) for i, (n, k) in enumerate(E_SHAPES)]
        out.append(_family_e(128, 16, dtype, 510 + 20 * t, m_r=130))
    out.append(_family_e(CAPACITY_N, CAPACITY_K, "f64", 550))
    out.append(_family_c_negligible())
    out += _family_d() + _family_f() + _family_g()
    assert len({c.name for c in out}) == len(out) and all(c.B <= 16 and c.n <= 128 for c in out)
    return tuple(out)


def names():
    return [c.name for c in cases()]


def by_name(name):
    return {c.name: c for c in cases()}[name]


CAPACITY_CASE = f"E_n{CAPACITY_N}_k{CAPACITY_K}_f64"


# ---- the reference and the oracle's own errors -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(name):
    """(x_ref [B, n] long double, NaN rows for NOT_POSITIVE_DEFINITE problems; KKT residual / scale [B])."""
    case = by_name(name)
    x = np.full((case.B, case.n), np.nan, dtype=LD); res = np.zeros(case.B)
    A, b = (case.A, case.b) if case.A_ref is None else (case.A_ref, case.b_ref)
    for p in range(case.B):
        if case.term[p] != SUCCESS:
            continue
        G, c = case.hessian(p)
        rows = slice(None) if case.keep is None else case.keep[p]
        x[p], res[p] = kkt_solve(G, c, A[p][rows].astype(LD), b[p][rows].astype(LD))
    x.setflags(write=False)
    return x, res


def pivoted_qr(A):
    """The oracle's QR of A^T: (|diag R|, rank by Eigen's default threshold, pivot order), as oracle.nls_oracle.null_space_solve takes them."""
    k, n = A.shape
    R, P = scipy.linalg.qr(A.T, mode="r", pivoting=True)
    diag = np.abs(np.diag(R[:k, :k]))
    return diag, int(np.sum(diag > diag.max() * min(n, k) * np.finfo(float).eps)), P


@dataclass
class OracleErrors:
    term: np.ndarray      # [B] the oracle's termination
    fwd: np.ndarray       # [B] forward error / 2^-52 (NaN where the problem is not a SUCCESS)
    be: np.ndarray        # [B] constraint backward error / 2^-52
    E_case: float         # the worst of fwd
    BE_case: float        # the worst of be


@functools.lru_cache(maxsize=None)
def oracle_errors(name):
    case = by_name(name)
    x_ref, _ = reference(name)
    term = np.empty(case.B, dtype=np.int64); fwd = np.full(case.B, np.nan); be = np.full(case.B, np.nan)
    for p in range(case.B):
        G, c = case.hessian(p)
        ok, x = N.null_space_solve(N.QPData(np.tril(G.astype(np.float64)), c.astype(np.float64), case.A[p], case.b[p], []))
        term[p] = SUCCESS if ok else NOT_POSITIVE_DEFINITE
        if ok and case.term[p] == SUCCESS:
            fwd[p] = forward_error(x, x_ref[p]) / EPS64
            be[p] = backward_error(case.A[p], case.b[p], x) / EPS64
    good = np.isfinite(fwd)
    return OracleErrors(term, fwd, be, float(fwd[good].max()) if good.any() else 0.0, float(be[good].max()) if good.any() else 0.0)


def forward_bound(name):
    """8 max(E_case, 8 eps), in units of the plan's eps."""
    return FACTOR * max(oracle_errors(name).E_case, FWD_FLOOR)


def backward_bound(name):
    return FACTOR * max(oracle_errors(name).BE_case, BE_FLOOR)
