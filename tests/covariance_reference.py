"""Reference of the parameter covariance (mo_qp_covariance, csrc/qp_covariance.hip) and the case table of its tests.  Host only: numpy and the
standard library, no torch, no GPU: tests/test_covariance_cpu.py imports it as well as tests/test_gpu_covariance.py.

THE TRUTH.  numpy.longdouble throughout, hand-written loops (as tests/nullspace_cases.py): Householder QR of A^T with column pivoting, the rank
by the device's rule |R_jj| > |R|_max eps min(n, k) with the PLAN's eps, Z = the last n - rank columns of Q, Cholesky of Z^T S Z with
S = sym(G) from the lower triangle, C = Z L^-T L^-1 Z^T.  A rank-deficient case carries `keep`, the rows that are independent by
construction: the truth is formed from those rows alone.
THE RESTATEMENT.  Plain numpy in the plan's dtype: np.linalg.qr(A^T, 'complete'), np.linalg.cholesky, a triangular solve.
THE ERROR.  |C - C_truth|_max / |C_truth|_max per problem; E_case = the restatement's worst over the case's batch.
THE BOUND ON THE DEVICE (the project's own, tests/test_gpu_nullspace_edges.py):  error <= 8 max(E_case, 8 eps), eps = 2^-52 / 2^-23.  An fp32
case holds fp32-rounded inputs.  A case whose truth is 0 (rank n) is compared for exact equality."""
import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np

LD = np.longdouble
EPS = {"f64": 2.0 ** -52, "f32": 2.0 ** -23}
NP = {"f64": np.float64, "f32": np.float32}
FACTOR, FLOOR = 8.0, 8.0
WELL_CONDITIONED_MAX = 64.0      # eps: what the restatement keeps on the well-conditioned families (test_covariance_cpu)
LDS_BYTES = 160 * 1024
OK, NONFINITE, BAD_INDEX, NOT_POSITIVE_DEFINITE = 0, 3, 4, 5


def lds_bytes(n, k, q, elem):
    """The capacity rule of include/mini_opt_hip.h: ((n | 1) (n + k) + 2 n + 2 k) scalars + 4 (q + 8) bytes, rounded up to 16."""
    return (((n | 1) * (n + k) + 2 * n + 2 * k) * elem + 4 * (q + 8) + 15) & ~15


def capacity_n(k, elem=8):
    """The largest n the rule admits at q = n."""
    n = 1
    while lds_bytes(n + 1, k, n + 1, elem) <= LDS_BYTES:
        n += 1
    return n


def threads(n, k):
    return 64 if n + k <= 48 else 256


def workgroups_per_cu(n, k, q, elem):
    """The launcher's per-CU ceiling (qp_covariance_grid)."""
    return max(1, min(LDS_BYTES // lds_bytes(n, k, q, elem), 32 // (threads(n, k) // 64)))


def sym_lower(G):
    L = np.tril(np.asarray(G))
    return L + np.tril(L, -1).swapaxes(-1, -2)


def ld_matmul(a, b):
    return (a[:, :, None] * b[None, :, :]).sum(axis=1)


# ---- the truth --------------------------------------------------------------------------------------------------------------------------
def householder_nullspace(A, eps):
    """(Z [n, n - rank], rank) of A [k, n] in long double: pivoted Householder QR of A^T, rank by |R_jj| > |R|_max eps min(n, k)."""
    A = np.asarray(A, dtype=LD)
    k, n = A.shape
    M = A.T.copy()
    Q = np.eye(n, dtype=LD)
    diag = []
    for j in range(min(n, k)):
        norms = (M[j:, j:] ** 2).sum(axis=0)
        piv = j + int(np.argmax(norms))
        if norms[piv - j] == 0:
            break
        M[:, [j, piv]] = M[:, [piv, j]]
        x = M[j:, j].copy()
        tail = (x[1:] ** 2).sum()
        if tail == 0:
            diag.append(abs(x[0]))
            continue
        beta = -np.sqrt(x[0] ** 2 + tail) if x[0] >= 0 else np.sqrt(x[0] ** 2 + tail)
        v = x.copy(); v[0] = x[0] - beta
        v = v / np.sqrt((v ** 2).sum())
        M[j:, j:] -= 2 * v[:, None] * (v[None, :] @ M[j:, j:])
        Q[:, j:] -= 2 * (Q[:, j:] @ v[:, None]) * v[None, :]
        diag.append(abs(beta))
    diag = np.array(diag, dtype=LD)
    rank = int(np.sum(diag > diag.max() * LD(eps) * min(n, k))) if len(diag) else 0
    return Q[:, rank:], rank


def cholesky_ld(H):
    """Lower Cholesky factor in long double; None if a pivot is <= 0."""
    n = H.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = H[j, j] - (L[j, :j] ** 2).sum()
        if not d > 0:
            return None
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (H[j + 1:, j] - (L[j + 1:, :j] * L[j, :j][None, :]).sum(axis=1)) / L[j, j]
    return L


def lower_inverse_ld(L):
    n = L.shape[0]
    X = np.zeros((n, n), dtype=LD)
    for j in range(n):
        X[j, j] = 1 / L[j, j]
        for i in range(j + 1, n):
            X[i, j] = -(L[i, j:i] * X[j:i, j]).sum() / L[i, i]
    return X


def truth(G, A=None, eps=EPS["f64"]):
    """C [n, n] in long double, or None if the reduced Hessian has a pivot <= 0.  G: any array whose lower triangle holds S; A [k, n] or None."""
    S = sym_lower(np.asarray(G, dtype=LD))
    n = S.shape[0]
    if A is None or A.shape[0] == 0:
        Z = np.eye(n, dtype=LD)
    else:
        Z, _ = householder_nullspace(A, eps)
    if Z.shape[1] == 0:
        return np.zeros((n, n), dtype=LD)
    H = ld_matmul(ld_matmul(Z.T, S), Z)
    L = cholesky_ld((H + H.T) / 2)
    if L is None:
        return None
    W = ld_matmul(Z, lower_inverse_ld(L).T)          # Z L^-T
    C = ld_matmul(W, W.T)
    return (C + C.T) / 2


def kkt_inverse_block(G, A):
    """The top-left n x n block of the inverse of [[S, A^T], [A, 0]] by Gauss-Jordan elimination with partial pivoting in long double."""
    S = sym_lower(np.asarray(G, dtype=LD))
    n, k = S.shape[0], A.shape[0]
    P = n + k
    K = np.zeros((P, 2 * P), dtype=LD)
    K[:n, :n] = S; K[:n, n:P] = A.T; K[n:P, :n] = A
    K[:, P:] = np.eye(P, dtype=LD)
    for j in range(P):
        piv = j + int(np.argmax(np.abs(K[j:, j])))
        if piv != j:
            K[[j, piv]] = K[[piv, j]]
        K[j] = K[j] / K[j, j]
        for i in range(P):
            if i != j:
                K[i] = K[i] - K[i, j] * K[j]
    return K[:n, P:P + n]


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def restatement(G, A, dtype):
    """The same quantity in plain numpy of the plan's dtype: complete QR of A^T (A of full row rank), Cholesky, a triangular solve."""
    t = NP[dtype]
    S = sym_lower(np.asarray(G, dtype=t))
    n = S.shape[0]
    if A is None or A.shape[0] == 0:
        Z = np.eye(n, dtype=t)
    else:
        Z = np.linalg.qr(np.asarray(A, dtype=t).T, "complete")[0][:, A.shape[0]:]
    if Z.shape[1] == 0:
        return np.zeros((n, n), dtype=t)
    L = np.linalg.cholesky(Z.T @ S @ Z)
    W = np.linalg.solve(L, Z.T)                       # (a triangular system)
    return (W.T @ W).astype(t)


def error(C, C_truth):
    """|C - C_truth|_max / |C_truth|_max in long double."""
    C_truth = np.asarray(C_truth, dtype=LD)
    return float(np.abs(np.asarray(C, dtype=LD) - C_truth).max() / np.abs(C_truth).max())


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    dtype: str                        # "f64" | "f32": every array holds values of that type
    G: np.ndarray                     # [B, n, n] symmetric
    A: Optional[np.ndarray] = None    # [B, k, n]
    keep: Optional[np.ndarray] = None     # [B, k] bool: the independent rows (rank-deficient cases)
    well_conditioned: bool = False

    @property
    def B(self):
        return self.G.shape[0]

    @property
    def n(self):
        return self.G.shape[1]

    @property
    def k(self):
        return 0 if self.A is None else self.A.shape[1]

    @property
    def eps(self):
        return EPS[self.dtype]

    def rows(self, p):
        """The rows of problem p the truth is formed from."""
        if self.A is None:
            return None
        return self.A[p] if self.keep is None else self.A[p][self.keep[p]]


def _round(a, dtype):
    return a if dtype == "f64" else a.astype(np.float32).astype(np.float64)


def _jtj(rng, B, m_r, n, dtype):
    J = rng.standard_normal((B, m_r, n))
    G = np.einsum("bqi,bqj->bij", J, J)
    return _round((G + G.transpose(0, 2, 1)) / 2, dtype)


def _spd(rng, B, n, cond):
    G = np.empty((B, n, n))
    for p in range(B):
        Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
        M = (Q * np.logspace(0.0, np.log10(cond), n)[None, :]) @ Q.T
        G[p] = (M + M.T) / 2
    return G


K0_SIZES = (1, 2, 15, 16, 17, 33, 64, 65)
EQ_SHAPES = ((2, 1), (7, 3), (17, 16), (33, 5), (64, 8), (96, 16))
EQ_SHAPES_F32 = ((7, 3), (33, 5), (64, 8))
FULL_RANK_SHAPES = ((3, 3), (16, 16))
DEFICIENT_SHAPES = ((7, 3), (33, 5))
SINGULAR_SHAPES = ((7, 5, 3), (12, 9, 4))     # (n, m_r, k): G = J^T J of rank m_r < n, m_r + k >= n
CAPACITY_K = 16
CAPACITY_N = capacity_n(CAPACITY_K)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for t, dtype in enumerate(("f64", "f32")):
        for i, n in enumerate(K0_SIZES):
            rng = np.random.default_rng(1000 + 100 * t + i)
            out.append(Case(f"k0_n{n}_{dtype}", dtype, _jtj(rng, 5, 2 * n, n, dtype), well_conditioned=True))
    out.append(Case("k0_cond1e6_n17_f64", "f64", _spd(np.random.default_rng(1300), 5, 17, 1e6)))
    for dtype, shapes, seed in (("f64", EQ_SHAPES, 1400), ("f32", EQ_SHAPES_F32, 1500)):
        for i, (n, k) in enumerate(shapes):
            rng = np.random.default_rng(seed + i)
            out.append(Case(f"eq_n{n}_k{k}_{dtype}", dtype, _jtj(rng, 5, 2 * n, n, dtype), _round(rng.uniform(-1, 1, (5, k, n)), dtype),
                            well_conditioned=n <= 33))
    rng = np.random.default_rng(1600)
    out.append(Case(f"eq_capacity_n{CAPACITY_N}_k{CAPACITY_K}_f64", "f64", _jtj(rng, 2, 2 * CAPACITY_N, CAPACITY_N, "f64"),
                    rng.uniform(-1, 1, (2, CAPACITY_K, CAPACITY_N))))
    for i, (n, k) in enumerate(FULL_RANK_SHAPES):
        rng = np.random.default_rng(1700 + i)
        out.append(Case(f"full_rank_n{n}_k{k}_f64", "f64", _jtj(rng, 5, 2 * n, n, "f64"), rng.uniform(-1, 1, (5, k, n))))
    for i, (n, k) in enumerate(DEFICIENT_SHAPES):
        rng = np.random.default_rng(1800 + i)
        B = 6
        A = rng.uniform(-1, 1, (B, k, n)); keep = np.ones((B, k), dtype=bool)
        for p in range(B):
            q = (0, k // 2, k - 1)[p % 3]
            if p < 3:
                # a duplicated row.  Two equal columns of A^T stay equal to the bit until one of them is the pivot; what the reflector
                # leaves of the other is rounding noise of a few eps of ITS norm, so a third row 16 times as long puts that noise a factor
                # 16 / k-ish below the rank threshold |R|_max eps min(n, k) instead of on it
                A[p, q] = A[p, (q + 1) % k]
                A[p, (q + 2) % k] *= 16.0
            else:
                A[p, q] = 0.0                        # a zero row
            keep[p, q] = False
        out.append(Case(f"deficient_n{n}_k{k}_f64", "f64", _jtj(rng, B, 2 * n, n, "f64"), A, keep=keep, well_conditioned=True))
    # the rank-deficient matrices of tests/nullspace_cases.py (families C and D)
    from tests import nullspace_cases as NC
    for name in ("C_negligible_rows_n10_k4", "D_one_axis_n8_k3", "D_repeated_axis_n9_k4", "D_zero_row_n10_k4", "D_zero_A_n5_k1"):
        c = NC.by_name(name)
        out.append(Case("nullspace_" + name, "f64", c.G, c.A, keep=c.keep, well_conditioned=True))
    for i, (n, m_r, k) in enumerate(SINGULAR_SHAPES):
        rng = np.random.default_rng(1900 + i)
        out.append(Case(f"singular_G_n{n}_mr{m_r}_k{k}_f64", "f64", _jtj(rng, 5, m_r, n, "f64"), rng.uniform(-1, 1, (5, k, n))))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def names():
    return [c.name for c in cases()]


def by_name(name):
    return {c.name: c for c in cases()}[name]


@functools.lru_cache(maxsize=None)
def reference(name):
    """C_truth [B, n, n] long double of a case (read-only)."""
    case = by_name(name)
    C = np.stack([truth(case.G[p], case.rows(p), case.eps) for p in range(case.B)])
    C.setflags(write=False)
    return C


@functools.lru_cache(maxsize=None)
def restatement_errors(name):
    """[B] errors of the restatement (0 where the truth is 0 and the restatement too)."""
    case = by_name(name)
    Ct = reference(name)
    out = np.zeros(case.B)
    for p in range(case.B):
        R = restatement(case.G[p], case.rows(p), case.dtype)
        out[p] = 0.0 if not Ct[p].any() and not R.any() else error(R, Ct[p])
    return out


def bound(name):
    """8 max(E_case, 8 eps) as an absolute relative error."""
    return FACTOR * max(float(restatement_errors(name).max()), FLOOR * by_name(name).eps)
