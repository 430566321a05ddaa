"""numpy float64 restatement of the batch-reduced gradients (mo_qp_gradients_shared) for test_shared_grad_cpu and
test_gpu_shared_grad.  Imports neither the product nor the oracle.  Not a test module: nothing here asserts.

V, U: [B, n + 2 m + k] states and adjoints, ok: [B] bool, var: [m] one constraint set, J: [m_r, n] ONE matrix, R: [B, m_r] or [1, m_r]."""
import numpy as np


def split(V, n, k, m):
    return V[:, :n], V[:, n + m:n + m + k], V[:, n + m + k:]     # x, y, z


def direct(n, k, m, var, V, U, ok, J=None, R=None):
    """(value, magnitude): every output as ONE float64 sum over the counted problems, and the same sum with every factor replaced by its
    absolute value -- the sum |a_p| |b_p| of the error bound."""
    sel = np.asarray(ok, dtype=bool)
    var = np.asarray(var, dtype=np.int64)
    x, y, z = (a[sel].astype(np.float64) for a in split(V, n, k, m))
    ux, uy, uz = (a[sel].astype(np.float64) for a in split(U, n, k, m))
    ab = np.abs
    M, Ma = np.einsum("pi,pj->ij", ux, x), np.einsum("pi,pj->ij", ab(ux), ab(x))
    val = {"G": -0.5 * (M + M.T), "c": -ux.sum(0), "A_eq": np.einsum("pi,pj->ij", y, ux) - np.einsum("pi,pj->ij", uy, x), "b_eq": -uy.sum(0),
           "cons_a": (z * ux[:, var] - uz * x[:, var]).sum(0), "cons_b": -uz.sum(0)}
    mag = {"G": 0.5 * (Ma + Ma.T), "c": ab(ux).sum(0), "A_eq": np.einsum("pi,pj->ij", ab(y), ab(ux)) + np.einsum("pi,pj->ij", ab(uy), ab(x)),
           "b_eq": ab(uy).sum(0), "cons_a": (ab(z) * ab(ux[:, var]) + ab(uz) * ab(x[:, var])).sum(0), "cons_b": ab(uz).sum(0)}
    if J is not None:
        J = np.asarray(J, dtype=np.float64)
        Rp = np.broadcast_to(np.asarray(R, dtype=np.float64), (len(V), J.shape[0]))[sel]
        Q, Qa = np.einsum("pq,pj->qj", Rp, ux), np.einsum("pq,pj->qj", ab(Rp), ab(ux))
        val.update(J=-J @ (M + M.T) - Q, r=-J @ ux.sum(0), lam=-np.trace(M))
        mag.update(J=ab(J) @ (Ma + Ma.T) + Qa, r=ab(J) @ ab(ux).sum(0), lam=np.trace(Ma))
    return val, mag


def chunk_len(B, num_cus):
    """Problems per chunk: at least 32, at most one chunk per CU -- a function of (batch, CU count) alone."""
    c = max(1, min(num_cus, (B + 31) // 32))
    return max(1, -(-B // c))


def chunks(B, num_cus):
    return -(-B // chunk_len(B, num_cus))


def chunked(n, k, m, var, V, U, ok, length, J=None, R=None):
    """The kernels' scheme: per chunk of `length` consecutive problems the partial moments M, A1, A2, Q and the column sums, a masked problem's
    rows SELECTED to zero; the partials summed in chunk order; the outputs from the totals."""
    B = len(V)
    ok = np.asarray(ok, dtype=bool)
    var = np.asarray(var, dtype=np.int64)
    zero = lambda a: np.where(ok[:, None], a, 0.0)     # (select: a masked row may hold NaN)
    x, y, z = (zero(a) for a in split(V, n, k, m))
    ux, uy, uz = (zero(a) for a in split(U, n, k, m))
    m_r = 0 if J is None else J.shape[0]
    r_shared = R is not None and len(R) == 1 and B != 1
    Rp = zero(np.broadcast_to(R, (B, m_r))) if R is not None else np.zeros((B, 0))
    tot = dict(M=np.zeros((n, n)), A1=np.zeros((k, n)), A2=np.zeros((k, n)), Q=np.zeros((m_r, n)), su=np.zeros(n), suy=np.zeros(k), suz=np.zeros(m), ca=np.zeros(m))
    for lo in range(0, B, length):
        s = slice(lo, min(lo + length, B))
        part = dict(M=ux[s].T @ x[s], A1=y[s].T @ ux[s], A2=uy[s].T @ x[s], Q=Rp[s].T @ ux[s], su=ux[s].sum(0), suy=uy[s].sum(0),
                    suz=uz[s].sum(0), ca=(z[s] * ux[s][:, var] - uz[s] * x[s][:, var]).sum(0))
        for key in tot:
            tot[key] = tot[key] + part[key]
    M, su = tot["M"], tot["su"]
    out = {"G": -0.5 * (M + M.T), "c": -su, "A_eq": tot["A1"] - tot["A2"], "b_eq": -tot["suy"], "cons_a": tot["ca"], "cons_b": -tot["suz"]}
    if J is not None:
        Q = np.outer(R[0], su) if r_shared else tot["Q"]
        out.update(J=-J @ (M + M.T) - Q, r=-J @ su, lam=-np.trace(M))
    return out


def bound(B, n, unit, mag):
    """2 (B + n + 8) unit sum |a_p| |b_p| per element."""
    return {key: 2.0 * (B + n + 8) * unit * v for key, v in mag.items()}
