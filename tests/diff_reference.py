"""numpy restatement of the differentiable-QP mathematics (include/mini_opt_hip.h above mo_kkt_solve).
Imports neither the product nor the oracle: dense K, LU solves, and every gradient formula written out.

State v = [x (n) | s (m) | y (k) | z (m)], residual F(v; theta) = [r_d | r_comp - mu | r_pe | r_pi] (qp.cc:391-420):
    r_d = G x + c - A^T y - C^T z     r_comp = s o z     r_pe = A x + b_eq     r_pi = C x + b - s,     C[i, var_i] = a_i
G is used as a symmetric matrix (pass sym(G)); A is k x n in mathematical orientation."""
import numpy as np


def cons_matrix(n, var, a):
    C = np.zeros((len(var), n))
    C[np.arange(len(var)), np.asarray(var, dtype=np.int64)] = a
    return C


def split(v, n, k, m):
    return v[:n], v[n:n + m], v[n + m:n + m + k], v[n + m + k:]


def residual(G, c, A, b_eq, var, a, b, v, mu=0.0):
    n, k, m = len(c), len(b_eq), len(var)
    x, s, y, z = split(v, n, k, m)
    C = cons_matrix(n, var, a)
    return np.concatenate([G @ x + c - A.T @ y - C.T @ z, s * z - mu, A @ x + b_eq, C @ x + b - s])


def kkt_matrix(G, A, var, a, v):
    """K = dF/dv, the matrix of BuildFullSystem."""
    n, k, m = G.shape[0], A.shape[0], len(var)
    _, s, _, z = split(v, n, k, m)
    C = cons_matrix(n, var, a)
    K = np.zeros((n + 2 * m + k, n + 2 * m + k))
    xs, ss, ys, zs = slice(0, n), slice(n, n + m), slice(n + m, n + m + k), slice(n + m + k, n + 2 * m + k)
    K[xs, xs] = G; K[xs, ys] = -A.T; K[xs, zs] = -C.T
    K[ss, ss] = np.diag(z); K[ss, zs] = np.diag(s)
    K[ys, xs] = A
    K[zs, xs] = C; K[zs, ss] = -np.eye(m)
    return K


def solve_direct(K, rhs):
    """delta with K delta = -rhs."""
    return np.linalg.solve(K, -rhs)


def solve_transposed(K, g):
    """u with K^T u = g, by LU on the full matrix."""
    return np.linalg.solve(K.T, g)


def transposed_through_direct(K, g, n, k, m, s):
    """The same u from a DIRECT solve: rho = [-g_x | -s o g_s | g_y | g_z], K delta = -rho, u = [delta_x | delta_s / s | -delta_y | -delta_z]."""
    gx, gs, gy, gz = split(g, n, k, m)
    d = solve_direct(K, np.concatenate([-gx, -s * gs, gy, gz]))
    dx, ds, dy, dz = split(d, n, k, m)
    return np.concatenate([dx, ds / s, -dy, -dz])


def transposed_through_reduced(G, A, var, a, v, g):
    """u from the reduced system H = G + C^T S^-1 Z C the kernels factorise (SolveForUpdate, qp.cc:318-364, r_ := rho, mu = 0), numpy's LU on
    the (n + k) system instead of the LDL^T."""
    n, k, m = G.shape[0], A.shape[0], len(var)
    _, s, _, z = split(v, n, k, m)
    gx, gs, gy, gz = split(g, n, k, m)
    r_d, r_comp, r_pe, r_pi = -gx, -s * gs, gy, gz
    C = cons_matrix(n, var, a)
    H = np.zeros((n + k, n + k))
    H[:n, :n] = G + C.T @ np.diag(z / s) @ C
    H[n:, :n] = A; H[:n, n:] = A.T
    rhs = -np.concatenate([r_d + C.T @ ((z / s) * r_pi) + C.T @ (r_comp / s), r_pe])
    sol = np.linalg.solve(H, rhs)
    dx, dy = sol[:n], -sol[n:]
    ds = C @ dx + r_pi
    dz = -(z / s) * ds - r_comp / s
    return np.concatenate([dx, ds / s, -dy, -dz])


def gradients(n, k, m, var, v, u, J=None, r=None):
    """Every gradient formula, from the state v and the adjoint u = K^-T g."""
    x, _, y, z = split(v, n, k, m)
    ux, _, uy, uz = split(u, n, k, m)
    var = np.asarray(var, dtype=np.int64)
    out = {
        "c": -ux,
        "G": -0.5 * (np.outer(ux, x) + np.outer(x, ux)),
        "A_eq": np.outer(y, ux) - np.outer(uy, x),          # k x n
        "b_eq": -uy,
        "cons_a": z * ux[var] - uz * x[var],
        "cons_b": -uz,
    }
    if J is not None:
        t, w = J @ ux, J @ x + r
        out["J"] = -np.outer(t, x) - np.outer(w, ux)         # m_r x n
        out["r"] = -t
        out["lam"] = -float(ux @ x)
    return out
