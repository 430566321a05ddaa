"""numpy restatement of the forward-mode mathematics of a QP solve (include/mini_opt_hip.h above mo_qp_tangent_rhs).
Imports neither the product nor the oracle.  From F(v*(theta); theta) = 0 follows K vdot = -rho with rho = F_theta thetadot:
    (G, c):   rho_d = sym(dG) x + dc - dA^T y - sum_i da_i z_i e_{var_i}
    J-level:  rho_d = dJ^T w + J^T tdot + dlam x - dA^T y - sum_i da_i z_i e_{var_i},   w = J x + r,  tdot = dJ x + dr
    rho_comp = 0      rho_pe = dA x + db_eq      rho_pi[i] = da_i x[var_i] + db_i
Tangents are a dict in mathematical orientation: "G" n x n (only its LOWER triangle is read), "c", "A" k x n, "b_eq", "a", "b", "J" m_r x n,
"r", "lam" (a scalar); a missing key is a zero tangent."""
import numpy as np

from tests import diff_reference as R


def sym_lower(dG):
    """The symmetric matrix whose lower triangle is that of dG."""
    low = np.tril(dG)
    return low + np.tril(dG, -1).T


def rho(n, k, m, var, v, tangents, J=None, r=None):
    x, _, y, z = R.split(v, n, k, m)
    var = np.asarray(var, dtype=np.int64)
    t = tangents
    rd = np.zeros(n)
    if J is None:
        if "G" in t:
            rd = rd + sym_lower(np.where(np.tril(np.ones((n, n), dtype=bool)), t["G"], 0.0)) @ x
        if "c" in t:
            rd = rd + t["c"]
    else:
        dJ = t.get("J", np.zeros_like(J))
        w = J @ x + r
        tdot = dJ @ x + t.get("r", np.zeros(J.shape[0]))
        rd = rd + dJ.T @ w + J.T @ tdot + float(t.get("lam", 0.0)) * x
    pe = np.zeros(k)
    if k:
        if "A" in t:
            rd = rd - t["A"].T @ y
            pe = pe + t["A"] @ x
        if "b_eq" in t:
            pe = pe + t["b_eq"]
    pi = np.zeros(m)
    if m:
        if "a" in t:
            np.subtract.at(rd, var, t["a"] * z)     # several rows may name one variable
            pi = pi + t["a"] * x[var]
        if "b" in t:
            pi = pi + t["b"]
    return np.concatenate([rd, np.zeros(m), pe, pi])


def vdot(G, A, var, a, v, rho_):
    """vdot with K vdot = -rho, by LU on the full K (G as a symmetric matrix, A k x n)."""
    return np.linalg.solve(R.kkt_matrix(G, A, var, a, v), -rho_)


def vdot_reduced(G, A, var, a, v, rho_):
    """The same vdot from the reduced system H = G + C^T S^-1 Z C the kernels factorise (SolveForUpdate, qp.cc:318-364, r_ := rho, mu = 0),
    numpy's LU on the (n + k) system."""
    n, k, m = G.shape[0], A.shape[0], len(var)
    _, s, _, z = R.split(v, n, k, m)
    r_d, r_comp, r_pe, r_pi = R.split(rho_, n, k, m)
    C = R.cons_matrix(n, var, a)
    H = np.zeros((n + k, n + k))
    H[:n, :n] = G + C.T @ np.diag(z / s) @ C
    H[n:, :n] = A; H[:n, n:] = A.T
    rhs = -np.concatenate([r_d + C.T @ ((z / s) * r_pi) + C.T @ (r_comp / s), r_pe])
    sol = np.linalg.solve(H, rhs)
    dx, dy = sol[:n], -sol[n:]
    ds = C @ dx + r_pi
    dz = -(z / s) * ds - r_comp / s
    return np.concatenate([dx, ds, dy, dz])
