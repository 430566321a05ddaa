"""numpy restatement of the right-hand-side mode of the fused fp64 step kernel (csrc/kkt_fused.hip, RHS = true):
the reduced right-hand side, ds, dz and the pre / post scaling of the transposed solve, formula for formula.  Imports neither the
product nor the oracle.  State v = [x | s | y | z], caller's vector rho = [rho_d (n) | rho_comp (m) | rho_pe (k) | rho_pi (m)];
G symmetric, A is k x n."""
import numpy as np

# (n, k, m, m_r) of tests/test_gpu_fused_rhs.py; J_LEVEL[i]: the J-level form of shape i is covered (even n); a shape the issue gives
# without m_r is QP-level only and gets m_r = 2 n here to build G = J^T J + lambda I from
SHAPES = [(20, 0, 0, 24), (20, 3, 10, 22), (31, 15, 62, 40), (32, 16, 40, 64), (33, 31, 66, 66), (64, 8, 32, 128), (64, 24, 100, 130),
          (63, 5, 70, 126), (90, 12, 128, 100), (96, 31, 64, 192), (128, 14, 64, 256), (128, 31, 128, 130), (127, 20, 100, 254),
          (48, 0, 96, 50), (16, 4, 8, 100)]
J_LEVEL = [s[0] % 2 == 0 for s in SHAPES]


def fused_rhs_solve(G, A, var, a, v, rhs, transpose=False, include_inequalities=True):
    """What mo_kkt_solve returns on the fused kernel: delta with K delta = -rhs, or with transpose u with K^T u = rhs."""
    n, k, m = G.shape[0], A.shape[0], len(var)
    var = np.asarray(var, dtype=np.int64)
    s, z = v[n:n + m], v[n + m + k:]
    rho_d, rho_comp, rho_pe, rho_pi = (np.array(t) for t in (rhs[:n], rhs[n:n + m], rhs[n + m:n + m + k], rhs[n + m + k:]))
    if transpose:                                   # rho = [-g_x | -s o g_s | g_y | g_z]
        rho_d, rho_comp = -rho_d, -(s * rho_comp)
    H = np.zeros((n + k, n + k))
    H[:n, :n] = G
    H[:n, n:] = A.T; H[n:, :n] = A
    rhs_x = -rho_d
    if include_inequalities:
        np.add.at(H, (var, var), a * (z / s) * a)                                  # Sigma = a^2 z / s
        np.add.at(rhs_x, var, -(a * (rho_comp + z * rho_pi) / s))
    sol = np.linalg.solve(H, np.concatenate([rhs_x, -rho_pe]))                     # unknowns [dx; -dy]
    dx, dy = sol[:n], -sol[n:]
    ds, dz = np.zeros(m), np.zeros(m)
    if include_inequalities:
        ds = a * dx[var] + rho_pi
        dz = -(rho_comp + z * ds) / s
    if transpose:
        return np.concatenate([dx, ds / s if include_inequalities else ds, -dy, -dz])
    return np.concatenate([dx, ds, dy, dz])
