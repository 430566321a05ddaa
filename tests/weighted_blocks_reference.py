"""numpy restatement of the residual-block cost with one weight per stacked residual row, 1/2 sum_i w_i (J x + r)_i^2 + 1/2 lam |x|^2
(include/mini_opt_hip.h above mo_linearize_blocks_weighted).  Imports neither the product nor the oracle.  A layout
is [(index tuple, R), ...]; a block's local Jacobian is an R x P array, its residual and its weights are R vectors.

Everything is written PAIR BY PAIR and ROW BY ROW, as the reference's pair rule (residual.hpp:206-224) with one factor per row -- not in the
t / s form the kernels evaluate: the pair q <= p of block b lands once on G_low[max(i, j), min(i, j)] (i = idx[p], j = idx[q]) with
sum_rho w_rho J[rho, p] J[rho, q], so a pair of local columns on one variable counts ONCE.  With the loss gradient of the lower entries,
W[i][j] = -(u_i x_j + x_i u_j) for i != j and W[i][i] = -u_i x_i, every gradient is the pair map transposed:
    dJ[rho, p] = w_rho (sum_q W(p, q) J[rho, q] - u_i r_rho)   with W(p, p) = 2 W[i][i], W(p, q) = W[i][i] for q != p on the same variable
    dr[rho] = -w_rho sum_p u_i J[rho, p]         dw[rho] = sum_{q <= p} W[i][j] J[rho, p] J[rho, q] - sum_p u_i J[rho, p] r_rho
A row whose weight is exactly 0 is never read by linearize and has dJ = dr = exactly 0.

absolute=True returns the same sums over absolute values (every term's magnitude) for error bounds; where the kernels reach a repeated pair
through t and s and take one product back (the correction term), that pair is counted three times."""
import numpy as np

from tests.blocks_diff_reference import pack, split_rows, symmetric, unpack  # noqa: F401  (the packing is that of the unweighted form)


def linearize(n, blocks, Js, rs, ws, lam=0.0, absolute=False):
    """(G_low, c, half_sq): lower triangle only; lam on the diagonal after the sum where > 0."""
    G, c, half = np.zeros((n, n)), np.zeros(n), 0.0
    ab = np.abs if absolute else (lambda z: z)
    for (idx, R), J, r, w in zip(blocks, Js, rs, ws):
        for rho in range(R):
            if w[rho] == 0:
                continue                        # the row's J values and r never enter the arithmetic
            for p in range(len(idx)):
                for q in range(p + 1):
                    i, j = idx[p], idx[q]
                    G[max(i, j), min(i, j)] += ab(w[rho]) * ab(J[rho, p]) * ab(J[rho, q])
                c[idx[p]] += ab(w[rho]) * ab(J[rho, p]) * ab(r[rho])
            half += 0.5 * ab(w[rho]) * r[rho] ** 2
    if lam > 0:
        G[np.arange(n), np.arange(n)] += lam
    return G, c, half


def _pair_weight(i, j, x, ux, absolute):
    if i == j:
        return abs(ux[i] * x[i]) if absolute else -ux[i] * x[i]
    return abs(ux[i] * x[j]) + abs(x[i] * ux[j]) if absolute else -(ux[i] * x[j] + x[i] * ux[j])


def gradients(blocks, Js, rs, ws, x, ux, absolute=False, correction=True):
    """(dJ per block, dr per block, dlambda, dw per block).  correction=False treats a pair of local columns on one variable as the dense
    J^T W J would -- dw = -s t without the pair rule's correction -- and is wrong wherever a block names a variable twice."""
    sgn = 1.0 if absolute else -1.0
    ab = np.abs if absolute else (lambda z: z)
    dJs, drs, dws = [], [], []
    for (idx, R), J, r, w in zip(blocks, Js, rs, ws):
        P = len(idx)
        dJ, dr, dw = np.zeros((R, P)), np.zeros(R), np.zeros(R)
        for rho in range(R):
            for p in range(P):
                i = idx[p]
                for q in range(P):
                    j = idx[q]
                    W = _pair_weight(i, j, x, ux, absolute)
                    if q == p:
                        dJ[rho, p] += 2.0 * W * ab(J[rho, q])
                    else:
                        dJ[rho, p] += W * ab(J[rho, q])
                    if q <= p:
                        mult = 1.0
                        if q < p and i == j:
                            mult = 3.0 if absolute else (1.0 if correction else 2.0)
                        dw[rho] += mult * W * ab(J[rho, p]) * ab(J[rho, q])
                dJ[rho, p] += sgn * ab(ux[i]) * ab(r[rho])
                dr[rho] += sgn * ab(ux[i]) * ab(J[rho, p])
                dw[rho] += sgn * ab(ux[i]) * ab(J[rho, p]) * ab(r[rho])
            if w[rho] == 0:
                dJ[rho], dr[rho] = 0.0, 0.0     # exactly, whatever the row holds
            else:
                dJ[rho] *= ab(w[rho])
                dr[rho] *= ab(w[rho])
        dJs.append(dJ)
        drs.append(dr)
        dws.append(dw)
    return dJs, drs, sgn * float(ab(ux) @ ab(x)), dws


def tangent_rhs(n, blocks, Js, rs, ws, x, tangents, absolute=False):
    """rho_d [n] = Gdot x + cdot + dlam x along `tangents`: {"J_blocks": [R x P per block], "r": [R per block], "weights": [R per block],
    "lam": scalar}; a missing key is a zero tangent.  The directional derivative of linearize, pair by pair and row by row."""
    ab = np.abs if absolute else (lambda z: np.asarray(z, dtype=float))
    x = ab(x)
    rd = np.zeros(n)
    t = tangents
    for b, ((idx, R), J, r, w) in enumerate(zip(blocks, Js, rs, ws)):
        P = len(idx)
        dJ = ab(t["J_blocks"][b]) if "J_blocks" in t else np.zeros((R, P))
        dr = ab(t["r"][b]) if "r" in t else np.zeros(R)
        dw = ab(t["weights"][b]) if "weights" in t else np.zeros(R)
        for rho in range(R):
            if w[rho] == 0 and dw[rho] == 0:
                continue
            wr, Jr, rr = ab(w[rho]), ab(J[rho]), ab(r[rho])
            for p in range(P):
                i = idx[p]
                for q in range(p + 1):
                    j = idx[q]
                    g = dw[rho] * Jr[p] * Jr[q]
                    if w[rho] != 0:
                        g += wr * (dJ[rho, p] * Jr[q] + Jr[p] * dJ[rho, q])
                    if i != j:
                        rd[i] += g * x[j]
                        rd[j] += g * x[i]
                    elif q == p:
                        rd[i] += g * x[i]
                    else:                       # a repeated index: the pair landed once, on the diagonal
                        rd[i] += (3.0 if absolute else 1.0) * g * x[i]
                rd[i] += dw[rho] * Jr[p] * rr
                if w[rho] != 0:
                    rd[i] += wr * (dJ[rho, p] * rr + Jr[p] * dr[rho])
    if "lam" in t:
        rd += ab(t["lam"]) * x
    return rd
