"""numpy restatement of the forward-mode right-hand side for residual-block input (include/mini_opt_hip.h above mo_qp_tangent_rhs_blocks;
DESIGN.md section 4.8, "Forward mode, block input").  Imports neither the product nor the oracle.  A layout is [(index tuple, R), ...], a
block's local Jacobian and its tangent are R x P arrays.

rho is written out PAIR BY PAIR, as the directional derivative of the reference's pair rule (residual.hpp:206-224) -- not in the t / tdot
form the kernel evaluates: the pair q <= p of block b lands once on G_low[max(i, j), min(i, j)] (i = idx[p], j = idx[q]), so its tangent
g = dJ[:, p] . J[:, q] + J[:, p] . dJ[:, q] gives rho_d[i] += g x_j and, where i != j, rho_d[j] += g x_i.  A repeated index inside a block
(i = j with q < p) therefore counts ONCE, which is the correction term of the header.  c[idx[p]] += J[:, p] . r gives
rho_d[idx[p]] += dJ[:, p] . r + J[:, p] . dr, and lambda I gives rho_d += dlam x.  Equality blocks ASSIGN their columns (a repeated index keeps
the last local column): only a winner's tangent reaches rho_pe[row] += dJeq[q, a] x[g] and rho_d[g] -= dJeq[q, a] y[row]; a loser's
entries are never touched and may be NaN.  Constraint rows as tangent_reference.rho.

Tangents: {"J_blocks": [R x P per block], "r": [R per block], "lam": scalar, "J_eq_blocks": [R x P per equality block], "r_eq": (k,),
"a": (m,), "b": (m,)}; a missing key is a zero tangent.

absolute=True returns, per element of rho, the sum of the magnitudes of the terms of the evaluation the header describes (t / tdot form):
the pair sums over absolute values, with a repeated-index pair counted three times -- the kernel adds its two products through t and tdot
and takes one of them back with the correction term."""
import numpy as np


def rho(n, k, m, blocks, Js, rs, v, tangents, eq_blocks=(), var=(), absolute=False):
    fl = np.result_type(np.asarray(v).dtype, np.float64)
    ab = (lambda z: np.abs(np.asarray(z, dtype=fl))) if absolute else (lambda z: np.asarray(z, dtype=fl))
    v = ab(v)
    x, y, z = v[:n], v[n + m:n + m + k], v[n + m + k:]
    t = tangents
    rd = np.zeros(n, dtype=fl)
    if "J_blocks" in t or "r" in t:
        for b, (idx, R) in enumerate(blocks):
            P = len(idx)
            J, r = ab(Js[b]), ab(rs[b])
            dJ = ab(t["J_blocks"][b]) if "J_blocks" in t else np.zeros((R, P), dtype=fl)
            dr = ab(t["r"][b]) if "r" in t else np.zeros(R, dtype=fl)
            for p in range(P):
                i = idx[p]
                for q in range(p + 1):
                    j = idx[q]
                    g = dJ[:, p] @ J[:, q] + J[:, p] @ dJ[:, q]
                    if i != j:
                        rd[i] += g * x[j]
                        rd[j] += g * x[i]
                    elif q == p:
                        rd[i] += g * x[i]
                    else:                       # a repeated index: the pair landed once, on the diagonal
                        rd[i] += (3.0 if absolute else 1.0) * g * x[i]
                rd[i] += dJ[:, p] @ r + J[:, p] @ dr
    if "lam" in t:
        rd += ab(t["lam"]) * x
    pe = np.zeros(k, dtype=fl)
    if k and "J_eq_blocks" in t:
        row = 0
        for b, (idx, R) in enumerate(eq_blocks):
            dJe = t["J_eq_blocks"][b]
            for a, g in enumerate(idx):
                if g in idx[a + 1:]:
                    continue                    # a later local column on the same variable overwrites this one: its tangent reaches nothing
                col = ab(dJe[:, a])
                for q in range(R):
                    pe[row + q] += col[q] * x[g]
                    rd[g] += (1.0 if absolute else -1.0) * col[q] * y[row + q]
            row += R
    if k and "r_eq" in t:
        pe += ab(t["r_eq"])
    pi = np.zeros(m, dtype=fl)
    for i in range(m):
        da = ab(t["a"][i]) if "a" in t else fl.type(0)
        db = ab(t["b"][i]) if "b" in t else fl.type(0)
        if not 0 <= var[i] < n:
            pi[i] = np.nan
            continue
        rd[var[i]] += (1.0 if absolute else -1.0) * da * z[i]    # several rows may name one variable
        pi[i] = da * x[var[i]] + db
    return np.concatenate([rd, np.zeros(m, dtype=fl), pe, pi])


def term_counts(n, k, m, blocks, eq_blocks=(), var=()):
    """Per element of rho, an upper bound on the roundings any term of the kernel's evaluation passes through, doubled, plus 8 (the form of
    bound_factor in tests/test_gpu_blocks_diff.py): a term of rho_d[i] is rounded at most P_b + 1 times inside t or tdot, once as a product,
    twice more in a correction term, and once per addition on its way into rho_d[i], of which there are at most N_i, the number of products
    the element sums: 2 R_b per local column on i, R_b + 1 per partner of a repeated index, R_b per winning equality column, one per
    constraint row on i and one for dlambda x_i.  So fewer than P_max + N_i + 4 roundings: c_i = 2 (P_max + N_i) + 8.  rho_pe[row] sums P_b + 1
    terms: 2 (P_b + 1) + 8; rho_pi one product and one sum: 8; rho_comp is exactly 0."""
    N = np.ones(n)
    Pmax = np.zeros(n)
    for idx, R in blocks:
        for p, i in enumerate(idx):
            partners = sum(1 for q, j in enumerate(idx) if q != p and j == i)
            N[i] += 2 * R + partners * (R + 1)
            Pmax[i] = max(Pmax[i], len(idx))
    for idx, R in eq_blocks:
        for a, g in enumerate(idx):
            if g not in idx[a + 1:]:
                N[g] += R
    for i in range(m):
        if 0 <= var[i] < n:
            N[var[i]] += 1
    pe = np.concatenate([np.full(R, 2.0 * (len(idx) + 1) + 8.0) for idx, R in eq_blocks]) if k else np.zeros(0)
    return np.concatenate([2.0 * (Pmax + N) + 8.0, np.zeros(m), pe, np.full(m, 8.0)])
