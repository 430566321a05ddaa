"""numpy restatement of residual-block input and of its gradients (include/mini_opt_hip.h above mo_qp_gradients_blocks).
Imports neither the product nor the oracle.  A layout is [(index tuple, R), ...]; a block's local Jacobian is an R x P array.

Forward (residual.hpp:186-250): per block and local pair q <= p, G_low[max(i, j), min(i, j)] += J[:, p] . J[:, q]; c[idx[p]] += J[:, p] . r;
lambda on the diagonal after the sum where > 0.  Equality blocks ASSIGN their columns: a repeated index keeps the last local column.
Backward: every gradient written out pair by pair with the weights w_b(p, q) of the header -- not the t / w form the kernel evaluates."""
import numpy as np


def pack(Js):
    """R x P blocks -> the packed values of one problem: each block column-major, in block order."""
    return np.concatenate([np.asarray(J).T.reshape(-1) for J in Js])


def unpack(values, blocks):
    out, off = [], 0
    for idx, R in blocks:
        P = len(idx)
        out.append(np.asarray(values[off:off + R * P]).reshape(P, R).T.copy())
        off += R * P
    return out


def split_rows(r, blocks):
    out, off = [], 0
    for _, R in blocks:
        out.append(np.asarray(r[off:off + R]))
        off += R
    return out


def linearize(n, blocks, Js, rs, lam=0.0):
    """(G_low, c): the reference's pair rule, lower triangle only."""
    G = np.zeros((n, n))
    c = np.zeros(n)
    for (idx, _), J, r in zip(blocks, Js, rs):
        for p in range(len(idx)):
            for q in range(p + 1):
                i, j = idx[p], idx[q]
                G[max(i, j), min(i, j)] += J[:, p] @ J[:, q]
            c[idx[p]] += J[:, p] @ r
    if lam > 0:
        G[np.arange(n), np.arange(n)] += lam
    return G, c


def symmetric(G_low):
    return G_low + G_low.T - np.diag(np.diag(G_low))


def jacobian(n, blocks, Js):
    """The stacked (sum R) x n matrix of UpdateJacobian: columns assigned in local order."""
    A = np.zeros((sum(R for _, R in blocks), n))
    row = 0
    for (idx, R), J in zip(blocks, Js):
        for a, g in enumerate(idx):
            A[row:row + R, g] = J[:, a]
        row += R
    return A


def gradients_blocks(blocks, Js, rs, x, ux, absolute=False):
    """(dJ per block, dr per block, dlambda).  absolute=True: the same sums over absolute values (every term's magnitude), for error bounds."""
    sgn = 1.0 if absolute else -1.0
    if absolute:
        Js, rs, x, ux = [np.abs(J) for J in Js], [np.abs(r) for r in rs], np.abs(x), np.abs(ux)
    dJs, drs = [], []
    for (idx, R), J, r in zip(blocks, Js, rs):
        P = len(idx)
        dJ = np.zeros((R, P))
        dr = np.zeros(R)
        for p in range(P):
            i = idx[p]
            for q in range(P):
                j = idx[q]
                if q == p:
                    w = sgn * 2.0 * ux[i] * x[i]
                elif j == i:
                    w = sgn * ux[i] * x[i]
                else:
                    w = sgn * (ux[i] * x[j] + x[i] * ux[j])
                dJ[:, p] += w * J[:, q]
            dJ[:, p] += sgn * ux[i] * r
            dr += sgn * ux[i] * J[:, p]
        dJs.append(dJ)
        drs.append(dr)
    return dJs, drs, sgn * float(ux @ x)


def gradients_eq_blocks(blocks, x, ux, y, uy, absolute=False):
    """(dJeq per block, dr_eq): dA_eq = y u_x^T - u_y x^T gathered at the columns that win their global column, exactly 0 elsewhere."""
    if absolute:
        x, ux, y, uy = np.abs(x), np.abs(ux), np.abs(y), np.abs(uy)
    dJs, row = [], 0
    for idx, R in blocks:
        dJ = np.zeros((R, len(idx)))
        for a, g in enumerate(idx):
            if g in idx[a + 1:]:
                continue                    # a later local column on the same variable overwrites this one
            for q in range(R):
                dJ[q, a] = y[row + q] * ux[g] + uy[row + q] * x[g] if absolute else y[row + q] * ux[g] - uy[row + q] * x[g]
        dJs.append(dJ)
        row += R
    return dJs, (np.abs(uy) if absolute else -np.asarray(uy))
