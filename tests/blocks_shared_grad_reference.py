"""numpy float64 restatement of the batch-reduced block gradients (mo_qp_gradients_blocks_shared) for
test_blocks_shared_grad_cpu and test_gpu_blocks_shared_grad.  Imports neither the product nor the oracle.  Not a test module: nothing here
asserts.

cost, eq: layouts [(index tuple, R), ...] (eq may be None); Jv: [values] ONE instance of the packed cost blocks; R: [B, rows] or [1, rows];
V, U: [B, n + 2 m + k] states and adjoints; ok: [B] bool.  Every result is a dict of "J_blocks" [values], "r" [rows], "lam" (a float) and,
with an eq layout, "J_eq_blocks" [eq values], "r_eq" [k] -- "r" is the per-problem dr summed, the gradient of an r the batch shares."""
import numpy as np

from tests import blocks_diff_reference as BR
from tests.shared_grad_reference import chunk_len, chunks  # noqa: F401  (the same chunks as the dense form)


def _xy(V, n, k, m):
    return V[:, :n], V[:, n + m:n + m + k]


def direct(n, k, m, cost, eq, Jv, R, V, U, ok, absolute=False):
    """The sum over the counted problems of blocks_diff_reference.gradients_blocks / gradients_eq_blocks.  absolute=True: the same sum with
    every factor replaced by its absolute value -- the sum |a| |b| of the error bound."""
    Js = BR.unpack(np.asarray(Jv, dtype=np.float64), cost)
    Rp = np.broadcast_to(np.asarray(R, dtype=np.float64), (len(V), np.shape(R)[1]))
    x, y = _xy(np.asarray(V, dtype=np.float64), n, k, m)
    ux, uy = _xy(np.asarray(U, dtype=np.float64), n, k, m)
    out = {"J_blocks": 0.0, "r": 0.0, "lam": 0.0}
    if eq is not None:
        out.update(J_eq_blocks=0.0, r_eq=0.0)
    for p in np.flatnonzero(np.asarray(ok, dtype=bool)):
        dJs, drs, dlam = BR.gradients_blocks(cost, Js, BR.split_rows(Rp[p], cost), x[p], ux[p], absolute=absolute)
        out["J_blocks"] = out["J_blocks"] + BR.pack(dJs)
        out["r"] = out["r"] + np.concatenate(drs)
        out["lam"] = out["lam"] + dlam
        if eq is not None:
            dJe, dre = BR.gradients_eq_blocks(eq, x[p], ux[p], y[p], uy[p], absolute=absolute)
            out["J_eq_blocks"] = out["J_eq_blocks"] + BR.pack(dJe)
            out["r_eq"] = out["r_eq"] + dre
    return out


def direct_batched(n, k, m, cost, eq, Jv, R, V, U, ok, absolute=False):
    """`direct` for batches too large for its Python loop over the problems: the same sums, block by block over all counted problems at
    once (float64 matrix products of the block's LOCAL vectors; no n x n moment is formed)."""
    sel = np.asarray(ok, dtype=bool)
    f = np.abs if absolute else (lambda a: a)
    sgn = 1.0 if absolute else -1.0
    Js = [f(J) for J in BR.unpack(np.asarray(Jv, dtype=np.float64), cost)]
    Rp = f(np.broadcast_to(np.asarray(R, dtype=np.float64), (len(V), np.shape(R)[1]))[sel])
    x, y = (f(a[sel]) for a in _xy(np.asarray(V, dtype=np.float64), n, k, m))
    ux, uy = (f(a[sel]) for a in _xy(np.asarray(U, dtype=np.float64), n, k, m))
    dJs, drs, row = [], [], 0
    for (idx, R_), J in zip(cost, Js):
        ii = np.asarray(idx)
        xl, ul = x[:, ii], ux[:, ii]
        W = ul.T @ xl + xl.T @ ul                                  # w_b(p, q) summed, but ...
        same = (ii[:, None] == ii[None, :]) & ~np.eye(len(ii), dtype=bool)
        W = np.where(same, (ul * xl).sum(0)[:, None], W)           # ... u_i x_i once for q != p on the same variable
        dJs.append(sgn * (J @ W.T + Rp[:, row:row + R_].T @ ul))
        drs.append(sgn * (J @ ul.sum(0)))
        row += R_
    out = {"J_blocks": BR.pack(dJs), "r": np.concatenate(drs), "lam": sgn * float(np.sum(ux * x))}
    if eq is not None:
        dJe, row = [], 0
        for idx, R_ in eq:
            d = np.zeros((R_, len(idx)))
            for a, g in enumerate(idx):
                if g not in idx[a + 1:]:
                    yu, ux_ = y[:, row:row + R_].T @ ux[:, g], uy[:, row:row + R_].T @ x[:, g]
                    d[:, a] = yu + ux_ if absolute else yu - ux_
            dJe.append(d)
            row += R_
        out.update(J_eq_blocks=BR.pack(dJe), r_eq=uy.sum(0) if absolute else -uy.sum(0))
    return out


def positions(blocks):
    """Per packed value, in the packing's order (block by block, column-major inside a block): (stacked row, global index)."""
    rows, idxs, row = [], [], 0
    for idx, R_ in blocks:
        for g in idx:
            rows.extend(range(row, row + R_))
            idxs.extend([g] * R_)
        row += R_
    return np.asarray(rows, dtype=np.int64), np.asarray(idxs, dtype=np.int64)


def from_moments(cost, eq, Jv, M, su, A1=None, A2=None, suy=None, Qp=None, r=None):
    """Every output from the totals: M = sum u_x x^T, su = sum u_x, A1 = sum y u_x^T, A2 = sum u_y x^T, suy = sum u_y and EITHER the packed
    Qp[e] = sum r[row_e] u_x[index_e] (an r per problem) OR the one r the batch shares."""
    Js = BR.unpack(np.asarray(Jv, dtype=np.float64), cost)
    S = M + M.T
    Qs = BR.unpack(Qp, cost) if Qp is not None else None
    dJs, drs, row = [], [], 0
    for b, ((idx, R_), J) in enumerate(zip(cost, Js)):
        P = len(idx)
        dJ = np.zeros((R_, P))
        dr = np.zeros(R_)
        for p in range(P):
            i = idx[p]
            for pp in range(P):
                dJ[:, p] -= J[:, pp] * S[i, idx[pp]]
            dJ[:, p] -= Qs[b][:, p] if Qs is not None else r[row:row + R_] * su[i]
            for q in range(P):
                if q != p and idx[q] == i:           # the repeated-index rule
                    dJ[:, p] += M[i, i] * J[:, q]
            dr -= su[i] * J[:, p]
        dJs.append(dJ)
        drs.append(dr)
        row += R_
    out = {"J_blocks": BR.pack(dJs), "r": np.concatenate(drs), "lam": -float(np.trace(M))}
    if eq is not None:
        dA = A1 - A2
        dJe, row = [], 0
        for idx, R_ in eq:
            d = np.zeros((R_, len(idx)))
            for a, g in enumerate(idx):
                if g not in idx[a + 1:]:              # local column a wins its global column
                    d[:, a] = dA[row:row + R_, g]
            dJe.append(d)
            row += R_
        out.update(J_eq_blocks=BR.pack(dJe), r_eq=-suy)
    return out


def chunked(n, k, m, cost, eq, Jv, R, V, U, ok, length):
    """The kernels' scheme: per chunk of `length` consecutive problems the partial moments, the column sums and the packed Q, a masked
    problem's rows SELECTED to zero; the partials summed in chunk order; the outputs from the totals.  A shared r forms no Q."""
    B = len(V)
    ok = np.asarray(ok, dtype=bool)
    zero = lambda a: np.where(ok[:, None], a, 0.0)     # (select: a masked row may hold NaN)
    x, y = (zero(a) for a in _xy(np.asarray(V, dtype=np.float64), n, k, m))
    ux, uy = (zero(a) for a in _xy(np.asarray(U, dtype=np.float64), n, k, m))
    R = np.asarray(R, dtype=np.float64)
    r_shared = len(R) == 1 and B != 1
    rows, idxs = positions(cost)
    Rp = zero(np.broadcast_to(R, (B, R.shape[1])))
    tot = dict(M=np.zeros((n, n)), A1=np.zeros((k, n)), A2=np.zeros((k, n)), su=np.zeros(n), suy=np.zeros(k), Q=np.zeros(len(rows)))
    for lo in range(0, B, length):
        s = slice(lo, min(lo + length, B))
        part = dict(M=ux[s].T @ x[s], A1=y[s].T @ ux[s], A2=uy[s].T @ x[s], su=ux[s].sum(0), suy=uy[s].sum(0),
                    Q=(Rp[s][:, rows] * ux[s][:, idxs]).sum(0))
        for key in tot:
            tot[key] = tot[key] + part[key]
    return from_moments(cost, eq, Jv, tot["M"], tot["su"], tot["A1"], tot["A2"], tot["suy"],
                        Qp=None if r_shared else tot["Q"], r=R[0] if r_shared else None)


def p_max(*layouts):
    return max(len(idx) for blocks in layouts if blocks is not None for idx, _ in blocks)


def bound(B, pmax, unit, mag):
    """2 (B + 3 P_max + 8) unit sum |a| |b| per element: an element is formed from at most 3 P_b + 1 totals, each a sum of B rounded
    products."""
    return {key: 2.0 * (B + 3 * pmax + 8) * unit * np.asarray(v) for key, v in mag.items()}
