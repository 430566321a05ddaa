"""numpy float64 restatement of the batch-reduced block gradients under per-row weights (mo_qp_gradients_blocks_weighted_shared; DESIGN.md
section 4.8.10) for test_blocks_weighted_shared_cpu and test_gpu_blocks_weighted_shared.  Imports neither the product nor the oracle.  Not
a test module: nothing here asserts.

cost: a layout [(index tuple, R), ...]; Jv: [values] ONE instance of the packed cost blocks; R, Wt: [B, rows] or [1, rows] (given once);
V, U: [B, n + ...] states and adjoints, whose first n columns are x and u_x; ok: [B] bool.  Every result is a dict of "J_blocks" [values],
"r" [rows], "weights" [rows] and "lam" (a float): the per-problem outputs of mo_qp_gradients_blocks_weighted summed over the counted
problems ("r" / "weights": the gradient of an r / of weights the batch shares).  Written in the t / s form of the header:
    t = J x_loc + r,  s = J u_loc,  a = w t,  c = w s  (both exactly 0 where w == 0)
    dJ[rho, p] = -sum_k (u[i_p] a_rho + x[i_p] c_rho) + (sum of J[rho, q'] over the OTHER local columns q' on p's variable) sum_k w_rho u[i_p] x[i_p]
    dr[rho] = -sum_k c_rho     dw[rho] = -sum_k s_rho t_rho + sum over the pairs {p, p'} on one variable i of J[rho, p] J[rho, p'] sum_k u_i x_i
    dlam = -sum_k sum_i u_i x_i"""
import numpy as np

from tests.blocks_diff_reference import pack, unpack
from tests.blocks_shared_grad_reference import p_max, positions  # noqa: F401
from tests.shared_grad_reference import chunk_len, chunks  # noqa: F401  (the same chunks as the other batch-reduced launches)

STAGE = 16   # problems the kernel stages at a time, at most


def _rows(a, B):
    a = np.asarray(a, dtype=np.float64)
    return np.broadcast_to(a, (B, a.shape[1]))


def _partner_sum(J, idx):
    """D[rho, p] = sum of J[rho, q'] over the other local columns q' on p's variable."""
    ii = np.asarray(idx)
    same = (ii[:, None] == ii[None, :]) & ~np.eye(len(ii), dtype=bool)      # [p, q']
    return J @ same.T.astype(np.float64)


def _pairs(idx):
    return [(p, q) for p in range(len(idx)) for q in range(p) if idx[p] == idx[q]]


def _finish(cost, Js, acc, acc2, csum, stsum, uxsum, partners=True, absolute=False):
    """The outputs from the batch sums: acc[e] = sum (u a + x c), acc2[e] = sum w u x per packed value; csum, stsum per stacked row; uxsum per
    variable.  partners=False drops the second term of dJ and of dw -- wrong wherever a block names a variable twice."""
    sgn = 1.0 if absolute else -1.0
    accs, acc2s = unpack(acc, cost), unpack(acc2, cost)
    dJs, dws, row = [], [], 0
    for b, ((idx, R_), J) in enumerate(zip(cost, Js)):
        dJ = sgn * accs[b]
        dw = sgn * stsum[row:row + R_].copy()
        if partners:
            dJ = dJ + _partner_sum(J, idx) * acc2s[b]
            for p, q in _pairs(idx):
                dw = dw + J[:, p] * J[:, q] * uxsum[idx[p]]
        dJs.append(dJ)
        dws.append(dw)
        row += R_
    return {"J_blocks": pack(dJs), "r": sgn * csum, "weights": np.concatenate(dws), "lam": sgn * float(np.sum(uxsum))}


def _stage_terms(cost, Js, x, ux, R, Wt, absolute=False):
    """Per problem of x [B', n]: a, c, s t [B', rows] and w with the zero rule applied -- the kernel's phase A."""
    a_, c_, st_, row = [], [], [], 0
    with np.errstate(invalid="ignore"):
        for (idx, R_), J in zip(cost, Js):
            ii = np.asarray(idx)
            t = x[:, ii] @ J.T + R[:, row:row + R_]
            s = ux[:, ii] @ J.T
            w = Wt[:, row:row + R_]
            a_.append(np.where(w == 0, 0.0, w * t))
            c_.append(np.where(w == 0, 0.0, w * s))
            st_.append(s * t)
            row += R_
    return np.concatenate(a_, axis=1), np.concatenate(c_, axis=1), np.concatenate(st_, axis=1)


def direct(n, cost, Jv, R, Wt, V, U, ok, absolute=False, partners=True):
    """Section 1 of the formulas over all counted problems at once.  absolute=True: every factor replaced by its absolute value and every
    term added -- the sum |terms| of the error bound (a pair of local columns on one variable is reached twice through t and s and taken
    back once by the partner term: counted three times)."""
    sel = np.asarray(ok, dtype=bool)
    f = np.abs if absolute else (lambda z: z)
    B = len(V)
    Js = [f(J) for J in unpack(np.asarray(Jv, dtype=np.float64), cost)]
    x, ux = f(np.asarray(V, dtype=np.float64)[sel, :n]), f(np.asarray(U, dtype=np.float64)[sel, :n])
    Rp, Wp = f(_rows(R, B)[sel]), f(_rows(Wt, B)[sel])
    a, c, st = _stage_terms(cost, Js, x, ux, Rp, Wp)
    rows, idxs = positions(cost)
    wz = np.where(Wp == 0, 0.0, Wp)
    acc = np.einsum("ke,ke->e", ux[:, idxs], a[:, rows]) + np.einsum("ke,ke->e", x[:, idxs], c[:, rows])
    acc2 = np.einsum("ke,ke->e", wz[:, rows], ux[:, idxs] * x[:, idxs])
    return _finish(cost, Js, acc, acc2, c.sum(0), st.sum(0), (ux * x).sum(0), partners, absolute)


def chunked(n, cost, Jv, R, Wt, V, U, ok, length, stage=STAGE):
    """The kernels' scheme: chunks of `length` consecutive problems; inside a chunk `stage` problems at a time get their a, c (and s t), and
    every packed value, row sum and variable sum is added problem by problem, a masked problem skipped whole; the chunk partials summed in
    chunk order; the outputs formed from the totals through the partner and pair lists."""
    B = len(V)
    ok = np.asarray(ok, dtype=bool)
    Js = unpack(np.asarray(Jv, dtype=np.float64), cost)
    X, UX = np.asarray(V, dtype=np.float64)[:, :n], np.asarray(U, dtype=np.float64)[:, :n]
    Rp, Wp = _rows(R, B), _rows(Wt, B)
    rows, idxs = positions(cost)
    nrows = Rp.shape[1]
    tot = dict(acc=np.zeros(len(rows)), acc2=np.zeros(len(rows)), c=np.zeros(nrows), st=np.zeros(nrows), ux=np.zeros(n))
    for lo in range(0, B, length):
        part = {key: np.zeros_like(v) for key, v in tot.items()}
        hi = min(lo + length, B)
        for p0 in range(lo, hi, stage):
            s = slice(p0, min(p0 + stage, hi))
            live = ok[s]
            if not live.any():
                continue
            x, ux, w = X[s][live], UX[s][live], Wp[s][live]          # (a masked problem's rows are never multiplied)
            a, c, st = _stage_terms(cost, Js, x, ux, Rp[s][live], w)
            for k in range(len(x)):
                part["acc"] += ux[k, idxs] * a[k, rows] + x[k, idxs] * c[k, rows]
                part["acc2"] += np.where(w[k, rows] == 0, 0.0, w[k, rows] * (ux[k, idxs] * x[k, idxs]))
                part["c"] += c[k]
                part["st"] += st[k]
                part["ux"] += ux[k] * x[k]
        for key in tot:
            tot[key] = tot[key] + part[key]
    return _finish(cost, Js, tot["acc"], tot["acc2"], tot["c"], tot["st"], tot["ux"])


def bound(B, pmax, unit, mag):
    """1.01 (2 B + 4 P_max + 8) unit sum |terms| per element, by counting the roundings of the working precision along the longest chain of
    an output element whose exact value is a sum of terms:
      t and s: P_b rounded products and at most P_b + 1 rounded adds each -- "weights" multiplies the two: 4 P_b + 2; the others use one;
      the weight (a = w t), the outer product (u a) and the sum of the two products of a problem: 3;
      a chunk's problems added in working precision, then the chunk totals in double (the working precision itself in fp64): at most
      chunk_len + chunks <= 2 B adds;
      the finish in double and its one rounding: 3.
    (1 + unit)^k - 1 <= 1.01 k unit for every k unit below 0.01.  `mag`: the sum |terms| per element, direct(..., absolute=True)."""
    return {key: 1.01 * (2 * B + 4 * pmax + 8) * unit * np.asarray(v) for key, v in mag.items()}
