"""What the tests of the sensitivity layer share (test_gpu_diff, test_gpu_tangent, test_gpu_blocks_diff, test_gpu_blocks_tangent,
test_gpu_shared_grad, test_gpu_blocks_shared_grad, test_gpu_fused_rhs, test_gpu_layouts, test_gpu_second_problem): problems, layouts, solve
parameters, the oracle's KKT solves, plans and guarded buffers.  Not a test module: nothing here asserts."""
import ctypes as C

import numpy as np
import torch

from mini_opt_amd import _lib as L
from mini_opt_amd import qp as Q
from mini_opt_amd import synth
from oracle import oracle as orc

DEV = "cuda:0"
UNIT = {torch.float64: 2.0 ** -53, torch.float32: 2.0 ** -24}
PARAMS = dict(initial_mu=1.0, sigma=0.1, termination_kkt_tol=1e-9, termination_complementarity_tol=1e-9, max_iterations=30)


def dev():
    return torch.device(DEV)


def T(a, dt=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev()).contiguous()


def rel_inf_rows(got, ref):
    return np.max(np.abs(got - ref), axis=1) / np.max(np.abs(ref), axis=1)


def cus():
    return torch.cuda.get_device_properties(dev()).multi_processor_count


def expand(t, B):
    return t.detach().expand(B, *t.shape[1:]).contiguous()


def ragged_batch(chunks):
    """4 chunks(4096) + 1: more than one chunk, a chunk length that is no multiple of four, a shorter last chunk.  `chunks`: the chunk count
    of (batch, CUs) of the launch under test (shared_grad_reference.chunks, blocks_shared_grad_reference.chunks)."""
    return 4 * chunks(4096, cus()) + 1


class Plan:
    """A plan of a test's own (mo_plan_create / mo_plan_destroy): plan flags the cached plans of mini_opt_amd.diff do not have, calls whose
    Python mirror makes a plan per call.  dtype: a torch dtype or MO_F64 / MO_F32; the handle is `.h`."""

    def __init__(self, n, k, m, m_r, dtype, batch, flags=0):
        desc = L.PlanDesc(n, k, m, m_r, Q._DT.get(dtype, dtype), 0, flags | L.EXTRA_PLAN_FLAGS, 0, int(batch))
        self.h = C.c_void_p()
        L.check(L.lib().mo_plan_create(C.byref(desc), C.byref(self.h)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        L.lib().mo_plan_destroy(self.h)


CANARY = 777.0


class Guarded:
    """`count` elements starting `off` elements into a buffer filled with the canary: a base off 16 bytes when off is odd."""

    def __init__(self, count, dt, off=1):
        self.buf = torch.full((off + count + 64,), CANARY, dtype=dt, device=dev())
        self.view = self.buf[off:off + count]
        self.off, self.count = off, count

    def intact(self):
        return bool(torch.all(self.buf[:self.off] == CANARY)) and bool(torch.all(self.buf[self.off + self.count:] == CANARY))


# ---- dense problems ----------------------------------------------------------------------------------------------------------------------------
def host_batch(n, k, m, m_r, B, stream, f32=False):
    """Interior states from mini_opt_amd.synth; an odd m drops the last constraint of the next even one."""
    mm = m + (m & 1)
    hb = synth.make_batch(n, k, mm, m_r, B, stream=stream)
    if mm != m:
        keep = np.r_[0:n + m, n + mm:n + mm + k + m]
        hb.vars = np.ascontiguousarray(hb.vars[:, keep])
        hb.cons_var, hb.cons_a, hb.cons_b = (np.ascontiguousarray(a[:, :m]) for a in (hb.cons_var, hb.cons_a, hb.cons_b))
        hb.m = m
    if f32:
        for key in ("J", "r", "A_eq", "b_eq", "cons_a", "cons_b", "vars", "mu"):
            setattr(hb, key, getattr(hb, key).astype(np.float32).astype(np.float64))
        hb.lam = float(np.float32(hb.lam))
    hb.G = np.einsum("bqi,bqj->bij", hb.J, hb.J) + hb.lam * np.eye(n)
    hb.c = np.einsum("bqi,bq->bi", hb.J, hb.r)
    return hb


def padded(a, ld, fill=0.0):
    """[B, rows, cols] -> [B, rows, ld] with `fill` beyond cols."""
    out = np.full(a.shape[:2] + (ld,), fill)
    out[:, :, :a.shape[2]] = a
    return out


def device_problem(hb, level, dt=torch.float64, J_layout="row", J_ld=None):
    kw = dict(n=hb.n, k=hb.k, m=hb.m)
    if hb.k:
        kw.update(A_eq=T(hb.A_eq, dt), b_eq=T(hb.b_eq, dt))
    if hb.m:
        kw.update(cons_var=T(hb.cons_var, torch.int32), cons_a=T(hb.cons_a, dt), cons_b=T(hb.cons_b, dt))
    if level == "G":
        return Q.BatchedQP(G=T(hb.G, dt), c=T(hb.c, dt), **kw)
    B, m_r, n = hb.J.shape
    if J_layout == "col":
        return Q.BatchedQP(J=T(padded(hb.J.transpose(0, 2, 1), J_ld or m_r), dt), r=T(hb.r, dt), lam=hb.lam, J_layout="col", J_rows=m_r, **kw)
    return Q.BatchedQP(J=T(padded(hb.J, J_ld or n), dt), r=T(hb.r, dt), lam=hb.lam, **kw)


def oracle_solver(hb, p, state=None):
    o = orc.Solver(orc.QP(G=np.tril(hb.G[p]), c=hb.c[p], A_eq=hb.A_eq[p].T if hb.k else None, b_eq=hb.b_eq[p] if hb.k else None,
                          cons_var=hb.cons_var[p], cons_a=hb.cons_a[p], cons_b=hb.cons_b[p]))
    if state is not None:
        o.variables[:] = state
    return o


def oracle_kkt_solves(o, n, k, m, rhs, g):
    """delta with K delta = -rhs and u with K^T u = g by LU on the oracle's full_system() matrix Hf at its current state.  Hf is the
    reference's BuildFullSystem: the row of r_comp divided by s, and the y and z unknowns negated, i.e. K = D_r Hf D_c with
    D_r = diag(1, s, 1, 1), D_c = diag(1, 1, -1, -1)."""
    Hf, _ = o.full_system()
    s = np.array(o.variables[n:n + m])
    d_r = np.concatenate([np.ones(n), s, np.ones(k + m)])
    d_c = np.concatenate([np.ones(n + m), -np.ones(k + m)])
    delta = d_c * np.linalg.solve(Hf, -rhs / d_r)
    u = np.linalg.solve(Hf.T, d_c * g) / d_r
    return delta, u


ACTIVE_SEED, ACTIVE_COUNT = 2024, 200


def active_set_problems():
    """n = 8, G = U U^T / n + I with U ~ U(-1, 1), c ~ 2 N(0, 1), 1 ... n single-variable rows on distinct variables with a = +-1,
    b ~ U(0.1, 1); g non-zero on the x block only.  Grouped by the number of rows (a batch has one shape): 25 problems for each m = 1 ... 8."""
    rng = np.random.default_rng(ACTIVE_SEED)
    n = 8
    groups = []
    for m in range(1, n + 1):
        cnt = ACTIVE_COUNT // n
        U = rng.uniform(-1, 1, (cnt, n, n))
        G = np.einsum("bik,bjk->bij", U, U) / n + np.eye(n)
        c = 2 * rng.normal(size=(cnt, n))
        var = np.stack([rng.permutation(n)[:m] for _ in range(cnt)]).astype(np.int32)
        a = rng.choice([-1.0, 1.0], (cnt, m))
        b = rng.uniform(0.1, 1.0, (cnt, m))
        gx = rng.normal(size=(cnt, n))
        groups.append(dict(n=n, m=m, G=G, c=c, var=var, a=a, b=b, gx=gx))
    return groups


# ---- residual-block layouts --------------------------------------------------------------------------------------------------------------------
N7_COST = [((3, 0, 5, 3), 3), ((6,), 2), ((1, 2, 4, 0, 6), 4), ((2, 2), 1), ((5, 4, 1), 6)]
LAM = 0.1   # the damping of the block autograd tests


def random_layout(rng, n, count, repeats=False):
    blocks = []
    for _ in range(count):
        R_ = int(rng.integers(1, 7))
        Pn = int(rng.integers(1, min(n, 8) + 1))
        if repeats and Pn >= 2 and rng.random() < 0.5:
            idx = list(rng.integers(0, n, Pn))
            idx[-1] = idx[0]         # a repeated variable inside the block
        else:
            idx = list(rng.permutation(n)[:Pn])   # out of order
        blocks.append((tuple(int(i) for i in idx), R_))
    return blocks


def autograd_layout(n, rng):
    if n == 64:
        return [(tuple(int(i) for i in rng.permutation(n)[:4]), 2) for _ in range(96)]
    return [(tuple(int(i) for i in rng.permutation(n)[:4]), 2) for _ in range(11)] + [((3, 0, 5, 3), 3)]     # one repeated variable


def bound_factor(blocks):
    """(2 R_b P_b + 8) per packed value and per stacked row."""
    per_val = np.concatenate([np.full(R_ * len(idx), 2 * R_ * len(idx) + 8.0) for idx, R_ in blocks])
    per_row = np.concatenate([np.full(R_, 2 * R_ * len(idx) + 8.0) for idx, R_ in blocks])
    return per_val, per_row
