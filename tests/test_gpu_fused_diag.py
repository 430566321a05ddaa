"""The fused fp64 step kernel of the 64 grid with its diagonal J^T J tiles on v_mfma_f64_4x4x4_4b_f64 (DIAG4, csrc/mo_fused_diag.h), against
the CPU oracle.  Inputs as in test_fused_kernels_take_every_layout_of_J (uniform J, A, r; lambda = 1e-3, or 0.5 when J has fewer rows than
variables); every step within the project's fp64 tolerance of oracle.batched_newton_step: 1e-10 rel-inf, status equal, alpha within 1e-9.
Shapes: the headline; fewer 4-row groups than the ring is deep; the m_r % 4 tail alone and tails of 1, 2 and 3 rows (staged through a ring
slot at the swizzled places); padded rows (n < 64) with the swizzle; the full y tile with every constraint lane; and 8 192 padded problems so
that every wave takes several in a row (a ring left dirty by the tile conversion would feed the next problem's padding)."""
import numpy as np
import pytest
import torch

from mini_opt_amd import qp as Q
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

CASES = [(64, 8, 32, 128, 7), (64, 8, 32, 8, 7), (64, 8, 32, 4, 7), (64, 0, 0, 3, 7), (64, 8, 32, 13, 7), (64, 8, 32, 14, 7), (64, 8, 32, 15, 7),
         (62, 8, 32, 20, 7), (34, 3, 5, 37, 7), (64, 15, 64, 36, 7), (50, 8, 32, 12, 8192)]


def T(a, dt=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=torch.device("cuda:0")).contiguous()


def rel_inf_rows(got, ref):
    return np.max(np.abs(got - ref), axis=1) / np.max(np.abs(ref), axis=1)


def make_case(n, k, m, m_r, B, seed):
    rng = np.random.default_rng(seed)
    J = rng.uniform(-1, 1, (B, m_r, n)); r = rng.uniform(-1, 1, (B, m_r))
    A = rng.uniform(-1, 1, (B, n, k)); b = rng.uniform(-1, 1, (B, k))
    cv = rng.integers(0, n, (B, m)).astype(np.int32); ca = rng.choice([-1.0, 1.0, 2.0], (B, m)); cb = rng.uniform(0.5, 2.0, (B, m))
    x = rng.uniform(-0.1, 0.1, (B, n)); sl = rng.uniform(0.2, 1.5, (B, m)); z = rng.uniform(0.1, 2, (B, m)); y = rng.uniform(-1, 1, (B, k))
    vars_ = np.concatenate([x, sl, y, z], axis=1); mu = np.full(B, 0.05)
    lam = 1e-3 if m_r >= n else 0.5      # (fewer rows than variables: J^T J alone is singular)
    return dict(J=J, r=r, A=A, b=b, cv=cv, ca=ca, cb=cb, vars_=vars_, mu=mu, lam=lam)


def gpu_step(n, k, m, c):
    prob = Q.BatchedQP(n=n, k=k, m=m, J=T(c["J"]), r=T(c["r"]), lam=c["lam"], A_eq=T(c["A"]), b_eq=T(c["b"]), cons_var=T(c["cv"], torch.int32),
                       cons_a=T(c["ca"]), cons_b=T(c["cb"]))
    s = Q.QPInteriorPointSolver(prob)
    assert s.step_kernel().startswith("fused"), s.step_kernel()
    s.SetVariables(T(c["vars_"]))
    delta, alpha, status = s.NewtonStep(T(c["mu"]), 0.995)
    return delta.cpu().numpy().copy(), alpha.cpu().numpy().copy(), status.cpu().numpy().copy()


@pytest.mark.parametrize("idx", range(len(CASES)), ids=["n%d_k%d_m%d_mr%d_b%d" % c for c in CASES])
def test_step_against_oracle(idx):
    n, k, m, m_r, B = CASES[idx]
    c = make_case(n, k, m, m_r, B, 1000 + idx)
    ref, ref_alpha, ref_status, _ = orc.batched_newton_step(n, k, m, J=c["J"], r=c["r"], lam=c["lam"], A_eq=c["A"], b_eq=c["b"], cons_var=c["cv"],
                                                            cons_a=c["ca"], cons_b=c["cb"], vars_=c["vars_"], mu=c["mu"])
    assert np.all(ref_status == 0)
    delta, alpha, status = gpu_step(n, k, m, c)
    err = rel_inf_rows(delta, ref).max()
    print("n=%d k=%d m=%d m_r=%d batch=%d: max rel-inf %.3e, max |alpha - ref| %.3e" % (n, k, m, m_r, B, err, np.abs(alpha - ref_alpha).max()))
    assert np.array_equal(status, ref_status)
    assert err < 1e-10
    np.testing.assert_allclose(alpha, ref_alpha, rtol=0, atol=1e-9)


def test_headline_shape_is_bit_reproducible():
    n, k, m, m_r, B = CASES[0]
    c = make_case(n, k, m, m_r, B, 1000)
    first, second = gpu_step(n, k, m, c), gpu_step(n, k, m, c)
    assert np.array_equal(first[0], second[0])
