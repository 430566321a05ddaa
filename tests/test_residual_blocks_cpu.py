"""CPU-side checks of the residual-block input: the packing helper against the dense stack of nls.stack_residuals, the NULL-argument
returns of the new C entry points (no GPU needed) and the scratch-free listing of residual_blocks.hip."""
import ctypes as C
import os
import re

import pytest
import torch

from mini_opt_amd import _lib as L
from mini_opt_amd import nls as NLS
from mini_opt_amd import qp as Q

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LISTING = os.path.join(ROOT, "mini_opt_amd", "csrc", "build", "residual_blocks-hip-amdgcn-amd-amdhsa-gfx950.s")


@pytest.fixture(scope="module")
def lib():
    L.build()
    return L.lib()


def _affine(R, P, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(R, P, generator=g, dtype=torch.float64)
    b = torch.randn(R, generator=g, dtype=torch.float64)

    def fn(x, want_J):   # r = A x^2 + b: J = A diag(2 x)
        r = (x * x) @ A.T + b
        return r, (A.unsqueeze(0) * (2 * x).unsqueeze(1) if want_J else None)
    return fn


def test_pack_blocks_round_trips_against_stack_residuals():
    n, B = 9, 5
    specs = [((3, 0, 7), 2), ((8,), 1), ((1, 2, 4, 5), 3), ((6, 3), 4)]
    residuals = [NLS.MakeResidual(idx, _affine(R, len(idx), s), R) for s, (idx, R) in enumerate(specs)]
    x = torch.randn(B, n, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    r_dense, J_dense = NLS.stack_residuals(residuals, n)(x, True)
    locals_ = [res.fn(x[:, list(res.index)], True) for res in residuals]
    packed = Q.pack_blocks([J for _, J in locals_])
    assert packed.shape == (B, sum(R * len(idx) for idx, R in specs))
    # block b is R x P column-major at offset sum R P of the blocks before it
    off = 0
    for (idx, R), (_, J) in zip(specs, locals_):
        for a in range(len(idx)):
            assert torch.equal(packed[:, off + a * R: off + (a + 1) * R], J[:, :, a])
        off += R * len(idx)
    back = Q.unpack_blocks(packed, [(R, len(idx)) for idx, R in specs])
    J_scatter = torch.zeros_like(J_dense)
    row = 0
    for (idx, R), Jb, (_, J) in zip(specs, back, locals_):
        assert torch.equal(Jb, J)
        J_scatter[:, row:row + R, list(idx)] = Jb
        row += R
    assert torch.equal(J_scatter, J_dense)
    assert torch.equal(torch.cat([r for r, _ in locals_], 1), r_dense)


def test_problem_from_residuals_keeps_its_residual_lists():
    costs = [NLS.MakeResidual((0, 1), _affine(2, 2, 0), 2)]
    eqs = [NLS.MakeResidual((1,), _affine(1, 1, 1), 1)]
    p = NLS.Problem.FromResiduals(2, costs, eqs)
    assert p.cost_residuals == costs and p.equality_residuals == eqs and p.cost_rows == 2 and p.equality_rows == 1
    q = NLS.Problem(2, costs[0].fn, cost_rows=2)
    assert q.cost_residuals is None and q.equality_residuals is None


def test_block_entry_points_reject_null_arguments(lib):
    h = C.c_void_p()
    one = (C.c_int32 * 1)(1)
    assert lib.mo_residual_layout_create(None, 1, one, one, one, C.byref(h)) == -1
    assert lib.mo_residual_layout_create(None, 1, one, one, one, None) == -1
    assert lib.mo_residual_layout_values(None) == -1 and lib.mo_residual_layout_rows(None) == -1
    assert lib.mo_residual_layout_destroy(None) == 0
    assert lib.mo_linearize_blocks(None, None, None, 0, None, 0, 0.0, None, 0, 1, None, 0, 1, None, 0, None, None) == -1
    assert lib.mo_jacobian_blocks(None, None, None, 0, None, 0, 1, None, 0, 1, 0, None, None) == -1
    prm = L.NlsParams()
    lib.mo_default_nls_params(C.byref(prm))
    assert lib.mo_nls_solve_blocks(None, None, None, None, 1, C.byref(prm), L.NLS_EVAL_FN(lambda u, w, s: 0), None, None, None, None, None,
                                   None) == -1
    assert b"NULL" in lib.mo_last_error()


def test_residual_blocks_kernels_use_no_scratch(lib):
    if not os.path.exists(LISTING):
        pytest.skip("no gfx950 listing of residual_blocks.hip in this build")
    text = open(LISTING).read()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)", text)
    sizes = re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", text)
    assert kernels and len(kernels) == len(sizes)
    assert all(s == "0" for s in sizes), dict(zip(kernels, sizes))
    assert "s_swappc_b64" not in text
