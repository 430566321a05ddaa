"""CPU checks of the batch-reduced block gradients (mo_qp_gradients_blocks_shared): the symbols and the struct mirror, the argument errors that
need no device, and the moment formulas and the chunked scheme against the masked sum of the per-problem block formulas."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import blocks_shared_grad_reference as BS
from tests.sens_fixtures import N7_COST, UNIT, random_layout

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
N7_EQ = [((0, 4, 0), 1), ((2, 6), 2)]     # local column 0 of the first block LOSES variable 0 to column 2


@pytest.fixture(scope="module")
def lib():
    from mini_opt_amd import _lib as L
    L.build()
    return L.lib()


def test_symbols_are_declared_and_exported(lib):
    from mini_opt_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "mini_opt_hip.h")).read()
    declared = set(re.findall(r"\b(mo_[a-z_]+)\s*\(", header))
    for name in ("mo_qp_gradients_blocks_shared_workspace", "mo_qp_gradients_blocks_shared"):
        assert name in declared and name in L.EXPORTS and hasattr(lib, name)
    major = int(re.search(r"#define\s+MO_VERSION_MAJOR\s+(\d+)", header).group(1))
    minor = int(re.search(r"#define\s+MO_VERSION_MINOR\s+(\d+)", header).group(1))
    assert f"{major}.{minor}".encode() in lib.mo_version_string()      # (the header and the library state one version)


def test_front_end_is_exported():
    import mini_opt_amd
    assert callable(mini_opt_amd.qp_gradients_blocks_shared)


def test_struct_mirror_matches_the_header_layout(tmp_path):
    from mini_opt_amd import _lib as L
    fields = [f for f, _ in L.BlockSharedGrads._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mini_opt_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(mo_block_shared_grads));']
    lines += [f'  printf("{f} %zu\\n", offsetof(mo_block_shared_grads, {f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "bsgrads.c", tmp_path / "bsgrads"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["size"]) == C.sizeof(L.BlockSharedGrads)
    for f in fields:
        assert int(out[f]) == getattr(L.BlockSharedGrads, f).offset, f


def test_argument_errors_without_gpu(lib):
    """Arguments are judged before the plan is looked at, so every refusal that follows from them alone needs no device; the workspace
    query judges the same and leaves `bytes` alone."""
    from mini_opt_amd import _lib as L
    p16, p32, lay = C.c_void_p(16), C.c_void_p(32), C.c_void_p(64)
    nbytes = C.c_int64(-1)

    def both(out, word, layout=lay, eq=None, J=p16, r=p16, r_stride=4, batch=4, query=True):
        ref = None if out is None else C.byref(out)
        assert lib.mo_qp_gradients_blocks_shared(None, layout, J, r, r_stride, eq, batch, p16, 8, p32, 8, None, None, ref, p16, 1 << 20, None) == -1, word
        assert word in lib.mo_last_error(), (word, lib.mo_last_error())
        if query:
            assert lib.mo_qp_gradients_blocks_shared_workspace(None, layout, eq, r_stride, batch, ref, C.byref(nbytes)) == -1, word
            assert word in lib.mo_last_error() and nbytes.value == -1, (word, lib.mo_last_error())

    g = L.BlockSharedGrads()
    g.dJ_blocks = 16
    both(g, b"plan")
    both(g, b"cost_layout", layout=None)
    both(None, b"out")
    both(g, b"batch", batch=-1)
    both(g, b"J_blocks", J=None, query=False)            # dJ_blocks without J_blocks
    both(g, b"J_blocks", r=None, query=False)            # ... or without r
    g = L.BlockSharedGrads()
    g.dr = 16
    both(g, b"r_stride")                                 # dr needs one r for the batch
    both(g, b"plan", r_stride=0)
    for member in ("dJ_eq_blocks", "dr_eq"):
        g = L.BlockSharedGrads()
        setattr(g, member, 16)
        both(g, b"eq_layout")                            # an equality member without eq_layout
        both(g, b"plan", eq=lay)
    assert lib.mo_qp_gradients_blocks_shared_workspace(None, lay, None, 4, 4, C.byref(g), None) == -1
    assert b"bytes" in lib.mo_last_error()


# ---- the front end (mini_opt_amd.diff): the partition of the block backward, the member table, the filled structs ---------------------------
def test_partition_of_the_block_backward():
    """(each, summed): what the batch shares goes to the reduced launches -- but r given once against J_blocks per problem is computed per
    problem."""
    from mini_opt_amd import diff as D
    names = ["J_blocks", "r", "lam", "J_eq_blocks", "r_eq", "cons_a", "cons_b"]
    assert list(D.QPSolveBlocksFunction.NAMES) == names
    part = lambda want, shared: D._partition(want, frozenset(shared), "r", "J_blocks")
    assert part(names, names) == ([], names)                                             # everything shared
    assert part(names, ()) == (names, [])                                                # nothing shared
    assert part(["J_blocks", "r", "lam"], ["r"]) == (["J_blocks", "r", "lam"], [])       # r shared, J_blocks per problem: each
    assert part(["r", "r_eq"], ["r", "r_eq"]) == (["r"], ["r_eq"])                       # ... also when dJ_blocks is not asked for
    assert part(["J_blocks", "r", "lam"], ["J_blocks", "r"]) == (["lam"], ["J_blocks", "r"])   # r and J_blocks both shared: summed
    assert part(["r_eq", "cons_a", "cons_b"], ["cons_a", "cons_b"]) == (["r_eq"], ["cons_a", "cons_b"])
    assert part(["r_eq", "cons_a", "cons_b"], ["r_eq", "J_eq_blocks"]) == (["cons_a", "cons_b"], ["r_eq"])


def test_block_member_table_against_the_structs():
    from mini_opt_amd import _lib as L
    from mini_opt_amd import diff as D
    assert tuple(D._BLOCK) == D.BLOCK_TANGENTS == ("J_blocks", "r", "lam", "J_eq_blocks", "r_eq", "cons_a", "cons_b")
    assert D.BLOCK_GRADIENTS == D.BLOCK_TANGENTS[:5]
    for struct, names, strided in ((L.BlockGrads, D.BLOCK_TANGENTS[:3], True), (L.BlockSharedGrads, D.BLOCK_GRADIENTS, False),
                                   (L.BlockTangents, D.BLOCK_TANGENTS, True)):
        fields = dict(struct._fields_)
        for name in names:
            ptr, stride, ld, _tail = D._BLOCK[name]
            assert fields[ptr] is C.c_void_p and ld is None and (not strided or fields[stride] is C.c_int64), (struct, name)
        assert {D._BLOCK[name][0] for name in names} == {f for f, t in struct._fields_ if t is C.c_void_p}   # every pointer has its name
    assert D._BLOCK["cons_a"][1] == D._BLOCK["cons_b"][1] == "dcons_stride"


def test_block_gradient_structs_are_filled_as_before():
    """_outputs on CPU tensors (no launch) for a cost layout of 23 values in 11 rows and an equality layout of 7 values in k = 3 rows, against
    the values qp_gradients_blocks (per problem, B = 5: strides values, rows, 1) and qp_gradients_blocks_shared (one instance per member,
    pointers alone) set member by member before the table."""
    import types
    from mini_opt_amd import _lib as L
    from mini_opt_amd import diff as D
    lay = lambda values, rows: types.SimpleNamespace(n=7, values=values, rows=rows, dtype=torch.float64, device=torch.device("cpu"))
    blocks = D._Blocks(lay(23, 11), lay(7, 3), 3, 4)
    fields = lambda g: {f: getattr(g, f) for f, _ in g._fields_}
    out, g = D._outputs(L.BlockGrads(), D._BLOCK, blocks, ("J_blocks", "r", "lam"), 5)
    assert [tuple(t.shape) for t in out.values()] == [(5, 23), (5, 11), (5,)]
    assert fields(g) == dict(dJ_blocks=out["J_blocks"].data_ptr(), dJ_stride=23, dr=out["r"].data_ptr(), dr_stride=11,
                             dlambda=out["lam"].data_ptr(), dlambda_stride=1)
    out, g = D._outputs(L.BlockGrads(), D._BLOCK, blocks, ("lam",), 5)
    assert fields(g) == dict(dJ_blocks=None, dJ_stride=0, dr=None, dr_stride=0, dlambda=out["lam"].data_ptr(), dlambda_stride=1)
    out, g = D._outputs(L.BlockSharedGrads(), D._BLOCK, blocks, D.BLOCK_GRADIENTS, 1, strided=False)
    assert [tuple(t.shape) for t in out.values()] == [(1, 23), (1, 11), (1,), (1, 7), (1, 3)]
    assert fields(g) == dict(dJ_blocks=out["J_blocks"].data_ptr(), dr=out["r"].data_ptr(), dlambda=out["lam"].data_ptr(),
                             dJ_eq_blocks=out["J_eq_blocks"].data_ptr(), dr_eq=out["r_eq"].data_ptr())
    out, g = D._outputs(L.BlockSharedGrads(), D._BLOCK, blocks, ("r_eq",), 1, strided=False)
    assert fields(g) == dict(dJ_blocks=None, dr=None, dlambda=None, dJ_eq_blocks=None, dr_eq=out["r_eq"].data_ptr())
    out, g = D._outputs(None, D._BLOCK, D._Blocks(None, lay(7, 3), 3, 4), ("J_eq_blocks", "r_eq"), 5)   # qp_gradients_eq_blocks: tensors alone
    assert g is None and [tuple(t.shape) for t in out.values()] == [(5, 7), (5, 3)] and all(t.dtype == torch.float64 for t in out.values())


# ---- the formulas ------------------------------------------------------------------------------------------------------------------------
def _case(name, integers=False):
    rng = np.random.default_rng({"n7": 7007, "n33": 3303}[name])
    if name == "n7":
        n, cost, eq = 7, N7_COST, N7_EQ
    else:
        n, cost = 33, random_layout(rng, 33, 14, repeats=True)
        eq = [((5, 20, 5, 32), 2), ((16, 0, 31), 1)]
        assert any(len(set(idx)) < len(idx) for idx, _ in cost)
    k, m, B = sum(R_ for _, R_ in eq), 3, 37
    draw = (lambda *s: rng.integers(-2, 3, s).astype(np.float64)) if integers else (lambda *s: rng.normal(size=s))
    values, rows = sum(R_ * len(idx) for idx, R_ in cost), sum(R_ for _, R_ in cost)
    V, U = draw(B, n + 2 * m + k), draw(B, n + 2 * m + k)
    ok = np.arange(B) % 5 != 2
    U[~ok] = np.nan
    return dict(n=n, k=k, m=m, cost=cost, eq=eq, Jv=draw(values), R=draw(B, rows), V=V, U=U, ok=ok, B=B)


@pytest.mark.parametrize("r_shared", [False, True], ids=["r_per_problem", "r_shared"])
@pytest.mark.parametrize("name", ["n7", "n33"])
def test_moment_formulas_equal_the_direct_sum(name, r_shared):
    """ONE chunk: the formulas of include/mini_opt_hip.h from the moments of the whole batch against the masked sum of the per-problem block
    gradients, on layouts with a repeated index inside a block and a losing equality column, every fifth problem masked with a NaN adjoint."""
    c = _case(name)
    R = c["R"][:1] if r_shared else c["R"]
    args = (c["n"], c["k"], c["m"], c["cost"], c["eq"], c["Jv"], R, c["V"], c["U"], c["ok"])
    want, mag = BS.direct(*args), BS.direct(*args, absolute=True)
    tol = BS.bound(c["B"], BS.p_max(c["cost"], c["eq"]), UNIT[torch.float64], mag)
    got = BS.chunked(*args, c["B"])
    assert set(got) == set(want)
    for key in want:
        err = np.abs(got[key] - want[key])
        assert np.all(np.isfinite(got[key])) and np.all(err <= tol[key]), (key, np.max(err))
    lost = BS.positions(c["eq"])   # the losing column is exactly zero
    assert got["J_eq_blocks"][0] == 0.0 and want["J_eq_blocks"][0] == 0.0 and lost[1][0] in (0, 5)


@pytest.mark.parametrize("name", ["n7", "n33"])
def test_batched_direct_sum_equals_the_loop(name):
    """direct_batched (what the GPU tests use beyond a few dozen problems) against direct: value and magnitude, within 8 B units of the magnitude;
    integers exactly."""
    for integers in (False, True):
        c = _case(name, integers=integers)
        args = (c["n"], c["k"], c["m"], c["cost"], c["eq"], c["Jv"], c["R"], c["V"], c["U"], c["ok"])
        mag = BS.direct(*args, absolute=True)
        for absolute in (False, True):
            want, got = BS.direct(*args, absolute=absolute), BS.direct_batched(*args, absolute=absolute)
            for key in want:
                if integers:
                    assert np.array_equal(got[key], want[key]), (key, absolute)
                assert np.all(np.abs(got[key] - want[key]) <= 8 * c["B"] * UNIT[torch.float64] * np.asarray(mag[key])), (key, absolute)


@pytest.mark.parametrize("r_shared", [False, True], ids=["r_per_problem", "r_shared"])
@pytest.mark.parametrize("name", ["n7", "n33"])
def test_chunked_scheme_against_the_direct_sum(name, r_shared):
    c = _case(name)
    R = c["R"][:1] if r_shared else c["R"]
    args = (c["n"], c["k"], c["m"], c["cost"], c["eq"], c["Jv"], R, c["V"], c["U"], c["ok"])
    want, mag = BS.direct(*args), BS.direct(*args, absolute=True)
    tol = BS.bound(c["B"], BS.p_max(c["cost"], c["eq"]), UNIT[torch.float64], mag)
    worst = 0.0
    for length in (4, 5, BS.chunk_len(c["B"], 256)):
        got = BS.chunked(*args, length)
        for key in want:
            ratio = np.max(np.abs(got[key] - want[key]) / np.where(tol[key] > 0, tol[key], 1.0))
            assert np.all(np.isfinite(got[key])) and ratio <= 1.0, (key, length, ratio)
            worst = max(worst, float(ratio))
    print(f"largest error / bound = {worst:.3e}")


@pytest.mark.parametrize("r_shared", [False, True], ids=["r_per_problem", "r_shared"])
@pytest.mark.parametrize("name", ["n7", "n33"])
def test_integer_data_gives_exactly_equal_results(name, r_shared):
    c = _case(name, integers=True)
    R = c["R"][:1] if r_shared else c["R"]
    args = (c["n"], c["k"], c["m"], c["cost"], c["eq"], c["Jv"], R, c["V"], c["U"], c["ok"])
    want = BS.direct(*args)
    for length in (4, 37):
        got = BS.chunked(*args, length)
        for key in want:
            assert np.array_equal(got[key], want[key]), (key, length)
