"""CPU checks of the batch-reduced block gradients under per-row weights (mo_qp_gradients_blocks_weighted_shared): the symbols and the struct
mirror, the argument errors that need no device, the opt-in flag of the front end, and the formulas and the chunked scheme of
tests/blocks_weighted_shared_reference.py against the masked sum of the per-problem weighted block formulas
(tests/weighted_blocks_reference.py, written pair by pair and row by row)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import blocks_weighted_shared_reference as WS
from tests import weighted_blocks_reference as WR
from tests.sens_fixtures import N7_COST, UNIT, autograd_layout

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("mo_qp_gradients_blocks_weighted_shared_workspace", "mo_qp_gradients_blocks_weighted_shared")
KEYS = ("J_blocks", "r", "weights", "lam")


@pytest.fixture(scope="module")
def lib():
    from mini_opt_amd import _lib as L
    L.build()
    return L.lib()


def test_symbols_are_declared_and_exported(lib):
    from mini_opt_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "mini_opt_hip.h")).read()
    declared = set(re.findall(r"\b(mo_[a-z_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name)
    assert b"0.5" in lib.mo_version_string()      # the ABI grew; nothing that existed changed


def test_front_end_is_exported_and_the_flag_is_opt_in():
    import mini_opt_amd
    from mini_opt_amd import diff as D
    assert callable(mini_opt_amd.qp_gradients_blocks_weighted_shared)
    assert inspect.signature(D.solve_qp).parameters["reduce_in_kernel"].default is False
    assert inspect.signature(D.QPSolveWeightedBlocksFunction.forward).parameters["reduce_in_kernel"].default is False
    assert "reduce_in_kernel" in D.solve_qp.__doc__ and "bit" in D.solve_qp.__doc__


def test_struct_mirror_matches_the_header_layout(tmp_path):
    from mini_opt_amd import _lib as L
    fields = [f for f, _ in L.BlockWeightedSharedGrads._fields_]
    assert fields == ["dJ_blocks", "dr", "dlambda", "dweights"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mini_opt_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(mo_block_weighted_shared_grads));']
    lines += [f'  printf("{f} %zu\\n", offsetof(mo_block_weighted_shared_grads, {f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "bwsgrads.c", tmp_path / "bwsgrads"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["size"]) == C.sizeof(L.BlockWeightedSharedGrads)
    for f in fields:
        assert int(out[f]) == getattr(L.BlockWeightedSharedGrads, f).offset, f


def test_argument_errors_without_gpu(lib):
    """Arguments are judged before the plan is looked at, so every refusal that follows from them alone needs no device; the workspace
    query judges the same and leaves `bytes` alone."""
    from mini_opt_amd import _lib as L
    p16, p32, lay = C.c_void_p(16), C.c_void_p(32), C.c_void_p(64)
    nbytes = C.c_int64(-1)

    def both(out, word, layout=lay, J=p16, r=p16, w=p16, r_stride=4, w_stride=4, batch=4, query=True):
        ref = None if out is None else C.byref(out)
        rc = lib.mo_qp_gradients_blocks_weighted_shared(None, layout, J, r, r_stride, w, w_stride, batch, p16, 8, p32, 8, None, None, ref, p16,
                                                        1 << 20, None)
        assert rc == -1 and word in lib.mo_last_error(), (word, rc, lib.mo_last_error())
        if query:
            assert lib.mo_qp_gradients_blocks_weighted_shared_workspace(None, layout, r_stride, w_stride, batch, ref, C.byref(nbytes)) == -1, word
            assert word in lib.mo_last_error() and nbytes.value == -1, (word, lib.mo_last_error())

    g = L.BlockWeightedSharedGrads()
    g.dJ_blocks = 16
    both(g, b"plan")
    both(g, b"cost_layout", layout=None)
    both(None, b"out")
    both(g, b"batch", batch=-1)
    both(g, b"J_blocks", J=None, query=False)
    both(g, b"J_blocks / r", r=None, query=False)
    both(g, b"weights", w=None, query=False)
    g = L.BlockWeightedSharedGrads()
    g.dr = 16
    both(g, b"r_stride")                                 # dr needs one r for the batch
    both(g, b"plan", r_stride=0)
    g = L.BlockWeightedSharedGrads()
    g.dweights = 16
    both(g, b"weights_stride")                           # dweights needs one instance of the weights
    both(g, b"plan", w_stride=0)
    assert lib.mo_qp_gradients_blocks_weighted_shared_workspace(None, lay, 4, 4, 4, C.byref(g), None) == -1
    assert b"bytes" in lib.mo_last_error()


def test_member_table_against_the_struct():
    from mini_opt_amd import _lib as L
    from mini_opt_amd import diff as D
    assert D._WEIGHTED_COST == ("J_blocks", "r", "lam", "weights")
    assert {D._WEIGHTED[name][0] for name in D._WEIGHTED_COST} == {f for f, _ in L.BlockWeightedSharedGrads._fields_}


# ---- the formulas ------------------------------------------------------------------------------------------------------------------------
def _case(name, integers=False, seed=0):
    """n7: N7_COST, which repeats a variable inside two blocks (partner and pair lists); n24: 12 blocks of 2 x 4 without repeats.  Every fifth
    problem is masked and holds NaN in u, r and the weights; rows with w == 0 (every seventh entry of the weights) hold NaN in r."""
    rng = np.random.default_rng({"n7": 7107, "n24": 2407}[name] + seed)
    if name == "n7":
        n, cost = 7, N7_COST
        assert any(len(set(idx)) < len(idx) for idx, _ in cost)
    else:
        n, cost = 24, autograd_layout(24, rng)[:11]
        assert all(len(set(idx)) == len(idx) for idx, _ in cost)
    B = 37
    draw = (lambda *s: rng.integers(-2, 3, s).astype(np.float64)) if integers else (lambda *s: rng.normal(size=s))
    values, rows = sum(R_ * len(idx) for idx, R_ in cost), sum(R_ for _, R_ in cost)
    V, U = draw(B, n + 3), draw(B, n + 3)
    ok = np.arange(B) % 5 != 2
    Wt = rng.integers(0, 4, (B, rows)).astype(np.float64) if integers else rng.uniform(0.25, 2.0, (B, rows))
    Wt.reshape(-1)[::7] = 0.0
    R = draw(B, rows)
    return dict(n=n, cost=cost, Jv=draw(values), R=R, Wt=Wt, V=V, U=U, ok=ok, B=B)


def _sharing(c, r_shared, w_shared, poison=True):
    """The case with r and / or the weights given once; poison: NaN in the masked problems and, for an r per problem, at the rows whose
    weight is 0."""
    R, Wt, U = (c["R"][:1] if r_shared else c["R"]).copy(), (c["Wt"][:1] if w_shared else c["Wt"]).copy(), c["U"].copy()
    if poison:
        U[~c["ok"]] = np.nan
        if not r_shared:
            R[np.broadcast_to(Wt, R.shape) == 0] = np.nan
            R[~c["ok"]] = np.nan
        if not w_shared:
            Wt[~c["ok"]] = np.nan
    return dict(c, R=R, Wt=Wt, U=U)


def _args(c):
    return (c["n"], c["cost"], c["Jv"], c["R"], c["Wt"], c["V"], c["U"], c["ok"])


def per_problem_sum(c, correction=True, absolute=False):
    """The sum over the counted problems of weighted_blocks_reference.gradients."""
    cost, n, B = c["cost"], c["n"], c["B"]
    Js = WR.unpack(c["Jv"], cost)
    R, Wt = np.broadcast_to(c["R"], (B, c["R"].shape[1])), np.broadcast_to(c["Wt"], (B, c["Wt"].shape[1]))
    out = dict(J_blocks=0.0, r=0.0, weights=0.0, lam=0.0)
    with np.errstate(invalid="ignore"):
        for p in np.flatnonzero(c["ok"]):
            dJs, drs, dlam, dws = WR.gradients(cost, Js, WR.split_rows(R[p], cost), WR.split_rows(Wt[p], cost), c["V"][p, :n], c["U"][p, :n],
                                               absolute=absolute, correction=correction)
            out["J_blocks"] = out["J_blocks"] + WR.pack(dJs)
            out["r"] = out["r"] + np.concatenate(drs)
            out["weights"] = out["weights"] + np.concatenate(dws)
            out["lam"] = out["lam"] + dlam
    return out


def _keys(r_shared, w_shared):
    """What a sharing combination may ask for: "r" / "weights" only when given once (and "weights" is NaN by design at a NaN r)."""
    return ("J_blocks", "lam") + (("r",) if r_shared else ()) + (("weights",) if w_shared and r_shared else ())


def _close(got, want, rel=1e-12):
    scale = np.max(np.abs(want)) if np.size(want) else 0.0
    return np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= rel * max(scale, 1e-300))


SHARING = pytest.mark.parametrize("r_shared,w_shared", [(False, False), (True, False), (False, True), (True, True)],
                                  ids=["r_w_per_problem", "r_once", "w_once", "r_w_once"])


@SHARING
@pytest.mark.parametrize("name", ["n7", "n24"])
def test_direct_equals_the_sum_of_the_per_problem_formulas(name, r_shared, w_shared):
    """Masked problems (NaN rows), rows with w == 0 and NaN in r: `direct` and its magnitude against the pair-by-pair formulas summed."""
    c = _sharing(_case(name), r_shared, w_shared)
    want, got = per_problem_sum(c), WS.direct(*_args(c))
    for key in _keys(r_shared, w_shared):
        assert _close(got[key], want[key]), (key, np.max(np.abs(got[key] - want[key])))
    if not r_shared:   # the zero rule: an r per problem holds NaN at every row whose weight is 0
        assert np.isnan(c["R"][c["ok"]]).any()
    # the magnitude: that of the pair-by-pair form, except at a packed value whose variable the block names twice -- there the t / s form
    # reaches the pair twice and takes it back once (three terms, not one), so the sum |terms| is larger, never smaller
    mag_want, mag_got = per_problem_sum(c, absolute=True), WS.direct(*_args(c), absolute=True)
    twice = np.concatenate([np.repeat([idx.count(g) > 1 for g in idx], R_) for idx, R_ in c["cost"]])
    assert twice.any() == (name == "n7")
    for key in _keys(r_shared, w_shared):
        if key == "J_blocks":
            assert _close(mag_got[key][~twice], mag_want[key][~twice]) and np.all(mag_got[key][twice] >= mag_want[key][twice])
        else:
            assert _close(mag_got[key], mag_want[key]), key


@SHARING
@pytest.mark.parametrize("name", ["n7", "n24"])
def test_chunked_scheme_equals_the_sum_of_the_per_problem_formulas(name, r_shared, w_shared):
    c = _sharing(_case(name), r_shared, w_shared)
    want = per_problem_sum(c)
    for length, stage in ((4, 16), (5, 2), (WS.chunk_len(c["B"], 256), 16), (c["B"], 3)):
        got = WS.chunked(*_args(c), length, stage)
        for key in _keys(r_shared, w_shared):
            assert _close(got[key], want[key]), (key, length, stage)


def test_weights_gradient_without_poison():
    """dweights is computed from whatever the data hold, so it is compared on clean data: both layouts, weights given once."""
    for name in ("n7", "n24"):
        c = _sharing(_case(name), False, True, poison=False)
        want = per_problem_sum(c)
        for got in (WS.direct(*_args(c)), WS.chunked(*_args(c), 5, 4)):
            for key in KEYS[:1] + KEYS[2:]:
                assert _close(got[key], want[key]), (name, key)


def test_dropping_the_partner_and_pair_terms_fails_on_n7_only():
    for name, differs in (("n7", True), ("n24", False)):
        c = _sharing(_case(name), True, True, poison=False)
        want, got = per_problem_sum(c), WS.direct(*_args(c), partners=False)
        for key in ("J_blocks", "weights"):
            assert _close(got[key], want[key]) != differs, (name, key)
        if differs:   # ... and dweights without its pair term is the dense -s t, the per-problem reference with correction=False
            assert _close(got["weights"], per_problem_sum(c, correction=False)["weights"])
            full = WS.direct(*_args(c))
            assert _close(full["weights"], want["weights"]) and _close(full["J_blocks"], want["J_blocks"])


def test_every_problem_masked_and_the_empty_batch_give_zeros():
    c = _sharing(_case("n7"), False, False)
    none = dict(c, ok=np.zeros(c["B"], dtype=bool))
    for got in (WS.direct(*_args(none)), WS.chunked(*_args(none), 5)):
        for key in KEYS:
            assert np.all(np.asarray(got[key]) == 0), key
    empty = dict(c, V=c["V"][:0], U=c["U"][:0], R=c["R"][:0], Wt=c["Wt"][:0], ok=c["ok"][:0])
    for key, v in WS.chunked(*_args(empty), 1).items():
        assert np.all(np.asarray(v) == 0), key


@pytest.mark.parametrize("name", ["n7", "n24"])
def test_integer_data_gives_exactly_equal_results(name):
    c = _sharing(_case(name, integers=True), True, True, poison=False)
    want, got = per_problem_sum(c), WS.direct(*_args(c))
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), key
        for length in (4, 37):
            assert np.array_equal(WS.chunked(*_args(c), length)[key], want[key]), (key, length)


def test_bound_counts_the_roundings_and_covers_the_chunked_scheme():
    """The bound is a count (1.01 (2 B + 4 P_max + 8) units of the magnitude), linear in the magnitude, and the float64 chunked scheme lies
    inside it at every chunk length."""
    c = _sharing(_case("n7"), True, True, poison=False)
    mag = WS.direct(*_args(c), absolute=True)
    pmax = WS.p_max(c["cost"])
    assert pmax == 5
    tol = WS.bound(c["B"], pmax, UNIT[torch.float64], mag)
    assert np.allclose(tol["J_blocks"], 1.01 * (2 * 37 + 4 * 5 + 8) * 2.0 ** -53 * mag["J_blocks"], rtol=1e-15)
    want = WS.direct(*_args(c))
    for length in (1, 4, 37):
        got = WS.chunked(*_args(c), length)
        for key in KEYS:
            assert np.all(np.abs(got[key] - want[key]) <= tol[key]), (key, length)
