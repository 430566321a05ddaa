"""CPU checks of the batch-reduced gradients (mo_qp_gradients_shared): the two symbols, the chunked scheme against the masked sum of the
per-problem formulas, and the summed formulas against central differences of a loss over a batch that shares its data."""
import os
import re

import numpy as np
import pytest
import torch

from tests import diff_reference as R
from tests import shared_grad_reference as S
from tests.sens_fixed_problem import LAM, M, K, N, MR, cost, fixed_problem, root
from tests.sens_fixtures import UNIT

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_symbols_are_declared_and_exported():
    from mini_opt_amd import _lib as L
    L.build()
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "mini_opt_hip.h")).read()
    declared = set(re.findall(r"\b(mo_[a-z_]+)\s*\(", header))
    for name in ("mo_qp_gradients_shared_workspace", "mo_qp_gradients_shared"):
        assert name in declared and name in L.EXPORTS and hasattr(lib, name)
    import mini_opt_amd
    assert callable(mini_opt_amd.qp_gradients_shared)


def test_argument_errors_without_gpu():
    """What the call judges from its arguments alone needs no device: the input level and what the batch must share."""
    import ctypes as C
    from mini_opt_amd import _lib as L
    L.build()
    lib = L.lib()
    p16 = C.c_void_p(16)
    nbytes = C.c_int64(-1)
    qp = L.Problem()
    qp.G, qp.G_stride, qp.G_ld, qp.c, qp.c_stride = 16, 0, 8, 16, 8
    jl = L.Problem()
    jl.J, jl.J_stride, jl.J_ld, jl.J_layout, jl.r, jl.r_stride = 16, 32, 8, L.MO_ROW_MAJOR, 16, 4
    g = L.QPGrads()
    g.dG, g.dG_ld = 16, 8
    for prob, grads, word in ((jl, g, b"dG"),):
        assert lib.mo_qp_gradients_shared(None, C.byref(prob), 4, p16, 8, p16, 8, None, None, C.byref(grads), p16, 1 << 20, None) == -1
        assert word in lib.mo_last_error()
        assert lib.mo_qp_gradients_shared_workspace(None, C.byref(prob), 4, C.byref(grads), C.byref(nbytes)) == -1 and nbytes.value == -1
    g = L.QPGrads()
    g.dJ, g.dJ_ld, g.dJ_layout = 16, 8, L.MO_ROW_MAJOR
    assert lib.mo_qp_gradients_shared(None, C.byref(qp), 4, p16, 8, p16, 8, None, None, C.byref(g), p16, 1 << 20, None) == -1   # (G, c) input
    assert b"dJ" in lib.mo_last_error()
    assert lib.mo_qp_gradients_shared(None, C.byref(jl), 4, p16, 8, p16, 8, None, None, C.byref(g), p16, 1 << 20, None) == -1   # a J per problem
    assert b"J_stride" in lib.mo_last_error()
    assert lib.mo_qp_gradients_shared(None, C.byref(qp), 4, p16, 8, p16, 8, None, None, None, p16, 1 << 20, None) == -1
    assert b"out" in lib.mo_last_error()
    g = L.QPGrads()
    g.dc = 16
    assert lib.mo_qp_gradients_shared(None, C.byref(qp), 4, p16, 8, p16, 8, None, None, C.byref(g), p16, 1 << 20, None) == -1   # NULL plan
    assert b"plan" in lib.mo_last_error()


# ---- the front end (mini_opt_amd.diff): the partition of a backward, the member table, the filled struct ------------------------------------
def test_partition_of_the_backward():
    """(each, summed): what the batch shares goes to the reduced launch -- but r given once against a J per problem is computed per problem."""
    from mini_opt_amd import diff as D
    names = ["G", "c", "J", "r", "lam", "A_eq", "b_eq", "cons_a", "cons_b"]
    part = lambda want, shared: D._partition(want, frozenset(shared), "r", "J")
    assert part(names, names) == ([], names)                                             # everything shared
    assert part(names, ()) == (names, [])                                                # nothing shared
    assert part(["J", "r", "lam"], ["r"]) == (["J", "r", "lam"], [])                     # r shared, J per problem: each
    assert part(["r", "lam"], ["r", "lam"]) == (["r"], ["lam"])                          # ... also when J's gradient is not asked for
    assert part(["J", "r", "lam"], ["J", "r"]) == (["lam"], ["J", "r"])                  # r and J both shared: summed
    assert part(["c", "cons_a", "cons_b"], ["cons_a", "cons_b"]) == (["c"], ["cons_a", "cons_b"])
    assert part(["c", "cons_a", "cons_b"], ["c"]) == (["cons_a", "cons_b"], ["c"])
    assert part(["c", "b_eq"], ["A_eq", "G"]) == (["c", "b_eq"], [])                     # shared inputs whose gradient is not asked for


def test_member_table_against_the_structs():
    import ctypes as C
    from mini_opt_amd import _lib as L
    from mini_opt_amd import diff as D
    assert tuple(D._DENSE) == D.GRADIENTS == ("G", "c", "J", "r", "lam", "A_eq", "b_eq", "cons_a", "cons_b")
    for struct in (L.QPGrads, L.QPTangents):
        fields = dict(struct._fields_)
        for name, (ptr, stride, ld, _tail) in D._DENSE.items():
            assert fields[ptr] is C.c_void_p and fields[stride] is C.c_int64 and (ld is None or fields[ld] is C.c_int32), (struct, name)
    assert len({entry[0] for entry in D._DENSE.values()}) == 9                           # nine pointers ...
    assert D._DENSE["cons_a"][1] == D._DENSE["cons_b"][1] == "dcons_stride"            # ... cons_a and cons_b behind one stride
    assert D._DENSE["lam"][3](None) == ()


def _filled(struct, out, pointers, **values):
    """Every field of `struct`: the pointers of `out` under the fields named in `pointers`, `values`, and nothing else set."""
    import ctypes as C
    want = {f: (None if t is C.c_void_p else 0) for f, t in struct._fields_}
    want.update({field: out[name].data_ptr() for name, field in pointers.items()})
    want.update(values)
    assert {f: getattr(struct, f) for f, _ in struct._fields_} == want


@pytest.mark.parametrize("case", ["row", "row_padded", "col", "col_padded", "G"])
def test_gradient_struct_is_filled_as_before(case):
    """_dense_outputs on CPU tensors (no launch) for (n, k, m, m_r) = (7, 3, 4, 9), per problem at B = 5 and summed at 1, against the values
    qp_gradients / qp_gradients_shared set member by member before the table: strides n n, n, n k, k, m, rows ld, m_r, 1 per problem and
    none summed; dG_ld = n, dA_ld = k, dJ_ld and dJ_layout those of problem.J; a dJ with a padded leading dimension zero-filled."""
    from mini_opt_amd import _lib as L
    from mini_opt_amd import diff as D
    from mini_opt_amd import qp as Q
    n, k, m, m_r, B = 7, 3, 4, 9, 5
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    common = dict(n=n, k=k, m=m, A_eq=z(B, n, k), b_eq=z(B, k), cons_var=torch.zeros(B, m, dtype=torch.int32), cons_a=z(B, m), cons_b=z(B, m))
    rows, ld, layout = {"row": (m_r, n, L.MO_ROW_MAJOR), "row_padded": (m_r, n + 3, L.MO_ROW_MAJOR), "col": (n, m_r, L.MO_COL_MAJOR),
                        "col_padded": (n, m_r + 3, L.MO_COL_MAJOR), "G": (0, 0, 0)}[case]
    if case == "G":
        prob = Q.BatchedQP(G=z(B, n, n), c=z(B, n), **common)
        want, pointers = ("G", "c", "A_eq", "b_eq", "cons_b"), dict(G="dG", c="dc", A_eq="dA_eq", b_eq="db_eq", cons_b="dcons_b")
        lds = dict(dG_ld=7, dA_ld=3)
        strides = dict(dG_stride=49, dc_stride=7, dA_stride=21, db_stride=3, dcons_stride=4)
        shapes = dict(G=(7, 7), c=(7,), A_eq=(7, 3), b_eq=(3,), cons_b=(4,))
    else:
        prob = Q.BatchedQP(J=z(B, rows, ld), r=z(B, m_r), J_layout=case[:3], J_rows=m_r, **common)
        want, pointers = ("J", "r", "lam", "cons_a", "cons_b"), dict(J="dJ", r="dr", lam="dlambda", cons_a="dcons_a", cons_b="dcons_b")
        lds = dict(dJ_ld=ld, dJ_layout=layout)
        strides = dict(dJ_stride=rows * ld, dr_stride=9, dlambda_stride=1, dcons_stride=4)
        shapes = dict(J=(rows, ld), r=(9,), lam=(), cons_a=(4,), cons_b=(4,))
    assert prob.m_r == (0 if case == "G" else m_r)
    for lead, strided in ((B, True), (1, False)):
        out, g = D._dense_outputs(prob, want, lead, strided)
        assert isinstance(g, L.QPGrads) and tuple(out) == want
        for name in want:
            assert tuple(out[name].shape) == (lead, *shapes[name]) and out[name].dtype == torch.float64 and out[name].is_contiguous()
        _filled(g, out, pointers, **lds, **(strides if strided else {}))
        if case.endswith("padded"):
            assert bool(torch.all(out["J"] == 0))
    out, g = D._dense_outputs(prob, (), B, True)                                         # nothing asked for: nothing set
    _filled(g, out, {})


def test_chunk_count_is_a_function_of_batch_and_cus():
    assert [S.chunks(B, 256) for B in (0, 1, 31, 32, 33, 64, 65, 4096, 65536, 65537)] == [0, 1, 1, 1, 2, 2, 3, 128, 256, 256]
    assert S.chunk_len(65536, 256) == 256 and S.chunk_len(65, 256) == 22 and S.chunk_len(1, 256) == 1
    for B in (1, 5, 37, 1000, 70001):
        for cus in (1, 8, 256):
            length = S.chunk_len(B, cus)
            assert S.chunks(B, cus) <= cus and (S.chunks(B, cus) - 1) * length < B <= S.chunks(B, cus) * length   # the last chunk is not empty


@pytest.mark.parametrize("r_shared", [False, True], ids=["r_per_problem", "r_shared"])
def test_chunked_scheme_against_the_masked_sum_of_the_per_problem_formulas(r_shared):
    """B = 37 problems of (n, k, m, m_r) = (7, 3, 4, 9), every fifth masked with a row of NaN as its adjoint: per-chunk partials, the
    chunk-order sum and the finish formulas give the masked sum of diff_reference.gradients within 2 (B + n + 8) 2^-53 sum |a_p| |b_p|."""
    n, k, m, m_r, B = 7, 3, 4, 9, 37
    rng = np.random.default_rng(4087)
    V = rng.normal(size=(B, n + 2 * m + k))
    U = rng.normal(size=(B, n + 2 * m + k))
    var = rng.permutation(n)[:m]
    J = rng.normal(size=(m_r, n))
    Rr = rng.normal(size=(1 if r_shared else B, m_r))
    ok = np.arange(B) % 5 != 2
    U[~ok] = np.nan
    want = None
    for p in np.flatnonzero(ok):
        gp = R.gradients(n, k, m, var, V[p], U[p], J=J, r=Rr[0 if r_shared else p])
        want = gp if want is None else {key: want[key] + gp[key] for key in gp}
    _, mag = S.direct(n, k, m, var, V, U, ok, J=J, R=Rr)
    tol = S.bound(B, n, UNIT[torch.float64], mag)
    worst = 0.0
    for length in (4, 5, 37, S.chunk_len(B, 256)):
        got = S.chunked(n, k, m, var, V, U, ok, length, J=J, R=Rr)
        assert set(got) == set(want)
        for key in want:
            err = np.abs(got[key] - want[key])
            assert np.all(np.isfinite(got[key])) and np.all(err <= tol[key]), (key, length, err.max())
            worst = max(worst, float(np.max(err)))
        assert np.array_equal(got["G"], got["G"].T)
    print(f"largest |chunked - masked sum| = {worst:.3e}")


def _fd(loss, th, key, idx, h=1e-6, symmetric=False):
    vals = []
    for sign in (1.0, -1.0):
        t = {k_: (np.array(v_, dtype=float, copy=True) if isinstance(v_, np.ndarray) and v_.dtype.kind == "f" else v_) for k_, v_ in th.items()}
        t[key][idx] += sign * h
        if symmetric and idx[0] != idx[1]:
            t[key][idx[::-1]] += sign * h
        vals.append(loss(t))
    return (vals[0] - vals[1]) / (2 * h)


def test_summed_formulas_against_central_differences():
    """l(theta) = sum_p g_p . v*_p(theta) over three copies of the fixed problem that differ in c (and, J-level, in r): central differences
    over every entry of a shared G (symmetric perturbation), A_eq, a, b and of a shared J and lam.  Step 1e-6 and bound 1e-7 of the
    group's largest gradient entry, as test_diff_cpu."""
    base, g0 = fixed_problem()
    rng = np.random.default_rng(77)
    B = 3
    gs = [g0] + [rng.normal(size=g0.shape) for _ in range(B - 1)]
    G0, c0 = cost(base)
    cs = [c0 + 0.1 * p * rng.normal(size=N) for p in range(B)]
    rs = [base["r"] + 0.1 * p * rng.normal(size=MR) for p in range(B)]
    shared_qp = dict(G=G0.copy(), A=base["A"], b_eq=base["b_eq"], var=base["var"], a=base["a"], b=base["b"])
    shared_j = dict(J=base["J"], lam=np.array([LAM]), A=base["A"], b_eq=base["b_eq"], var=base["var"], a=base["a"], b=base["b"])
    v_qp = [root(dict(shared_qp, c=cs[p])) for p in range(B)]
    v_j = [root(dict(shared_j, r=rs[p])) for p in range(B)]

    def adjoints(vs, Gs):
        return np.stack([R.solve_transposed(R.kkt_matrix(Gs, base["A"], base["var"], base["a"], vs[p]), gs[p]) for p in range(B)])

    loss_qp = lambda th: sum(gs[p] @ root(dict(th, c=cs[p]), v_qp[p]) for p in range(B))
    loss_j = lambda th: sum(gs[p] @ root(dict(th, r=rs[p]), v_j[p]) for p in range(B))
    ok = np.ones(B, dtype=bool)
    grads = S.chunked(N, K, M, base["var"], np.stack(v_qp), adjoints(v_qp, G0), ok, 2)
    Gj = base["J"].T @ base["J"] + LAM * np.eye(N)
    grads_j = S.chunked(N, K, M, base["var"], np.stack(v_j), adjoints(v_j, Gj), ok, 2, J=base["J"], R=np.stack(rs))
    worst = {}

    def group(name, loss, th, key, analytic, symmetric=False):
        fd = np.zeros_like(analytic)
        for idx in np.ndindex(*analytic.shape):
            fd[idx] = _fd(loss, th, key, idx, symmetric=symmetric)
        want = analytic + analytic.T - np.diag(np.diag(analytic)) if symmetric else analytic   # both mirror entries move
        worst[name] = np.max(np.abs(fd - want)) / np.max(np.abs(want))
        print(f"{name}: max |fd - analytic| / max |analytic| = {worst[name]:.3e}")

    group("G", loss_qp, shared_qp, "G", grads["G"], symmetric=True)
    group("A_eq", loss_qp, shared_qp, "A", grads["A_eq"])
    group("cons_a", loss_qp, shared_qp, "a", grads["cons_a"])
    group("cons_b", loss_qp, shared_qp, "b", grads["cons_b"])
    group("J", loss_j, shared_j, "J", grads_j["J"])
    group("lam", loss_j, shared_j, "lam", np.array([grads_j["lam"]]))
    assert max(worst.values()) < 1e-7, worst
