"""Where a problem batch lives in memory (test infrastructure, not product code): the case table of tests/test_layout_dispatch_cpu.py and
tests/test_gpu_layouts.py, and the three layouts of one batch of B = 9 problems that both tests use.

 packed     what mini_opt_amd.qp.BatchedQP.as_struct() writes: stride = extent, G_ld = n, A_ld = k, cons_stride = m, bases as allocated
 scattered  every array in a buffer of its own, filled with a canary; a pad of its own per problem row (so that no two arrays share a
            stride), leading dimensions beyond the extent, the base an ODD number of elements into the allocation (fp64: 8 bytes off a
            16-byte boundary, fp32 / int32: 4 bytes off), a guard of more than two whole problem rows behind the last row.  J comes in two
            variants: "scattered" keeps what the selector looks at (16-byte aligned base, J_ld = n, an even / multiple-of-4 stride), so the
            same instantiation runs as for the packed layout and the results must be the same bits; "moved" has an odd stride (fp64: the
            gather stream, fp32: the generic kernel).
 shared     every input has stride 0: one J, r, G, c, A_eq, b_eq, constraint set and mu for the whole batch, no lambda_vec; only the state
            differs per problem.

The numbers of a layout (layout()) are plain Python, so the CPU test can hand them to the selector; Buf / Env put a batch on the device."""
import collections
import ctypes as C
import functools

import numpy as np

B = 9
CANARY = -777.25                 # the floating-point canary (as tests/test_gpu_fused_rhs.py)
CANARY_I32 = -0x5A5A5A5B         # int32 buffers: no valid index, status or count

# mo::Mode, mo::FusedFamily, the J streams and mo::KernelKind (csrc/mo_kernels.h, csrc/mo_fused_select.h)
MODE_LINEARIZE, MODE_RESIDUAL, MODE_STEP, MODE_ITERATE, MODE_SOLVE = range(5)
FUSED_STEP, FUSED_SOLVE, FUSED_LINEARIZE, FUSED_TINY = range(4)
JMODE_VECTOR, JMODE_FLAT, JMODE_GATHER = range(3)
KERNEL_GENERIC, KERNEL_FUSED_F64, KERNEL_FUSED_F32 = range(3)
STEP_NO_INEQUALITIES = 1
COMPLEMENTARITY, PREDICTOR_CORRECTOR = 0, 2
KEY_FIELDS = ("family", "nt", "wps", "qpl", "mc", "jmode", "ny", "pck", "f32", "pad")

# One row of the table.  key: the FusedKey mo_newton_step is meant to select for the case's FIRST level in the packed layout (None: the generic
# kernel); unit: the translation unit that key lives in.  moved: the case also runs with the moved J stream.  J_extra: row-major J with
# J_ld = n + J_extra in every layout.
Case = collections.namedtuple("Case", "id dtype levels shape key unit moved force_generic no_tiny J_extra")


def _case(id, dtype, levels, shape, key, unit, moved=False, force_generic=False, no_tiny=False, J_extra=0):
    return Case(id, dtype, levels, shape, key, unit, moved, force_generic, no_tiny, J_extra)


#                id          dtype  levels  (n, k, m, m_r)        family      nt wps qpl mc jmode      ny pck f32 pad   unit
# (m_r a little off the issue's table -- 26 / 28 for 24, 46 for 44, 62 for 60, 76 for 72, 12 for 8 -- wherever its r_stride = m_r + 1 would equal
# its c_stride = n + 5 or its cons_stride = m + 1)
CASES = [
    _case("tiny",     "f64", "JG", (8, 2, 4, 16),     (FUSED_TINY, 1, 3, 0, 1, JMODE_VECTOR, 1, 1, 0, 0), "tiny"),
    _case("n32",      "f64", "JG", (20, 3, 10, 26),   (FUSED_STEP, 2, 4, 0, 1, JMODE_VECTOR, 1, 1, 0, 0), "main", moved=True),
    _case("flat",     "f64", "J",  (31, 3, 7, 33),    (FUSED_STEP, 2, 3, 0, 1, JMODE_FLAT, 1, 1, 0, 0), "main"),
    _case("gather",   "f64", "J",  (32, 4, 16, 64),   (FUSED_STEP, 2, 4, 0, 1, JMODE_GATHER, 1, 1, 0, 0), "gather", J_extra=5),
    _case("diag4",    "f64", "J",  (64, 8, 32, 128),  (FUSED_STEP, 4, 3, 0, 1, JMODE_VECTOR, 1, 1, 0, 0), "main", moved=True),
    _case("diag4pad", "f64", "J",  (50, 8, 32, 13),   (FUSED_STEP, 4, 3, 0, 1, JMODE_VECTOR, 1, 1, 0, 0), "main"),
    _case("ny2",      "f64", "J",  (32, 16, 40, 64),  (FUSED_STEP, 2, 3, 0, 2, JMODE_VECTOR, 2, 1, 0, 0), "ny2"),
    # (34 variables, not the issue's 32: the lean two-slot Solve kernel exists on the 64 grid only, and this is the case that reaches it)
    _case("mc2",      "f64", "J",  (34, 4, 65, 36),   (FUSED_STEP, 4, 2, 0, 2, JMODE_VECTOR, 1, 1, 0, 0), "main"),
    _case("mc4",      "f64", "G",  (20, 3, 129, 0),   (FUSED_STEP, 2, 3, 1, 4, JMODE_VECTOR, 1, 1, 0, 0), "mc4"),
    _case("ny3",      "f64", "J",  (40, 33, 8, 46),   (FUSED_STEP, 4, 1, 0, 2, JMODE_VECTOR, 3, 1, 0, 0), "ny34"),
    _case("ny4",      "f64", "J",  (56, 48, 8, 62),   (FUSED_STEP, 4, 1, 0, 2, JMODE_VECTOR, 4, 1, 0, 0), "ny34"),
    _case("n96",      "f64", "J",  (66, 4, 10, 72),   (FUSED_STEP, 6, 2, 0, 1, JMODE_VECTOR, 1, 1, 0, 0), "main", moved=True),
    _case("n128",     "f64", "J",  (98, 4, 10, 100),  (FUSED_STEP, 8, 1, 0, 1, JMODE_VECTOR, 1, 1, 0, 0), "main"),
    _case("f32-64",   "f32", "JG", (64, 8, 32, 128),  (FUSED_STEP, 4, 3, 0, 1, JMODE_VECTOR, 1, 1, 1, 0), "f32", moved=True),
    _case("f32-pad",  "f32", "JG", (20, 4, 10, 28),   (FUSED_STEP, 4, 3, 0, 1, JMODE_VECTOR, 1, 1, 1, 1), "f32"),
    _case("f32-128",  "f32", "JG", (68, 4, 8, 76),    (FUSED_STEP, 8, 2, 0, 1, JMODE_VECTOR, 1, 1, 1, 1), "f32"),
    _case("gen-f64",  "f64", "JG", (20, 3, 10, 26),   None, "generic", force_generic=True),
    _case("gen-f32",  "f32", "JG", (20, 3, 10, 26),   None, "generic", force_generic=True),
    _case("gen-large", "f64", "J", (190, 6, 8, 12),   None, "generic-large"),
]
BY_ID = {c.id: c for c in CASES}
ITEMS = [(c.id, level) for c in CASES for level in c.levels]            # every (case, input level)


def elem(case):
    return 8 if case.dtype == "f64" else 4


# ---- the numbers of a layout ---------------------------------------------------------------------------------------------------------------
# name -> (inner, outer): `outer` rows of `inner` elements, leading dimension ld >= inner between the rows.  Matrices in the memory order of
# the C ABI: G, A_eq, G_out column-major (outer = columns), J row-major (outer = rows).
def shapes(case):
    n, k, m, m_r = case.shape
    V = n + 2 * m + k
    return {"J": (n, m_r), "r": (m_r, 1), "G": (n, n), "c": (n, 1), "A": (k, n), "b": (k, 1), "cons": (m, 1), "lam": (1, 1), "vars": (V, 1),
            "mu": (1, 1), "delta": (V, 1), "r_out": (V, 1), "G_out": (n, n), "c_out": (n, 1), "x": (n, 1), "cons_b_out": (m, 1), "x_out": (n, 1)}


Arr = collections.namedtuple("Arr", "offset stride ld guard")   # all in elements; stride 0: one instance for the batch


def layout(case, variant, r_aligned=False):
    """name -> Arr for `variant` in packed / scattered / moved / shared.  r_aligned: r keeps a 16-byte aligned base and a stride divisible by
    4 (what fused_f32_supported asks of mo_linearize in fp32)."""
    n, k, m, m_r = case.shape
    V = n + 2 * m + k
    sh = shapes(case)
    J_ld = n + case.J_extra
    vec = 2 if case.dtype == "f64" else 4                       # elements of a 16-byte piece
    out = {}
    if variant == "packed":
        for name, (inner, outer) in sh.items():
            out[name] = Arr(0, inner * outer, inner, 0)
        out["J"] = Arr(0, m_r * J_ld, J_ld, 0)
        return out
    if variant == "shared":                                     # inputs: stride 0, bases as allocated; state and outputs stay packed
        out = layout(case, "packed")
        for name in ("J", "r", "G", "c", "A", "b", "cons", "mu"):
            out[name] = out[name]._replace(stride=0)
        return out
    assert variant in ("scattered", "moved")
    ld = {"G": n + 3, "A": k + 1 if k else 0, "G_out": n + 2, "J": J_ld}
    fixed = {"cons": m + 1, "b": k + 2, "c": n + 5, "r": m_r + 1, "lam": 2, "mu": 3, "vars": V + 3, "delta": V + 7, "r_out": V + 5}
    taken = set(fixed.values())
    for index, (name, (inner, outer)) in enumerate(sh.items()):
        l = ld.get(name, inner)
        stride = fixed.get(name, l * outer + 3 + index)         # a deterministic pad of 3 + index elements ...
        while name not in fixed and stride in taken:            # ... and one more wherever another array has that stride already
            stride += 1
        taken.add(stride)
        out[name] = Arr(1, stride, l, 2 * stride + 16)
    if variant == "scattered":                                  # the same stream: what fused_needs_gather / fused_f32_supported look at is kept
        stride = m_r * J_ld + vec
        out["J"] = Arr(vec, stride, J_ld, 2 * stride + 16)
    else:                                                       # moved: an odd stride
        stride = m_r * J_ld + (1 if (m_r * J_ld) % 2 == 0 else 2)
        out["J"] = Arr(1, stride, J_ld, 2 * stride + 16)
    if r_aligned:
        stride = (m_r + 4) & ~3
        while stride in {a.stride for name, a in out.items() if name != "r"}:
            stride += 4
        out["r"] = Arr(4, stride, m_r, 2 * stride + 16)
    return out


def assert_distinct_strides(case, lay, names):
    """No two of the arrays `names` of a scattered layout share a stride (empty arrays aside)."""
    sh = shapes(case)
    strides = [lay[name].stride for name in set(names) if sh[name][0] * sh[name][1] > 0]
    assert len(set(strides)) == len(strides), (case.id, {name: lay[name].stride for name in names})


# ---- problem data --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_data(case_id, shared=False):
    """The inputs of a case as float64 numpy arrays (make_case of tests/test_gpu_fused_diag.py; fp32 cases rounded through float32 as the
    fp32 tests do): lambda 0.5 where J has fewer rows than variables, else 1e-3 -- per problem lam_vec = lambda (1 + p / 10), mu = 0.05
    (1 + p / 10).  shared: problem 0's inputs for every problem, one scalar lambda and one mu; the state still differs per problem."""
    case = BY_ID[case_id]
    n, k, m, m_r = case.shape
    mr = m_r if m_r else 2 * n                                  # (G, c) only cases: G from a J of their own
    rng = np.random.default_rng(4000 + [c.id for c in CASES].index(case_id))
    f = (lambda a: a.astype(np.float32).astype(np.float64)) if case.dtype == "f32" else (lambda a: a)
    J = f(rng.uniform(-1, 1, (B, mr, n))); r = f(rng.uniform(-1, 1, (B, mr)))
    A = f(rng.uniform(-1, 1, (B, n, k))); b = f(rng.uniform(-1, 1, (B, k)))
    cv = rng.integers(0, n, (B, m)).astype(np.int32); ca = rng.choice([-1.0, 1.0, 2.0], (B, m)); cb = f(rng.uniform(0.5, 2.0, (B, m)))
    x = rng.uniform(-0.1, 0.1, (B, n)); sl = rng.uniform(0.2, 1.5, (B, m)); z = rng.uniform(0.1, 2, (B, m)); y = rng.uniform(-1, 1, (B, k))
    vars_ = f(np.concatenate([x, sl, y, z], axis=1))
    scale = 1.0 + np.arange(B) / 10.0
    lam = f((1e-3 if mr >= n else 0.5) * scale); mu = f(0.05 * scale)
    if shared:
        J, r, A, b, cv, ca, cb = (np.repeat(a[:1], B, axis=0) for a in (J, r, A, b, cv, ca, cb))
        lam = np.repeat(lam[:1], B); mu = np.repeat(mu[:1], B)
    G = f(np.einsum("bqi,bqj->bij", J, J) + lam[:, None, None] * np.eye(n))          # symmetric: [b, col, row] is its column-major memory
    c = f(np.einsum("bqi,bq->bi", J, r))
    d = dict(J=J, r=r, A=A, b=b, cv=cv, ca=ca, cb=cb, vars=vars_, lam=lam, mu=mu, G=G, c=c)
    for a in d.values():
        a.setflags(write=False)
    return d


# ---- a batch on the device -------------------------------------------------------------------------------------------------------------------
class Buf:
    """One array of the batch in a buffer of its own: element (p, o, i) at offset + p stride + o ld + i; everything else -- the elements in
    front of the base, the pads between rows and columns, the guard -- holds the canary."""

    def __init__(self, batch, inner, outer, arr, dtype, device, data=None):
        import torch
        self.torch = torch
        rows = 1 if arr.stride == 0 else batch
        extent = (outer - 1) * arr.ld + inner if inner * outer else 0
        total = arr.offset + (rows - 1) * arr.stride + extent + arr.guard
        self.canary = CANARY_I32 if dtype == torch.int32 else CANARY
        self.buf = torch.full((max(total, 1),), self.canary, dtype=dtype, device=device)
        ar = lambda count: torch.arange(count, device=device, dtype=torch.int64)
        self.index = (arr.offset + ar(rows)[:, None, None] * arr.stride + ar(outer)[None, :, None] * arr.ld + ar(inner)[None, None, :]).reshape(rows, -1)
        self.shape = (rows, outer, inner)
        self.is_data = torch.zeros(max(total, 1), dtype=torch.bool, device=device)
        self.is_data[self.index.reshape(-1)] = True
        self.arr = arr
        self.lay_name = None             # the array of layout() this buffer follows (None: a record array without a stride of its own)
        if data is not None:
            t = torch.tensor(np.asarray(data), device=device).to(dtype).reshape(-1, outer * inner)[:rows]
            self.buf[self.index.reshape(-1)] = t.reshape(-1)
        self.before = self.buf.clone()

    @property
    def ptr(self):
        """The base address (NULL for an empty array)."""
        if self.index.numel() == 0:
            return None
        return C.c_void_p(self.buf.data_ptr() + self.arr.offset * self.buf.element_size())

    def address(self):
        return self.buf.data_ptr() + self.arr.offset * self.buf.element_size()

    def get(self):
        """The data elements, [rows, outer * inner], contiguous."""
        return self.buf[self.index.reshape(-1)].reshape(self.shape[0], -1)

    def canaries_intact(self):
        return bool(self.torch.equal(bits(self.buf[~self.is_data]), bits(self.before[~self.is_data])))

    def unchanged(self):
        return bool(self.torch.equal(bits(self.buf), bits(self.before)))


def bits(t):
    import torch
    return t.contiguous().view(torch.uint8)


def same_bits(a, b):
    """As _same_bits of tests/test_gpu_queue_coverage.py."""
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


class Env:
    """The inputs of one (case, level) in one layout on the device, the mo_problem that describes them, and the output buffers of the calls
    made on it.  check() asserts that no call changed an input or touched a canary."""

    def __init__(self, case, level, variant, data, device, r_aligned=False, wrong_lambda=True):
        import torch
        from mini_opt_amd import _lib as L
        self.case, self.level, self.variant, self.device = case, level, variant, device
        self.dt = torch.float64 if case.dtype == "f64" else torch.float32
        self.lay = layout(case, variant, r_aligned)
        self.sh = shapes(case)
        n, k, m, m_r = case.shape
        self.inputs, self.outputs = {}, {}
        put = self._input
        p = L.Problem()
        if level == "J":
            J = np.full((B, m_r, n + case.J_extra), 7.7); J[:, :, :n] = data["J"]          # (columns beyond n: never read)
            self.inputs["J"] = Buf(B, n + case.J_extra, m_r, self.lay["J"], self.dt, device, J)
            self.inputs["J"].lay_name = "J"
            put("r", data["r"])
            p.J, p.J_stride, p.J_ld, p.J_layout = self.inputs["J"].ptr, self.lay["J"].stride, self.lay["J"].ld, L.MO_ROW_MAJOR
            p.r, p.r_stride = self.inputs["r"].ptr, self.lay["r"].stride
            if variant == "shared":
                p.lam = float(data["lam"][0])
            else:                                                  # per-problem damping; the scalar is wrong and must be ignored
                put("lam", data["lam"])
                p.lam = 123.0 if wrong_lambda else float(data["lam"][0])
                p.lambda_vec, p.lambda_stride = self.inputs["lam"].ptr, self.lay["lam"].stride
        else:
            put("G", data["G"]); put("c", data["c"])
            p.G, p.G_stride, p.G_ld = self.inputs["G"].ptr, self.lay["G"].stride, self.lay["G"].ld
            p.c, p.c_stride = self.inputs["c"].ptr, self.lay["c"].stride
        if k:
            put("A", data["A"]); put("b", data["b"])
            p.A_eq, p.A_stride, p.A_ld = self.inputs["A"].ptr, self.lay["A"].stride, self.lay["A"].ld
            p.b_eq, p.b_stride = self.inputs["b"].ptr, self.lay["b"].stride
        if m:
            put("cons_var", data["cv"], "cons", torch.int32); put("cons_a", data["ca"], "cons"); put("cons_b", data["cb"], "cons")
            p.cons_var, p.cons_a, p.cons_b = (self.inputs[name].ptr for name in ("cons_var", "cons_a", "cons_b"))
            p.cons_stride = self.lay["cons"].stride
        put("mu", data["mu"])
        put("vars", data["vars"])
        self.prob = p

    def _input(self, name, data, lay=None, dtype=None):
        inner, outer = self.sh[lay or name]
        self.inputs[name] = Buf(B, inner, outer, self.lay[lay or name], dtype or self.dt, self.device, data)
        self.inputs[name].lay_name = lay or name
        return self.inputs[name]

    def state(self, data):
        """A fresh in / out state (mo_iterate and mo_qp_solve update it in place)."""
        return self.out("state", lay="vars", data=data)

    def out(self, name, width=None, dtype=None, lay=None, data=None, batch=B):
        """An output buffer: one of the arrays of layout(), or a [batch][width] record array the C ABI gives no stride (packed: as
        allocated; every other layout: 16-byte aligned, 4 canaries in front and 16 + 2 width behind)."""
        if width is None:
            inner, outer = self.sh[lay or name]
            arr = self.lay[lay or name]
        else:
            inner, outer = width, 1
            arr = Arr(0, width, width, 0) if self.variant in ("packed", "shared") else Arr(4, width, width, 2 * width + 16)
        self.outputs[name] = Buf(batch, inner, outer, arr, dtype or self.dt, self.device, data)
        self.outputs[name].lay_name = None if width is not None else (lay or name)
        return self.outputs[name]

    def check(self, tag=""):
        if self.variant in ("scattered", "moved"):
            assert_distinct_strides(self.case, self.lay, [buf.lay_name for bufs in (self.inputs, self.outputs) for buf in bufs.values() if buf.lay_name])
        for name, buf in self.inputs.items():
            assert buf.unchanged(), (self.case.id, self.level, self.variant, tag, "input changed", name)
        for name, buf in self.outputs.items():
            assert buf.canaries_intact(), (self.case.id, self.level, self.variant, tag, "canary touched", name)

    def alignments(self):
        """name -> base address % 16 of every input."""
        return {name: buf.address() % 16 for name, buf in self.inputs.items() if buf.index.numel()}
