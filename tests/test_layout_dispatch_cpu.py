"""Which kernel serves the calls of tests/test_gpu_layouts.py, decided on the CPU: every case of tests/layout_cases.py, in every mode the GPU
test runs and in each of its memory layouts (packed, scattered, moved J stream, shared), goes through mo::decide_kernel
(tests/cpp/layout_dispatch_driver.cpp against the current sources, linked with the host-only objects of the fused units and of the generic
kernel; nothing is launched).  What the GPU test relies on is asserted here: the packed, the same-stream scattered and the shared layout of a
call select the SAME instantiation (so the GPU test may ask for the same bits); each case reaches the family, grid, stream, y tiles and slots
its row names; the moved stream goes where mo_fused_select.h says; and together the cases touch every translation unit.  The distinct keys
are printed with the cases that select them."""
import os
import subprocess

import pytest

from tests import layout_cases as LC
from tests import solve_param_cases as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mini_opt_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
UNITS = ["kkt_fused", "kkt_fused_gather", "kkt_fused_ny2", "kkt_fused_ny34", "kkt_fused_mc4", "kkt_fused_tiny", "kkt_fused_f32", "kkt_generic"]
# (label, mode, flags, barrier strategy): the calls of the GPU test
CALLS = [("step", LC.MODE_STEP, 0, LC.COMPLEMENTARITY), ("step-noineq", LC.MODE_STEP, LC.STEP_NO_INEQUALITIES, LC.COMPLEMENTARITY),
         ("residual", LC.MODE_RESIDUAL, 0, LC.COMPLEMENTARITY), ("iterate", LC.MODE_ITERATE, 0, LC.COMPLEMENTARITY),
         ("iterate-pc", LC.MODE_ITERATE, 0, LC.PREDICTOR_CORRECTOR), ("solve", LC.MODE_SOLVE, 0, LC.COMPLEMENTARITY),
         ("solve-pc", LC.MODE_SOLVE, 0, LC.PREDICTOR_CORRECTOR), ("linearize", LC.MODE_LINEARIZE, 0, LC.COMPLEMENTARITY)]
BASE = 0x7f0000100000    # what an allocator hands out: far more than 16-byte aligned


def variants_of(case, call):
    out = ["packed", "scattered", "shared"] + (["moved"] if case.moved else [])
    if call == "linearize" and case.dtype == "f32":
        out.append("moved-r")          # the scattered layout with r 4 bytes off a 16-byte boundary: fused_f32_supported asks 16
    return out


def line_of(case, level, call, mode, flags, strategy, variant):
    n, k, m, m_r = case.shape
    if mode == LC.MODE_LINEARIZE:
        k = m = 0                      # mo_linearize works on the cost alone
    f32_linearize = mode == LC.MODE_LINEARIZE and case.dtype == "f32"
    lay = LC.layout(case, "scattered" if variant == "moved-r" else variant, r_aligned=f32_linearize and variant == "scattered")
    e = LC.elem(case)
    addr, here = {}, BASE
    for name, arr in lay.items():      # one allocation per array, the base `offset` elements into it
        addr[name] = here + arr.offset * e
        here += 1 << 20
    J = level == "J"
    tok = dict(label="%s|%s|%s|%s" % (case.id, level, call, variant), n=n, k=k, m=m, m_r=m_r if J else 0, dtype=0 if case.dtype == "f64" else 1,
               force_generic=int(case.force_generic), no_tiny=int(case.no_tiny), mode=mode, flags=flags, strategy=strategy, batch=LC.B,
               J=addr["J"] if J else 0, J_stride=lay["J"].stride, J_ld=lay["J"].ld, r=addr["r"] if J else 0, r_stride=lay["r"].stride,
               lam=addr["lam"] if J and variant != "shared" else 0, lam_stride=lay["lam"].stride,
               G=0 if J else addr["G"], G_stride=lay["G"].stride, G_ld=lay["G"].ld, c=0 if J else addr["c"], c_stride=lay["c"].stride,
               A=addr["A"] if k else 0, A_stride=lay["A"].stride, A_ld=lay["A"].ld, b=addr["b"] if k else 0, b_stride=lay["b"].stride,
               cons_var=addr["cons"] if m else 0, cons_a=addr["cons"] if m else 0, cons_b=addr["cons"] if m else 0, cons_stride=lay["cons"].stride,
               vars=addr["vars"], vars_stride=lay["vars"].stride, mu=addr["mu"], mu_stride=lay["mu"].stride,
               delta=addr["delta"] if mode in (LC.MODE_STEP, LC.MODE_ITERATE) else 0, delta_stride=lay["delta"].stride,
               r_out=addr["r_out"] if mode == LC.MODE_RESIDUAL else 0, r_out_stride=lay["r_out"].stride,
               G_out=addr["G_out"] if mode == LC.MODE_LINEARIZE else 0, G_out_stride=lay["G_out"].stride, G_out_ld=lay["G_out"].ld,
               c_out=addr["c_out"] if mode == LC.MODE_LINEARIZE else 0, c_out_stride=lay["c_out"].stride)
    if variant in ("scattered", "moved", "moved-r"):          # the alignments the scattered layout promises, on the addresses the driver sees
        odd = [name for name in ("r", "G", "c", "A", "b", "cons", "lam", "vars", "mu", "delta", "r_out", "G_out", "c_out")
               if not (name == "r" and f32_linearize and variant == "scattered")]
        assert all(addr[name] % 16 == e for name in odd), (case.id, variant)
        assert addr["J"] % 16 == (e if variant == "moved" else 0)
    return " ".join("%s=%d" % (key, val) if key != "label" else "label=%s" % val for key, val in tok.items())


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """run(name, lines) -> {(case id, level, call, variant): record}: the driver, built once, on a file of lines."""
    out = tmp_path_factory.mktemp("layout_dispatch")
    jobs = [(u, subprocess.Popen([HIPCC, "--cuda-host-only", "-O0", "-std=c++17", "-w", "-c", os.path.join(CSRC, u + ".hip"), "-o", str(out / (u + ".o"))],
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)) for u in UNITS]
    jobs.append(("driver", subprocess.Popen([HIPCC, "--cuda-host-only", "-O1", "-std=c++17", "-x", "hip", "-c",
                                             os.path.join(ROOT, "tests", "cpp", "layout_dispatch_driver.cpp"), "-o", str(out / "driver.o")],
                                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for name, job in jobs:
        text = job.communicate(timeout=900)[0]
        assert job.returncode == 0, (name, text[-4000:])
    exe = str(out / "driver")
    res = subprocess.run([HIPCC, "-Wl,--unresolved-symbols=ignore-all", "-o", exe] + [str(out / (n + ".o")) for n, _ in jobs], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]

    def run(name, lines):
        with open(out / name, "w") as f:
            f.write("\n".join(lines) + "\n")
        res = subprocess.run([exe, str(out / name)], capture_output=True, text=True, timeout=900)
        assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
        got = {}
        for row in res.stdout.splitlines():
            cols = row.split("\t")
            label = tuple(cols[0].split("|"))
            got[label] = dict(kind=int(cols[1]), key=tuple(map(int, cols[2:12])), found=int(cols[12]), unit=cols[13], large=int(cols[14]), name=cols[15])
        assert len(got) == len(lines)
        return got
    return run


@pytest.fixture(scope="module")
def decisions(driver):
    """{(case id, level, call, variant): record} of every call of the GPU layout test."""
    lines = []
    for case in LC.CASES:
        for level in case.levels:
            for call, mode, flags, strategy in CALLS:
                if call == "linearize" and level != "J":
                    continue
                lines += [line_of(case, level, call, mode, flags, strategy, variant) for variant in variants_of(case, call)]
    return driver("cases.txt", lines)


def test_packed_scattered_and_shared_layouts_select_the_same_instantiation(decisions):
    for (cid, level, call, variant), d in decisions.items():
        if variant not in ("scattered", "shared"):
            continue
        packed = decisions[cid, level, call, "packed"]
        assert (d["kind"], d["key"], d["name"], d["large"]) == (packed["kind"], packed["key"], packed["name"], packed["large"]), (cid, level, call, variant, d, packed)
    for label, d in decisions.items():
        if d["kind"] != LC.KERNEL_GENERIC:
            assert d["found"] == 1, ("rows of the unit's table with this key", label, d)     # exactly one row per key


def test_each_case_selects_what_its_row_names(decisions):
    for case in LC.CASES:
        for i, level in enumerate(case.levels):
            d = decisions[case.id, level, "step", "packed"]
            if case.key is None:
                assert d["kind"] == LC.KERNEL_GENERIC and d["name"] == "generic", (case.id, d)
                assert d["large"] == (case.unit == "generic-large"), (case.id, d)
                for call in ("residual", "iterate", "iterate-pc", "solve", "solve-pc"):
                    assert decisions[case.id, level, call, "packed"]["kind"] == LC.KERNEL_GENERIC
                continue
            want = dict(zip(LC.KEY_FIELDS, case.key))
            if i > 0 and want["family"] != LC.FUSED_TINY:
                want["qpl"] = 1                                     # the (G, c) twin of the row's key
            if case.dtype == "f32" and level == "G":               # the fp32 step kernel takes J-level input only; Solve / Iterate / residual take both
                assert d["kind"] == LC.KERNEL_GENERIC, (case.id, d)
            else:
                assert d["kind"] == (LC.KERNEL_FUSED_F32 if case.dtype == "f32" else LC.KERNEL_FUSED_F64), (case.id, level, d)
                assert d["key"] == tuple(want[f] for f in LC.KEY_FIELDS) and d["unit"] == case.unit, (case.id, level, d, want)
                assert decisions[case.id, level, "step-noineq", "packed"]["key"] == d["key"]
            # Solve / Iterate / residual: the Solve family on the same grid, stream and y tiles (the one-tile kernel and fp32: the same unit)
            for call in ("residual", "iterate", "iterate-pc", "solve", "solve-pc"):
                s = dict(zip(LC.KEY_FIELDS, decisions[case.id, level, call, "packed"]["key"]))
                assert decisions[case.id, level, call, "packed"]["kind"] != LC.KERNEL_GENERIC, (case.id, level, call)
                assert s["family"] == (LC.FUSED_TINY if want["family"] == LC.FUSED_TINY else LC.FUSED_SOLVE), (case.id, level, call, s)
                assert (s["nt"], s["jmode"], s["ny"], s["f32"], s["pad"]) == (want["nt"], want["jmode"], want["ny"], want["f32"], want["pad"]), (case.id, level, call, s)
                assert s["qpl"] == (0 if case.dtype == "f32" or want["family"] == LC.FUSED_TINY else int(level == "G"))
    # both strategies of the Solve kernel's second solve: the lean instantiations (pck = 0) under COMPLEMENTARITY, pck = 1 under PREDICTOR_CORRECTOR
    for cid in ("ny2", "mc2"):
        for call, pck in (("solve", 0), ("iterate", 0), ("residual", 0), ("solve-pc", 1), ("iterate-pc", 1)):
            assert dict(zip(LC.KEY_FIELDS, decisions[cid, "J", call, "packed"]["key"]))["pck"] == pck, (cid, call)
    lean = {d["key"] for (cid, level, call, variant), d in decisions.items() if d["kind"] == LC.KERNEL_FUSED_F64 and d["key"][7] == 0}
    assert len(lean) == 2, lean
    # the standalone linearisation: fused fp64 for every J-level case up to n = 128 (odd n on the gather stream), fp32 at n = 64
    for case in LC.CASES:
        if "J" not in case.levels:
            continue
        d = decisions[case.id, "J", "linearize", "packed"]
        n = case.shape[0]
        if case.force_generic or n > 128 or (case.dtype == "f32" and n != 64):
            assert d["kind"] == LC.KERNEL_GENERIC, (case.id, d)
        else:
            key = dict(zip(LC.KEY_FIELDS, d["key"]))
            assert key["family"] == LC.FUSED_LINEARIZE and key["f32"] == (case.dtype == "f32"), (case.id, d)
            if case.dtype == "f64":
                assert key["jmode"] == (LC.JMODE_GATHER if n % 2 or case.J_extra else LC.JMODE_VECTOR), (case.id, d)


def test_the_moved_stream_goes_where_the_selector_says(decisions):
    seen = 0
    for (cid, level, call, variant), d in decisions.items():
        if variant not in ("moved", "moved-r"):
            continue
        seen += 1
        case = LC.BY_ID[cid]
        packed = decisions[cid, level, call, "packed"]
        if level == "G":                                            # no J: nothing moves
            assert (d["kind"], d["key"]) == (packed["kind"], packed["key"])
        elif case.dtype == "f32":
            assert d["kind"] == LC.KERNEL_GENERIC and d["name"] == "generic", (cid, call, variant, d)
        else:
            key, was = dict(zip(LC.KEY_FIELDS, d["key"])), dict(zip(LC.KEY_FIELDS, packed["key"]))
            assert d["kind"] == LC.KERNEL_FUSED_F64 and key["jmode"] == LC.JMODE_GATHER and d["unit"] == "gather", (cid, call, d)
            assert (key["family"], key["nt"], key["ny"], key["qpl"]) == (was["family"], was["nt"], was["ny"], was["qpl"])
    assert seen >= 20


def test_the_cases_touch_every_translation_unit(decisions, capsys):
    units, keys = set(), {}
    for (cid, level, call, variant), d in sorted(decisions.items()):
        unit = "generic-large" if d["large"] else d["unit"]
        units.add(unit)
        keys.setdefault((unit, d["key"] if d["kind"] != LC.KERNEL_GENERIC else (), d["name"]), set()).add("%s-%s %s%s" % (cid, level, call, "" if variant == "packed" else " (" + variant + ")"))
    with capsys.disabled():
        print("\ndistinct keys the layout cases select (unit: family nt wps qpl mc jmode ny pck f32 pad, name <- case-level call):")
        for (unit, key, name), users in sorted(keys.items()):
            packed = sorted(u for u in users if "(" not in u)
            others = sorted(u for u in users if "(" in u)
            print("  %-13s %-30s %-26s <- %s" % (unit, " ".join(map(str, key)), name, ", ".join(packed if packed else others)))
    assert units >= {"main", "gather", "ny2", "ny34", "mc4", "tiny", "f32", "generic", "generic-large"}, units


# ---- the Solve kernels of tests/test_gpu_solve_params.py ---------------------------------------------------------------------------------------
def test_solve_param_cases_select_their_solve_instantiation(driver):
    """MODE_SOLVE of every case of tests/solve_param_cases.py (its first input level, packed, as the GPU test calls it) under each barrier
    strategy: the name mo_plan_solve_kernel reports and the FusedKey -- family, grid, input level, slots, J stream, y tiles, fp32, pad, and
    pck: the lean instantiations (pck = 0) of the ny2 and the mc2 case under COMPLEMENTARITY / FIXED_DECREASE, pck = 1 under
    PREDICTOR_CORRECTOR and everywhere else.  Exactly one row of the unit's table carries each key."""
    strategies = (("comp", SP.COMPLEMENTARITY), ("fixed", SP.FIXED_DECREASE), ("pc", SP.PREDICTOR_CORRECTOR))
    lines = [line_of(case, SP.level_of(case), call, LC.MODE_SOLVE, 0, strategy, "packed") for case in SP.CASES for call, strategy in strategies]
    got = driver("solve_param_cases.txt", lines)
    lean_seen = set()
    for case in SP.CASES:
        name, want = SP.EXPECTED[case.id]
        for call, strategy in strategies:
            d = got[case.id, SP.level_of(case), call, "packed"]
            assert d["name"] == name, (case.id, call, d)
            if want is None:
                assert d["kind"] == LC.KERNEL_GENERIC and d["large"] == (case.unit == "generic-large"), (case.id, call, d)
                continue
            assert d["kind"] == (LC.KERNEL_FUSED_F32 if want.f32 else LC.KERNEL_FUSED_F64) and d["found"] == 1, (case.id, call, d)
            key = dict(zip(LC.KEY_FIELDS, d["key"]))
            pck = 0 if want.lean and strategy != SP.PREDICTOR_CORRECTOR else 1
            assert (key["family"], key["nt"], key["qpl"], key["mc"], key["jmode"], key["ny"], key["pck"], key["f32"], key["pad"]) == \
                (want.family, want.nt, want.qpl, want.mc, want.jmode, want.ny, pck, want.f32, want.pad), (case.id, call, key, want)
            if not pck:
                lean_seen.add(case.id)
    assert lean_seen == {"ny2", "mc2"}, lean_seen
