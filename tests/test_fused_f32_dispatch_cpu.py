"""The dispatch of the fused fp32 kernels is data (csrc/mo_fused_select.h: fused_f32_supported / fused_f32_select / fused_f32_name, reached
through decide_kernel, the decision mo_api.hip takes; and the table of csrc/kkt_fused_f32.hip).  This test walks a shape lattice on the CPU
(tests/cpp/fused_f32_dispatch_driver.cpp against the current sources, linked with the host-only object of the fp32 unit; nothing is
launched) and checks every point against the coverage and the instantiation table restated here, independently, from the shape alone.
No tolerance, no excluded points."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mini_opt_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
LINEARIZE, RESIDUAL, STEP, ITERATE, SOLVE, RHS = range(6)
STEP_FAMILY, SOLVE_FAMILY, LINEARIZE_FAMILY = 0, 1, 2
NUM_CUS = 256
FIELDS = ("n", "k", "m", "mode", "flags", "kind", "m_r", "batch", "sr", "fused", "family", "nt", "wps", "pad", "grid", "block", "zero_ticket",
          "static_rounds", "stagger", "chain_prio")


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    out = tmp_path_factory.mktemp("fused_f32_dispatch")
    jobs = [("unit", subprocess.Popen([HIPCC, "--cuda-host-only", "-O0", "-std=c++17", "-w", "-c", os.path.join(CSRC, "kkt_fused_f32.hip"), "-o", str(out / "unit.o")],
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)),
            ("driver", subprocess.Popen([HIPCC, "--cuda-host-only", "-O1", "-std=c++17", "-x", "hip", "-c",
                                         os.path.join(ROOT, "tests", "cpp", "fused_f32_dispatch_driver.cpp"), "-o", str(out / "driver.o")],
                                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))]
    for name, job in jobs:
        text = job.communicate(timeout=900)[0]
        assert job.returncode == 0, (name, text[-4000:])
    exe = str(out / "driver")
    res = subprocess.run([HIPCC, "-Wl,--unresolved-symbols=ignore-all", "-o", exe, str(out / "unit.o"), str(out / "driver.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    res = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    points = []
    for line in open(out / "points.txt"):
        cols = line.rstrip("\n").split("\t")
        rec = dict(zip(FIELDS, map(int, cols[:len(FIELDS)])))
        rec["name"], rec["found"] = cols[len(FIELDS)], int(cols[len(FIELDS) + 1])
        points.append(rec)
    counters = dict((line.split("\t")[0], int(line.split("\t")[1])) for line in open(out / "counters.txt"))
    table = [tuple(map(int, line.split("\t"))) for line in open(out / "table.txt")]
    return points, counters, table


def covered(s):
    """The coverage rule, from the shape alone.  kind 0: (G, c); 1: packed, 16-byte aligned, row-major J; 2 column-major; 3 J_ld > n;
    4 an 8-byte aligned J; 5 an odd J_stride."""
    n, mode = s["n"], s["mode"]
    if n % 4 or not 4 <= n <= 128 or mode == RHS:
        return False
    if mode == LINEARIZE:      # the cost alone: k, m and the flags play no part
        return n in (64, 128) and s["kind"] == 1 and s["m_r"] % 4 == 0
    if s["k"] > 16 or s["m"] > 64:
        return False
    if mode == STEP:
        return s["kind"] == 1
    if mode in (SOLVE, ITERATE) and s["flags"]:
        return False
    return s["kind"] in (0, 1)


def expected(s):
    """The instantiation table: (family, NT, WPS, PAD) and the name."""
    n, mode, big = s["n"], s["mode"], s["n"] > 64
    size = 128 if big else 64
    if mode == LINEARIZE:
        return (LINEARIZE_FAMILY, 8, 2, 0) if big else (LINEARIZE_FAMILY, 4, 3, 0), "fused_linearize_f32_n%d" % size
    pad = int(n != size)
    if mode == STEP:
        return (STEP_FAMILY, 8, 2, pad) if big else (STEP_FAMILY, 4, 3, pad), "fused_mfma_f32_n%d" % size
    return (SOLVE_FAMILY, 8, 1, pad) if big else (SOLVE_FAMILY, 4, 3, pad), "fused_solve_%s_f32_n%d" % ("qp" if s["kind"] == 0 else "mfma", size)


def test_the_walk_counts_no_violation(walk):
    _, c, _ = walk
    assert c["points"] == 10 * 3 * 3 * 6 * 2 * (1 + 5 * 3) * 5 * 3 and c["fused_f32"] > 10000, c
    for name in ("kind_is_not_the_predicate", "other_fused_kind", "forced_not_generic", "f64_plan_f32_kernel", "f64_plan_f32_predicate", "denormalised_key"):
        assert c[name] == 0, (name, c)


def test_every_point_follows_the_coverage_and_the_table(walk):
    points, c, _ = walk
    assert len(points) == c["points"]
    wrong = [s for s in points if bool(s["fused"]) != covered(s)]
    assert not wrong, (len(wrong), wrong[:5])
    for s in points:
        if not s["fused"]:
            assert s["name"] == "generic" and s["found"] == 0, s
            continue
        key, name = expected(s)
        assert (s["family"], s["nt"], s["wps"], s["pad"]) == key and s["name"] == name and s["found"] == 1, s
        rounds = s["sr"] if s["sr"] >= 0 else (2 if s["mode"] == SOLVE else 8) if s["n"] > 32 else (6 if s["mode"] == SOLVE else 32)
        grid = max(1, min(NUM_CUS, (s["batch"] + 3) // 4))
        assert s["static_rounds"] == rounds and s["grid"] == grid and s["block"] == 256 * s["wps"], s
        assert s["zero_ticket"] == int(not (rounds > 0 and s["batch"] <= rounds * 4 * grid)), s
        assert s["stagger"] == 0 and s["chain_prio"] == 0, s


def test_named_points_inside_and_outside(walk):
    points, _, _ = walk
    pick = lambda **kw: [s for s in points if all(s[key] == val for key, val in kw.items())]
    inside = [dict(n=60, mode=STEP, kind=1, k=16, m=64)]
    inside += [dict(n=128, k=16, m=64, mode=mode, kind=1, m_r=64, flags=0) for mode in (LINEARIZE, RESIDUAL, STEP, ITERATE, SOLVE)]
    for case in inside:
        got = pick(**case)
        assert got and all(s["fused"] for s in got), case
    assert all(s["pad"] == 1 for s in pick(n=60, mode=STEP, kind=1, k=16, m=64))
    not_linearize = [dict(mode=mode) for mode in (RESIDUAL, STEP, ITERATE, SOLVE)]
    outside = [dict(n=63), dict(mode=STEP, kind=0), dict(mode=LINEARIZE, n=60), dict(mode=LINEARIZE, m_r=6), dict(mode=RHS)]
    outside += [dict(kind=kind) for kind in (2, 3, 4, 5)]
    outside += [dict(k=17, **mode) for mode in not_linearize] + [dict(m=65, **mode) for mode in not_linearize]
    for case in outside:
        got = pick(**case)
        assert got and not any(s["fused"] for s in got), case


def test_every_row_of_the_table_is_selected_and_no_key_has_two_rows(walk):
    _, _, table = walk
    assert len(table) == 10
    assert len({row[:-1] for row in table}) == len(table), "a key has two rows"
    unselected = [row[:-1] for row in table if row[-1] == 0]
    assert not unselected, unselected
