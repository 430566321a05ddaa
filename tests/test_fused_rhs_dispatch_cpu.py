"""The dispatch of mo_kkt_solve's fused kernels is data (csrc/mo_fused_select.h: fused_rhs_supported / fused_rhs_select behind decide_kernel, and the table of
csrc/kkt_fused_rhs.hip): the right-hand-side kernel of a shape is the twin of that shape's step kernel.  This test walks a shape lattice on the
CPU (tests/cpp/fused_rhs_dispatch_driver.cpp against the current sources, linked with the host-only object of the new unit; nothing is
launched) and checks the rule from both sides: what the driver counts itself (supported implies the step is supported, equal launch
descriptions, one row per key), and the coverage restated here, independently, from the shape alone."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mini_opt_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
STEP_NO_INEQUALITIES = 1


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    out = tmp_path_factory.mktemp("fused_rhs_dispatch")
    jobs = [("unit", subprocess.Popen([HIPCC, "--cuda-host-only", "-O0", "-std=c++17", "-w", "-c", os.path.join(CSRC, "kkt_fused_rhs.hip"), "-o", str(out / "unit.o")],
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)),
            ("driver", subprocess.Popen([HIPCC, "--cuda-host-only", "-O1", "-std=c++17", "-x", "hip", "-c",
                                         os.path.join(ROOT, "tests", "cpp", "fused_rhs_dispatch_driver.cpp"), "-o", str(out / "driver.o")],
                                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))]
    for name, job in jobs:
        text = job.communicate(timeout=900)[0]
        assert job.returncode == 0, (name, text[-4000:])
    exe = str(out / "driver")
    res = subprocess.run([HIPCC, "-Wl,--unresolved-symbols=ignore-all", "-o", exe, str(out / "unit.o"), str(out / "driver.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    res = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    fields = ("n", "k", "m", "kind", "m_r", "flags", "no_tiny", "supported", "nt", "wps", "qpl", "mc", "jmode", "ny")
    shapes = []
    for line in open(out / "shapes.txt"):
        cols = line.rstrip("\n").split("\t")
        rec = dict(zip(fields, map(int, cols[:len(fields)])))
        rec["name"], rec["found"] = cols[len(fields)], int(cols[len(fields) + 1])
        shapes.append(rec)
    counters = dict((line.split("\t")[0], int(line.split("\t")[1])) for line in open(out / "counters.txt"))
    table = [tuple(map(int, line.split("\t"))) for line in open(out / "table.txt")]
    return shapes, counters, table


def covered(s):
    """The coverage rule, from the shape alone.  kind 0: (G, c); 1: packed, 16-byte aligned, row-major J; 2 column-major; 3 J_ld > n;
    4 an 8-byte aligned J; 5 an odd J_stride."""
    n, k, m = s["n"], s["k"], s["m"]
    if not (2 <= n <= 128 and k <= 31 and m <= 128):
        return False
    if s["kind"] not in (0, 1) or (s["kind"] == 1 and n % 2):
        return False
    one_tile = n + k <= 15 and m <= 64 and (s["kind"] == 0 or s["m_r"] <= 64) and not s["no_tiny"]
    return not one_tile


def test_supported_points_are_the_twins_of_their_step(walk):
    _, c, _ = walk
    assert c["points"] > 500000 and c["supported"] > 50000, c
    for name in ("supported_without_step", "launch_differs", "rows_not_one", "f32_supported", "not_rhs_mode_supported", "null_rhs_supported",
                 "varies_with_batch", "decision_differs"):
        assert c[name] == 0, (name, c)


def test_coverage_is_the_rule_of_the_header(walk):
    shapes, _, _ = walk
    wrong = [s for s in shapes if bool(s["supported"]) != covered(s)]
    assert not wrong, (len(wrong), wrong[:5])
    grid = lambda n: 2 if n <= 32 else 4 if n <= 64 else 6 if n <= 96 else 8
    for s in shapes:
        if not s["supported"]:
            assert s["name"] == "generic"
            continue
        assert s["found"] == 1
        assert s["nt"] == grid(s["n"]) and s["qpl"] == (s["kind"] == 0) and s["jmode"] == 0
        assert s["ny"] == (2 if s["k"] > 15 else 1) and s["mc"] == (2 if (s["m"] > 64 or s["ny"] == 2) else 1)
        assert s["name"] == "fused_rhs_%s_f64_n%d" % ("qp" if s["qpl"] else "mfma", 16 * s["nt"])
    # the points the coverage names as outside, one by one (flags 0, default plan)
    pick = lambda **kw: [s for s in shapes if s["flags"] == 0 and s["no_tiny"] == 0 and all(s[key] == val for key, val in kw.items())]
    for outside in (dict(n=64, k=32, m=64, kind=0), dict(n=64, k=8, m=129, kind=0), dict(n=64, k=8, m=64, kind=2, m_r=64),
                    dict(n=63, k=8, m=64, kind=1, m_r=64), dict(n=33, k=8, m=64, kind=1, m_r=130), dict(n=8, k=7, m=64, kind=0),
                    dict(n=7, k=8, m=0, kind=0), dict(n=64, k=8, m=64, kind=3, m_r=64), dict(n=64, k=8, m=64, kind=4, m_r=64),
                    dict(n=64, k=8, m=64, kind=5, m_r=65), dict(n=129, k=0, m=0, kind=0), dict(n=1, k=0, m=0, kind=0)):
        got = pick(**outside)
        assert got and not any(s["supported"] for s in got), outside
    for inside in (dict(n=64, k=8, m=64, kind=1, m_r=130), dict(n=63, k=8, m=64, kind=0), dict(n=8, k=8, m=0, kind=0),
                   dict(n=8, k=7, m=65, kind=0), dict(n=8, k=7, m=64, kind=1, m_r=65), dict(n=128, k=31, m=128, kind=1, m_r=8)):
        got = pick(**inside)
        assert got and all(s["supported"] for s in got), inside
    # MO_STEP_NO_INEQUALITIES and MO_KKT_TRANSPOSE do not change which kernel runs
    by_shape = {}
    for s in shapes:
        by_shape.setdefault((s["n"], s["k"], s["m"], s["kind"], s["m_r"], s["no_tiny"]), set()).add((s["supported"], s["nt"], s["wps"], s["mc"], s["ny"]))
    assert all(len(v) == 1 for v in by_shape.values())


def test_every_row_of_the_table_is_selected_and_no_key_has_two_rows(walk):
    _, _, table = walk
    assert len(table) == 24
    assert all(row[0] == 0 and row[5] == 0 and row[7] == 1 for row in table)      # the STEP family's keys, vector stream
    assert len({row[:-1] for row in table}) == len(table), "a key has two rows"
    unselected = [row[:-1] for row in table if row[-1] == 0]
    assert not unselected, unselected
