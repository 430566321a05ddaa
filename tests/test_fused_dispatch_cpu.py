"""The fused fp64 dispatch is data (csrc/mo_fused_select.h + one kernel table per translation unit): this test walks a shape lattice through
decide_kernel (the decision mo_api.hip takes: fused_supported / fused_select / fused_name behind it) and the tables on the CPU and compares every point with a recording of what the hand-written
launchers of commit 662741eb chose (tests/golden/fused_dispatch: distinct launch descriptions + one index per lattice point, keys in
normalised form -- template defaults written out, the constant sweep-flavour argument of that commit dropped).

The host program is built from the CURRENT sources: tests/cpp/fused_dispatch_driver.cpp against the selector header, linked with the
host-only objects of the six fused units (hipcc --cuda-host-only: the tables and launch_fused, no device code, so the link leaves the
device blobs unresolved; nothing is ever launched).  No tolerance, no excluded points."""
import json
import lzma
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mini_opt_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden", "fused_dispatch")
HIPCC = "/opt/rocm/bin/hipcc"
UNITS = ["kkt_fused", "kkt_fused_gather", "kkt_fused_ny2", "kkt_fused_ny34", "kkt_fused_mc4", "kkt_fused_tiny"]
FIELDS = ["family", "nt", "wps", "qpl", "mc", "jmode", "ny", "pck", "grid", "block", "zero_ticket", "stagger", "chain_prio", "static_rounds", "name"]


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    """Builds the driver, runs it once; returns (records, index, tables) of the current sources."""
    out = tmp_path_factory.mktemp("fused_dispatch")
    jobs = [(u, subprocess.Popen([HIPCC, "--cuda-host-only", "-O0", "-std=c++17", "-w", "-c", os.path.join(CSRC, u + ".hip"), "-o", str(out / (u + ".o"))],
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)) for u in UNITS]
    jobs.append(("driver", subprocess.Popen([HIPCC, "--cuda-host-only", "-O1", "-std=c++17", "-x", "hip", "-c",
                                             os.path.join(ROOT, "tests", "cpp", "fused_dispatch_driver.cpp"), "-o", str(out / "driver.o")],
                                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for name, job in jobs:
        text = job.communicate(timeout=900)[0]
        assert job.returncode == 0, (name, text[-4000:])
    exe = str(out / "driver")
    res = subprocess.run([HIPCC, "-Wl,--unresolved-symbols=ignore-all", "-o", exe] + [str(out / (n + ".o")) for n, _ in jobs], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    res = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    records = [line.rstrip("\n").split("\t") for line in open(out / "records.txt")]
    index = np.fromfile(out / "index.u16", dtype=np.uint16)
    tables = [line.rstrip("\n").split("\t") for line in open(out / "tables.txt")]
    return records, index, tables


@pytest.fixture(scope="module")
def golden():
    g = json.load(open(os.path.join(GOLD, "records.json")))
    assert g["fields"] == FIELDS
    index = np.frombuffer(lzma.decompress(open(os.path.join(GOLD, "index.u16.xz"), "rb").read()), dtype=np.uint16)
    return [None] + [[str(v) for v in row] for row in g["rows"]], index   # record 0: fused_supported is false


def test_every_lattice_point_matches_the_recorded_dispatch(walk, golden):
    records, index, _ = walk
    gold_records, gold_index = golden
    assert len(index) == len(gold_index) == 9261000
    # fused_supported
    assert records[0] == ["unsupported"]
    unsupported_differs = np.nonzero((index == 0) != (gold_index == 0))[0]
    assert len(unsupported_differs) == 0, ("fused_supported differs at lattice points", unsupported_differs[:10].tolist())
    # the launch description, field by field (key, grid, block, zero_ticket, stagger, chain_prio, static_rounds) and fused_name
    gold_id = {tuple(r): i for i, r in enumerate(gold_records) if r}
    to_gold = np.array([0] + [gold_id.get(tuple(r[:len(FIELDS)]), -1) for r in records[1:]], dtype=np.int64)
    differs = np.nonzero(to_gold[index] != gold_index.astype(np.int64))[0]
    report = []
    for point in differs[:10]:
        got, want = records[index[point]], gold_records[gold_index[point]]
        report.append((int(point), {f: (w, g) for f, g, w in zip(FIELDS, got, want) if g != w}))
    assert len(differs) == 0, ("%d lattice points differ; point -> field: (recorded, now)" % len(differs), report)
    # the key of every supported point is in a table, once
    not_found = [r for r in records[1:] if r[len(FIELDS)] != "1"]
    assert not not_found, not_found[:10]


def test_every_table_row_is_selected_somewhere_on_the_lattice(walk, golden):
    _, _, tables = walk
    gold_records, _ = golden
    assert tables, "no table rows"
    unselected = [row[:-1] for row in tables if int(row[-1]) == 0]
    assert not unselected, ("table rows no lattice point selects (unit, family, nt, wps, qpl, mc, jmode, ny, pck)", unselected)
    keys = [tuple(row[1:-1]) for row in tables]
    assert len(set(keys)) == len(keys), "a key has two rows"
    # and the tables hold exactly the instantiations the recording selects
    assert set(keys) == {tuple(r[:8]) for r in gold_records if r}
