"""The DIAG4 index maps of the fused fp64 step kernel (csrc/mo_fused_diag.h: diagonal J^T J tiles on v_mfma_f64_4x4x4_4b_f64), walked on the CPU.

tests/cpp/fused_diag_driver.cpp is compiled against the header the kernel includes.  For n = 64, 62, 50 and 34 it lays a random 4 x n group of
J into a ring slot by the LDS-DMA map (lane (g, j) fetches piece j ^ 4 X[g]), performs the table's operand reads and the 4x4x4 block products
lane by lane with the instruction layout tools/microbench.hip measured on gfx950 (profiles/diag4_microbench.txt: a block is the four quads
i + 4 blk of the 16-lane rows k), stages the ten accumulators and reads them back in the 16x16x4 C/D layout.  Asserted:
  * all four diagonal tiles equal J^T J exactly (same fma order over the four rows), both triangles;
  * the lane's own 16-byte read returns piece j of its row and is conflict-free in the four 16-lane groups a ds_read_b128 is served in;
  * all ten 8-byte operand reads are conflict-free in the two 32-lane groups of a ds_read_b64 (64 banks of 4 bytes);
  * the five instructions cover the ten lower sub-block pairs (p, q) of a tile exactly once."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [64, 62, 50, 34]


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    out = tmp_path_factory.mktemp("fused_diag")
    exe = str(out / "driver")
    res = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "mini_opt_amd", "csrc"),
                          os.path.join(ROOT, "tests", "cpp", "fused_diag_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    res = subprocess.run([exe] + [str(n) for n in SIZES], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    lines = [dict(kv.split("=") for kv in line.split()) for line in res.stdout.splitlines()]
    return {int(d["n"]): d for d in lines if "n" in d}, [d for d in lines if "pairs_once" in d][0]


@pytest.mark.parametrize("n", SIZES)
def test_diagonal_tiles_exact_and_reads_conflict_free(walk, n):
    per_n, _ = walk
    d = per_n[n]
    assert d["natural_ok"] == "1", "the lane's own 16-byte read does not return piece j of its row"
    assert d["tiles_exact"] == "1", "a diagonal tile differs from J^T J"
    assert d["natural_conflict_free"] == "1", "ds_read_b128 of the lane's own piece: bank conflict"
    assert d["operand_conflict_free"] == "1", "ds_read_b64 of a block operand: bank conflict"


def test_ten_sub_block_pairs_covered_once(walk):
    assert walk[1]["pairs_once"] == "1"
