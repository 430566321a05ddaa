"""bench.py's multi-rank path with REAL launches: two ranks started by torch.distributed.run share the one GPU of the test box
(ranks wrap around the visible devices), gloo stands in for RCCL (two ranks on one device cannot form an RCCL communicator).  Everything
else is the code the driver runs at N > 1: config-5 sharding, per-rank plans and launches, barriers, MAX / SUM, the roofline block."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_on_one_gpu_run_config5_shards():
    env = dict(os.environ, MO_BENCH_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2",
           "--config", "cfg5", "--batch", "16384", "--full"]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout
    out = json.loads(lines[0])
    # the N > 1 line carries its own correctness figure: both ranks checked a strided 256-problem sample of their shard against the oracle,
    # reduced over the gloo control plane; no cpu_baseline at N > 1
    par = out["parity"]
    assert par["passed"] is True and par["ranks"] == 2 and par["sample"] == 512 and par["max_rel_inf"] < 1e-10 and par["status_disagreements"] == 0
    assert out["status_ok"] == out["status_total"] == out["config"]["batch_total"] == 32768
    assert "cpu_baseline" not in out
    assert out["n_gpus"] == 2 and out["steps"] == 4 and out["scaling"] == "strong"
    assert out["config"]["name"] == "cfg5" and out["config"]["batch_per_gpu"] == 16384 and out["config"]["batch_total"] == 32768
    assert out["config"]["kernel"] == "fused_mfma_f64_n64"
    assert out["value"] > 1e6 and out["unit"] == "steps/s"                       # whole-job rate of both ranks
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 - 32768) < 1e-3 * 32768  # value = units of all ranks / max time
    assert out["roofline"]["bound"] == "hbm" and 0 < out["roofline"]["frac"] < 1
    assert out["status_ok"] == out["status_total"]


def test_bare_gpus_flag_runs_two_real_ranks():
    """The driver's scaling command is a bare `python bench.py --gpus N`: the parent (which never touches the GPU) starts the ranks as child
    processes and relays rank 0's line.  Here N = 2 on the box's one GPU with gloo standing in for RCCL."""
    env = dict(os.environ, MO_BENCH_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2", "--config", "cfg5",
           "--batch", "16384", "--no-cpu-baseline", "--sustain-seconds", "0.3", "--full"]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), res.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["batch_total"] == 32768 and out["config"]["kernel"] == "fused_mfma_f64_n64"
    assert out["value"] > 1e6 and out["status_ok"] == out["status_total"]
    assert out["sustained"]["seconds"] >= 0.3 and out["sustained"]["value"] > 1e6


def test_two_ranks_on_one_gpu_fall_back_from_rccl_to_gloo():
    """Without MO_BENCH_BACKEND the ranks ask for RCCL.  Two ranks on ONE device cannot form an RCCL communicator: both must notice, agree over
    the gloo control plane to time over gloo instead, and the run must still produce its line (a driver-run `--gpus N` never exits non-zero
    because of the library that carries its barrier)."""
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "MO_BENCH_BACKEND"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--config", "cfg5",
           "--batch", "8192", "--no-cpu-baseline", "--sustain-seconds", "0", "--full"]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), res.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["batch_total"] == 16384 and out["status_ok"] == out["status_total"]
    assert out["timing_sync"] == "rccl" or out["timing_sync"].startswith("gloo (rccl unavailable"), out["timing_sync"]


def test_solve_mode_two_ranks_and_single_rank():
    """`bench.py --mode solve` (one mo_qp_solve launch per step): two ranks on the one GPU with the all-rank parity block -- termination state and
    iteration count of every checked problem equal to the oracle's Solve, optimum within 1e-6 -- and the single-rank line with the flop roofline
    and the oracle's Solve as cpu_baseline."""
    env = dict(os.environ, MO_BENCH_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--mode", "solve", "--steps", "3", "--warmup", "1", "--config", "cfg3",
           "--batch", "8192", "--sustain-seconds", "0", "--full"]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    out = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][0])
    assert out["unit"] == "solves/s" and out["n_gpus"] == 2 and out["config"]["kernel"] == "fused_solve_mfma_f64_n64"
    assert out["parity"]["passed"] is True and out["parity"]["sample"] == 512 and out["parity"]["solve_disagreements"] == 0
    assert out["status_ok"] == out["status_total"] == 16384
    assert out["roofline"]["bound"] == "mfma" and out["roofline"]["unit"] == "TFLOP/s" and 0 < out["roofline"]["frac"] < 1
    assert 6.0 < out["roofline"]["mean_iterations"] < 10.0
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--mode", "solve", "--steps", "3", "--warmup", "1", "--batch", "4096", "--sustain-seconds", "0",
           "--cpu-seconds", "2", "--full"]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    out = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][0])
    assert out["n_gpus"] == 1 and out["parity"]["passed"] is True and out["parity"]["sample"] == 4096      # the whole batch at N = 1
    assert out["cpu_baseline"]["unit"] == "solves/s" and out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["one_core"]["cores"] == 1
    assert out["value"] > 20 * out["cpu_baseline"]["value"]


def _plain_env():
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "MO_BENCH_BACKEND"):
        env.pop(k, None)
    return env


def _line(res):
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), res.stdout
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_step(tmp_path):
    """A plain `bench.py --steps K --warmup W --dump-outputs DIR` at the default workload (cfg3, batch 65 536): K timed steps, the headline
    line only, and the last step's delta / alpha / status -- a seeded sample of the batch, the whole of it exceeds the budget -- written
    identically by two runs and equal to the oracle's step on the same problems, regenerated here from the same seed."""
    import numpy as np
    import torch

    from mini_opt_amd import synth
    from oracle import oracle as orc
    runs = []
    for d in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path / d)]
        runs.append(_line(subprocess.run(cmd, cwd=ROOT, env=_plain_env(), capture_output=True, text=True, timeout=600)))
    out = runs[0]
    assert out["steps"] == 7 and out["warmup"] == 2 and out["unit"] == "steps/s" and out["dtype"] == "f64" and out["higher_is_better"] is True
    assert out["metric"] == "batched dense KKT Newton steps/sec, n=64 fp64" and out["config"]["batch_per_gpu"] == 65536
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 - 65536) < 1e-3 * 65536
    assert not {"parity", "status_ok", "roofline", "cpu_baseline", "sustained"} & set(out)
    names = ("sample_index", "delta", "alpha", "status")
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f + ".npy" for f in names)
    assert sum(os.path.getsize(tmp_path / "a" / (f + ".npy")) for f in names) <= 64 * 10 ** 6
    a = {f: np.load(tmp_path / "a" / (f + ".npy")) for f in names}
    b = {f: np.load(tmp_path / "b" / (f + ".npy")) for f in names}
    idx = a["sample_index"].astype(np.int64)
    V = 64 + 2 * 32 + 8
    assert 0 < len(idx) < 65536 and np.all(np.diff(idx) > 0)
    assert a["delta"].shape == (len(idx), V) and a["alpha"].shape == (len(idx), 2) and a["status"].shape == (len(idx),)
    assert all(v.dtype == np.float64 for v in a.values()) and np.all(a["status"] == 0)
    for f in names:
        assert np.array_equal(a[f], b[f]), f
    d = synth.CONFIGS["cfg3"]
    dev = torch.device("cuda:0")
    prob, vars_, mu = synth.make_batch_torch(d["n"], d["k"], d["m"], d["m_r"], 65536, dev, torch.float64, seed=synth.SEED)
    pick = np.arange(0, len(idx), max(1, len(idx) // 64))
    tix = torch.as_tensor(idx[pick], device=dev)
    h = lambda t: t.index_select(0, tix).double().cpu().numpy()
    ref, ref_alpha, ref_status, _ = orc.batched_newton_step(
        d["n"], d["k"], d["m"], J=h(prob.J), r=h(prob.r), lam=prob.lam, A_eq=h(prob.A_eq), b_eq=h(prob.b_eq),
        cons_var=prob.cons_var.index_select(0, tix).cpu().numpy(), cons_a=h(prob.cons_a), cons_b=h(prob.cons_b), vars_=h(vars_), mu=h(mu))
    got = a["delta"][pick]
    assert np.all(ref_status == 0)
    assert (np.max(np.abs(got - ref), axis=1) / np.max(np.abs(ref), axis=1)).max() < 1e-10
    assert np.max(np.abs(a["alpha"][pick] - ref_alpha)) < 1e-9


def test_plain_solve_run_dumps_the_solver_outputs(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--mode", "solve", "--batch", "2048", "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(tmp_path)]
    out = _line(subprocess.run(cmd, cwd=ROOT, env=_plain_env(), capture_output=True, text=True, timeout=600))
    assert out["steps"] == 2 and out["unit"] == "solves/s" and "parity" not in out
    import numpy as np
    f = {name[:-4]: np.load(tmp_path / name) for name in os.listdir(tmp_path)}
    assert set(f) == {"sample_index", "variables", "termination_state", "num_iterations", "iterations", "lagrange_multipliers", "status"}
    assert np.array_equal(f["sample_index"], np.arange(2048.0))
    assert f["variables"].shape == (2048, 64 + 2 * 32 + 8) and f["iterations"].shape == (2048, 10, 14)
    assert np.all(f["status"] == 0) and np.all((f["num_iterations"] >= 1) & (f["num_iterations"] <= 10))
    assert np.all(np.isfinite(f["variables"]))
