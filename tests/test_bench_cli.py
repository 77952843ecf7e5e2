"""bench.py's command line: --steps, ms_per_step, --dump-outputs and --full.

CPU: dump_outputs' file format and its fixed sample. GPU: one plain run and one --full run of the benchmark at the
reduced shape of tests/test_gpu_branching.py::test_bench_shaped_workload_auto_trunk (3 scan points x 24 t1 x 60 tau
steps, chi = 32), the dumped outputs against the CPU oracle at that test's bound (1e-11 relative)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = ["--t1", "24", "--scan", "3", "--n-tau", "60", "--chi", "32"]


def _load(d):
    v = np.load(os.path.join(d, "outputs.npy"))
    i = np.load(os.path.join(d, "outputs_index.npy"))
    assert v.dtype == np.float64 and i.dtype == np.float64 and v.ndim == 2 and v.shape == (i.shape[0], 2)
    return v[:, 0] + 1j * v[:, 1], i.astype(np.int64)


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    import torch

    import bench
    rng = np.random.default_rng(5)
    x = rng.normal(size=1000) + 1j * rng.normal(size=1000)
    info = bench.dump_outputs(str(tmp_path / "whole"), torch.from_numpy(x))
    v, i = _load(str(tmp_path / "whole"))
    assert info["values"] == 1000 and not info["sampled"]
    assert np.array_equal(v, x) and np.array_equal(i, np.arange(1000))
    monkeypatch.setattr(bench, "DUMP_MAX_VALUES", 96)
    info = bench.dump_outputs(str(tmp_path / "a"), torch.from_numpy(x))
    bench.dump_outputs(str(tmp_path / "b"), torch.from_numpy(x))
    va, ia = _load(str(tmp_path / "a"))
    vb, ib = _load(str(tmp_path / "b"))
    assert info["values"] == 96 and info["of"] == 1000 and info["sampled"]
    assert np.array_equal(ia, ib) and np.array_equal(va, vb)           # the same positions in every run
    assert np.all(np.diff(ia) >= 0) and ia.min() >= 0 and ia.max() < 1000
    assert np.array_equal(va, x[ia])


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        *SHAPE, *extra], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_what_the_plan_computed(tmp_path):
    import bench
    from oracle import oracle
    from pyaceqd_amd import engine
    d = str(tmp_path / "dump")
    line = _bench("--dump-outputs", d)
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "traj-steps/s" and line["higher_is_better"] is True and line["dtype"] == "c128 (fp64)"
    assert abs(line["value"] - 3 * 24 * 60 / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    assert "single_run" not in line and "cpu_baseline" not in line
    systems, grid, pt, rho0, ops, tr = bench.build_workload(24, 60, 32, scan=3)
    v, i = _load(d)
    total = 3 * 24 * 61 * len(ops)
    assert v.shape[0] == total and np.array_equal(i, np.arange(total))
    ref = oracle.propagate(systems, grid, rho0, ops, tr, pt=pt, nthreads=8)
    for a, b in zip(engine.split_output(v, tr, len(ops)), ref):
        assert float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b)))) < 1e-11


@pytest.mark.gpu
def test_full_run_adds_single_run_and_cpu_baseline():
    line = _bench("--full", "--cpu-seconds", "0.2")
    assert line["single_run"]["sweep_ms"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["unit"] == "traj-steps/s"
