"""Pulse sampling off the sample raster (sample_ch, pqd_common.h) in its older consumers: every free-propagator
builder, the pulse-window logic (idle_half_step, free_win_kernel) and the one-wave no-PT kernel, with the
Hilbert-space kernel on the same system. GPU only.

helpers.random_system samples at dt / (4 n_sub), so every exponential-midpoint time of every other test lands on a
sample and the interpolation weight is 0 or 1. helpers.offgrid_channels puts the samples on a raster incommensurate
with dt that covers only the middle of the run: midpoints fall between samples, before the first and after the last
(clamping). The degenerate rasters (one sample, samples that end before ta, samples that begin after the last step)
clamp every midpoint.

Tolerances
  1e-12 relative to max|reference| for free propagators against helpers.numpy_free_props (scipy expm of the
      Liouvillian at the interpolated samples): test_gpu_parity.test_free_propagators' figure.
  byte equality between PQD_WIN=1 and PQD_WIN=0, and 1e-11 against the C oracle, for the pulse windows: the two
      assertions of test_gpu_windows.test_windows_bit_identical_and_oracle.
  1e-12 against the C oracle for a 12-step no-PT run on either kernel (test_gpu_parity.test_sweep_no_pt's and
      test_gpu_hilbert's figure). The oracle and the numpy restatement agree to 8e-16 on this sampling.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle
from pyaceqd_amd import _lib, engine, pt as ptmod
from pyaceqd_amd.engine import MTO, Trajectories
from tests import helpers as H
from tests.test_gpu_hilbert_envelope import RASTERS, degenerate_raster
from tests.test_gpu_parity import _traj, rel
from tests.test_gpu_windows import SEGMENTS

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ 1. free propagators
@functools.lru_cache(maxsize=None)
def _free_case(N, kind, n_sub):
    sysd, grid = H.random_system(N, n_steps=10, n_sub=n_sub, seed=20 * N + n_sub)
    degenerate_raster(sysd, grid, kind)
    return sysd, grid, H.numpy_free_props(sysd, grid)


@pytest.mark.parametrize("n_sub", [1, 3])
@pytest.mark.parametrize("kind", RASTERS)
@pytest.mark.parametrize("N,switch,value", [(2, "PQD_FP4", "1"), (2, "PQD_FP4", "0"), (3, None, None), (4, None, None),
                                            (5, "PQD_FPM", "0"), (5, "PQD_FPM", "1"), (6, "PQD_FPM", "0"),
                                            (6, "PQD_FPM", "1")])
def test_free_propagators_off_the_sample_raster(monkeypatch, N, switch, value, kind, n_sub):
    """each builder: the packed N2 = 4 kernel and the general one in its place, N2 = 9, N2 = 16, and N2 = 25, 36 on
    the matrix cores and in LDS"""
    if switch:
        monkeypatch.setenv(switch, value)
    sysd, grid, ref = _free_case(N, kind, n_sub)
    got = engine.free_propagators(sysd, grid)
    err = rel(got, ref)
    print(f"free propagators N={N} {switch}={value} {kind} n_sub={n_sub}: rel err {err:.3e}")
    assert got.shape == ref.shape and err < 1e-12


# ------------------------------------------------------------------------------------------ 2. pulse windows
def _offgrid_windowed_systems(N, n_steps, seed):
    """test_gpu_windows' five pulse supports on the off-grid raster with zero end values: the edges of a support fall
    between sample points, so the half steps at an edge interpolate between a zero sample and a non-zero one"""
    out = []
    for k, segs in enumerate(SEGMENTS):
        sysd, grid = H.random_system(N, n_steps=n_steps, seed=seed + k)
        H.offgrid_channels(sysd, grid, cover=(0.013, 0.981), floor=0.0)
        chans = []
        for X, f in sysd.channels:
            f = np.array(f)
            keep = np.zeros(len(f), bool)
            for a, b in segs:
                keep[int(a * len(f)):int(b * len(f))] = True
            f[~keep] = 0.0
            chans.append((X, f))
        sysd.channels = chans
        out.append(sysd)
    return out, grid


@pytest.mark.parametrize("case", ["quad", "batched", "nopt", "n6"])
def test_windows_off_the_sample_raster(monkeypatch, case):
    N = {"batched": 3, "n6": 6}.get(case, 2)
    chi = {"nopt": None, "n6": 16}.get(case, 32 if N == 2 else 16)
    monkeypatch.setenv("PQD_FUSE", "1")
    monkeypatch.setenv("PQD_SPLIT", "0")
    n_steps, n_traj = 40, 17
    systems, grid = _offgrid_windowed_systems(N, n_steps, seed=10 * N)
    tr = _traj(n_steps, N, n_traj, seed=N + 5)
    tr.system = np.array([k % len(systems) for k in range(n_traj)])
    pt = None if chi is None else ptmod.random_pt(N, chi, D=min(N * N, 4), n_slices=7, seed=chi, eps=0.1)
    ops = [H.ketbra(N, 0, 0), H.ketbra(N, 1, 0), H.random_rho(N, seed=4)]
    rho0 = H.random_rho(N)
    res = {}
    for w in ("1", "0"):
        monkeypatch.setenv("PQD_WIN", w)
        plan = engine.Plan(systems, grid, rho0, ops, tr, pt=pt)
        plan.execute()
        res[w] = (plan.download(), plan.info()[0], plan.windows())
    assert res["1"][1] == res["0"][1] and not res["0"][2]
    expect = {"quad": "register-resident TLS quads", "nopt": "no PT (one wave per trajectory)"}.get(
        case, "batched lock-step sweep")
    assert res["1"][1] == expect
    assert res["1"][2] == (case in ("quad", "nopt"))  # the windows are in use where the plan's kernels read them
    for x, y in zip(res["1"][0], res["0"][0]):
        assert np.array_equal(x, y)
    ref = oracle.propagate(systems, grid, rho0, ops, tr, pt=pt, nthreads=8)
    assert len(ref) == n_traj
    errs = [rel(a, b) for a, b in zip(res["1"][0], ref)]
    print(f"windows off-grid {case}: max rel err vs oracle {max(errs):.3e}")
    for a, b in zip(res["1"][0], ref):
        assert a.shape == b.shape
    assert max(errs) < 1e-11


# ------------------------------------------------------------------------------------------ 3. both no-PT paths
def _no_pt_run():
    """one off-grid system at N = 3 on whichever no-PT kernel the process's PQD_HILBERT selects: (path, rel err vs the
    oracle)"""
    N, n_steps = 3, 12
    sysd, grid = H.random_system(N, n_steps=n_steps, n_sub=2, seed=33)
    H.offgrid_channels(sysd, grid)
    rng = np.random.default_rng(34)
    A = lambda: (rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))) / N  # noqa: E731
    tr = Trajectories(np.array([0, 3]), np.array([n_steps, n_steps]),
                      [MTO(0, 0, True, 1, A()), MTO(0, 7, False, 2, A()), MTO(1, 5, True, 0, A())])
    ops = [H.ketbra(N, 0, 0), H.ketbra(N, N - 1, 0), np.eye(N)]
    rho0 = H.random_rho(N)
    plan = engine.Plan(sysd, grid, rho0, ops, tr)
    plan.execute()
    got = plan.download()
    ref = oracle.propagate(sysd, grid, rho0, ops, tr)
    assert len(got) == len(ref) == 2
    return plan.describe()["path"], max(rel(a, b) for a, b in zip(got, ref))


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_sampling import _no_pt_run
path, err = _no_pt_run()
print("RESULT " + json.dumps({"path": path, "err": err}))
"""


def test_same_offgrid_system_on_both_no_pt_paths(monkeypatch):
    """the one-wave no-PT kernel reads stored free propagators, the Hilbert-space kernel samples the pulse itself:
    one off-grid system at N = 3 on each (PQD_HILBERT=1 in a fresh child process, as it is read at plan creation)"""
    monkeypatch.delenv("PQD_HILBERT", raising=False)
    path, err = _no_pt_run()
    print(f"off-grid N=3 on the one-wave kernel: rel err vs oracle {err:.3e}")
    assert path == str(_lib.PQD_PATH_NOPT)
    assert err < 1e-12
    env = dict(os.environ, PQD_HILBERT="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, REPO], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print(f"off-grid N=3 on the Hilbert-space kernel: rel err vs oracle {res['err']:.3e}")
    assert res["path"] == str(_lib.PQD_PATH_HILBERT)
    assert res["err"] < 1e-12
