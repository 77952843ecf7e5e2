"""The lean instance of the lock-step sweep kernel (pt_sweep.hip LEAN). GPU only.

Plans with the headline configuration (N = 4, chi = 64, 8 trajectories per workgroup, default switches) run an instance
of pt_sweep_kernel compiled for that configuration alone, which keeps its step metadata (each wave's PT units, the
slice schedule) in registers. Its arithmetic and its order are those of the general instance, so its outputs must agree
with the general instance's (PQD_SWEEP_LEAN=0) to 1e-12 relative, a tenth of the 1e-11 the project holds against the
CPU oracle, and with the oracle to 1e-11. Covered: one full workgroup (8 trajectories), a second workgroup with one
trajectory (9), and the 29-trajectory two-system mix of test_gpu_branching (applyBefore MTOs, MTOs at step 0, MTO-free
trajectories, windows that open before the MTO, second MTOs, workgroups that start late), each with a D = 16 PT and a
dictionary PT (D = 9: units of two rows), with and without shared trunks. The grid (36 steps) is longer than the PT
(12 slices), so the sweep runs into the repeated last slice.
"""
import numpy as np
import pytest

from oracle import oracle
from pyaceqd_amd import engine, pt as ptmod
from pyaceqd_amd.engine import Grid
from tests import helpers as H
from tests.test_gpu_branching import g2_reuse_shape, rel

pytestmark = pytest.mark.gpu

N, CHI, N_STEPS = 4, 64, 36
_inputs, _oracle = {}, {}


def inputs(n_traj, D):
    """(systems, grid, rho0, ops, trajectories, pt) of a case, built once"""
    key = (n_traj, D)
    if key not in _inputs:
        n_sys = 2 if n_traj == 29 else 1
        systems = [H.random_system(N, n_steps=N_STEPS, seed=40 + k)[0] for k in range(n_sys)]
        tr = g2_reuse_shape(N_STEPS, n_traj, N, n_sys=n_sys, seed=n_traj + D)
        pt = ptmod.random_pt(N, CHI, D=D, n_slices=12, seed=CHI + D, eps=0.12)
        ops = [H.ketbra(N, 0, 0), H.ketbra(N, 1, 0), np.eye(N)]
        _inputs[key] = (systems if n_sys > 1 else systems[0], Grid(0.0, 0.1, N_STEPS), H.random_rho(N), ops, tr, pt)
    return _inputs[key]


def oracle_outputs(n_traj, D):
    """the CPU oracle's outputs of a case (every trajectory from step 0: independent of PQD_BRANCH), computed once"""
    key = (n_traj, D)
    if key not in _oracle:
        sysd, grid, rho0, ops, tr, pt = inputs(n_traj, D)
        _oracle[key] = oracle.propagate(sysd, grid, rho0, ops, tr, pt=pt, nthreads=8)
    return _oracle[key]


def run(n_traj, D):
    sysd, grid, rho0, ops, tr, pt = inputs(n_traj, D)
    plan = engine.Plan(sysd, grid, rho0, ops, tr, pt=pt)
    plan.execute()
    return plan, plan.download()


def base_env(monkeypatch, branch="1"):
    monkeypatch.setenv("PQD_SPLIT", "0")
    monkeypatch.setenv("PQD_BT", "8")
    monkeypatch.setenv("PQD_BRANCH", branch)


@pytest.mark.parametrize("branch", ["0", "1"])
@pytest.mark.parametrize("D", [16, 9])
@pytest.mark.parametrize("n_traj", [8, 9, 29])
def test_lean_matches_oracle_and_general_instance(monkeypatch, n_traj, D, branch):
    base_env(monkeypatch, branch)
    plan, got = run(n_traj, D)
    assert plan.info()[:2] == (engine.Plan.PATHS[1], 8)
    assert plan.sweep_lean()
    monkeypatch.setenv("PQD_SWEEP_LEAN", "0")
    plan_g, gen = run(n_traj, D)
    assert not plan_g.sweep_lean()
    ref = oracle_outputs(n_traj, D)
    assert len(got) == len(gen) == len(ref) == n_traj
    e_or = max(rel(a, b) for a, b in zip(got, ref))
    e_gen = max(rel(a, b) for a, b in zip(got, gen))
    print(f"lean n_traj={n_traj} D={D} branch={branch}: vs oracle {e_or:.3e}, vs general instance {e_gen:.3e}")
    for a, b, c in zip(got, ref, gen):
        assert a.shape == b.shape == c.shape
    assert e_or < 1e-11, e_or
    assert e_gen < 1e-12, e_gen


@pytest.mark.parametrize("env,lean", [({}, True), ({"PQD_SWEEP_LEAN": "0"}, False), ({"PQD_PT_MODE": "1"}, False),
                                      ({"PQD_FUSE": "0"}, False)])
def test_lean_instance_selection(monkeypatch, env, lean):
    """the lean instance runs by default and only for the configuration it is compiled for"""
    base_env(monkeypatch)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plan, got = run(9, 9)
    assert plan.info()[:2] == (engine.Plan.PATHS[1], 8)
    assert plan.sweep_lean() == lean
    e_or = max(rel(a, b) for a, b in zip(got, oracle_outputs(9, 9)))
    assert e_or < 1e-11, e_or


def test_other_shapes_run_the_general_instance(monkeypatch):
    base_env(monkeypatch)
    sysd, grid = H.random_system(N, n_steps=12, seed=3)
    pt = ptmod.random_pt(N, 32, D=16, n_slices=6, seed=5, eps=0.12)
    plan = engine.Plan(sysd, grid, H.random_rho(N), [H.ketbra(N, 1, 1)], g2_reuse_shape(12, 8, N, seed=1), pt=pt)
    assert not plan.sweep_lean()
