"""Outputs read inside the fused column phase of the lean sweep instance (pt_sweep.hip LeanCol). GPU only.

From the first step after a workgroup's last MTO and activation (SweepParams::blk_fast) the lean instance reads a step's
outputs from the operands of the fused column operator F(n), in the wave that owns the trajectory, and runs two barriers
a step; before that step, on the block's last two steps and with PQD_LEAN_RO=0 it runs the closure pass as before. The
states are the same bits either way and the outputs differ by the order of a 64-term and a 16-term sum, so every case
is held to the project's tolerances three ways: 1e-12 relative against the lean instance with PQD_LEAN_RO=0 and against
the general instance (PQD_SWEEP_LEAN=0), 1e-11 against the CPU oracle; and Plan.sweep_readout() must report the path.

Trajectory i of a case has its MTO pair at step 1 + (5 i mod 14), so the fast region starts mid-run (step 15 of 40 at
most), and its window ends at 40 - (3 i mod 11): the waves of a workgroup stop storing at different steps while the
others go on. Trajectory 2 opens its window six steps after its MTO. Cases:
  * 8, 9 and 3 trajectories: a full workgroup, a second one with one trajectory and seven empty slots, a partial one;
  * an applyBefore MTO on the last step of one trajectory: its workgroup never qualifies and sweep_readout() says so;
  * 1, 2, 3 and 4 output operators; two systems in one workgroup (F and W per wave); D = 16 and the 9-slice dictionary;
  * a PT of 30 slices (the slice set, and with it the closure vector of sched[n - 1], still changes inside the fast
    region) and one of 40 (a new set on every step to the end of the grid);
  * PQD_BRANCH 0 and 1; three execute() calls of one plan with bitwise equal outputs.
"""
import dataclasses

import numpy as np
import pytest

from oracle import oracle
from pyaceqd_amd import engine, pt as ptmod
from pyaceqd_amd.engine import MTO, Grid, Trajectories
from tests import helpers as H
from tests.test_gpu_branching import rel
from tests.test_gpu_sweep_ptloop import GMAP, OPS

pytestmark = pytest.mark.gpu

N, CHI, N_STEPS = 4, 64, 40
_inputs, _oracle = {}, {}


def trajectories(n_traj, n_sys, last_mto):
    rng = np.random.default_rng(100 + n_traj)
    A = rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))
    Cm = rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))
    A, Cm = A / np.linalg.norm(A), Cm / np.linalg.norm(Cm)
    beg, end, mtos = [], [], []
    for i in range(n_traj):
        t1 = 1 + (5 * i) % 14
        mtos += [MTO(i, t1, False, 2, A), MTO(i, t1, False, 1, Cm)]
        beg.append(t1 + 6 if i == 2 else t1)   # trajectory 2: the window opens after the slot's last MTO
        end.append(N_STEPS - (3 * i) % 11)
    if last_mto:   # trajectory 0 ends at N_STEPS: an MTO before its last output
        mtos.append(MTO(0, N_STEPS, True, 0, A))
    system = np.arange(n_traj) % n_sys if n_sys > 1 else None
    return Trajectories(np.array(beg), np.array(end), mtos, system=system)


def inputs(n_traj, D=16, n_slices=5, n_out=3, n_sys=1, last_mto=False):
    """(systems, grid, rho0, ops, trajectories, pt) of a case, built once"""
    key = (n_traj, D, n_slices, n_out, n_sys, last_mto)
    if key not in _inputs:
        systems = [H.random_system(N, n_steps=N_STEPS, seed=80 + k)[0] for k in range(n_sys)]
        pt = ptmod.random_pt(N, CHI, D=D, n_slices=n_slices, seed=CHI + D + n_slices, eps=0.12)
        pt = dataclasses.replace(pt, gmap=GMAP[D])
        _inputs[key] = (systems if n_sys > 1 else systems[0], Grid(0.0, 0.1, N_STEPS), H.random_rho(N), OPS[:n_out],
                        trajectories(n_traj, n_sys, last_mto), pt)
    return key, _inputs[key]


def oracle_outputs(key):
    if key not in _oracle:
        sysd, grid, rho0, ops, tr, pt = _inputs[key]
        _oracle[key] = oracle.propagate(sysd, grid, rho0, ops, tr, pt=pt, nthreads=8)
    return _oracle[key]


def base_env(monkeypatch, branch="1"):
    monkeypatch.setenv("PQD_SPLIT", "0")
    monkeypatch.setenv("PQD_BT", "8")
    monkeypatch.setenv("PQD_BRANCH", branch)


def run(case):
    plan = engine.Plan(*case[:5], pt=case[5])
    plan.execute()
    return plan, plan.download()


def check(monkeypatch, branch="1", readout=True, **kw):
    """the readout in the column phase against the closure pass of the lean instance and the general instance (1e-12)
    and against the CPU oracle (1e-11); sweep_readout() reports the path"""
    base_env(monkeypatch, branch)
    key, case = inputs(**kw)
    plan, got = run(case)
    assert plan.info()[:2] == (engine.Plan.PATHS[1], 8)
    assert plan.sweep_lean()
    assert plan.sweep_readout() == readout
    monkeypatch.setenv("PQD_LEAN_RO", "0")
    plan_o, old = run(case)
    assert plan_o.sweep_lean() and not plan_o.sweep_readout()
    monkeypatch.setenv("PQD_SWEEP_LEAN", "0")
    plan_g, gen = run(case)
    assert not plan_g.sweep_lean() and not plan_g.sweep_readout()
    ref = oracle_outputs(key)
    assert len(got) == len(old) == len(gen) == len(ref) == kw["n_traj"]
    for a, b, c, d in zip(got, ref, gen, old):
        assert a.shape == b.shape == c.shape == d.shape
    e_or = max(rel(a, b) for a, b in zip(got, ref))
    e_old = max(rel(a, b) for a, b in zip(got, old))
    e_gen = max(rel(a, b) for a, b in zip(got, gen))
    print(f"readout {kw} branch={branch}: vs oracle {e_or:.3e}, vs closure pass {e_old:.3e}, "
          f"vs general instance {e_gen:.3e}")
    assert e_or < 1e-11, e_or
    assert e_old < 1e-12, e_old
    assert e_gen < 1e-12, e_gen


@pytest.mark.parametrize("branch", ["0", "1"])
@pytest.mark.parametrize("n_traj", [8, 9, 3])
def test_block_shapes(monkeypatch, n_traj, branch):
    """a full workgroup, a second one with seven empty slots, a partial one; window ends and a late window differ"""
    check(monkeypatch, branch, n_traj=n_traj)


@pytest.mark.parametrize("n_traj", [8, 3])
def test_mto_on_the_last_step_never_qualifies(monkeypatch, n_traj):
    check(monkeypatch, readout=False, n_traj=n_traj, last_mto=True)


def test_one_block_of_two_qualifies(monkeypatch):
    """the MTO on the last step keeps trajectory 0's workgroup on the closure pass; the other one reads in the columns"""
    check(monkeypatch, n_traj=9, last_mto=True)


@pytest.mark.parametrize("n_out", [1, 2, 4])
def test_output_counts(monkeypatch, n_out):
    check(monkeypatch, n_traj=9, n_out=n_out)


@pytest.mark.parametrize("D", [16, 9])
def test_two_systems_in_one_block(monkeypatch, D):
    check(monkeypatch, n_traj=9, D=D, n_sys=2)


@pytest.mark.parametrize("D", [16, 9])
@pytest.mark.parametrize("n_slices", [30, N_STEPS])
def test_slice_set_changes_inside_the_fast_region(monkeypatch, D, n_slices):
    check(monkeypatch, n_traj=9, D=D, n_slices=n_slices, n_out=4)


def test_repeated_execute_is_bitwise_stable(monkeypatch):
    base_env(monkeypatch)
    key, case = inputs(n_traj=9, n_slices=N_STEPS, n_out=4)
    plan = engine.Plan(*case[:5], pt=case[5])
    assert plan.sweep_readout()
    runs = []
    for _ in range(3):
        plan.execute()
        runs.append([np.array(a, copy=True) for a in plan.download()])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a, b)
    e_or = max(rel(a, b) for a, b in zip(runs[0], oracle_outputs(key)))
    assert e_or < 1e-11, e_or
