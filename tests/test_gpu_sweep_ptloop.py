"""The PT phase of the lean sweep instance (pt_sweep.hip LeanPt). GPU only.

The lean instance contracts a wave's one or two PT units in a routine of its own: slice loads from a scalar base with
the k-steps unrolled and kept ahead of the MFMAs, the second unit's first k-steps loaded while the first unit finishes.
Its arithmetic is that of the general instance, so every case is held to the tolerances of test_gpu_sweep_lean: 1e-12
relative against the general instance (PQD_SWEEP_LEAN=0), 1e-11 against the CPU oracle. Cases that file does not have:
  * a slice set that changes on every step to the end of the grid (n_slices = steps) and a PT of one slice repeated
    from step 0, each with 16 slices per step and one row per unit (every wave: two one-row units) and with 9 slices
    (seven waves with one two-row unit, one wave with two one-row units); the row -> slice maps are set here so that
    the unit lists are these whatever the generator's seed;
  * one trajectory alone in a workgroup (seven empty slots), also as the second workgroup of the 9-trajectory cases;
  * one and four output operators (four is the lean limit 8 n_out 16 <= 512);
  * three execute() calls of one plan give bitwise equal outputs (a missing wait shows as run-to-run differences).
"""
import dataclasses

import numpy as np
import pytest

from oracle import oracle
from pyaceqd_amd import engine, pt as ptmod
from pyaceqd_amd.engine import Grid
from tests import helpers as H
from tests.test_gpu_branching import g2_reuse_shape, rel

pytestmark = pytest.mark.gpu

N, CHI, N_STEPS = 4, 64, 24
# row -> slice: a permutation for D = 16; for D = 9 seven slices with two rows and two with one
GMAP = {16: np.random.default_rng(16).permutation(16),
        9: np.random.default_rng(9).permutation(np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 8]))}
OPS = [H.ketbra(N, 0, 0), H.ketbra(N, 1, 0), np.eye(N), H.ketbra(N, 2, 3)]
_inputs, _oracle = {}, {}


def inputs(n_traj, D, n_slices, n_out):
    """(system, grid, rho0, ops, trajectories, pt) of a case, built once"""
    key = (n_traj, D, n_slices, n_out)
    if key not in _inputs:
        sysd = H.random_system(N, n_steps=N_STEPS, seed=70)[0]
        tr = g2_reuse_shape(N_STEPS, n_traj, N, seed=n_traj + D)
        pt = ptmod.random_pt(N, CHI, D=D, n_slices=n_slices, seed=CHI + D + n_slices, eps=0.12)
        pt = dataclasses.replace(pt, gmap=GMAP[D])
        _inputs[key] = (sysd, Grid(0.0, 0.1, N_STEPS), H.random_rho(N), OPS[:n_out], tr, pt)
    return _inputs[key]


def oracle_outputs(*key):
    if key not in _oracle:
        sysd, grid, rho0, ops, tr, pt = inputs(*key)
        _oracle[key] = oracle.propagate(sysd, grid, rho0, ops, tr, pt=pt, nthreads=8)
    return _oracle[key]


def base_env(monkeypatch):
    monkeypatch.setenv("PQD_SPLIT", "0")
    monkeypatch.setenv("PQD_BT", "8")


def run(*key):
    plan = engine.Plan(*inputs(*key)[:5], pt=inputs(*key)[5])
    plan.execute()
    return plan, plan.download()


def check(monkeypatch, *key):
    """the lean instance against the CPU oracle (1e-11) and the general instance (1e-12)"""
    base_env(monkeypatch)
    plan, got = run(*key)
    assert plan.info()[:2] == (engine.Plan.PATHS[1], 8)
    assert plan.sweep_lean()
    monkeypatch.setenv("PQD_SWEEP_LEAN", "0")
    plan_g, gen = run(*key)
    assert not plan_g.sweep_lean()
    ref = oracle_outputs(*key)
    assert len(got) == len(gen) == len(ref) == key[0]
    for a, b, c in zip(got, ref, gen):
        assert a.shape == b.shape == c.shape
    e_or = max(rel(a, b) for a, b in zip(got, ref))
    e_gen = max(rel(a, b) for a, b in zip(got, gen))
    print(f"ptloop n_traj={key[0]} D={key[1]} n_slices={key[2]} n_out={key[3]}: vs oracle {e_or:.3e}, "
          f"vs general instance {e_gen:.3e}")
    assert e_or < 1e-11, e_or
    assert e_gen < 1e-12, e_gen


@pytest.mark.parametrize("D", [16, 9])
@pytest.mark.parametrize("n_slices", [N_STEPS, 1])
def test_slice_schedule_ends(monkeypatch, D, n_slices):
    """a new slice set on every step up to the last, and one slice set repeated from step 0"""
    check(monkeypatch, 9, D, n_slices, 3)


@pytest.mark.parametrize("D", [16, 9])
def test_one_trajectory_alone(monkeypatch, D):
    check(monkeypatch, 1, D, 5, 3)


@pytest.mark.parametrize("n_out", [1, 4])
def test_output_counts(monkeypatch, n_out):
    check(monkeypatch, 9, 16, 5, n_out)


@pytest.mark.parametrize("D", [16, 9])
def test_repeated_execute_is_bitwise_stable(monkeypatch, D):
    base_env(monkeypatch)
    key = (9, D, N_STEPS, 3)
    sysd, grid, rho0, ops, tr, pt = inputs(*key)
    plan = engine.Plan(sysd, grid, rho0, ops, tr, pt=pt)
    assert plan.sweep_lean()
    runs = []
    for _ in range(3):
        plan.execute()
        runs.append([np.array(a, copy=True) for a in plan.download()])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a, b)
    e_or = max(rel(a, b) for a, b in zip(runs[0], oracle_outputs(*key)))
    assert e_or < 1e-11, e_or
