"""The lean sweep's column operands staged in LDS a step ahead (pt_sweep.hip LeanStage). GPU only.

In the fast region of a workgroup whose trajectories share one system, the PT phase of step n copies F(n + 1), W(n + 1)
and the closure vector step n + 1 reads into LDS, and the column phase of step n + 1 takes them from there; workgroups
that mix systems, and every workgroup with PQD_LEAN_STAGE=0, load them where they are used. The values and every
operation on them are the same, so each case asks for outputs bitwise equal to the PQD_LEAN_STAGE=0 run of the same
plan, for 1e-11 against the CPU oracle (the bound of the readout tests), and for Plan.sweep_stage() to count the
workgroups that stage.

The cases are those of tests/test_gpu_sweep_readout.py (N = 4, chi = 64, 40 steps, PQD_SPLIT=0, PQD_BT=8; built once and
shared with it, the oracle's outputs too): trajectory i has its MTO pair at step 1 + (5 i mod 14) and its window ends at
40 - (3 i mod 11), so slots leave their windows inside the fast region one by one (F still needed, W and the closure
vector not), and trajectory 2 opens its window six steps after its MTO (a slot outside its window when the region
starts). The drives are Gaussian envelopes on rotating phases, so F(n) and W(n) differ at every step (F staged for the
wrong step shows), and the 30- and 40-slice PTs change the slice set, and with it the closure vector, inside the region
(the vector of the wrong set shows).
  * 8, 9 and 3 trajectories, PQD_BRANCH 0 and 1: a full workgroup, two of which one has seven empty slots, a partial one;
  * 1, 2 and 4 outputs: the W piece loaded by 16, 32 and 64 lanes;
  * n_slices 30 and 40 with D = 16 and the 9-slice dictionary;
  * two systems: the block order groups trajectories by system, so 8 trajectories make one mixed workgroup (no staging)
    and 9 a mixed one and a second one with a single trajectory (staging): same results both ways;
  * two execute() calls of one plan, bitwise equal (nothing stale in the area from the run before);
  * PQD_LEAN_RO=0 and PQD_SWEEP_LEAN=0: no fast region, sweep_stage() is 0.
"""
import numpy as np
import pytest

from pyaceqd_amd import engine
from tests.test_gpu_branching import rel
from tests.test_gpu_sweep_readout import base_env, inputs, oracle_outputs, run

pytestmark = pytest.mark.gpu

BT = 8


def staging_blocks(n_traj, n_sys=1):
    """workgroups that stage: slots are filled eight at a time in block order, which groups the trajectories by system
    (trajectory i belongs to system i mod n_sys); each workgroup of these cases has fast steps (every MTO and
    activation lies before step 15 and every window ends at step 30 or later), so it stages when it holds one system"""
    systems = sorted(i % n_sys for i in range(n_traj))
    return sum(len(set(systems[b:b + BT])) == 1 for b in range(0, n_traj, BT))


def check(monkeypatch, branch="1", **kw):
    base_env(monkeypatch, branch)
    key, case = inputs(**kw)
    plan, got = run(case)
    assert plan.info()[:2] == (engine.Plan.PATHS[1], BT)
    assert plan.sweep_lean() and plan.sweep_readout()
    want = staging_blocks(kw["n_traj"], kw.get("n_sys", 1))
    assert plan.sweep_stage() == want, (plan.sweep_stage(), want)
    monkeypatch.setenv("PQD_LEAN_STAGE", "0")
    plan_o, old = run(case)
    assert plan_o.sweep_lean() and plan_o.sweep_readout() and plan_o.sweep_stage() == 0
    ref = oracle_outputs(key)
    assert len(got) == len(old) == len(ref) == kw["n_traj"]
    for a, b, c in zip(got, old, ref):
        assert a.shape == b.shape == c.shape
    d_old = max(float(np.max(np.abs(a - b))) for a, b in zip(got, old))
    e_or = max(rel(a, b) for a, b in zip(got, ref))
    print(f"stage {kw} branch={branch}: {want} staging workgroups, largest difference to PQD_LEAN_STAGE=0 {d_old:.3e}, "
          f"vs oracle {e_or:.3e}")
    assert d_old == 0.0, d_old
    for a, b in zip(got, old):
        assert np.array_equal(a, b)
    assert e_or < 1e-11, e_or


@pytest.mark.parametrize("branch", ["0", "1"])
@pytest.mark.parametrize("n_traj", [8, 9, 3])
def test_block_shapes(monkeypatch, n_traj, branch):
    check(monkeypatch, branch, n_traj=n_traj)


@pytest.mark.parametrize("n_out", [1, 2, 4])
def test_output_counts(monkeypatch, n_out):
    check(monkeypatch, n_traj=9, n_out=n_out)


@pytest.mark.parametrize("D", [16, 9])
@pytest.mark.parametrize("n_slices", [30, 40])
def test_slice_set_changes_inside_the_fast_region(monkeypatch, D, n_slices):
    check(monkeypatch, n_traj=9, D=D, n_slices=n_slices, n_out=4)


@pytest.mark.parametrize("n_traj, staging", [(8, 0), (9, 1)])
def test_two_systems_in_one_block_do_not_stage(monkeypatch, n_traj, staging):
    assert staging_blocks(n_traj, 2) == staging
    check(monkeypatch, n_traj=n_traj, n_sys=2)


def test_repeated_execute_is_bitwise_stable(monkeypatch):
    base_env(monkeypatch)
    key, case = inputs(n_traj=9, n_slices=40, n_out=4)
    plan = engine.Plan(*case[:5], pt=case[5])
    assert plan.sweep_stage() == 2
    runs = []
    for _ in range(2):
        plan.execute()
        runs.append([np.array(a, copy=True) for a in plan.download()])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    e_or = max(rel(a, b) for a, b in zip(runs[0], oracle_outputs(key)))
    assert e_or < 1e-11, e_or


@pytest.mark.parametrize("switch", ["PQD_LEAN_RO", "PQD_SWEEP_LEAN"])
def test_no_fast_region_no_staging(monkeypatch, switch):
    base_env(monkeypatch)
    monkeypatch.setenv(switch, "0")
    key, case = inputs(n_traj=9)
    plan, got = run(case)
    assert not plan.sweep_readout() and plan.sweep_stage() == 0
    e_or = max(rel(a, b) for a, b in zip(got, oracle_outputs(key)))
    assert e_or < 1e-11, e_or
