"""PT rows that stay exactly zero get no unit in the batched sweep (pqd_live_rows, pt_sweep.hip LeanPt partial units;
DESIGN.md §4.1). GPU only.

Shape: N = 4, chi = 64 (the lean instance exists for no other bond), the 9 trajectories of tests/live_rows_cases.py
(one full workgroup and one with a single occupied slot; t1 = 4 .. 12, windows of 48 steps, the pulse inside the t1
grid), 2 and 4 outputs, PQD_SPLIT=0, PQD_MSPLIT=0 and PQD_BT=8 so that the plan runs the batched sweep. Every case checks:
  * the outputs are np.array_equal to the same library's with PQD_LIVE_ROWS=0 (all rows contracted, the list the plan
    always had): skipped rows are zero, and the rows that are contracted, whole or in column-group parts, run the same
    MFMAs with the same operands in the same order;
  * they are within 1e-11 of the CPU oracle (the bound of the neighbouring lean tests);
  * PQD_LIVE_ROWS=2 (synchronize checks the stored M and F for a nonzero entry from a live column into a dead row)
    passes and gives the same outputs again;
  * Plan.live_rows() is the set the host test asks for, and describe() says live= / parts= exactly when rows are left out;
  * with every row live, describe() is the line of the PQD_LIVE_ROWS=0 plan, units hash included;
  * with the PT slices of the dead rows replaced by finite random values the outputs do not change: the rows are really
    skipped (and with one live row's slice scaled they do change).
Cases: every host case at N = 4 that changes the mask, a dictionary PT (rows sharing slices: units of two rows, split
where the quarters need it), PQD_SWEEP_LEAN=0 (the general instance with rows absent from its list), PQD_LEAN_STAGE=0,
PQD_LIVE_PART=0 (whole rows of the live ones only), a plan with the trunk pre-pass (which keeps all rows), a
chi = 32 plan on the general instance, and the x-polarised six-level model (N = 6: 10 live rows of 36) on the general
instance with four trajectories per workgroup.
"""
import dataclasses

import numpy as np
import pytest

from oracle import oracle
from pyaceqd_amd import engine, opgrammar, pt as ptmod
from tests import live_rows_cases as LC
from tests.test_gpu_branching import rel

pytestmark = pytest.mark.gpu

N = 4
_cases, _pts, _oracle = {}, {}, {}


def case(name, n_out):
    if (name, n_out) not in _cases:
        _cases[name, n_out] = LC.build(name, n_out)
    return _cases[name, n_out]


def make_pt(chi, dictionary, N=N):
    """a random PT of 5 slice sets: one slice per row in a shuffled order, or the biexciton's 9-entry dictionary"""
    if (chi, dictionary, N) not in _pts:
        if dictionary:
            gmap, pairs = ptmod.pair_dictionary(opgrammar.to_matrix("1*(|1><1|_4 + |2><2|_4) + 2*|3><3|_4", N))
            p = ptmod.random_pt(N, chi, D=len(pairs), n_slices=5, seed=chi + 9, eps=0.12)
        else:
            gmap = np.random.default_rng(chi).permutation(N * N).astype(np.int32)
            p = ptmod.random_pt(N, chi, D=N * N, n_slices=5, seed=chi + 16, eps=0.12)
        _pts[chi, dictionary, N] = dataclasses.replace(p, gmap=np.asarray(gmap, dtype=np.int32))
    return _pts[chi, dictionary, N]


def oracle_outputs(name, n_out, chi, dictionary):
    key = (name, n_out, chi, dictionary)
    if key not in _oracle:
        sysd, grid, rho0, ops, tr, _ = case(name, n_out)
        _oracle[key] = oracle.propagate(sysd, grid, rho0, ops, tr, pt=make_pt(chi, dictionary, len(rho0)), nthreads=8)
    return _oracle[key]


def run(c, pt):
    sysd, grid, rho0, ops, tr, _ = c
    plan = engine.Plan(sysd, grid, rho0, ops, tr, pt=pt)
    plan.execute()
    return plan, plan.download()


def check(monkeypatch, name, n_out=2, chi=64, dictionary=False, lean=True, parts=None, env=(), N=N, bt=8):
    monkeypatch.setenv("PQD_SPLIT", "0")
    monkeypatch.setenv("PQD_MSPLIT", "0")
    monkeypatch.setenv("PQD_BT", "8")
    for k, v in env:
        monkeypatch.setenv(k, v)
    c, pt = case(name, n_out), make_pt(chi, dictionary, N)
    expect = c[5]
    plan, got = run(c, pt)
    assert plan.info()[:2] == (engine.Plan.PATHS[1], bt)
    assert plan.sweep_lean() == lean
    live, d = plan.live_rows(), plan.describe()
    assert live == engine.live_rows(c[0], c[2], c[4])
    if expect is not None:
        assert live == expect
    dead = [a for a in range(N * N) if a not in live]
    assert ("live" in d) == bool(dead)
    if dead:
        assert int(d["live"], 16) == sum(1 << a for a in live)
        if parts is not None:
            assert d["parts"] == str(parts), d
    # the same plan with every row contracted
    monkeypatch.setenv("PQD_LIVE_ROWS", "0")
    plan0, all_rows = run(c, pt)
    d0 = plan0.describe()
    assert plan0.live_rows() == list(range(N * N)) and "live" not in d0
    if dead:
        assert d["units"] != d0["units"]
    else:
        assert d == d0
    # ... and with the operators' zero blocks verified at synchronize
    monkeypatch.setenv("PQD_LIVE_ROWS", "2")
    plan2, verified = run(c, pt)
    assert plan2.live_rows() == live
    monkeypatch.setenv("PQD_LIVE_ROWS", "1")
    ref = oracle_outputs(name, n_out, chi, dictionary)
    assert len(got) == len(all_rows) == len(verified) == len(ref) == 9
    d_all = max(float(np.max(np.abs(a - b))) for a, b in zip(got, all_rows))
    e_or = max(rel(a, b) for a, b in zip(got, ref))
    print(f"live rows {name} n_out={n_out} chi={chi} dict={dictionary} env={dict(env)}: {len(live)} live, "
          f"parts={d.get('parts')}, umax={d['umax']}, largest difference to PQD_LIVE_ROWS=0 {d_all:.3e}, vs oracle {e_or:.3e}")
    for a, b, v in zip(got, all_rows, verified):
        assert np.array_equal(a, b)
        assert np.array_equal(a, v)
    assert e_or < 1e-11, e_or
    # slices that only dead rows read, scrambled: nothing changes; a live row's slice scaled: something does
    only_dead = sorted(set(pt.gmap[dead]) - set(pt.gmap[live])) if dead else []
    if only_dead:
        rng = np.random.default_rng(3)
        Q = pt.Q.copy()
        shape = Q[:, only_dead].shape
        Q[:, only_dead] = rng.normal(size=shape) + 1j * rng.normal(size=shape)
        _, scr = run(c, dataclasses.replace(pt, Q=Q))
        for a, b in zip(got, scr):
            assert np.array_equal(a, b)
        Q = pt.Q.copy()
        Q[:, pt.gmap[live[-1]]] *= 0.5
        _, ctl = run(c, dataclasses.replace(pt, Q=Q))
        assert any(not np.array_equal(a, b) for a, b in zip(got, ctl))
    return plan, d


@pytest.mark.parametrize("n_out", [2, 4])
@pytest.mark.parametrize("name, parts", [("x_only", 1), ("y_only", 1), ("x_only_no_lindblad", 1), ("mto_leaves", 0),
                                         ("mto_left_no_lindblad", 1), ("rho0_y_coherence", None), ("two_systems", 1)])
def test_masks(monkeypatch, name, parts, n_out):
    """10, 10 and 9 live rows: a whole row on every wave and quarters of the rest on eight or four of them; 12 rows: a
    whole row and a half row each; 13 rows: no balanced list of two items per wave, whole rows of the live ones; 16: all"""
    check(monkeypatch, name, n_out=n_out, parts=parts)


@pytest.mark.parametrize("name", ["both", "y_last_sample", "coupl_xy"])
def test_all_rows_live_is_the_plan_it_was(monkeypatch, name):
    check(monkeypatch, name)


@pytest.mark.parametrize("name", ["x_only", "x_only_no_lindblad"])
def test_dictionary_pt(monkeypatch, name):
    check(monkeypatch, name, n_out=4, dictionary=True)


@pytest.mark.parametrize("name", ["x_only", "x_only_no_lindblad"])
def test_general_instance(monkeypatch, name):
    """PQD_SWEEP_LEAN=0: whole-row units of the live rows on the general instance, never a partial unit"""
    check(monkeypatch, name, lean=False, parts=0, env=[("PQD_SWEEP_LEAN", "0")])


def test_general_instance_dictionary(monkeypatch):
    check(monkeypatch, "x_only", dictionary=True, lean=False, parts=0, env=[("PQD_SWEEP_LEAN", "0")])


@pytest.mark.parametrize("switch", ["PQD_LEAN_STAGE", "PQD_LEAN_RO", "PQD_LIVE_PART"])
def test_lean_switches(monkeypatch, switch):
    plan, d = check(monkeypatch, "x_only", n_out=4, parts=0 if switch == "PQD_LIVE_PART" else 1, env=[(switch, "0")])
    if switch == "PQD_LEAN_STAGE":
        assert plan.sweep_stage() == 0


def test_staging_runs_beside_partial_units(monkeypatch):
    plan, d = check(monkeypatch, "x_only", n_out=4, parts=1)
    assert plan.sweep_readout() and plan.sweep_stage() == 2


def test_trunk_pre_pass(monkeypatch):
    """the trunks contract all rows and hand their checkpoints to slots whose lists leave the dead rows out"""
    plan, d = check(monkeypatch, "x_only", parts=1, env=[("PQD_TRUNK", "1")])
    assert int(d["n_trunk"]) >= 1


def test_chi32_general_instance(monkeypatch):
    check(monkeypatch, "x_only", chi=32, lean=False, parts=0)


def test_six_level_general_instance(monkeypatch):
    """N = 6, chi = 64, four trajectories per workgroup, units of up to four rows: 10 of the 36 rows are contracted"""
    check(monkeypatch, "six_level", N=6, bt=4, lean=False, parts=0)
