"""The lean sweep applies F(n) to the live rows only: three k-steps of the compact row index instead of four
(pt_sweep.hip LeanCol KC = 3, pqd_live_col_map). GPU only.

Shape: that of tests/test_gpu_live_rows.py (N = 4, chi = 64, the 9 trajectories of tests/live_rows_cases.py with windows
of 48 steps: steps of the fast region before a slot's window run the form without outputs, steps inside it the form
that reads them), PQD_SPLIT=0, PQD_MSPLIT=0, PQD_BT=8. Every compacted case checks that
  * Plan.sweep_colk() is 3 and describe() ends with colk=3 behind live= and parts=;
  * the outputs are np.array_equal to the same plan's with PQD_LIVE_COL=0 (four k-steps, colk absent from describe(),
    the rest of the line unchanged) and with PQD_LIVE_ROWS=0 (every row contracted and multiplied): the compact index is
    increasing on the live rows and the f64 MFMA adds its products as an ordered FMA chain, so every live row gets the
    same products in the same order and the outputs are summed from the same values in the same order;
  * they are within 1e-11 of the CPU oracle, the bound of the neighbouring lean tests.
Cases: 10, 10, 9 and 12 live rows and a plan of two systems (its workgroups mix systems, so they load F and W from
memory and not from the staging area) at 1, 2 and 4 outputs; a dictionary PT, PQD_LEAN_STAGE=0 and a trunk pre-pass on
the 10-row case; 13 and 16 live rows keep four k-steps and the describe() line of PQD_LIVE_COL=0; PQD_LIVE_ROWS=2
(synchronize verifies that no stored M or F leads from a live column into a dead row, which is what lets the product
leave those rows out) passes with the same outputs.
"""
import numpy as np
import pytest

from pyaceqd_amd import engine
from tests.test_gpu_branching import rel
from tests.test_gpu_live_rows import case, make_pt, oracle_outputs, run

pytestmark = pytest.mark.gpu


def setup(monkeypatch, env=()):
    monkeypatch.setenv("PQD_SPLIT", "0")
    monkeypatch.setenv("PQD_MSPLIT", "0")
    monkeypatch.setenv("PQD_BT", "8")
    for k, v in env:
        monkeypatch.setenv(k, v)


def check(monkeypatch, name, n_out=2, dictionary=False, env=()):
    setup(monkeypatch, env)
    c, pt = case(name, n_out), make_pt(64, dictionary)
    plan, got = run(c, pt)
    assert plan.info()[:2] == (engine.Plan.PATHS[1], 8)
    assert plan.sweep_lean() and plan.sweep_readout()
    d = plan.describe()
    assert plan.sweep_colk() == 3 and d["parts"] == "1" and d["colk"] == "3", d
    assert list(d)[-3:] == ["live", "parts", "colk"]
    n_live = len(plan.live_rows())
    assert 9 <= n_live <= 12
    monkeypatch.setenv("PQD_LIVE_COL", "0")
    plan4, four = run(c, pt)
    d4 = plan4.describe()
    assert plan4.sweep_colk() == 4 and "colk" not in d4
    assert {k: v for k, v in d.items() if k != "colk"} == d4
    monkeypatch.delenv("PQD_LIVE_COL")
    monkeypatch.setenv("PQD_LIVE_ROWS", "0")
    plan0, all_rows = run(c, pt)
    assert plan0.sweep_colk() == 4 and "live" not in plan0.describe()
    monkeypatch.setenv("PQD_LIVE_ROWS", "1")
    ref = oracle_outputs(name, n_out, 64, dictionary)
    assert len(got) == len(four) == len(all_rows) == len(ref) == 9
    d_four = max(float(np.max(np.abs(a - b))) for a, b in zip(got, four))
    d_all = max(float(np.max(np.abs(a - b))) for a, b in zip(got, all_rows))
    e_or = max(rel(a, b) for a, b in zip(got, ref))
    print(f"col compact {name} n_out={n_out} dict={dictionary} env={dict(env)}: {n_live} live, stage={plan.sweep_stage()}, "
          f"largest difference to PQD_LIVE_COL=0 {d_four:.3e}, to PQD_LIVE_ROWS=0 {d_all:.3e}, vs oracle {e_or:.3e}")
    for a, b, z in zip(got, four, all_rows):
        assert np.array_equal(a, b)
        assert np.array_equal(a, z)
    assert e_or < 1e-11, e_or
    return plan, got


@pytest.mark.parametrize("n_out", [1, 2, 4])
@pytest.mark.parametrize("name", ["x_only", "y_only", "x_only_no_lindblad", "mto_left_no_lindblad", "two_systems"])
def test_compacted(monkeypatch, name, n_out):
    plan, _ = check(monkeypatch, name, n_out=n_out)
    if name == "two_systems":   # trajectories are packed by system (5 and 4): the full workgroup holds both systems and
        assert plan.sweep_stage() == 1   # loads its operands in place, the one with a single slot stages
    else:
        assert plan.sweep_stage() >= 1


def test_dictionary_pt(monkeypatch):
    check(monkeypatch, "x_only", n_out=4, dictionary=True)


def test_operands_loaded_in_place(monkeypatch):
    plan, _ = check(monkeypatch, "x_only", n_out=4, env=[("PQD_LEAN_STAGE", "0")])
    assert plan.sweep_stage() == 0


def test_trunk_pre_pass(monkeypatch):
    plan, _ = check(monkeypatch, "x_only", env=[("PQD_TRUNK", "1")])
    assert int(plan.describe()["n_trunk"]) >= 1


@pytest.mark.parametrize("name", ["mto_leaves", "both"])
def test_more_than_12_live_rows_keep_four_k_steps(monkeypatch, name):
    setup(monkeypatch)
    c, pt = case(name, 2), make_pt(64, False)
    plan, got = run(c, pt)
    assert len(plan.live_rows()) == (13 if name == "mto_leaves" else 16)
    assert plan.sweep_lean() and plan.sweep_colk() == 4
    monkeypatch.setenv("PQD_LIVE_COL", "0")
    plan4, four = run(c, pt)
    assert plan.describe() == plan4.describe() and "colk" not in plan.describe()
    for a, b in zip(got, four):
        assert np.array_equal(a, b)


def test_zero_blocks_verified(monkeypatch):
    """PQD_LIVE_ROWS=2: the plan still compacts, synchronize finds no entry of M or F from a live column into a dead
    row, and the outputs are those of the default plan"""
    _, got = check(monkeypatch, "x_only", n_out=4)
    monkeypatch.setenv("PQD_LIVE_ROWS", "2")
    c, pt = case("x_only", 4), make_pt(64, False)
    plan2, verified = run(c, pt)
    assert plan2.sweep_colk() == 3
    for a, b in zip(got, verified):
        assert np.array_equal(a, b)
