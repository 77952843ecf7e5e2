"""Liouville rows that stay exactly zero (pqd_live_rows), on the host: no GPU.

The batched sweep gives such rows no PT unit, so the analysis must never call a row dead that can hold a value. Each
case of tests/live_rows_cases.py is checked three ways:
  * engine.live_rows (the exported C function) equals the closure restated in numpy there, and the set the case
    names (for the two cases that must widen the x-only mask: a strict superset of it);
  * the CPU oracle, which contracts every row, gives outputs np.array_equal to its own after the PT slices of every
    row reported dead are replaced by finite random values (a row that ever held a nonzero value would show);
  * a control: scaling the slice of one live row does change the outputs, so the comparison can fail.
The PT has one slice per row (an injective gmap), chi = 16, four slice sets.
"""
import dataclasses

import numpy as np
import pytest

from oracle import oracle
from pyaceqd_amd import engine, pt as ptmod
from tests import live_rows_cases as LC


def case_pt(N, seed):
    p = ptmod.random_pt(N, 16, D=N * N, n_slices=4, seed=seed, eps=0.2)
    return dataclasses.replace(p, gmap=np.random.default_rng(seed).permutation(N * N).astype(np.int32))


@pytest.mark.parametrize("name", LC.HOST_CASES)
def test_live_rows(name):
    sysd, grid, rho0, ops, tr, expect = LC.build(name)
    N = (sysd[0] if isinstance(sysd, list) else sysd).dim
    live = engine.live_rows(sysd, rho0, tr)
    ref = LC.numpy_live_rows(sysd, rho0, tr)
    print(f"{name}: live rows {live}")
    assert live == ref
    if expect is not None:
        assert live == expect
    else:  # an MTO or an initial coherence that leaves G, X, B: more than the x-only rows
        assert set(live) > set(LC.X_ONLY)
    dead = [a for a in range(N * N) if a not in live]
    pt = case_pt(N, 7 + N)
    base = oracle.propagate(sysd, grid, rho0, ops, tr, pt=pt)
    # the pulse lies inside the window: without the (random, unnormalised) PT the outputs are O(0.01 - 1), not rounding noise
    peak = max(float(np.max(np.abs(o))) for o in oracle.propagate(sysd, grid, rho0, ops, tr))
    assert 1e-2 < peak < 10, peak
    if dead:
        rng = np.random.default_rng(5)
        Q = pt.Q.copy()
        shape = Q[:, pt.gmap[dead]].shape
        Q[:, pt.gmap[dead]] = rng.normal(size=shape) + 1j * rng.normal(size=shape)
        scr = oracle.propagate(sysd, grid, rho0, ops, tr, pt=dataclasses.replace(pt, Q=Q))
        for a, b in zip(base, scr):
            assert np.array_equal(a, b)
    Q = pt.Q.copy()
    Q[:, pt.gmap[live[-1]]] *= 0.5
    ctl = oracle.propagate(sysd, grid, rho0, ops, tr, pt=dataclasses.replace(pt, Q=Q))
    assert any(not np.array_equal(a, b) for a, b in zip(base, ctl))


def test_no_trajectories_argument():
    """traj may be left out: the closure under the generators alone"""
    sysd, _, rho0, _, _, _ = LC.build("x_only")
    assert engine.live_rows(sysd, rho0) == LC.X_ONLY
    sysd, _, rho0, _, _, _ = LC.build("both")
    assert engine.live_rows(sysd, rho0) == LC.ALL16
