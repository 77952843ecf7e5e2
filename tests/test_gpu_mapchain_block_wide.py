"""The periodic map-chain sweep by position (csrc/mapchain_wide.hip, pqd_calc_onetime_parallel_block_wide):
calc_onetime_parallel_block at dim 7..24 under the wide opt-in, and at dim 2..6 through the wide entry, against the C
oracle, the packed kernels of mapchain.hip and the reference Fortran's goldens. GPU only.

rel(), the inputs (_mk, _ops, H.random_rho) and the bound 1e-11 (TOL_SWEEP) are those of
tests/test_gpu_mapchain_wide.py; 1e-12 against the Fortran goldens is the bound tests/test_gpu_parity.py gives them.
The first test takes the sizes and the nine-point time_sparse of test_gpu_parity.py::
test_mapchain_blocked_sweep_block_mode_vs_oracle (n_tb 12, nx_tau 9, n_map 7 and 18: trunk ends inside the period, at
n_tb, inside (n_tb, n_map] and past it), the dims of test_gpu_mapchain_wide.py's first test for their tile shapes.

Worst values observed on an MI355X: against the oracle 3.0e-14 over the six dims (dim 7, n_map 7), 1.2e-14 over the
family and tile edges, 3.0e-15 for the degenerate sizes; the wide entry at dim 2..6 7.2e-15 against the oracle, 1.5e-14
against the default path, 1.2e-15 against the Fortran goldens. The end-to-end figures are in test_end_to_end_at_dim_8's
docstring.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle
from pyaceqd_amd import _lib
from pyaceqd_amd.two_time import propagate_tau_module as M
from tests import helpers as H

pytestmark = pytest.mark.gpu
F = lambda maps: np.asfortranarray(np.asarray(maps).transpose(1, 2, 0))  # noqa: E731
TS9 = np.array([0.0, 0.15, 0.4, 0.75, 1.1, 1.2, 1.25, 2.0, 3.3])
TOL_SWEEP, TOL_GOLDEN = 1e-11, 1e-12


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def _mk(rng, N2, dim):
    return np.eye(N2) + 0.05 * (rng.normal(size=(N2, N2)) + 1j * rng.normal(size=(N2, N2))) / dim


def _ops(rng, dim):
    return [rng.normal(size=(dim, dim)) + 1j * rng.normal(size=(dim, dim)) for _ in range(3)]


@functools.lru_cache(maxsize=None)
def _inputs(dim, n_map):
    """(dm_block in the Fortran layout, dm_s, rho, ops) of one size: built once, read-only afterwards"""
    rng = np.random.default_rng(2000 + 31 * dim + n_map)
    N2 = dim * dim
    dm_block = F(np.stack([_mk(rng, N2, dim) for _ in range(n_map)]))
    dm_s = np.asfortranarray(_mk(rng, N2, dim))
    dm_block.setflags(write=False)
    dm_s.setflags(write=False)
    return dm_block, dm_s, H.random_rho(dim, seed=dim).reshape(N2), _ops(rng, dim)


def _ts_of_ends(ends):
    """time_sparse whose trunk ends on a 0.1 grid are `ends` (p >= 1: between the grid points; 0: t = 0)"""
    return np.array([0.0 if p == 0 else 0.1 * p - 0.05 for p in ends])


def _time_for(ts):
    return np.round(np.arange(int(round(max(ts) / 0.1)) + 4) * 0.1, 6)


def _args(dim, n_tb, nx_tau, n_map, ts, time=None):
    dm_block, dm_s, rho, ops = _inputs(dim, n_map)
    return (dm_block, dm_s, rho, n_tb, nx_tau, dim, *ops, _time_for(ts) if time is None else time, ts)


def _sweep(dim, n_tb, nx_tau, n_map, ts, name, time=None):
    a = _args(dim, n_tb, nx_tau, n_map, ts, time)
    ref = oracle.calc_onetime_parallel_block(*a)
    got = M.calc_onetime_parallel_block_wide(*a)
    assert got.shape == ref.shape == (len(ts), n_tb * nx_tau + 1) and np.all(np.isfinite(got))
    e = rel(got, ref)
    print(f"{name}: GPU vs oracle {e:.3e}")
    assert e < TOL_SWEEP
    return got, ref


def _schedule(time, ts, n_tb, nx_tau, n_map):
    L = _lib.lib()
    time, ts = np.ascontiguousarray(time, dtype=np.float64), np.ascontiguousarray(ts, dtype=np.float64)
    rows = C.c_int32(-1)
    a = (_lib.fptr(time), len(time), _lib.fptr(ts), len(ts), n_tb, nx_tau, n_map)
    _lib.check(L.pqd_mc_wide_block_schedule(*a, None, C.byref(rows), None, 0))
    sched = np.zeros((rows.value, 9), dtype=np.int32)
    _lib.check(L.pqd_mc_wide_block_schedule(*a, None, C.byref(rows), _lib.iptr(sched), rows.value))
    return sched


def _timing():
    ms, nl = C.c_double(), C.c_int32()
    _lib.check(_lib.lib().pqd_mc_wide_timing(_lib.context().handle, C.byref(ms), C.byref(nl)))
    return ms.value, nl.value


# ------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("n_map", [7, 18])
@pytest.mark.parametrize("dim", [7, 8, 10, 13, 16, 24])
def test_block_vs_oracle(dim, n_map):
    n_tb, nx_tau = (5, 3) if dim == 24 else (12, 9)
    _sweep(dim, n_tb, nx_tau, n_map, TS9, f"block dim {dim} n_tb {n_tb} nx_tau {nx_tau} n_map {n_map}",
           time=np.round(np.arange(60) * 0.1, 6))


# ------------------------------------------------------------------------------------------ 2. family and tile edges
def _edge_ends(n_tb, n_ring, n_str):
    """n_ring trunk ends inside the period (n_tb - 1 among them), then n_str from n_tb on (n_tb first, then n_tb + 1
    .. n_tb + 4: with n_map = 6 and n_tb = 4 those at 5 and 6 lie inside (n_tb, n_map])"""
    return sorted((n_tb - 1 - k) % n_tb for k in range(n_ring)) + sorted(n_tb + k % 5 for k in range(n_str))


@pytest.mark.parametrize("n_ring", [0, 1, 15, 16, 17, 31, 32, 33])
@pytest.mark.parametrize("n_map", [2, 4, 6])
@pytest.mark.parametrize("dim", [7, 9])
def test_family_and_tile_edges(dim, n_map, n_ring):
    """the border between the ring and the straight trajectories around the 16-column tiles and the 32-column
    workgroup tiles, with 0, 1 and 17 straight trajectories behind it: a tile that straddles the border is issued in
    both families"""
    n_tb, nx_tau = 4, 3
    for n_str in (0, 1, 17):
        if n_ring + n_str == 0:
            continue
        ends = _edge_ends(n_tb, n_ring, n_str)
        assert (n_ring == 0 or n_tb - 1 in ends) and (n_str == 0 or n_tb in ends)
        assert n_str < 17 or n_map < 6 or any(n_tb < p <= n_map for p in ends)
        _sweep(dim, n_tb, nx_tau, n_map, _ts_of_ends(ends), f"dim {dim} n_map {n_map} ring {n_ring} straight {n_str}")


# ------------------------------------------------------------------------------------------ 3. degenerate sizes
@pytest.mark.parametrize("case", ["nx_tau 0", "n_tb 1", "one ring", "one straight"])
@pytest.mark.parametrize("dim", [7, 10])
def test_degenerate_sizes(dim, case):
    n_tb, nx_tau, n_map, ends = {"nx_tau 0": (5, 0, 3, [0, 2, 4, 5, 7]), "n_tb 1": (1, 2, 1, [0, 0, 1, 2, 4]),
                                 "one ring": (4, 3, 2, [3]), "one straight": (4, 3, 6, [5])}[case]
    got, _ = _sweep(dim, n_tb, nx_tau, n_map, _ts_of_ends(ends), f"dim {dim} {case}")
    assert got.shape == (len(ends), n_tb * nx_tau + 1)


# ------------------------------------------------------------------------------------------ 4. one step launch a position
@pytest.mark.parametrize("n_map", [2, 6])
def test_one_step_launch_per_position(n_map):
    dim, n_tb, nx_tau = 7, 4, 3
    ends = _edge_ends(n_tb, 17, 17)
    ts = _ts_of_ends(ends)
    _sweep(dim, n_tb, nx_tau, n_map, ts, f"launch count, n_map {n_map}")
    _, launches = _timing()
    sched = _schedule(_time_for(ts), ts, n_tb, nx_tau, n_map).tolist()
    steps = sum(1 for r in sched[:-1] if r[1] > r[0] or r[4] > r[3] or r[5])
    spawns = sum(1 for r in sched if r[8] > r[7])
    two = sum(1 for r in sched[:-1] if r[1] > r[0] and (r[4] > r[3] or r[5]) and r[2] != r[6])
    print(f"n_map {n_map}: {launches} launches = 1 + {steps} steps + {spawns} spawns; {two} positions with two families")
    assert two > 0
    assert launches == 1 + steps + spawns


# ------------------------------------------------------------------------------------------ 5. reproducibility
@pytest.mark.parametrize("dim", [7, 16])
def test_same_bits_twice(dim):
    a = _args(dim, 12, 9, 18, TS9, np.round(np.arange(60) * 0.1, 6))
    first = M.calc_onetime_parallel_block_wide(*a)
    assert np.array_equal(first, M.calc_onetime_parallel_block_wide(*a))
    assert np.array_equal(first, M.calc_onetime_parallel_block(*a, wide=True))


# ------------------------------------------------------------------------------------------ 6. dim 2..6
@pytest.mark.parametrize("n_map", [7, 18])
@pytest.mark.parametrize("dim", [2, 3, 4, 5, 6])
def test_wide_entry_below_dim_7(dim, n_map):
    time = np.round(np.arange(60) * 0.1, 6)
    got, _ = _sweep(dim, 12, 9, n_map, TS9, f"wide entry dim {dim} n_map {n_map}", time=time)
    a = _args(dim, 12, 9, n_map, TS9, time)
    default = M.calc_onetime_parallel_block(*a)
    assert np.array_equal(default, M.calc_onetime_parallel_block(*a, wide=True))   # dim <= 6: the keyword changes nothing
    e = rel(got, default)
    print(f"wide entry dim {dim} n_map {n_map}: vs the default path {e:.3e}")
    assert e < TOL_SWEEP


@pytest.mark.parametrize("dim", [2, 4, 6])
def test_wide_entry_vs_fortran_golden(golden_dir, dim):
    z = np.load(f"{golden_dir}/fortran_onetime_block_d{dim}.npz")
    r = M.calc_onetime_parallel_block_wide(dm_block=F(z["dm_block"]), dm_s=z["dm_s"], rho_init=z["rho_init"],
                                           n_tb=int(z["n_tb"]), nx_tau=int(z["nx_tau"]), dim=dim, opa=z["opa"],
                                           opb=z["opb"], opc=z["opc"], time=z["time"], time_sparse=z["time_sparse"])
    e = rel(r, z["result"])
    print(f"wide entry dim {dim} vs the Fortran golden: {e:.3e}")
    assert e < TOL_GOLDEN


# ------------------------------------------------------------------------------------------ 7. end to end
def _indist(system, lift, tmp_path):
    """Indistinguishability(dm=True, phonons=False) on a sensor model, sigma of the two-level system lifted by `lift`;
    tb, gaussian_t and dt of test_gpu_parity.py::test_indistinguishability_map_sweeps_vs_reference_golden. The decay
    (lifetime 2) and the sensor losses empty the system within a period."""
    from pyaceqd_amd.pulses import ChirpedPulse
    from pyaceqd_amd.two_time.purity import Indistinguishability
    rest = np.eye(2 ** lift.count("otimes"))
    low = np.kron(np.array([[0, 1], [0, 0]], dtype=complex), rest)
    opts = {"gamma_e": 0.5, "lindblad": True, "phonons": False, "wide_maps": True, "epsilon": 0.05, "linewidth1": 0.5,
            "temp_dir": str(tmp_path) + "/"}
    return Indistinguishability(system, "|0><1|_2" + lift, "|1><0|_2" + lift, ChirpedPulse(tau_0=1.0, e_start=0, e0=1, t0=6),
                                options=opts, dm=True, sigma_x_mat=low, sigma_xdag_mat=low.conj().T, dt=0.1, tb=20,
                                dt_small=0.5, gaussian_t=12)


def _g2_tl_vs_direct(system, lift, tmp_path):
    """max rel() of G2_tl (the periodic time-local map chain) against G2() (direct propagation with multitime operators)"""
    tl = _indist(system, lift, tmp_path)
    (t_a, a), (t_b, b) = tl.G2_tl(), tl.G2()
    assert a.shape == b.shape and np.array_equal(t_a, t_b) and np.max(np.abs(b)) > 1e-3
    return rel(a, b)


# G2_tl against G2() at dim 4 on tls_one_sensor, _g2_tl_vs_direct(tls_one_sensor, " otimes Id_2", tmp_path), where every
# stage is the dim <= 6 code this sweep leaves as it was (measured on an MI355X). The two are not the same number to
# rounding: G2() propagates through a train of pulses, G2_tl repeats the maps of one period.
E2E_DIM4 = 7.615e-04


def test_end_to_end_at_dim_8(monkeypatch, tmp_path):
    """Indistinguishability(tls_two_sensor, dm=True, wide_maps=True): with the maps computed once on the object, G1_tl
    and G2_tl on the GPU sweep against the same calls with oracle.calc_onetime_parallel_block in its place (1e-11);
    calc_indistinguishability gives two finite numbers in [0, 1]; G2_tl against the direct G2() within 10 times the
    same comparison at dim 4 on tls_one_sensor (E2E_DIM4 = 7.615e-04).

    Measured at dim 8: G1_tl 6.7e-16 and G2_tl 5.4e-16 from the oracle's sweep on the same maps; indistinguishability
    0.8693, purity 0.7951; G2_tl 3.581e-05 from G2(), under the bound 7.615e-03."""
    from pyaceqd_amd.two_level_system.tls import tls_two_sensor
    from pyaceqd_amd.two_time import purity
    lift = " otimes Id_2 otimes Id_2"
    tl = _indist(tls_two_sensor, lift, tmp_path)
    tl.get_tl()
    assert tl.tl_map.shape == (64, 64)
    g1, g2 = tl.G1_tl()[1], tl.G2_tl()[1]
    _, nl = _timing()
    assert nl > 0                                            # the sweep by position ran
    ind = np.array(tl.calc_indistinguishability())
    g2_direct = tl.G2()[1]
    with monkeypatch.context() as mp:
        mp.setattr(purity.propagate_tau_module, "calc_onetime_parallel_block",
                   lambda *a, wide=None, **k: oracle.calc_onetime_parallel_block(*a, **k))
        g1_ref, g2_ref = tl.G1_tl()[1], tl.G2_tl()[1]
    e1, e2, e_d = rel(g1, g1_ref), rel(g2, g2_ref), rel(g2, g2_direct)
    print(f"dim 8: G1_tl vs oracle sweep {e1:.3e}, G2_tl {e2:.3e}; indistinguishability, purity {ind}; "
          f"G2_tl vs G2() {e_d:.3e}")
    assert np.max(np.abs(g2_ref)) > 1e-3 and e1 < TOL_SWEEP and e2 < TOL_SWEEP
    assert ind.shape == (2,) and np.all(np.isfinite(ind)) and np.all((ind >= 0) & (ind <= 1))
    assert e_d < 10 * E2E_DIM4


# ------------------------------------------------------------------------------------------ 8. refusals
def _unsupported(fn, *a, **k):
    with pytest.raises(_lib.PQDError) as ei:
        fn(*a, **k)
    assert ei.value.code == _lib.PQD_ERR_UNSUPPORTED, ei.value
    return str(ei.value)


def test_refusals(monkeypatch):
    z = lambda *s: np.zeros(s, dtype=complex, order="F")  # noqa: E731
    t, ts = np.array([0.0, 0.1]), np.array([0.0])
    o8 = [z(8, 8)] * 3
    monkeypatch.delenv("PQD_WIDE_MAPS", raising=False)
    for kw in ({}, {"wide": False}):
        assert "dim 8 not in [2, 6]" in _unsupported(M.calc_onetime_parallel_block, z(64, 64, 2), z(64, 64), z(64), 2, 1,
                                                      8, *o8, t, ts, **kw)
    assert "dim 8 not in [2, 6]" in _unsupported(M.calc_twotime_phonon_block, z(64, 64, 1, 2), z(64, 64, 2), z(64, 64, 2),
                                                  z(64, 64), z(64), 2, 1, 8, *o8, t, ts)
    o25 = [z(25, 25)] * 3
    a25 = (z(625, 625, 1), z(625, 625), z(625), 2, 1, 25, *o25, t, ts)
    assert "dim 25 not in [2, 24]" in _unsupported(M.calc_onetime_parallel_block_wide, *a25)
    assert "dim 25 not in [2, 24]" in _unsupported(M.calc_onetime_parallel_block, *a25, wide=True)
