"""The map-chain sweep by position (csrc/mapchain_wide.hip): calc_onetime_parallel and propagate_tau at dim 7..24, and
at dim 2..6 under PQD_MC_WIDE=1, against the C oracle, the packed kernels of mapchain.hip and the reference Fortran's
goldens. GPU only.

Bounds as in tests/test_gpu_mapchain_paths.py, on rel() as defined there: 1e-11 for the sweep, 1e-12 for propagate_tau
(1e-12 against the Fortran goldens, the bound of tests/test_gpu_parity.py). Inputs as there: near-identity random maps
(_mk), dense random operators (_ops), H.random_rho. The dims of the first test are chosen for their tile shapes with
16 x 16 x 4 matrix-core tiles in workgroup tiles of 64 rows: n = 49 (row and k tails), 64 (exact), 100 (k exact, rows
not), 169, 256, 576 (the maximum).

Worst values observed on an MI355X: calc_onetime_parallel against the oracle 9.2e-15 over the six dims (dim 10), 1.0e-14
over the column-tile cases (dim 9, 33 trajectories with gaps), 5.7e-15 with n_tau = 0 and 1, 5.5e-15 for the window that
ends on the last map; propagate_tau 1.4e-14 (dim 24), 5.0e-15 below; PQD_MC_WIDE=1 at dim 2..6: 4.1e-15 against the
oracle, 5.7e-15 against the default path, propagate_tau 2.6e-15, 1.7e-15 against the Fortran goldens. The end-to-end
figures are in test_end_to_end_at_dim_8's docstring.
"""
import functools

import numpy as np
import pytest

from oracle import oracle
from pyaceqd_amd import _lib
from pyaceqd_amd.two_time import propagate_tau_module as M
from tests import helpers as H

pytestmark = pytest.mark.gpu
F = lambda maps: np.asfortranarray(np.asarray(maps).transpose(1, 2, 0))  # noqa: E731
TS15 = np.array([0.0, 0.05, 0.7, 0.75, 0.8, 0.8, 1.2, 1.3, 1.31, 2.55, 4.0, 6.4, 7.9, 10.0, 10.85])
TOL_SWEEP, TOL_TAU, TOL_GOLDEN = 1e-11, 1e-12, 1e-12


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def _mk(rng, N2, dim):
    return np.eye(N2) + 0.05 * (rng.normal(size=(N2, N2)) + 1j * rng.normal(size=(N2, N2))) / dim


def _ops(rng, dim):
    return [rng.normal(size=(dim, dim)) + 1j * rng.normal(size=(dim, dim)) for _ in range(3)]


@functools.lru_cache(maxsize=None)
def _inputs(dim, n_maps):
    """(maps in the Fortran layout, rho, ops, time) of one size: built once, read-only afterwards"""
    rng = np.random.default_rng(1000 + dim)
    N2 = dim * dim
    maps = F(np.stack([_mk(rng, N2, dim) for _ in range(n_maps)]))
    maps.setflags(write=False)
    time = np.round(np.arange(n_maps + 1) * 0.1, 6)
    return maps, H.random_rho(dim, seed=dim).reshape(N2), _ops(rng, dim), time


def _ts_for(n_maps, n_tau):
    """the 15-point list cut to the maps: every trunk end j - 1 + n_tau stays inside them"""
    return np.array([t for t in TS15 if int(np.sum(np.arange(n_maps + 1) * 0.1 < t - 1e-9)) + n_tau <= n_maps])


def _ts_of_ends(ends):
    """time_sparse whose trunk ends on a 0.1 grid are `ends` (p >= 1: between the grid points; 0: t = 0)"""
    return np.array([0.0 if p == 0 else 0.1 * p - 0.05 for p in ends])


def _sweep(dim, n_maps, n_tau, ts, name):
    maps, rho, ops, time = _inputs(dim, n_maps)
    a = (maps, rho, n_tau, dim, *ops, time, ts)
    ref = oracle.calc_onetime_parallel(*a, nthreads=8)
    got = M.calc_onetime_parallel(*a)
    assert got.shape == ref.shape == (len(ts), n_tau + 1) and np.all(np.isfinite(got))
    e = rel(got, ref)
    print(f"{name}: GPU vs oracle {e:.3e}")
    assert e < TOL_SWEEP
    return got, ref


# ------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("dim", [7, 8, 10, 13, 16, 24])
def test_onetime_vs_oracle(dim):
    n_maps, n_tau = (30, 8) if dim == 24 else (60, 12)
    ts = _ts_for(n_maps, n_tau)
    assert ts[0] == 0.0 and len(ts) >= 9 and np.sum(ts == 0.8) == 2   # a start at 0, two equal trunk ends
    _sweep(dim, n_maps, n_tau, ts, f"onetime dim {dim} ({len(ts)} trajectories)")


# ------------------------------------------------------------------------------------------ 2. column-tile edges
@pytest.mark.parametrize("ends", ["equal", "by one", "gaps"])
@pytest.mark.parametrize("n_t", [1, 16, 17, 33])
@pytest.mark.parametrize("dim", [7, 9])
def test_column_tile_edges(dim, n_t, ends):
    """n_t + 1 columns (the trunk state is one) around the 16-column tiles and the 32-column workgroup tiles; all
    trajectories spawned at once, one per position, and with gaps longer than the tau window (positions where only the
    trunk column is live)"""
    n_tau = 4
    p = {"equal": [3] * n_t, "by one": list(range(1, n_t + 1)), "gaps": [6 * i for i in range(n_t)]}[ends]
    n_maps = 200
    assert max(p) + n_tau <= n_maps
    _sweep(dim, n_maps, n_tau, _ts_of_ends(p), f"dim {dim} n_t {n_t} ends {ends}")


# ------------------------------------------------------------------------------------------ 3. n_tau = 0 and 1
@pytest.mark.parametrize("n_tau", [0, 1])
@pytest.mark.parametrize("dim", [7, 10])
def test_shortest_windows(dim, n_tau):
    ts = _ts_for(60, n_tau)
    assert len(ts) == 11
    got, ref = _sweep(dim, 60, n_tau, ts, f"dim {dim} n_tau {n_tau}")
    assert got.shape == (11, n_tau + 1)


# ------------------------------------------------------------------------------------------ 4. the last map
def test_window_ends_on_the_last_map():
    dim, n_maps = 7, 60
    maps, rho, ops, time = _inputs(dim, n_maps)
    ts = np.array([0.0, 0.5])  # trunk ends 0 and 5: the second sweep reads maps 6 .. 5 + n_tau of 60
    _sweep(dim, n_maps, 55, ts, "window that ends on the last map")
    with pytest.raises(ValueError, match="would read map 61 of 60"):
        M.calc_onetime_parallel(maps, rho, 56, dim, *ops, time, ts)
    # the same text as below dim 7
    m2, r2, o2, t2 = _inputs(2, 60)
    with pytest.raises(ValueError, match="would read map 61 of 60"):
        M.calc_onetime_parallel(m2, r2, 56, 2, *o2, t2, ts)
    with pytest.raises(ValueError, match="would read map"):
        M.calc_onetime_parallel(maps, rho, 0, dim, *ops, time, np.array([0.0, 7.5]))


# ------------------------------------------------------------------------------------------ 5. reproducibility
@pytest.mark.parametrize("dim", [7, 16])
def test_same_bits_twice(dim):
    maps, rho, ops, time = _inputs(dim, 60)
    a = (maps, rho, 12, dim, *ops, time, _ts_for(60, 12))
    first = M.calc_onetime_parallel(*a)
    assert np.array_equal(first, M.calc_onetime_parallel(*a))
    t = M.propagate_tau(maps, rho, 20, dim, 3)
    assert np.array_equal(t, M.propagate_tau(maps, rho, 20, dim, 3))


# ------------------------------------------------------------------------------------------ 6. PQD_MC_WIDE=1 below dim 7
@pytest.mark.parametrize("dim", [2, 3, 4, 5, 6])
def test_forced_below_dim_7(monkeypatch, dim):
    """the inputs of test_gpu_mapchain_paths.test_onetime_map_by_map_without_pipeline: tiles that are mostly padding"""
    rng = np.random.default_rng(dim)
    N2 = dim * dim
    n_tau, n_tfull = 40, 260
    maps = np.stack([_mk(rng, N2, dim) for _ in range(n_tfull - 1)])
    time = np.round(np.arange(n_tfull) * 0.1, 6)
    ops = _ops(rng, dim)
    rho = H.random_rho(dim).reshape(N2)
    a = (F(maps), rho, n_tau, dim, *ops, time, TS15)
    ref = oracle.calc_onetime_parallel(*a, nthreads=8)
    monkeypatch.delenv("PQD_MC_WIDE", raising=False)
    default = M.calc_onetime_parallel(*a)
    tau_default = M.propagate_tau(F(maps), rho, 25, dim, 3)
    monkeypatch.setenv("PQD_MC_WIDE", "1")
    wide = M.calc_onetime_parallel(*a)
    tau_wide = M.propagate_tau(F(maps), rho, 25, dim, 3)
    ms, nl = _timing()
    assert nl == 25   # the call did run on the step kernel: one launch per map
    e_o, e_d = rel(wide, ref), rel(wide, default)
    e_t = max(rel(tau_wide, oracle.propagate_tau(F(maps), rho, 25, dim, 3)), rel(tau_wide, tau_default))
    print(f"PQD_MC_WIDE=1 dim {dim}: vs oracle {e_o:.3e}, vs the default path {e_d:.3e}, propagate_tau {e_t:.3e}")
    assert wide.shape == ref.shape and e_o < TOL_SWEEP and e_d < TOL_SWEEP
    assert e_t < TOL_TAU


def _timing():
    import ctypes as C
    ms, nl = C.c_double(), C.c_int32()
    _lib.check(_lib.lib().pqd_mc_wide_timing(_lib.context().handle, C.byref(ms), C.byref(nl)))
    return ms.value, nl.value


@pytest.mark.parametrize("dim", [2, 4, 6])
def test_forced_below_dim_7_vs_fortran_golden(monkeypatch, golden_dir, dim):
    monkeypatch.setenv("PQD_MC_WIDE", "1")
    z = np.load(f"{golden_dir}/fortran_propagate_tau_d{dim}.npz")
    e_t = rel(M.propagate_tau(F(z["dm_tl"]), z["rho_init"], int(z["n_tau"]), dim, int(z["j_start"])), z["rho_out"])
    z = np.load(f"{golden_dir}/fortran_onetime_d{dim}.npz")
    r = M.calc_onetime_parallel(F(z["dm_tl"]), z["rho_init"], int(z["n_tau"]), dim, z["opa"], z["opb"], z["opc"],
                                z["time"], z["time_sparse"])
    e = rel(r, z["result"])
    print(f"PQD_MC_WIDE=1 dim {dim} vs the Fortran goldens: onetime {e:.3e}, propagate_tau {e_t:.3e}")
    assert e < TOL_GOLDEN and e_t < TOL_GOLDEN


# ------------------------------------------------------------------------------------------ 7. propagate_tau
@pytest.mark.parametrize("dim", [7, 13, 24])
def test_propagate_tau_vs_oracle(dim):
    n_maps = 30
    maps, rho, _, _ = _inputs(dim, 30 if dim == 24 else 60)
    maps = maps[:, :, :n_maps]
    N2 = dim * dim
    worst = 0.0
    for n_tau, j_start in ((0, 0), (1, 0), (25, 0), (5, n_maps - 5), (0, n_maps)):
        got = M.propagate_tau(maps, rho, n_tau, dim, j_start)
        ref = oracle.propagate_tau(maps, rho, n_tau, dim, j_start)
        assert got.shape == ref.shape == (N2, n_tau + 1)
        assert np.array_equal(got[:, 0], rho)
        worst = max(worst, rel(got, ref))
    print(f"propagate_tau dim {dim}: GPU vs oracle {worst:.3e}")
    assert worst < TOL_TAU
    # the last map is used: the same sweep one map earlier ends elsewhere
    a = M.propagate_tau(maps, rho, 5, dim, n_maps - 5)
    b = M.propagate_tau(maps, rho, 5, dim, n_maps - 6)
    assert np.all(a[:, 5] != b[:, 5])
    for n_tau, j_start in ((6, n_maps - 5), (1, n_maps), (n_maps + 1, 0), (1, -1)):
        with pytest.raises(ValueError, match="outside"):
            M.propagate_tau(maps, rho, n_tau, dim, j_start)


# ------------------------------------------------------------------------------------------ 8. refusals
def _unsupported(fn, *a, **k):
    with pytest.raises(_lib.PQDError) as ei:
        fn(*a, **k)
    assert ei.value.code == _lib.PQD_ERR_UNSUPPORTED, ei.value
    return str(ei.value)


def test_refusals():
    z = lambda *s: np.zeros(s, dtype=complex, order="F")  # noqa: E731
    t, ts = np.array([0.0, 0.1]), np.array([0.0])
    o25 = [z(25, 25)] * 3
    assert "dim 25 not in [2, 24]" in _unsupported(M.calc_onetime_parallel, z(625, 625, 1), z(625), 0, 25, *o25, t, ts)
    assert "dim 25 not in [2, 24]" in _unsupported(M.propagate_tau, z(625, 625, 1), z(625), 1, 25, 0)
    # the entry points this sweep does not serve keep their limit and their words at dim 8
    o8 = [z(8, 8)] * 3
    assert "dim 8 not in [2, 6]" in _unsupported(M.calc_onetime_parallel_block, z(64, 64, 2), z(64, 64), z(64), 2, 1, 8,
                                                  *o8, t, ts)
    assert "dim 8 not in [2, 6]" in _unsupported(M.calc_twotime_phonon_block, z(64, 64, 1, 2), z(64, 64, 2), z(64, 64, 2),
                                                  z(64, 64), z(64), 2, 1, 8, *o8, t, ts)
    assert "N2 64" in _unsupported(M.map_tail, np.zeros((64, 64), complex), np.zeros((64, 1), complex),
                                   np.zeros(64, complex), 3)


# ------------------------------------------------------------------------------------------ 9. end to end
# The same comparison at dim 4 on tls_one_sensor, where every stage is the dim <= 6 code this sweep leaves as it was
# (measured on an MI355X with that code): fortran_only False / True
E2E_DIM4 = {False: 3.579e-15, True: 3.024e-15}


def _e2e(system, lift, dim, fortran_only):
    """max rel() of the time-local-map correlation against the direct propagation with multitime operators"""
    from pyaceqd_amd.pulses import ChirpedPulse
    from pyaceqd_amd.two_time import correlations as corr
    pulse = ChirpedPulse(tau_0=0.4, e_start=0.0, e0=2.0, t0=0.3, alpha=0.5)
    # in brackets: the direct functions build "(A*B)", and `*` binds tighter than `otimes`
    up, down, one = ("(" + s + lift + ")" for s in ("|1><0|_2", "|0><1|_2", "Id_2"))
    t_axis = np.array([0.0, 0.3, 0.6, 1.0])
    rho0 = np.zeros((dim, dim), dtype=complex)
    rho0[0, 0] = 1
    opts = lambda **k: dict(lindblad=True, phonons=False, epsilon=0.05, **k)  # noqa: E731
    kw = dict(tau_max=2.0, dt=0.1)
    _, _, G = corr.tl_two_op_two_time(system, t_axis, pulse, opA=up, opB=down, rho0=rho0, use_dm=True,
                                      fortran_only=fortran_only, options=opts(wide_maps=True), **kw)
    if fortran_only:
        # the Fortran call reads the row-major vec(rho) column-major, that is rho^T: handed (1, A, B) it returns
        # Tr(A^T E(tau)[rho B^T]) = <B^T(t) A^T(t + tau)>, the three-op function of (B^T, A^T, 1)
        _, _, ref = corr.three_op_two_time(system, t_axis, pulse, opA=up, opB=down, opC=one, options=opts(), **kw)
    else:
        _, _, ref = corr.two_op_two_time(system, t_axis, pulse, opA=up, opB=down, options=opts(), **kw)
    assert G.shape == ref.shape == (4, 21) and np.max(np.abs(ref)) > 1e-3
    return rel(G, ref)


@pytest.mark.parametrize("fortran_only", [False, True])
def test_end_to_end_at_dim_8(fortran_only):
    """tl_two_op_two_time(tls_two_sensor, use_dm=True) against the direct propagation with multitime operators
    (two_op_two_time; for fortran_only=True the three-op function its convention amounts to). The bound is 10 times
    the same comparison at dim 4 on tls_one_sensor: 10 x 3.579e-15 (fortran_only=False) and 10 x 3.024e-15 (True).

    Measured at dim 8: 9.765e-15 (False) and 8.622e-15 (True), under the bound (3.579e-14, 3.024e-14).
    The first build of the sweep gave 3.784e-14 and 7.037e-14, above it, and the sweep was not what exceeded it: on the
    same time-local maps the GPU sweep was 1.8e-15 (2.8e-15) from the oracle's sweep, the oracle's sweep on those maps
    was as far from the direct propagation as the GPU's, and numpy's pinv in place of pqd_tl_dynmap_pseudo gave 7.8e-15
    (6.9e-15). The 64 x 64 maps are well conditioned (condition 1.12); the time-local maps of csrc/tlmap_wide.hip were
    1.3e-14 from numpy's, the size of that kernel's Jacobi stop rule n eps = 1.4e-14 at n = 64, and the sweep multiplies
    20 to 30 of them. With that stop rule at sqrt(n) eps (LAPACK zgesvj's) the figures are those of the first line."""
    from pyaceqd_amd.two_level_system.tls import tls_two_sensor
    e = _e2e(tls_two_sensor, " otimes Id_2 otimes Id_2", 8, fortran_only)
    print(f"tl_two_op_two_time(use_dm=True, fortran_only={fortran_only}) at dim 8 vs the direct propagation: {e:.3e}")
    assert e < 10 * E2E_DIM4[fortran_only]
