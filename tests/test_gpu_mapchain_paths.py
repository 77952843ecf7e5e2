"""The map-by-map kernels of mapchain.hip on the paths the other files leave out, against the C oracle. GPU only.

* mc_tau_kernel, the tau sweep without the register pipeline (PQD_MC_PIPE=0), in all three modes at dims 2-6. For modes 0
  and 1 it is reached with PQD_MC_BLOCKED=0. Both kernels form the states with the same products in the same order, but
  the outputs agree only to rounding, not bit for bit: mc_tau_kernel sums the trace with fused multiply-adds, the
  pipelined kernel rounds each product w_q y_q before adding.
* mode 2 (calc_twotime_phonon_block) at the dims with padding lanes (3 and 5) and at dim 2 over three waves, with
  n_tauc = 0, 1, a middle value and n_t, n_map below and above n_tb, and trunk ends at 1, inside n_tb, at n_tb and at
  n_tb + 1 (from n_tb on the wrap test `jj + j_start == n_tb + 1` never fires) and further out.
* tau windows shorter than the pipelined kernels' prefetch depth (dims 2 and 3, all three modes): only the guarded
  remainder loop runs and the lookahead map cursor is past the last step from its first load on.
* propagate_tau with n_tau = 0 and j_start = 0, and at the end of the map stack.
* the refusal of a mode-0 sweep that would read past dm_tl, with PQD_MC_BLOCKED=0.

Bounds as in test_gpu_parity.py: 1e-11 for the sweeps, 1e-12 for propagate_tau. Worst GPU-against-oracle values observed
on an MI355X: calc_onetime_parallel 3.4e-15, calc_onetime_parallel_block 3.7e-15, calc_twotime_phonon_block 2.6e-15,
propagate_tau 2.2e-15; mc_tau_kernel against the pipelined kernel 8.5e-16 at most, never bit-equal (the trace sums)."""
import numpy as np
import pytest

from oracle import oracle
from pyaceqd_amd.two_time import propagate_tau_module as M
from tests import helpers as H

pytestmark = pytest.mark.gpu
F = lambda maps: np.asfortranarray(np.asarray(maps).transpose(1, 2, 0))  # noqa: E731
DIMS = [2, 3, 4, 5, 6]


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def _mk(rng, N2, dim):
    return np.eye(N2) + 0.05 * (rng.normal(size=(N2, N2)) + 1j * rng.normal(size=(N2, N2))) / dim


def _ops(rng, dim):
    return [rng.normal(size=(dim, dim)) + 1j * rng.normal(size=(dim, dim)) for _ in range(3)]


def _both_tau_kernels(monkeypatch, call, ref, name, tol=1e-11):
    """`call()` with the pipelined tau kernel and with mc_tau_kernel, each against `ref`, and against each other"""
    monkeypatch.delenv("PQD_MC_PIPE", raising=False)
    piped = call()
    monkeypatch.setenv("PQD_MC_PIPE", "0")
    plain = call()
    e_plain, e_piped, e_both = rel(plain, ref), rel(piped, ref), rel(plain, piped)
    print(f"{name}: mc_tau_kernel vs oracle {e_plain:.3e}, pipelined vs oracle {e_piped:.3e}, "
          f"one vs the other {e_both:.3e} (bit-equal: {np.array_equal(plain, piped)})")
    assert plain.shape == ref.shape
    assert e_plain < tol and e_piped < tol and e_both < tol
    # column 1 comes from the trunk kernel, which both calls share
    assert np.array_equal(plain[:, 0], piped[:, 0])
    return plain


@pytest.mark.parametrize("dim", DIMS)
def test_onetime_map_by_map_without_pipeline(monkeypatch, dim):
    """calc_onetime_parallel on the inputs of test_mapchain_blocked_sweep_vs_oracle with n_tau = 40"""
    monkeypatch.setenv("PQD_MC_BLOCKED", "0")
    rng = np.random.default_rng(dim)
    N2 = dim * dim
    n_tau, n_tfull = 40, 260
    maps = np.stack([_mk(rng, N2, dim) for _ in range(n_tfull - 1)])
    time = np.round(np.arange(n_tfull) * 0.1, 6)
    ts = np.array([0.0, 0.05, 0.7, 0.75, 0.8, 0.8, 1.2, 1.3, 1.31, 2.55, 4.0, 6.4, 7.9, 10.0, 10.85])
    ops = _ops(rng, dim)
    rho = H.random_rho(dim).reshape(N2)
    a = (F(maps), rho, n_tau, dim, *ops, time, ts)
    ref = oracle.calc_onetime_parallel(*a, nthreads=8)
    _both_tau_kernels(monkeypatch, lambda: M.calc_onetime_parallel(*a), ref, f"onetime dim {dim}")


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("n_map", [7, 18])
def test_onetime_block_map_by_map_without_pipeline(monkeypatch, dim, n_map):
    """calc_onetime_parallel_block on the inputs of test_mapchain_blocked_sweep_block_mode_vs_oracle"""
    monkeypatch.setenv("PQD_MC_BLOCKED", "0")
    rng = np.random.default_rng(10 + dim)
    N2 = dim * dim
    n_tb, nx_tau = 12, 9
    dm_block = np.stack([_mk(rng, N2, dim) for _ in range(n_map)])
    dm_s = _mk(rng, N2, dim)
    time = np.round(np.arange(60) * 0.1, 6)
    ts = np.array([0.0, 0.15, 0.4, 0.75, 1.1, 1.2, 1.25, 2.0, 3.3])
    ops = _ops(rng, dim)
    rho = H.random_rho(dim).reshape(N2)
    a = (F(dm_block), np.asfortranarray(dm_s), rho, n_tb, nx_tau, dim, *ops, time, ts)
    ref = oracle.calc_onetime_parallel_block(*a)
    _both_tau_kernels(monkeypatch, lambda: M.calc_onetime_parallel_block(*a), ref, f"onetime_block dim {dim} n_map {n_map}")


def _phonon_inputs(dim, n_map, n_tauc, n_t):
    rng = np.random.default_rng(300 + dim)
    N2 = dim * dim
    n_tb, nx_tau = 5, 3
    sep1 = F([_mk(rng, N2, dim) for _ in range(n_map)])
    sep2 = F([_mk(rng, N2, dim) for _ in range(n_map)])
    dm_s = np.asfortranarray(_mk(rng, N2, dim))
    # dm_taucs2(:, :, i, jj): one map stack per trajectory i <= n_tauc (propagate_tau.f90:466-476)
    tc = np.zeros((N2, N2, n_tauc, n_map), dtype=complex, order="F")
    for i in range(n_tauc):
        for jj in range(n_map):
            tc[:, :, i, jj] = _mk(rng, N2, dim)
    time = np.round(np.arange(30) * 0.1, 6)
    # trunk ends j = 1 + #{time < ts}: 1, 3 (inside n_tb), 5 = n_tb, 6 = n_tb + 1, 10; the rest anywhere up to 13
    fixed = [0.0, 0.15, 0.4, 0.5, 0.85]
    ts = np.sort(np.concatenate([fixed, np.round(rng.uniform(0.0, 1.2, n_t - len(fixed)), 2)]))
    j = 1 + np.array([np.sum(time < t) for t in ts])
    assert {1, 3, n_tb, n_tb + 1, 10} <= set(j.tolist())
    ops = _ops(rng, dim)
    rho = H.random_rho(dim, seed=300 + dim).reshape(N2)
    return (tc, sep1, sep2, dm_s, rho, n_tb, nx_tau, dim, *ops, time, ts)


@pytest.mark.parametrize("dim", [2, 3, 5])
@pytest.mark.parametrize("n_map", [3, 7])
@pytest.mark.parametrize("tauc", ["0", "1", "mid", "n_t"])
def test_twotime_phonon_block_vs_oracle(monkeypatch, dim, n_map, tauc):
    n_t = 2 * (64 // (dim * dim)) + 1
    n_tauc = {"0": 0, "1": 1, "mid": n_t // 2, "n_t": n_t}[tauc]
    a = _phonon_inputs(dim, n_map, n_tauc, n_t)
    ref = oracle.calc_twotime_phonon_block(*a)
    got = _both_tau_kernels(monkeypatch, lambda: M.calc_twotime_phonon_block(*a), ref,
                            f"twotime_phonon_block dim {dim} n_map {n_map} n_tauc {n_tauc}")
    assert got.shape == (n_t, 16)
    # dm_taucs2 reaches the rows i < n_tauc (every tau column: the first step reads it at jj = 1) and no other row
    b = (a[0] * 1.01,) + a[1:]
    other = M.calc_twotime_phonon_block(*b)
    assert np.array_equal(other[n_tauc:], got[n_tauc:]) and np.array_equal(other[:, 0], got[:, 0])
    assert np.all(other[:n_tauc, 1:] != got[:n_tauc, 1:])


@pytest.mark.parametrize("dim", [4, 6])
def test_twotime_phonon_block_without_pipeline_other_dims(monkeypatch, dim):
    """mc_tau_kernel in mode 2 at the remaining dims"""
    n_t = 2 * (64 // (dim * dim)) + 1 if dim == 4 else 5
    a = _phonon_inputs(dim, 7, n_t // 2, n_t)
    ref = oracle.calc_twotime_phonon_block(*a)
    _both_tau_kernels(monkeypatch, lambda: M.calc_twotime_phonon_block(*a), ref, f"twotime_phonon_block dim {dim}")


def test_twotime_phonon_block_accepts_no_taucs_array():
    """n_tauc = 0: nothing is read from dm_taucs2, whatever its other extents"""
    a = list(_phonon_inputs(3, 7, 0, 15))
    ref = M.calc_twotime_phonon_block(*a)
    a[0] = np.zeros((9, 9, 0, 0), dtype=complex, order="F")
    assert np.array_equal(M.calc_twotime_phonon_block(*a, n_map=7), ref)


def _short_window_cases(mode):
    if mode == 0:
        return [(n_tau,) for n_tau in (0, 1, 2, 3, 5)]
    return [(n_tb, nx_tau, n_map) for n_tb, nx_tau in ((2, 0), (1, 1), (1, 2), (3, 1), (1, 3), (5, 1)) for n_map in (1, 3, 7)]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dim", [2, 3])
def test_windows_shorter_than_the_prefetch_depth(monkeypatch, dim, mode):
    """tau windows of 0 to 5 steps at dims 2 and 3, where the pipelined kernels prefetch 4 and 2 maps ahead: the
    unrolled loop runs once at most, the guarded remainder does the work, and the lookahead map cursor runs past the
    last step from its first load on (it must hand out a valid map there). dim 3 has padding lanes; n_t leaves one
    trajectory in the third wave. Every shape on the default path, with PQD_MC_BLOCKED=0 (modes 0 and 1: mode 2 has no
    blocked sweep, its default path is that one already and is not run twice) and with PQD_MC_PIPE=0 in addition, each
    against the oracle."""
    N2 = dim * dim
    n_t = 2 * (64 // N2) + 1
    rng = np.random.default_rng(700 + 10 * dim + mode)
    time = 0.1 * np.arange(30)
    ts = np.sort(np.concatenate([[0.0], rng.uniform(0.0, 1.2, n_t - 1)]))
    ops = _ops(rng, dim)
    rho = H.random_rho(dim, seed=700 + dim).reshape(N2)
    maps = [_mk(rng, N2, dim) for _ in range(29)]  # dm_tl; its head serves as dm_block / dm_sep1
    sep2 = [_mk(rng, N2, dim) for _ in range(7)]
    dm_s = np.asfortranarray(_mk(rng, N2, dim))
    n_tauc = n_t // 2
    tc = np.zeros((N2, N2, n_tauc, 7), dtype=complex, order="F")
    for i in range(n_tauc):
        for jj in range(7):
            tc[:, :, i, jj] = _mk(rng, N2, dim)
    paths = [{}, {"PQD_MC_BLOCKED": "0"}, {"PQD_MC_BLOCKED": "0", "PQD_MC_PIPE": "0"}]
    worst = 0.0
    for case in _short_window_cases(mode):
        if mode == 0:
            a, n_tau = (F(maps), rho, case[0], dim, *ops, time, ts), case[0]
            name = "calc_onetime_parallel"
        else:
            n_tb, nx_tau, n_map = case
            n_tau = n_tb * nx_tau
            if mode == 1:
                a = (F(maps[:n_map]), dm_s, rho, n_tb, nx_tau, dim, *ops, time, ts)
                name = "calc_onetime_parallel_block"
            else:
                a = (np.asfortranarray(tc[:, :, :, :n_map]), F(maps[:n_map]), F(sep2[:n_map]), dm_s, rho, n_tb, nx_tau,
                     dim, *ops, time, ts)
                name = "calc_twotime_phonon_block"
        ref = getattr(oracle, name)(*a)
        assert ref.shape == (n_t, n_tau + 1) and np.all(np.isfinite(ref))
        for env in (paths[::2] if mode == 2 else paths):
            for k in ("PQD_MC_BLOCKED", "PQD_MC_PIPE"):
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            got = getattr(M, name)(*a)
            assert got.shape == ref.shape
            e = rel(got, ref)
            worst = max(worst, e)
            assert e < 1e-11, (case, env, e)
    print(f"short windows dim {dim} mode {mode}: worst GPU vs oracle {worst:.3e}")


@pytest.mark.parametrize("dim", DIMS)
def test_propagate_tau_vs_oracle(dim):
    rng = np.random.default_rng(500 + dim)
    N2 = dim * dim
    n_maps = 30
    maps = F([_mk(rng, N2, dim) for _ in range(n_maps)])
    rho = H.random_rho(dim, seed=500 + dim).reshape(N2)
    worst = 0.0
    for n_tau, j_start in ((0, 0), (1, 0), (25, 0), (5, n_maps - 5), (0, n_maps)):
        got = M.propagate_tau(maps, rho, n_tau, dim, j_start)
        ref = oracle.propagate_tau(maps, rho, n_tau, dim, j_start)
        assert got.shape == ref.shape == (N2, n_tau + 1)
        assert np.array_equal(got[:, 0], rho)
        worst = max(worst, rel(got, ref))
    print(f"propagate_tau dim {dim}: GPU vs oracle {worst:.3e}")
    assert worst < 1e-12
    # the last map is used: the same sweep one map earlier ends elsewhere
    a = M.propagate_tau(maps, rho, 5, dim, n_maps - 5)
    b = M.propagate_tau(maps, rho, 5, dim, n_maps - 6)
    assert np.all(a[:, 5] != b[:, 5])
    for n_tau, j_start in ((6, n_maps - 5), (1, n_maps), (n_maps + 1, 0), (1, -1)):
        with pytest.raises(ValueError, match="outside"):
            M.propagate_tau(maps, rho, n_tau, dim, j_start)


@pytest.mark.parametrize("pipe", ["1", "0"])
def test_map_by_map_refuses_reads_past_the_maps(monkeypatch, pipe):
    """test_mapchain_blocked_refuses_reads_past_the_maps with the blocked sweep switched off: the same refusal, and the
    longest window that still fits is answered"""
    monkeypatch.setenv("PQD_MC_BLOCKED", "0")
    monkeypatch.setenv("PQD_MC_PIPE", pipe)
    dim, N2, n_tfull = 2, 4, 30
    rng = np.random.default_rng(9)
    maps = np.stack([_mk(rng, N2, dim) for _ in range(n_tfull - 1)])
    time = np.round(np.arange(n_tfull) * 0.1, 6)
    ops = _ops(rng, dim)
    rho = H.random_rho(dim).reshape(N2)
    ts = np.array([0.0, 0.5])  # trunk ends j = 1, 6: the second sweep reads maps 6 .. 5 + n_tau of 29
    with pytest.raises(ValueError, match="would read map"):
        M.calc_onetime_parallel(F(maps), rho, 25, dim, *ops, time, ts)
    a = M.calc_onetime_parallel(F(maps), rho, 24, dim, *ops, time, ts)
    assert rel(a, oracle.calc_onetime_parallel(F(maps), rho, 24, dim, *ops, time, ts)) < 1e-11
    with pytest.raises(ValueError, match="would read map"):
        M.calc_onetime_parallel(F(maps), rho, 0, dim, *ops, time, np.array([0.0, 3.5]))
