"""Dressed states for dim 7..24 on the device (csrc/dressed_wide.hip through pqd_dressed_states_wide). GPU only.

The kernel against numpy.linalg.eigh on what is independent of phase and basis, with the bounds of test_gpu_dressed.py
(`check_eigenpairs`: 1e-12 eigenvalues and residuals, 1e-13 unitarity, 1e-11 single projectors, 1e-9 clusters; a numpy
restatement of the kernel's round-robin Jacobi stays at or below 5.8e-15 on all of them at N = 24). Occupations against
the reference's formula in numpy at atol 1e-12: with |v| <= 1 and |rho| entries of order a few, N^2 eps max|rho| is
6e-13 at N = 24. Then matrices chosen to be hard for Jacobi, batch independence, the error path, a closed form, and the
drop-in callers.

The kernel takes ONE problem per workgroup (one wave each), so every problem count is a multiple of it; the counts
below are 1, 2, 3 and 7 per system (n_steps 0, 1, 2, 6) and, once per N, 1101. A launch has at most 65,536
workgroups, each looping over problems that far apart; one test runs 70,001 problems through that loop.
"""
import numpy as np
import pytest

from pyaceqd_amd import _lib, engine, tools
from pyaceqd_amd.engine import Grid, System
from pyaceqd_amd.general_system.general_dressed_states import dressed_states
from pyaceqd_amd.pulses import ChirpedPulse
from pyaceqd_amd.two_level_system.tls import tls_photon, tls_photon_two_sensor, tls_photons, \
    tls_photons_dressed_states
from pyaceqd_amd.four_level_system.linear import biexciton_photons, biexciton_photons_dressed_states, \
    biexciton_photons_extended, biexciton_photons_extended_dressed_states
from tests.test_gpu_dressed import check_eigenpairs, hamiltonians, literal_occupations, random_systems

pytestmark = pytest.mark.gpu

PROBLEMS_PER_WORKGROUP = 1


def _unitary(rng, n):
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n)))
    return Q


# ----------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("N", [7, 8, 13, 16, 18, 23, 24])
def test_kernel_against_eigh(N):
    rng = np.random.default_rng(1000 + N)
    cases = [(n_sys, n_steps, n_chan) for n_sys in (1, 3) for n_steps in (0, 1, 2, 6) for n_chan in (0, 1, 4)]
    cases.append((1, 1100, 2))   # above 1,000 problems: the grid-stride loop's first pass only, but every block index
    for n_sys, n_steps, n_chan in cases:
        grid = Grid(-1.5, 0.07, n_steps)
        systems = random_systems(N, n_sys, n_chan, grid, rng)
        H = np.stack([hamiltonians(s, grid) for s in systems])
        rho = rng.normal(size=H.shape) + 1j * rng.normal(size=H.shape)
        ev, vec, occ = engine.dressed_states(systems, grid, rho=rho)
        assert ev.shape == (n_sys, n_steps + 1, N)
        check_eigenpairs(H.reshape(-1, N, N), ev.reshape(-1, N), vec.reshape(-1, N, N),
                         f"N={N} n_sys={n_sys} n_steps={n_steps} n_chan={n_chan}")
        np.testing.assert_allclose(occ, literal_occupations(vec, rho), rtol=0, atol=1e-12)
        ev2, vec2, occ2 = engine.dressed_states(systems, grid, rho=rho, want_vectors=False)
        assert vec2 is None
        np.testing.assert_array_equal(ev2, ev)
        np.testing.assert_array_equal(occ2, occ)
    # a single System (not a list) drops the system axis; without rho there are no occupations
    ev1, vec1, occ1 = engine.dressed_states(systems[0], grid)
    assert occ1 is None
    np.testing.assert_array_equal(ev1, ev[0])
    np.testing.assert_array_equal(vec1, vec[0])


@pytest.mark.parametrize("N", [9, 24])
def test_clamped_sample_range(N):
    """the samples cover the middle of the grid only: before and after, the end samples are held"""
    rng = np.random.default_rng(1200 + N)
    grid = Grid(2.0, 0.1, 100)
    systems = random_systems(N, 2, 2, grid, rng, short_samples=True)
    H = np.stack([hamiltonians(s, grid) for s in systems])
    assert np.array_equal(H[0, 0], H[0, 20]) and np.array_equal(H[0, -1], H[0, -20])   # held ends
    assert not np.array_equal(H[0, 40], H[0, 50])
    ev, vec, _ = engine.dressed_states(systems, grid)
    check_eigenpairs(H.reshape(-1, N, N), ev.reshape(-1, N), vec.reshape(-1, N, N), f"clamped N={N}")


def test_more_problems_than_workgroups():
    """the launch stops at 65,536 workgroups and each loops over problems 65,536 apart: with 70,001 problems the first
    4,465 workgroups take a second one (checked vectorised: eigenvalues, residuals, unitarity, occupations)"""
    N, n_steps = 7, 70000
    rng = np.random.default_rng(1250)
    grid = Grid(0.0, 0.001, n_steps)
    (s,) = random_systems(N, 1, 1, grid, rng)
    H = hamiltonians(s, grid)
    rho = rng.normal(size=H.shape) + 1j * rng.normal(size=H.shape)
    ev, vec, occ = engine.dressed_states(s, grid, rho=rho)
    scale = np.maximum(1.0, np.linalg.norm(H, axis=(1, 2)))
    assert np.max(np.abs(ev - np.linalg.eigvalsh(H)) / scale[:, None]) <= 1e-12
    V = vec.transpose(0, 2, 1)
    assert np.max(np.linalg.norm(H @ V - V * ev[:, None, :], axis=1) / scale[:, None]) <= 1e-12
    assert np.max(np.linalg.norm(V.conj().transpose(0, 2, 1) @ V - np.eye(N), 2, axis=(1, 2))) <= 1e-13
    np.testing.assert_allclose(occ, literal_occupations(vec, rho), rtol=0, atol=1e-12)
    assert not np.array_equal(ev[0], ev[65536]) and not np.array_equal(ev[4464], ev[70000])


def hard_matrices_wide(N, rng):
    U = _unitary(rng, N)
    lam = np.array([1.0, 1.0] + list(range(2, N)), dtype=float)
    split = lam.copy()
    split[1] += 1e-9
    two = np.array([2.0] * (N // 2) + [-1.0] * (N - N // 2))
    three = np.array([0.0] * (N // 3) + [1.0] * (N // 3) + [3.0] * (N - 2 * (N // 3)))
    A = rng.normal(size=(N, N))
    span = np.diag(1e3 * np.array([(-1.0) ** k / (1 + k // 2) for k in range(N)])).astype(complex)
    iu = np.triu_indices(N, 1)
    mags = np.logspace(-8, 0, len(iu[0]))
    span[iu] = mags * np.exp(1j * rng.uniform(0, 2 * np.pi, len(mags)))
    span = np.triu(span) + np.triu(span, 1).conj().T
    jc = np.diag(-2.0 * np.arange(N)).astype(complex)
    for k in range(N - 1):
        jc[k, k + 1] = jc[k + 1, k] = 0.06 * np.sqrt(k + 1)
    U2, U3 = _unitary(rng, N), _unitary(rng, N)
    return {
        "zero": np.zeros((N, N), dtype=complex),
        "diagonal descending": np.diag(np.arange(N, 0, -1.0)).astype(complex),
        "repeated eigenvalues": U @ np.diag(lam) @ U.conj().T,
        "pair split by 1e-9": U @ np.diag(split) @ U.conj().T,
        "two-level spectrum": U2 @ np.diag(two) @ U2.conj().T,
        "three-level spectrum": U3 @ np.diag(three) @ U3.conj().T,
        "imaginary off-diagonals": np.diag(rng.normal(size=N) * 5).astype(complex) + 1j * (A - A.T),
        "entries 1e-8..1e3": span,
        "Jaynes-Cummings tridiagonal": jc,
    }


@pytest.mark.parametrize("N", [7, 18, 24])
def test_hard_matrices(N):
    """each alone and all as one batch; a problem that misses the 40-sweep cap raises (PQD_ERR_NUMERIC), so the
    degenerate spectra converging is part of every call below"""
    rng = np.random.default_rng(1300 + N)
    mats = hard_matrices_wide(N, rng)
    grid = Grid(0.0, 1.0, 0)
    for name, Hm in mats.items():
        ev, vec, _ = engine.dressed_states([System(dim=N, H0=Hm)], grid)
        check_eigenpairs(Hm[None], ev[0], vec[0], f"N={N} {name}")
    ev, vec, _ = engine.dressed_states([System(dim=N, H0=Hm) for Hm in mats.values()], grid)
    check_eigenpairs(np.stack(list(mats.values())), ev[:, 0], vec[:, 0], f"N={N} batch of hard matrices")
    ev, vec, _ = engine.dressed_states(System(dim=N, H0=mats["zero"]), grid)
    np.testing.assert_array_equal(ev[0], np.zeros(N))
    np.testing.assert_array_equal(vec[0], np.eye(N))
    ev, vec, _ = engine.dressed_states(System(dim=N, H0=mats["diagonal descending"]), grid)
    np.testing.assert_array_equal(ev[0], np.arange(1.0, N + 1))
    np.testing.assert_array_equal(vec[0], np.eye(N)[::-1])


def test_outputs_do_not_depend_on_the_batch():
    """one system's outputs alone and as member 0, 37 and 69 of a batch of 70 mixed systems are the same bits"""
    N = 18
    rng = np.random.default_rng(1400)
    grid = Grid(0.0, 0.1, 5)
    others = []
    for k in range(70):
        others += random_systems(N, 1, k % 5, grid, rng)
    others[3] = System(dim=N, H0=np.zeros((N, N), dtype=complex))
    others[40] = System(dim=N, H0=hard_matrices_wide(N, rng)["two-level spectrum"])   # a slow neighbour
    (mine,) = random_systems(N, 1, 2, grid, rng)
    rho1 = rng.normal(size=(1, 6, N, N)) + 1j * rng.normal(size=(1, 6, N, N))
    ev0, vec0, occ0 = engine.dressed_states([mine], grid, rho=rho1)
    for pos in (0, 37, 69):
        batch = list(others)
        batch[pos] = mine
        rho = rng.normal(size=(70, 6, N, N)) + 1j * rng.normal(size=(70, 6, N, N))
        rho[pos] = rho1[0]
        ev, vec, occ = engine.dressed_states(batch, grid, rho=rho)
        np.testing.assert_array_equal(ev[pos], ev0[0])
        np.testing.assert_array_equal(vec[pos], vec0[0])
        np.testing.assert_array_equal(occ[pos], occ0[0])


def test_error_paths():
    rng = np.random.default_rng(1500)
    grid = Grid(0.0, 0.1, 40)
    (s,) = random_systems(12, 1, 1, grid, rng)
    X, f = s.channels[0]
    f = np.array(f)
    f[len(f) // 2] = np.nan
    s.channels = [(X, f)]
    with pytest.raises(_lib.PQDError) as e:
        engine.dressed_states(s, grid)
    assert isinstance(e.value, _lib.NumericError) and e.value.code == 5        # PQD_ERR_NUMERIC
    # the context stays usable
    d = np.arange(12.0, 0.0, -1.0)
    ev, _, _ = engine.dressed_states(System(dim=12, H0=np.diag(d).astype(complex)), grid)
    np.testing.assert_array_equal(ev[5], d[::-1])
    with pytest.raises(_lib.PQDError, match=r"dim 25 not in \[7, 24\]") as e:
        engine.dressed_states(System(dim=25, H0=np.eye(25, dtype=complex)), grid)
    assert e.value.code == _lib.PQD_ERR_UNSUPPORTED


# ----------------------------------------------------------------------------------------------- the callers
def test_jaynes_cummings_closed_form():
    """tls_photon with three photons, no pulse: H0 = delta n + g (sigma+ b + sigma- b^dagger) splits into |0,0> (0),
    the top state |1,3> (3 delta) and the manifolds k = 1..3 with (2k - 1) delta / 2 +- sqrt(delta^2 + 4 g^2 k) / 2"""
    delta, g = -2.0, 0.06
    res = dressed_states(tls_photon, [2, 4], 0, 1, dt=0.1, n_phot1=3)
    t, pop, e_values = res[0], res[1], res[2]
    assert e_values.shape == (11, 8) and pop.shape == (11, 8)
    want = [0.0, 3 * delta]
    for k in (1, 2, 3):
        root = np.sqrt(delta ** 2 + 4 * g ** 2 * k)
        want += [0.5 * ((2 * k - 1) * delta - root), 0.5 * ((2 * k - 1) * delta + root)]
    np.testing.assert_allclose(e_values, np.sort(want)[None].repeat(11, axis=0), rtol=0, atol=1e-12)
    np.testing.assert_allclose(res[3].sum(axis=1), 1.0, rtol=0, atol=1e-10)


def _check_wrapper(res, low, n, dt_rho):
    t, pop, e_values, ds_occ, s_colors, n_colors, e_vectors, rho = res
    n_t = len(t)
    assert pop.shape == (n_t, n) and e_values.shape == (n_t, n) and ds_occ.shape == (n_t, n)
    assert e_vectors.shape == (n_t, n, n) and rho.shape == (n_t, n, n)
    assert len(s_colors) == n and all(len(c) == n_t for c in s_colors) and n_colors.shape == (n, n_t)
    (s,) = low.systems
    assert s.dim == n and low.n_t == [n_t]
    H = hamiltonians(s, low.grid)
    w = np.linalg.eigvalsh(H)
    np.testing.assert_allclose(e_values, w, rtol=0, atol=1e-12)
    # residuals and unitarity only: two equal cavity modes give level pairs a weak pulse splits by far less than
    # 1e-6 ||H||, where a single projector is conditioned like eps ||H|| / gap (numpy's own eigh moves as much)
    V = e_vectors.transpose(0, 2, 1)                                  # columns = eigenvectors
    scale = np.maximum(1.0, np.linalg.norm(H, axis=(1, 2)))
    resid = np.linalg.norm(H @ V - V * e_values[:, None, :], axis=1).max(axis=1) / scale
    unit = np.linalg.norm(V.conj().transpose(0, 2, 1) @ V - np.eye(n), 2, axis=(1, 2))
    print(f"wrapper dim {n}: resid={resid.max():.2e} unit={unit.max():.2e}")
    assert resid.max() <= 1e-12 and unit.max() <= 1e-13
    np.testing.assert_allclose(ds_occ, literal_occupations(e_vectors, rho), rtol=0, atol=1e-12)
    np.testing.assert_allclose(ds_occ.sum(axis=1), 1.0, rtol=0, atol=1e-10)
    t_ref, rho_ref = tools.compose_dm(dt_rho, dim=n)
    np.testing.assert_array_equal(t, t_ref)
    np.testing.assert_allclose(pop, np.diagonal(rho_ref, axis1=1, axis2=2), rtol=0, atol=1e-12)
    return e_values


def test_tls_photons_wrapper_under_a_gaussian_pulse():
    p = ChirpedPulse(tau_0=0.8, e_start=0.0, e0=4.0, t0=2.0)
    res = tls_photons_dressed_states(0, 4, p, dt=0.1, return_eigenvectors=True)
    assert len(res) == 8
    low = tls_photons(0, 4, p, dt=0.1, lower_only=True)
    out = tls_photons(0, 4, p, dt=0.1, output_ops=tools.output_ops_dm([2, 3, 3]))
    e_values = _check_wrapper(res, low, 18, out)
    assert np.ptp(e_values[:, 0]) > 0.05                               # the pulse dresses the levels
    assert len(tls_photons_dressed_states(0, 1, p, dt=0.1)) == 6


@pytest.mark.parametrize("model", ["biexciton_photons", "biexciton_photons_extended"])
def test_biexciton_cavity_wrappers(model):
    p = ChirpedPulse(tau_0=0.8, e_start=-2.0, e0=5.0, t0=2.0, polar_x=0.8)
    if model == "biexciton_photons":
        res = biexciton_photons_dressed_states(0, 4, p, dt=0.1, n_phot1=1, n_phot2=1, return_eigenvectors=True)
        low = biexciton_photons(0, 4, p, dt=0.1, n_phot1=1, n_phot2=1, lower_only=True)
        out = biexciton_photons(0, 4, p, dt=0.1, n_phot1=1, n_phot2=1, output_ops=tools.output_ops_dm([4, 2, 2]))
        n = 16
    else:
        res = biexciton_photons_extended_dressed_states(0, 4, p, dt=0.1, return_eigenvectors=True)
        low = biexciton_photons_extended(0, 4, p, dt=0.1, lower_only=True)
        out = biexciton_photons_extended(0, 4, p, dt=0.1, output_ops=tools.output_ops_dm(18))
        n = 18
    _check_wrapper(res, low, n, out)


def test_trajectories_form_is_one_launch():
    pulses = [ChirpedPulse(tau_0=0.8, e_start=0.5, e0=a, t0=2.0) for a in (1.0, 3.0, 5.0)]
    singles = [tls_photons_dressed_states(0, 4, p, dt=0.1, return_eigenvectors=True) for p in pulses]
    before = engine.DRESSED_LAUNCHES
    batch = tls_photons_dressed_states(0, 4, dt=0.1, return_eigenvectors=True,
                                       trajectories=[{"pulses": (p,)} for p in pulses])
    assert engine.DRESSED_LAUNCHES - before == 1
    assert len(batch) == 3
    for one, many in zip(singles, batch):
        assert len(many) == 8
        np.testing.assert_array_equal(many[0], one[0])
        np.testing.assert_allclose(many[2], one[2], rtol=0, atol=1e-13)   # eigenvalues
        np.testing.assert_allclose(many[3], one[3], rtol=0, atol=1e-13)   # occupations
        np.testing.assert_allclose(many[1], one[1], rtol=0, atol=1e-12)   # populations of the batched propagation
        assert many[4] == one[4]
    # a shorter trajectory keeps its own length
    short = tls_photons_dressed_states(0, 4, dt=0.1, trajectories=[{"pulses": (pulses[0],)},
                                                                    {"pulses": (pulses[1],), "t_end": 2.0}])
    assert short[0][2].shape == (41, 18) and short[1][2].shape == (21, 18)
    np.testing.assert_allclose(short[1][2], singles[1][2][:21], rtol=0, atol=1e-13)


def test_dim_24_takes_two_propagation_calls(monkeypatch):
    calls = []
    real = tls_photon_two_sensor

    def spy(*a, **k):
        calls.append(len(k["output_ops"]))
        return real(*a, **k)
    p = ChirpedPulse(tau_0=0.3, e_start=0.0, e0=2.0, t0=0.5)
    res = dressed_states(spy, [2, 3, 2, 2], 0, 1, p, dt=0.1, return_eigenvectors=True)
    assert calls == [150, 150, 300]            # two propagation slices, then the lowering (which runs nothing)
    t, pop, e_values, ds_occ, s_colors, n_colors, e_vectors, rho = res
    assert rho.shape == (11, 24, 24) and e_values.shape == (11, 24)
    np.testing.assert_allclose(rho, rho.conj().transpose(0, 2, 1), rtol=0, atol=1e-10)
    np.testing.assert_allclose(np.trace(rho, axis1=1, axis2=2), 1.0, rtol=0, atol=1e-10)
    np.testing.assert_allclose(ds_occ.sum(axis=1), 1.0, rtol=0, atol=1e-10)
    np.testing.assert_allclose(ds_occ, literal_occupations(e_vectors, rho), rtol=0, atol=1e-12)
    assert abs(rho[0, 0, 0] - 1.0) < 1e-12 and np.max(np.abs(rho[-1] - rho[0])) > 1e-3     # the pulse moved the state
