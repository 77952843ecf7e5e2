"""Dressed states on the device (csrc/dressed.hip through pqd_dressed_states). GPU only.

The kernel against numpy.linalg.eigh for N = 2..6 on what is independent of phase and basis (eigenvalues, residuals,
unitarity, projectors onto clusters of close eigenvalues), its phase convention, the occupations against the
reference's formula evaluated in numpy, and the drop-in callers: `system_ace_stream(dressedstates=True)` on the three
models, the `*_dressed_states` wrappers, and the batched `trajectories=` form.

Tolerances (issue / DESIGN.md §5): 1e-12 max(1, ||H||_F) for eigenvalues and residuals is the project's
free-propagator tolerance against the oracle; a converged fp64 Jacobi at N <= 6 sits two orders below it.
"""
import numpy as np
import pytest

from pyaceqd_amd import _lib, engine, opgrammar, tools
from pyaceqd_amd.constants import hbar
from pyaceqd_amd.engine import Grid, System
from pyaceqd_amd.general_system import general_system as gs
from pyaceqd_amd.pulses import ChirpedPulse, CWLaser
from pyaceqd_amd.two_level_system.tls import tls, tls_dressed_states
from pyaceqd_amd.four_level_system.linear import biexciton, biexciton_dressed_states, biexciton_ops
from pyaceqd_amd.six_level_system.linear import sixls_linear, sixls_linear_dressed_states, sixls_ops

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------------------------- numpy side
def _herm(rng, n, scale):
    M = rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))
    return scale * (M + M.conj().T) / 2


def _unitary(rng, n):
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n)))
    return Q


def hamiltonians(system, grid):
    """H(t_n) of a System on the grid, with the device's sampling rule: linear interpolation, clamped at both ends"""
    t = grid.times
    H = np.repeat(np.asarray(system.H0, dtype=complex)[None], len(t), axis=0)
    for X, f in system.channels:
        f = np.asarray(f, dtype=complex)
        ts = system.sample_t0 + system.sample_dt * np.arange(len(f))
        ft = np.interp(t, ts, f.real) + 1j * np.interp(t, ts, f.imag)
        H = H + ft[:, None, None] * X[None] + ft.conj()[:, None, None] * X.conj().T[None]
    return H


def _clusters(w, tol):
    groups, cur = [], [0]
    for k in range(1, len(w)):
        if w[k] - w[k - 1] <= tol:
            cur.append(k)
        else:
            groups.append(cur)
            cur = [k]
    return groups + [cur]


def check_eigenpairs(H, evals, evecs, what=""):
    """H (P, N, N) against evals (P, N) and evecs (P, N, N) with evecs[p, j] = eigenvector j"""
    P, N, _ = H.shape
    assert evals.shape == (P, N) and evecs.shape == (P, N, N)
    worst = dict(eval=0.0, resid=0.0, unit=0.0, single=0.0, cluster=0.0)
    for p in range(P):
        nrm = np.linalg.norm(H[p])
        scale = max(1.0, nrm)
        w, U = np.linalg.eigh(H[p])
        V = evecs[p].T                                            # columns = eigenvectors
        assert np.all(np.diff(evals[p]) >= 0), f"{what} problem {p}: eigenvalues not ascending"
        worst["eval"] = max(worst["eval"], np.max(np.abs(evals[p] - w)) / scale)
        worst["resid"] = max(worst["resid"], np.max(np.linalg.norm(H[p] @ V - V * evals[p], axis=0)) / scale)
        worst["unit"] = max(worst["unit"], np.linalg.norm(V.conj().T @ V - np.eye(N), 2))
        np.testing.assert_allclose(np.linalg.norm(V, axis=0), 1.0, atol=1e-14)
        for g in _clusters(w, 1e-6 * nrm):
            mine = V[:, g] @ V[:, g].conj().T
            ref = U[:, g] @ U[:, g].conj().T
            key = "single" if len(g) == 1 else "cluster"
            worst[key] = max(worst[key], np.linalg.norm(mine - ref, 2))
        # phase: the first component above 1e-12 is real and positive
        for j in range(N):
            k = int(np.argmax(np.abs(evecs[p, j]) > 1e-12))
            assert evecs[p, j, k].imag == 0.0 and evecs[p, j, k].real > 0.0, f"{what} problem {p} vector {j}"
    print(f"{what}: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    assert worst["eval"] <= 1e-12, (what, worst)
    assert worst["resid"] <= 1e-12, (what, worst)
    assert worst["unit"] <= 1e-13, (what, worst)
    assert worst["single"] <= 1e-11, (what, worst)
    assert worst["cluster"] <= 1e-9, (what, worst)


def literal_occupations(evecs, rho):
    """general_dressed_states.py:161-165 as it stands: Re sum_ik v[i] conj(v[k]) rho[i][k]"""
    return np.einsum("...ji,...jk,...ik->...j", evecs, evecs.conj(), rho).real


def random_systems(N, n_sys, n_chan, grid, rng, short_samples=False):
    T = max(grid.dt * grid.n_steps, grid.dt)
    out = []
    for _ in range(n_sys):
        ns = int(rng.integers(3, 12))
        if short_samples:   # the samples cover the middle of the grid only: both ends are clamped
            t0, sdt = grid.ta + 0.3 * T, 0.4 * T / (ns - 1)
        else:               # the grid times fall between the samples
            t0, sdt = grid.ta - 0.013 * T, 1.031 * T / (ns - 1)
        chans = [(rng.uniform(1, 10) * (rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))) / 2,
                  rng.normal(size=ns) + 1j * rng.normal(size=ns)) for _ in range(n_chan)]
        out.append(System(dim=N, H0=_herm(rng, N, rng.uniform(1, 10)), channels=chans, sample_t0=t0, sample_dt=sdt))
    return out


def hard_matrices(N, rng):
    U = _unitary(rng, N)
    lam = np.array([1.0, 1.0] + list(range(2, N)), dtype=float)
    split = lam.copy()
    split[1] += 1e-9
    A = rng.normal(size=(N, N))
    span = np.diag(np.array([1e3, -1e3, 500.0, -500.0, 250.0, -250.0][:N])).astype(complex)
    iu = np.triu_indices(N, 1)
    mags = np.logspace(-8, 0, len(iu[0]))
    span[iu] = mags * np.exp(1j * rng.uniform(0, 2 * np.pi, len(mags)))
    span = np.triu(span) + np.triu(span, 1).conj().T
    return {
        "zero": np.zeros((N, N), dtype=complex),
        "diagonal descending": np.diag(np.arange(N, 0, -1.0)).astype(complex),
        "repeated eigenvalues": U @ np.diag(lam) @ U.conj().T,
        "pair split by 1e-9": U @ np.diag(split) @ U.conj().T,
        "imaginary off-diagonals": np.diag(rng.normal(size=N) * 5).astype(complex) + 1j * (A - A.T),
        "entries 1e-8..1e3": span,
    }


# ----------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("N", [2, 3, 4, 5, 6])
def test_kernel_against_eigh(N):
    rng = np.random.default_rng(100 + N)
    for n_sys in (1, 3):
        for n_steps in (0, 1, 62, 63, 64, 257):
            for n_chan in (0, 1, 4):
                grid = Grid(-1.5, 0.07, n_steps)
                systems = random_systems(N, n_sys, n_chan, grid, rng)
                H = np.stack([hamiltonians(s, grid) for s in systems])
                rho = rng.normal(size=H.shape) + 1j * rng.normal(size=H.shape)
                ev, vec, occ = engine.dressed_states(systems, grid, rho=rho)
                assert ev.shape == (n_sys, n_steps + 1, N)
                check_eigenpairs(H.reshape(-1, N, N), ev.reshape(-1, N), vec.reshape(-1, N, N),
                                 f"N={N} n_sys={n_sys} n_steps={n_steps} n_chan={n_chan}")
                np.testing.assert_allclose(occ, literal_occupations(vec, rho), rtol=0, atol=1e-13)
                ev2, vec2, occ2 = engine.dressed_states(systems, grid, rho=rho, want_vectors=False)
                assert vec2 is None
                np.testing.assert_array_equal(ev2, ev)
                np.testing.assert_array_equal(occ2, occ)
    # a single System (not a list) drops the system axis; without rho there are no occupations
    ev1, vec1, occ1 = engine.dressed_states(systems[0], grid)
    assert occ1 is None
    np.testing.assert_array_equal(ev1, ev[0])
    np.testing.assert_array_equal(vec1, vec[0])


@pytest.mark.parametrize("N", [2, 3, 4, 5, 6])
def test_clamped_sample_range(N):
    """the samples cover the middle of the grid only: before and after, the end samples are held"""
    rng = np.random.default_rng(200 + N)
    grid = Grid(2.0, 0.1, 100)
    systems = random_systems(N, 2, 2, grid, rng, short_samples=True)
    H = np.stack([hamiltonians(s, grid) for s in systems])
    assert np.array_equal(H[0, 0], H[0, 20]) and np.array_equal(H[0, -1], H[0, -20])   # held ends
    assert not np.array_equal(H[0, 40], H[0, 50])
    ev, vec, _ = engine.dressed_states(systems, grid)
    check_eigenpairs(H.reshape(-1, N, N), ev.reshape(-1, N), vec.reshape(-1, N, N), f"clamped N={N}")


@pytest.mark.parametrize("N", [2, 3, 4, 5, 6])
def test_hard_matrices(N):
    rng = np.random.default_rng(300 + N)
    mats = hard_matrices(N, rng)
    if N == 4:  # the undriven biexciton with degenerate excitons
        so = biexciton_ops(delta_xy=0)[0]
        mats["biexciton delta_xy=0"] = sum(opgrammar.to_matrix(s, 4) for s in so)
    grid = Grid(0.0, 1.0, 0)
    for name, Hm in mats.items():
        ev, vec, _ = engine.dressed_states([System(dim=N, H0=Hm)], grid)
        check_eigenpairs(Hm[None], ev[0], vec[0], f"N={N} {name}")
    # and all of them as one batch
    ev, vec, _ = engine.dressed_states([System(dim=N, H0=Hm) for Hm in mats.values()], grid)
    check_eigenpairs(np.stack(list(mats.values())), ev[:, 0], vec[:, 0], f"N={N} batch of hard matrices")
    z = mats["zero"]
    ev, vec, _ = engine.dressed_states(System(dim=N, H0=z), grid)
    np.testing.assert_array_equal(ev[0], np.zeros(N))
    np.testing.assert_array_equal(vec[0], np.eye(N))
    ev, vec, _ = engine.dressed_states(System(dim=N, H0=mats["diagonal descending"]), grid)
    np.testing.assert_array_equal(ev[0], np.arange(1.0, N + 1))
    np.testing.assert_array_equal(vec[0], np.eye(N)[::-1])


def test_nan_sample_raises_numeric_error():
    rng = np.random.default_rng(7)
    grid = Grid(0.0, 0.1, 40)
    (s,) = random_systems(4, 1, 1, grid, rng)
    X, f = s.channels[0]
    f = np.array(f)
    f[len(f) // 2] = np.nan
    s.channels = [(X, f)]
    with pytest.raises(_lib.NumericError):
        engine.dressed_states(s, grid)
    # the context stays usable
    ev, _, _ = engine.dressed_states(System(dim=4, H0=np.diag([3.0, 1.0, 2.0, 0.0])), grid)
    np.testing.assert_array_equal(ev[5], [0.0, 1.0, 2.0, 3.0])


# ----------------------------------------------------------------------------------------------- the driver
def _capture_systems(monkeypatch):
    """the Systems system_ace_stream hands to the dressed-state launch"""
    seen = {}
    real = gs.dressed_states

    def spy(systems, grid, **kw):
        seen["systems"], seen["grid"] = list(systems), grid
        return real(systems, grid, **kw)

    monkeypatch.setattr(gs, "dressed_states", spy)
    return seen


@pytest.mark.parametrize("sampling", ["ace_file", "exact"])
def test_tls_rotating_frame_closed_form(monkeypatch, sampling):
    seen = _capture_systems(monkeypatch)
    p = CWLaser(e0=0.35, e_start=-1.3)
    tab = tls(0, 20, p, dt=0.1, rf=True, dressedstates=True, pulse_sampling=sampling)
    assert tab.shape == (1 + 2 + 4, 201) and tab.dtype == np.complex128
    np.testing.assert_allclose(tab[0].real, 0.1 * np.arange(201), atol=1e-12)
    (s,) = seen["systems"]
    assert len(s.channels) == 2 and not s.lindblad
    H = hamiltonians(s, seen["grid"])
    g, delta = H[:, 1, 0], H[:, 1, 1].real
    assert np.all(np.abs(g) > 0.1) and np.all(np.abs(delta) > 1.0) and np.allclose(H[:, 0, 0], 0)
    # g = -pi hbar f / 2 from the pulse channel, Delta' = -hbar omega from the rf channel
    np.testing.assert_allclose(np.abs(g), 0.5 * np.pi * hbar * 0.35, rtol=1e-6)
    np.testing.assert_allclose(delta, 1.3, rtol=1e-6)
    root = np.sqrt(delta ** 2 + 4 * np.abs(g) ** 2)
    np.testing.assert_allclose(tab[1].real, 0.5 * (delta - root), rtol=0, atol=1e-12)
    np.testing.assert_allclose(tab[2].real, 0.5 * (delta + root), rtol=0, atol=1e-12)
    assert np.all(tab[1:3].imag == 0)
    vec = tab[3:].T.reshape(-1, 2, 2)
    check_eigenpairs(H, tab[1:3].real.T, vec, f"tls rf {sampling}")


@pytest.mark.parametrize("model", ["biexciton", "sixls_linear"])
def test_undriven_models_are_diagonal(model):
    if model == "biexciton":
        tab = biexciton(0, 5, dt=0.5, delta_b=4, delta_xy=0.3, dressedstates=True)
        H0 = sum(opgrammar.to_matrix(s, 4) for s in biexciton_ops(delta_xy=0.3, delta_b=4)[0])
    else:
        tab = sixls_linear(0, 5, dt=0.5, delta_b=4, dressedstates=True)
        H0 = sum(opgrammar.to_matrix(s, 6) for s in sixls_ops(delta_b=4)[0])
    N = H0.shape[0]
    assert tab.shape == (1 + N + N * N, 11)
    d = np.diag(H0).real
    assert np.array_equal(H0, np.diag(d)) and len(set(d)) == N
    order = np.argsort(d, kind="stable")
    for k in range(11):
        np.testing.assert_array_equal(tab[1: 1 + N, k].real, d[order])
        np.testing.assert_array_equal(tab[1 + N:, k].reshape(N, N), np.eye(N)[order])


def test_sixls_no_pulse_gives_the_field_basis():
    p = ChirpedPulse(tau_0=2.0, e_start=0.0, e0=3.0, t0=8.0)
    res = sixls_linear_dressed_states(0, 16, p, dt=0.5, bx=3.0, lindblad=True, no_pulse=True,
                                      return_eigenvectors=True, plot=False)
    t, pop, e_values, ds_occ, s_colors, n_colors, e_vectors, rho = res
    n_t = 33
    assert t.shape == (n_t,) and e_values.shape == (n_t, 6) and e_vectors.shape == (n_t, 6, 6)
    assert rho.shape == (n_t, 6, 6) and len(s_colors) == 6 and n_colors.shape == (6, n_t)
    H0 = sum(opgrammar.to_matrix(s, 6) for s in sixls_ops(bx=3.0, lindblad=True)[0])
    assert np.count_nonzero(H0 - np.diag(np.diag(H0))) == 4          # the field mixes bright and dark states
    for k in range(n_t):
        np.testing.assert_array_equal(e_vectors[k], e_vectors[0])    # constant in time
        np.testing.assert_array_equal(e_values[k], e_values[0])
    check_eigenpairs(H0[None], e_values[:1], e_vectors[:1], "sixls bx=3 no_pulse")
    w, U = np.linalg.eigh(H0)
    overlap = np.abs(e_vectors[0].conj() @ U)                         # |<v_j|u_l>|: identity up to phase
    np.testing.assert_allclose(overlap, np.eye(6), atol=1e-11)
    rot = tools.rotate_basis(rho, e_vectors[0])
    np.testing.assert_allclose(rot, rot.conj().transpose(0, 2, 1), atol=1e-12)
    np.testing.assert_allclose(np.trace(rot, axis1=1, axis2=2), 1.0, atol=1e-10)
    assert np.max(pop[:, 1].real) > 0.05                              # the pulse did drive the dot


@pytest.mark.parametrize("model", ["tls", "biexciton"])
def test_wrappers_under_a_gaussian_pulse(model):
    if model == "tls":
        p = ChirpedPulse(tau_0=3.0, e_start=0.0, e0=3.0, t0=12.0)
        res = tls_dressed_states(0, 24, p, dt=0.1, lindblad=True, phonons=False, return_eigenvectors=True)
        out = tls(0, 24, p, dt=0.1, lindblad=True, phonons=False, output_ops=tools.output_ops_dm(2))
        N = 2
    else:
        p = ChirpedPulse(tau_0=3.0, e_start=-2.0, e0=5.0, t0=12.0, polar_x=0.8)
        res = biexciton_dressed_states(0, 24, p, dt=0.25, lindblad=True, phonons=False, return_eigenvectors=True)
        out = biexciton(0, 24, p, dt=0.25, lindblad=True, phonons=False, output_ops=tools.output_ops_dm(4))
        N = 4
    t, pop, e_values, ds_occ, s_colors, n_colors, e_vectors, rho = res
    t_ref, rho_ref = tools.compose_dm(out, dim=N)
    np.testing.assert_array_equal(t, t_ref)
    np.testing.assert_allclose(rho, rho_ref, rtol=0, atol=1e-12)       # the same propagation, run again
    np.testing.assert_array_equal(pop, np.diagonal(rho, axis1=1, axis2=2))
    np.testing.assert_allclose(ds_occ.sum(axis=1), 1.0, rtol=0, atol=1e-10)
    np.testing.assert_allclose(ds_occ, literal_occupations(e_vectors, rho), rtol=0, atol=1e-13)
    assert np.ptp(e_values[:, 0]) > 0.05                               # the pulse dresses the levels
    assert np.all(np.diff(e_values, axis=1) >= 0)
    assert len(s_colors) == N and all(len(c) == len(t) for c in s_colors) and n_colors.shape == (N, len(t))
    short = tls_dressed_states(0, 4, p, dt=0.5) if model == "tls" else biexciton_dressed_states(0, 4, p, dt=0.5)
    assert len(short) == 6


def test_trajectories_form_is_one_launch():
    areas = [0.5, 1.0, 2.0, 3.5, 5.0]
    pulses = [ChirpedPulse(tau_0=3.0, e_start=0.5, e0=a, t0=12.0) for a in areas]
    singles = [tls_dressed_states(0, 24, p, dt=0.1, lindblad=True, return_eigenvectors=True) for p in pulses]
    before = engine.DRESSED_LAUNCHES
    batch = tls_dressed_states(0, 24, dt=0.1, lindblad=True, return_eigenvectors=True,
                               trajectories=[{"pulses": (p,)} for p in pulses])
    assert engine.DRESSED_LAUNCHES - before == 1
    assert len(batch) == 5
    for one, many in zip(singles, batch):
        assert len(many) == 8
        np.testing.assert_array_equal(many[0], one[0])
        np.testing.assert_allclose(many[2], one[2], rtol=0, atol=1e-13)   # eigenvalues
        np.testing.assert_allclose(many[3], one[3], rtol=0, atol=1e-13)   # occupations, evaluated on the device
        np.testing.assert_allclose(many[1], one[1], rtol=0, atol=1e-12)   # populations of the batched propagation
        assert many[4] == one[4]
    # the driver's own batched table: one table per drive, from one launch
    before = engine.DRESSED_LAUNCHES
    tabs = tls(0, 24, dt=0.1, dressedstates=True, trajectories=[{"pulses": (p,)} for p in pulses])
    assert engine.DRESSED_LAUNCHES - before == 1 and len(tabs) == 5
    for tab, one in zip(tabs, singles):
        np.testing.assert_allclose(tab[1:3].real.T, one[2], rtol=0, atol=1e-13)
