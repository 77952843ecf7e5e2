"""Dynamical maps on the Hilbert-space paths (pqd_dynmap_wide, engine.dynmap_wide, the wide_maps opt-in of the drop-in
layer): the map instances of lind_hilbert.hip and lind_hilbert_pt.hip and the device-side assembly. GPU only.

Reference: products of the half-step superoperators of tests/helpers.numpy_free_props (scipy's expm of the full
Liouvillian), computed once per case. Tolerance: 1e-12 relative to max|reference| (rel(), as tests/test_gpu_hilbert.py),
the bound the two kernels are held to. Equality (np.array_equal) where the arithmetic is the same: against the route
through N^2 trace outputs on N^2 MTO-prepared trajectories (multiplying by 1 and adding zeros is exact), between the
scalar and the sequence form of get_M_t, and under another number of bond slices in flight.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from pyaceqd_amd import _lib, engine
from pyaceqd_amd import pt as ptmod
from pyaceqd_amd.engine import MTO, Grid, System, Trajectories
from pyaceqd_amd.general_system import general_system as gs
from pyaceqd_amd.pulses import ChirpedPulse
from tests import helpers as H

pytestmark = pytest.mark.gpu
TOL = 1e-12


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def _dense(rng, N):
    return rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))


def _superop(m, N):
    A = np.asarray(m.op)
    return {0: np.kron(A, A.conj()), 1: np.kron(A, np.eye(N)), 2: np.kron(np.eye(N), A.T)}[m.kind]


def _map_product(M, n_steps, N, mtos=()):
    """dm[n - 1] = the superoperator of steps 0 .. n with the MTO factors of numpy_propagate.apply in a step's order"""
    S = np.eye(N * N, dtype=complex)
    dm = []
    for n in range(n_steps + 1):
        for m in mtos:
            if m.step == n and m.before:
                S = _superop(m, N) @ S
        if n >= 1:
            dm.append(S)
        for m in mtos:
            if m.step == n and not m.before:
                S = _superop(m, N) @ S
        if n == n_steps:
            break
        S = M[2 * n + 1] @ (M[2 * n] @ S)
    return np.array(dm)


@functools.lru_cache(maxsize=None)
def _case(N, n_sub=1, scale=1, n_steps=None):
    """system, grid and the half-step superoperators of one case (computed once, read-only afterwards)"""
    n_steps = n_steps or (2 if N == 24 else 4)
    sysd, grid = H.random_system(N, n_chan=2, n_lind=2, n_steps=n_steps, dt=0.1, n_sub=n_sub, seed=N)
    sysd.H0 = sysd.H0 * scale
    return sysd, grid, H.numpy_free_props(sysd, grid)


def _trace_route(sysd, grid, mtos=(), pt=None, **kw):
    """the maps as general_system._dynmap builds them: N^2 trajectories prepared by two MTOs, N^2 unit outputs"""
    N = sysd.dim
    N2 = N * N
    ket = lambda a, b: H.ketbra(N, a, b)  # noqa: E731
    ops = [ket(a % N, a // N) for a in range(N2)]
    ms = []
    for beta in range(N2):
        i, j = divmod(beta, N)
        ms += [MTO(beta, 0, True, 1, ket(i, 0)), MTO(beta, 0, True, 2, ket(0, j))]
        ms += [MTO(beta, m.step, m.before, m.kind, m.op) for m in mtos]
    tr = Trajectories(np.zeros(N2, dtype=int), np.full(N2, grid.n_steps), ms)
    outs = engine.propagate(sysd, grid, ket(0, 0), ops, tr, pt=pt, **kw)
    return np.stack(outs, axis=2)[1:]


# ------------------------------------------------------------------------------------------ 1. parity without a PT
@pytest.mark.parametrize("N,n_sub,scale", [(7, 1, 1), (7, 2, 1), (8, 1, 1), (8, 2, 1), (13, 1, 1), (13, 2, 1),
                                           (17, 1, 1), (18, 1, 1), (24, 1, 1), (8, 1, 20)])
def test_parity_without_a_pt(N, n_sub, scale):
    """7: first above the old limit; 8: N^2 is one wave; 13, 18: a ragged last wave; 17: the first N^2 above a plan's
    256 outputs; 24: the LDS maximum; H0 x 20 at N = 8: several Taylor factors per sub-step (s > 1)"""
    sysd, grid, M = _case(N, n_sub, scale)
    dm = engine.dynmap_wide(sysd, grid)
    ref = _map_product(M, grid.n_steps, N)
    assert dm.shape == (1, grid.n_steps, N * N, N * N)
    print(f"N={N} n_sub={n_sub} scale={scale}: rel err {rel(dm[0], ref):.3e}")
    assert rel(dm[0], ref) < TOL


# ------------------------------------------------------------------------------------------ 2. the existing route
@pytest.mark.parametrize("N", [8, 13])
def test_same_bits_as_the_trace_route(N):
    sysd, grid, _ = _case(N)
    dm = engine.dynmap_wide(sysd, grid)[0]
    old = _trace_route(sysd, grid)
    assert old.shape == dm.shape
    print(f"N={N}: max abs difference to the trace route {np.max(np.abs(dm - old)):.3e}")
    assert np.array_equal(dm, old)


# ------------------------------------------------------------------------------------------ 3. MTOs inside the map
def test_mtos_inside_the_map():
    N = 8
    sysd, grid, M = _case(N)
    rng = np.random.default_rng(31)
    A = lambda: _dense(rng, N) / N  # noqa: E731
    mtos = [MTO(0, 0, True, 0, A()), MTO(0, 2, False, 1, A()), MTO(0, 1, True, 2, A()), MTO(0, 1, True, 1, A())]
    dm = engine.dynmap_wide(sysd, grid, mtos=mtos)[0]
    ref = _map_product(M, grid.n_steps, N, mtos)
    print(f"MTOs inside the map: rel err {rel(dm, ref):.3e}")
    assert rel(dm, ref) < TOL
    assert np.array_equal(dm, _trace_route(sysd, grid, mtos))


# ------------------------------------------------------------------------------------------ 4. below dim 7
@pytest.mark.parametrize("N", [2, 4, 6])
def test_below_dim_7_through_the_engine(N):
    sysd, grid = H.random_system(N, n_steps=4, seed=40 + N)
    dm = engine.dynmap_wide(sysd, grid)[0]
    ref = _map_product(engine.free_propagators(sysd, grid), grid.n_steps, N)
    print(f"N={N}: rel err to the free propagators' product {rel(dm, ref):.3e}")
    assert rel(dm, ref) < TOL


# ------------------------------------------------------------------------------------------ 5. get_M_t
def _pulse():
    return ChirpedPulse(tau_0=0.4, e_start=0.0, e0=2.0, t0=0.3, alpha=0.5)


def test_get_M_t_at_dim_8():
    from pyaceqd_amd.two_level_system.tls import tls_two_sensor
    kw = dict(dt=0.1, lindblad=True, epsilon=0.05, n_sub=2)
    run = lambda **k: tls_two_sensor(0, 1, _pulse(), wide_maps=True, **kw, **k)  # noqa: E731
    sysd = tls_two_sensor(0, 1, _pulse(), lower_only=True, **kw).systems[0]
    M = run(get_M_t=0.2)
    assert M.shape == (64, 64)
    assert np.array_equal(M, engine.dynmap_wide(sysd, Grid(0.2, 0.1, 1, 2))[0, 0])
    P = H.numpy_free_props(sysd, Grid(0.2, 0.1, 1, 2))
    print(f"get_M_t: rel err to expm {rel(M, P[1] @ P[0]):.3e}")
    assert rel(M, P[1] @ P[0]) < TOL
    times = [0.0, 0.1, 0.2, 0.3, 0.234]
    Ms = run(get_M_t=times)
    assert Ms.shape == (5, 64, 64)
    for k, t in enumerate(times):
        assert np.array_equal(Ms[k], run(get_M_t=t)), t
    # the on-grid one-step maps in order are the cumulative map
    _, dm = run(calc_dynmap=True)
    S = np.eye(64, dtype=complex)
    for n in range(4):
        S = Ms[n] @ S
        print(f"product of {n + 1} one-step maps: rel err {rel(S, dm[n]):.3e}")
        assert rel(S, dm[n]) < (n + 1) * TOL


def test_get_M_t_sequence_at_dim_4():
    from pyaceqd_amd.four_level_system.linear import biexciton
    times = [0.0, 0.5, 0.3]
    run = lambda t: biexciton(0, 2, _pulse(), dt=0.1, lindblad=True, get_M_t=t)  # noqa: E731
    Ms = run(times)
    assert Ms.shape == (3, 16, 16)
    for k, t in enumerate(times):
        assert np.array_equal(Ms[k], run(t))


# ------------------------------------------------------------------------------------------ 6. with a PT
def _pt_maps(sysd, grid, M, pt):
    """the numpy_propagate recursion on all basis columns at once: st[alpha, beta, d]"""
    N2 = sysd.dim ** 2
    st = np.einsum("ab,d->abd", np.eye(N2), pt.bond0).astype(complex)
    sched = pt.schedule(grid.n_steps)
    dm = []
    for n in range(grid.n_steps):
        st = np.einsum("xa,abd->xbd", M[2 * n], st)
        Qs = pt.Q[sched[n]]
        st = np.stack([st[a] @ Qs[pt.gmap[a]] for a in range(N2)])
        st = np.einsum("xa,abd->xbd", M[2 * n + 1], st)
        dm.append(st @ pt.closure[sched[n]])
    return np.array(dm)


@pytest.mark.parametrize("N,chi", [(7, 3), (8, 5), (18, 2)])
def test_parity_with_a_pt(N, chi, monkeypatch):
    sysd, grid, M = _case(N, n_steps=3)
    pt = ptmod.random_pt(N, chi, 4, n_slices=4, seed=N, eps=0.1)
    monkeypatch.delenv("PQD_HBPT_G", raising=False)
    dm = engine.dynmap_wide(sysd, grid, pt=pt)[0]
    ref = _pt_maps(sysd, grid, M, pt)
    print(f"N={N} chi={chi}: rel err {rel(dm, ref):.3e}")
    assert dm.shape == ref.shape and rel(dm, ref) < TOL
    if N == 7:  # the slices in flight (3 by default here) do not change a bit
        monkeypatch.setenv("PQD_HBPT_G", "1")
        assert np.array_equal(engine.dynmap_wide(sysd, grid, pt=pt)[0], dm)


def test_pt_at_dim_2_against_the_sweep_path():
    N, chi = 2, 7
    sysd, grid = H.random_system(N, n_steps=5, seed=52)
    pt = ptmod.random_pt(N, chi, 4, n_slices=4, seed=5, eps=0.1)
    _, old = gs._dynmap(sysd, grid, pt, H.random_rho(N), None, [], grid.ta, grid.dt, N, None)
    dm = engine.dynmap_wide(sysd, grid, pt=pt)[0]
    print(f"N=2 chi=7: rel err to calc_dynmap on the sweep path {rel(dm, old):.3e}")
    assert dm.shape == old.shape and rel(dm, old) < TOL


# ------------------------------------------------------------------------------------------ 7. through the wrappers
def test_calc_dynmap_through_tls_two_sensor():
    from pyaceqd_amd.two_level_system.tls import tls_two_sensor
    kw = dict(dt=0.1, lindblad=True, epsilon=0.05)
    plain = tls_two_sensor(0, 1, _pulse(), **kw)
    res, dm = tls_two_sensor(0, 1, _pulse(), calc_dynmap=True, wide_maps=True, **kw)
    assert dm.shape == (10, 64, 64) and res.shape == plain.shape == (3, 11)
    print(f"result vs the plain call: rel err {rel(res, plain):.3e}")
    assert rel(res, plain) < TOL
    rho = dm[:, :, 0].reshape(10, 8, 8)  # rho0 = |0><0|: column 0
    occ = np.stack([np.einsum("nii->n", rho[:, :4, :4]), np.einsum("nii->n", rho[:, 4:, 4:])])
    print(f"dm @ vec(rho0) vs the occupations: rel err {rel(occ, plain[1:, 1:]):.3e}")
    assert rel(occ, plain[1:, 1:]) < TOL
    assert np.max(np.abs(plain[2])) > 1e-3  # the pulse did drive the system


def test_get_M_t_through_tls_photons_is_a_physical_map():
    from pyaceqd_amd.two_level_system.tls import tls_photons
    M = tls_photons(0, 1, _pulse(), dt=0.1, lindblad=True, get_M_t=0.3, wide_maps=True)
    assert M.shape == (324, 324)
    N = 18
    diag = np.arange(N) * (N + 1)
    tr = M[diag].sum(axis=0)
    want = np.zeros(N * N)
    want[diag] = 1
    print(f"trace preservation: max abs err {np.max(np.abs(tr - want)):.3e}")
    assert np.max(np.abs(tr - want)) < TOL
    T = M.reshape(N, N, N, N)
    herm = np.max(np.abs(T - T.transpose(1, 0, 3, 2).conj())) / np.max(np.abs(M))
    print(f"Hermiticity preservation: rel err {herm:.3e}")
    assert herm < TOL
    assert np.max(np.abs(M - np.eye(N * N))) > 1e-3


# ------------------------------------------------------------------------------------------ 8. refusals and errors
def _raises(code, fn, *a, **k):
    with pytest.raises((_lib.PQDError, ValueError)) as ei:
        fn(*a, **k)
    assert ei.value.code == code, ei.value
    return str(ei.value)


def test_refusals_name_the_value():
    s9, g9 = H.random_system(8, n_lind=9, n_steps=2, seed=1)
    assert "n_lind 9" in _raises(3, engine.dynmap_wide, s9, g9)
    s8, g8 = H.random_system(8, n_steps=2, seed=2)
    s8.H0 = s8.H0 * 1e6
    assert "norm bound" in _raises(3, engine.dynmap_wide, s8, g8)
    s25 = System(dim=25, H0=np.zeros((25, 25)))
    assert "dim 25 not in [2, 24]" in _raises(3, engine.dynmap_wide, s25, Grid(0, 0.1, 1))
    ok, g = H.random_system(8, n_steps=2, seed=2)
    assert "n_steps 0" in _raises(1, engine.dynmap_wide, ok, Grid(0, 0.1, 0))
    # a wrong dm_len, through the C-ABI itself
    ctx = _lib.context()
    sc, keep = ok.to_c()
    gc = g.to_c()
    dm = np.zeros(2 * 64 * 64, dtype=np.complex128)
    rc = _lib.lib().pqd_dynmap_wide(ctx.handle, C.byref(sc), C.byref(gc), None, None, 1, None, 0, None, None, None,
                                    None, _lib.cptr(dm), dm.size - 1)
    assert rc == 1 and b"dm_len 8191" in _lib.lib().pqd_last_error()
    rc = _lib.lib().pqd_dynmap_wide(ctx.handle, C.byref(sc), C.byref(gc), None, None, 0, None, 0, None, None, None,
                                    None, _lib.cptr(dm), dm.size)
    assert rc == 1 and b"n_maps 0" in _lib.lib().pqd_last_error()


def test_nan_in_h0_is_a_numeric_error():
    s8, g8 = H.random_system(8, n_steps=2, seed=3)
    s8.H0 = s8.H0.copy()
    s8.H0[2, 5] = np.nan
    with pytest.raises(_lib.NumericError):
        engine.dynmap_wide(s8, g8)
    ok, g = H.random_system(8, n_steps=2, seed=3)  # the context stays usable
    assert np.all(np.isfinite(engine.dynmap_wide(ok, g)))
