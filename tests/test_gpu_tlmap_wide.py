"""Time-local maps at map sizes 37 .. 576 (csrc/tlmap_wide.hip: the block-Jacobi pinv behind pqd_tl_dynmap_pseudo and
tools.calc_tl_dynmap_pseudo) against oracle.tl_dynmap_pseudo, the numpy restatement that tests/test_pyref_golden.py pins
to the reference's own function.

Error measure: max|got - ref| / max|ref| (as tests/test_gpu_wide_maps.py). Bound 1e-10, the one this function is held to
on its goldens. "Graded" maps are Q1 diag(s) Q2 with Haar-like Q (numpy.linalg.qr of complex normal matrices, fresh per
map) and s log-spaced from 1 to 1e-3: the condition number 1e3 keeps eps * cond (2e-13) far below the bound, and two
LAPACK routes (gesdd inside numpy's pinv, gesvd) agree to 5e-15 (full rank) and 2.2e-14 (rank-deficient) on such inputs.
The kernel changes its column block (8 -> 4, a pair's lanes 32 -> 64) between n = 128 and 129: 127 .. 130 are test points.
"""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle
from pyaceqd_amd import _lib
from pyaceqd_amd import tools as T

pytestmark = pytest.mark.gpu
TOL = 1e-10
PQD_ERR_ARG = 1


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def _haar(rng, n):
    return np.linalg.qr(rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n)))[0]


def _graded(rng, n, n_maps, tail=None):
    """n_maps maps Q1 diag(s) Q2, s log-spaced 1 .. 1e-3; `tail` replaces the last len(tail) singular values"""
    dm = np.empty((n_maps, n, n), dtype=np.complex128)
    for i in range(n_maps):
        s = np.logspace(0, -3, n)
        if tail is not None:
            s[-len(tail):] = tail
        dm[i] = (_haar(rng, n) * s) @ _haar(rng, n)
    return dm


def _times(n_maps):
    return np.round(np.arange(n_maps + 1) * 0.1, 6)


def _capi(dm, rcond, ctx=None):
    dm = np.ascontiguousarray(dm, dtype=np.complex128)
    out = np.empty_like(dm)
    ctx = ctx or _lib.context()
    with ctx.lock:
        _lib.check(_lib.lib().pqd_tl_dynmap_pseudo(ctx.handle, _lib.cptr(dm), len(dm), dm.shape[1], rcond, _lib.cptr(out)))
    return out


def _sweeps():
    n = C.c_int32(0)
    ctx = _lib.context()
    _lib.check(_lib.lib().pqd_tl_dynmap_sweeps(ctx.handle, C.byref(n)))
    return n.value


# ------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("n", [37, 49, 50, 64, 65, 100, 127, 128, 129, 130, 256, 324, 576])
def test_parity_on_graded_maps(n):
    n_maps = 2 if n == 576 else 3 if n >= 256 else 4
    dm = _graded(np.random.default_rng(n), n, n_maps)
    got = T.calc_tl_dynmap_pseudo(dm, _times(n_maps))
    ref = oracle.tl_dynmap_pseudo(dm)
    assert got.shape == ref.shape
    assert np.array_equal(got[0], dm[0])
    err = rel(got, ref)
    print(f"n = {n}: rel err {err:.3e}, sweeps {_sweeps()}")
    assert err < TOL


# ------------------------------------------------------------------------------------------ 2. more maps than workgroups
def test_more_maps_than_the_grid_has_workgroups():
    """3,000 cumulative products of near-unitary steps at n = 37 (the construction of test_tl_dynmap_large_vs_oracle):
    vs the oracle, and the time-local maps give back the steps. Every singular value is close to 1."""
    import scipy.linalg as sla
    n, n_maps = 37, 3000
    rng = np.random.default_rng(37)
    G = 0.05 * (rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n)))
    base = sla.expm(G - G.conj().T)
    steps = np.empty((n_maps, n, n), dtype=complex)
    for i in range(n_maps):
        steps[i] = base @ (np.eye(n) + 1e-3 * np.sin(0.01 * i) * (G + G.conj().T))
    dm = np.empty_like(steps)
    acc = np.eye(n, dtype=complex)
    for i in range(n_maps):
        acc = steps[i] @ acc
        dm[i] = acc
    got = T.calc_tl_dynmap_pseudo(dm, _times(n_maps))
    e_or, e_st = rel(got, oracle.tl_dynmap_pseudo(dm)), rel(got, steps)
    print(f"3000 maps of 37: vs oracle {e_or:.3e}, vs the steps {e_st:.3e}, sweeps {_sweeps()}")
    assert e_or < 1e-9
    assert e_st < 1e-9


# ------------------------------------------------------------------------------------------ 3. the cut-off
@pytest.mark.parametrize("n", [37, 64, 324])
def test_cut_off_with_a_gap_on_both_sides(n):
    dm = _graded(np.random.default_rng(1000 + n), n, 3, tail=[0.0, 0.0, 0.0, 1e-14, 1e-14])
    got = T.calc_tl_dynmap_pseudo(dm, _times(3))
    err = rel(got, oracle.tl_dynmap_pseudo(dm))
    print(f"n = {n}, rank n - 5: rel err {err:.3e}, sweeps {_sweeps()}")
    assert err < TOL


# ------------------------------------------------------------------------------------------ 4. rcond
@pytest.mark.parametrize("n", [37, 100])
def test_rcond_is_honoured(n):
    dm = _graded(np.random.default_rng(2000 + n), n, 3, tail=[1e-8, 1e-8, 1e-8])
    ref6 = oracle.tl_dynmap_pseudo(dm, rcond=1e-6)
    ref12 = oracle.tl_dynmap_pseudo(dm, rcond=1e-12)
    assert rel(ref12, ref6) > 1e4   # the two cuts give different maps: a hard-wired rcond cannot pass
    err = rel(_capi(dm, 1e-6), ref6)
    print(f"n = {n}, rcond 1e-6: rel err {err:.3e}")
    assert err < TOL


# ------------------------------------------------------------------------------------------ 5. batch independence
@pytest.mark.parametrize("n", [49, 100])
def test_a_map_does_not_depend_on_its_batch(n):
    dm = _graded(np.random.default_rng(3000 + n), n, 70)
    full = _capi(dm, 1e-12)
    assert np.array_equal(full, _capi(dm, 1e-12))
    for i in (1, 37, 69):
        alone = _capi(dm[i - 1:i + 1], 1e-12)
        assert np.array_equal(alone[1], full[i]), i


# ------------------------------------------------------------------------------------------ 6. through the product
def test_through_tls_two_sensor():
    from pyaceqd_amd.pulses import ChirpedPulse
    from pyaceqd_amd.two_level_system.tls import tls_two_sensor
    pulse = ChirpedPulse(tau_0=0.4, e_start=0.0, e0=2.0, t0=0.3, alpha=0.5)
    res, dm = tls_two_sensor(0, 2, pulse, calc_dynmap=True, wide_maps=True, dt=0.1, lindblad=True, epsilon=0.05)
    t = np.real(res[0])
    assert dm.shape == (20, 64, 64) and len(t) == 21
    tl = T.calc_tl_dynmap_pseudo(dm, t)
    assert tl.shape == (len(t) - 1, 64, 64)
    assert np.array_equal(tl[0], dm[0])
    for i in range(1, len(tl)):
        cond = np.linalg.cond(dm[i - 1])
        err = rel(tl[i] @ dm[i - 1], dm[i])
        print(f"step {i}: cond {cond:.3e}, tl[i] dm[i-1] vs dm[i] {err:.3e}")
        assert cond < 1e4
        assert err < 1e-9


# ------------------------------------------------------------------------------------------ 7. timing, dispatch
def test_timing_and_the_small_kernel_after_a_wide_call(golden_dir):
    L = _lib.lib()
    ctx = _lib.Context(_lib.context().device)
    ms = C.c_double(-1.0)
    assert L.pqd_tl_dynmap_timing(ctx.handle, C.byref(ms)) == PQD_ERR_ARG
    assert b"no pqd_tl_dynmap_pseudo call" in L.pqd_last_error()
    dm = _graded(np.random.default_rng(7), 40, 3)
    wide = _capi(dm, 1e-12, ctx)
    assert rel(wide, oracle.tl_dynmap_pseudo(dm)) < TOL
    _lib.check(L.pqd_tl_dynmap_timing(ctx.handle, C.byref(ms)))
    print(f"3 maps of 40: kernel {ms.value:.3f} ms")
    assert ms.value > 0.0
    z = np.load(os.path.join(golden_dir, "pyref_tlmap.npz"))
    for name in ("d4", "d5", "rank2", "rank4"):
        d = z[f"{name}_dm"][:len(z[f"{name}_times"]) - 1]
        assert rel(_capi(d, 1e-12, ctx), z[f"{name}_tl"]) < TOL, name
    _lib.check(L.pqd_tl_dynmap_timing(ctx.handle, C.byref(ms)))
    assert ms.value > 0.0
