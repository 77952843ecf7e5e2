"""The single-wave time-local-map kernel (csrc/tlmap.hip, map sizes n <= 36: every product caller at Hilbert dimension
<= 6) at every size, through the rcond cut-off, and against a multi-precision truth.

Error measure: rel = max|got - ref| / max|ref| per map, in units of
    u = eps (|T|_2 |A|_2 + |E|_2) / s_min_kept / max|T|          (helpers.tl_unit; A = dm[i-1], E = dm[i], T = ref),
the first-order change of E pinv(A) under eps-sized backward errors in A and E: about eps * cond, 1e-15 for a map with
singular values near 1 and 1e-7 at condition 1e9. A flat bound cannot serve both ends. Bounds:
  * 4 u against the truth of tests/golden/mp_tlmap_truth.npz (60-digit SVD; tests/test_tlmap_truth_host.py shows on
    the CPU that numpy's pinv is within 0.91 u of it and the kernel's algorithm, restated in numpy, within 0.78 u);
  * 5 u against numpy's pinv where there is no truth: the kernel's 4 plus the reference's 1.
Agreement of two LAPACK routes (gesdd, gesvd) is not used as evidence here: they share the bidiagonalisation, agree to
6e-15 at every condition number, and are eps * cond from the truth together.

A map with a singular value within 1 % of rcond * s_max (helpers.tl_near_cut) has no defined answer (a Jacobi singular
value is good to eps * s_max, 2e-4 relative at the cut 1e-12 * s_max) and is left out; the chains assert that this
leaves out at most 2 % of their maps.

numpy's pinv itself is several u from the truth on some well-conditioned maps (cond about 2, u about 4 eps: its
constant, not eps * cond, decides there; up to 14 u on the first two maps of semigroup chains). The chain seeds below
are ones where numpy stays within 1 u of a long-double run of helpers.tl_jacobi_restated on every compared map, which
is what the 5 u bound assumes of the reference (0.92, 0.88, 0.87 and 0.88 u at N = 2, 3, 4 and 6; at N = 5 no seed
of 130 did better than 1.25 u, and the one used is at 1.38 u). They were chosen on the CPU from the reference alone:
at most two maps near the cut, numpy's distance from that long-double run, and how well numpy's own time-local maps
give back the step (1.9 .. 2.5 eps cond, 3.9 at N = 5, where no seed of 130 was below 3.8; the bound is 5).

Every call also checks pqd_tl_dynmap_sweeps: at least 1, at most 2 more than the numpy restatement needs for the worst
map of the call (FMA contraction can move a rotation across the threshold), never more than 30 (the cap is 40).
The restatement evaluates the rotation of A fused, as the kernel's instructions do: with exactly equal columns a plain
float64 c x - s y is an exact zero where the kernel keeps a product's rounding error and goes on to orthogonalise such
residue, and a restatement without that expected 6 sweeps at n = 9 where the kernel, rightly by its rule, runs 10.

Worst figures measured on an MI355X: profiles/r24/tlmap_small/README.md.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from oracle import oracle
from pyaceqd_amd import _lib
from pyaceqd_amd import tools as T
from tests.conftest import GOLDEN
from tests.helpers import (EPS, tl_graded, tl_haar, tl_jacobi_restated, tl_kept, tl_near_cut, tl_rel,
                           tl_semigroup_chain, tl_unit)

pytestmark = pytest.mark.gpu
PQD_ERR_NUMERIC = 5
U_TRUTH, U_NUMPY = 4.0, 5.0
CHAIN_SEEDS = {2: 204, 3: 325, 4: 403, 5: 549, 6: 608}   # see the docstring; 2, 3, 4 as in make_golden_tlmap_truth.py
N_CHAIN = 120


def _call(dm, rcond):
    """pqd_tl_dynmap_pseudo as it is: (status, maps, sweep count of the call, message)"""
    dm = np.ascontiguousarray(dm, dtype=np.complex128)
    out = np.full_like(dm, np.nan)
    L, ctx = _lib.lib(), _lib.context()
    sw = C.c_int32(-7)
    with ctx.lock:
        rc = L.pqd_tl_dynmap_pseudo(ctx.handle, _lib.cptr(dm), len(dm), dm.shape[1], rcond, _lib.cptr(out))
        msg = L.pqd_last_error().decode() if rc else ""
        _lib.check(L.pqd_tl_dynmap_sweeps(ctx.handle, C.byref(sw)))
    return rc, out, sw.value, msg


def _through_tools(dm):
    """tools.calc_tl_dynmap_pseudo (rcond 1e-12) and the sweep count of its call"""
    out = T.calc_tl_dynmap_pseudo(dm, np.round(np.arange(len(dm) + 1) * 0.1, 6))
    sw = C.c_int32(-7)
    _lib.check(_lib.lib().pqd_tl_dynmap_sweeps(_lib.context().handle, C.byref(sw)))
    return out, sw.value


def _check_sweeps(sweeps, dm, rcond, expected=None):
    """the call's sweep count against the restatement's for its worst map; returns the latter"""
    if expected is None:
        expected = int(tl_jacobi_restated(dm, rcond)[1].max())
    assert 1 <= sweeps <= min(30, expected + 2), (sweeps, expected)
    return expected


def _run(dm, rcond=1e-12, expected=None):
    """a clean call: the maps, out[0] bit-equal to dm[0], the sweep count checked; returns (maps, sweeps)"""
    rc, out, sweeps, msg = _call(dm, rcond)
    assert rc == 0, msg
    assert np.array_equal(out[0], dm[0])
    _check_sweeps(sweeps, dm, rcond, expected)
    return out, sweeps


def _units(got, ref, dm, rcond, skip=()):
    """worst rel / u over the maps i >= 1 of a chain that are not in `skip`, and the worst rel"""
    worst_u = worst = 0.0
    for i in range(1, len(dm)):
        if i in skip:
            continue
        r = tl_rel(got[i], ref[i])
        worst, worst_u = max(worst, r), max(worst_u, r / tl_unit(dm[i - 1], dm[i], ref[i], rcond))
    return worst_u, worst


# ------------------------------------------------------------------------------------------ 1. the truth
with np.load(os.path.join(GOLDEN, "mp_tlmap_truth.npz"), allow_pickle=False) as _z:
    TRUTH = {str(k): (_z[f"{k}_A"], _z[f"{k}_E"], _z[f"{k}_T"], float(_z[f"{k}_rcond"])) for k in _z["names"]}


@pytest.mark.parametrize("name", list(TRUTH))
def test_against_the_multiprecision_truth(name):
    A, E, Tr, rcond = TRUTH[name]
    out, sweeps = _run(np.stack([A, E]), rcond)
    r = tl_rel(out[1], Tr) / tl_unit(A, E, Tr, rcond)
    print(f"{name}: rel {tl_rel(out[1], Tr):.3e} = {r:.2f} u, sweeps {sweeps}")
    assert r <= U_TRUTH


# ------------------------------------------------------------------------------------------ 2. every size
@pytest.mark.parametrize("n", range(1, 37))
def test_every_size_on_graded_maps(n):
    dm = tl_graded(np.random.default_rng(4000 + n), n, 4)
    out, sweeps = _run(dm)
    wu, w = _units(out, oracle.tl_dynmap_pseudo(dm), dm, 1e-12)
    print(f"n = {n}: worst rel {w:.3e} = {wu:.2f} u, sweeps {sweeps}")
    assert wu <= U_NUMPY
    assert w < 1e-12


# ------------------------------------------------------------------------------------------ 3. through the cut-off
@functools.lru_cache(maxsize=None)
def _chain(N):
    """the step, the 120 cumulative maps, numpy's time-local maps, the maps left out, the kept ranks of dm[i-1], and the
    restatement's largest sweep count"""
    step, dm = tl_semigroup_chain(N, CHAIN_SEEDS[N], N_CHAIN)
    ref = oracle.tl_dynmap_pseudo(dm)
    skip = frozenset(i for i in range(1, N_CHAIN) if tl_near_cut(dm[i - 1], 1e-12))
    kept = [tl_kept(dm[i - 1], 1e-12)[1] for i in range(1, N_CHAIN)]
    for a in (step, dm, ref):
        a.setflags(write=False)
    return step, dm, ref, skip, kept, int(tl_jacobi_restated(dm, 1e-12)[1].max())


@pytest.mark.parametrize("N", [2, 3, 4, 5, 6])
def test_semigroup_chain_through_the_cut_off(N):
    step, dm, ref, skip, kept, expected = _chain(N)
    n = N * N
    assert len(skip) <= 0.02 * (N_CHAIN - 1), sorted(skip)
    assert kept[0] == n and kept[-1] == 1 and all(a >= b for a, b in zip(kept, kept[1:]))
    got, sweeps = _through_tools(dm)
    assert got.shape == dm.shape and np.array_equal(got[0], dm[0])
    _check_sweeps(sweeps, dm, 1e-12, expected)
    wu, w = _units(got, ref, dm, 1e-12, skip)
    # the full-rank stretch: the time-local map is the step again, to eps * cond of the map that was inverted
    wstep = 0.0
    full = [i for i in range(1, N_CHAIN) if kept[i - 1] == n]
    for i in full:
        s = tl_kept(dm[i - 1], 1e-12)[0]
        wstep = max(wstep, tl_rel(got[i], step) / (EPS * s[0] / s[-1]))
    print(f"N = {N}: {len(skip)} maps left out, rank {kept[0]} -> {kept[-1]}, full rank up to map {full[-1]}; "
          f"worst {wu:.2f} u (rel {w:.3e}); vs the step {wstep:.2f} eps cond; sweeps {sweeps} (restated {expected})")
    assert len(full) >= 20
    assert wu <= U_NUMPY
    assert wstep <= 5.0


# ------------------------------------------------------------------------------------------ 4. rcond
@pytest.mark.parametrize("n", [9, 36])
def test_rcond_moves_the_cut(n):
    dm = tl_graded(np.random.default_rng(5000 + n), n, 3, tail=[1e-8] * 3)
    ref6, ref12 = oracle.tl_dynmap_pseudo(dm, rcond=1e-6), oracle.tl_dynmap_pseudo(dm, rcond=1e-12)
    assert tl_rel(ref12, ref6) > 1e4   # the two cuts give different maps: a hard-wired rcond cannot pass
    for rcond, ref in ((1e-6, ref6), (1e-12, ref12)):
        wu, w = _units(_run(dm, rcond)[0], ref, dm, rcond)
        print(f"n = {n}, rcond {rcond:g}: worst {wu:.2f} u (rel {w:.3e})")
        assert wu <= U_NUMPY


@pytest.mark.parametrize("n", [9, 36])
def test_rcond_half_keeps_the_top_of_the_spectrum(n):
    dm = tl_graded(np.random.default_rng(5100 + n), n, 3, cond=1e6)
    kept = tl_kept(dm[0], 0.5)[1]
    assert 1 <= kept <= 2 < n and not tl_near_cut(dm[0], 0.5) and not tl_near_cut(dm[1], 0.5)
    wu, w = _units(_run(dm, 0.5)[0], oracle.tl_dynmap_pseudo(dm, rcond=0.5), dm, 0.5)
    print(f"n = {n}, rcond 0.5 keeps {kept}: worst {wu:.2f} u (rel {w:.3e})")
    assert wu <= U_NUMPY


@pytest.mark.parametrize("n", [9, 36])
def test_rcond_one_keeps_nothing(n):
    """numpy's rule is a strict s > rcond * s_max: at rcond = 1 not even s_max passes"""
    dm = tl_graded(np.random.default_rng(5200 + n), n, 3)
    ref = oracle.tl_dynmap_pseudo(dm, rcond=1.0)
    assert not ref[1:].any()
    out, _ = _run(dm, 1.0)
    assert not out[1:].any()


@pytest.mark.parametrize("n", [9, 36])
def test_rcond_zero(n):
    """on full-rank maps, and on maps with one exactly-zero column c: no rotation changes that column, its s_j is exactly
    0 and 0 > 0 drops it. LAPACK's smallest singular value of such a map is about 1e-18, not 0, so numpy's pinv at
    rcond = 0 inverts it and is no reference. The reference is the same pinv written without the column: row c of
    pinv(A) is zero and the other rows are pinv(A without column c), a full-rank n x (n - 1) problem that numpy solves
    at rcond = 0; the unit is taken on that problem too."""
    dm = tl_graded(np.random.default_rng(5300 + n), n, 3)
    wu, w = _units(_run(dm, 0.0)[0], oracle.tl_dynmap_pseudo(dm, rcond=0.0), dm, 0.0)
    print(f"n = {n}, rcond 0, full rank: worst {wu:.2f} u (rel {w:.3e})")
    assert wu <= U_NUMPY
    c = n // 2
    dm[:, :, c] = 0.0
    rest = np.delete(np.arange(n), c)
    out, _ = _run(dm, 0.0)
    wu = w = 0.0
    for i in (1, 2):
        A, E = dm[i - 1][:, rest], dm[i][:, rest]
        assert tl_kept(A, 0.0)[1] == n - 1
        ref = E @ np.linalg.pinv(A, rcond=0.0)
        r = tl_rel(out[i], ref)
        w, wu = max(w, r), max(wu, r / tl_unit(A, E, ref, 0.0))
    print(f"n = {n}, rcond 0, a zero column: worst {wu:.2f} u (rel {w:.3e})")
    assert wu <= U_NUMPY


# ------------------------------------------------------------------------------------------ 5. structured inputs
def _structured(kind, n):
    rng = np.random.default_rng(6000 + n)
    if kind == "identity":
        return np.eye(n, dtype=complex)
    if kind == "permutation":
        return np.eye(n, dtype=complex)[rng.permutation(n)]
    if kind == "diagonal_descending":
        return np.diag(np.logspace(0, -3, n) * np.exp(1j * np.arange(n))).astype(complex)
    if kind == "diagonal_ascending":
        return np.diag(np.logspace(-3, 0, n) * np.exp(1j * np.arange(n))).astype(complex)
    if kind == "equal_columns":      # exact rank 1, and alpha = beta in the first rotation of every pair
        return np.repeat(rng.normal(size=(n, 1)) + 1j * rng.normal(size=(n, 1)), n, axis=1)
    if kind == "zero":
        return np.zeros((n, n), dtype=complex)
    if kind == "hermitian_repeated":   # eigenvalues 1, -1, 1 (n = 2: 1, -1) and distinct others: a repeated s = 1
        d = np.concatenate([[1.0, -1.0, 1.0], 0.8 - 0.02 * np.arange(n)])[:n]
        Q = tl_haar(rng, n)
        A = (Q * d) @ Q.conj().T
        return 0.5 * (A + A.conj().T)
    raise ValueError(kind)


NO_ROTATION = ("identity", "permutation", "diagonal_descending", "diagonal_ascending", "zero")


@pytest.mark.parametrize("n", [2, 9, 36])
@pytest.mark.parametrize("kind", NO_ROTATION + ("equal_columns", "hermitian_repeated"))
def test_structured_inputs(kind, n):
    A = _structured(kind, n)
    E = tl_graded(np.random.default_rng(6100 + n), n, 1)[0]
    dm = np.stack([A, E])
    out, sweeps = _run(dm)
    ref = oracle.tl_dynmap_pseudo(dm)
    if kind in NO_ROTATION:
        assert sweeps == 1
    if kind == "zero":
        assert not ref[1].any() and not out[1].any()
        return
    if kind == "equal_columns":
        assert tl_kept(A, 1e-12)[1] == 1
    assert not tl_near_cut(A, 1e-12)
    wu, w = _units(out, ref, dm, 1e-12)
    print(f"{kind}, n = {n}: {wu:.2f} u (rel {w:.3e}), sweeps {sweeps}")
    assert wu <= U_NUMPY


# ------------------------------------------------------------------------------------------ 6. batches
@pytest.mark.parametrize("n", [9, 36])
def test_a_map_does_not_depend_on_its_batch(n):
    dm = tl_graded(np.random.default_rng(7000 + n), n, 70)
    expected = tl_jacobi_restated(dm, 1e-12)[1]
    full, _ = _run(dm, expected=int(expected.max()))
    assert np.all(np.isfinite(full))
    assert np.array_equal(full, _run(dm, expected=int(expected.max()))[0])
    for i in (1, 37, 69):
        alone, _ = _run(dm[i - 1:i + 1], expected=int(expected[i]))
        assert np.array_equal(alone[1], full[i]), i
    wu, w = _units(full, oracle.tl_dynmap_pseudo(dm), dm, 1e-12)
    print(f"n = {n}, 70 maps: worst {wu:.2f} u (rel {w:.3e})")
    assert wu <= U_NUMPY


@pytest.mark.parametrize("n", [9, 36])
def test_one_map_is_handed_back(n):
    dm = tl_graded(np.random.default_rng(7100 + n), n, 1)
    rc, out, sweeps, msg = _call(dm, 1e-12)
    assert rc == 0, msg
    assert np.array_equal(out, dm)
    assert sweeps == 0          # no kernel ran


# ------------------------------------------------------------------------------------------ 8. error flags
def test_a_nan_is_reported_and_the_other_maps_are_delivered():
    dm = tl_graded(np.random.default_rng(8000), 16, 6)
    clean, _ = _run(dm)
    bad = dm.copy()
    bad[3, 5, 7] = np.nan
    rc, out, sweeps, msg = _call(bad, 1e-12)
    assert rc == PQD_ERR_NUMERIC
    assert "non-finite value (NaN/Inf) in the singular values of a map" in msg
    assert 1 <= sweeps <= 30
    for i in (0, 1, 2, 5):      # out[3] = bad[3] pinv(bad[2]) and out[4] = bad[4] pinv(bad[3]) see the NaN
        assert np.array_equal(out[i], clean[i]), i
    assert np.isnan(out[3]).any() and np.isnan(out[4]).any()
    with pytest.raises(_lib.NumericError):
        T.calc_tl_dynmap_pseudo(bad, np.round(np.arange(7) * 0.1, 6))
