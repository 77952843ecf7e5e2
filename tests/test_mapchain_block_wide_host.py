"""Host side of the periodic map-chain sweep by position (pqd_calc_onetime_parallel_block_wide, dim 2..24). No GPU.

* pqd_mc_wide_block_schedule, the per-position schedule the host loop of that call walks, drives a numpy restatement of
  the loop (spawn, then one product per family) that is compared with oracle.calc_onetime_parallel_block, the C
  restatement of propagate_tau.f90:189-295. Bound 1e-12: double precision against double precision over at most about
  120 products of near-identity maps (observed 3e-15).
* the structure of every row: the ring range inside [0, n_ring), the straight range inside [n_ring, n_t), the two map
  cursors, the spawn ranges a partition of the trajectories.
* the refusals of the C-ABI that return before the device is touched, on a zeroed placeholder context (as
  tests/test_mapchain_wide_host.py), and the Python opt-in rule.
* the new symbols are declared in include/pqd.h and exported."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import oracle
from pyaceqd_amd import _lib
from pyaceqd_amd.two_time import propagate_tau_module as M
from tests import helpers as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PQD_ERR_ARG, PQD_ERR_UNSUPPORTED = 1, 3   # include/pqd.h
TOL = 1e-12
F = lambda maps: np.asfortranarray(np.asarray(maps).transpose(1, 2, 0))  # noqa: E731
# (n_tb, nx_tau, n_map): n_map below, at and above n_tb; a period of one map; no tau window; the sizes of
# tests/test_gpu_parity.py::test_mapchain_blocked_sweep_block_mode_vs_oracle
SHAPES = [(4, 3, 2), (4, 3, 4), (4, 3, 6), (1, 2, 1), (5, 0, 3), (12, 9, 7), (12, 9, 18)]


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def trunk_ends_for(n_tb, n_map):
    """0, inside the period, n_tb - 1 twice (two equal ends), n_tb, inside (n_tb, n_map], past n_map; never decreasing"""
    ends = {0, n_tb // 2, n_tb - 1, n_tb, n_tb + 1, max(n_tb, n_map) + 3}
    if n_map > n_tb:
        ends |= {n_tb + 1, n_map}
    ends = sorted(ends)
    at = ends.index(n_tb - 1)
    return ends[:at] + [n_tb - 1] + ends[at:]


def ts_of_ends(ends):
    """time_sparse whose trunk ends on a 0.1 grid are `ends` (p >= 1: between the grid points; 0: t = 0)"""
    return np.array([0.0 if p == 0 else 0.1 * p - 0.05 for p in ends])


def schedule(time, ts, n_tb, nx_tau, n_map):
    L = _lib.lib()
    time, ts = np.ascontiguousarray(time, dtype=np.float64), np.ascontiguousarray(ts, dtype=np.float64)
    pos = np.zeros(len(ts), dtype=np.int32)
    rows = C.c_int32(-1)
    a = (_lib.fptr(time), len(time), _lib.fptr(ts), len(ts), n_tb, nx_tau, n_map)
    assert L.pqd_mc_wide_block_schedule(*a, _lib.iptr(pos), C.byref(rows), None, 0) == 0, L.pqd_last_error()
    sched = np.full((rows.value, 9), -7, dtype=np.int32)
    assert L.pqd_mc_wide_block_schedule(*a, None, C.byref(rows), _lib.iptr(sched), rows.value) == 0, L.pqd_last_error()
    assert rows.value == len(sched)
    return pos, sched


def walk(sched, pos, dm_block, dm_s, rho, n_tau, dim, opa, opb, opc):
    """the host loop of the sweep in numpy, driven by the schedule's rows alone: spawns, then one product per family.
    dm_block (n_map, N2, N2), vectors in the Fortran's column-major view"""
    n_t, n_map, N2 = len(pos), len(dm_block), dim * dim
    mat = lambda v: v.reshape(dim, dim, order="F")  # noqa: E731
    the_map = lambda m: dm_block[m] if m < n_map else dm_s  # noqa: E731
    X = np.zeros((N2, n_t), dtype=complex)
    trunk_state = np.array(rho, dtype=complex)
    out = np.zeros((n_t, n_tau + 1), dtype=complex)
    for q, (r_lo, r_hi, r_map, s_lo, s_hi, trunk, s_map, sp_lo, sp_hi) in enumerate(sched.tolist()):
        for i in range(sp_lo, sp_hi):
            out[i, 0] = np.trace(opa @ opb @ opc @ mat(trunk_state))
            X[:, i] = (opc @ mat(trunk_state) @ opa).reshape(N2, order="F")
        if q == len(sched) - 1:
            assert r_lo == r_hi and s_lo == s_hi and not trunk   # the last row holds spawns only
            break
        for lo, hi, m in ((r_lo, r_hi, r_map), (s_lo, s_hi, s_map)):
            for i in range(lo, hi):
                assert pos[i] <= q < pos[i] + n_tau
                X[:, i] = the_map(m) @ X[:, i]
                out[i, q - pos[i] + 1] = np.trace(opb @ mat(X[:, i]))
        if trunk:
            trunk_state = the_map(s_map) @ trunk_state
    return out


def _case(dim, n_tb, nx_tau, n_map):
    rng = np.random.default_rng(100 * dim + 10 * n_tb + n_map)
    N2 = dim * dim
    mk = lambda: np.eye(N2) + 0.05 * (rng.normal(size=(N2, N2)) + 1j * rng.normal(size=(N2, N2))) / dim  # noqa: E731
    dm_block, dm_s = np.stack([mk() for _ in range(n_map)]), mk()
    ops = [rng.normal(size=(dim, dim)) + 1j * rng.normal(size=(dim, dim)) for _ in range(3)]
    ends = trunk_ends_for(n_tb, n_map)
    time = np.round(np.arange(max(ends) + 3) * 0.1, 6)
    return dm_block, dm_s, H.random_rho(dim).reshape(N2), ops, time, ts_of_ends(ends), ends


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "tb%d-x%d-map%d" % s)
@pytest.mark.parametrize("dim", [2, 3])
def test_schedule_walk_against_oracle(dim, shape):
    n_tb, nx_tau, n_map = shape
    dm_block, dm_s, rho, ops, time, ts, ends = _case(dim, *shape)
    pos, sched = schedule(time, ts, n_tb, nx_tau, n_map)
    assert pos.tolist() == ends
    assert {0, n_tb - 1, n_tb} <= set(ends) and ends.count(n_tb - 1) == 2 and max(ends) > n_map
    assert n_map <= n_tb or any(n_tb < p <= n_map for p in ends)
    got = walk(sched, pos, dm_block, dm_s, rho, n_tb * nx_tau, dim, *ops)
    ref = oracle.calc_onetime_parallel_block(F(dm_block), np.asfortranarray(dm_s), rho, n_tb, nx_tau, dim, *ops, time, ts)
    assert got.shape == ref.shape == (len(ts), n_tb * nx_tau + 1)
    e = rel(got, ref)
    print(f"dim {dim} (n_tb, nx_tau, n_map) {shape}: schedule walk vs oracle {e:.3e}")
    assert e < TOL


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "tb%d-x%d-map%d" % s)
def test_schedule_rows(shape):
    n_tb, nx_tau, n_map = shape
    n_tau = n_tb * nx_tau
    ends = trunk_ends_for(n_tb, n_map)
    time = np.round(np.arange(max(ends) + 3) * 0.1, 6)
    pos, sched = schedule(time, ts_of_ends(ends), n_tb, nx_tau, n_map)
    n_t, n_ring = len(ends), sum(p < n_tb for p in ends)
    assert len(sched) == max(ends) + n_tau + 1
    spawned = []
    two = 0
    for q, (r_lo, r_hi, r_map, s_lo, s_hi, trunk, s_map, sp_lo, sp_hi) in enumerate(sched.tolist()):
        live = [i for i in range(n_t) if ends[i] <= q < ends[i] + n_tau]
        assert 0 <= r_lo <= r_hi <= n_ring <= s_lo <= s_hi <= n_t, (q, sched[q])
        assert list(range(r_lo, r_hi)) + list(range(s_lo, s_hi)) == live, (q, sched[q], live)
        assert r_map == min(q % n_tb, n_map) and s_map == min(q, n_map)
        assert trunk == (1 if q < max(ends) else 0)
        assert list(range(sp_lo, sp_hi)) == [i for i in range(n_t) if ends[i] == q]
        spawned += list(range(sp_lo, sp_hi))
        two += r_hi > r_lo and (s_hi > s_lo or trunk) and r_map != s_map
    assert spawned == list(range(n_t))                    # the spawn ranges partition [0, n_t)
    if nx_tau > 0 and n_tb > 1:
        assert two > 0                                    # both cursors at one position, on different maps


def _call(dim, n_t=3, null=None, n_tb=2, nx_tau=1, n_map=2, name="pqd_calc_onetime_parallel_block_wide"):
    """the C-ABI call on a placeholder context: (status, message)"""
    L = _lib.lib()
    ctx = C.cast(C.create_string_buffer(512), C.c_void_p)
    N2 = max(1, dim * dim)
    a = {"dm": np.zeros(N2 * N2 * 2, dtype=np.complex128), "dm_s": np.zeros(N2 * N2, dtype=np.complex128),
         "rho": np.zeros(N2, dtype=np.complex128), "opA": np.zeros(N2, dtype=np.complex128),
         "opB": np.zeros(N2, dtype=np.complex128), "opC": np.zeros(N2, dtype=np.complex128),
         "time": 0.1 * np.arange(6), "ts": np.zeros(3), "out": np.zeros(3 * 3, dtype=np.complex128)}
    ptr = {k: (None if k == null else (_lib.fptr(v) if v.dtype == np.float64 else _lib.cptr(v))) for k, v in a.items()}
    rc = getattr(L, name)(ctx, ptr["dm"], ptr["dm_s"], ptr["rho"], n_tb, nx_tau, n_map, n_t, 6, dim, ptr["opA"],
                          ptr["opB"], ptr["opC"], ptr["time"], ptr["ts"], ptr["out"])
    return rc, L.pqd_last_error().decode()


def test_block_wide_takes_dim_2_to_24():
    for dim in (25, 1, 0):
        rc, msg = _call(dim)
        assert rc == PQD_ERR_UNSUPPORTED and "dim %d not in [2, 24]" % dim in msg
    # dim 8 and 24 pass the dimension check: the next refusals are the argument checks
    for dim in (8, 24):
        rc, msg = _call(dim, n_t=0)
        assert rc == PQD_ERR_ARG and "bad sizes" in msg
    for null in ("dm", "dm_s", "rho", "opA", "opB", "opC", "time", "ts", "out"):
        rc, msg = _call(8, null=null)
        assert rc == PQD_ERR_ARG and "NULL" in msg, null
    for kw in ({"n_tb": 0}, {"n_map": 0}, {"nx_tau": -1}):
        rc, msg = _call(8, **kw)
        assert rc == PQD_ERR_ARG and "bad block sizes" in msg, kw
    # the existing entry keeps its limit and its words
    rc, msg = _call(8, name="pqd_calc_onetime_parallel_block")
    assert rc == PQD_ERR_UNSUPPORTED and "dim 8 not in [2, 6]" in msg


def test_schedule_refuses_bad_arguments():
    L = _lib.lib()
    time, ts = np.ascontiguousarray(0.1 * np.arange(40)), np.array([0.0, 0.35, 0.35, 0.95])   # ends 0, 4, 4, 10
    rows = C.c_int32(0)
    good = (_lib.fptr(time), len(time), _lib.fptr(ts), len(ts), 4, 3, 2)
    call = L.pqd_mc_wide_block_schedule
    assert call(None, *good[1:], None, C.byref(rows), None, 0) == PQD_ERR_ARG
    assert call(*good[:2], None, *good[3:], None, C.byref(rows), None, 0) == PQD_ERR_ARG
    assert call(*good, None, None, None, 0) == PQD_ERR_ARG
    assert call(*good[:3], 0, *good[4:], None, C.byref(rows), None, 0) == PQD_ERR_ARG
    for at, bad in ((4, 0), (5, -1), (6, 0)):   # n_tb, nx_tau, n_map
        a = list(good)
        a[at] = bad
        assert call(*a, None, C.byref(rows), None, 0) == PQD_ERR_ARG
        assert b"bad block sizes" in L.pqd_last_error()
    assert call(*good, None, C.byref(rows), None, 0) == 0 and rows.value == 10 + 12 + 1
    short = np.zeros((rows.value - 1, 9), dtype=np.int32)
    assert call(*good, None, C.byref(rows), _lib.iptr(short), len(short)) == PQD_ERR_ARG
    assert b"rows" in L.pqd_last_error()


def test_python_opt_in(monkeypatch):
    """without the opt-in calc_onetime_parallel_block at dim 8 keeps the [2, 6] refusal; with it the call goes to the
    wide entry. _lib.context() is replaced by a placeholder, which neither refusal reads (both return before the device
    is touched; the wide entry is sent n_t = 0 for that)."""
    import threading

    class Ctx:
        handle = C.cast(C.create_string_buffer(512), C.c_void_p)
        lock = threading.RLock()
    monkeypatch.setattr(M, "_ctx", lambda: Ctx)
    z = lambda *s: np.zeros(s, dtype=complex, order="F")  # noqa: E731
    t, ts = np.array([0.0, 0.1]), np.array([0.0])
    a = (z(64, 64, 2), z(64, 64), z(64), 2, 1, 8, z(8, 8), z(8, 8), z(8, 8), t, ts)
    monkeypatch.delenv("PQD_WIDE_MAPS", raising=False)
    for kw in ({}, {"wide": None}, {"wide": False}):
        with pytest.raises(_lib.PQDError, match=r"dim 8 not in \[2, 6\]") as ei:
            M.calc_onetime_parallel_block(*a, **kw)
        assert ei.value.code == PQD_ERR_UNSUPPORTED
    monkeypatch.setenv("PQD_WIDE_MAPS", "1")
    with pytest.raises(_lib.PQDError, match=r"dim 8 not in \[2, 6\]"):
        M.calc_onetime_parallel_block(*a, wide=False)
    # opted in: past the dimension check, refused for the sizes (n_t = 0)
    for kw in ({"wide": None}, {"wide": True}):
        with pytest.raises(ValueError, match="bad sizes"):
            M.calc_onetime_parallel_block(*a, n_t=0, **kw)
    monkeypatch.delenv("PQD_WIDE_MAPS")
    with pytest.raises(ValueError, match="bad sizes"):
        M.calc_onetime_parallel_block_wide(*a, n_t=0)
    with pytest.raises(_lib.PQDError, match=r"dim 25 not in \[2, 24\]"):
        M.calc_onetime_parallel_block_wide(z(625, 625, 1), z(625, 625), z(625), 2, 1, 25, *[z(25, 25)] * 3, t, ts)
    # at dim <= 6 the keyword changes nothing: the same entry, here its own size refusal
    for kw in ({}, {"wide": True}):
        with pytest.raises(ValueError, match="bad sizes"):
            M.calc_onetime_parallel_block(z(4, 4, 2), z(4, 4), z(4), 2, 1, 2, z(2, 2), z(2, 2), z(2, 2), t, ts, n_t=0, **kw)


def test_new_symbols_declared_and_exported():
    src = open(os.path.join(REPO, "include", "pqd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = C.CDLL(_lib.LIB_PATH)
    for name in ("pqd_calc_onetime_parallel_block_wide", "pqd_mc_wide_block_schedule"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _lib.EXPORTED and hasattr(L, name)
