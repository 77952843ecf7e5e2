"""Host side of the map-chain sweep by position (csrc/mapchain_wide.hip, dim 7..24). No GPU.

* pqd_mc_wide_schedule, the per-position schedule the host loop of pqd_calc_onetime_parallel runs above dim 6, against
  a brute-force restatement: for every position q the set of trajectories with p_i <= q < p_i + n_tau, the trunk flag
  q < max p_i and the set with p_i == q, from trunk ends found by the Fortran's own loop (propagate_tau.f90:144-151).
* the refusals of the C-ABI that return before the device is touched, on a zeroed placeholder context (as
  tests/test_capi_hilbert.py): pqd_calc_onetime_parallel and pqd_propagate_tau take dim 2..24, the block and
  phonon-block sweeps and pqd_map_tail keep dim <= 6 with their messages.
* the new symbols are declared in include/pqd.h and exported."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pyaceqd_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PQD_ERR_ARG, PQD_ERR_UNSUPPORTED = 1, 3   # include/pqd.h

TIME = np.round(np.arange(260) * 0.1, 6)
TS15 = np.array([0.0, 0.05, 0.7, 0.75, 0.8, 0.8, 1.2, 1.3, 1.31, 2.55, 4.0, 6.4, 7.9, 10.0, 10.85])
CASES = {
    "15 points": (TIME, TS15),
    "15 points, 60 maps": (TIME[:61], TS15[TS15 < 4.5]),
    "all equal": (TIME, np.full(17, 0.7)),
    "all at zero": (TIME, np.zeros(5)),
    "one by one": (TIME, TIME[3:36] + 0.05),
    "gaps": (TIME, np.array([0.0, 0.3, 5.0, 5.0, 11.1, 20.0])),
    "single": (TIME, np.array([1.25])),
}


def trunk_ends(time, ts):
    """p_i = j_i - 1 of the Fortran loop: j only ever grows"""
    pos, j = [], 1
    for t in ts:
        while j <= len(time) and time[j - 1] < t:
            j += 1
        pos.append(j - 1)
    return pos


def schedule(time, ts, n_tau):
    L = _lib.lib()
    time, ts = np.ascontiguousarray(time, dtype=np.float64), np.ascontiguousarray(ts, dtype=np.float64)
    pos = np.zeros(len(ts), dtype=np.int32)
    rows = C.c_int32(-1)
    a = (_lib.fptr(time), len(time), _lib.fptr(ts), len(ts), n_tau)
    assert L.pqd_mc_wide_schedule(*a, _lib.iptr(pos), C.byref(rows), None, 0) == 0, L.pqd_last_error()
    sched = np.full((rows.value, 5), -7, dtype=np.int32)
    assert L.pqd_mc_wide_schedule(*a, None, C.byref(rows), _lib.iptr(sched), rows.value) == 0, L.pqd_last_error()
    assert rows.value == len(sched)
    return pos, sched


@pytest.mark.parametrize("n_tau", [0, 1, 3, 12, 40])
@pytest.mark.parametrize("case", sorted(CASES))
def test_schedule_against_brute_force(case, n_tau):
    time, ts = CASES[case]
    pos, sched = schedule(time, ts, n_tau)
    ref = trunk_ends(time, ts)
    assert pos.tolist() == ref and all(a <= b for a, b in zip(ref, ref[1:]))
    n_t, p_max = len(ref), max(ref)
    Q = max(p + n_tau for p in ref)                       # Q_of (pqd_host.cpp)
    assert len(sched) == Q + 1
    covered = np.zeros((n_t, n_tau + 1), dtype=int)       # (i, k): column k + 1 of the result
    for q, (lo, hi, trunk, s_lo, s_hi) in enumerate(sched.tolist()):
        live = [i for i in range(n_t) if ref[i] <= q < ref[i] + n_tau]
        spawn = [i for i in range(n_t) if ref[i] == q]
        assert 0 <= lo <= hi <= n_t and 0 <= s_lo <= s_hi <= n_t
        assert list(range(lo, hi)) == live, (q, lo, hi, live)          # a contiguous range
        assert list(range(s_lo, s_hi)) == spawn, (q, s_lo, s_hi, spawn)
        assert trunk == (1 if q < p_max else 0)
        for i in spawn:
            covered[i, 0] += 1
        for i in live:
            covered[i, q - ref[i] + 1] += 1
    assert np.all(covered == 1)                           # every (i, k) exactly once
    assert sched[Q, 0] == sched[Q, 1] and sched[Q, 2] == 0  # the last row holds spawns only
    if "gaps" in case and n_tau in (1, 3, 12):
        # positions where the trunk runs on with no trajectory in flight
        assert any(lo == hi and trunk for lo, hi, trunk, _, _ in sched.tolist())


def test_schedule_refuses_bad_arguments():
    L = _lib.lib()
    time, ts = np.ascontiguousarray(TIME), np.ascontiguousarray(TS15)
    rows = C.c_int32(0)
    good = (_lib.fptr(time), len(time), _lib.fptr(ts), len(ts), 5)
    assert L.pqd_mc_wide_schedule(None, *good[1:], None, C.byref(rows), None, 0) == PQD_ERR_ARG
    assert L.pqd_mc_wide_schedule(*good, None, None, None, 0) == PQD_ERR_ARG
    assert L.pqd_mc_wide_schedule(*good[:3], 0, 5, None, C.byref(rows), None, 0) == PQD_ERR_ARG
    assert L.pqd_mc_wide_schedule(*good[:4], -1, None, C.byref(rows), None, 0) == PQD_ERR_ARG
    assert L.pqd_mc_wide_schedule(*good, None, C.byref(rows), None, 0) == 0
    short = np.zeros((rows.value - 1, 5), dtype=np.int32)
    assert L.pqd_mc_wide_schedule(*good, None, C.byref(rows), _lib.iptr(short), len(short)) == PQD_ERR_ARG
    assert b"rows" in L.pqd_last_error()


def _onetime(dim, n_t=3, null=None, name="pqd_calc_onetime_parallel"):
    """the sweep's C-ABI call on a placeholder context: (status, message)"""
    L = _lib.lib()
    ctx = C.cast(C.create_string_buffer(512), C.c_void_p)
    N2 = dim * dim
    n_tfull, n_tau = 6, 2
    a = {"dm": np.zeros(N2 * N2 * (n_tfull - 1), dtype=np.complex128), "rho": np.zeros(N2, dtype=np.complex128),
         "opA": np.zeros(N2, dtype=np.complex128), "opB": np.zeros(N2, dtype=np.complex128),
         "opC": np.zeros(N2, dtype=np.complex128), "time": 0.1 * np.arange(n_tfull), "ts": np.zeros(3),
         "out": np.zeros(3 * (n_tau + 1), dtype=np.complex128)}
    ptr = {k: (None if k == null else (_lib.fptr(v) if v.dtype == np.float64 else _lib.cptr(v))) for k, v in a.items()}
    if name == "pqd_calc_onetime_parallel":
        rc = L.pqd_calc_onetime_parallel(ctx, ptr["dm"], ptr["rho"], n_tau, n_t, n_tfull, dim, ptr["opA"], ptr["opB"],
                                         ptr["opC"], ptr["time"], ptr["ts"], ptr["out"])
    elif name == "pqd_calc_onetime_parallel_block":
        rc = L.pqd_calc_onetime_parallel_block(ctx, ptr["dm"], ptr["dm"], ptr["rho"], 2, 1, 2, n_t, n_tfull, dim,
                                               ptr["opA"], ptr["opB"], ptr["opC"], ptr["time"], ptr["ts"], ptr["out"])
    else:
        rc = L.pqd_calc_twotime_phonon_block(ctx, ptr["dm"], ptr["dm"], ptr["dm"], ptr["dm"], ptr["rho"], 2, 1, 2, n_t,
                                             n_tfull, 1, dim, ptr["opA"], ptr["opB"], ptr["opC"], ptr["time"], ptr["ts"],
                                             ptr["out"])
    return rc, L.pqd_last_error().decode()


def test_onetime_parallel_takes_dim_2_to_24():
    for dim in (25, 1, 0, 31):
        rc, msg = _onetime(dim)
        assert rc == PQD_ERR_UNSUPPORTED and "dim %d not in [2, 24]" % dim in msg
    # dim 8 and 24 pass the dimension check: the next refusals are the argument checks
    for dim in (8, 24):
        rc, msg = _onetime(dim, n_t=0)
        assert rc == PQD_ERR_ARG and "bad sizes" in msg
    for null in ("dm", "rho", "opA", "opB", "opC", "time", "ts", "out"):
        rc, msg = _onetime(8, null=null)
        assert rc == PQD_ERR_ARG and "NULL" in msg, null


def test_propagate_tau_takes_dim_2_to_24():
    L = _lib.lib()
    ctx = C.cast(C.create_string_buffer(512), C.c_void_p)
    for dim in (25, 1):
        N2 = max(1, dim * dim)
        dm, rho = np.zeros(4, dtype=np.complex128), np.zeros(N2, dtype=np.complex128)
        out = np.zeros(N2 * 2, dtype=np.complex128)
        rc = L.pqd_propagate_tau(ctx, _lib.cptr(dm), 1, _lib.cptr(rho), 1, dim, 0, _lib.cptr(out))
        assert rc == PQD_ERR_UNSUPPORTED and b"dim %d not in [2, 24]" % dim in L.pqd_last_error()
    # dim 8 passes the dimension check: the window past the maps is the next refusal
    dm, rho, out = np.zeros(4, dtype=np.complex128), np.zeros(64, dtype=np.complex128), np.zeros(192, dtype=np.complex128)
    rc = L.pqd_propagate_tau(ctx, _lib.cptr(dm), 1, _lib.cptr(rho), 2, 8, 0, _lib.cptr(out))
    assert rc == PQD_ERR_ARG and b"outside" in L.pqd_last_error()
    assert L.pqd_propagate_tau(ctx, None, 1, _lib.cptr(rho), 1, 8, 0, _lib.cptr(out)) == PQD_ERR_ARG


def test_the_other_sweeps_keep_dim_6():
    for name in ("pqd_calc_onetime_parallel_block", "pqd_calc_twotime_phonon_block"):
        for dim in (8, 7, 24):
            rc, msg = _onetime(dim, name=name)
            assert rc == PQD_ERR_UNSUPPORTED and "dim %d not in [2, 6]" % dim in msg, name
    L = _lib.lib()
    ctx = C.cast(C.create_string_buffer(512), C.c_void_p)
    z = np.zeros(64 * 64, dtype=np.complex128)
    assert L.pqd_map_tail(ctx, _lib.cptr(z), 64, _lib.cptr(z), 1, _lib.cptr(z), 1, _lib.cptr(z)) == PQD_ERR_UNSUPPORTED
    assert b"N2 64" in L.pqd_last_error()


def test_timing_entry_refuses_null():
    L = _lib.lib()
    ms, nl = C.c_double(), C.c_int32()
    assert L.pqd_mc_wide_timing(None, C.byref(ms), C.byref(nl)) == PQD_ERR_ARG
    ctx = C.cast(C.create_string_buffer(512), C.c_void_p)
    assert L.pqd_mc_wide_timing(ctx, None, C.byref(nl)) == PQD_ERR_ARG


def test_new_symbols_declared_and_exported():
    src = open(os.path.join(REPO, "include", "pqd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = C.CDLL(_lib.LIB_PATH)
    for name in ("pqd_mc_wide_schedule", "pqd_mc_wide_timing"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _lib.EXPORTED and hasattr(L, name)
    assert "not in [2, 24]" in src and "PQD_MC_WIDE" in src
