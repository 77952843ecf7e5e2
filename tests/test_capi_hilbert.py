"""The dimension limits of the C-ABI after the Hilbert-space path (PQD_PATH_HILBERT): plans without a PT take dim <= 24
(dim > 6 with at most 8 jump operators), every entry point that builds N^2 x N^2 superoperators keeps dim <= 6. All of
these are refused before the context is touched, so no GPU is needed: the context handed in is a zeroed placeholder."""
import ctypes as C
import os
import re

import numpy as np

from pyaceqd_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _system(dim, n_lind=0):
    keep = {"H0": np.zeros((dim, dim), dtype=np.complex128)}
    s = _lib.pqd_system()
    s.dim, s.hbar, s.H0 = dim, 1.0, _lib.cptr(keep["H0"])
    if n_lind:
        keep["lr"] = np.full(n_lind, 0.1)
        keep["lo"] = np.zeros((n_lind, dim, dim), dtype=np.complex128)
        s.n_lind, s.lind_rates, s.lind_ops = n_lind, _lib.fptr(keep["lr"]), _lib.cptr(keep["lo"])
    return s, keep


def _plan_rc(dim, n_lind=0, n_out=1):
    """pqd_plan_create without a PT on a placeholder context: (status, message)"""
    L = _lib.lib()
    ctx = C.create_string_buffer(256)
    s, keep = _system(dim, n_lind)
    g = _lib.pqd_grid()
    g.ta, g.dt, g.n_steps, g.n_sub = 0.0, 0.1, 3, 1
    rho0 = np.zeros(dim * dim, dtype=np.complex128)
    ops = np.zeros(max(1, n_out) * dim * dim, dtype=np.complex128)
    b, e, o = np.zeros(1, np.int32), np.full(1, 3, np.int32), np.zeros(1, np.int64)
    tr = _lib.pqd_traj()
    tr.n_traj, tr.out_begin, tr.out_end, tr.out_offset = 1, _lib.iptr(b), _lib.iptr(e), _lib.lptr(o)
    h = C.c_void_p()
    rc = L.pqd_plan_create(C.cast(ctx, C.c_void_p), C.byref(s), C.byref(g), None, None, _lib.cptr(rho0), n_out,
                           _lib.cptr(ops), C.byref(tr), 4 * max(1, n_out), C.byref(h))
    return rc, L.pqd_last_error().decode()


def test_path_constant_matches_the_header():
    src = open(os.path.join(REPO, "include", "pqd.h")).read()
    assert int(re.search(r"#define PQD_PATH_HILBERT (\d+)", src).group(1)) == _lib.PQD_PATH_HILBERT == 5
    assert int(re.search(r"#define PQD_PATH_NOPT (\d+)", src).group(1)) == _lib.PQD_PATH_NOPT == 0


def test_plan_without_pt_accepts_dim_up_to_24():
    for dim in (25, 31):
        rc, msg = _plan_rc(dim)
        assert rc == _lib.PQD_ERR_UNSUPPORTED and "dim %d not in [2, 24]" % dim in msg
    rc, msg = _plan_rc(1)
    assert rc == _lib.PQD_ERR_UNSUPPORTED and "dim 1" in msg
    # dim 7, 8 and 24 pass the dimension check: the next refusal is the (deliberately bad) output count
    for dim in (7, 8, 24):
        rc, msg = _plan_rc(dim, n_out=0)
        assert rc == 1 and "n_out" in msg


def test_jump_operator_limit_above_dim_6():
    rc, msg = _plan_rc(8, n_lind=9)
    assert rc == _lib.PQD_ERR_UNSUPPORTED and "n_lind 9 not in [0, 8]" in msg
    rc, msg = _plan_rc(8, n_lind=8, n_out=0)       # 8 jump operators are inside the limit
    assert rc == 1 and "n_out" in msg
    rc, msg = _plan_rc(6, n_lind=9, n_out=0)       # dim <= 6 keeps its unlimited superoperator path
    assert rc == 1 and "n_out" in msg


def test_superoperator_entry_points_keep_dim_6():
    L = _lib.lib()
    ctx = C.cast(C.create_string_buffer(256), C.c_void_p)
    g = _lib.pqd_grid()
    g.ta, g.dt, g.n_steps, g.n_sub = 0.0, 0.1, 1, 1
    s, keep = _system(8)
    M = np.zeros(2 * 64 * 64, dtype=np.complex128)
    assert L.pqd_free_propagators(ctx, C.byref(s), C.byref(g), _lib.cptr(M)) == _lib.PQD_ERR_UNSUPPORTED
    assert b"dim 8 not in [2, 6]" in L.pqd_last_error()
    d = _lib.pqd_pt_desc()
    h = C.c_void_p()
    assert L.pqd_pt_create(ctx, 8, C.byref(d), C.byref(h)) == _lib.PQD_ERR_UNSUPPORTED
    assert b"dim 8" in L.pqd_last_error()
